// Static-background removal on the device: the ensemble minimum of a recording, per pixel, and the saturating
// subtraction f -> max(f, bg) - bg.  Integer in, integer out: the frames that leave here are uint8 frames like any
// other, so every correlation kernel and precision (the exact first pass included) applies to them unchanged.
//
// Both kernels stream: a lane owns 16 consecutive bytes of the image and moves them with 16-byte loads and stores.
// Where the frames are not 16-byte aligned (pixels % 16 != 0, or an offset view) the same lanes fall back to byte
// accesses; the last lane of an image covers the pixels % 16 tail either way.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "piv_kernels.h"

namespace tpiv {

namespace {

typedef uint8_t u8x16 __attribute__((ext_vector_type(16)));

constexpr int kThreads = 256;
constexpr int kUnroll = 4;         // frames whose loads a lane has in flight at once (frame_min)

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// acc[p] = min(acc[p], frames[f][p]) over f < n.  No atomics: each lane owns its 16 bytes of acc.
template <bool kVec>
__global__ __launch_bounds__(kThreads) void frame_min_kernel(const uint8_t* __restrict__ frames, int n, long long pixels,
                                                              uint8_t* __restrict__ acc) {
    const long long p0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * 16;
    if (p0 >= pixels) return;
    if constexpr (kVec) {
        const u8x16* __restrict__ src = reinterpret_cast<const u8x16*>(frames + p0);
        const long long step = pixels / 16;
        u8x16 m = *reinterpret_cast<const u8x16*>(acc + p0);
        int f = 0;
        for (; f + kUnroll <= n; f += kUnroll) {
            u8x16 v[kUnroll];
#pragma unroll
            for (int k = 0; k < kUnroll; ++k) v[k] = src[(long long)(f + k) * step];
#pragma unroll
            for (int k = 0; k < kUnroll; ++k) m = __builtin_elementwise_min(m, v[k]);
        }
        for (; f < n; ++f) m = __builtin_elementwise_min(m, src[(long long)f * step]);
        *reinterpret_cast<u8x16*>(acc + p0) = m;
    } else {
        const int cnt = pixels - p0 < 16 ? (int)(pixels - p0) : 16;
        uint8_t m[16];
        for (int k = 0; k < cnt; ++k) m[k] = acc[p0 + k];
        for (int f = 0; f < n; ++f) {
            const uint8_t* __restrict__ src = frames + (long long)f * pixels + p0;
            for (int k = 0; k < cnt; ++k) m[k] = src[k] < m[k] ? src[k] : m[k];
        }
        for (int k = 0; k < cnt; ++k) acc[p0 + k] = m[k];
    }
}

// out[f][p] = max(frames[f][p], bg[p]) - bg[p].  out may be frames itself (each byte is read before it is written, by
// the same lane), so neither carries __restrict__; a partial overlap is not supported.  A lane takes two frames per
// step, both loads ahead of both stores, so that two 16-byte loads per lane are in flight.
template <bool kVec>
__global__ __launch_bounds__(kThreads) void subtract_background_kernel(const uint8_t* frames, int n, long long pixels,
                                                                        const uint8_t* __restrict__ bg, uint8_t* out) {
    const long long p0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * 16;
    if (p0 >= pixels) return;
    if constexpr (kVec) {
        const u8x16 b = *reinterpret_cast<const u8x16*>(bg + p0);
        int f = 2 * blockIdx.y;
        for (; f + 1 < n; f += 2 * gridDim.y) {
            const long long o0 = (long long)f * pixels + p0, o1 = o0 + pixels;
            const u8x16 v0 = *reinterpret_cast<const u8x16*>(frames + o0);
            const u8x16 v1 = *reinterpret_cast<const u8x16*>(frames + o1);
            *reinterpret_cast<u8x16*>(out + o0) = __builtin_elementwise_sub_sat(v0, b);
            *reinterpret_cast<u8x16*>(out + o1) = __builtin_elementwise_sub_sat(v1, b);
        }
        if (f < n) {                                           // odd n: the last frame alone
            const long long o = (long long)f * pixels + p0;
            *reinterpret_cast<u8x16*>(out + o) = __builtin_elementwise_sub_sat(*reinterpret_cast<const u8x16*>(frames + o), b);
        }
    } else {
        const int cnt = pixels - p0 < 16 ? (int)(pixels - p0) : 16;
        uint8_t b[16];
        for (int k = 0; k < cnt; ++k) b[k] = bg[p0 + k];
        for (int f = blockIdx.y; f < n; f += gridDim.y) {
            const long long o = (long long)f * pixels + p0;
            for (int k = 0; k < cnt; ++k) {
                const uint8_t v = frames[o + k];
                out[o + k] = v > b[k] ? (uint8_t)(v - b[k]) : (uint8_t)0;
            }
        }
    }
}

}  // namespace

hipError_t launch_frame_min(const uint8_t* frames, int n, long long pixels, uint8_t* acc, hipStream_t stream) {
    if (n <= 0 || pixels <= 0) return hipSuccess;
    const long long lanes = (pixels + 15) / 16;
    const long long blocks = (lanes + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const bool vec = pixels % 16 == 0 && aligned16(frames) && aligned16(acc);
    if (vec)
        hipLaunchKernelGGL(frame_min_kernel<true>, dim3((unsigned)blocks), dim3(kThreads), 0, stream, frames, n, pixels, acc);
    else
        hipLaunchKernelGGL(frame_min_kernel<false>, dim3((unsigned)blocks), dim3(kThreads), 0, stream, frames, n, pixels, acc);
    return hipGetLastError();
}

hipError_t launch_subtract_background(const uint8_t* frames, int n, long long pixels, const uint8_t* bg, uint8_t* out,
                                      hipStream_t stream) {
    if (n <= 0 || pixels <= 0) return hipSuccess;
    const long long lanes = (pixels + 15) / 16;
    const long long blocks = (lanes + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const bool vec = pixels % 16 == 0 && aligned16(frames) && aligned16(bg) && aligned16(out);
    const int rows = vec ? (n + 1) / 2 : n;                 // frame steps (the vector form takes two frames per step)
    const dim3 grid((unsigned)blocks, rows < 65535 ? rows : 65535);
    if (vec)
        hipLaunchKernelGGL(subtract_background_kernel<true>, grid, dim3(kThreads), 0, stream, frames, n, pixels, bg, out);
    else
        hipLaunchKernelGGL(subtract_background_kernel<false>, grid, dim3(kThreads), 0, stream, frames, n, pixels, bg, out);
    return hipGetLastError();
}

}  // namespace tpiv
