// Geometric rectification on the device: out[f][r][c] = the frame sampled at the source position the map holds for output
// pixel (r, c), the same map for every frame of a launch.  Integer in, integer out, integer in between: the map is signed
// Q8 (q = floor(s * 256 + 0.5), int32 [H, W, 2], x first), the bilinear weights are Q8 and the Catmull-Rom weights a Q10
// table, so every implementation of the lines in include/torchpiv_hip.h gives the same bytes -- which a float kernel built
// with -ffp-contract=fast-honor-pragmas could not promise.
//
// A lane owns four horizontally adjacent output pixels: it reads their eight map words once (two 16-byte loads) and then
// walks the frames of its chunk, gathering the taps of each and writing one 4-byte store per frame, so the map is read
// once per launch and not once per frame.  Where a row is no multiple of four pixels long, or the map or the output is
// not aligned for those accesses, the same lanes read the map word by word and write bytes; the last lane of a row then
// covers its W % 4 tail.  The grid's second dimension splits the frames into chunks of kFrameChunk, so that a launch of
// few frames still fills the device.  Every tap index is clamped to the frame unconditionally: no address is ever formed
// from an unclamped map entry, whatever the map holds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "piv_kernels.h"

namespace tpiv {

namespace {

constexpr int kThreads = 256;
constexpr int kFrameChunk = DEWARP_FRAME_CHUNK;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the four Q10 weights of fraction f, one 8-byte LDS read
__device__ __forceinline__ void weights(const int16_t* tab, int f, int w[4]) {
    const uint2 t = *reinterpret_cast<const uint2*>(tab + 4 * f);
    w[0] = (int)(int16_t)(t.x & 0xffffu);
    w[1] = (int)t.x >> 16;
    w[2] = (int)(int16_t)(t.y & 0xffffu);
    w[3] = (int)t.y >> 16;
}

// One output pixel.  Outside (qx < 0, qy < 0, qx > (W - 1) << 8 or qy > (H - 1) << 8; the host stores such entries as
// (-1, -1)): fill.  Linear: (sum wy wx p + 32768) >> 16 with the weights (256 - f, f) on the taps ix, ix + 1.  Cubic:
// clamp((sum Ty[a] Tx[b] p + (1 << 19)) >> 20, 0, 255) on the taps ix - 1 .. ix + 2; |sum| <= 255 * 1280^2 < 2^31.  H * W
// < 2^31 (the C entry checks it), so an offset inside a frame is an int.
template <bool kCubic>
__device__ __forceinline__ uint32_t sample(const uint8_t* __restrict__ src, int H, int W, int qx, int qy, uint32_t fill,
                                           const int16_t* tab) {
    const bool outside = qx < 0 || qy < 0 || qx > ((W - 1) << 8) || qy > ((H - 1) << 8);
    const int ix = qx >> 8, iy = qy >> 8, fx = qx & 255, fy = qy & 255;
    int v;
    if constexpr (kCubic) {
        int tx[4], ty[4], xo[4];
        weights(tab, fx, tx);
        weights(tab, fy, ty);
#pragma unroll
        for (int b = 0; b < 4; ++b) xo[b] = clampi(ix - 1 + b, 0, W - 1);
        int acc = 1 << 19;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const uint8_t* __restrict__ row = src + clampi(iy - 1 + a, 0, H - 1) * W;
            int s = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) s += tx[b] * (int)row[xo[b]];
            acc += ty[a] * s;
        }
        v = clampi(acc >> 20, 0, 255);
    } else {
        const int x0 = clampi(ix, 0, W - 1), x1 = clampi(ix + 1, 0, W - 1);
        const uint8_t* __restrict__ r0 = src + clampi(iy, 0, H - 1) * W;
        const uint8_t* __restrict__ r1 = src + clampi(iy + 1, 0, H - 1) * W;
        const int top = (256 - fx) * (int)r0[x0] + fx * (int)r0[x1];
        const int bot = (256 - fx) * (int)r1[x0] + fx * (int)r1[x1];
        v = ((256 - fy) * top + fy * bot + 32768) >> 16;
    }
    return outside ? fill : (uint32_t)v;
}

// frames: the source, frame f at element offset off[f] (off == nullptr: f * pixels); out [n, H, W].  kVec: W % 4 == 0, the
// map 16-byte and out 4-byte aligned (decided by the launcher, uniform over the grid).
template <bool kVec, bool kCubic>
__global__ __launch_bounds__(kThreads) void dewarp_kernel(const uint8_t* __restrict__ frames,
                                                           const long long* __restrict__ off, int n, int H, int W,
                                                           const int32_t* __restrict__ map,
                                                           const int16_t* __restrict__ table, uint32_t fill,
                                                           uint8_t* __restrict__ out) {
    __shared__ __attribute__((aligned(8))) int16_t tab[kCubic ? 1024 : 4];
    if constexpr (kCubic) {
        for (int i = threadIdx.x; i < 1024; i += kThreads) tab[i] = table[i];
        __syncthreads();
    }
    const int per_row = (W + 3) / 4;                                    // lanes of a row
    const long long lane = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (lane >= (long long)H * per_row) return;
    const int r = (int)(lane / per_row), c0 = (int)(lane % per_row) * 4;
    const long long pixels = (long long)H * W, p0 = (long long)r * W + c0;
    const int cnt = kVec ? 4 : (W - c0 < 4 ? W - c0 : 4);
    int qx[4], qy[4];
    if constexpr (kVec) {
        const int4 m0 = *reinterpret_cast<const int4*>(map + 2 * p0);
        const int4 m1 = *reinterpret_cast<const int4*>(map + 2 * p0 + 4);
        qx[0] = m0.x, qy[0] = m0.y, qx[1] = m0.z, qy[1] = m0.w;
        qx[2] = m1.x, qy[2] = m1.y, qx[3] = m1.z, qy[3] = m1.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            qx[k] = k < cnt ? map[2 * (p0 + k)] : -1;
            qy[k] = k < cnt ? map[2 * (p0 + k) + 1] : -1;
        }
    }
    for (int f0 = blockIdx.y * kFrameChunk; f0 < n; f0 += gridDim.y * kFrameChunk) {
        const int f1 = f0 + kFrameChunk < n ? f0 + kFrameChunk : n;
#pragma unroll(kCubic ? 1 : 2)
        for (int f = f0; f < f1; ++f) {
            const uint8_t* __restrict__ src = frames + (off ? off[f] : (long long)f * pixels);
            uint8_t* __restrict__ dst = out + (long long)f * pixels + p0;
            uint32_t px[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) px[k] = sample<kCubic>(src, H, W, qx[k], qy[k], fill, tab);
            if constexpr (kVec) {
                *reinterpret_cast<uint32_t*>(dst) = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < cnt) dst[k] = (uint8_t)px[k];
            }
        }
    }
}

}  // namespace

hipError_t launch_dewarp(const uint8_t* frames, const long long* src_off, int n, int H, int W, const int32_t* map,
                         const int16_t* table, int interp, int fill, uint8_t* out, hipStream_t stream) {
    if (n <= 0 || H <= 0 || W <= 0) return hipSuccess;
    const long long lanes = (long long)H * ((W + 3) / 4);
    const long long blocks = (lanes + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const int chunks = (n + kFrameChunk - 1) / kFrameChunk;
    const dim3 grid((unsigned)blocks, chunks < 65535 ? chunks : 65535);
    const bool vec = W % 4 == 0 && ((uintptr_t)map & 15u) == 0 && ((uintptr_t)out & 3u) == 0;
    const bool cubic = interp == DEWARP_CUBIC;
    auto* kernel = vec ? (cubic ? dewarp_kernel<true, true> : dewarp_kernel<true, false>)
                       : (cubic ? dewarp_kernel<false, true> : dewarp_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, stream, frames, src_off, n, H, W, map, table, (uint32_t)fill, out);
    return hipGetLastError();
}

}  // namespace tpiv
