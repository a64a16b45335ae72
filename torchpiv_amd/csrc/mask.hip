// Geometric masks on the device: the pixel step (out = mask ? 0 : frame), the count of masked pixels per interrogation
// window, and the step that writes excluded cells into the fields of a pass.  Integer in, integer out for the frames: what
// leaves apply_mask_kernel is a uint8 frame like any other, so every correlation kernel and precision applies unchanged.
//
// apply_mask_kernel streams like background.hip's subtract_background_kernel: a lane owns 16 consecutive bytes of the
// image and moves them with 16-byte loads and stores, two frames per step; where the frames are not 16-byte aligned
// (pixels % 16 != 0, or an offset view) the same lanes fall back to byte accesses; the last lane of an image covers the
// pixels % 16 tail either way.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "piv_kernels.h"

namespace tpiv {

namespace {

typedef uint8_t u8x16 __attribute__((ext_vector_type(16)));

constexpr int kThreads = 256;
constexpr int kWave = 64;

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// out[f][p] = mask[p] != 0 ? 0 : frames[f][p], as frames & keep with keep = 0x00 on masked pixels and 0xFF elsewhere.
// out may be frames itself (each byte is read before it is written, by the same lane), so neither carries __restrict__;
// a partial overlap is not supported.  Both loads of a step go ahead of both stores.
template <bool kVec>
__global__ __launch_bounds__(kThreads) void apply_mask_kernel(const uint8_t* frames, int n, long long pixels,
                                                               const uint8_t* __restrict__ mask, uint8_t* out) {
    const long long p0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * 16;
    if (p0 >= pixels) return;
    if constexpr (kVec) {
        const u8x16 m = *reinterpret_cast<const u8x16*>(mask + p0);
        const u8x16 keep = __builtin_convertvector(m == (u8x16)(0), u8x16);      // (a true lane of the comparison is -1)
        int f = 2 * blockIdx.y;
        for (; f + 1 < n; f += 2 * gridDim.y) {
            const long long o0 = (long long)f * pixels + p0, o1 = o0 + pixels;
            const u8x16 v0 = *reinterpret_cast<const u8x16*>(frames + o0);
            const u8x16 v1 = *reinterpret_cast<const u8x16*>(frames + o1);
            *reinterpret_cast<u8x16*>(out + o0) = v0 & keep;
            *reinterpret_cast<u8x16*>(out + o1) = v1 & keep;
        }
        if (f < n) {                                           // odd n: the last frame alone
            const long long o = (long long)f * pixels + p0;
            *reinterpret_cast<u8x16*>(out + o) = *reinterpret_cast<const u8x16*>(frames + o) & keep;
        }
    } else {
        const int cnt = pixels - p0 < 16 ? (int)(pixels - p0) : 16;
        uint8_t keep[16];
        for (int k = 0; k < cnt; ++k) keep[k] = mask[p0 + k] ? (uint8_t)0 : (uint8_t)0xFF;
        for (int f = blockIdx.y; f < n; f += gridDim.y) {
            const long long o = (long long)f * pixels + p0;
            for (int k = 0; k < cnt; ++k) out[o + k] = frames[o + k] & keep[k];
        }
    }
}

// count[i * n_cols + j] = masked pixels of window (i, j): rows i (ws - ov) ... + ws, columns j (ws - ov) ... + ws.  A
// wavefront per window, its lanes over the window's ws * ws bytes, one shuffle reduction, no atomics and no LDS: any ws and
// any overlap below it take the same path.  grid (optional): count > limit.
__global__ __launch_bounds__(kThreads) void mask_coverage_kernel(const uint8_t* __restrict__ mask, int H, int W, int ws,
                                                                  int step, int n_rows, int n_cols,
                                                                  int32_t* __restrict__ count, uint8_t* __restrict__ grid,
                                                                  int limit) {
    const int lane = threadIdx.x % kWave;
    const long long w = (long long)blockIdx.x * (kThreads / kWave) + threadIdx.x / kWave;      // wave-uniform
    if (w >= (long long)n_rows * n_cols) return;
    const int y0 = (int)(w / n_cols) * step, x0 = (int)(w % n_cols) * step;
    int c = 0;
    for (int k = lane; k < ws * ws; k += kWave) {
        const int y = y0 + k / ws, x = x0 + k % ws;
        if (y < H && x < W) c += mask[(long long)y * W + x] != 0;          // (a window of the grid never leaves the frame)
    }
    for (int d = kWave / 2; d > 0; d /= 2) c += __shfl_down(c, d, kWave);
    if (lane == 0) {
        if (count) count[w] = c;
        if (grid) grid[w] = c > limit;
    }
}

// Excluded cells of every pair: u = v = +0.0, invalid = value, status = 2 (invalid on input, not flagged).
__global__ __launch_bounds__(kThreads) void mask_fields_kernel(double* __restrict__ u, double* __restrict__ v,
                                                                uint8_t* __restrict__ invalid, uint8_t* __restrict__ status,
                                                                const uint8_t* __restrict__ grid, long long total,
                                                                int cells, uint8_t value) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total || !grid[i % cells]) return;
    u[i] = 0.0;
    v[i] = 0.0;
    invalid[i] = value;
    if (status) status[i] = 2;
}

// ---- the per-pair forms: mask f for frame f, grid f for pair f (tpiv_apply_mask_pairs, tpiv_mask_coverage_pairs,
// tpiv_mask_fields_pairs).  The kernels above stay as they are.

// out[i] = masks[i] != 0 ? 0 : frames[i] over the n * pixels bytes as one array: a lane owns 16 consecutive bytes.  out may be
// frames itself (each byte is read before it is written, by the same lane).
template <bool kVec>
__global__ __launch_bounds__(kThreads) void apply_mask_pairs_kernel(const uint8_t* frames, long long total,
                                                                     const uint8_t* __restrict__ masks, uint8_t* out) {
    const long long p0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * 16;
    if (p0 >= total) return;
    if constexpr (kVec) {
        const u8x16 m = *reinterpret_cast<const u8x16*>(masks + p0);
        const u8x16 keep = __builtin_convertvector(m == (u8x16)(0), u8x16);
        *reinterpret_cast<u8x16*>(out + p0) = *reinterpret_cast<const u8x16*>(frames + p0) & keep;
    } else {
        const int cnt = total - p0 < 16 ? (int)(total - p0) : 16;
        for (int k = 0; k < cnt; ++k) out[p0 + k] = masks[p0 + k] ? (uint8_t)0 : frames[p0 + k];
    }
}

// mask_coverage_kernel with the pair along the grid's second dimension: count [n, n_rows, n_cols] (optional), grid likewise.
// A plan runs it for every batch, so where the windows start and end on 16-byte boundaries of 16-byte aligned rows (kVec:
// ws, ws - ov and W multiples of 16, the masks aligned) a lane takes 16 mask bytes per load; the same counts either way.
template <bool kVec>
__global__ __launch_bounds__(kThreads) void mask_coverage_pairs_kernel(const uint8_t* __restrict__ masks, int n, int H, int W,
                                                                        int ws, int step, int n_rows, int n_cols,
                                                                        int32_t* __restrict__ count,
                                                                        uint8_t* __restrict__ grid, int limit) {
    const int lane = threadIdx.x % kWave;
    const long long w = (long long)blockIdx.x * (kThreads / kWave) + threadIdx.x / kWave;      // wave-uniform
    const long long cells = (long long)n_rows * n_cols;
    if (w >= cells) return;
    const int y0 = (int)(w / n_cols) * step, x0 = (int)(w % n_cols) * step;
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const uint8_t* __restrict__ mask = masks + (long long)f * H * W;
        int c = 0;
        if constexpr (kVec) {
            const int per_row = ws >> 4;
            for (int k = lane; k < ws * per_row; k += kWave) {
                const int y = y0 + k / per_row, x = x0 + 16 * (k % per_row);
                if (y < H && x < W) {                                   // (x and W are multiples of 16: the chunk is inside)
                    const u8x16 v = *reinterpret_cast<const u8x16*>(mask + (long long)y * W + x);
                    c += __builtin_reduce_add(__builtin_convertvector(v != (u8x16)(0), u8x16) & (u8x16)(1));
                }
            }
        } else {
            for (int k = lane; k < ws * ws; k += kWave) {
                const int y = y0 + k / ws, x = x0 + k % ws;
                if (y < H && x < W) c += mask[(long long)y * W + x] != 0;
            }
        }
        for (int d = kWave / 2; d > 0; d /= 2) c += __shfl_down(c, d, kWave);
        if (lane == 0) {
            if (count) count[f * cells + w] = c;
            if (grid) grid[f * cells + w] = c > limit;
        }
    }
}

// mask_fields_kernel with grids [batch, n_rows, n_cols]: cell i of the fields reads byte i
__global__ __launch_bounds__(kThreads) void mask_fields_pairs_kernel(double* __restrict__ u, double* __restrict__ v,
                                                                      uint8_t* __restrict__ invalid,
                                                                      uint8_t* __restrict__ status,
                                                                      const uint8_t* __restrict__ grids, long long total,
                                                                      uint8_t value) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total || !grids[i]) return;
    u[i] = 0.0;
    v[i] = 0.0;
    invalid[i] = value;
    if (status) status[i] = 2;
}

}  // namespace

hipError_t launch_apply_mask_pairs(const uint8_t* frames, int n, long long pixels, const uint8_t* masks, uint8_t* out,
                                   hipStream_t stream) {
    if (n <= 0 || pixels <= 0) return hipSuccess;
    const long long total = (long long)n * pixels;
    const long long blocks = ((total + 15) / 16 + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    if (total % 16 == 0 && aligned16(frames) && aligned16(masks) && aligned16(out))
        hipLaunchKernelGGL(apply_mask_pairs_kernel<true>, dim3((unsigned)blocks), dim3(kThreads), 0, stream, frames, total,
                           masks, out);
    else
        hipLaunchKernelGGL(apply_mask_pairs_kernel<false>, dim3((unsigned)blocks), dim3(kThreads), 0, stream, frames, total,
                           masks, out);
    return hipGetLastError();
}

hipError_t launch_mask_coverage_pairs(const uint8_t* masks, int n, int H, int W, int ws, int ov, int n_rows, int n_cols,
                                      int32_t* count, uint8_t* grid, int limit, hipStream_t stream) {
    const long long windows = (long long)n_rows * n_cols;
    if (windows <= 0 || n <= 0) return hipSuccess;
    const long long blocks = (windows + kThreads / kWave - 1) / (kThreads / kWave);
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 launch((unsigned)blocks, n < 65535 ? n : 65535);
    if (ws % 16 == 0 && (ws - ov) % 16 == 0 && W % 16 == 0 && aligned16(masks))
        hipLaunchKernelGGL(mask_coverage_pairs_kernel<true>, launch, dim3(kThreads), 0, stream, masks, n, H, W, ws, ws - ov,
                           n_rows, n_cols, count, grid, limit);
    else
        hipLaunchKernelGGL(mask_coverage_pairs_kernel<false>, launch, dim3(kThreads), 0, stream, masks, n, H, W, ws, ws - ov,
                           n_rows, n_cols, count, grid, limit);
    return hipGetLastError();
}

hipError_t launch_mask_fields_pairs(double* u, double* v, uint8_t* invalid, uint8_t* status, const uint8_t* grids, int batch,
                                    int n_rows, int n_cols, int invalid_value, hipStream_t stream) {
    const long long total = (long long)batch * n_rows * n_cols;
    if (total <= 0) return hipSuccess;
    const long long blocks = (total + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mask_fields_pairs_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, stream, u, v, invalid, status,
                       grids, total, (uint8_t)invalid_value);
    return hipGetLastError();
}

hipError_t launch_apply_mask(const uint8_t* frames, int n, long long pixels, const uint8_t* mask, uint8_t* out,
                             hipStream_t stream) {
    if (n <= 0 || pixels <= 0) return hipSuccess;
    const long long lanes = (pixels + 15) / 16;
    const long long blocks = (lanes + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const bool vec = pixels % 16 == 0 && aligned16(frames) && aligned16(mask) && aligned16(out);
    const int rows = vec ? (n + 1) / 2 : n;                 // frame steps (the vector form takes two frames per step)
    const dim3 grid((unsigned)blocks, rows < 65535 ? rows : 65535);
    if (vec)
        hipLaunchKernelGGL(apply_mask_kernel<true>, grid, dim3(kThreads), 0, stream, frames, n, pixels, mask, out);
    else
        hipLaunchKernelGGL(apply_mask_kernel<false>, grid, dim3(kThreads), 0, stream, frames, n, pixels, mask, out);
    return hipGetLastError();
}

hipError_t launch_mask_coverage(const uint8_t* mask, int H, int W, int ws, int ov, int n_rows, int n_cols, int32_t* count,
                                uint8_t* grid, int limit, hipStream_t stream) {
    const long long windows = (long long)n_rows * n_cols;
    if (windows <= 0) return hipSuccess;
    const long long blocks = (windows + kThreads / kWave - 1) / (kThreads / kWave);
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mask_coverage_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, stream, mask, H, W, ws, ws - ov,
                       n_rows, n_cols, count, grid, limit);
    return hipGetLastError();
}

hipError_t launch_mask_fields(double* u, double* v, uint8_t* invalid, uint8_t* status, const uint8_t* grid, int batch,
                              int n_rows, int n_cols, int invalid_value, hipStream_t stream) {
    const long long total = (long long)batch * n_rows * n_cols;
    if (total <= 0) return hipSuccess;
    const long long blocks = (total + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mask_fields_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, stream, u, v, invalid, status, grid,
                       total, n_rows * n_cols, (uint8_t)invalid_value);
    return hipGetLastError();
}

}  // namespace tpiv
