// Tile-wise adaptive histogram equalization (CLAHE) of uint8 frames on the device, in integer arithmetic, every step as
// tests/equalize_model.py and include/torchpiv_hip.h state it, so the result is that model's bit for bit and every
// correlation kernel and precision applies to the equalized frames unchanged.
//
// Two kernels.  equalize_table_kernel: one workgroup of 256 lanes per (frame, tile) -- the histogram of the tile's pixels
// in LDS, then a lane per bin: clip at L, the excess E spread once over all bins, a 256-bin inclusive prefix sum (a
// shuffle scan per wavefront and the four wavefront totals through LDS), and the table lut[256] written to the workspace
// [n, ky, kx, 256].  equalize_map_kernel: one workgroup per rectangle between tile centres of a frame, so that all its
// pixels blend the same four tables; they are staged in LDS interleaved (one dword per grey level holds the four tables'
// bytes: one LDS read per pixel), the weights along y are per row, those along x per column, and the divisor 2 Dy Dx is
// the rectangle's.
//
// The histogram's contention.  PIV frames are dark: most pixels of a tile fall into a handful of bins, and an all-zero
// frame puts all of them into one.  An LDS atomic of a wavefront whose lanes name one address runs lane after lane, and
// private histograms per wavefront do not change that -- the 64 lanes of ONE instruction are the conflict.  So equal
// values are combined within the wavefront before the atomic: up to kPeel times the wavefront takes the value of its
// first lane still waiting, counts the lanes that hold the same one (a ballot) and has that lane add the count; the
// lanes left after that (a tile of noise: nearly all, which then rarely share a bin) add 1 each.  An all-zero tile costs
// one atomic per 64 pixels, a tile with 99 % of its pixels in one bin two or three, and with the atomics 64 times fewer
// the four wavefronts share one histogram.  (depth.hip counts 65536 bins, where equal values in one instruction are
// rare enough to leave to the hardware.)
//
// The map's division.  out = num / den with num = 2 s + Dy Dx < 2^28 and den = 2 Dy Dx <= 819200 uniform over the
// rectangle, quotient <= 255.  est = float(num) * (1.0f / float(den)): float(den) is exact (den < 2^24), float(num), the
// IEEE reciprocal and the product are each rounded once, relative error <= 2^-24 each, so est = Q (1 + e) with
// |e| < 2^-22 and Q = num / den < 256, |est - Q| < 2^-14.  Hence floor(Q) - 1 <= floor(est) <= floor(Q) + 1, and one
// exact integer step -- down if q den > num, else up if (q + 1) den <= num -- gives floor(Q) for every input.
// (q + 1) den <= 257 * 819200 fits 32 bits.  No hardware integer division per pixel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "piv_kernels.h"

namespace tpiv {

namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kPeel = 4;
static_assert(kThreads == 256, "a lane per bin");

__device__ __forceinline__ int edge(int i, int n, int k) { return (int)(((long long)i * n) / k); }

// hist[v] += 1 for every lane with `active`, equal values of the wavefront combined (file header).  Called by all lanes
// of a wavefront together.
__device__ __forceinline__ void count(uint32_t* hist, uint32_t v, bool active, int lane) {
    bool rem = active;
#pragma unroll
    for (int it = 0; it < kPeel; ++it) {
        const unsigned long long m = __ballot(rem);
        if (m == 0) break;
        const int leader = __ffsll(m) - 1;
        const uint32_t lv = (uint32_t)__shfl((int)v, leader);
        const unsigned long long same = __ballot(rem && v == lv);
        if (lane == leader) atomicAdd(&hist[lv], (uint32_t)__popcll(same));
        rem = rem && v != lv;
    }
    if (rem) atomicAdd(&hist[v], 1u);
}

// luts[f][ty][tx][b] for the tile (blockIdx.y, blockIdx.x) of the frames blockIdx.z, + gridDim.z, ...
__global__ __launch_bounds__(kThreads) void equalize_table_kernel(const uint8_t* __restrict__ frames, int n, int H, int W,
                                                                   int ky, int kx, int clip_q8,
                                                                   uint8_t* __restrict__ luts) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t sh_sum[kWaves], sh_first[kWaves], sh_tot[kWaves], sh_cb0;
    const int b = threadIdx.x, lane = b & (kWave - 1), wave = b / kWave;
    const int tx = blockIdx.x, ty = blockIdx.y;
    const int x0 = edge(tx, W, kx), x1 = edge(tx + 1, W, kx), y0 = edge(ty, H, ky), y1 = edge(ty + 1, H, ky);
    const int th = y1 - y0;
    const uint32_t N = (uint32_t)(x1 - x0) * (uint32_t)th;
    uint32_t L = (uint32_t)(((unsigned long long)clip_q8 * N) >> 16);
    L = L > 1 ? L : 1;
    // a lane takes four pixels of a row at a time: an aligned dword where every row starts on a dword boundary (the
    // chunks then start at x0 rounded down and the pixels in front of x0 are masked), bytes otherwise
    const bool vec = (W & 3) == 0 && ((uintptr_t)frames & 3u) == 0;
    const int xa = vec ? (x0 & ~3) : x0;
    const int cw = (x1 - xa + 3) >> 2;                          // chunks per row
    const int items = cw * th;
    const int drow = kThreads / cw, dcol = kThreads - drow * cw;
    for (int f = blockIdx.z; f < n; f += gridDim.z) {
        const uint8_t* __restrict__ fp = frames + (long long)f * H * W;
        hist[b] = 0;
        __syncthreads();
        int row = b / cw, col = b - row * cw;
        for (int base = 0; base < items; base += kThreads) {    // uniform trip count: count() is a wavefront's call
            const bool valid = base + b < items;
            uint32_t px = 0, mask = 0;
            if (valid) {
                const int x = xa + 4 * col;
                const uint8_t* __restrict__ p = fp + (long long)(y0 + row) * W + x;
                if (vec) {
                    px = *reinterpret_cast<const uint32_t*>(p);          // x + 3 < W: W is a multiple of 4
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (x + j >= x0 && x + j < x1) mask |= 1u << j;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (x + j < x1) {
                            px |= (uint32_t)p[j] << (8 * j);
                            mask |= 1u << j;
                        }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) count(hist, (px >> (8 * j)) & 255u, (mask >> j) & 1u, lane);
            row += drow;
            col += dcol;
            if (col >= cw) {
                col -= cw;
                ++row;
            }
        }
        __syncthreads();
        // a lane per bin from here on
        const uint32_t h = hist[b];
        uint32_t ex = h > L ? h - L : 0;
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1) ex += (uint32_t)__shfl_xor((int)ex, o);
        const unsigned long long present = __ballot(h > 0);
        if (lane == 0) {
            sh_sum[wave] = ex;
            sh_first[wave] = present ? (uint32_t)(wave * kWave + __ffsll(present) - 1) : 256u;
        }
        __syncthreads();
        uint32_t E = 0, b0 = 256;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            E += sh_sum[w];
            b0 = sh_first[w] < b0 ? sh_first[w] : b0;
        }
        const uint32_t r = E & 255u;
        const uint32_t h2 = (h < L ? h : L) + (E >> 8) + ((((uint32_t)b + 1) * r >> 8) - ((uint32_t)b * r >> 8));
        uint32_t c = h2;                                        // inclusive prefix sum within the wavefront
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)c, o);
            if (lane >= o) c += t;
        }
        if (lane == kWave - 1) sh_tot[wave] = c;
        if ((uint32_t)b == b0) sh_cb0 = c;                      // (N > 0: some bin is present)
        __syncthreads();
        uint32_t cb0 = sh_cb0;
#pragma unroll
        for (int w = 0; w < kWaves - 1; ++w) {
            if (w < wave) c += sh_tot[w];
            if ((uint32_t)w < (b0 >> 6)) cb0 += sh_tot[w];
        }
        const uint32_t d = N - cb0;
        uint32_t v = 0;
        if (d != 0) v = (510u * (c > cb0 ? c - cb0 : 0u) + d) / (2u * d);       // 510 N + d < 2^27
        luts[((((long long)f * ky + ty) * kx + tx) << 8) + b] = (uint8_t)v;
        __syncthreads();                                        // the next frame clears what was just read
    }
}

// One axis of a rectangle between tile centres: rectangle i of an axis of n pixels in k tiles.  c: the doubled centre of the
// lower tile, D: the doubled distance to the upper tile's, [s, e): the rectangle's pixels, i1: the upper tile.  k == 1: the
// whole axis, D = 1 and the weight of the upper tile 0 (single).
struct Axis {
    int c, D, s, e, i1;
    bool single;
};

__device__ __forceinline__ Axis axis(int i, int n, int k) {
    Axis a;
    if (k == 1) {
        a.c = 0, a.D = 1, a.s = 0, a.e = n, a.i1 = 0, a.single = true;
        return a;
    }
    const int e0 = edge(i, n, k), e1 = edge(i + 1, n, k), e2 = edge(i + 2, n, k);
    a.c = e0 + e1;
    a.D = e2 - e0;
    a.s = i == 0 ? 0 : a.c >> 1;                                // the first pixel p with 2p + 1 >= c
    a.e = i == k - 2 ? n : (e1 + e2) >> 1;
    a.i1 = i + 1;
    a.single = false;
    return a;
}

__device__ __forceinline__ int weight1(const Axis& a, int p) {
    if (a.single) return 0;
    const int w = 2 * p + 1 - a.c;
    return w < 0 ? 0 : (w > a.D ? a.D : w);
}

struct Rect {
    uint32_t wy0, wy1, Dx, DD, den;
    float rden;
};

// one pixel: grey level g, weight wx1 of the right-hand tiles
__device__ __forceinline__ uint32_t blend(const uint32_t* tab, const Rect& q, uint32_t g, uint32_t wx1) {
    const uint32_t e = tab[g], wx0 = q.Dx - wx1;
    const uint32_t top = wx0 * (e & 255u) + wx1 * ((e >> 8) & 255u);
    const uint32_t bot = wx0 * ((e >> 16) & 255u) + wx1 * (e >> 24);
    const uint32_t num = 2u * (q.wy0 * top + q.wy1 * bot) + q.DD;
    uint32_t o = (uint32_t)((float)num * q.rden);               // num / den, off by one at most (file header)
    if (o * q.den > num)
        --o;
    else if ((o + 1) * q.den <= num)
        ++o;
    return o;
}

// out = the blend of the four neighbour tables for the rectangle (blockIdx.y, blockIdx.x) of the frames blockIdx.z, ...
// kVec: every row starts on a 16-byte boundary in frames and in out; a lane then moves the aligned 16-byte groups that lie
// inside the rectangle as one load and one store, and the pixels of a group that straddles the rectangle's edge byte by
// byte.  Otherwise (odd widths, odd offsets) every group starts at the rectangle's edge and moves byte by byte.  A
// pixel is read and written by the same lane and no other pixel is, so out == frames is fine.
template <bool kVec>
__global__ __launch_bounds__(kThreads) void equalize_map_kernel(const uint8_t* frames, int n, int H, int W, int ky, int kx,
                                                                 const uint8_t* __restrict__ luts, uint8_t* out) {
    __shared__ uint32_t tab[256];
    const Axis ax = axis(blockIdx.x, W, kx), ay = axis(blockIdx.y, H, ky);
    const int ix0 = blockIdx.x, iy0 = blockIdx.y;
    Rect q;
    q.Dx = (uint32_t)ax.D;
    q.DD = (uint32_t)ax.D * (uint32_t)ay.D;
    q.den = 2u * q.DD;
    q.rden = 1.0f / (float)q.den;
    const int xa = kVec ? (ax.s & ~15) : ax.s;
    const int cw = (ax.e - xa + 15) >> 4;                       // 16-byte groups per row
    const int items = cw * (ay.e - ay.s);
    const int drow = kThreads / cw, dcol = kThreads - drow * cw;
    for (int f = blockIdx.z; f < n; f += gridDim.z) {
        const uint8_t* __restrict__ t = luts + (((long long)f * ky * kx) << 8) + threadIdx.x;
        tab[threadIdx.x] = (uint32_t)t[((long long)iy0 * kx + ix0) << 8] | ((uint32_t)t[((long long)iy0 * kx + ax.i1) << 8] << 8) |
                           ((uint32_t)t[((long long)ay.i1 * kx + ix0) << 8] << 16) |
                           ((uint32_t)t[((long long)ay.i1 * kx + ax.i1) << 8] << 24);
        __syncthreads();
        const long long fo = (long long)f * H * W;
        int row = threadIdx.x / cw, col = threadIdx.x - row * cw;
        for (int it = threadIdx.x; it < items; it += kThreads) {
            const int y = ay.s + row, x = xa + 16 * col;
            q.wy1 = (uint32_t)weight1(ay, y);
            q.wy0 = (uint32_t)ay.D - q.wy1;
            const long long o = fo + (long long)y * W + x;
            if (kVec && x >= ax.s && x + 16 <= ax.e) {
                const uint4 v = *reinterpret_cast<const uint4*>(frames + o);
                const uint32_t in[4] = {v.x, v.y, v.z, v.w};
                uint32_t res[4];
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    uint32_t w = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        w |= blend(tab, q, (in[d] >> (8 * j)) & 255u, (uint32_t)weight1(ax, x + 4 * d + j)) << (8 * j);
                    res[d] = w;
                }
                *reinterpret_cast<uint4*>(out + o) = make_uint4(res[0], res[1], res[2], res[3]);
            } else {
                for (int j = 0; j < 16; ++j) {
                    const int xx = x + j;
                    if (xx >= ax.s && xx < ax.e) out[o + j] = (uint8_t)blend(tab, q, frames[o + j], (uint32_t)weight1(ax, xx));
                }
            }
            row += drow;
            col += dcol;
            if (col >= cw) {
                col -= cw;
                ++row;
            }
        }
        __syncthreads();                                        // the next frame's tables go where these were read
    }
}

}  // namespace

hipError_t launch_equalize(const uint8_t* frames, int n, int H, int W, int tile, int clip_q8, uint8_t* out, uint8_t* luts,
                           hipStream_t stream) {
    if (n <= 0 || H <= 0 || W <= 0) return hipSuccess;
    if (tile < EQUALIZE_TILE_MIN || tile > EQUALIZE_TILE_MAX || clip_q8 < EQUALIZE_CLIP_Q8_MIN || clip_q8 > EQUALIZE_CLIP_Q8_MAX)
        return hipErrorInvalidValue;
    const int ky = equalize_tiles(H, tile), kx = equalize_tiles(W, tile);
    if (ky > 65535) return hipErrorInvalidValue;
    const unsigned nz = n < 65535 ? n : 65535;
    hipLaunchKernelGGL(equalize_table_kernel, dim3(kx, ky, nz), dim3(kThreads), 0, stream, frames, n, H, W, ky, kx, clip_q8,
                       luts);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    const dim3 grid(kx > 1 ? kx - 1 : 1, ky > 1 ? ky - 1 : 1, nz);
    const bool vec = W % 16 == 0 && (((uintptr_t)frames | (uintptr_t)out) & 15u) == 0;
    if (vec)
        hipLaunchKernelGGL(equalize_map_kernel<true>, grid, dim3(kThreads), 0, stream, frames, n, H, W, ky, kx, luts, out);
    else
        hipLaunchKernelGGL(equalize_map_kernel<false>, grid, dim3(kThreads), 0, stream, frames, n, H, W, ky, kx, luts, out);
    return hipGetLastError();
}

}  // namespace tpiv
