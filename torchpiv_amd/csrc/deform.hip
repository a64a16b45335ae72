// Iterative image deformation behind the last pass (include/torchpiv_hip.h: tpiv_deform_nodes / _warp / _combine).  The
// last pass's field becomes a grid of Q8 half shifts (the nodes), both frames of a pair are warped by the dense, bilinear
// field between the nodes -- frame a by -h, frame b by +h -- into uint8 frames, the unchanged first pass measures the
// residual on them and the combine adds it to the shift that was applied.  Integer in, integer out, integer in between up
// to that last addition, so every implementation of the header's lines gives the same bytes.
//
// Nodes and combine: a lane per cell.  The node kernel stages a 16 x 16 block of cells with a halo of two in LDS
// (quantised values and validity), forms the neighbour substitution of invalid cells on the block with a halo of one (at
// the edge-replicated coordinates the smoothing reads), then the 3 x 3 binomial: one launch, no work memory.
//
// Warp: one kernel for both frames, so the dense shift is formed once per pixel.  A workgroup of 256 lanes owns a tile of
// 64 x 32 output pixels, a lane four horizontally adjacent pixels in two rows 16 apart.  The workgroup
//   1. computes the node cell and the Q8 weight of the tile's 64 columns and 32 rows once, into LDS;
//   2. stages the nodes the tile touches in LDS (at most 65 x 33) and takes their minimum and maximum per component: the
//      dense shift is a convex combination of them, rounded to nearest, so it stays inside that interval;
//   3. derives from it the bounding box of the tile's source footprint in each frame: the clamped Q8 corners, shifted by
//      the extreme h, plus the interpolation's taps;
//   4. if both boxes fit the fixed LDS patches (48 rows x 96 bytes per frame, the left edge aligned down to 16 bytes),
//      loads them in 16-byte row pieces -- rows and whole pieces clamp at the frame edge while loading (the edge byte
//      replicated), so the sampler needs no clamp -- and samples every pixel from LDS: per tap row two dword reads and
//      one byte alignment give the four taps;
//   5. otherwise (a predictor discontinuity, a huge gradient) takes the per-pixel global gather with clamped taps: the
//      same arithmetic, the same bytes.  The choice is uniform over the workgroup.
// The 16-byte pieces need W % 16 == 0 and 16-byte aligned frames; other frames fill the patch byte by byte.  W % 4 != 0 or
// an unaligned output falls back to byte stores.  Every global address comes from a clamped index.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "piv_kernels.h"

namespace tpiv {

namespace {

constexpr int kThreads = 256;
constexpr int kTW = 64, kTH = 32;             // output tile
constexpr int kPW = 96, kPH = 48;             // LDS patch per frame: bytes per row (a multiple of 16), rows
constexpr int kNodeW = 66, kNodeH = 34;       // staged nodes: at most 63 / st + 2 <= 65 columns, 31 / st + 2 <= 33 rows
constexpr int kNB = 16;                       // node kernel: cells per side of a block

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ int floordiv(int a, int b) {       // b > 0
    return a >= 0 ? a / b : -((-a + b - 1) / b);
}

// ---- nodes ------------------------------------------------------------------------------------------------------------

// clamp(rint(w * 128), -16383, 16383): the product is exact (or +-inf, which the clamp takes)
__device__ __forceinline__ int quantise(double w) {
    const double t = rint(w * 128.0);
    return (int)(t < -16383.0 ? -16383.0 : (t > 16383.0 ? 16383.0 : t));
}

__device__ __forceinline__ bool finite64(double x) {
    return (__double_as_longlong(x) & 0x7ff0000000000000LL) != 0x7ff0000000000000LL;
}

__global__ __launch_bounds__(kThreads) void deform_nodes_kernel(const double* __restrict__ u, const double* __restrict__ v,
                                                                const uint8_t* __restrict__ invalid, int n_rows, int n_cols,
                                                                int smooth, int16_t* __restrict__ nodes) {
    constexpr int kA = kNB + 4, kB = kNB + 2;
    __shared__ int qa[kA * kA][2];      // quantised values, halo 2
    __shared__ uint8_t ok[kA * kA];     // 1 = in the grid and valid
    __shared__ int sb[kB * kB][2];      // after the substitution, halo 1, at edge-replicated coordinates
    const int tid = threadIdx.x;
    const int c0 = blockIdx.x * kNB, r0 = blockIdx.y * kNB;
    const size_t field = (size_t)blockIdx.z * n_rows * n_cols;
    for (int i = tid; i < kA * kA; i += kThreads) {
        const int gr = r0 - 2 + i / kA, gc = c0 - 2 + i % kA;
        int qx = 0, qy = 0;
        uint8_t good = 0;
        if (gr >= 0 && gr < n_rows && gc >= 0 && gc < n_cols) {
            const size_t cell = field + (size_t)gr * n_cols + gc;
            const double uu = u[cell], vv = v[cell];
            if (invalid[cell] == 0 && finite64(uu) && finite64(vv)) {
                good = 1;
                qx = quantise(uu);
                qy = quantise(vv);
            }
        }
        qa[i][0] = qx;
        qa[i][1] = qy;
        ok[i] = good;
    }
    __syncthreads();
    for (int i = tid; i < kB * kB; i += kThreads) {
        const int gr = clampi(r0 - 1 + i / kB, 0, n_rows - 1), gc = clampi(c0 - 1 + i % kB, 0, n_cols - 1);
        const int at = (gr - r0 + 2) * kA + (gc - c0 + 2);
        int qx = qa[at][0], qy = qa[at][1];
        if (!ok[at]) {      // the mean of the valid neighbours, rounded half up; cells outside the grid were staged as not ok
            int sx = 0, sy = 0, k = 0;
#pragma unroll
            for (int dr = -1; dr <= 1; ++dr)
#pragma unroll
                for (int dc = -1; dc <= 1; ++dc) {
                    const int nb = at + dr * kA + dc;
                    if ((dr != 0 || dc != 0) && ok[nb]) {
                        sx += qa[nb][0];
                        sy += qa[nb][1];
                        ++k;
                    }
                }
            qx = k ? floordiv(2 * sx + k, 2 * k) : 0;
            qy = k ? floordiv(2 * sy + k, 2 * k) : 0;
        }
        sb[i][0] = qx;
        sb[i][1] = qy;
    }
    __syncthreads();
    const int tx = tid % kNB, ty = tid / kNB;
    const int r = r0 + ty, c = c0 + tx;
    if (r >= n_rows || c >= n_cols) return;
    const int at = (ty + 1) * kB + tx + 1;
    int qx = sb[at][0], qy = sb[at][1];
    if (smooth) {
        int sx = 0, sy = 0;
#pragma unroll
        for (int dr = -1; dr <= 1; ++dr)
#pragma unroll
            for (int dc = -1; dc <= 1; ++dc) {
                const int w = (dr == 0 ? 2 : 1) * (dc == 0 ? 2 : 1);
                sx += w * sb[at + dr * kB + dc][0];
                sy += w * sb[at + dr * kB + dc][1];
            }
        qx = (sx + 8) >> 4;
        qy = (sy + 8) >> 4;
    }
    const size_t cell = field + (size_t)r * n_cols + c;
    reinterpret_cast<uint32_t*>(nodes)[cell] = ((uint32_t)qx & 0xffffu) | ((uint32_t)qy << 16);
}

// ---- combine ----------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kThreads) void deform_combine_kernel(const int16_t* __restrict__ nodes,
                                                                  const double* __restrict__ du, const double* __restrict__ dv,
                                                                  const uint8_t* __restrict__ dval, size_t n,
                                                                  double* __restrict__ u, double* __restrict__ v,
                                                                  uint8_t* __restrict__ invalid) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t q = reinterpret_cast<const uint32_t*>(nodes)[i];
    const int qx = (int)(int16_t)(q & 0xffffu), qy = (int)q >> 16;
    u[i] = (double)qx * (1.0 / 128) + du[i];      // the product is exact: one rounding
    v[i] = (double)qy * (1.0 / 128) + dv[i];
    invalid[i] = dval[i];
}

// ---- warp -------------------------------------------------------------------------------------------------------------

// node cell r and Q8 weight w (0..256) of pixel coordinate y along an axis of n windows
__device__ __forceinline__ void axis_cell(int y, int n, int ws, int st, int& r, int& w) {
    r = 0;
    w = 0;
    if (n == 1) return;
    const int a = 2 * y - (ws - 1);
    r = clampi(floordiv(a, 2 * st), 0, n - 2);
    const int t = clampi(a - 2 * r * st, 0, 2 * st);
    w = (256 * t + st) / (2 * st);
}

// the four Q10 weights of fraction f, one 8-byte LDS read
__device__ __forceinline__ void weights(const int16_t* tab, int f, int w[4]) {
    const uint2 t = *reinterpret_cast<const uint2*>(tab + 4 * f);
    w[0] = (int)(int16_t)(t.x & 0xffffu);
    w[1] = (int)t.x >> 16;
    w[2] = (int)(int16_t)(t.y & 0xffffu);
    w[3] = (int)t.y >> 16;
}

// A cubic pixel value leaves its sampler through an empty asm statement, which keeps the shift, the clamp and the packing
// of a lane's four bytes separate instructions.  Fused into gfx950's v_ashr_pk_u8_i32 (two shifts, two clamps, two bytes)
// a pair of pixels arrived with the old upper half of the destination register still in place -- the instruction writes
// 16 bits, the packing behind it took them for 32 -- and the third byte of a lane's dword came out with bit 0 set.
__device__ __forceinline__ uint32_t opaque(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(v));
#endif
    return v;
}

// One pixel from global memory, taps clamped to the frame: tpiv_dewarp's arithmetic without its outside case.
template <bool kCubic>
__device__ __forceinline__ uint32_t sample_gather(const uint8_t* __restrict__ src, int H, int W, int qx, int qy,
                                                  const int16_t* tab) {
    const int ix = qx >> 8, iy = qy >> 8, fx = qx & 255, fy = qy & 255;
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
        return opaque((uint32_t)clampi(acc >> 20, 0, 255));
    } else {
        const int x0 = clampi(ix, 0, W - 1), x1 = clampi(ix + 1, 0, W - 1);
        const uint8_t* __restrict__ r0 = src + clampi(iy, 0, H - 1) * W;
        const uint8_t* __restrict__ r1 = src + clampi(iy + 1, 0, H - 1) * W;
        const int top = (256 - fx) * (int)r0[x0] + fx * (int)r0[x1];
        const int bot = (256 - fx) * (int)r1[x0] + fx * (int)r1[x1];
        return (uint32_t)(((256 - fy) * top + fy * bot + 32768) >> 16);
    }
}

// The same pixel from the LDS patch whose byte (0, 0) is frame position (py, px) (edge-replicated while loading).  The box
// test guarantees that every tap lies inside the patch.  Per tap row: the two dwords around the first tap, aligned.
template <bool kCubic>
__device__ __forceinline__ uint32_t sample_lds(const uint8_t* pt, int px, int py, int qx, int qy, const int16_t* tab) {
    const int ix = qx >> 8, iy = qy >> 8, fx = qx & 255, fy = qy & 255;
    constexpr int kLo = kCubic ? 1 : 0;
    const int o = (iy - kLo - py) * kPW + (ix - kLo - px);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(pt + (o & ~3));
    const uint32_t sh = (uint32_t)o & 3u;
    if constexpr (kCubic) {
        int tx[4], ty[4];
        weights(tab, fx, tx);
        weights(tab, fy, ty);
        int acc = 1 << 19;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const uint32_t t = __builtin_amdgcn_alignbyte(w[a * (kPW / 4) + 1], w[a * (kPW / 4)], sh);
            const int s = tx[0] * (int)(t & 255u) + tx[1] * (int)((t >> 8) & 255u) + tx[2] * (int)((t >> 16) & 255u) +
                          tx[3] * (int)(t >> 24);
            acc += ty[a] * s;
        }
        return opaque((uint32_t)clampi(acc >> 20, 0, 255));
    } else {
        const uint32_t t0 = __builtin_amdgcn_alignbyte(w[1], w[0], sh);
        const uint32_t t1 = __builtin_amdgcn_alignbyte(w[kPW / 4 + 1], w[kPW / 4], sh);
        const int top = (256 - fx) * (int)(t0 & 255u) + fx * (int)((t0 >> 8) & 255u);
        const int bot = (256 - fx) * (int)(t1 & 255u) + fx * (int)((t1 >> 8) & 255u);
        return (uint32_t)(((256 - fy) * top + fy * bot + 32768) >> 16);
    }
}

// `rows` x `pieces` 16-byte pieces of the frame `src` from frame position (py, px) on into the patch; px % 16 == 0.
// kWide (W % 16 == 0, 16-byte aligned frames): a piece lies inside the row or outside it as a whole.
template <bool kWide>
__device__ __forceinline__ void load_patch(uint8_t* pt, const uint8_t* __restrict__ src, int H, int W, int px, int py,
                                           int rows, int pieces, int tid) {
    for (int i = tid; i < rows * pieces; i += kThreads) {
        const int pr = i / pieces, k = i - pr * pieces;
        const uint8_t* __restrict__ row = src + clampi(py + pr, 0, H - 1) * W;
        const int gx = px + 16 * k;
        uint4 val;
        if constexpr (kWide) {
            if (gx >= 0 && gx < W) {
                val = *reinterpret_cast<const uint4*>(row + gx);
            } else {
                const uint32_t e = (uint32_t)row[gx < 0 ? 0 : W - 1] * 0x01010101u;
                val = make_uint4(e, e, e, e);
            }
        } else {
            uint32_t d[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                d[j] = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) d[j] |= (uint32_t)row[clampi(gx + 4 * j + b, 0, W - 1)] << (8 * b);
            }
            val = make_uint4(d[0], d[1], d[2], d[3]);
        }
        *reinterpret_cast<uint4*>(pt + pr * kPW + 16 * k) = val;
    }
}

// kVec: W % 4 == 0 and 4-byte aligned outputs; wide: load_patch's kWide (both decided by the launcher, uniform).
template <bool kCubic, bool kVec>
__global__ __launch_bounds__(kThreads) void deform_warp_kernel(DeformWarpParams p, int wide) {
    __shared__ __attribute__((aligned(16))) uint8_t patch[2][kPH * kPW + 16];      // (+ 16: the second dword of the last tap row)
    __shared__ __attribute__((aligned(8))) int16_t tab[kCubic ? 1024 : 4];
    __shared__ uint32_t node[kNodeH * kNodeW];       // x | y << 16
    __shared__ uint32_t colinfo[kTW], rowinfo[kTH];  // staged node index | index of the next node << 8 | weight << 16
    __shared__ int box[4];                           // min hx, max hx, min hy, max hy over the staged nodes
    const int tid = threadIdx.x;
    const int H = p.H, W = p.W, st = p.ws - p.ov;
    const int tx0 = blockIdx.x * kTW, ty0 = blockIdx.y * kTH, f = blockIdx.z;
    const int tw = W - tx0 < kTW ? W - tx0 : kTW, th = H - ty0 < kTH ? H - ty0 : kTH;

    // 1. the tile's columns and rows: node cell and weight.  The cells grow with the coordinate: the first pixel has the
    // lowest, the last the highest
    int cb, rb, ce, re, wdummy;
    axis_cell(tx0, p.n_cols, p.ws, st, cb, wdummy);
    axis_cell(ty0, p.n_rows, p.ws, st, rb, wdummy);
    axis_cell(tx0 + tw - 1, p.n_cols, p.ws, st, ce, wdummy);
    axis_cell(ty0 + th - 1, p.n_rows, p.ws, st, re, wdummy);
    const int ncn = (ce + 1 < p.n_cols ? ce + 1 : p.n_cols - 1) - cb + 1;
    const int nrn = (re + 1 < p.n_rows ? re + 1 : p.n_rows - 1) - rb + 1;
    if (tid < kTW) {
        int c, w;
        axis_cell(tx0 + (tid < tw ? tid : tw - 1), p.n_cols, p.ws, st, c, w);
        const int c1 = c + 1 < p.n_cols ? c + 1 : p.n_cols - 1;
        colinfo[tid] = (uint32_t)(c - cb) | ((uint32_t)(c1 - cb) << 8) | ((uint32_t)w << 16);
    } else if (tid < kTW + kTH) {
        const int j = tid - kTW;
        int r, w;
        axis_cell(ty0 + (j < th ? j : th - 1), p.n_rows, p.ws, st, r, w);
        const int r1 = r + 1 < p.n_rows ? r + 1 : p.n_rows - 1;
        rowinfo[j] = (uint32_t)(r - rb) | ((uint32_t)(r1 - rb) << 8) | ((uint32_t)w << 16);
    }
    if (tid == kThreads - 1) {
        box[0] = 0x7fffffff;
        box[1] = -0x7fffffff;
        box[2] = 0x7fffffff;
        box[3] = -0x7fffffff;
    }
    if constexpr (kCubic) {
        for (int i = tid; i < 1024; i += kThreads) tab[i] = p.table[i];
    }
    __syncthreads();

    // 2. the nodes the tile touches, and their extremes
    {
        const uint32_t* __restrict__ gn = reinterpret_cast<const uint32_t*>(p.nodes) + (size_t)f * p.n_rows * p.n_cols;
        int x0 = 0x7fffffff, x1 = -0x7fffffff, y0 = 0x7fffffff, y1 = -0x7fffffff;
        for (int i = tid; i < nrn * ncn; i += kThreads) {
            const int rr = i / ncn, cc = i - rr * ncn;
            const uint32_t q = gn[(size_t)(rb + rr) * p.n_cols + cb + cc];
            node[rr * kNodeW + cc] = q;
            const int hx = (int)(int16_t)(q & 0xffffu), hy = (int)q >> 16;
            x0 = hx < x0 ? hx : x0;
            x1 = hx > x1 ? hx : x1;
            y0 = hy < y0 ? hy : y0;
            y1 = hy > y1 ? hy : y1;
        }
        if (tid < nrn * ncn) {
            atomicMin(&box[0], x0);
            atomicMax(&box[1], x1);
            atomicMin(&box[2], y0);
            atomicMax(&box[3], y1);
        }
    }
    __syncthreads();

    // 3. the source footprint of the tile in each frame, in whole pixels: frame a is read at clamp(x - h), frame b at
    // clamp(x + h), and clamping is monotonic
    constexpr int kLo = kCubic ? 1 : 0, kHi = kCubic ? 2 : 1;
    const int XM = (W - 1) << 8, YM = (H - 1) << 8;
    const int xl = tx0 << 8, xr = (tx0 + tw - 1) << 8, yt = ty0 << 8, yb = (ty0 + th - 1) << 8;
    const int hx0 = box[0], hx1 = box[1], hy0 = box[2], hy1 = box[3];
    int px[2], py[2], rows[2], pieces[2];
    bool fits = p.force_gather == 0;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int a0 = clampi(s ? xl + hx0 : xl - hx1, 0, XM) >> 8, a1 = clampi(s ? xr + hx1 : xr - hx0, 0, XM) >> 8;
        const int b0 = clampi(s ? yt + hy0 : yt - hy1, 0, YM) >> 8, b1 = clampi(s ? yb + hy1 : yb - hy0, 0, YM) >> 8;
        px[s] = (a0 - kLo) & ~15;
        py[s] = b0 - kLo;
        const int cols = a1 + kHi - px[s] + 1;
        rows[s] = b1 + kHi - py[s] + 1;
        pieces[s] = (cols + 15) >> 4;
        fits = fits && cols <= kPW && rows[s] <= kPH;
    }
    const size_t frame = (size_t)f * H * W;
    const uint8_t* __restrict__ srcA = p.A + frame;
    const uint8_t* __restrict__ srcB = p.B + frame;

    // 4. the patches
    if (fits) {
        if (wide) {
            load_patch<true>(patch[0], srcA, H, W, px[0], py[0], rows[0], pieces[0], tid);
            load_patch<true>(patch[1], srcB, H, W, px[1], py[1], rows[1], pieces[1], tid);
        } else {
            load_patch<false>(patch[0], srcA, H, W, px[0], py[0], rows[0], pieces[0], tid);
            load_patch<false>(patch[1], srcB, H, W, px[1], py[1], rows[1], pieces[1], tid);
        }
    }
    if (tid == 0 && p.counter) atomicAdd(&p.counter[fits ? 0 : 1], 1);
    __syncthreads();

    // 5. the pixels: four in a row per lane, two rows 16 apart
    const int lx = (tid & 15) * 4, ly = tid >> 4;
    const int x = tx0 + lx;
    if (x >= W) return;
    const int cnt = kVec ? 4 : (W - x < 4 ? W - x : 4);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int yl = ly + 16 * j, y = ty0 + yl;
        if (y >= H) break;
        const uint32_t ri = rowinfo[yl];
        const int wy = (int)(ri >> 16);
        const uint32_t* n0 = node + (ri & 255u) * kNodeW;
        const uint32_t* n1 = node + ((ri >> 8) & 255u) * kNodeW;
        uint32_t oa = 0, ob = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t ci = colinfo[lx + k];     // (columns past the frame were staged as its last column)
            const int wx = (int)(ci >> 16);
            const uint32_t q00 = n0[ci & 255u], q01 = n0[(ci >> 8) & 255u], q10 = n1[ci & 255u], q11 = n1[(ci >> 8) & 255u];
            const int hx = ((256 - wy) * ((256 - wx) * (int)(int16_t)(q00 & 0xffffu) + wx * (int)(int16_t)(q01 & 0xffffu)) +
                            wy * ((256 - wx) * (int)(int16_t)(q10 & 0xffffu) + wx * (int)(int16_t)(q11 & 0xffffu)) + 32768) >> 16;
            const int hy = ((256 - wy) * ((256 - wx) * ((int)q00 >> 16) + wx * ((int)q01 >> 16)) +
                            wy * ((256 - wx) * ((int)q10 >> 16) + wx * ((int)q11 >> 16)) + 32768) >> 16;
            const int xq = (x + k < W ? x + k : W - 1) << 8;
            const int qxa = clampi(xq - hx, 0, XM), qya = clampi((y << 8) - hy, 0, YM);
            const int qxb = clampi(xq + hx, 0, XM), qyb = clampi((y << 8) + hy, 0, YM);
            uint32_t va, vb;
            if (fits) {
                va = sample_lds<kCubic>(patch[0], px[0], py[0], qxa, qya, tab);
                vb = sample_lds<kCubic>(patch[1], px[1], py[1], qxb, qyb, tab);
            } else {
                va = sample_gather<kCubic>(srcA, H, W, qxa, qya, tab);
                vb = sample_gather<kCubic>(srcB, H, W, qxb, qyb, tab);
            }
            oa |= va << (8 * k);
            ob |= vb << (8 * k);
        }
        uint8_t* __restrict__ da = p.wa + frame + (size_t)y * W + x;
        uint8_t* __restrict__ db = p.wb + frame + (size_t)y * W + x;
        if constexpr (kVec) {
            *reinterpret_cast<uint32_t*>(da) = oa;
            *reinterpret_cast<uint32_t*>(db) = ob;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < cnt) {
                    da[k] = (uint8_t)(oa >> (8 * k));
                    db[k] = (uint8_t)(ob >> (8 * k));
                }
        }
    }
}

}  // namespace

hipError_t launch_deform_nodes(const double* u, const double* v, const uint8_t* invalid, int batch, int n_rows, int n_cols,
                               int smooth, int16_t* nodes, hipStream_t stream) {
    if (batch <= 0 || n_rows <= 0 || n_cols <= 0) return hipSuccess;
    const dim3 grid((unsigned)((n_cols + kNB - 1) / kNB), (unsigned)((n_rows + kNB - 1) / kNB), (unsigned)batch);
    if (grid.y > 65535u || grid.z > 65535u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(deform_nodes_kernel, grid, dim3(kThreads), 0, stream, u, v, invalid, n_rows, n_cols, smooth, nodes);
    return hipGetLastError();
}

hipError_t launch_deform_combine(const int16_t* nodes, const double* du, const double* dv, const uint8_t* dval, size_t cells,
                                 double* u, double* v, uint8_t* invalid, hipStream_t stream) {
    if (cells == 0) return hipSuccess;
    const size_t blocks = (cells + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffffULL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(deform_combine_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, stream, nodes, du, dv, dval, cells, u,
                       v, invalid);
    return hipGetLastError();
}

hipError_t launch_deform_warp(const DeformWarpParams& p, hipStream_t stream) {
    if (p.batch <= 0 || p.H <= 0 || p.W <= 0) return hipSuccess;
    const dim3 grid((unsigned)((p.W + kTW - 1) / kTW), (unsigned)((p.H + kTH - 1) / kTH), (unsigned)p.batch);
    if (grid.y > 65535u || grid.z > 65535u) return hipErrorInvalidValue;
    const bool vec = p.W % 4 == 0 && (((uintptr_t)p.wa | (uintptr_t)p.wb) & 3u) == 0;
    const int wide = p.W % 16 == 0 && (((uintptr_t)p.A | (uintptr_t)p.B) & 15u) == 0;
    const bool cubic = p.interp == DEWARP_CUBIC;
    auto* kernel = vec ? (cubic ? deform_warp_kernel<true, true> : deform_warp_kernel<false, true>)
                       : (cubic ? deform_warp_kernel<true, false> : deform_warp_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, stream, p, wide);
    return hipGetLastError();
}

}  // namespace tpiv
