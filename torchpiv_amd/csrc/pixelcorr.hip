// Single-pixel ensemble correlation (include/torchpiv_hip.h: tpiv_pixel_corr_add / _peaks).
//
// The add kernel.  A workgroup of four wavefronts owns a rectangle of whole bins (owner computes: nobody else touches their
// cells of acc, so the one int64 read-modify-write per call needs no atomics) and walks it in tiles of 8 x 32 pixels.  A
// lane owns four adjacent pixels of a tile row; the four wavefronts share the tile and split the displacement ROWS: in a
// pass over 4 JW rows, wave w takes the rows j0 + w, j0 + w + 4, ..., JW of them, and keeps 4 pixels x D columns x JW rows
// of partial sums in registers over the whole batch (JW by D so that these are at most 136 registers: PixelSplit).  The
// frames are staged four pairs at a time as one dword per pixel -- a 4 x 4 byte transpose on the way into LDS -- so that
// one v_dot4_u32_u8 adds a pixel's products of four pairs; pairs beyond the batch, pixels of a outside the owned bins and
// pixels of b outside the frame are staged as zeros, which keeps the inner loop free of branches.  Behind the batch the
// sums of a row go through a per-wave LDS slab, eight displacement columns at a time, where one lane per (bin, column) adds
// the bin's pixels of this tile and does the read-modify-write.  A bin larger than a tile is walked by its owner tile after
// tile; the same lane updates the same cell every time, so program order keeps the updates apart.
//
// Overflow.  A lane's sum: batch x 255^2 <= 256 x 65025 < 2^24.  A bin's sum of one tile: at most 256 pixels of those,
// 256 x 256 x 65025 = 4 261 478 400 < 2^32 = 4 294 967 296: uint32 all the way to the widening add into acc -- the reason
// for kPixelCorrMaxBatch = 256.  mom: 256 x 65025 < 2^24 per call.
//
// The peaks kernel: one wavefront per bin, the D x D plane of coefficients in LDS; float64 one operation at a time.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "piv_kernels.h"

namespace tpiv {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = 4;
constexpr int kTH = 8, kTW = 32;           // tile: 8 rows of 32 pixels = 64 lanes x 4 adjacent pixels
constexpr int kQuads = 4;                  // groups of four pairs staged per round
constexpr int kChunk = 8;                  // displacement columns per trip through the reduction slab

template <int R>
struct PixelSplit {
    static constexpr int D = 2 * R + 1;
    static constexpr int kFit = 136 / (4 * D);                           // rows of D x 4 sums that fit 136 registers
    static constexpr int kNeed = (D + kWaves - 1) / kWaves;              // rows a wave needs to cover all D in one pass
    static constexpr int JW = kFit < 1 ? 1 : (kFit < kNeed ? kFit : kNeed);
    static constexpr int JG = kWaves * JW;                               // displacement rows per pass
    static constexpr int kPasses = (D + JG - 1) / JG;
    static constexpr int kBRows = kTH + JG - 1;
    static constexpr int kBCols = (kTW + 2 * R + 3 + 3) / 4 * 4;         // + up to 3 columns in front: the tile starts 4-aligned
};

struct PixelAddParams {
    const uint8_t* a;
    const uint8_t* b;
    long long* acc;
    int batch, H, W, ky, kx, sy, sx;
    int nby, nbx;              // bins
    int gby, gbx;              // bins per workgroup (rows, columns)
    int ngx;                   // workgroups per row of groups
    int vec;                   // frames 4-byte aligned and W % 4 == 0: dword loads
};

// four adjacent pixels (x .. x + 3) of up to four pairs, transposed: out[k] = the bytes of pixel x + k in pairs 0..3.  Zero
// outside [ylo, yhi) x [xlo, xhi) and for pairs >= n.  vec: rows start 4-byte aligned, so x % 4 == 0 allows a dword load.
__device__ __forceinline__ void stage4(const uint8_t* __restrict__ f, long long plane, int n, int W, int y, int x, int ylo,
                                       int yhi, int xlo, int xhi, bool vec, uint32_t out[4]) {
    uint32_t r[4] = {0u, 0u, 0u, 0u};
    if (y >= ylo && y < yhi && x + 3 >= xlo && x < xhi) {
        const long long o = (long long)y * W + x;
        if (vec && (x & 3) == 0 && x >= xlo && x + 4 <= xhi) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n) r[k] = *reinterpret_cast<const uint32_t*>(f + k * plane + o);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k < n) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (x + e >= xlo && x + e < xhi) r[k] |= (uint32_t)f[k * plane + o + e] << (8 * e);
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        out[e] = ((r[0] >> (8 * e)) & 0xffu) | (((r[1] >> (8 * e)) & 0xffu) << 8) | (((r[2] >> (8 * e)) & 0xffu) << 16) |
                 (((r[3] >> (8 * e)) & 0xffu) << 24);
}

template <int R>
__global__ __launch_bounds__(kThreads) void pixel_corr_add_kernel(PixelAddParams p) {
    using S = PixelSplit<R>;
    constexpr int D = S::D, JW = S::JW, JG = S::JG;
    __shared__ uint32_t sa[kQuads][kTH * kTW];
    __shared__ uint32_t sb[kQuads][S::kBRows * S::kBCols];
    __shared__ uint32_t red[kWaves][kChunk][kTH * kTW];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int ly = lane >> 3, lx4 = (lane & 7) * 4;
    const int gy = blockIdx.x / p.ngx, gx = blockIdx.x % p.ngx;
    const int by0 = gy * p.gby, bx0 = gx * p.gbx;                         // first bin of the group
    const int nby = min(p.gby, p.nby - by0), nbx = min(p.gbx, p.nbx - bx0);
    const int ry0 = by0 * p.ky, rx0 = bx0 * p.kx;                         // the owned pixel rectangle
    const int ry1 = ry0 + nby * p.ky, rx1 = rx0 + nbx * p.kx;
    const long long plane = (long long)p.H * p.W;
    const int n_quads = (p.batch + 3) / 4;
    // b tile: column c is frame column bx_org + c, bx_org 4-aligned; the lane's first column of displacement column 0 is xo
    const int xshift = p.sx - R;
    const int xo = ((xshift % 4) + 4) % 4;

    for (int ty0 = ry0; ty0 < ry1; ty0 += kTH) {
        for (int tx0 = rx0; tx0 < rx1; tx0 += kTW) {
            const int bx_org = tx0 + xshift - xo;
#pragma unroll 1
            for (int pass = 0; pass < S::kPasses; ++pass) {
                const int j0 = pass * JG;
                const int by_org = ty0 + p.sy - R + j0;                  // b tile: row r is frame row by_org + r
                uint32_t s[JW][D][4];
#pragma unroll
                for (int jj = 0; jj < JW; ++jj)
#pragma unroll
                    for (int i = 0; i < D; ++i)
#pragma unroll
                        for (int k = 0; k < 4; ++k) s[jj][i][k] = 0u;

#pragma unroll 1
                for (int q0 = 0; q0 < n_quads; q0 += kQuads) {
                    __syncthreads();                                     // the round before has been read
                    {   // a: kQuads x 64 groups of four pixels, one per thread
                        const int q = tid >> 6, g = tid & 63;
                        const int pair0 = 4 * (q0 + q);
                        const int n = min(max(p.batch - pair0, 0), 4);
                        uint32_t o[4];
                        stage4(p.a + (long long)pair0 * plane, plane, n, p.W, ty0 + (g >> 3), tx0 + (g & 7) * 4, ry0, ry1, rx0,
                               rx1, p.vec != 0, o);
                        *reinterpret_cast<uint4*>(&sa[q][g * 4]) = make_uint4(o[0], o[1], o[2], o[3]);
                    }
                    constexpr int kGroups = S::kBCols / 4, kPerQuad = S::kBRows * kGroups;
                    for (int idx = tid; idx < kQuads * kPerQuad; idx += kThreads) {
                        const int q = idx / kPerQuad, rem = idx % kPerQuad;
                        const int r = rem / kGroups, g = rem % kGroups;
                        const int pair0 = 4 * (q0 + q);
                        const int n = min(max(p.batch - pair0, 0), 4);
                        uint32_t o[4];
                        stage4(p.b + (long long)pair0 * plane, plane, n, p.W, by_org + r, bx_org + g * 4, 0, p.H, 0, p.W,
                               p.vec != 0, o);
                        *reinterpret_cast<uint4*>(&sb[q][r * S::kBCols + g * 4]) = make_uint4(o[0], o[1], o[2], o[3]);
                    }
                    __syncthreads();
                    const int nq = min(kQuads, n_quads - q0);
#pragma unroll 1
                    for (int q = 0; q < nq; ++q) {
                        const uint4 av = *reinterpret_cast<const uint4*>(&sa[q][ly * kTW + lx4]);
                        const uint32_t a4[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
                        for (int jj = 0; jj < JW; ++jj) {
                            if (j0 + jj * kWaves + wave < D) {           // (the same in every lane of a wave)
                                const uint32_t* __restrict__ row = &sb[q][(ly + jj * kWaves + wave) * S::kBCols + lx4 + xo];
                                uint32_t bv[D + 3];
#pragma unroll
                                for (int c = 0; c < D + 3; ++c) bv[c] = row[c];
#pragma unroll
                                for (int i = 0; i < D; ++i)
#pragma unroll
                                    for (int k = 0; k < 4; ++k)
                                        s[jj][i][k] = __builtin_amdgcn_udot4(a4[k], bv[i + k], s[jj][i][k], false);
                            }
                        }
                    }
                }

                // the sums of this tile into the bins: per row of the wave, kChunk columns at a time through red[wave]
#pragma unroll
                for (int jj = 0; jj < JW; ++jj) {
                    const int j = j0 + jj * kWaves + wave;
#pragma unroll
                    for (int ic = 0; ic < D; ic += kChunk) {
                        const int cw = D - ic < kChunk ? D - ic : kChunk;
                        __syncthreads();
#pragma unroll
                        for (int il = 0; il < kChunk; ++il)
                            if (ic + il < D)
                                *reinterpret_cast<uint4*>(&red[wave][il][ly * kTW + lx4]) =
                                    make_uint4(s[jj][ic + il][0], s[jj][ic + il][1], s[jj][ic + il][2], s[jj][ic + il][3]);
                        __syncthreads();
                        if (j < D) {
                            const int n_combo = nby * nbx * cw;
                            for (int c = lane; c < n_combo; c += 64) {
                                const int il = c % cw, bb = c / cw;
                                const int br = bb / nbx, bc = bb % nbx;
                                const int y_lo = max(ry0 + br * p.ky, ty0), y_hi = min(ry0 + (br + 1) * p.ky, ty0 + kTH);
                                const int x_lo = max(rx0 + bc * p.kx, tx0), x_hi = min(rx0 + (bc + 1) * p.kx, tx0 + kTW);
                                if (y_lo >= y_hi || x_lo >= x_hi) continue;
                                uint32_t sum = 0u;
                                for (int y = y_lo; y < y_hi; ++y)
                                    for (int x = x_lo; x < x_hi; ++x) sum += red[wave][il][(y - ty0) * kTW + (x - tx0)];
                                const long long cell = ((long long)(by0 + br) * p.nbx + (bx0 + bc)) * (D * D) + j * D + ic + il;
                                p.acc[cell] += (long long)sum;
                            }
                        }
                    }
                }
            }
        }
    }
}

// mom[0..3][y][x] += sum over the batch of a, a^2, b, b^2
__global__ __launch_bounds__(kThreads) void pixel_corr_mom_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                                   int batch, long long pixels, long long* __restrict__ mom) {
    const long long px = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (px >= pixels) return;
    uint32_t s0 = 0u, s1 = 0u, s2 = 0u, s3 = 0u;
    for (int f = 0; f < batch; ++f) {
        const uint32_t va = a[(long long)f * pixels + px], vb = b[(long long)f * pixels + px];
        s0 += va;
        s1 += va * va;
        s2 += vb;
        s3 += vb * vb;
    }
    mom[px] += (long long)s0;
    mom[pixels + px] += (long long)s1;
    mom[2 * pixels + px] += (long long)s2;
    mom[3 * pixels + px] += (long long)s3;
}

template <int R>
hipError_t launch_add_r(const PixelAddParams& p, int groups, hipStream_t stream) {
    hipLaunchKernelGGL(pixel_corr_add_kernel<R>, dim3((unsigned)groups), dim3(kThreads), 0, stream, p);
    return hipGetLastError();
}

// ---- peaks ------------------------------------------------------------------------------------------------------------

struct PixelPeakParams {
    const long long* acc;
    const long long* mom;
    double *u, *v, *peak, *ratio, *corr;
    uint8_t* status;
    int n_pairs, H, W, ky, kx, R, sy, sx, nby, nbx;
};

constexpr int kMaxD = 2 * kPixelCorrMaxRadius + 1;

__global__ __launch_bounds__(64) void pixel_corr_peaks_kernel(PixelPeakParams p) {
#pragma clang fp contract(off)
    __shared__ double sC[kMaxD * kMaxD];
    __shared__ double rv[64];
    __shared__ long long rl[64];
    __shared__ int ri[64];
    const int lane = threadIdx.x;
    const long long bin = blockIdx.x;
    const int br = (int)(bin / p.nbx), bc = (int)(bin % p.nbx);
    const int D = 2 * p.R + 1, DD = D * D, npx = p.ky * p.kx;
    const int y0 = br * p.ky, x0 = bc * p.kx;
    const long long pixels = (long long)p.H * p.W;
    const long long* __restrict__ m0 = p.mom;
    const long long* __restrict__ m1 = p.mom + pixels;
    const long long* __restrict__ m2 = p.mom + 2 * pixels;
    const long long* __restrict__ m3 = p.mom + 3 * pixels;
    const long long N = p.n_pairs;
    const double nan = __builtin_nan("");
    double* corr = p.corr ? p.corr + bin * DD : nullptr;

    int status = 0;
    if (y0 + p.sy - p.R < 0 || y0 + p.ky - 1 + p.sy + p.R > p.H - 1 || x0 + p.sx - p.R < 0 ||
        x0 + p.kx - 1 + p.sx + p.R > p.W - 1)
        status = 1;
    if (!status) {
        // exact int64 numerators; every one below 2^57 (include/torchpiv_hip.h): N acc <= 2^16 (2^16 2^8 255^2) < 2^56 and
        // the sum of 256 products of two moments <= 2^8 (2^16 255)^2 < 2^56, squares alike
        long long part = 0;
        for (int k = lane; k < npx; k += 64) {
            const long long o = (long long)(y0 + k / p.kx) * p.W + x0 + k % p.kx;
            part += N * m1[o] - m0[o] * m0[o];
        }
        rl[lane] = part;
        __syncthreads();
        long long va = 0;
        for (int k = 0; k < 64; ++k) va += rl[k];
        int flat = va == 0;
        for (int d = lane; d < DD; d += 64) {
            const int dy = p.sy + d / D - p.R, dx = p.sx + d % D - p.R;
            long long cross = 0, vb = 0;
            for (int k = 0; k < npx; ++k) {
                const int y = y0 + k / p.kx, x = x0 + k % p.kx;
                const long long o = (long long)y * p.W + x, ob = (long long)(y + dy) * p.W + x + dx;
                cross += m0[o] * m2[ob];
                vb += N * m3[ob] - m2[ob] * m2[ob];
            }
            const long long num = N * p.acc[bin * DD + d] - cross;
            flat |= vb == 0;
            const double prod = (double)va * (double)vb;
            sC[d] = (double)num / sqrt(prod);
        }
        ri[lane] = flat;
        __syncthreads();
        for (int k = 0; k < 64; ++k) flat |= ri[k];
        if (flat) status = 2;
        __syncthreads();
    }
    if (status == 1 || status == 2) {
        if (corr)
            for (int d = lane; d < DD; d += 64) corr[d] = 0.0;
        if (lane == 0) {
            p.u[bin] = p.v[bin] = p.peak[bin] = p.ratio[bin] = nan;
            p.status[bin] = (uint8_t)status;
        }
        return;
    }
    if (corr)
        for (int d = lane; d < DD; d += 64) corr[d] = sC[d];
    // min C, then the first arg-max of M = (C - min C) + 1e-7 in raster order
    double lo = sC[lane < DD ? lane : 0];
    for (int d = lane; d < DD; d += 64) lo = sC[d] < lo ? sC[d] : lo;
    rv[lane] = lo;
    __syncthreads();
    for (int k = 0; k < 64; ++k) lo = rv[k] < lo ? rv[k] : lo;
    __syncthreads();
    double best = -1.0;
    int at = DD;
    for (int d = lane; d < DD; d += 64) {
        const double m = (sC[d] - lo) + 1e-7;
        if (m > best) {
            best = m;
            at = d;
        }
    }
    rv[lane] = best;
    ri[lane] = at;
    __syncthreads();
    for (int k = 0; k < 64; ++k)
        if (rv[k] > best || (rv[k] == best && ri[k] < at)) {
            best = rv[k];
            at = ri[k];
        }
    __syncthreads();
    const int pj = at / D, pi = at % D;
    double u = nan, v = nan, peak = nan, ratio = nan;
    if (pj == 0 || pj == D - 1 || pi == 0 || pi == D - 1) {
        status = 3;
    } else {
        const double lm = log(best);
        const double lxp = log((sC[at + 1] - lo) + 1e-7), lxm = log((sC[at - 1] - lo) + 1e-7);
        const double lyp = log((sC[at + D] - lo) + 1e-7), lym = log((sC[at - D] - lo) + 1e-7);
        const double ddx = (lxm - lxp) / (2.0 * (lxp + lxm) - 4.0 * lm);
        const double ddy = (lym - lyp) / (2.0 * (lyp + lym) - 4.0 * lm);
        if (!(fabs(ddx) <= 1.0) || !(fabs(ddy) <= 1.0)) {        // (a NaN fails the comparison)
            status = 4;
        } else {
            double second = 0.0;                                       // M >= 1e-7 > 0 everywhere
            for (int d = lane; d < DD; d += 64) {
                const int j = d / D, i = d % D;
                if (j >= pj - 2 && j <= pj + 2 && i >= pi - 2 && i <= pi + 2) continue;
                const double m = (sC[d] - lo) + 1e-7;
                second = m > second ? m : second;
            }
            rv[lane] = second;
            __syncthreads();
            for (int k = 0; k < 64; ++k) second = rv[k] > second ? rv[k] : second;
            u = (double)(p.sx + pi - p.R) + ddx;
            v = (double)(p.sy + pj - p.R) + ddy;
            peak = sC[at];
            ratio = best / second;
        }
    }
    if (lane == 0) {
        p.u[bin] = u;
        p.v[bin] = v;
        p.peak[bin] = peak;
        p.ratio[bin] = ratio;
        p.status[bin] = (uint8_t)status;
    }
}

}  // namespace

hipError_t launch_pixel_corr_add(const uint8_t* a, const uint8_t* b, int batch, int H, int W, int ky, int kx, int radius,
                                 int sy, int sx, long long* acc, long long* mom, hipStream_t stream) {
    if (batch <= 0) return hipSuccess;
    const long long pixels = (long long)H * W;
    const long long mblocks = (pixels + kThreads - 1) / kThreads;
    if (mblocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pixel_corr_mom_kernel, dim3((unsigned)mblocks), dim3(kThreads), 0, stream, a, b, batch, pixels, mom);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;

    PixelAddParams p{};
    p.a = a;
    p.b = b;
    p.acc = acc;
    p.batch = batch;
    p.H = H;
    p.W = W;
    p.ky = ky;
    p.kx = kx;
    p.sy = sy;
    p.sx = sx;
    p.nby = H / ky;
    p.nbx = W / kx;
    p.gby = ky >= kTH ? 1 : kTH / ky;
    p.gbx = kx >= kTW ? 1 : kTW / kx;
    p.ngx = (p.nbx + p.gbx - 1) / p.gbx;
    const long long groups = (long long)p.ngx * ((p.nby + p.gby - 1) / p.gby);
    if (groups > 0x7fffffffLL) return hipErrorInvalidValue;
    p.vec = W % 4 == 0 && ((uintptr_t)a & 3u) == 0 && ((uintptr_t)b & 3u) == 0;
    switch (radius) {
#define TPIV_PIXEL_R(R) case R: return launch_add_r<R>(p, (int)groups, stream);
        TPIV_PIXEL_R(3) TPIV_PIXEL_R(4) TPIV_PIXEL_R(5) TPIV_PIXEL_R(6) TPIV_PIXEL_R(7) TPIV_PIXEL_R(8) TPIV_PIXEL_R(9)
        TPIV_PIXEL_R(10) TPIV_PIXEL_R(11) TPIV_PIXEL_R(12) TPIV_PIXEL_R(13) TPIV_PIXEL_R(14) TPIV_PIXEL_R(15) TPIV_PIXEL_R(16)
#undef TPIV_PIXEL_R
    }
    return hipErrorInvalidValue;
}

hipError_t launch_pixel_corr_peaks(const long long* acc, const long long* mom, int n_pairs, int H, int W, int ky, int kx,
                                   int radius, int sy, int sx, double* u, double* v, double* peak, double* ratio,
                                   uint8_t* status, double* corr, hipStream_t stream) {
    PixelPeakParams p{};
    p.acc = acc;
    p.mom = mom;
    p.u = u;
    p.v = v;
    p.peak = peak;
    p.ratio = ratio;
    p.corr = corr;
    p.status = status;
    p.n_pairs = n_pairs;
    p.H = H;
    p.W = W;
    p.ky = ky;
    p.kx = kx;
    p.R = radius;
    p.sy = sy;
    p.sx = sx;
    p.nby = H / ky;
    p.nbx = W / kx;
    const long long bins = (long long)p.nby * p.nbx;
    if (bins <= 0) return hipSuccess;
    if (bins > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pixel_corr_peaks_kernel, dim3((unsigned)bins), dim3(64), 0, stream, p);
    return hipGetLastError();
}

}  // namespace tpiv
