// Correlation-statistics uncertainty (Wieneke, Meas. Sci. Technol. 26 (2015) 074002) of a batch of vector fields: the
// a-posteriori 1-sigma estimate of each vector's random error (include/torchpiv_hip.h: tpiv_uncertainty,
// tpiv_plan_set_uncertainty).
//
// One workgroup per window.  It samples the window's two half-shifted patches (ws + 2R + 1 pixels a side, Q8 bilinear,
// edge replicate) straight from the uint8 frames into LDS as int16, takes the core means off, and then runs the two
// components one after the other: the per-pixel asymmetry contributions d of the component go to LDS as int32 once, and
// every lane walks strips of four adjacent core pixels, reading each row segment of d it needs once (16-byte pieces) and
// accumulating d * d' over all lags of the half plane in its own 64-bit integer accumulators (a 32 x 32 -> 64 bit
// multiply-add each).  Nothing crosses lanes before the strips are done; then one shuffle reduction per wavefront, one
// LDS trip per workgroup, and lane 0 counts the lags and runs the float64 epilogue.
//
// Every sum is an exact integer: |a'|, |b'| <= 1020, |d| < 2^21, d * d' < 2^42, a sum over at most 128^2 core pixels
// < 2^56, var <= 81 * 2^56 < 2^63.  The epilogue is one IEEE float64 operation per step; contraction is off for this unit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "piv_kernels.h"

#pragma clang fp contract(off)

namespace tpiv {

namespace {

constexpr int kMaxThreads = 256;
constexpr int kStrip = 4;                                  // adjacent core pixels a lane takes at a time

__host__ __device__ constexpr int round4(int x) { return (x + 3) & ~3; }
// row pitch of d in LDS: the strips of a row and the lag margin behind the last one, in whole 16-byte pieces
__host__ __device__ constexpr int d_pitch(int ws, int R) { return round4(ws) + round4(2 * R); }
// accumulators of a component: S(0, 0..R), then S(k, -R..R) for k = 1..R
__host__ __device__ constexpr int n_acc(int R) { return R + 1 + R * (2 * R + 1); }

struct Layout {
    int P, pitch, patch16, d_words;                        // patch16: int16 elements of one patch, padded to 16 bytes
    size_t bytes;
};
__host__ __device__ inline Layout layout(int ws, int R) {
    Layout l;
    l.P = ws + 2 * R + 1;
    l.pitch = d_pitch(ws, R);
    l.patch16 = (l.P * l.P + 7) & ~7;
    l.d_words = (ws + 2 * R) * l.pitch;
    l.bytes = (size_t)l.patch16 * 2 * 2 + (size_t)l.d_words * 4 + (size_t)(kMaxThreads / 64) * (n_acc(R) + 2) * 8;
    return l;
}

// Q8 half shift: clamp(rint(u * 128), -32767, 32767); the product is exact, rint rounds ties to even
__device__ __forceinline__ int half_shift_q8(double u) { return (int)fmin(fmax(rint(u * 128.0), -32767.0), 32767.0); }

// frame sampled at (qy, qx) in Q8: the four taps clamped to the frame, weights (256 - f, f), rounded to Q2 grey levels
__device__ __forceinline__ int sample_q8(const uint8_t* __restrict__ f, int H, int W, int qy, int qx) {
    const int iy = qy >> 8, fy = qy & 255, ix = qx >> 8, fx = qx & 255;
    const int r0 = min(max(iy, 0), H - 1), r1 = min(max(iy + 1, 0), H - 1);
    const int c0 = min(max(ix, 0), W - 1), c1 = min(max(ix + 1, 0), W - 1);
    const uint8_t* __restrict__ p0 = f + (size_t)r0 * W;
    const uint8_t* __restrict__ p1 = f + (size_t)r1 * W;
    const int top = (256 - fx) * p0[c0] + fx * p0[c1], bot = (256 - fx) * p1[c0] + fx * p1[c1];
    return ((256 - fy) * top + fy * bot + 8192) >> 14;
}

__device__ __forceinline__ long long wave_sum(long long x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
    return x;
}

// the closing three-point Gaussian propagation; NaN where the peak is not one
__device__ __forceinline__ double sigma_of(long long C0, long long S2, long long var) {
    const double sd = __dsqrt_rn((double)var), s2 = (double)S2, c0 = (double)C0;
    const double cp = (s2 + sd) * 0.5, cm = (s2 - sd) * 0.5;
    if (C0 <= 0 || !(cm > 0) || !(c0 * c0 > cp * cm)) return __longlong_as_double(0x7ff8000000000000LL);
    const double lp = log(cp), lm = log(cm), l0 = log(c0);
    return (lp - lm) / (4.0 * l0 - 2.0 * lm - 2.0 * lp);
}

template <int R>
__global__ __launch_bounds__(kMaxThreads) void uncertainty_kernel(UncertaintyParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char unc_smem[];
    constexpr int NA = n_acc(R), NR = NA + 2;              // reduced per component: the accumulators, S2, C0
    constexpr int SEG = kStrip + round4(2 * R);            // d values a strip reads of one row
    const Layout L = layout(p.ws, R);
    int16_t* const sA = reinterpret_cast<int16_t*>(unc_smem);
    int16_t* const sB = sA + L.patch16;
    int32_t* const sD = reinterpret_cast<int32_t*>(sB + L.patch16);
    long long* const red = reinterpret_cast<long long*>(sD + L.d_words);

    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    const int ws = p.ws, P = L.P, pitch = L.pitch, H = p.H, W = p.W;
    const int cells = p.n_rows * p.n_cols;
    const size_t item = blockIdx.x;                        // batch * cells < 2^31 (checked by the launcher)
    const int pair = (int)(item / cells), cell = (int)(item % cells);
    const int st = ws - p.ov, y0 = (cell / p.n_cols) * st, x0 = (cell % p.n_cols) * st;

    // (uniform over the workgroup: every lane reads the same three values)
    const double u = p.u[item], v = p.v[item];
    const bool off = (p.invalid && p.invalid[item] != 0) || (p.exclude && p.exclude[(size_t)pair * p.exclude_stride + cell] != 0) ||
                     !(fabs(u) < __longlong_as_double(0x7ff0000000000000LL)) ||
                     !(fabs(v) < __longlong_as_double(0x7ff0000000000000LL));
    if (off) {
        if (tid == 0) {
            p.su[item] = p.sv[item] = __longlong_as_double(0x7ff8000000000000LL);
            if (p.stats)
                for (int k = 0; k < 8; ++k) p.stats[item * 8 + k] = 0;
        }
        return;
    }
    const int hx = half_shift_q8(u), hy = half_shift_q8(v);
    const uint8_t* __restrict__ fa = p.A + (size_t)pair * H * W;
    const uint8_t* __restrict__ fb = p.B + (size_t)pair * H * W;

    // the two patches, raw, and the core sums
    int sum_a = 0, sum_b = 0;                              // <= 1020 per pixel, <= 74 pixels per lane at P = 137
    for (int e = tid; e < P * P; e += nt) {
        const int i = e / P - R, j = e % P - R;
        const int qy = (y0 + i) * 256, qx = (x0 + j) * 256;
        const int va = sample_q8(fa, H, W, qy - hy, qx - hx), vb = sample_q8(fb, H, W, qy + hy, qx + hx);
        sA[e] = (int16_t)va;
        sB[e] = (int16_t)vb;
        const bool core = i >= 0 && i < ws && j >= 0 && j < ws;
        sum_a += core ? va : 0;
        sum_b += core ? vb : 0;
    }
    {
        const long long wa = wave_sum(sum_a), wb = wave_sum(sum_b);
        if (lane == 0) {
            red[2 * wave] = wa;
            red[2 * wave + 1] = wb;
        }
    }
    __syncthreads();
    int ma = 0, mb = 0;
    {
        long long ta = 0, tb = 0;
        for (int w = 0; w < nw; ++w) {
            ta += red[2 * w];
            tb += red[2 * w + 1];
        }
        const int N = ws * ws;
        ma = (int)((ta + N / 2) / N);
        mb = (int)((tb + N / 2) / N);
    }
    // (a lane takes the means off the elements it wrote itself)
    for (int e = tid; e < P * P; e += nt) {
        sA[e] = (int16_t)(sA[e] - ma);
        sB[e] = (int16_t)(sB[e] - mb);
    }
    __syncthreads();                                       // the patches are complete; red is free again

    long long C0 = 0, out_S2[2] = {0, 0}, out_S00[2] = {0, 0}, out_var[2] = {0, 0};
    int out_n[2] = {0, 0};
    const int rows_d = ws + 2 * R, strips_row = (ws + kStrip - 1) / kStrip, strips = ws * strips_row;
#pragma unroll 1
    for (int comp = 0; comp < 2; ++comp) {
        // d of this component for -R <= i, j <= ws - 1 + R, zero in the padding of a row; S2 and C0 over the core
        const int nb = comp == 0 ? 1 : P;                  // the neighbour: [i][j + 1] or [i + 1][j]
        long long s2 = 0, c0 = 0;
        for (int e = tid; e < rows_d * pitch; e += nt) {
            const int i = e / pitch, j = e % pitch;
            int d = 0;
            if (j < rows_d) {
                const int at = i * P + j;
                const int a0 = sA[at], b0 = sB[at], a1 = sA[at + nb], b1 = sB[at + nb];
                d = a0 * b1 - a1 * b0;
                if (i >= R && i < R + ws && j >= R && j < R + ws) {
                    s2 += a0 * b1 + a1 * b0;
                    c0 += a0 * b0;
                }
            }
            sD[e] = d;
        }
        __syncthreads();

        long long acc[NA];
#pragma unroll
        for (int n = 0; n < NA; ++n) acc[n] = 0;
        for (int s = tid; s < strips; s += nt) {
            const int i = s / strips_row, j0 = (s % strips_row) * kStrip;
            int d0[kStrip];
#pragma unroll
            for (int t = 0; t < kStrip; ++t) d0[t] = j0 + t < ws ? sD[(i + R) * pitch + j0 + R + t] : 0;
#pragma unroll
            for (int k = 0; k <= R; ++k) {
                int seg[SEG];
                const int4* __restrict__ row = reinterpret_cast<const int4*>(sD + (i + R + k) * pitch + j0);
#pragma unroll
                for (int q = 0; q < SEG / 4; ++q) {
                    const int4 x = row[q];
                    seg[4 * q] = x.x;
                    seg[4 * q + 1] = x.y;
                    seg[4 * q + 2] = x.z;
                    seg[4 * q + 3] = x.w;
                }
#pragma unroll
                for (int l = (k == 0 ? 0 : -R); l <= R; ++l) {
                    const int n = k == 0 ? l : R + 1 + (k - 1) * (2 * R + 1) + (l + R);
#pragma unroll
                    for (int t = 0; t < kStrip; ++t) acc[n] += (long long)d0[t] * (long long)seg[t + R + l];
                }
            }
        }
        // one reduction per wavefront, one LDS trip per workgroup
#pragma unroll
        for (int n = 0; n < NA; ++n) acc[n] = wave_sum(acc[n]);
        s2 = wave_sum(s2);
        c0 = wave_sum(c0);
        if (lane == 0) {
#pragma unroll
            for (int n = 0; n < NA; ++n) red[wave * NR + n] = acc[n];
            red[wave * NR + NA] = s2;
            red[wave * NR + NA + 1] = c0;
        }
        __syncthreads();                                   // (also: every strip is done before d is rebuilt)
        if (tid == 0) {
            auto total = [&](int n) {
                long long t = 0;
                for (int w = 0; w < nw; ++w) t += red[w * NR + n];
                return t;
            };
            const long long S00 = total(0);
            long long var = S00;
            int cnt = 0;
            for (int n = 1; n < NA; ++n) {
                const long long S = total(n);
                if (20 * S > S00) {                        // Wieneke's 5 % cut, in integers
                    var += 2 * S;
                    ++cnt;
                }
            }
            out_S2[comp] = total(NA);
            out_S00[comp] = S00;
            out_var[comp] = var;
            out_n[comp] = cnt;
            C0 = total(NA + 1);
        }
        __syncthreads();                                   // red is read before the next component writes it
    }
    if (tid == 0) {
        p.su[item] = sigma_of(C0, out_S2[0], out_var[0]);
        p.sv[item] = sigma_of(C0, out_S2[1], out_var[1]);
        if (p.stats) {
            long long* __restrict__ o = p.stats + item * 8;
            o[0] = C0;
            o[1] = out_S2[0];
            o[2] = out_S00[0];
            o[3] = out_var[0];
            o[4] = out_S2[1];
            o[5] = out_S00[1];
            o[6] = out_var[1];
            o[7] = out_n[0] + 256 * out_n[1];
        }
    }
}

template <int R>
hipError_t launch_r(const UncertaintyParams& p, unsigned blocks, int threads, hipStream_t stream) {
    const size_t smem = layout(p.ws, R).bytes;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&uncertainty_kernel<R>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(uncertainty_kernel<R>, dim3(blocks), dim3(threads), smem, stream, p);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_uncertainty(const UncertaintyParams& p, hipStream_t stream) {
    if (p.batch <= 0) return hipSuccess;
    const long long items = (long long)p.batch * p.n_rows * p.n_cols;
    if (items >= (1LL << 31) || p.ws < UNCERTAINTY_MIN_WS || p.ws > UNCERTAINTY_MAX_WS || p.radius < 0 ||
        p.radius > UNCERTAINTY_MAX_RADIUS)
        return hipErrorInvalidValue;
    // a lane per strip of four core pixels: one wavefront covers a 16 x 16 window, four a 32 x 32 one
    const int strips = p.ws * ((p.ws + kStrip - 1) / kStrip);
    const int threads = strips <= 64 ? 64 : (strips <= 128 ? 128 : 256);
    switch (p.radius) {
        case 0: return launch_r<0>(p, (unsigned)items, threads, stream);
        case 1: return launch_r<1>(p, (unsigned)items, threads, stream);
        case 2: return launch_r<2>(p, (unsigned)items, threads, stream);
        case 3: return launch_r<3>(p, (unsigned)items, threads, stream);
        default: return launch_r<4>(p, (unsigned)items, threads, stream);
    }
}

}  // namespace tpiv
