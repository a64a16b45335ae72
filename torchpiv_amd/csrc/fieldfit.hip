// Local least-squares polynomial fit of a batch of vector fields: the denoised vector and its first derivatives per
// cell, from the (2 radius + 1)^2 neighbourhood with the missing vectors left out (include/torchpiv_hip.h:
// tpiv_field_fit has the definition and the operation order).
//
// One lane per cell, one workgroup per kTC x kTR tile.  The tile and its `radius` halo are staged in LDS once, with
// the skip bytes and the finiteness test already folded in: a cell that is not data, or lies outside the grid, is
// staged as the one NaN pattern kNoData in both components, so the neighbour loop reads validity and value from the
// same word.  The body is a template of radius and order: the neighbour loop and the elimination unroll over
// compile-time offsets and indices, every array below is indexed by constants only, and nothing lives in scratch.
// The moments of the offsets are small integers and are summed as such; every floating-point operation is one IEEE
// float64 operation, contraction is off for this unit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "piv_kernels.h"

#pragma clang fp contract(off)

namespace tpiv {

namespace {

constexpr int kTC = FIELDFIT_TILE_COLS, kTR = FIELDFIT_TILE_ROWS;
constexpr int kThreads = kTC * kTR;
static_assert(kTC == 64 && kThreads <= 1024, "a wavefront per tile row");

constexpr long long kNoData = 0x7ff8000000000000LL;   // staged for what is not data; also the NaN written out
constexpr long long kExpMask = 0x7ff0000000000000LL;
constexpr double kPivotTol = 1.0 / 1073741824.0;      // 2^-30

__device__ __forceinline__ bool is_finite(double x) { return (__double_as_longlong(x) & kExpMask) != kExpMask; }

// the basis 1, i, j, i^2, i j, j^2 as exponents of (i, j)
__device__ __forceinline__ constexpr int exp_i(int q) { return q == 1 ? 1 : q == 3 ? 2 : q == 4 ? 1 : 0; }
__device__ __forceinline__ constexpr int exp_j(int q) { return q == 2 ? 1 : q == 4 ? 1 : q == 5 ? 2 : 0; }
__device__ __forceinline__ constexpr int ipow(int x, int e) {
    int r = 1;
    for (int k = 0; k < e; ++k) r *= x;
    return r;
}

template <int R, int ORD>
__global__ __launch_bounds__(kThreads) void field_fit_kernel(FieldFitParams p) {
    constexpr int kPitch = kTC + 2 * R, kRows = kTR + 2 * R, kCells = kPitch * kRows;
    constexpr int N = ORD == 2 ? 6 : 3;               // unknowns
    constexpr int D = 2 * ORD;                        // highest total degree among the moments
    __shared__ double su[kCells], sv[kCells];
    const int tid = threadIdx.x, tx = tid % kTC, ty = tid / kTC;
    const int c0 = blockIdx.x * kTC, r0 = blockIdx.y * kTR;
    const size_t cells = (size_t)p.n_rows * p.n_cols;
    const size_t field = (size_t)blockIdx.z * cells;
    const double nan = __longlong_as_double(kNoData);

    for (int s = tid; s < kCells; s += kThreads) {
        const int hr = s / kPitch, hc = s - hr * kPitch;
        const int gr = r0 - R + hr, gc = c0 - R + hc;
        double uh = nan, vh = nan;
        if (gr >= 0 && gr < p.n_rows && gc >= 0 && gc < p.n_cols) {
            const size_t g = field + (size_t)gr * p.n_cols + gc;
            const double ug = p.u[g], vg = p.v[g];
            const bool ok = (p.skip == nullptr || p.skip[g] == 0) && is_finite(ug) && is_finite(vg);
            uh = ok ? ug : nan;
            vh = ok ? vg : nan;
        }
        su[s] = uh;
        sv[s] = vh;
    }
    __syncthreads();
    const int r = r0 + ty, c = c0 + tx;
    if (r >= p.n_rows || c >= p.n_cols) return;
    const int at = (ty + R) * kPitch + tx + R;

    // the moments sum i^a j^b over the data cells (int32) and the right-hand sides sum w i^a j^b (float64), the
    // neighbours in row-major order.  A term whose factor i^a j^b is 0 is left out: the sums start at +0.0 and a sum
    // of this kind is never -0.0, so adding w * 0 = +-0.0 would leave its bits as they are.
    int mom[D + 1][D + 1];
    double bu[N], bv[N];
#pragma unroll
    for (int a = 0; a <= D; ++a)
#pragma unroll
        for (int b = 0; b <= D; ++b) mom[a][b] = 0;
#pragma unroll
    for (int q = 0; q < N; ++q) bu[q] = bv[q] = 0.0;
#pragma unroll
    for (int j = -R; j <= R; ++j) {
#pragma unroll
        for (int i = -R; i <= R; ++i) {
            const double wu = su[at + j * kPitch + i], wv = sv[at + j * kPitch + i];
            const bool ok = __double_as_longlong(wu) != kNoData;
#pragma unroll
            for (int a = 0; a <= D; ++a)
#pragma unroll
                for (int b = 0; a + b <= D; ++b) {
                    const int f = ipow(i, a) * ipow(j, b);
                    if (f != 0) mom[a][b] += ok ? f : 0;
                }
#pragma unroll
            for (int q = 0; q < N; ++q) {
                const int f = ipow(i, exp_i(q)) * ipow(j, exp_j(q));
                if (f != 0) {
                    const double tu = wu * (double)f, tv = wv * (double)f;
                    bu[q] = ok ? bu[q] + tu : bu[q];
                    bv[q] = ok ? bv[q] + tv : bv[q];
                }
            }
        }
    }
    const int count = mom[0][0];
    const double sum_u = bu[0], sum_v = bv[0];

    // LDL^T of the normal matrix without pivoting (lower triangle; the right-hand sides ride along), then the pivot test
    double A[N][N], L[N][N], d[N], m0[N];
#pragma unroll
    for (int q = 0; q < N; ++q)
#pragma unroll
        for (int s = 0; s <= q; ++s) A[q][s] = (double)mom[exp_i(q) + exp_i(s)][exp_j(q) + exp_j(s)];
#pragma unroll
    for (int q = 0; q < N; ++q) m0[q] = A[q][q];
    bool acc = true, acc3 = false, acc6 = false;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        d[k] = A[k][k];
        acc = acc && (d[k] > kPivotTol * m0[k]);
        if (k == 2) acc3 = acc;
        if (k == 5) acc6 = acc;
#pragma unroll
        for (int q = k + 1; q < N; ++q) {
            const double l = A[q][k] / d[k];
#pragma unroll
            for (int s = k + 1; s <= q; ++s) A[q][s] = A[q][s] - l * A[s][k];
            bu[q] = bu[q] - l * bu[k];
            bv[q] = bv[q] - l * bv[k];
            L[q][k] = l;
        }
    }
    double yu[N], yv[N];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        yu[k] = bu[k] / d[k];
        yv[k] = bv[k] / d[k];
    }
    // back substitution over the leading 3 x 3 block (the linear fit) and, at order 2, over all six unknowns
    double lu[3], lv[3];
#pragma unroll
    for (int k = 2; k >= 0; --k) {
        double tu = yu[k], tv = yv[k];
#pragma unroll
        for (int q = k + 1; q < 3; ++q) {
            tu = tu - L[q][k] * lu[q];
            tv = tv - L[q][k] * lv[q];
        }
        lu[k] = tu;
        lv[k] = tv;
    }
    double o0u = lu[0], o1u = lu[1], o2u = lu[2], o0v = lv[0], o1v = lv[1], o2v = lv[2];
    int order = acc3 ? 1 : (count >= 1 ? 0 : -1);
    if (ORD == 2) {
        double qu[N], qv[N];
#pragma unroll
        for (int k = N - 1; k >= 0; --k) {
            double tu = yu[k], tv = yv[k];
#pragma unroll
            for (int q = k + 1; q < N; ++q) {
                tu = tu - L[q][k] * qu[q];
                tv = tv - L[q][k] * qv[q];
            }
            qu[k] = tu;
            qv[k] = tv;
        }
        o0u = acc6 ? qu[0] : o0u;
        o1u = acc6 ? qu[1] : o1u;
        o2u = acc6 ? qu[2] : o2u;
        o0v = acc6 ? qv[0] : o0v;
        o1v = acc6 ? qv[1] : o1v;
        o2v = acc6 ? qv[2] : o2v;
        order = acc6 ? 2 : order;
    }
    if (order <= 0) {
        const double n = (double)count;
        o0u = order == 0 ? sum_u / n : nan;
        o0v = order == 0 ? sum_v / n : nan;
        o1u = o2u = o1v = o2v = nan;
    }
    const size_t cell = field + (size_t)r * p.n_cols + c, plane = (size_t)p.batch * cells;
    p.fit[cell] = o0u;
    p.fit[plane + cell] = o1u;
    p.fit[2 * plane + cell] = o2u;
    p.fit[3 * plane + cell] = o0v;
    p.fit[4 * plane + cell] = o1v;
    p.fit[5 * plane + cell] = o2v;
    p.count[cell] = (uint8_t)count;
    p.order[cell] = (int8_t)order;
}

template <int R>
void launch_order(const FieldFitParams& p, dim3 grid, hipStream_t stream) {
    if (p.order_max == 2)
        hipLaunchKernelGGL((field_fit_kernel<R, 2>), grid, dim3(kThreads), 0, stream, p);
    else
        hipLaunchKernelGGL((field_fit_kernel<R, 1>), grid, dim3(kThreads), 0, stream, p);
}

}  // namespace

hipError_t launch_field_fit(const FieldFitParams& p, hipStream_t stream) {
    if (p.batch <= 0) return hipSuccess;
    if (p.radius < 1 || p.radius > 3 || p.order_max < 1 || p.order_max > 2) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((p.n_cols + kTC - 1) / kTC), (unsigned)((p.n_rows + kTR - 1) / kTR), (unsigned)p.batch);
    if (grid.y > 65535u || grid.z > 65535u) return hipErrorInvalidValue;
    if (p.radius == 1) launch_order<1>(p, grid, stream);
    if (p.radius == 2) launch_order<2>(p, grid, stream);
    if (p.radius == 3) launch_order<3>(p, grid, stream);
    return hipGetLastError();
}

}  // namespace tpiv
