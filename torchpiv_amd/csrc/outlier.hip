// Normalized median test (Westerweel & Scarano, Exp. Fluids 39, 2005) on a batch of vector fields: the spatial
// validation between and after the passes (include/torchpiv_hip.h: tpiv_median_test, tpiv_plan_set_outlier).
//
// One lane per cell, one workgroup per kTC x kTR tile.  The tile and its one-cell halo are staged in LDS once, with
// the mask already folded in: an invalid or out-of-grid cell is staged as +inf, so the eight neighbours a lane reads
// back are the inputs of the sorting network as they stand, and every mask byte of a row segment is read from memory
// once (by the lane that stages the cell).  A lane keeps its own cell's raw u, v and mask byte in registers.
//
// Order.  Values are sorted as the integers sort_key() maps them to: the order of `<` on finite doubles with -0.0
// before +0.0 (so that ties leave no choice: the picked median is one bit pattern) and +inf above every finite value.
// Residuals are >= 0, where the bit pattern itself is that key.  The two order statistics are picked by the number of
// valid neighbours with select chains over the network's named outputs -- nothing is indexed at run time, so nothing
// lives in scratch.  Every arithmetic operation is one IEEE float64 operation; contraction is off for this unit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "piv_kernels.h"

#pragma clang fp contract(off)

namespace tpiv {

namespace {

constexpr int kTC = OUTLIER_TILE_COLS, kTR = OUTLIER_TILE_ROWS;
constexpr int kThreads = kTC * kTR;
constexpr int kPitch = kTC + 2;                       // halo tile: (kTR + 2) rows of kTC + 2 cells
constexpr int kRing = 2 * kPitch + 2 * kTR;           // halo cells around the tile
static_assert(kTC == 64 && kThreads <= 1024 && kRing <= kThreads, "a wavefront per tile row; the ring is staged in one step");

constexpr long long kInfBits = 0x7ff0000000000000LL;

// involution: double bits <-> a signed integer that orders like the value (-0.0 below +0.0)
__device__ __forceinline__ long long sort_key(long long bits) { return bits ^ ((bits >> 63) & 0x7fffffffffffffffLL); }

__device__ __forceinline__ void cswap(long long& a, long long& b) {
    const bool s = b < a;
    const long long lo = s ? b : a, hi = s ? a : b;
    a = lo;
    b = hi;
}

// 19 compare-exchanges, ascending.  (Eight named values, not an array: over an array the compiler turns the picks below
// back into a run-time index, and the array into scratch.)
struct Eight {
    long long x0, x1, x2, x3, x4, x5, x6, x7;
};

__device__ __forceinline__ void sort8(Eight& e) {
    cswap(e.x0, e.x1); cswap(e.x2, e.x3); cswap(e.x4, e.x5); cswap(e.x6, e.x7);
    cswap(e.x0, e.x2); cswap(e.x1, e.x3); cswap(e.x4, e.x6); cswap(e.x5, e.x7);
    cswap(e.x1, e.x2); cswap(e.x5, e.x6); cswap(e.x0, e.x4); cswap(e.x3, e.x7);
    cswap(e.x1, e.x5); cswap(e.x2, e.x6);
    cswap(e.x1, e.x4); cswap(e.x3, e.x6);
    cswap(e.x2, e.x4); cswap(e.x3, e.x5);
    cswap(e.x3, e.x4);
}

// the median of the k smallest of sorted values s0 <= ... <= s4 <= ... (1 <= k <= 8): s[(k-1)/2] for odd k,
// (s[k/2-1] + s[k/2]) * 0.5 for even k; the two are picked bit by bit of their index
__device__ __forceinline__ double pick_median(double s0, double s1, double s2, double s3, double s4, int k) {
    const int j = (k - 1) >> 1, h = k >> 1;           // j in 0..3, h in 0..4
    const double lo01 = (j & 1) ? s1 : s0, lo23 = (j & 1) ? s3 : s2;
    const double lo = (j & 2) ? lo23 : lo01;
    const double hi01 = (h & 1) ? s1 : s0, hi23 = (h & 1) ? s3 : s2;
    const double hi03 = (h & 2) ? hi23 : hi01;
    const double hi = (h & 4) ? s4 : hi03;
    return (k & 1) ? lo : (lo + hi) * 0.5;
}

__device__ __forceinline__ double key_value(long long key) { return __longlong_as_double(sort_key(key)); }
__device__ __forceinline__ long long residual(double s, double med) { return __double_as_longlong(fabs(s - med)); }

// one component: the neighbourhood median and whether the centre lies outside threshold * (median residual + eps)
__device__ __forceinline__ bool component(const double* __restrict__ t, int at, int k, double centre, double threshold,
                                          double eps, double& med) {
    Eight e;
    e.x0 = sort_key(__double_as_longlong(t[at - kPitch - 1]));
    e.x1 = sort_key(__double_as_longlong(t[at - kPitch]));
    e.x2 = sort_key(__double_as_longlong(t[at - kPitch + 1]));
    e.x3 = sort_key(__double_as_longlong(t[at - 1]));
    e.x4 = sort_key(__double_as_longlong(t[at + 1]));
    e.x5 = sort_key(__double_as_longlong(t[at + kPitch - 1]));
    e.x6 = sort_key(__double_as_longlong(t[at + kPitch]));
    e.x7 = sort_key(__double_as_longlong(t[at + kPitch + 1]));
    sort8(e);
    const double s0 = key_value(e.x0), s1 = key_value(e.x1), s2 = key_value(e.x2), s3 = key_value(e.x3),
                 s4 = key_value(e.x4), s5 = key_value(e.x5), s6 = key_value(e.x6), s7 = key_value(e.x7);
    med = pick_median(s0, s1, s2, s3, s4, k);
    // the residuals of the sorted values are those of the neighbours (a staged +inf stays +inf); they are >= 0, where
    // the bit pattern is its own sort key
    e.x0 = residual(s0, med); e.x1 = residual(s1, med); e.x2 = residual(s2, med); e.x3 = residual(s3, med);
    e.x4 = residual(s4, med); e.x5 = residual(s5, med); e.x6 = residual(s6, med); e.x7 = residual(s7, med);
    sort8(e);
    const double rmed = pick_median(__longlong_as_double(e.x0), __longlong_as_double(e.x1), __longlong_as_double(e.x2),
                                    __longlong_as_double(e.x3), __longlong_as_double(e.x4), k);
    return fabs(centre - med) > threshold * (rmed + eps);
}

__global__ __launch_bounds__(kThreads) void median_test_kernel(OutlierParams p) {
    __shared__ double su[(kTR + 2) * kPitch], sv[(kTR + 2) * kPitch];
    const int tid = threadIdx.x, tx = tid % kTC, ty = tid / kTC;
    const int c0 = blockIdx.x * kTC, r0 = blockIdx.y * kTR;
    const size_t field = (size_t)blockIdx.z * p.n_rows * p.n_cols;
    const double inf = __longlong_as_double(kInfBits);

    // own cell
    const int r = r0 + ty, c = c0 + tx;
    const bool inside = r < p.n_rows && c < p.n_cols;
    const size_t cell = field + (size_t)r * p.n_cols + c;
    double uc = 0.0, vc = 0.0;
    uint8_t mc = 1;
    if (inside) {
        uc = p.u[cell];
        vc = p.v[cell];
        mc = p.invalid[cell];
    }
    const int at = (ty + 1) * kPitch + tx + 1;
    su[at] = mc == 0 ? uc : inf;
    sv[at] = mc == 0 ? vc : inf;
    // the halo ring: top row, bottom row, then the left and right columns
    if (tid < kRing) {
        int hr, hc;
        if (tid < 2 * kPitch) {
            hr = tid < kPitch ? 0 : kTR + 1;
            hc = tid < kPitch ? tid : tid - kPitch;
        } else {
            const int q = tid - 2 * kPitch;
            hr = 1 + (q >> 1);
            hc = (q & 1) ? kTC + 1 : 0;
        }
        const int gr = r0 - 1 + hr, gc = c0 - 1 + hc;
        double uh = inf, vh = inf;
        if (gr >= 0 && gr < p.n_rows && gc >= 0 && gc < p.n_cols) {
            const size_t g = field + (size_t)gr * p.n_cols + gc;
            const double ug = p.u[g], vg = p.v[g];           // (unconditional: three loads in flight, not a mask-then-value chain)
            const bool ok = p.invalid[g] == 0;
            uh = ok ? ug : inf;
            vh = ok ? vg : inf;
        }
        su[hr * kPitch + hc] = uh;
        sv[hr * kPitch + hc] = vh;
    }
    __syncthreads();
    if (!inside) return;

    // valid neighbours: the staged cells that are not +inf.  Counted on u alone: the contract is finite input; a valid
    // cell whose u is +inf, or whose v alone is not finite, is miscounted (nothing faults, nothing else is promised)
    int k = 0;
#pragma unroll
    for (int dr = -1; dr <= 1; ++dr)
#pragma unroll
        for (int dc = -1; dc <= 1; ++dc)
            if (dr != 0 || dc != 0) k += __double_as_longlong(su[at + dr * kPitch + dc]) != kInfBits;

    double mu = uc, mv = vc;
    bool flag = false;
    if (k >= p.min_neighbours) {
        const bool fu = component(su, at, k, uc, p.threshold, p.eps, mu);
        const bool fv = component(sv, at, k, vc, p.threshold, p.eps, mv);
        flag = fu | fv;
    }
    p.status[cell] = (uint8_t)((flag ? 1 : 0) | (mc != 0 ? 2 : 0));
    if (p.invalid_out) p.invalid_out[cell] = (uint8_t)((mc != 0 || flag) ? 1 : 0);
    // replace: the field with its flagged cells at the neighbourhood median; otherwise the medians themselves
    if (p.out_u) p.out_u[cell] = (p.replace && !flag) ? uc : mu;
    if (p.out_v) p.out_v[cell] = (p.replace && !flag) ? vc : mv;
}

}  // namespace

hipError_t launch_median_test(const OutlierParams& p, hipStream_t stream) {
    if (p.batch <= 0) return hipSuccess;
    const dim3 grid((unsigned)((p.n_cols + kTC - 1) / kTC), (unsigned)((p.n_rows + kTR - 1) / kTR), (unsigned)p.batch);
    if (grid.y > 65535u || grid.z > 65535u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(median_test_kernel, grid, dim3(kThreads), 0, stream, p);
    return hipGetLastError();
}

}  // namespace tpiv
