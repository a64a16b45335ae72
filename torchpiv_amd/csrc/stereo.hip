// Stereoscopic reconstruction: the three components (U, V, W) of every cell from the two in-plane fields that two
// cameras deliver and the cameras' viewing tangents (include/torchpiv_hip.h: tpiv_stereo_reconstruct has the definition
// and the operation order).
//
// A streaming kernel: 4 (8 with the sigmas) float64 planes in and 4 (7) out per pair, about ten operations per value.
// What a cell's geometry contributes -- da, db, g, the tangent sums and, with the sigmas, the six squared weights of the
// error propagation -- does not depend on the pair, so a lane computes it once, keeps it in registers and walks
// STEREO_BLOCK_PAIRS pairs of the stack with it: the four tangent planes are read once per STEREO_BLOCK_PAIRS pairs and
// not once per pair.  The grid is (cell blocks, pair blocks).  A lane owns VEC adjacent cells: two (16-byte loads and
// stores) when the cell count is even and every plane is 16-byte aligned, else one (8-byte).
// The per-pair summary is a second launch that reads res and status back, one workgroup per pair, every lane summing its
// cells in ascending order and the lanes combined by a fixed tree: no floating-point atomics, the same bytes every time.
// Every floating-point operation is one IEEE float64 operation, contraction is off for this unit.
// Below it, the self-calibration's triangulation (tpiv_stereo_triangulate) in the same layout.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "piv_kernels.h"

#pragma clang fp contract(off)

namespace tpiv {

namespace {

constexpr int kThreads = STEREO_BLOCK_THREADS, kPairs = STEREO_BLOCK_PAIRS, kSum = STEREO_SUM_THREADS;
static_assert(kThreads % 64 == 0 && kSum == 1024, "whole wavefronts; the summary tree starts at 512");

constexpr long long kNaN = 0x7ff8000000000000LL;      // the NaN written out
constexpr long long kExpMask = 0x7ff0000000000000LL;

__device__ __forceinline__ bool is_finite(double x) { return (__double_as_longlong(x) & kExpMask) != kExpMask; }

template <int VEC>
struct alignas(8 * VEC) DV {
    double x[VEC];
};
template <int VEC>
struct alignas(VEC) BV {
    uint8_t x[VEC];
};
template <int VEC>
__device__ __forceinline__ DV<VEC> load(const double* p, size_t i) {
    return *reinterpret_cast<const DV<VEC>*>(p + i);
}
template <int VEC>
__device__ __forceinline__ void store(double* p, size_t i, const DV<VEC>& v) {
    *reinterpret_cast<DV<VEC>*>(p + i) = v;
}

template <int VEC, bool SIG>
__global__ __launch_bounds__(kThreads) void stereo_kernel(StereoParams p) {
    const size_t cells = (size_t)p.cells;
    const size_t c0 = ((size_t)blockIdx.x * kThreads + threadIdx.x) * VEC;
    if (c0 >= cells) return;                          // (VEC == 2: cells is even, both cells are inside)
    const double nan = __longlong_as_double(kNaN);

    // the geometry of this lane's cells, once for all its pairs
    double da[VEC], db[VEC], g[VEC], sa[VEC], sb[VEC];
    double gg[VEC], da2[VEC], db2[VEC], wu1[VEC], wu2[VEC], wuv[VEC], wv1[VEC], wv2[VEC], wvu[VEC];
    int cls[VEC];                                     // 1: skipped, 3: no geometry, 0: reconstruct
    {
        const DV<VEC> a1 = load<VEC>(p.a1, c0), b1 = load<VEC>(p.b1, c0), a2 = load<VEC>(p.a2, c0), b2 = load<VEC>(p.b2, c0);
        BV<VEC> sk{};
        if (p.skip != nullptr) sk = *reinterpret_cast<const BV<VEC>*>(p.skip + c0);
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            da[k] = a1.x[k] - a2.x[k];
            db[k] = b1.x[k] - b2.x[k];
            da2[k] = da[k] * da[k];
            db2[k] = db[k] * db[k];
            g[k] = da2[k] + db2[k];
            sa[k] = a1.x[k] + a2.x[k];
            sb[k] = b1.x[k] + b2.x[k];
            const bool geo = is_finite(a1.x[k]) && is_finite(b1.x[k]) && is_finite(a2.x[k]) && is_finite(b2.x[k]) && g[k] != 0.0;
            cls[k] = sk.x[k] != 0 ? 1 : (geo ? 0 : 3);
            if (SIG) {
                const double ma = sa[k] * 0.5, mb = sb[k] * 0.5;
                const double ka = ma * da[k] / g[k], kb = ma * db[k] / g[k];
                const double la = mb * db[k] / g[k], lb = mb * da[k] / g[k];
                const double cu1 = 0.5 - ka, cu2 = 0.5 + ka, cv1 = 0.5 - la, cv2 = 0.5 + la;
                gg[k] = g[k] * g[k];
                wu1[k] = cu1 * cu1;
                wu2[k] = cu2 * cu2;
                wuv[k] = kb * kb;
                wv1[k] = cv1 * cv1;
                wv2[k] = cv2 * cv2;
                wvu[k] = lb * lb;
            }
        }
    }

    const int pair0 = blockIdx.y * kPairs;
    const int pair1 = pair0 + kPairs < p.batch ? pair0 + kPairs : p.batch;
    for (int pair = pair0; pair < pair1; ++pair) {
        const size_t at = (size_t)pair * cells + c0;
        const DV<VEC> u1 = load<VEC>(p.u1, at), v1 = load<VEC>(p.v1, at), u2 = load<VEC>(p.u2, at), v2 = load<VEC>(p.v2, at);
        DV<VEC> s1, t1, s2, t2;
        if (SIG) {
            s1 = load<VEC>(p.su1, at);
            t1 = load<VEC>(p.sv1, at);
            s2 = load<VEC>(p.su2, at);
            t2 = load<VEC>(p.sv2, at);
        }
        DV<VEC> oU, oV, oW, oR, oSU, oSV, oSW;
        BV<VEC> oS;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const bool data = is_finite(u1.x[k]) && is_finite(v1.x[k]) && is_finite(u2.x[k]) && is_finite(v2.x[k]);
            const int st = cls[k] != 0 ? cls[k] : (data ? 0 : 2);
            const double du = u1.x[k] - u2.x[k], dv = v1.x[k] - v2.x[k];
            const double W = (da[k] * du + db[k] * dv) / g[k];
            const double U = ((u1.x[k] + u2.x[k]) - sa[k] * W) * 0.5;
            const double V = ((v1.x[k] + v2.x[k]) - sb[k] * W) * 0.5;
            const double eu = du - da[k] * W, ev = dv - db[k] * W;
            const double res = __dsqrt_rn((eu * eu + ev * ev) * 0.5);
            const double blank = st == 1 ? p.fill : nan;
            oU.x[k] = st == 0 ? U : blank;
            oV.x[k] = st == 0 ? V : blank;
            oW.x[k] = st == 0 ? W : blank;
            oR.x[k] = st == 0 ? res : nan;
            oS.x[k] = (uint8_t)st;
            if (SIG) {
                const double q1 = s1.x[k] * s1.x[k], q2 = s2.x[k] * s2.x[k], r1 = t1.x[k] * t1.x[k], r2 = t2.x[k] * t2.x[k];
                const double qs = q1 + q2, rs = r1 + r2;
                const double sW = __dsqrt_rn((da2[k] * qs + db2[k] * rs) / gg[k]);
                const double sU = __dsqrt_rn(wu1[k] * q1 + wu2[k] * q2 + wuv[k] * rs);
                const double sV = __dsqrt_rn(wv1[k] * r1 + wv2[k] * r2 + wvu[k] * qs);
                const bool ok = st == 0 && is_finite(s1.x[k]) && is_finite(t1.x[k]) && is_finite(s2.x[k]) && is_finite(t2.x[k]);
                oSU.x[k] = ok ? sU : nan;
                oSV.x[k] = ok ? sV : nan;
                oSW.x[k] = ok ? sW : nan;
            }
        }
        store<VEC>(p.U, at, oU);
        store<VEC>(p.V, at, oV);
        store<VEC>(p.W, at, oW);
        store<VEC>(p.res, at, oR);
        if (SIG) {
            store<VEC>(p.sU, at, oSU);
            store<VEC>(p.sV, at, oSV);
            store<VEC>(p.sW, at, oSW);
        }
        *reinterpret_cast<BV<VEC>*>(p.status + at) = oS;
    }
}

// pair_count = the status-0 cells of the pair; pair_rms = sqrt(sum res^2 / count): lane t sums its cells t, t + kSum, ...
// in ascending order from +0.0, then the lanes fold in halves -- acc[t] = acc[t] + acc[t + s] for s = 512, 256 .. 1.
__global__ __launch_bounds__(kSum) void stereo_summary_kernel(StereoParams p) {
    __shared__ double acc[kSum];
    __shared__ int cnt[kSum];
    const int t = threadIdx.x;
    const size_t cells = (size_t)p.cells, base = (size_t)blockIdx.x * cells;
    double sum = 0.0;
    int n = 0;
#pragma unroll 4
    for (size_t c = t; c < cells; c += kSum) {
        const double r = p.res[base + c];
        const bool ok = p.status[base + c] == 0;
        const double q = r * r;
        sum = ok ? sum + q : sum;
        n += ok ? 1 : 0;
    }
    acc[t] = sum;
    cnt[t] = n;
    __syncthreads();
    for (int s = kSum / 2; s >= 1; s >>= 1) {
        if (t < s) {
            acc[t] = acc[t] + acc[t + s];
            cnt[t] += cnt[t + s];
        }
        __syncthreads();
    }
    if (t == 0) {
        p.pair_count[blockIdx.x] = cnt[0];
        p.pair_rms[blockIdx.x] = cnt[0] > 0 ? __dsqrt_rn(acc[0] / (double)cnt[0]) : __longlong_as_double(kNaN);
    }
}

template <int VEC>
void launch_vec(const StereoParams& p, hipStream_t stream) {
    const long long per_block = (long long)kThreads * VEC;
    const dim3 grid((unsigned)((p.cells + per_block - 1) / per_block), (unsigned)((p.batch + kPairs - 1) / kPairs));
    if (p.su1 != nullptr)
        hipLaunchKernelGGL((stereo_kernel<VEC, true>), grid, dim3(kThreads), 0, stream, p);
    else
        hipLaunchKernelGGL((stereo_kernel<VEC, false>), grid, dim3(kThreads), 0, stream, p);
}

bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

}  // namespace

hipError_t launch_stereo_reconstruct(const StereoParams& p, hipStream_t stream) {
    if (p.batch <= 0) return hipSuccess;
    if (p.cells < 1 || (p.batch + kPairs - 1) / kPairs > 65535) return hipErrorInvalidValue;
    bool wide = p.cells % 2 == 0 && (p.skip == nullptr || ((uintptr_t)p.skip & 1) == 0) && ((uintptr_t)p.status & 1) == 0;
    const void* planes[] = {p.u1, p.v1, p.u2, p.v2, p.su1, p.sv1, p.su2, p.sv2, p.a1, p.b1, p.a2, p.b2,
                            p.U,  p.V,  p.W,  p.res, p.sU, p.sV, p.sW};
    for (const void* q : planes) wide = wide && aligned16(q);       // (an absent plane is null: aligned)
    if (wide)
        launch_vec<2>(p, stream);
    else
        launch_vec<1>(p, stream);
    hipError_t he = hipGetLastError();
    if (he != hipSuccess) return he;
    hipLaunchKernelGGL(stereo_summary_kernel, dim3((unsigned)p.batch), dim3(kSum), 0, stream, p);
    return hipGetLastError();
}

// ---- self-calibration: the point between the two cameras' lines of sight per cell of a disparity field, and the sums of a
// plane fit through those points (include/torchpiv_hip.h: tpiv_stereo_triangulate has the definition and the operation
// order).  The streaming kernel has stereo_kernel's layout -- a lane keeps X, Y and skip of its VEC cells and walks kPairs
// items of the stack: 2 planes in and up to 4 planes and a byte out per item.  The sums are a second launch, one workgroup
// of kSum lanes per item: lane t walks the cells t, t + kSum, ... and triangulates them AGAIN (about 60 operations, two
// divisions and a root per cell: the same function, so the same bits) instead of reading Mx, My, Mz back, which the caller
// may not have asked for; it reads dx, dy, X, Y and skip only.  Nine accumulators per lane, folded one after the other
// through one 8 KiB LDS array by pair_rms's tree.  One workgroup per item is what the fixed order costs without work
// memory: a large grid at a small batch leaves most of the device idle in this second launch (profiles/selfcal).
namespace {

struct TriPoint {
    double x, y, z, gap;
    int st;
};

__device__ __forceinline__ TriPoint triangulate(const TriangulateParams& p, bool centres, double dx, double dy, double X,
                                                double Y, bool skipped) {
    const double hx = dx * 0.5, hy = dy * 0.5;
    const double q1x = X - hx, q1y = Y - hy, q2x = X + hx, q2y = Y + hy;
    const double d1x = q1x - p.C1[0], d1y = q1y - p.C1[1], d1z = 0.0 - p.C1[2];
    const double d2x = q2x - p.C2[0], d2y = q2y - p.C2[1], d2z = 0.0 - p.C2[2];
    const double wx = p.C1[0] - p.C2[0], wy = p.C1[1] - p.C2[1], wz = p.C1[2] - p.C2[2];
    const double a = d1x * d1x + d1y * d1y + d1z * d1z;
    const double b = d1x * d2x + d1y * d2y + d1z * d2z;
    const double c = d2x * d2x + d2y * d2y + d2z * d2z;
    const double d = d1x * wx + d1y * wy + d1z * wz;
    const double e = d2x * wx + d2y * wy + d2z * wz;
    const double den = a * c - b * b;
    const double s = (b * e - c * d) / den, t = (a * e - b * d) / den;
    const double p1x = p.C1[0] + s * d1x, p1y = p.C1[1] + s * d1y, p1z = p.C1[2] + s * d1z;
    const double p2x = p.C2[0] + t * d2x, p2y = p.C2[1] + t * d2y, p2z = p.C2[2] + t * d2z;
    const double gx = p1x - p2x, gy = p1y - p2y, gz = p1z - p2z;
    TriPoint o;
    o.x = (p1x + p2x) * 0.5;
    o.y = (p1y + p2y) * 0.5;
    o.z = (p1z + p2z) * 0.5;
    o.gap = __dsqrt_rn(gx * gx + gy * gy + gz * gz);
    const double r = o.z - ((p.plane[0] + p.plane[1] * o.x) + p.plane[2] * o.y);
    const bool data = is_finite(dx) && is_finite(dy);
    const bool lines = is_finite(den) && den > 0.0;
    o.st = skipped ? 1 : !centres ? 3 : !data ? 2 : !lines ? 3 : o.gap > p.gap_max ? 4 : __builtin_fabs(r) > p.tol ? 5 : 0;
    return o;
}

__device__ __forceinline__ bool centres_finite(const TriangulateParams& p) {
    return is_finite(p.C1[0]) && is_finite(p.C1[1]) && is_finite(p.C1[2]) && is_finite(p.C2[0]) && is_finite(p.C2[1]) &&
           is_finite(p.C2[2]);
}

template <int VEC, bool PTS>
__global__ __launch_bounds__(kThreads) void triangulate_kernel(TriangulateParams p) {
    const size_t cells = (size_t)p.cells;
    const size_t c0 = ((size_t)blockIdx.x * kThreads + threadIdx.x) * VEC;
    if (c0 >= cells) return;                          // (VEC == 2: cells is even, both cells are inside)
    const double nan = __longlong_as_double(kNaN);
    const bool centres = centres_finite(p);
    const DV<VEC> X = load<VEC>(p.X, c0), Y = load<VEC>(p.Y, c0);
    BV<VEC> sk{};
    if (p.skip != nullptr) sk = *reinterpret_cast<const BV<VEC>*>(p.skip + c0);
    const int item0 = blockIdx.y * kPairs;
    const int item1 = item0 + kPairs < p.batch ? item0 + kPairs : p.batch;
    for (int item = item0; item < item1; ++item) {
        const size_t at = (size_t)item * cells + c0;
        const DV<VEC> dx = load<VEC>(p.dx, at), dy = load<VEC>(p.dy, at);
        DV<VEC> oX, oY, oZ, oG;
        BV<VEC> oS;
#pragma unroll
        for (int k = 0; k < VEC; ++k) {
            const TriPoint m = triangulate(p, centres, dx.x[k], dy.x[k], X.x[k], Y.x[k], sk.x[k] != 0);
            const bool blank = m.st >= 1 && m.st <= 3;
            oX.x[k] = blank ? nan : m.x;
            oY.x[k] = blank ? nan : m.y;
            oZ.x[k] = blank ? nan : m.z;
            oG.x[k] = blank ? nan : m.gap;
            oS.x[k] = (uint8_t)m.st;
        }
        if (PTS) {
            store<VEC>(p.Mx, at, oX);
            store<VEC>(p.My, at, oY);
            store<VEC>(p.Mz, at, oZ);
            store<VEC>(p.gap, at, oG);
        }
        *reinterpret_cast<BV<VEC>*>(p.status + at) = oS;
    }
}

// count = the status-0 cells of the item; sums[0..8] = the sums of x, y, z, xx, xy, yy, xz, yz, zz over them with (x, y, z) =
// M - centre: lane t sums its cells t, t + kSum, ... in ascending order from +0.0, then the lanes fold in halves.
__global__ __launch_bounds__(kSum) void triangulate_sums_kernel(TriangulateParams p) {
    __shared__ double acc[kSum];
    __shared__ int cnt[kSum];
    const int t = threadIdx.x;
    const size_t cells = (size_t)p.cells, base = (size_t)blockIdx.x * cells;
    const bool centres = centres_finite(p);
    double sum[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) sum[k] = 0.0;
    int n = 0;
#pragma unroll 2
    for (size_t c = t; c < cells; c += kSum) {
        const bool skipped = p.skip != nullptr && p.skip[c] != 0;
        const TriPoint m = triangulate(p, centres, p.dx[base + c], p.dy[base + c], p.X[c], p.Y[c], skipped);
        const bool ok = m.st == 0;
        const double x = m.x - p.centre[0], y = m.y - p.centre[1], z = m.z - p.centre[2];
        const double q[9] = {x, y, z, x * x, x * y, y * y, x * z, y * z, z * z};
#pragma unroll
        for (int k = 0; k < 9; ++k) sum[k] = ok ? sum[k] + q[k] : sum[k];
        n += ok ? 1 : 0;
    }
    cnt[t] = n;
#pragma unroll                                        // (sum[] stays in registers)
    for (int k = 0; k < 9; ++k) {
        __syncthreads();                              // (the fold before has been read out)
        acc[t] = sum[k];
        __syncthreads();
        for (int s = kSum / 2; s >= 1; s >>= 1) {
            if (t < s) {
                acc[t] = acc[t] + acc[t + s];
                if (k == 0) cnt[t] += cnt[t + s];
            }
            __syncthreads();
        }
        if (t == 0) p.sums[(size_t)blockIdx.x * 9 + k] = acc[0];
    }
    if (t == 0) p.count[blockIdx.x] = cnt[0];
}

template <int VEC>
void launch_triangulate_vec(const TriangulateParams& p, hipStream_t stream) {
    const long long per_block = (long long)kThreads * VEC;
    const dim3 grid((unsigned)((p.cells + per_block - 1) / per_block), (unsigned)((p.batch + kPairs - 1) / kPairs));
    if (p.Mx != nullptr)
        hipLaunchKernelGGL((triangulate_kernel<VEC, true>), grid, dim3(kThreads), 0, stream, p);
    else
        hipLaunchKernelGGL((triangulate_kernel<VEC, false>), grid, dim3(kThreads), 0, stream, p);
}

}  // namespace

hipError_t launch_stereo_triangulate(const TriangulateParams& p, hipStream_t stream) {
    if (p.batch <= 0) return hipSuccess;
    if (p.cells < 1 || (p.batch + kPairs - 1) / kPairs > 65535) return hipErrorInvalidValue;
    bool wide = p.cells % 2 == 0 && (p.skip == nullptr || ((uintptr_t)p.skip & 1) == 0) && ((uintptr_t)p.status & 1) == 0;
    const void* planes[] = {p.dx, p.dy, p.X, p.Y, p.Mx, p.My, p.Mz, p.gap};
    for (const void* q : planes) wide = wide && aligned16(q);       // (an absent plane is null: aligned)
    if (wide)
        launch_triangulate_vec<2>(p, stream);
    else
        launch_triangulate_vec<1>(p, stream);
    hipError_t he = hipGetLastError();
    if (he != hipSuccess) return he;
    hipLaunchKernelGGL(triangulate_sums_kernel, dim3((unsigned)p.batch), dim3(kSum), 0, stream, p);
    return hipGetLastError();
}

}  // namespace tpiv
