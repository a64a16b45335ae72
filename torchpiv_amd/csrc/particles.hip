// Particle images of uint8 frames and their pairing between the two frames of a pair (include/torchpiv_hip.h:
// tpiv_particle_count / tpiv_particle_detect / tpiv_particle_match have the definitions and the operation order).
//
// Detection.  A wavefront owns one image row, a workgroup kRows adjacent rows of one frame (the rows above and below a
// wavefront's row are its neighbours' rows: they meet in the L1).  The row is walked in steps of 64 lanes x 4 pixels; a
// lane reads, for each of the three rows, the eight bytes from two pixels left of its first pixel on -- one 8-byte load
// at whatever alignment the row has; the lanes at the two ends of a row gather theirs byte by byte, in bounds -- and
// tests its four pixels in registers.  The list is in raster order by construction, never by arrival: the counting
// launch leaves one count per row, a scan per frame turns them into row_start, and the writing launch walks the rows
// again; inside a row the place of a peak is row_start + the peaks of the steps before + the peaks of the lower lanes
// (four ballots and their prefix popcounts) + the lane's own lower pixels.  The neighbourhood test runs in both
// launches; no peak bit mask is kept between them.
//
// Matching.  A lane per particle of frame a.  The first launch interpolates the predictor, walks the rows of frame b's
// list that the radius reaches (row_start; a binary search for the first column inside each row's segment), keeps the
// nearest candidate (ascending list index, strict comparison: ties go to the lower index) and lowers the candidate's
// claim word to the bit pattern of its d2 (64-bit unsigned atomic minimum; d2 >= +0.0, so the patterns order like the
// values).  The second launch lowers a second word to the index of the claimant among those that hold the minimum, the
// third gives every particle its verdict.  Minima of integers do not depend on the order of arrival, and each launch
// only reads what the launch before it completed.
//
// Every floating-point operation is one IEEE float64 operation; contraction is off for this unit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "piv_kernels.h"

#pragma clang fp contract(off)

namespace tpiv {

namespace {

typedef unsigned long long u64;

constexpr int kRows = PARTICLE_BLOCK_ROWS, kPx = PARTICLE_LANE_PIXELS;
constexpr int kThreads = 64 * kRows, kStep = 64 * kPx;
static_assert(kPx == 4 && kThreads == 256, "four ballots per step; the table is staged by 256 lanes");

constexpr long long kNaN = 0x7ff8000000000000LL;
constexpr int kNoParticle = 255;      // status of the list entries behind a frame's last particle

__device__ __forceinline__ unsigned byte_of(u64 w, int k) { return (unsigned)(w >> (8 * k)) & 0xffu; }

// the pixels c0 - 2 .. c0 + 5 of a row, pixel c0 - 2 + k in byte k; 0 outside the row (no reported pixel reads those)
__device__ __forceinline__ u64 load_span(const uint8_t* __restrict__ row, int c0, int W) {
    u64 w = 0;
    if (c0 >= 2 && c0 + 5 < W) {
        __builtin_memcpy(&w, row + c0 - 2, 8);
    } else {
        for (int k = 0; k < 8; ++k) {
            const int c = c0 - 2 + k;
            if (c >= 0 && c < W) w |= (u64)row[c] << (8 * k);
        }
    }
    return w;
}

// bit j: pixel c0 + j of the middle row is a particle image (level, interior column, the eight neighbours)
__device__ __forceinline__ unsigned peaks_of(u64 up, u64 mid, u64 dn, int c0, int W, unsigned level) {
    unsigned m = 0;
#pragma unroll
    for (int j = 0; j < kPx; ++j) {
        const int c = c0 + j;
        const unsigned I = byte_of(mid, j + 2);
        bool ok = c >= 1 && c <= W - 2 && I >= level;
        ok = ok && I > byte_of(up, j + 1) && I > byte_of(up, j + 2) && I > byte_of(up, j + 3) && I > byte_of(mid, j + 1);
        ok = ok && I >= byte_of(mid, j + 3) && I >= byte_of(dn, j + 1) && I >= byte_of(dn, j + 2) && I >= byte_of(dn, j + 3);
        m |= ok ? 1u << j : 0u;
    }
    return m;
}

__device__ __forceinline__ double subpixel(double L, double C, double R) {
    const double den = (L - 2.0 * C) + R;
    return den < 0.0 ? (L - R) / (2.0 * den) : 0.0;
}

template <bool WRITE>
__global__ __launch_bounds__(kThreads) void particle_rows_kernel(ParticleParams p) {
    __shared__ double tab[256];
    if (WRITE) {
        tab[threadIdx.x] = p.table[threadIdx.x];
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * kRows + wave, f = blockIdx.y;
    const int H = p.H, W = p.W;
    if (r >= H) return;
    int32_t* rs = p.row_start + (size_t)f * (H + 1);
    if (r == 0 || r == H - 1) {                       // border rows hold no particle image
        if (!WRITE && lane == 0) rs[r] = 0;
        return;
    }
    const uint8_t* __restrict__ mid = p.frames + ((size_t)f * H + r) * W;
    const uint8_t* __restrict__ up = mid - W;
    const uint8_t* __restrict__ dn = mid + W;
    const int base = WRITE ? rs[r] : 0;
    const u64 below = (1ull << lane) - 1;
    int run = 0;
    for (int s = 0; s < W; s += kStep) {              // (wave-uniform: every lane takes every ballot)
        const int c0 = s + lane * kPx;
        unsigned m = 0;
        u64 wu = 0, wm = 0, wd = 0;
        if (c0 < W) {
            wu = load_span(up, c0, W);
            wm = load_span(mid, c0, W);
            wd = load_span(dn, c0, W);
            m = peaks_of(wu, wm, wd, c0, W, (unsigned)p.level);
            if (m != 0 && p.mask != nullptr) {
                const uint8_t* __restrict__ mk = p.mask + (size_t)r * W + c0;
#pragma unroll
                for (int j = 0; j < kPx; ++j)
                    if (((m >> j) & 1u) && mk[j] != 0) m &= ~(1u << j);
            }
        }
        const u64 b0 = __ballot(m & 1u), b1 = __ballot(m & 2u), b2 = __ballot(m & 4u), b3 = __ballot(m & 8u);
        if (WRITE) {
            int idx = base + run + __popcll(b0 & below) + __popcll(b1 & below) + __popcll(b2 & below) + __popcll(b3 & below);
#pragma unroll
            for (int j = 0; j < kPx; ++j) {
                if ((m >> j) & 1u) {
                    if (idx < p.capacity) {
                        const unsigned I = byte_of(wm, j + 2);
                        const double C = tab[I];
                        const double ox = subpixel(tab[byte_of(wm, j + 1)], C, tab[byte_of(wm, j + 3)]);
                        const double oy = subpixel(tab[byte_of(wu, j + 2)], C, tab[byte_of(wd, j + 2)]);
                        const size_t o = (size_t)f * p.capacity + idx;
                        p.x[o] = (double)(c0 + j) + ox;
                        p.y[o] = (double)r + oy;
                        p.peak[o] = (uint8_t)I;
                    }
                    ++idx;
                }
            }
        }
        run += __popcll(b0) + __popcll(b1) + __popcll(b2) + __popcll(b3);
    }
    if (!WRITE && lane == 0) rs[r] = run;
}

// row_start of one frame in place: the per-row counts become their exclusive prefix sums, entry H and count the total
__global__ __launch_bounds__(256) void particle_scan_kernel(int32_t* row_start, int32_t* count, int H) {
    __shared__ int part[256];
    const int f = blockIdx.x, t = threadIdx.x;
    int32_t* rs = row_start + (size_t)f * (H + 1);
    const int k = (H + 255) / 256;
    const int lo = min(t * k, H), hi = min(lo + k, H);
    int s = 0;
    for (int r = lo; r < hi; ++r) s += rs[r];
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const int add = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    int pre = part[t] - s;
    for (int r = lo; r < hi; ++r) {
        const int c = rs[r];
        rs[r] = pre;
        pre += c;
    }
    if (t == 255) {
        rs[H] = part[255];
        count[f] = part[255];
    }
}

// the centres c[j0], c[j1] around x and the weight of c[j1]; constant outside the centres (j0 == j1, t = 0)
__device__ __forceinline__ void bracket(const double* __restrict__ c, int n, double x, int& j0, int& j1, double& t) {
    int lo = 0, hi = n;
    while (lo < hi) {                                 // lo = how many centres are <= x
        const int m = (lo + hi) >> 1;
        if (c[m] <= x)
            lo = m + 1;
        else
            hi = m;
    }
    j0 = max(lo - 1, 0);
    j1 = min(lo, n - 1);
    t = j1 > j0 ? (x - c[j0]) / (c[j1] - c[j0]) : 0.0;
}

__device__ __forceinline__ double bilinear(const double* __restrict__ g, int nc, int x0, int x1, double tx, int y0, int y1,
                                           double ty) {
    const double g00 = g[(size_t)y0 * nc + x0], g01 = g[(size_t)y0 * nc + x1];
    const double g10 = g[(size_t)y1 * nc + x0], g11 = g[(size_t)y1 * nc + x1];
    const double a = g00 + tx * (g01 - g00), b = g10 + tx * (g11 - g10);
    return a + ty * (b - a);
}

// the stored length of a list: its frame's count, capped
__device__ __forceinline__ int stored(const int32_t* __restrict__ rs, int H, int cap) { return min(rs[H], cap); }

__global__ __launch_bounds__(256) void match_nearest_kernel(ParticleMatchParams p) {
    const int i = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (i >= p.cap_a) return;
    const int H = p.H;
    const size_t oa = (size_t)f * p.cap_a + i, ob = (size_t)f * p.cap_b;
    const double nan = __longlong_as_double(kNaN);
    if (i >= stored(p.rsa + (size_t)f * (H + 1), H, p.cap_a)) {
        p.match[oa] = -1;
        p.status[oa] = (uint8_t)kNoParticle;
        p.d2[oa] = nan;
        return;
    }
    const double x = p.xa[oa], y = p.ya[oa];
    int x0, x1, y0, y1;
    double tx, ty;
    bracket(p.xc, p.n_cols, x, x0, x1, tx);
    bracket(p.yc, p.n_rows, y, y0, y1, ty);
    const size_t field = (size_t)f * p.n_rows * p.n_cols;
    const double px = x + bilinear(p.up + field, p.n_cols, x0, x1, tx, y0, y1, ty);
    const double py = y + bilinear(p.vp + field, p.n_cols, x0, x1, tx, y0, y1, ty);
    if (!(px >= 0.0 && px <= (double)(p.W - 1) && py >= 0.0 && py <= (double)(H - 1))) {     // (a NaN is outside)
        p.match[oa] = -1;
        p.status[oa] = 3;
        p.d2[oa] = nan;
        return;
    }
    const double R = p.radius, R2 = R * R;
    const int rlo = (int)fmax(ceil(py - R - 0.5), 0.0), rhi = (int)fmin(floor(py + R + 0.5), (double)(H - 1));
    const int32_t* __restrict__ rsb = p.rsb + (size_t)f * (H + 1);
    const int nb = stored(rsb, H, p.cap_b);
    const double* __restrict__ xb = p.xb + ob;
    const double* __restrict__ yb = p.yb + ob;
    // the columns are scanned half a pixel beyond the radius on either side: what lies outside is farther than R by far
    // more than the rounding of d2, so the scan sees every candidate of the definition
    const double xlo = px - R - 0.5, xhi = px + R + 0.5;
    int best = -1;
    double best_d2 = nan;
    for (int rr = rlo; rr <= rhi; ++rr) {
        int lo = min(rsb[rr], nb);
        const int end = min(rsb[rr + 1], nb);
        int hi = end;
        while (lo < hi) {                             // lo = the first entry of the row with x >= xlo
            const int m = (lo + hi) >> 1;
            if (xb[m] < xlo)
                lo = m + 1;
            else
                hi = m;
        }
        for (int j = lo; j < end && xb[j] <= xhi; ++j) {
            const double dx = px - xb[j], dy = py - yb[j];
            const double d2 = dx * dx + dy * dy;
            if (d2 <= R2 && (best < 0 || d2 < best_d2)) {
                best = j;
                best_d2 = d2;
            }
        }
    }
    p.match[oa] = best;
    p.status[oa] = best < 0 ? 1 : 0;
    p.d2[oa] = best_d2;
    if (best >= 0) atomicMin(p.claim_d2 + ob + best, (u64)__double_as_longlong(best_d2));
}

__global__ __launch_bounds__(256) void match_claim_kernel(ParticleMatchParams p) {
    const int i = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    if (i >= p.cap_a) return;
    const size_t oa = (size_t)f * p.cap_a + i, ob = (size_t)f * p.cap_b;
    if (p.status[oa] != 0) return;
    const int j = p.match[oa];
    if ((u64)__double_as_longlong(p.d2[oa]) == p.claim_d2[ob + j]) atomicMin(p.claim_i + ob + j, (unsigned)i);
}

__global__ __launch_bounds__(256) void match_verdict_kernel(ParticleMatchParams p) {
    const int i = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
    bool won = false;
    if (i < p.cap_a) {
        const size_t oa = (size_t)f * p.cap_a + i, ob = (size_t)f * p.cap_b;
        if (p.status[oa] == 0) {
            won = p.claim_i[ob + p.match[oa]] == (unsigned)i;
            if (!won) {
                p.match[oa] = -1;
                p.status[oa] = 2;
            }
        }
    }
    const u64 winners = __ballot(won);
    if ((threadIdx.x & 63) == 0 && winners != 0) atomicAdd(p.matched + f, (int)__popcll(winners));
}

hipError_t launch_rows(const ParticleParams& p, bool write, hipStream_t stream) {
    if (p.n <= 0) return hipSuccess;
    if (p.H < 3 || p.W < 3 || p.n > 65535) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((p.H + kRows - 1) / kRows), (unsigned)p.n);
    if (write)
        hipLaunchKernelGGL(particle_rows_kernel<true>, grid, dim3(kThreads), 0, stream, p);
    else
        hipLaunchKernelGGL(particle_rows_kernel<false>, grid, dim3(kThreads), 0, stream, p);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_particle_count(const ParticleParams& p, hipStream_t stream) {
    hipError_t he = launch_rows(p, false, stream);
    if (he != hipSuccess || p.n <= 0) return he;
    hipLaunchKernelGGL(particle_scan_kernel, dim3((unsigned)p.n), dim3(256), 0, stream, p.row_start, p.count, p.H);
    return hipGetLastError();
}

hipError_t launch_particle_detect(const ParticleParams& p, hipStream_t stream) { return launch_rows(p, true, stream); }

hipError_t launch_particle_match(const ParticleMatchParams& p, hipStream_t stream) {
    if (p.n <= 0 || p.cap_a <= 0) return hipSuccess;
    if (p.n > 65535 || p.n_rows < 1 || p.n_cols < 1 || p.H < 1 || p.W < 1) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((p.cap_a + 255) / 256), (unsigned)p.n);
    hipLaunchKernelGGL(match_nearest_kernel, grid, dim3(256), 0, stream, p);
    hipLaunchKernelGGL(match_claim_kernel, grid, dim3(256), 0, stream, p);
    hipLaunchKernelGGL(match_verdict_kernel, grid, dim3(256), 0, stream, p);
    return hipGetLastError();
}

}  // namespace tpiv
