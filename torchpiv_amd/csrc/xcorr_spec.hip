// Spectrally filtered instances of the tile kernel for 16x16, 32x32 and 64x64 windows: pass 1, DWS and CWS.
// Phase-only correlation and robust phase correlation (Eckstein & Vlachos, Meas. Sci. Technol. 20 (2009) 055401): the
// cross-spectrum P of a window pair is divided by its own magnitude, floored at tau = floor x mean |P|, and weighted with the
// spectrum W of the expected particle-image correlation; the peak of the inverse of Q = W P / max(|P|, tau) is taken as in
// every other pass.  Definition, line by line: include/torchpiv_hip.h (tpiv_plan_set_correlation); tests/phase_model.py has
// the same in numpy.
//
// Same staging, in-register transforms, transposes and peak stage as xcorr_tile_body (xcorr_tile.hpp, fast operation order,
// work item = (pair, window group), per-XCD work queue); what differs:
//   * every pass removes the window mean in front of the transform and divides by nothing: Q is invariant to a scale factor
//     in either frame, and the mean-free energies sum (a - mean a)^2, sum (b - mean b)^2 decide whether the window is empty
//     (a zero, masked or constant window: both spectra of such a pair are rounding noise, which the filter would raise to
//     full weight) -- an empty window gets Q = 0, i.e. the zero map, and in pass 1 the dead flag of a zero-sum window.
//     The test is exact equality with 0 in float32: exact for integer-valued staged windows (pass 1, DWS, zeroed or masked
//     pixels, and a CWS window of a constant region, whose lerp a + w (b - a) returns the constant).  A CWS window that is
//     constant only up to rounding (the reference-order per-pixel staging of border windows can produce one) is NOT empty:
//     its map is the filtered rounding noise, and only the peak ratio rejects it;
//   * spec_filter() sits between the cross-spectrum and the inverse column transform.  The lane is kx, the register index ky:
//     the lane loads g_x[|kx|] once, g_y[|ky|] is a wave-uniform load per register.  The packed spectrum holds 4 P, and the
//     sign the swap-free 64x64 transposition leaves on odd bins is undone inside cross(): the lane's value IS 4 P, its
//     magnitude 4 |P|, and with tau formed from the mean of those magnitudes the factor 4 leaves
//     Q = W (4P) / max(|4P|, floor mean |4P|).  cross() forms 4 P from the separated spectra (see there): the filter
//     divides by |P|, so the products must be accurate relative to |A| |B|, not to |A|^2 + |B|^2;
//     In the paired half inverse a lane holds ky = 0 .. WS/2 of column kx and its mirror lane the conjugates of the rest:
//     the mean counts ky = 0 and WS/2 once and the others twice, and both lanes of a pair apply the same W (W is even);
//   * the inverse transform is the unnormalised one: a pure circular shift peaks at sum W.
// Every 64x64 instance runs the swap-free first transposition: the mean removal is an fma per sample here, so the sign of
// the odd samples of lanes 32..63 rides on its constants in the DWS instance too.
// inverse_rows, pass_shift, up_sign / sflip and the dispatch come from xcorr_variant.hpp, which also says why the work loop
// is this unit's own text.
#include "xcorr_variant.hpp"

namespace tpiv {

// Q = W P / max(|P|, tau) on the lane's bins, in place.  NB = WS: b[ky] = P(ky, kx) for every ky (full inverse); NB = WS/2 + 1:
// ky = 0 .. WS/2 (paired half inverse: the bins 1 .. WS/2 - 1 stand for their mirror images in the partner lane as well).
// r_c: the lane's kx.  empty: the window has no mean-free energy in one of the frames.  Returns "Q is zero everywhere".
// (Kept a device function of its own so that the ensemble body can take it.)
template <int WS, int NB>
__device__ __forceinline__ bool spec_filter(cf (&b)[NB], const SpecParams& s, int r_c, bool empty) {
    constexpr int M = WS / 2;
    constexpr bool HALF = NB == M + 1;
    static_assert(HALF || NB == WS, "all bins of the column, or its first half with the Nyquist bin");
    const float* __restrict__ gy = s.tab;                 // g_y[0 .. WS/2], then g_x[0 .. WS/2]
    const float* __restrict__ gx = s.tab + (M + 1);
    const float wx = gx[r_c <= M ? r_c : WS - r_c];
    float acc = 0.0f;
    static_for<0, NB>([&](auto kc) TPIV_LAMBDA_INLINE {
        constexpr int k = decltype(kc)::value;
        const float mag = __builtin_amdgcn_sqrtf(b[k].x * b[k].x + b[k].y * b[k].y);
        acc += (HALF && k != 0 && k != M) ? 2.0f * mag : mag;
    });
    const float tot = grp_sum<WS>(acc);
    const float tau = s.floor * (tot * (1.0f / (float)(WS * WS)));
    const bool zero = empty || !(tot > 0.0f);
    // (finite: a bin that is exactly 0 has rsq = inf, takes this side of the minimum and stays 0)
    const float inv_tau = zero ? 0.0f : fminf(1.0f / tau, 3.0e38f);
    static_for<0, NB>([&](auto kc) TPIV_LAMBDA_INLINE {
        constexpr int k = decltype(kc)::value;
        constexpr int ka = k <= M ? k : WS - k;
        const float p2 = b[k].x * b[k].x + b[k].y * b[k].y;
        const float n = fminf(__builtin_amdgcn_rsqf(p2), inv_tau) * (gy[ka] * wx);
        b[k].x *= n;
        b[k].y *= n;
    });
    return zero;
}

// 4 conj(A) B of the packed transform Z = A + iB, from the separated spectra: with zk = Z(k) = a + ib and zm = Z(-k) =
// c + id,  a + c = 2 Re A,  b - d = 2 Im A,  b + d = 2 Re B,  c - a = 2 Im B.  The plain passes form the same number as
// re = 2 (ad + bc), im = (c^2 - a^2) + (d^2 - b^2) (CrossPlain), whose large terms cancel where |A| and |B| differ:
// an ABSOLUTE error of u (|A|^2 + |B|^2) per bin, nothing to a correlation sum, but divided by |P| = |A| |B| here.
// sg (+-1): the sign the swap-free 64x64 transposition leaves on the odd bins of exactly one of zk, zm (inverse_rows);
// applied to zm, both are the true values or both negated, and every product below is the same.
struct CrossSeparated {
    static constexpr float EVEN = 1.0f;
    __device__ __forceinline__ cf operator()(cf zk, cf zm, float sg) const {
        const float ar2 = fmaf(zm.x, sg, zk.x), br2 = fmaf(zm.y, sg, zk.y);
        const float ai2 = fmaf(-zm.y, sg, zk.y), bi2 = fmaf(zm.x, sg, -zk.x);
        cf pr_;
        pr_.x = fmaf(ar2, br2, ai2 * bi2);
        pr_.y = fmaf(ar2, bi2, -(ai2 * br2));
        return pr_;
    }
};

template <int WS, int MODE, bool PLANAR>
__device__ __forceinline__ void xcorr_spec_body(const PassParams& p, const SpecParams& s) {
    using G = TileGeo<WS, PLANAR>;
    static_assert(WS == 16 || WS == 32 || WS == 64, "tile sizes of the spectral kernels");
    constexpr bool FAST = true;
    constexpr int RBH = 64 * (WS + 1) <= G::LDS_FLOATS ? 1 : 2;      // slow-path row buffer pieces
    static_assert(MODE == MODE_PASS1 || 64 * (WS / RBH + 1) <= G::LDS_FLOATS,
                  "slow-path row buffer (shifted passes) must fit the tile LDS");
    constexpr int LDSF = (MODE == MODE_CWS && CoopGeo<WS>::LDS_FLOATS > G::LDS_FLOATS)
                             ? CoopGeo<WS>::LDS_FLOATS : G::LDS_FLOATS;
    __shared__ __attribute__((aligned(16))) float tile[LDSF];

    using TW = std::conditional_t<WS == 16, TwRegs<WS>, TwLiteral>;
    TW tw;
    if constexpr (!std::is_same<TW, TwLiteral>::value) tw.init();

    const int N = p.n_rows * p.n_cols;
    const int groups = (N + G::WPW - 1) / G::WPW;
    const int items = p.batch * groups;                   // < 2^31 (checked by the launcher)
    const int st = p.ws - p.ov;

    // per-XCD work queue over (pair, group) items, as in xcorr_tile_body
    constexpr int QCH = WS <= 16 ? 4 : 1;
    const int xcd = blockIdx.x & 7;
    const int chunk = (int)(((long long)items + 7) / 8);
    const int lo = __builtin_amdgcn_readfirstlane(xcd * chunk < items ? xcd * chunk : items);
    const int hi = __builtin_amdgcn_readfirstlane(items - lo > chunk ? lo + chunk : items);
    unsigned* const ctr = p.work_ctr + xcd * 16;
    int q_base = 0;
    int q_left = 0;
    auto q_issue = [&]() TPIV_LAMBDA_INLINE -> unsigned {
        unsigned v = 0;
        if (QCH == 1 || q_left == 0) {
            if (fresh_lane() == 0) v = atomicAdd(ctr, (unsigned)QCH);
        }
        return v;
    };
    auto q_take = [&](unsigned q_raw) TPIV_LAMBDA_INLINE -> int {
        if (QCH == 1 || q_left == 0) {
            const unsigned v = (unsigned)__builtin_amdgcn_readfirstlane((int)q_raw);
            q_base = v < (unsigned)(hi - lo) ? lo + (int)v : hi;
            q_left = QCH;
        }
        const int it = q_base + (QCH - q_left);
        --q_left;
        return it;
    };
    auto geom_of = [&](int item, int w) TPIV_LAMBDA_INLINE {
        ItemGeom g;
        g.pair = fast_div(item, p.groups_magic, p.groups_shift);
        const int gi = item - g.pair * groups;
        const int win_raw = gi * G::WPW + w;
        g.active = win_raw < N ? 1 : 0;
        g.win = g.active ? win_raw : N - 1;
        const int wrow = fast_div(g.win, p.ncols_magic, p.ncols_shift);
        g.y0 = wrow * st;
        g.x0 = (g.win - wrow * p.n_cols) * st;
        g.fidx = (size_t)g.pair * N + g.win;
        return g;
    };

    int item = q_take(q_issue());
    if (item >= hi) return;
    int nitem = q_take(q_issue());
    constexpr bool RECOMPUTE = WS >= 32;
    float vx, vy;
    RawRows<WS, MODE> raw;
    ItemGeom gcur;
    CoopOff<WS> coff;
    if constexpr (MODE == MODE_CWS) coff.init(fresh_lane() % WS, p.W);
    {
        const int l0 = fresh_lane();
        gcur = geom_of(item, l0 / WS);
        pass_shift<MODE>(p, gcur, vx, vy);
        issue_rows<WS, MODE, FAST>(p, gcur, l0 % WS, vx, vy, raw, coff);
    }

    constexpr bool NOSWAP = WS == 64;

    for (int nnitem; item < hi; item = nitem, nitem = nnitem) {
        const unsigned q_raw = q_issue();
        const int lane = fresh_lane();
        const int w = lane / WS;
        const int r = lane % WS;
        const ItemGeom g = RECOMPUTE ? geom_of(item, w) : gcur;
        const bool active = g.active != 0;
        const size_t fidx = g.fidx;
        const int nit = nitem < hi ? nitem : item;
        const ItemGeom gnext = geom_of(nit, w);
        float nvx, nvy;
        pass_shift<MODE>(p, gnext, nvx, nvy);

        cf x[WS];
        float sa, sb;
        convert_rows<WS, MODE, RBH, FAST, false, 0>(p, g, r, lane, vx, vy, raw, x, sa, sb, tile);
        if constexpr (WS >= 64) nnitem = q_take(q_raw);
        if constexpr (WS <= 32) issue_rows<WS, MODE, FAST>(p, gnext, r, nvx, nvy, raw, coff);

        if (p.dbg_win != nullptr && active) {     // test hook: the staged (shifted) windows
            int rr = r;
            asm volatile("" : "+v"(rr));
            float* d = p.dbg_win + fidx * 2 * WS * WS + rr * WS;
#pragma unroll
            for (int k = 0; k < WS; ++k) {
                d[k] = x[k].x;
                d[WS * WS + k] = x[k].y;
            }
        }

        // ---- mean removal in front of the transform (the shifted passes' fast staging forms no sums: they are formed here),
        //      the sign of the swap-free transposition on the same fma, and the mean-free energies
        if constexpr (MODE != MODE_PASS1) {
            sa = 0.f;
            sb = 0.f;
#pragma unroll
            for (int k = 0; k < WS; ++k) {
                sa += x[k].x;
                sb += x[k].y;
            }
        }
        sa = grp_sum<WS>(sa);
        sb = grp_sum<WS>(sb);
        bool empty;
        {
            const float ma = sa * (1.0f / (WS * WS)), mb = sb * (1.0f / (WS * WS));
            const unsigned sg = NOSWAP ? up_sign() : 0u;
            const float one_o = sflip(1.0f, sg), nma = -ma, nmb = -mb, nma_o = sflip(nma, sg), nmb_o = sflip(nmb, sg);
            float ea = 0.f, eb = 0.f;
#pragma unroll
            for (int k = 0; k < WS; ++k) {
                x[k].x = (k & 1) ? fmaf(x[k].x, one_o, nma_o) : x[k].x + nma;
                x[k].y = (k & 1) ? fmaf(x[k].y, one_o, nmb_o) : x[k].y + nmb;
                ea = fmaf(x[k].x, x[k].x, ea);
                eb = fmaf(x[k].y, x[k].y, eb);
            }
            ea = grp_sum<WS>(ea);
            eb = grp_sum<WS>(eb);
            empty = (ea == 0.f) || (eb == 0.f);
        }

        // ---- forward 2-D transform of a + i*b: rows in registers, transpose, columns in registers
        fft_inreg<WS, 1>(x, tw);
        transpose_tile<WS, PLANAR, NOSWAP>(x, tile, fresh_lane());
        fft_inreg<WS, 1>(x, tw);

        float crow[WS];
        const bool zero = inverse_rows<WS, PLANAR, NOSWAP, false>(
            x, tile, tw, CrossSeparated{},
            [&](auto& bins, int r_c) TPIV_LAMBDA_INLINE { return spec_filter<WS>(bins, s, r_c, empty); }, crow);
        wave_sync();                                  // tile reads done: it becomes the map

        if constexpr (WS > 32) {
            const int lane_p = fresh_lane();
            issue_rows<WS, MODE, FAST>(p, geom_of(nit, lane_p / WS), lane_p % WS, nvx, nvy, raw, coff);
        }
        vx = nvx;
        vy = nvy;
        if constexpr (!RECOMPUTE) gcur = gnext;

        // pass 1: an empty window is dead as a zero-sum window of the plain first pass is; a shifted pass hands its zero map
        // to the peak stage, whose peak ratio makes it invalid
        const bool dead = MODE == MODE_PASS1 && zero;
        if constexpr (RECOMPUTE) {
            const int lane_e = fresh_lane();
            const int w_e = lane_e / WS, r_e = lane_e % WS;
            const int pair_e = fast_div(item, p.groups_magic, p.groups_shift);
            const int win_raw_e = (item - pair_e * groups) * G::WPW + w_e;
            const bool active_e = win_raw_e < N;
            const int win_e = active_e ? win_raw_e : N - 1;
            const size_t fidx_e = (size_t)pair_e * N + win_e;
            peak_analysis<WS, PLANAR, false>(p, crow, tile, w_e, r_e, active_e, dead, fidx_e);
        } else {
            peak_analysis<WS, PLANAR, false>(p, crow, tile, w, r, active, dead, fidx);
        }
        wave_sync();
        if constexpr (WS < 64) nnitem = q_take(q_raw);
    }
}

template <int WS, int MODE, int OCC, bool PLANAR>
__global__ __launch_bounds__(64, OCC) void xcorr_spec_kernel(PassParams p, SpecParams s) {
    xcorr_spec_body<WS, MODE, PLANAR>(p, s);
}

// Wavefronts per SIMD and LDS layout per instance (profiles/phase/kernel_resources.txt; none uses scratch):
//   16x16: four wavefronts, complex tiles, full inverse (as the production instances); CWS: THREE -- built for four it
//     sits at the 128-VGPR cap with 8 bytes of scratch
//   32x32: three wavefronts, planar tiles and the paired half inverse (as production)
//   64x64 pass 1 / DWS: TWO wavefronts (production: three), planar tiles and the paired half inverse: 176 / 180 VGPRs, above
//     the 168 of three
//   64x64 CWS: ONE wavefront, complex tiles, full inverse (production's full kernel; no fast-path / list split): its staging
//     alone needs 230 VGPRs, and with the filter's two sweeps over the 64 products the 256 of two leave 28 bytes of scratch
template <int WS, int MODE>
struct SpecCfg {
    static constexpr int OCC = WS == 16 ? (MODE == MODE_CWS ? 3 : 4) : (WS == 32 ? 3 : (MODE == MODE_CWS ? 1 : 2));
    static constexpr bool PLANAR = WS == 16 ? false : (WS == 32 ? true : MODE != MODE_CWS);
};

int spec_occ(int ws, int mode) { return cfg_occ<SpecCfg>(ws, mode); }
bool spec_planar(int ws, int mode) { return cfg_planar<SpecCfg>(ws, mode); }

// one filtered pass up to its peak records; p.work_ctr zeroed by the caller (piv_launch.hip: launch_xcorr_spec)
hipError_t launch_xcorr_spec_tile(const PassParams& p, int mode, const SpecParams& s, int n_cu, hipStream_t stream) {
    return for_ws_mode(p.ws, mode, hipErrorInvalidValue, [&](auto w, auto m) {
        constexpr int WS = decltype(w)::value, MODE = decltype(m)::value;
        using C = SpecCfg<WS, MODE>;
        return launch_variant_tile<WS>(xcorr_spec_kernel<WS, MODE, C::OCC, C::PLANAR>, p, s, n_cu, stream);
    });
}

}  // namespace tpiv
