// Weighted-window instances of the tile kernel for 16x16, 32x32 and 64x64 windows: pass 1, DWS and CWS.
// Every staged window is multiplied by a separable weight W(y, x) = g_y[y] g_x[x] (a Gaussian, or all ones) in front of the
// forward transform; the cross-correlation, the peak stage and the combine are those of every float32 pass.  Definition, line
// by line: include/torchpiv_hip.h (tpiv_plan_set_weighting); tests/weighting_model.py has the same in numpy.
//
// Same staging, in-register transforms, transposes, paired half inverse and peak stage as xcorr_tile_body (xcorr_tile.hpp,
// fast operation order, work item = (pair, window group), per-XCD work queue); what differs sits between the staging and the
// forward row transform:
//   * the plain window mean is removed first (a' = a - mean a: exactly 0 for a constant integer-valued window), then the
//     W-weighted mean mu = sum W a' / sum W of the remainder, so that the weighted signal W (a' - mu) has no DC -- otherwise
//     the map carries the pedestal W * W centred at zero displacement;
//   * the lane is the window row: it loads g_y[r] once, g_x[k] is a wave-uniform load per register.  Per sample and frame:
//     the subtraction of the mean, one fma for sum_k g_x[k] a'[k], and the weighting (a' - mu) c_k with c_k = g_x[k] x (the
//     lane's g_y[r], pass 1's 1 / mean, the power of two 0.5 / WS that carries the 1 / n^2 of the inverse and the 1 / 4 of the
//     packed cross-spectrum, and the sign of the swap-free 64x64 transposition on odd samples of lanes 32..63);
//   * a window whose weighted energy sum x^2 is exactly 0 in float32 in either frame (zero, masked, constant) is empty: its
//     map is set to exactly 0, and in pass 1 it is dead as a zero-sum window of the plain first pass is.  A CWS window that
//     is constant only up to the rounding of its bilinear samples is NOT empty (as in xcorr_spec.hip).
// Every 64x64 instance runs the swap-free first transposition: the weighting is a multiply per sample here, so the sign
// rides on its constants in the DWS instance too.
// inverse_rows, pass_shift, up_sign / sflip and the dispatch come from xcorr_variant.hpp, which also says why the work loop
// is this unit's own text.
#include "xcorr_variant.hpp"

namespace tpiv {

template <int WS, int MODE, bool PLANAR>
__device__ __forceinline__ void xcorr_win_body(const PassParams& p, const WinParams& s) {
    using G = TileGeo<WS, PLANAR>;
    static_assert(WS == 16 || WS == 32 || WS == 64, "tile sizes of the weighted kernels");
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
    // the lane's row weight, and 1 / sum W = 1 / (sum g_y  sum g_x): the same for every window, kept in a scalar register
    const float* __restrict__ const gxt = s.tab + WS;         // s.tab: g_y[0 .. WS-1], then g_x[0 .. WS-1]
    float gyr, inv_sw;
    {
        const int r0 = fresh_lane() % WS;
        gyr = s.tab[r0];
        const float sy = grp_sum<WS>(gyr), sx = grp_sum<WS>(gxt[r0]);
        inv_sw = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(1.0f / (sy * sx))));
    }

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

        // ---- plain mean, weighted remainder, weighting (the shifted passes' fast staging forms no sums: they are formed here)
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
        bool zero;
        {
            const float ma = sa * (1.0f / (WS * WS)), mb = sb * (1.0f / (WS * WS));
            float wa_ = 0.f, wb_ = 0.f;
            static_for<0, WS>([&](auto kc) TPIV_LAMBDA_INLINE {
                constexpr int k = decltype(kc)::value;
                const float gk = gxt[k];
                x[k].x -= ma;
                x[k].y -= mb;
                wa_ = fmaf(gk, x[k].x, wa_);
                wb_ = fmaf(gk, x[k].y, wb_);
            });
            const float mua = grp_sum<WS>(wa_ * gyr) * inv_sw, mub = grp_sum<WS>(wb_ * gyr) * inv_sw;
            // pass 1 divides by the window mean (B:513-514); a zero-sum window is dead as in the plain first pass
            float ka = 1.f, kb = 1.f;
            bool dead0 = false;
            if constexpr (MODE == MODE_PASS1) {
                dead0 = (sa == 0.f) || (sb == 0.f);
                ka = dead0 ? 0.f : 1.0f / ma;
                kb = dead0 ? 0.f : 1.0f / mb;
            }
            constexpr float PRE = 0.5f / (float)WS;       // 1 / n^2 of the inverse and 1 / 4 of the cross-spectrum algebra: exact
            const unsigned sg = NOSWAP ? up_sign() : 0u;
            const float ta = gyr * (ka * PRE), tb = gyr * (kb * PRE);
            const float ta_o = sflip(ta, sg), tb_o = sflip(tb, sg);
            float ea = 0.f, eb = 0.f;
            static_for<0, WS>([&](auto kc) TPIV_LAMBDA_INLINE {
                constexpr int k = decltype(kc)::value;
                const float gk = gxt[k];
                x[k].x = (x[k].x - mua) * (((k & 1) ? ta_o : ta) * gk);
                x[k].y = (x[k].y - mub) * (((k & 1) ? tb_o : tb) * gk);
                ea = fmaf(x[k].x, x[k].x, ea);
                eb = fmaf(x[k].y, x[k].y, eb);
            });
            ea = grp_sum<WS>(ea);
            eb = grp_sum<WS>(eb);
            zero = dead0 || (ea == 0.f) || (eb == 0.f);
        }

        // ---- forward 2-D transform of a + i*b: rows in registers, transpose, columns in registers
        fft_inreg<WS, 1>(x, tw);
        transpose_tile<WS, PLANAR, NOSWAP>(x, tile, fresh_lane());
        fft_inreg<WS, 1>(x, tw);

        float crow[WS];
        inverse_rows<WS, PLANAR, NOSWAP, true>(x, tile, tw, CrossPlain{},
                                               [&](auto&, int) TPIV_LAMBDA_INLINE { return zero; }, crow);      // no filter
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
__global__ __launch_bounds__(64, OCC) void xcorr_win_kernel(PassParams p, WinParams s) {
    xcorr_win_body<WS, MODE, PLANAR>(p, s);
}

// Wavefronts per SIMD and LDS layout per instance (profiles/weighting/kernel_resources.txt; none uses scratch):
//   16x16: four wavefronts, complex tiles, full inverse (as the production instances); CWS: THREE -- built for four it sits
//     at the 128-VGPR cap with 100 bytes of scratch
//   32x32: three wavefronts, planar tiles and the paired half inverse (as production)
//   64x64 pass 1 / DWS: TWO wavefronts (production: three), planar tiles and the paired half inverse -- built for three they
//     sit at the 168-VGPR cap with 328 / 236 bytes of scratch
//   64x64 CWS: TWO wavefronts, complex tiles, full inverse (production's full kernel; no fast-path / list split): 248 VGPRs
//     (the spectral instance needs one wavefront: nothing of the filter's two sweeps is held here)
template <int WS, int MODE>
struct WinCfg {
    static constexpr int OCC = WS == 16 ? (MODE == MODE_CWS ? 3 : 4) : (WS == 32 ? 3 : 2);
    static constexpr bool PLANAR = WS == 16 ? false : (WS == 32 ? true : MODE != MODE_CWS);
};

int win_occ(int ws, int mode) { return cfg_occ<WinCfg>(ws, mode); }
bool win_planar(int ws, int mode) { return cfg_planar<WinCfg>(ws, mode); }

// one weighted pass up to its peak records; p.work_ctr zeroed by the caller (piv_launch.hip: launch_xcorr_win)
hipError_t launch_xcorr_win_tile(const PassParams& p, int mode, const WinParams& s, int n_cu, hipStream_t stream) {
    return for_ws_mode(p.ws, mode, hipErrorInvalidValue, [&](auto w, auto m) {
        constexpr int WS = decltype(w)::value, MODE = decltype(m)::value;
        using C = WinCfg<WS, MODE>;
        return launch_variant_tile<WS>(xcorr_win_kernel<WS, MODE, C::OCC, C::PLANAR>, p, s, n_cu, stream);
    });
}

}  // namespace tpiv
