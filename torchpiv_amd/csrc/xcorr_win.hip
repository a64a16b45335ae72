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
// The production instances of xcorr_tile.hpp and the spectral ones of xcorr_spec.hip are not touched: this body is separate.
#include "xcorr_tile.hpp"

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
    auto shift_of = [&](const ItemGeom& g, float& vx, float& vy) TPIV_LAMBDA_INLINE {
        if constexpr (MODE == MODE_PASS1) {
            vx = 0.f;
            vy = 0.f;
        } else if constexpr (MODE == MODE_CWS) {
            pred_half_shift_cws_f32(p, g.fidx, vx, vy);
        } else {
            double sx, sy;
            pred_half_shift<MODE>(p, g.fidx, sx, sy);
            vx = (float)sx;
            vy = (float)sy;
        }
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
        shift_of(gcur, vx, vy);
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
    auto up_sign = []() TPIV_LAMBDA_INLINE { return fresh_lane() >= 32 ? 0x80000000u : 0u; };
    auto sflip = [](float v, unsigned sg) TPIV_LAMBDA_INLINE { return __uint_as_float(__float_as_uint(v) ^ sg); };

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
        shift_of(gnext, nvx, nvy);

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

        constexpr bool HALF_INV = PLANAR && (WS == 32 || WS == 64);
        float crow[WS];
        // 4 P = conj(2A) (2B) of the packed transform Z = A + iB, as xcorr_tile_body forms it: with zk = Z(k) = a + ib and
        // zm = Z(-k) = c + id,  re = 2 (a d + b c),  im = (c^2 - a^2) + (d^2 - b^2).  two (+-2): the sign the swap-free 64x64
        // transposition leaves on the odd bins of exactly one of zk, zm (`two_odd` of xcorr_tile_body).
        auto cross = [&](cf zk, cf zm, float two) TPIV_LAMBDA_INLINE {
            const float a_ = zk.x, b_ = zk.y, c_ = zm.x, d_ = zm.y;
            cf pr_;
            pr_.x = (a_ * d_ + b_ * c_) * two;
            pr_.y = (c_ * c_ - a_ * a_) + (d_ * d_ - b_ * b_);
            return pr_;
        };
        if constexpr (HALF_INV) {
            constexpr int M = WS / 2;
            cf h[M];
            {
                const int lane_c = fresh_lane();
                const int r_c = lane_c % WS;
                const int partner = (lane_c - r_c) + ((WS - r_c) % WS);
                const float two_odd = (NOSWAP && (lane_c & 31) != 0) ? -2.0f : 2.0f;
                cf pc[M + 1];
                static_for<0, M + 1>([&](auto kc) TPIV_LAMBDA_INLINE {
                    constexpr int ky = decltype(kc)::value;
                    constexpr int nky = (WS - ky) % WS;
                    const cf z2 = x[FFT_POS<nky, WS>];
                    cf m1;
                    m1.x = __shfl(z2.x, partner, 64);
                    m1.y = __shfl(z2.y, partner, 64);
                    pc[ky] = cross(x[FFT_POS<ky, WS>], m1, (ky & 1) ? two_odd : 2.0f);
                });
                const bool odd = r_c > M;
                const float fs = (r_c == 0 || r_c == M) ? 1.0f : 0.0f;
                static_for<0, M>([&](auto kc) TPIV_LAMBDA_INLINE {
                    constexpr int k = decltype(kc)::value;
                    cf pr_;
                    pr_.x = __shfl(pc[M - k].x, partner, 64);
                    pr_.y = __shfl(pc[M - k].y, partner, 64);
                    const cf sm{pc[k].x + pr_.x, pc[k].y - pr_.y};
                    const cf tt = twmul<k, WS, -1>(cf{pc[k].x - pr_.x, pc[k].y + pr_.y});
                    h[k].x = odd ? tt.x : __builtin_fmaf(-fs, tt.y, sm.x);
                    h[k].y = odd ? tt.y : __builtin_fmaf(fs, tt.x, sm.y);
                });
            }
            fft_inreg<M, -1>(h, tw);
            cf hs[M + 1], z[M];
            transpose_half_pairs<WS, PLANAR>(h, hs, tile, fresh_lane());
            c2r_inreg<WS>(hs, z);
            static_for<0, WS>([&](auto xc) TPIV_LAMBDA_INLINE {
                constexpr int x_ = decltype(xc)::value;
                const float c_ = (x_ & 1) ? z[FFT_POS<x_ / 2, M>].y : z[FFT_POS<x_ / 2, M>].x;
                crow[x_] = zero ? 0.0f : c_;
            });
        } else {
            cf t[WS];
            {
                const int lane_c = fresh_lane();
                const int r_c = lane_c % WS;
                const int partner = (lane_c - r_c) + ((WS - r_c) % WS);
                const float two_odd = (NOSWAP && (lane_c & 31) != 0) ? -2.0f : 2.0f;
                static_for<0, WS / 2 + 1>([&](auto kc) TPIV_LAMBDA_INLINE {
                    constexpr int ky = decltype(kc)::value;
                    constexpr int nky = (WS - ky) % WS;
                    constexpr int p1 = FFT_POS<ky, WS>, p2 = FFT_POS<nky, WS>;
                    const float two = (ky & 1) ? two_odd : 2.0f;
                    const cf z1 = x[p1];
                    if constexpr (ky == nky) {
                        cf m1;
                        m1.x = __shfl(z1.x, partner, 64);
                        m1.y = __shfl(z1.y, partner, 64);
                        t[ky] = cross(z1, m1, two);
                    } else {
                        const cf z2 = x[p2];
                        cf m1, m2;
                        m1.x = __shfl(z2.x, partner, 64);
                        m1.y = __shfl(z2.y, partner, 64);
                        m2.x = __shfl(z1.x, partner, 64);
                        m2.y = __shfl(z1.y, partner, 64);
                        t[ky] = cross(z1, m1, two);
                        t[nky] = cross(z2, m2, two);
                    }
                });
            }
            fft_inreg<WS, -1>(t, tw);
            cf hs[WS / 2 + 1], z[WS / 2];
            transpose_half<WS, PLANAR>(t, hs, tile, fresh_lane());
            c2r_inreg<WS>(hs, z);
            static_for<0, WS>([&](auto xc) TPIV_LAMBDA_INLINE {
                constexpr int x_ = decltype(xc)::value;
                const float c_ = (x_ & 1) ? z[FFT_POS<x_ / 2, WS / 2>].y : z[FFT_POS<x_ / 2, WS / 2>].x;
                crow[x_] = zero ? 0.0f : c_;
            });
        }
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

int win_occ(int ws, int mode) {
    switch (ws) {
        case 16: return mode == MODE_CWS ? WinCfg<16, MODE_CWS>::OCC : (mode == MODE_DWS ? WinCfg<16, MODE_DWS>::OCC : WinCfg<16, MODE_PASS1>::OCC);
        case 32: return mode == MODE_CWS ? WinCfg<32, MODE_CWS>::OCC : (mode == MODE_DWS ? WinCfg<32, MODE_DWS>::OCC : WinCfg<32, MODE_PASS1>::OCC);
        case 64: return mode == MODE_CWS ? WinCfg<64, MODE_CWS>::OCC : (mode == MODE_DWS ? WinCfg<64, MODE_DWS>::OCC : WinCfg<64, MODE_PASS1>::OCC);
        default: return 0;
    }
}
bool win_planar(int ws, int mode) { return ws == 32 || (ws == 64 && mode != MODE_CWS); }

template <int WS, int MODE>
static hipError_t launch_win(const PassParams& p_in, const WinParams& s, int n_cu, hipStream_t stream) {
    using C = WinCfg<WS, MODE>;
    static_assert(C::PLANAR == (WS == 32 || (WS == 64 && MODE != MODE_CWS)), "win_planar names the layout");
    PassParams p = p_in;
    const unsigned blocks = tile_grid<WS>(p, n_cu);
    if (blocks == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL((xcorr_win_kernel<WS, MODE, C::OCC, C::PLANAR>), dim3(blocks), dim3(64), 0, stream, p, s);
    return hipGetLastError();
}

template <int WS>
static hipError_t launch_win_ws(const PassParams& p, int mode, const WinParams& s, int n_cu, hipStream_t stream) {
    switch (mode) {
        case MODE_PASS1: return launch_win<WS, MODE_PASS1>(p, s, n_cu, stream);
        case MODE_DWS: return launch_win<WS, MODE_DWS>(p, s, n_cu, stream);
        case MODE_CWS: return launch_win<WS, MODE_CWS>(p, s, n_cu, stream);
        default: return hipErrorInvalidValue;
    }
}

// one weighted pass up to its peak records; p.work_ctr zeroed by the caller (piv_launch.hip: launch_xcorr_win)
hipError_t launch_xcorr_win_tile(const PassParams& p, int mode, const WinParams& s, int n_cu, hipStream_t stream) {
    switch (p.ws) {
        case 16: return launch_win_ws<16>(p, mode, s, n_cu, stream);
        case 32: return launch_win_ws<32>(p, mode, s, n_cu, stream);
        case 64: return launch_win_ws<64>(p, mode, s, n_cu, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace tpiv
