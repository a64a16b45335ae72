// Ensemble (sum-of-correlation) instances of the tile kernel for 16x16, 32x32 and 64x64 windows: pass 1, DWS and CWS.
// (Meinhart, Wereley & Santiago, J. Fluids Eng. 122 (2000) 285: add the correlation maps of all pairs of a recording
// window by window and take the peak of the summed map once.)
//
// Same staging, in-register transforms and transposes as xcorr_tile_body (xcorr_tile.hpp, fast operation order), with the
// inverse_rows, pass_shift and dispatch of xcorr_variant.hpp; the work loop is this unit's own, and the peak stage is
// replaced by an epilogue that adds the raw map into acc float32 [N, ws, ws], fftshift layout:
//   * a work item is a window GROUP (64 / WS windows), not a (pair, group): the wavefront that takes a group owns its
//     accumulator rows for the whole launch and loops over the pairs of the launch in ascending order.  No atomics, one
//     owner per cell: the same sequence of launches gives the same bits.
//   * REGSUM (16x16, 32x32, 64x64 pass 1 / DWS): the pair sum T = C_0 + C_1 + ... stays in WS registers per lane (lane =
//     map row) and acc is touched once per launch, acc <- acc + T, with 16-byte loads and stores.
//     !REGSUM (64x64 CWS, whose staging alone needs 230 VGPRs): the lane adds its row to acc once per pair inside the pair
//     loop -- still one owner per cell and deterministic; the rows stay in L2 between the pairs of an item.
//   * the predictor of a shifted pass is one field for all pairs: indexed by window only.
//   * raw map: what peak_analysis would receive, with the constant factor of the fast shifted order (1/4 n^2, a power of
//     two) applied -- before any minimum subtraction and before the 1e-7.  A pass-1 window whose pixel sum is 0 in either
//     frame is transformed as zeros (ka = kb = 0 below) and so contributes the zero map.
#include "xcorr_variant.hpp"

namespace tpiv {

template <int WS, int MODE, bool PLANAR, bool REGSUM>
__device__ __forceinline__ void xcorr_ens_body(const PassParams& p, float* __restrict__ acc) {
    using G = TileGeo<WS, PLANAR>;
    static_assert(WS == 16 || WS == 32 || WS == 64, "tile sizes of the ensemble kernels");
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
    const int items = (N + G::WPW - 1) / G::WPW;          // window groups: < 2^31 (checked by the launcher)
    const int st = p.ws - p.ov;
    const int B = p.batch;

    // per-XCD work queue over the groups (see xcorr_tile_body): one dequeue per group, i.e. per B pairs
    const int xcd = blockIdx.x & 7;
    const int chunk = (int)(((long long)items + 7) / 8);
    const int lo = __builtin_amdgcn_readfirstlane(xcd * chunk < items ? xcd * chunk : items);
    const int hi = __builtin_amdgcn_readfirstlane(items - lo > chunk ? lo + chunk : items);
    unsigned* const ctr = p.work_ctr + xcd * 16;
    auto q_issue = [&]() TPIV_LAMBDA_INLINE -> unsigned {
        unsigned v = 0;
        if (fresh_lane() == 0) v = atomicAdd(ctr, 1u);
        return v;
    };
    auto q_take = [&](unsigned q_raw) TPIV_LAMBDA_INLINE -> int {
        const unsigned v = (unsigned)__builtin_amdgcn_readfirstlane((int)q_raw);
        return v < (unsigned)(hi - lo) ? lo + (int)v : hi;
    };
    // per-lane geometry of (group, pair); fidx indexes the SHARED predictor: window only
    auto geom_of = [&](int item, int pair, int w) TPIV_LAMBDA_INLINE {
        ItemGeom g;
        g.pair = pair;
        const int win_raw = item * G::WPW + w;
        g.active = win_raw < N ? 1 : 0;
        g.win = g.active ? win_raw : N - 1;
        const int wrow = fast_div(g.win, p.ncols_magic, p.ncols_shift);
        g.y0 = wrow * st;
        g.x0 = (g.win - wrow * p.n_cols) * st;
        g.fidx = (size_t)g.win;
        return g;
    };

    int item = q_take(q_issue());
    if (item >= hi) return;
    int nitem = q_take(q_issue());
    float vx, vy;
    RawRows<WS, MODE> raw;
    CoopOff<WS> coff;
    if constexpr (MODE == MODE_CWS) coff.init(fresh_lane() % WS, p.W);
    {
        const int l0 = fresh_lane();
        const ItemGeom g0 = geom_of(item, 0, l0 / WS);
        pass_shift<MODE>(p, g0, vx, vy);
        issue_rows<WS, MODE, FAST>(p, g0, l0 % WS, vx, vy, raw, coff);
    }

    constexpr bool FASTN = MODE != MODE_PASS1;
    constexpr bool NOSWAP = WS == 64 && MODE != MODE_DWS;
    constexpr float END_SCALE = FASTN ? 0.25f / (float)(WS * WS) : 1.0f;      // a power of two: exact

    // the lane's accumulator row (fftshift layout), or nullptr for the idle window slots of the last group
    auto acc_row = [&](int item_) TPIV_LAMBDA_INLINE -> float4* {
        const int lane_e = fresh_lane();
        const int win_raw = item_ * G::WPW + lane_e / WS;
        int ys = ((lane_e % WS) + WS / 2) % WS;
        asm volatile("" : "+v"(ys));                     // opaque: keeps the store addresses out of the loop's registers
        return win_raw < N ? reinterpret_cast<float4*>(acc + ((size_t)win_raw * WS + ys) * WS) : nullptr;
    };
    // row[k] (un-shifted column k) into the accumulator row: acc[x'] += row[(x' + WS/2) % WS]
    auto add_row = [&](float4* d, const float (&row)[WS]) TPIV_LAMBDA_INLINE {
        if (d != nullptr) {
            static_for<0, WS / 4>([&](auto qc) TPIV_LAMBDA_INLINE {
                constexpr int q = decltype(qc)::value;
                float4 t = d[q];
                t.x += row[(4 * q + 0 + WS / 2) % WS];
                t.y += row[(4 * q + 1 + WS / 2) % WS];
                t.z += row[(4 * q + 2 + WS / 2) % WS];
                t.w += row[(4 * q + 3 + WS / 2) % WS];
                d[q] = t;
            });
        }
    };

    for (int nnitem; item < hi; item = nitem, nitem = nnitem) {
        const unsigned q_raw = q_issue();
        float sum[REGSUM ? WS : 1];
        if constexpr (REGSUM) {
#pragma unroll
            for (int k = 0; k < WS; ++k) sum[k] = 0.0f;
        }
        for (int pr = 0; pr < B; ++pr) {
            const int lane = fresh_lane();
            const int w = lane / WS;
            const int r = lane % WS;
            const ItemGeom g = geom_of(item, pr, w);
            // the step after this one: the next pair of the group, or pair 0 of the next group (the last step of the
            // launch simply re-loads its own rows: no branch around the prefetch)
            const bool last = pr == B - 1;
            const int nit = last ? (nitem < hi ? nitem : item) : item;
            const int npr = last ? 0 : pr + 1;
            const ItemGeom gnext = geom_of(nit, npr, w);
            float nvx, nvy;
            pass_shift<MODE>(p, gnext, nvx, nvy);

            cf x[WS];
            float sa, sb;
            convert_rows<WS, MODE, RBH, FAST, false, 0>(p, g, r, lane, vx, vy, raw, x, sa, sb, tile);
            if constexpr (WS <= 32) issue_rows<WS, MODE, FAST>(p, gnext, r, nvx, nvy, raw, coff);

            if constexpr (!FASTN) {
                // pass 1: (x - mean) / mean, with the 0.5 / WS of the transform pair folded in (xcorr_tile_body)
                sa = grp_sum<WS>(sa);
                sb = grp_sum<WS>(sb);
                const float ma = sa * (1.0f / (WS * WS)), mb = sb * (1.0f / (WS * WS));
                const bool dead = (sa == 0.f) || (sb == 0.f);      // zero window: transformed as zeros -> the zero map
                const float ka = dead ? 0.f : 1.0f / ma;
                const float kb = dead ? 0.f : 1.0f / mb;
                constexpr float PRE = 0.5f / (float)WS;
                const float oa = -ma * ka, ob = -mb * kb;
                const float kas = ka * PRE, kbs = kb * PRE, oas = oa * PRE, obs = ob * PRE;
                const unsigned sg = NOSWAP ? up_sign() : 0u;
                const float kao = sflip(kas, sg), kbo = sflip(kbs, sg), oao = sflip(oas, sg), obo = sflip(obs, sg);
#pragma unroll
                for (int k = 0; k < WS; ++k) {
                    x[k].x = (k & 1) ? fmaf(x[k].x, kao, oao) : fmaf(x[k].x, kas, oas);
                    x[k].y = (k & 1) ? fmaf(x[k].y, kbo, obo) : fmaf(x[k].y, kbs, obs);
                }
            } else if constexpr (NOSWAP) {
                const unsigned sg = up_sign();
#pragma unroll
                for (int k = 1; k < WS; k += 2) {
                    x[k].x = sflip(x[k].x, sg);
                    x[k].y = sflip(x[k].y, sg);
                }
            }

            fft_inreg<WS, 1>(x, tw);
            if constexpr (FASTN) {      // the window mean leaves in the DC bin of the row transform (xcorr_tile_body)
                constexpr int P0 = FFT_POS<0, WS>;
                if constexpr (NOSWAP) {
                    constexpr int PH = FFT_POS<WS / 2, WS>;
                    const bool up = up_sign() != 0u;
                    const float ta = grp_sum<WS>(up ? x[PH].x : x[P0].x);
                    const float tb = grp_sum<WS>(up ? x[PH].y : x[P0].y);
                    x[P0].x -= up ? 0.0f : ta * (1.0f / WS);
                    x[P0].y -= up ? 0.0f : tb * (1.0f / WS);
                    x[PH].x -= up ? ta * (1.0f / WS) : 0.0f;
                    x[PH].y -= up ? tb * (1.0f / WS) : 0.0f;
                } else {
                    const float ta = grp_sum<WS>(x[P0].x);
                    const float tb = grp_sum<WS>(x[P0].y);
                    x[P0].x -= ta * (1.0f / WS);
                    x[P0].y -= tb * (1.0f / WS);
                }
            }
            transpose_tile<WS, PLANAR, NOSWAP>(x, tile, fresh_lane());
            fft_inreg<WS, 1>(x, tw);

            float crow[WS];
            inverse_rows<WS, PLANAR, NOSWAP, false>(x, tile, tw, CrossPlain{},
                                                    [](auto&, int) TPIV_LAMBDA_INLINE { return false; }, crow);      // no filter
            wave_sync();                                  // tile reads done: the next step's staging may use it

            if constexpr (WS > 32) {
                const int lane_p = fresh_lane();
                issue_rows<WS, MODE, FAST>(p, geom_of(nit, npr, lane_p / WS), lane_p % WS, nvx, nvy, raw, coff);
            }
            vx = nvx;
            vy = nvy;

            // ---- epilogue: the raw map of this pair joins the sum
            if constexpr (FASTN) {
#pragma unroll
                for (int k = 0; k < WS; ++k) crow[k] *= END_SCALE;
            }
            if constexpr (REGSUM) {
#pragma unroll
                for (int k = 0; k < WS; ++k) sum[k] += crow[k];
            } else {
                add_row(acc_row(item), crow);
            }
        }
        if constexpr (REGSUM) add_row(acc_row(item), sum);
        nnitem = q_take(q_raw);
    }
}

template <int WS, int MODE, int OCC, bool PLANAR, bool REGSUM>
__global__ __launch_bounds__(64, OCC) void xcorr_ens_kernel(PassParams p, float* acc) {
    xcorr_ens_body<WS, MODE, PLANAR, REGSUM>(p, acc);
}

// Wavefronts per SIMD, LDS layout and where the pair sum lives, per instance (profiles/ensemble/kernel_resources.txt):
//   16x16: four wavefronts, complex tiles, sum in registers (as the production instances + 16 VGPRs); CWS: THREE -- its
//     production instance sits at the 128-VGPR cap of four, and the 16 registers of the sum would go to scratch
//   32x32: three wavefronts, planar tiles and the paired half inverse, sum in registers (+ 32 VGPRs inside the 168 cap)
//   64x64 pass 1 / DWS: TWO wavefronts (production: three) so that the 64 registers of the sum fit without scratch; planar
//     tiles and the paired half inverse as in production
//   64x64 CWS: two wavefronts, complex tiles (production's full kernel); its row joins acc once per pair
template <int WS, int MODE>
struct EnsCfg {
    static constexpr int OCC = WS == 16 ? (MODE == MODE_CWS ? 3 : 4) : (WS == 32 ? 3 : 2);
    static constexpr bool PLANAR = WS == 16 ? false : (WS == 32 ? true : MODE != MODE_CWS);
    static constexpr bool REGSUM = !(WS == 64 && MODE == MODE_CWS);
};

template <int WS, int MODE>
static hipError_t launch_ens(const PassParams& p_in, float* acc, int n_cu, hipStream_t stream) {
    using G = TileGeo<WS>;
    using C = EnsCfg<WS, MODE>;
    PassParams p = p_in;
    const long long N = (long long)p.n_rows * p.n_cols;
    const long long groups = (N + G::WPW - 1) / G::WPW;
    if (groups <= 0 || groups >= (1ll << 31) - 64 || p.batch < 1) return hipErrorInvalidValue;
    fast_div_setup((unsigned)groups, p.groups_magic, p.groups_shift);
    fast_div_setup((unsigned)p.n_cols, p.ncols_magic, p.ncols_shift);
    const long long cap = (long long)n_cu * 4 * C::OCC;        // the resident set: every wavefront pulls groups until none is left
    const long long blocks = groups < cap ? groups : cap;
    hipLaunchKernelGGL((xcorr_ens_kernel<WS, MODE, C::OCC, C::PLANAR, C::REGSUM>), dim3((unsigned)((blocks + 7) / 8 * 8)),
                       dim3(64), 0, stream, p, acc);
    return hipGetLastError();
}

// acc [N, ws, ws] += the raw maps of p.batch pairs; p.work_ctr zeroed by the caller (piv_launch.hip: launch_ensemble_add)
hipError_t launch_xcorr_ens(const PassParams& p, int mode, float* acc, int n_cu, hipStream_t stream) {
    return for_ws_mode(p.ws, mode, hipErrorInvalidValue, [&](auto w, auto m) {
        return launch_ens<decltype(w)::value, decltype(m)::value>(p, acc, n_cu, stream);
    });
}

// ---- peak stage on accumulated maps: M = acc / n (one float32 division per cell), then peak_analysis as in production
template <int WS, bool PLANAR>
__global__ __launch_bounds__(64, 2) void peak_ens_kernel(PassParams p, const float* __restrict__ acc, int n_maps, float n_pairs) {
    using G = TileGeo<WS, PLANAR>;
    __shared__ float tile[G::LDS_FLOATS];
    const int lane = threadIdx.x;
    const int w = lane / WS, r = lane % WS;
    const int win_raw = blockIdx.x * G::WPW + w;
    const bool active = win_raw < n_maps;
    const int win = active ? win_raw : n_maps - 1;
    float crow[WS];
    const int ys = (r + WS / 2) % WS;
    const float4* __restrict__ src = reinterpret_cast<const float4*>(acc + ((size_t)win * WS + ys) * WS);
    static_for<0, WS / 4>([&](auto qc) TPIV_LAMBDA_INLINE {
        constexpr int q = decltype(qc)::value;
        const float4 t = src[q];
        crow[(4 * q + 0 + WS / 2) % WS] = __fdiv_rn(t.x, n_pairs);
        crow[(4 * q + 1 + WS / 2) % WS] = __fdiv_rn(t.y, n_pairs);
        crow[(4 * q + 2 + WS / 2) % WS] = __fdiv_rn(t.z, n_pairs);
        crow[(4 * q + 3 + WS / 2) % WS] = __fdiv_rn(t.w, n_pairs);
    });
    peak_analysis<WS, PLANAR>(p, crow, tile, w, r, active, false, (size_t)win);
}

hipError_t launch_peak_ens(const PassParams& p, const float* acc, int n_maps, long long n_pairs, hipStream_t stream) {
    if (n_maps < 1 || n_pairs < 1 || n_pairs > (1ll << 24)) return hipErrorInvalidValue;      // n exact in float32
    const float nf = (float)n_pairs;
    switch (p.ws) {
        case 16:
            hipLaunchKernelGGL((peak_ens_kernel<16, false>), dim3((n_maps + 3) / 4), dim3(64), 0, stream, p, acc, n_maps, nf);
            break;
        case 32:
            hipLaunchKernelGGL((peak_ens_kernel<32, false>), dim3((n_maps + 1) / 2), dim3(64), 0, stream, p, acc, n_maps, nf);
            break;
        case 64:
            hipLaunchKernelGGL((peak_ens_kernel<64, false>), dim3(n_maps), dim3(64), 0, stream, p, acc, n_maps, nf);
            break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace tpiv
