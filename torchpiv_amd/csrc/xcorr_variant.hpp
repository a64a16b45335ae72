// What the variant units of the tile kernel share: xcorr_spec.hip (spectrally filtered passes), xcorr_win.hip (weighted
// windows) and xcorr_ens.hip (ensemble correlation), each for 16x16, 32x32 and 64x64 windows in pass 1, DWS and CWS.
//
// All three keep the staging, the in-register transforms, the transposes and the paired half inverse of xcorr_tile_body
// (xcorr_tile.hpp) in its fast operation order, with the per-XCD work queue.  xcorr_tile_body itself is deliberately NOT a
// client of this header: the production units build with their own scheduler flags and compile to the same objects with or
// without it.
//
//   inverse_rows       cross-spectrum -> paired half inverse (planar 32x32 / 64x64 tiles) or full inverse -> c2r -> the
//                      lane's map row.  Used by all three units.
//   pass_shift, up_sign, sflip, CrossPlain: small shared device pieces.
//   for_ws_mode, cfg_occ / cfg_planar, launch_variant_tile: from (ws, mode) to an instance, on the host.
//
// Each unit keeps its own work loop.  The ensemble unit's items are window groups with an inner pair loop.  The spectral and
// the weighted unit share the text of their loop over (pair, window group) items but not a function: with the step between
// staging and forward transform behind a call of its own, the optimiser orders the operands of ten twiddle sums of the
// first 64x64 row transform of the CWS instances the other way round, the backend fuses the other product of each into its
// fma, and the fields of those two instances change in their last bits (profiles/variant_body/README.md).  That step stays
// in the body's own text until twmul (fft_inreg.hpp) writes its fused form out.
//
// Every 64x64 instance of the spectral and the weighted unit runs the swap-free first transposition (NOSWAP): their
// pre-transform step touches every sample anyway, so the sign of the odd samples of lanes 32..63 rides on its constants in
// the DWS instance too.  (The ensemble unit's DWS instance has no such step and keeps the swapping transposition.)
//
// An empty window (zero, masked, constant) is found by exact equality of a float32 energy with 0: exact for integer-valued
// staged windows (pass 1, DWS, zeroed or masked pixels, and a CWS window of a constant region, whose lerp a + w (b - a)
// returns the constant).  A CWS window that is constant only up to rounding (the reference-order per-pixel staging of
// border windows can produce one) is NOT empty.  In pass 1 an empty window is dead as a zero-sum window of the plain first
// pass is; a shifted pass hands its zero map to the peak stage, whose peak ratio makes it invalid.
#pragma once
#include "xcorr_tile.hpp"

namespace tpiv {

// half the predictor's displacement of the item's window: what the staging of a shifted pass moves the two windows by
template <int MODE>
__device__ __forceinline__ void pass_shift(const PassParams& p, const ItemGeom& g, float& vx, float& vy) {
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
}

// the sign bit the swap-free 64x64 transposition wants on the odd samples of lanes 32..63, and its application
__device__ __forceinline__ unsigned up_sign() { return fresh_lane() >= 32 ? 0x80000000u : 0u; }
__device__ __forceinline__ float sflip(float v, unsigned sg) { return __uint_as_float(__float_as_uint(v) ^ sg); }

// x: the packed 2-D transform Z = A + iB of a window pair, lane = kx, register FFT_POS<ky> = ky.  crow: the lane's row of the
// (unnormalised) inverse of the cross-spectrum.  Returns what filter returned.
//   cross(zk, zm, c)   the product of the bin from zk = Z(k) and zm = Z(-k) (fetched from the mirror lane).  c is Cross::EVEN on
//                      even ky and on odd ky carries the sign the swap-free 64x64 transposition leaves on the odd bins of
//                      exactly one of zk, zm: -EVEN in lanes other than 0 and 32, EVEN elsewhere.  The plain re / im form
//                      takes c = +-2 as its factor, the separated-spectra form c = +-1 as a sign: no extra multiply.
//   filter(bins, r_c)  acts on the lane's products in place in front of the inverse column transform and returns "the map is
//                      zero".  r_c: the lane's kx.  Paired half inverse: bins = ky 0 .. WS/2 (the bins 1 .. WS/2 - 1 stand
//                      for their mirror images in the partner lane as well); full inverse: every ky.
//   ZERO_MAP           the returned flag forces the row to exactly 0.
// The full inverse writes the products straight into the column transform's input (one form serves all three units).
template <int WS, bool PLANAR, bool NOSWAP, bool ZERO_MAP, class TW, class Cross, class Filter>
__device__ __forceinline__ bool inverse_rows(cf (&x)[WS], float* tile, TW& tw, Cross cross, Filter filter, float (&crow)[WS]) {
    constexpr bool HALF_INV = PLANAR && (WS == 32 || WS == 64);
    constexpr int M = WS / 2;
    constexpr float c_even = Cross::EVEN;
    bool zero;
    cf hs[M + 1], z[M];
    if constexpr (HALF_INV) {
        cf h[M];
        {
            const int lane_c = fresh_lane();
            const int r_c = lane_c % WS;
            const int partner = (lane_c - r_c) + ((WS - r_c) % WS);
            const float c_odd = (NOSWAP && (lane_c & 31) != 0) ? -c_even : c_even;
            cf pc[M + 1];
            static_for<0, M + 1>([&](auto kc) TPIV_LAMBDA_INLINE {
                constexpr int ky = decltype(kc)::value;
                constexpr int nky = (WS - ky) % WS;
                const cf z2 = x[FFT_POS<nky, WS>];
                cf m1;
                m1.x = __shfl(z2.x, partner, 64);
                m1.y = __shfl(z2.y, partner, 64);
                pc[ky] = cross(x[FFT_POS<ky, WS>], m1, (ky & 1) ? c_odd : c_even);
            });
            zero = filter(pc, r_c);
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
        transpose_half_pairs<WS, PLANAR>(h, hs, tile, fresh_lane());
    } else {
        cf t[WS];
        {
            const int lane_c = fresh_lane();
            const int r_c = lane_c % WS;
            const int partner = (lane_c - r_c) + ((WS - r_c) % WS);
            const float c_odd = (NOSWAP && (lane_c & 31) != 0) ? -c_even : c_even;
            static_for<0, M + 1>([&](auto kc) TPIV_LAMBDA_INLINE {
                constexpr int ky = decltype(kc)::value;
                constexpr int nky = (WS - ky) % WS;
                constexpr int p1 = FFT_POS<ky, WS>, p2 = FFT_POS<nky, WS>;
                const float c = (ky & 1) ? c_odd : c_even;
                const cf z1 = x[p1];
                if constexpr (ky == nky) {
                    cf m1;
                    m1.x = __shfl(z1.x, partner, 64);
                    m1.y = __shfl(z1.y, partner, 64);
                    t[ky] = cross(z1, m1, c);
                } else {
                    const cf z2 = x[p2];
                    cf m1, m2;
                    m1.x = __shfl(z2.x, partner, 64);
                    m1.y = __shfl(z2.y, partner, 64);
                    m2.x = __shfl(z1.x, partner, 64);
                    m2.y = __shfl(z1.y, partner, 64);
                    t[ky] = cross(z1, m1, c);
                    t[nky] = cross(z2, m2, c);
                }
            });
            zero = filter(t, r_c);
        }
        fft_inreg<WS, -1>(t, tw);
        transpose_half<WS, PLANAR>(t, hs, tile, fresh_lane());
    }
    c2r_inreg<WS>(hs, z);
    static_for<0, WS>([&](auto xc) TPIV_LAMBDA_INLINE {
        constexpr int x_ = decltype(xc)::value;
        const float c_ = (x_ & 1) ? z[FFT_POS<x_ / 2, M>].y : z[FFT_POS<x_ / 2, M>].x;
        crow[x_] = (ZERO_MAP && zero) ? 0.0f : c_;
    });
    return zero;
}

// 4 P = conj(2A) (2B) of the packed transform Z = A + iB, as xcorr_tile_body forms it: with zk = Z(k) = a + ib and
// zm = Z(-k) = c + id,  re = 2 (a d + b c),  im = (c^2 - a^2) + (d^2 - b^2).  two = +-2 (inverse_rows).
struct CrossPlain {
    static constexpr float EVEN = 2.0f;
    __device__ __forceinline__ cf operator()(cf zk, cf zm, float two) const {
        const float a_ = zk.x, b_ = zk.y, c_ = zm.x, d_ = zm.y;
        cf pr_;
        pr_.x = (a_ * d_ + b_ * c_) * two;
        pr_.y = (c_ * c_ - a_ * a_) + (d_ * d_ - b_ * b_);
        return pr_;
    }
};

// ---- host side: from (ws, mode) to an instance ------------------------------------------------------------------------
// f(integral_constant WS, integral_constant MODE) for the window sizes and modes of the variant kernels; `none` otherwise
template <class R, class F>
static R for_ws_mode(int ws, int mode, R none, F f) {
    auto with_ws = [&](auto wsc) -> R {
        switch (mode) {
            case MODE_PASS1: return f(wsc, std::integral_constant<int, MODE_PASS1>{});
            case MODE_DWS: return f(wsc, std::integral_constant<int, MODE_DWS>{});
            case MODE_CWS: return f(wsc, std::integral_constant<int, MODE_CWS>{});
            default: return none;
        }
    };
    switch (ws) {
        case 16: return with_ws(std::integral_constant<int, 16>{});
        case 32: return with_ws(std::integral_constant<int, 32>{});
        case 64: return with_ws(std::integral_constant<int, 64>{});
        default: return none;
    }
}

// what a Cfg<WS, MODE> struct chose, for the kernel names (piv_launch.hip)
template <template <int, int> class Cfg>
static int cfg_occ(int ws, int mode) {
    return for_ws_mode(ws, mode, 0, [](auto w, auto m) { return Cfg<decltype(w)::value, decltype(m)::value>::OCC; });
}
template <template <int, int> class Cfg>
static bool cfg_planar(int ws, int mode) {
    return for_ws_mode(ws, mode, false, [](auto w, auto m) { return Cfg<decltype(w)::value, decltype(m)::value>::PLANAR; });
}

// one spectral or weighted tile kernel over the grid of the plain tile kernels; s: its second kernel argument
template <int WS, class Kernel, class Arg>
static hipError_t launch_variant_tile(Kernel kernel, const PassParams& p_in, const Arg& s, int n_cu, hipStream_t stream) {
    PassParams p = p_in;
    const unsigned blocks = tile_grid<WS>(p, n_cu);
    if (blocks == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64), 0, stream, p, s);
    return hipGetLastError();
}

}  // namespace tpiv
