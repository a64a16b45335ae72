// In-register (per-lane) complex FFT codelets for the PIV tile kernels.
//
// One lane holds a whole line of N complex samples in registers (N = 8..128)
// and transforms it with compile-time-unrolled radix-4 (first stage radix-2
// when log2 N is odd) butterflies, in one of two forms: butterfly-first
// (decimation in frequency, fft_dif) or twiddle-first (decimation in time,
// fft_twf; fewer instructions).  All array indices
// and twiddles are compile-time constants, so the array lives in VGPRs and the
// trivial twiddles (1, -i, -1, i) cost nothing.  The output is left in
// digit-reversed order: output bin k sits at fft_pos(k, N), in either form.
//
// The header also compiles as plain host C++ (tests/test_host_logic.py::test_fft_codelets_on_host builds
// it with g++ and checks it against numpy.fft).
#pragma once
#include <type_traits>

#if defined(__HIPCC__)
#define TPIV_HD __host__ __device__ __forceinline__
#else
#define TPIV_HD inline
#endif
// the bodies handed to static_for must be inlined, or the register arrays they touch get
// their address taken and end up in scratch memory
#define TPIV_LAMBDA_INLINE __attribute__((always_inline))

namespace tpiv {

#include "twiddles.inc"

struct cf {
    float x, y;
};

// Test-only switch (tools/diag/libtorchpiv_hip_mutant_tw.so, tests/test_gpu_shifted_maps.py): -DTPIV_MUTANT_TWIDDLE=eps scales
// the first non-trivial twiddle w_N^1 of every codelet (fft_inreg.hpp, fft_mixed.hpp, the run-time table of the mixed-radix
// generic kernel) by 1 + eps, and the plain DFT's table entry w_n^1 by 1 + 100 eps (xcorr_generic.hip).  Values only: no
// index, no branch changes.  The shipped library never defines it (the factor is then 1, and the code is the same
// instruction for instruction).
#ifdef TPIV_MUTANT_TWIDDLE
constexpr bool MUT_TW_ON = true;
constexpr float MUT_TW = (float)(1.0 + (double)(TPIV_MUTANT_TWIDDLE));
constexpr float MUT_TW_PLAIN = (float)(1.0 + 100.0 * (double)(TPIV_MUTANT_TWIDDLE));     // xcorr_generic_kernel's table
#else
constexpr bool MUT_TW_ON = false;
constexpr float MUT_TW = 1.0f;
#endif
// (the factor of twiddle w_N^K: MUT_TW for K = 1 mod N, else 1)
template <int K, int N>
constexpr float mut_tw() { return (((K % N) + N) % N == 1) ? MUT_TW : 1.0f; }

TPIV_HD cf cadd(cf a, cf b) { return cf{a.x + b.x, a.y + b.y}; }
TPIV_HD cf csub(cf a, cf b) { return cf{a.x - b.x, a.y - b.y}; }

constexpr bool radix2_first(int n) { return n == 2 || n == 8 || n == 32 || n == 128; }

// register position of output bin k after the size-n DIF transform
constexpr int fft_pos(int k, int n) {
    if (n <= 1) return 0;
    if (radix2_first(n)) return (k % 2) * (n / 2) + fft_pos(k / 2, n / 2);
    return (k % 4) * (n / 4) + fft_pos(k / 4, n / 4);
}

// compile-time constant form: indexing a register array with fft_pos(k, n) directly would
// leave a run-time call to the (recursive) function and push the array into scratch
template <int K, int N>
inline constexpr int FFT_POS = fft_pos(K, N);

template <int J, int END, typename F>
TPIV_HD void static_for(F&& f) {
    if constexpr (J < END) {
        f(std::integral_constant<int, J>{});
        static_for<J + 1, END>(f);
    }
}

// a * exp(-DIR * 2*pi*i * K / N)   (DIR = +1 forward, -1 inverse)
template <int K, int N, int DIR>
TPIV_HD cf twmul(cf a) {
    constexpr int idx = ((K % N) * (128 / N)) % 128;
    if constexpr (idx == 0) {
        return a;
    } else if constexpr (idx == 32) {
        return DIR > 0 ? cf{a.y, -a.x} : cf{-a.y, a.x};
    } else if constexpr (idx == 64) {
        return cf{-a.x, -a.y};
    } else if constexpr (idx == 96) {
        return DIR > 0 ? cf{-a.y, a.x} : cf{a.y, -a.x};
    } else {
        constexpr float c = TW_COS[idx] * mut_tw<K, N>();
        constexpr float s = (DIR > 0 ? -TW_SIN[idx] : TW_SIN[idx]) * mut_tw<K, N>();
        return cf{a.x * c - a.y * s, a.x * s + a.y * c};
    }
}

// ---- where the twiddle constants live ------------------------------------------------------------
// TwLiteral: as 32-bit literals inside the instructions (8-byte encodings; a constant used by several
// instructions is moved to an SGPR by the compiler, and an SGPR operand halves the issue rate on
// MI355X).  TwRegs<NTOP>: the N/4 - 1 non-trivial first-quadrant magnitudes cos(2 pi k / NTOP) and
// their negatives in VGPRs, so that every twiddle product is a plain 4-byte v_mul_f32 / v_fmac_f32.
struct TwLiteral {};

template <int NTOP>
struct TwRegs {
    static constexpr int STEP = 128 / NTOP;             // stride in the 128-entry table
    static constexpr int NV = NTOP / 4 - 1;             // table entries STEP, 2 STEP, ..., 32 - STEP
    float pos[NV > 0 ? NV : 1], neg[NV > 0 ? NV : 1];
    TPIV_HD void init() {
        static_for<0, NV>([&](auto ic) TPIV_LAMBDA_INLINE {
            constexpr int i = decltype(ic)::value;
            pos[i] = TW_COS[(i + 1) * STEP];
            neg[i] = -TW_COS[(i + 1) * STEP];
#if defined(__HIP_DEVICE_COMPILE__)
            asm volatile("" : "+v"(pos[i]), "+v"(neg[i]));      // opaque: stays a register operand
#endif
        });
    }
    template <int R, bool NEG>
    TPIV_HD float m() const {                            // (+-) cos(2 pi R / 128), R a multiple of STEP in 1..31
        static_assert(R % STEP == 0 && R > 0 && R < 32, "not a twiddle of this transform");
        return NEG ? neg[R / STEP - 1] : pos[R / STEP - 1];
    }
};

// the constants of w = exp(-DIR * 2*pi*i * K / N) = C + i S (non-trivial K only) and -S, from either twiddle source
template <int K, int N, int DIR, typename TW>
TPIV_HD void tw_consts(const TW& tw, float& C, float& S, float& nS) {
    constexpr int idx = ((K % N) * (128 / N)) % 128;
    static_assert(idx % 32 != 0, "trivial twiddles take no constants");
    if constexpr (std::is_same<TW, TwLiteral>::value) {
        constexpr float c = TW_COS[idx] * mut_tw<K, N>();
        constexpr float s = (DIR > 0 ? -TW_SIN[idx] : TW_SIN[idx]) * mut_tw<K, N>();
        C = c;
        S = s;
        nS = -s;
    } else {
        // cos = (+-) M[rc], sin = (+-) M[rs] with M[r] = cos(2 pi r / 128) = sin(2 pi (32 - r) / 128)
        constexpr int q = idx / 32, r = idx % 32;
        constexpr int rc = (q % 2 == 0) ? r : 32 - r;
        constexpr int rs = (q % 2 == 0) ? 32 - r : r;
        constexpr bool cneg = (q == 1 || q == 2);
        constexpr bool sneg0 = (q == 2 || q == 3);
        constexpr bool sneg = DIR > 0 ? !sneg0 : sneg0;   // multiply by exp(-DIR * i * theta)
        C = tw.template m<rc, cneg>();
        S = tw.template m<rs, sneg>();
        nS = tw.template m<rs, !sneg>();
        if constexpr (MUT_TW_ON && mut_tw<K, N>() != 1.0f) {
            C *= MUT_TW;
            S *= MUT_TW;
            nS *= MUT_TW;
        }
    }
}

TPIV_HD float fma_f(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_fmaf(a, b, c);
#else
    return a * b + c;
#endif
}

// w b with its fma written out, either twiddle source
template <int K, int N, int DIR, typename TW>
TPIV_HD cf twmul_f(cf b, const TW& tw) {
    constexpr int idx = ((K % N) * (128 / N)) % 128;
    if constexpr (idx % 32 == 0) {
        return twmul<K, N, DIR>(b);
    } else {
        float C, S, nS;
        tw_consts<K, N, DIR>(tw, C, S, nS);
        return cf{fma_f(b.y, nS, b.x * C), fma_f(b.y, C, b.x * S)};
    }
}

// the twiddle product of the butterfly-first form: literals go through twmul, whose multiply-adds the backend contracts (kept as
// it is: the units on that form stay instruction for instruction what they were), register constants through twmul_f
template <int K, int N, int DIR, typename TW>
TPIV_HD cf twmul_t(cf a, const TW& tw) {
    if constexpr (std::is_same<TW, TwLiteral>::value) {
        return twmul<K, N, DIR>(a);
    } else {
        return twmul_f<K, N, DIR>(a, tw);
    }
}

template <int N, int OFF, int DIR, int TOTAL, typename TW = TwLiteral>
struct FFTStage {
    static TPIV_HD void run(cf (&x)[TOTAL], const TW& tw = TW{}) {
        if constexpr (N == 2) {
            cf a = x[OFF], b = x[OFF + 1];
            x[OFF] = cadd(a, b);
            x[OFF + 1] = csub(a, b);
        } else if constexpr (radix2_first(N)) {
            static_for<0, N / 2>([&](auto jc) TPIV_LAMBDA_INLINE {
                constexpr int j = decltype(jc)::value;
                cf a = x[OFF + j], b = x[OFF + j + N / 2];
                x[OFF + j] = cadd(a, b);
                x[OFF + j + N / 2] = twmul_t<j, N, DIR>(csub(a, b), tw);
            });
            FFTStage<N / 2, OFF, DIR, TOTAL, TW>::run(x, tw);
            FFTStage<N / 2, OFF + N / 2, DIR, TOTAL, TW>::run(x, tw);
        } else if constexpr (N >= 4) {
            static_for<0, N / 4>([&](auto jc) TPIV_LAMBDA_INLINE {
                constexpr int j = decltype(jc)::value;
                cf a = x[OFF + j], b = x[OFF + j + N / 4], c = x[OFF + j + N / 2],
                   d = x[OFF + j + 3 * N / 4];
                cf t0 = cadd(a, c), t1 = csub(a, c), t2 = cadd(b, d), bd = csub(b, d);
                // forward: t3 = -i (b - d); inverse: t3 = +i (b - d)
                cf t3 = DIR > 0 ? cf{bd.y, -bd.x} : cf{-bd.y, bd.x};
                x[OFF + j] = cadd(t0, t2);
                x[OFF + j + N / 4] = twmul_t<j, N, DIR>(cadd(t1, t3), tw);
                x[OFF + j + N / 2] = twmul_t<2 * j, N, DIR>(csub(t0, t2), tw);
                x[OFF + j + 3 * N / 4] = twmul_t<3 * j, N, DIR>(csub(t1, t3), tw);
            });
            if constexpr (N > 4) {
                FFTStage<N / 4, OFF, DIR, TOTAL, TW>::run(x, tw);
                FFTStage<N / 4, OFF + N / 4, DIR, TOTAL, TW>::run(x, tw);
                FFTStage<N / 4, OFF + N / 2, DIR, TOTAL, TW>::run(x, tw);
                FFTStage<N / 4, OFF + 3 * N / 4, DIR, TOTAL, TW>::run(x, tw);
            }
        }
    }
};

// The butterfly-first (decimation-in-frequency) form above: additions, then the twiddle products of the outputs.
template <int N, int DIR, typename TW>
TPIV_HD void fft_dif(cf (&x)[N], const TW& tw) {
    FFTStage<N, 0, DIR, N, TW>::run(x, tw);
}

// ---- twiddle-first (decimation-in-time) form ---------------------------------------------------------
// The same radix plan read from the other end: the N-point transform of x is combined from the N/4-point (N/2-point at a
// radix-2 level) transforms Y_m of the samples x[4n + m], with the twiddles w = w_N^k IN FRONT of the butterfly, where the
// butterfly's additions ride on the multiply-adds:
//   a + w b                   two nested fma per component
//   a - w b = 2a - (a + w b)  one fma per component (2.0f is an inline constant)
// A twiddled radix-2 butterfly is 6 instructions instead of 8, a radix-4 one 24 instead of 28.  Every fma is written out
// (__builtin_fmaf; a plain expression of the same order on the host), so the form does not depend on what the backend
// contracts.  Trivial twiddles (1, -+i, -1) keep the plain addition and subtraction.  Rounding: DESIGN.md 3.4b.
//
// The sub-transforms come back in natural order and each level writes its results where it likes -- after unrolling every
// value is its own SSA name -- so the top level puts bin k into x[FFT_POS<k, N>], the register the form above leaves it in.

// p = a + w b,  q = a - w b,  w = exp(-DIR * 2*pi*i * K / N)
template <int K, int N, int DIR, typename TW>
TPIV_HD void tw_butterfly(cf a, cf b, const TW& tw, cf& p, cf& q) {
    constexpr int idx = ((K % N) * (128 / N)) % 128;
    if constexpr (idx % 32 == 0) {
        const cf wb = twmul<K, N, DIR>(b);
        p = cadd(a, wb);
        q = csub(a, wb);
    } else {
        float C, S, nS;
        tw_consts<K, N, DIR>(tw, C, S, nS);
        p = cf{fma_f(b.x, C, fma_f(b.y, nS, a.x)), fma_f(b.x, S, fma_f(b.y, C, a.y))};
        q = cf{fma_f(2.0f, a.x, -p.x), fma_f(2.0f, a.y, -p.y)};
    }
}

// y[k] = bin k (natural order) of the N-point transform of x[OFF + STRIDE * n], n = 0 .. N-1; x is only read
template <int N, int OFF, int STRIDE, int DIR, int TOTAL, typename TW>
struct FFTTwFirst {
    static TPIV_HD void run(const cf (&x)[TOTAL], cf (&y)[N], const TW& tw) {
        if constexpr (N == 1) {
            y[0] = x[OFF];
        } else if constexpr (N == 2) {
            const cf a = x[OFF], b = x[OFF + STRIDE];
            y[0] = cadd(a, b);
            y[1] = csub(a, b);
        } else if constexpr (radix2_first(N)) {
            cf y0[N / 2], y1[N / 2];
            FFTTwFirst<N / 2, OFF, 2 * STRIDE, DIR, TOTAL, TW>::run(x, y0, tw);
            FFTTwFirst<N / 2, OFF + STRIDE, 2 * STRIDE, DIR, TOTAL, TW>::run(x, y1, tw);
            static_for<0, N / 2>([&](auto kc) TPIV_LAMBDA_INLINE {
                constexpr int k = decltype(kc)::value;
                tw_butterfly<k, N, DIR>(y0[k], y1[k], tw, y[k], y[k + N / 2]);
            });
        } else {
            cf y0[N / 4], y1[N / 4], y2[N / 4], y3[N / 4];
            // sub-transform by sub-transform in the order of m, so that inputs die early.  (Measured on the 64x64 unit's
            // register allocation: the order 0, 2, 1, 3 and asm pins behind each sub-transform both spill more.)
            FFTTwFirst<N / 4, OFF, 4 * STRIDE, DIR, TOTAL, TW>::run(x, y0, tw);
            FFTTwFirst<N / 4, OFF + STRIDE, 4 * STRIDE, DIR, TOTAL, TW>::run(x, y1, tw);
            FFTTwFirst<N / 4, OFF + 2 * STRIDE, 4 * STRIDE, DIR, TOTAL, TW>::run(x, y2, tw);
            FFTTwFirst<N / 4, OFF + 3 * STRIDE, 4 * STRIDE, DIR, TOTAL, TW>::run(x, y3, tw);
            static_for<0, N / 4>([&](auto kc) TPIV_LAMBDA_INLINE {
                constexpr int k = decltype(kc)::value;
                cf t0, t1, t2, t3;
                tw_butterfly<2 * k, N, DIR>(y0[k], y2[k], tw, t0, t1);                               // Y0 +- w^2k Y2
                tw_butterfly<3 * k, N, DIR>(twmul_f<k, N, DIR>(y1[k], tw), y3[k], tw, t2, t3);      // w^k Y1 +- w^3k Y3
                // forward: -i t3; inverse: +i t3
                const cf r3 = DIR > 0 ? cf{t3.y, -t3.x} : cf{-t3.y, t3.x};
                y[k] = cadd(t0, t2);
                y[k + N / 4] = cadd(t1, r3);
                y[k + N / 2] = csub(t0, t2);
                y[k + 3 * N / 4] = csub(t1, r3);
            });
        }
    }
};

template <int N, int DIR, typename TW>
TPIV_HD void fft_twf(cf (&x)[N], const TW& tw) {
    cf y[N];
    FFTTwFirst<N, 0, 1, DIR, N, TW>::run(x, y, tw);
    static_for<0, N>([&](auto kc) TPIV_LAMBDA_INLINE {
        constexpr int k = decltype(kc)::value;
        x[FFT_POS<k, N>] = y[k];
    });
}

// Which form a translation unit's fft_inreg / c2r_inreg calls run: the 64x64 and 32x32 tile units (xcorr_ws64, xcorr_ws32,
// xcorr_ws32c) define TPIV_FFT_TWIDDLE_FIRST in front of their includes; every other unit keeps the butterfly-first form
// (DESIGN.md 3.1).  A template argument, not a second body under one name: the two choices are two functions.
#ifdef TPIV_FFT_TWIDDLE_FIRST
constexpr bool FFT_TWIDDLE_FIRST = true;
#else
constexpr bool FFT_TWIDDLE_FIRST = false;
#endif

// Unnormalised N-point transform of x[0..N) in place; bin k ends at x[fft_pos(k, N)].
template <int N, int DIR, bool TWF = FFT_TWIDDLE_FIRST>
TPIV_HD void fft_inreg(cf (&x)[N]) {
    if constexpr (TWF) fft_twf<N, DIR>(x, TwLiteral{});
    else FFTStage<N, 0, DIR, N>::run(x);
}
// the same with the twiddle constants taken from `tw` (TwRegs<N>, or TwLiteral{} for the form above)
template <int N, int DIR, typename TW, bool TWF = FFT_TWIDDLE_FIRST>
TPIV_HD void fft_inreg(cf (&x)[N], const TW& tw) {
    if constexpr (TWF) fft_twf<N, DIR>(x, tw);
    else FFTStage<N, 0, DIR, N, TW>::run(x, tw);
}

// (Used by the tile kernels for WS <= 32: same-box A/B 2.4 % (32x32 CWS pass) to 5.8 % (32x32 pass 1)
//  faster than the full complex transform; 64x64 is at its register limit and keeps the complex form.)
// Real N-point inverse transform of a Hermitian spectrum through ONE N/2-point complex transform
// (the classic even/odd packing): in  Y[k], k = 0..N/2 (natural order; the imaginary parts of the
// DC and Nyquist bins are ignored, as in any c2r transform); out  r[2m] = h[fft_pos(m, N/2)].x,
// r[2m+1] = h[fft_pos(m, N/2)].y  with  r[n] = sum_k Y[k] exp(+2 pi i k n / N)  (unnormalised).
// With z[m] = r[2m] + i r[2m+1]:  z = IDFT_{N/2}(G),  G[k] = (Y[k] + conj Y[M-k]) + i w^k (Y[k] - conj Y[M-k]),
// w = exp(2 pi i / N), M = N/2; the pair (k, M-k) shares S = Y[k] + conj Y[M-k], T = w^k (Y[k] - conj Y[M-k]):
// G[k] = S + i T,  G[M-k] = conj(S) + i conj(T).
template <int N, bool TWF = FFT_TWIDDLE_FIRST>
TPIV_HD void c2r_inreg(const cf (&Y)[N / 2 + 1], cf (&h)[N / 2]) {
    constexpr int M = N / 2;
    static_assert(M >= 2, "N >= 4");
    h[0] = cf{Y[0].x + Y[M].x, Y[0].x - Y[M].x};
    static_for<1, M / 2>([&](auto kc) TPIV_LAMBDA_INLINE {
        constexpr int k = decltype(kc)::value;
        const cf A = Y[k], B = Y[M - k];
        const cf S{A.x + B.x, A.y - B.y};
        const cf T = twmul<k, N, -1>(cf{A.x - B.x, A.y + B.y});
        h[k] = cf{S.x - T.y, S.y + T.x};
        h[M - k] = cf{S.x + T.y, T.x - S.y};
    });
    h[M / 2] = cf{2.0f * Y[M / 2].x, -2.0f * Y[M / 2].y};
    fft_inreg<M, -1, TWF>(h);
}

}  // namespace tpiv
