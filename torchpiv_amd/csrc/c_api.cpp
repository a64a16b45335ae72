// C ABI of the PIV engine (include/torchpiv_hip.h): argument checking, geometry,
// the predictor's spline operators (host, float64) and the multipass plan.
// Compiled with hipcc as host code; the kernels live in xcorr_ws*.hip / piv_launch.hip.
#include "../../include/torchpiv_hip.h"

#include <hip/hip_runtime.h>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "piv_kernels.h"

namespace {

thread_local std::string g_err;
#ifdef TPIV_STAMPS
unsigned long long* g_stamps = nullptr;      // diagnostic builds (make stamps) only: device buffer for phase stamps
#else
constexpr unsigned long long* g_stamps = nullptr;      // the production library keeps no state
#endif

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

int hip_fail(hipError_t e, const char* what) {
    return fail(TPIV_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(expr)                                   \
    do {                                                \
        hipError_t e_ = (expr);                         \
        if (e_ != hipSuccess) return hip_fail(e_, #expr); \
    } while (0)

// The function-level seam (tpiv_pass1 / tpiv_iter / tpiv_debug_*) works in a caller-provided buffer:
// the library keeps no device state between calls.
int check_work(const void* work, size_t have, size_t need) {
    if (need == 0) return TPIV_OK;
    if (!work || have < need)
        return fail(TPIV_EINVAL, "work buffer too small: need " + std::to_string(need) + " bytes (tpiv_work_bytes), got " +
                                     std::to_string(have));
    return TPIV_OK;
}

// "No output may overlap an input or another output": 0 = none does, 1 = an output overlaps an input, 2 = two outputs
// overlap.  A null or empty span overlaps nothing (the only empty span in use is an absent table, whose pointer is null).
struct Span { const void* p; size_t n; };
int aliased(const Span* in, int n_in, const Span* out, int n_out) {
    auto overlap = [](const Span& x, const Span& y) {
        const char *a = (const char*)x.p, *b = (const char*)y.p;
        return a && b && x.n && y.n && a < b + y.n && b < a + x.n;
    };
    for (int i = 0; i < n_out; ++i) {
        for (int j = 0; j < n_in; ++j)
            if (overlap(out[i], in[j])) return 1;
        for (int j = i + 1; j < n_out; ++j)
            if (overlap(out[i], out[j])) return 2;
    }
    return 0;
}

// 8/16/32/64: tile kernel (xcorr_tile.hpp); 128 pass 1: xcorr_big.hpp; anything else in 2..256 (and
// shifted 128x128 passes): generic-size DFT kernel (xcorr_generic.hip)
bool supported_ws(int ws) { return ws >= 2 && ws <= 256; }

// B:503-507 argument checks, then what the kernels cover
int check_window(int H, int W, int ws, int ov, int val_win) {
    if (ov >= ws) return fail(TPIV_EINVAL, "Overlap has to be smaller than the window_size");
    if (ws > H || ws > W) return fail(TPIV_EINVAL, "window size cannot be larger than the image");
    if (ws <= 0 || ov < 0 || H <= 0 || W <= 0) return fail(TPIV_EINVAL, "non-positive size");
    if (!supported_ws(ws))
        return fail(TPIV_EUNSUPPORTED, "window size must be in 2..256 (got " + std::to_string(ws) + ")");
    // (odd sizes: the generic kernel reproduces the reference's ws x (ws-1) irfft2 map; ws = 1 has no map)
    if (ws % 2 != 0 && ws < 3) return fail(TPIV_EUNSUPPORTED, "window size 1 has an empty correlation map in the reference");
    const bool pow2 = ws == 8 || ws == 16 || ws == 32 || ws == 64 || ws == 128;
    if (val_win < 0 || (pow2 && 2 * val_win >= ws))
        return fail(TPIV_EUNSUPPORTED, "validation half-window must satisfy 2*val_win < window size");
    if (((long long)H + 32) * W >= (1LL << 30)) return fail(TPIV_EUNSUPPORTED, "frame too large");   // 32-bit flat indices
    return TPIV_OK;
}

int n_cu_of_current_device(int* n_cu) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    static thread_local int cached_dev = -1, cached_cu = 0;
    if (cached_dev != dev) {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, dev));
        cached_dev = dev;
        cached_cu = prop.multiProcessorCount;
    }
    *n_cu = cached_cu;
    return TPIV_OK;
}

void field_shape(int H, int W, int ws, int ov, int* nr, int* nc) {
    *nr = (H - ws) / (ws - ov) + 1;
    *nc = (W - ws) / (ws - ov) + 1;
}

// floor division for the (possibly negative) centring shift of B:582-592
long long floordiv(long long a, long long b) {
    long long q = a / b, r = a % b;
    return (r != 0 && ((r < 0) != (b < 0))) ? q - 1 : q;
}

void coords_1d(int size, int n, int ws, int ov, double* out) {
    const long long shift = floordiv((long long)size - 1 - ((long long)(n - 1) * (ws - ov) + (ws - 1)), 2);
    for (int i = 0; i < n; ++i) out[i] = (double)i * (ws - ov) + ws / 2.0 + (double)shift;
}

// ---- cubic B-spline interpolation operator (FITPACK regrid, s = 0) -------------
// knots: 4x x[0], x[2..n-3], 4x x[n-1]  (not-a-knot at x[1] and x[n-2])
struct Bspl {
    std::vector<long double> t;
    int n;
    explicit Bspl(int n_, const double* x) : t(n_ + 4), n(n_) {
        for (int i = 0; i < 4; ++i) t[i] = x[0];
        for (int i = 2; i <= n - 3; ++i) t[i + 2] = x[i];
        for (int i = 0; i < 4; ++i) t[n + i] = x[n - 1];
    }
    // span l with t[l] <= xx < t[l+1], 3 <= l <= n-1; the 4 non-zero cubic B-splines
    // N_{l-3..l}(xx) by the de Boor-Cox recurrence
    int eval(long double xx, long double h[4]) const {
        int l = 3;
        while (l < n - 1 && xx >= t[l + 1]) ++l;
        long double hh[4];
        h[0] = 1.0L;
        for (int j = 1; j <= 3; ++j) {
            for (int i = 0; i < j; ++i) hh[i] = h[i];
            h[0] = 0.0L;
            for (int i = 0; i < j; ++i) {
                const int li = l + i + 1, lj = li - j;
                const long double f = hh[i] / (t[li] - t[lj]);
                h[i] += f * (t[li] - xx);
                h[i + 1] = f * (xx - t[lj]);
            }
        }
        return l;
    }
};

int spline_matrix(int nc, const double* xc, int nf, const double* xf, double* A) {
    if (nc < 4) return fail(TPIV_EINVAL, "the spline predictor needs at least 4 coarse points per axis");
    for (int i = 1; i < nc; ++i)
        if (!(xc[i] > xc[i - 1])) return fail(TPIV_EINVAL, "coarse coordinates must increase strictly");
    Bspl bs(nc, xc);
    const int n = nc;
    // collocation matrix C[i][j] = B_j(x_i): rows have 4 non-zeros at columns l-3..l
    std::vector<long double> C((size_t)n * n, 0.0L);
    for (int i = 0; i < n; ++i) {
        long double h[4];
        const int l = bs.eval((long double)xc[i], h);
        for (int k = 0; k < 4; ++k) C[(size_t)i * n + (l - 3 + k)] = h[k];
    }
    // Inv = C^-1: banded LU (forward elimination with partial pivoting inside the band,
    // lower bandwidth <= 3) applied to the identity, then back-substitution (the upper
    // bandwidth grows to <= 6 through the row swaps).
    std::vector<long double> Inv((size_t)n * n, 0.0L);
    for (int i = 0; i < n; ++i) Inv[(size_t)i * n + i] = 1.0L;
    const int kl = 3, ku = 6;
    for (int col = 0; col < n; ++col) {
        int piv = col;
        long double best = fabsl(C[(size_t)col * n + col]);
        for (int r = col + 1; r < n && r <= col + kl; ++r) {
            const long double v = fabsl(C[(size_t)r * n + col]);
            if (v > best) {
                best = v;
                piv = r;
            }
        }
        if (best == 0.0L) return fail(TPIV_EINVAL, "singular spline collocation matrix");
        if (piv != col) {
            for (int k = 0; k < n; ++k) {
                std::swap(C[(size_t)piv * n + k], C[(size_t)col * n + k]);
                std::swap(Inv[(size_t)piv * n + k], Inv[(size_t)col * n + k]);
            }
        }
        const int k_hi = col + ku + 1 < n ? col + ku + 1 : n;
        for (int r = col + 1; r < n && r <= col + kl; ++r) {
            const long double f = C[(size_t)r * n + col] / C[(size_t)col * n + col];
            if (f == 0.0L) continue;
            for (int k = col; k < k_hi; ++k) C[(size_t)r * n + k] -= f * C[(size_t)col * n + k];
            for (int k = 0; k < n; ++k) Inv[(size_t)r * n + k] -= f * Inv[(size_t)col * n + k];
        }
    }
    for (int i = n - 1; i >= 0; --i) {
        const int k_hi = i + ku + 1 < n ? i + ku + 1 : n;
        const long double d = 1.0L / C[(size_t)i * n + i];
        for (int j = 0; j < n; ++j) {
            long double acc = Inv[(size_t)i * n + j];
            for (int k = i + 1; k < k_hi; ++k) acc -= C[(size_t)i * n + k] * Inv[(size_t)k * n + j];
            Inv[(size_t)i * n + j] = acc * d;
        }
    }
    for (int f = 0; f < nf; ++f) {
        long double xx = xf[f];
        if (xx < xc[0]) xx = xc[0];            // FITPACK fpbisp clamps the arguments
        if (xx > xc[n - 1]) xx = xc[n - 1];
        long double h[4];
        const int l = bs.eval(xx, h);
        for (int j = 0; j < n; ++j) {
            long double acc = 0.0L;
            for (int k = 0; k < 4; ++k) acc += h[k] * Inv[(size_t)(l - 3 + k) * n + j];
            A[(size_t)f * n + j] = (double)acc;
        }
    }
    return TPIV_OK;
}

bool valid_precision(int p) { return p == TPIV_PREC_FAST || p == TPIV_PREC_REFERENCE || p == TPIV_PREC_F64 || p == TPIV_PREC_EXACT; }

struct PassGeo {
    int ws, ov, n_rows, n_cols;
    std::vector<double> x, y;
};

}  // namespace

struct tpiv_plan {
    int H = 0, W = 0, n_pass = 0, mode = 0, max_batch = 0, val_win = 3, device = 0, precision = 0;
    double val_ratio = 1.2;
    std::vector<PassGeo> geo;
    // device workspace
    std::vector<double*> u, v;           // per pass (all but the last): [max_batch, N_p]
    std::vector<uint8_t*> val;
    // per pass p >= 1: the spline operators from pass p-1 to p in banded form (piv_kernels.h: BandedPredictParams)
    std::vector<double*> Wy32, Ax32;
    std::vector<int*> k0y32, k0x32;
    std::vector<int> KY, KX;
    double *u0 = nullptr, *v0 = nullptr, *T = nullptr;      // predictor hand-off: raw fields ...
    uint8_t* pmask = nullptr;                               // ... and the thresholded mask (PassParams::pmask)
    float* peak_raw = nullptr;           // [max_batch, max N_p, 8] hand-off tile kernel -> finalize
    size_t peak_raw_bytes = 0;
    int last_batch = 0;                  // batch of the last tpiv_plan_run (tpiv_plan_exact_fallbacks)
    unsigned* exact_count = nullptr;     // TPIV_PREC_EXACT: the float64-list length of the last run's first pass (copied out
                                         // of peak_raw, which the later passes reuse)
    // normalized median test between / after the passes (tpiv_plan_set_outlier); off: nothing below is allocated
    int outlier_kind = 0, outlier_min = 3;
    double outlier_threshold = 2.0, outlier_eps = 0.1;
    std::vector<uint8_t*> ostatus;       // per pass: [max_batch, N_p] status map of the last run
    double *raw_u = nullptr, *raw_v = nullptr;   // a pass before the last writes here; the test writes the pass's fields
    uint8_t* raw_val = nullptr;          // the last pass's mask as the peak-ratio test left it; the test writes the caller's
    // geometric mask (tpiv_plan_set_mask); off: nothing is enqueued for it.  mgrid: per pass [N_p], 1 = excluded cell
    bool mask_on = false;
    std::vector<uint8_t*> mgrid;
    // per-pair masks (tpiv_plan_set_pair_masks); off: nothing below is allocated.  pgrid: per pass [max_batch, N_p], what the
    // last tpiv_plan_run_masked computed; pair_run: set while that call enqueues, so that the settle steps and the
    // uncertainty kernel read pgrid instead of mgrid
    bool pair_on = false, pair_run = false;
    std::vector<uint8_t*> pgrid;
    // correlation-statistics uncertainty behind the last pass (tpiv_plan_set_uncertainty); off: nothing is enqueued for it
    int unc_kind = 0, unc_radius = 3;
    double *unc_su = nullptr, *unc_sv = nullptr;     // [max_batch, N_last] of the last run
    // image deformation behind the last pass (tpiv_plan_set_deform); off: nothing is enqueued for it
    int def_iters = 0, def_interp = 0, def_smooth = 1;
    int16_t *def_nodes = nullptr, *def_table = nullptr;      // [max_batch, N_last, 2]; the plan's copy of the Q10 table
    uint8_t *def_wa = nullptr, *def_wb = nullptr;            // [max_batch, H, W]
    double *def_du = nullptr, *def_dv = nullptr;             // the residual pass, [max_batch, N_last]
    uint8_t* def_dval = nullptr;
    double *def_su = nullptr, *def_sv = nullptr;             // a round before the last combines here when the median test is on
    hipEvent_t def_ev[2] = {nullptr, nullptr};               // around the rounds of a run
    bool def_ran = false;
    // ensemble correlation (tpiv_plan_set_ensemble); off: nothing below is allocated.  One accumulator sized for the largest
    // pass; the batch-1 fields of every pass and the shared predictor hand-off of their own, so that tpiv_plan_run in between
    // disturbs nothing
    bool ens_on = false;
    float* ens_acc = nullptr;
    std::vector<double*> ens_u, ens_v;   // per pass: [N_p], the ensemble field as its settle step left it
    std::vector<uint8_t*> ens_val;
    double *ens_u0 = nullptr, *ens_v0 = nullptr;
    uint8_t* ens_pmask = nullptr;
    int ens_pass = -1, ens_done = -1;    // the pass between begin and end; the highest pass ended
    long long ens_pairs = 0;             // pairs added since begin
    // spectrally filtered passes (tpiv_plan_set_correlation); off: nothing is allocated and every pass is the plain one
    int corr_kind = 0;
    double corr_floor = 0.0;
    std::vector<float*> corr_tab;        // per pass: g_y[0 .. ws/2], then g_x[0 .. ws/2]
    tpiv::SpecParams spec(int pass) const { return tpiv::SpecParams{corr_tab[pass], (float)corr_floor}; }
    // weighted interrogation windows (tpiv_plan_set_weighting); off: nothing is allocated and every pass is the plain one
    int wt_kind = 0;
    std::vector<float*> wt_tab;          // per pass: g_y[0 .. ws-1], then g_x[0 .. ws-1]
    bool last_filtered = false;          // the last tpiv_plan_run ran filtered or weighted passes: its first pass took no exact scheme
    std::vector<char> sub_recorded;      // per timed run: the three sub-events of the exact first pass were recorded
    std::vector<void*> allocs;
    // optional per-kernel timing: events[run][2*slot + {0,1}]
    bool timing = false;
    std::vector<std::vector<hipEvent_t>> events;
    size_t runs_recorded = 0;

    ~tpiv_plan() {
        for (void* p : allocs) (void)hipFree(p);
        for (auto& r : events)
            for (hipEvent_t e : r) (void)hipEventDestroy(e);
        for (hipEvent_t e : def_ev)
            if (e) (void)hipEventDestroy(e);
    }
    int n_slots() const { return 2 * n_pass - 1; }
    // TPIV_PREC_EXACT: three more events per run inside slot 0 (behind the locating pass, the refinement, the float64 list pass)
    double exact_ms[4] = {0, 0, 0, 0};   // their mean durations at the last tpiv_plan_get_timing (+ finalize)
    hipEvent_t* sub_events() {
        if (!exact_count || !ev(0, 0)) return nullptr;
        return events[runs_recorded].data() + 2 * n_slots();
    }
    // event for (current run, slot, begin/end); nullptr when timing is off or the record is full
    hipEvent_t ev(int slot, int end) {
        if (!timing || runs_recorded >= 512) return nullptr;
        if (events.size() <= runs_recorded) {
            std::vector<hipEvent_t> r(2 * n_slots() + 3, nullptr);
            for (auto& e : r)
                if (hipEventCreate(&e) != hipSuccess) return nullptr;
            events.push_back(std::move(r));
        }
        return events[runs_recorded][2 * slot + end];
    }
    template <typename T_>
    int alloc(T_** out, size_t count) {
        void* p = nullptr;
        hipError_t e = hipMalloc(&p, count * sizeof(T_) + 16);
        if (e != hipSuccess) return fail(TPIV_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
        allocs.push_back(p);
        *out = static_cast<T_*>(p);
        return TPIV_OK;
    }
};

namespace {

// a plan's workspace lives on the device it was created on: whatever allocates or launches for it checks first
int check_plan_device(const tpiv_plan* plan) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != plan->device) return fail(TPIV_EINVAL, "plan was created on another device");
    return TPIV_OK;
}

// The feature pairs a plan refuses: every setter that switches a feature on walks its rows, in this order, against what the
// plan already has (refuse_combination).  The guard of direct users of the C ABI; the Python layer refuses the same pairs
// before it gets here (torchpiv_amd/options.py: EXCLUSIONS).
enum Feature { F_PAIR_MASKS, F_UNCERTAINTY, F_DEFORM, F_CORRELATION, F_WEIGHTING, F_ENSEMBLE };
#define HAS(field) [](const tpiv_plan* p) { return bool(p->field); }
const struct Refusal { Feature subject; bool (*on)(const tpiv_plan*); const char* msg; } REFUSALS[] = {
    {F_PAIR_MASKS, HAS(ens_on), "per-pair masks do not combine with ensemble correlation"},
    {F_UNCERTAINTY, HAS(ens_on), "uncertainty= does not combine with ensemble correlation"},
    {F_UNCERTAINTY, HAS(corr_kind), "uncertainty= does not combine with correlation="},
    {F_UNCERTAINTY, HAS(wt_kind), "uncertainty= does not combine with weighting= (its estimator sums over a top-hat window)"},
    {F_DEFORM, HAS(ens_on), "deform= does not combine with ensemble correlation"},
    {F_DEFORM, HAS(corr_kind), "deform= does not combine with correlation="},
    {F_CORRELATION, HAS(unc_kind), "correlation= does not combine with uncertainty="},
    {F_CORRELATION, HAS(def_iters), "correlation= does not combine with deform="},
    {F_CORRELATION, HAS(ens_on), "correlation= does not combine with ensemble correlation"},
    {F_CORRELATION, HAS(wt_kind), "correlation= does not combine with weighting="},
    {F_WEIGHTING, HAS(unc_kind), "weighting= does not combine with uncertainty= (its estimator sums over a top-hat window)"},
    {F_WEIGHTING, HAS(ens_on), "weighting= does not combine with ensemble correlation"},
    {F_WEIGHTING, HAS(corr_kind), "weighting= does not combine with correlation="},
    {F_ENSEMBLE, HAS(unc_kind), "ensemble correlation does not combine with uncertainty="},
    {F_ENSEMBLE, HAS(def_iters), "ensemble correlation does not combine with deform="},
    {F_ENSEMBLE, HAS(corr_kind), "ensemble correlation does not combine with correlation="},
    {F_ENSEMBLE, HAS(wt_kind), "ensemble correlation does not combine with weighting="},
    {F_ENSEMBLE, HAS(pair_on), "ensemble correlation does not combine with per-pair masks"},
};
#undef HAS

int refuse_combination(const tpiv_plan* plan, Feature subject) {
    for (const Refusal& r : REFUSALS)
        if (r.subject == subject && r.on(plan)) return fail(TPIV_EINVAL, r.msg);
    return TPIV_OK;
}

// band of one operator row: PRED_BW taps around the largest entry (clipped to the matrix); returns
// the largest magnitude left outside so that the caller can verify the truncation is harmless
constexpr int PRED_BW = 65;

int band_start(const double* row, int nc, int bw) {
    int c = 0;
    double best = -1.0;
    for (int j = 0; j < nc; ++j)
        if (std::fabs(row[j]) > best) {
            best = std::fabs(row[j]);
            c = j;
        }
    int st = c - bw / 2;
    if (st < 0) st = 0;
    if (st + bw > nc) st = nc - bw;
    return st;
}

template <typename T>
int upload(tpiv_plan* pl, T** dst, const std::vector<T>& src) {
    int rc = pl->alloc(dst, src.size());
    if (rc) return rc;
    hipError_t e = hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpy(banded operator)");
    return TPIV_OK;
}

// The two spline operators in the form predict_mfma.hip takes: per block of 32 fine rows / columns a dense
// K x 32 weight tile over the union of the block's 65-tap bands (zero elsewhere).
int build_banded(tpiv_plan* pl, int p, int nrc, int ncc, int nrf, int ncf, const std::vector<double>& ay,
                 const std::vector<double>& ax) {
    double leak = 0.0;
    // band starts, monotone in the fine index; `leak` = the largest weight left outside a band
    auto starts = [&leak](const std::vector<double>& op, int nf, int nc, int bw) {
        std::vector<int> st(nf);
        for (int f = 0; f < nf; ++f) {
            const double* row = &op[(size_t)f * nc];
            int s = band_start(row, nc, bw);
            if (f > 0 && s < st[f - 1]) s = st[f - 1];
            st[f] = s;
            for (int j = 0; j < nc; ++j)
                if ((j < s || j >= s + bw) && std::fabs(row[j]) > leak) leak = std::fabs(row[j]);
        }
        return st;
    };
    auto tiles32 = [](const std::vector<double>& op, const std::vector<int>& st, int nf, int nc, int bw,
                      std::vector<double>& tile, std::vector<int>& k0v) {
        const int nb = (nf + 31) / 32;
        int K = 0;
        k0v.resize(nb);
        for (int b = 0; b < nb; ++b) {
            const int f1 = std::min(32 * b + 31, nf - 1);
            k0v[b] = st[32 * b];
            K = std::max(K, st[f1] + bw - st[32 * b]);
        }
        K = (K + 7) / 8 * 8;                                     // the kernels take two K-steps of 4 per trip
        tile.assign((size_t)nb * K * 32, 0.0);
        for (int f = 0; f < nf; ++f)
            for (int j = st[f]; j < st[f] + bw; ++j)
                tile[((size_t)(f / 32) * K + (j - k0v[f / 32])) * 32 + f % 32] = op[(size_t)f * nc + j];
        return K;
    };
    const int bwy = nrc < PRED_BW ? nrc : PRED_BW, bwx = ncc < PRED_BW ? ncc : PRED_BW;
    const std::vector<int> sy = starts(ay, nrf, nrc, bwy), sx = starts(ax, ncf, ncc, bwx);
    if (leak > 1e-17) return fail(TPIV_EUNSUPPORTED, "spline operator does not fit the 65-tap band");
    std::vector<double> wy32, ax32;
    std::vector<int> k0y32, k0x32;
    pl->KY[p] = tiles32(ay, sy, nrf, nrc, bwy, wy32, k0y32);
    pl->KX[p] = tiles32(ax, sx, ncf, ncc, bwx, ax32, k0x32);
    int rc = upload(pl, &pl->Wy32[p], wy32);
    if (!rc) rc = upload(pl, &pl->Ax32[p], ax32);
    if (!rc) rc = upload(pl, &pl->k0y32[p], k0y32);
    if (!rc) rc = upload(pl, &pl->k0x32[p], k0x32);
    return rc;
}

}  // namespace

extern "C" {

int tpiv_version(void) { return TPIV_VERSION; }

const char* tpiv_last_error(void) { return g_err.c_str(); }

int tpiv_field_shape(int H, int W, int ws, int ov, int* n_rows, int* n_cols) {
    if (ov >= ws) return fail(TPIV_EINVAL, "Overlap has to be smaller than the window_size");
    if (ws > H || ws > W) return fail(TPIV_EINVAL, "window size cannot be larger than the image");
    field_shape(H, W, ws, ov, n_rows, n_cols);
    return TPIV_OK;
}

int tpiv_coordinates(int H, int W, int ws, int ov, double* x, double* y) {
    int nr, nc;
    int rc = tpiv_field_shape(H, W, ws, ov, &nr, &nc);
    if (rc) return rc;
    coords_1d(W, nc, ws, ov, x);
    coords_1d(H, nr, ws, ov, y);
    return TPIV_OK;
}

int tpiv_spline_matrix(int nc, const double* xc, int nf, const double* xf, double* A) {
    return spline_matrix(nc, xc, nf, xf, A);
}

// what the first pass and the shifted passes hand their kernels alike; the callers add what is their own
static tpiv::PassParams pass_params(const uint8_t* a, const uint8_t* b, int batch, int H, int W, int ws, int ov,
                                    double val_ratio, int val_win, int precision, double* u, double* v, uint8_t* invalid,
                                    float* dbg_win, float* dbg_corr) {
    tpiv::PassParams p{};
    p.A = a;
    p.B = b;
    p.batch = batch;
    p.H = H;
    p.W = W;
    p.ws = ws;
    p.ov = ov;
    field_shape(H, W, ws, ov, &p.n_rows, &p.n_cols);
    p.u = u;
    p.v = v;
    p.val = invalid;
    p.val_ratio = val_ratio;
    p.val_win = val_win;
    p.dbg_win = dbg_win;
    p.dbg_corr = dbg_corr;
    p.stamps = g_stamps;
    p.precision = precision;
    return p;
}

static int pass1_impl(const uint8_t* a, const uint8_t* b, int batch, int H, int W, int ws, int ov,
                      double val_ratio, int val_win, int precision, double* u, double* v, uint8_t* invalid,
                      void* work, size_t work_bytes, float* dbg_win, float* dbg_corr, void* stream,
                      hipEvent_t* sub_events = nullptr, const tpiv::SpecParams* spec = nullptr,
                      const tpiv::WinParams* win = nullptr) {
    int rc = check_window(H, W, ws, ov, val_win);
    if (rc) return rc;
    if (spec || win) precision = TPIV_PREC_FAST;      // a filtered or weighted first pass is a float32 kernel at every precision
    if (!valid_precision(precision)) return fail(TPIV_EINVAL, "precision must be TPIV_PREC_FAST, TPIV_PREC_REFERENCE, TPIV_PREC_F64 or TPIV_PREC_EXACT");
    if (batch <= 0) return TPIV_OK;
    tpiv::PassParams p = pass_params(a, b, batch, H, W, ws, ov, val_ratio, val_win, precision, u, v, invalid, dbg_win, dbg_corr);
    p.sub_events = sub_events;
    rc = check_work(work, work_bytes, tpiv::peak_raw_bytes(ws, batch, p.n_rows * p.n_cols, precision));
    if (rc) return rc;
    p.peak_raw = static_cast<float*>(work);
    int n_cu;
    rc = n_cu_of_current_device(&n_cu);
    if (rc) return rc;
    if (win) HIP_TRY(tpiv::launch_xcorr_win(p, tpiv::MODE_PASS1, *win, n_cu, (hipStream_t)stream));
    else if (spec) HIP_TRY(tpiv::launch_xcorr_spec(p, tpiv::MODE_PASS1, *spec, n_cu, (hipStream_t)stream));
    else HIP_TRY(tpiv::launch_xcorr(p, tpiv::MODE_PASS1, n_cu, (hipStream_t)stream));
    return TPIV_OK;
}

int tpiv_pass1(const uint8_t* a, const uint8_t* b, int batch, int H, int W, int ws, int ov,
               double val_ratio, int val_win, int precision, double* u, double* v, uint8_t* invalid,
               void* work, size_t work_bytes, void* stream) {
    return pass1_impl(a, b, batch, H, W, ws, ov, val_ratio, val_win, precision, u, v, invalid, work, work_bytes,
                      nullptr, nullptr, stream);
}

size_t tpiv_work_bytes(int H, int W, int ws, int ov, int batch) {
    if (ov >= ws || ws > H || ws > W || ws <= 0 || ov < 0 || batch <= 0 || !supported_ws(ws)) return 0;
    int nr, nc;
    field_shape(H, W, ws, ov, &nr, &nc);
    const size_t a = tpiv::peak_raw_bytes(ws, batch, nr * nc, TPIV_PREC_EXACT);          // the largest of the precisions
    const size_t a1 = tpiv::peak_raw_bytes(ws, batch, nr * nc, TPIV_PREC_REFERENCE);
    const size_t b = tpiv::peak_raw_bytes(ws, batch, nr * nc, TPIV_PREC_FAST, true);     // TPIV_MODE_CWS_FAST: generic kernel
    return std::max(a, std::max(a1, b));
}

int tpiv_predict(int mode, int batch, int nrc, int ncc, int nrf, int ncf, const double* Ay,
                 const double* Ax, const double* u_c, const double* v_c, const uint8_t* invalid_c,
                 double* work, double* u0, double* v0, double* u2, double* v2, void* stream) {
    if (mode != TPIV_MODE_DWS && mode != TPIV_MODE_CWS) return fail(TPIV_EKEY, "unknown multipass mode");
    if (batch <= 0) return TPIV_OK;
    tpiv::PredictParams q{};
    q.batch = batch;
    q.mode = mode;
    q.nrc = nrc;
    q.ncc = ncc;
    q.nrf = nrf;
    q.ncf = ncf;
    q.Ay = Ay;
    q.Ax = Ax;
    q.u_c = u_c;
    q.v_c = v_c;
    q.val_c = invalid_c;
    q.T = work;
    q.u0 = u0;
    q.v0 = v0;
    q.u2 = u2;
    q.v2 = v2;
    HIP_TRY(tpiv::launch_predict(q, (hipStream_t)stream));
    return TPIV_OK;
}

static int run_iter(int mode, int precision, const uint8_t* a, const uint8_t* b, int batch, int H, int W, int ws,
                    int ov, const double* u0, const double* v0, const double* u2, const double* v2,
                    double val_ratio, int val_win, double* u, double* v, uint8_t* invalid, double* du,
                    double* dv, float* dbg_win, float* dbg_corr, void* work, size_t work_bytes, void* stream,
                    const uint8_t* pmask = nullptr, const tpiv::SpecParams* spec = nullptr,
                    const tpiv::WinParams* win = nullptr) {
    if (mode != TPIV_MODE_DWS && mode != TPIV_MODE_CWS && mode != TPIV_MODE_CWS_FAST)
        return fail(TPIV_EKEY, "unknown multipass mode");
    int rc = check_window(H, W, ws, ov, val_win);
    if (rc) return rc;
    if (mode == TPIV_MODE_CWS_FAST && ws < 2) return fail(TPIV_EINVAL, "window too small");
    if (mode != TPIV_MODE_CWS_FAST && !pmask && (!u2 || !v2)) return fail(TPIV_EINVAL, "tpiv_iter: u2 / v2 missing");
    if (!u0 || !v0) return fail(TPIV_EINVAL, "tpiv_iter: u0 / v0 missing");
    if (!valid_precision(precision)) return fail(TPIV_EINVAL, "precision must be TPIV_PREC_FAST, TPIV_PREC_REFERENCE, TPIV_PREC_F64 or TPIV_PREC_EXACT");
    if (batch <= 0) return TPIV_OK;
    tpiv::PassParams p = pass_params(a, b, batch, H, W, ws, ov, val_ratio, val_win, precision, u, v, invalid, dbg_win, dbg_corr);
    p.u0 = u0;
    p.v0 = v0;
    p.u2 = u2;
    p.v2 = v2;
    p.pmask = pmask;           // plan path: raw predictor in u0 / v0 + mask (piv_kernels.h)
    p.du = du;
    p.dv = dv;
    rc = check_work(work, work_bytes,
                    tpiv::peak_raw_bytes(ws, batch, p.n_rows * p.n_cols, TPIV_PREC_FAST, mode == TPIV_MODE_CWS_FAST));
    if (rc) return rc;
    p.peak_raw = static_cast<float*>(work);
    int n_cu;
    rc = n_cu_of_current_device(&n_cu);
    if (rc) return rc;
    if (win) HIP_TRY(tpiv::launch_xcorr_win(p, mode, *win, n_cu, (hipStream_t)stream));
    else if (spec) HIP_TRY(tpiv::launch_xcorr_spec(p, mode, *spec, n_cu, (hipStream_t)stream));
    else HIP_TRY(tpiv::launch_xcorr(p, mode, n_cu, (hipStream_t)stream));
    return TPIV_OK;
}

int tpiv_iter(int mode, const uint8_t* a, const uint8_t* b, int batch, int H, int W, int ws, int ov,
              const double* u0, const double* v0, const double* u2, const double* v2,
              double val_ratio, int val_win, int precision, double* u, double* v, uint8_t* invalid, double* du,
              double* dv, void* work, size_t work_bytes, void* stream) {
    return run_iter(mode, precision, a, b, batch, H, W, ws, ov, u0, v0, u2, v2, val_ratio, val_win, u, v, invalid,
                    du, dv, nullptr, nullptr, work, work_bytes, stream);
}

int tpiv_debug_pass(int mode, int precision, const uint8_t* a, const uint8_t* b, int batch, int H, int W, int ws,
                    int ov, const double* u2, const double* v2, const double* zero, double* u, double* v,
                    uint8_t* invalid, float* win, float* corr, void* work, size_t work_bytes, void* stream) {
    if (mode == 0)      // the float32 kernel; TPIV_PREC_EXACT: the exact pass, whose maps come from its locating kernel alone
        return pass1_impl(a, b, batch, H, W, ws, ov, 1.2, 3, precision == TPIV_PREC_EXACT ? TPIV_PREC_EXACT : TPIV_PREC_FAST,
                          u, v, invalid, work, work_bytes, win, corr, stream);
    if (!zero || !u2 || !v2) return fail(TPIV_EINVAL, "tpiv_debug_pass: shifted passes need u2, v2 and a zero field");
    // CWS_Fast takes its shift from u0, v0 (B:644-653): the given predictor goes there
    const bool cwsf = mode == TPIV_MODE_CWS_FAST;
    return run_iter(mode, precision, a, b, batch, H, W, ws, ov, cwsf ? u2 : zero, cwsf ? v2 : zero, u2, v2, 1.2, 3, u, v,
                    invalid, nullptr, nullptr, win, corr, work, work_bytes, stream);
}

static int check_correlation(const char* who, int kind, double dx, double dy, double floor) {
    if (kind != TPIV_CORR_PHASE && kind != TPIV_CORR_RPC)
        return fail(TPIV_EINVAL, std::string(who) + ": kind must be TPIV_CORR_NONE, TPIV_CORR_PHASE or TPIV_CORR_RPC");
    if (!(dx >= 0.0 && dx <= 16.0) || !(dy >= 0.0 && dy <= 16.0))
        return fail(TPIV_EINVAL, std::string(who) + ": the particle-image diameters must be in 0..16 pixels");
    if (kind == TPIV_CORR_PHASE && (dx != 0.0 || dy != 0.0))
        return fail(TPIV_EINVAL, std::string(who) + ": phase-only correlation has diameter 0");
    if (!(floor >= 0x1p-20 && floor <= 0x1p-4)) return fail(TPIV_EINVAL, std::string(who) + ": floor must be in 2^-20..2^-4");
    return TPIV_OK;
}

int tpiv_debug_pass_spec(int mode, int kind, double floor, const float* tab, const uint8_t* a, const uint8_t* b, int batch,
                         int H, int W, int ws, int ov, const double* u2, const double* v2, const double* zero, double* u,
                         double* v, uint8_t* invalid, float* win, float* corr, void* work, size_t work_bytes, void* stream) {
    if (int rc = check_correlation("tpiv_debug_pass_spec", kind, 0.0, 0.0, floor)) return rc;
    if (mode == TPIV_MODE_CWS_FAST) return fail(TPIV_EUNSUPPORTED, "correlation=: the CWS_Fast iteration has no filtered kernel");
    if (mode != 0 && mode != TPIV_MODE_DWS && mode != TPIV_MODE_CWS) return fail(TPIV_EKEY, "unknown multipass mode");
    if (!tpiv::spec_size(ws))
        return fail(TPIV_EUNSUPPORTED, "correlation=: filtered passes cover window sizes 16, 32 and 64 (got " + std::to_string(ws) + ")");
    if (!tab) return fail(TPIV_EINVAL, "tpiv_debug_pass_spec: tables missing");
    const tpiv::SpecParams sp{tab, (float)floor};
    if (mode == 0)
        return pass1_impl(a, b, batch, H, W, ws, ov, 1.2, 3, TPIV_PREC_FAST, u, v, invalid, work, work_bytes, win, corr, stream,
                          nullptr, &sp);
    if (!zero || !u2 || !v2) return fail(TPIV_EINVAL, "tpiv_debug_pass_spec: shifted passes need u2, v2 and a zero field");
    return run_iter(mode, TPIV_PREC_FAST, a, b, batch, H, W, ws, ov, zero, zero, u2, v2, 1.2, 3, u, v, invalid, nullptr, nullptr,
                    win, corr, work, work_bytes, stream, nullptr, &sp);
}

int tpiv_debug_pass_weighted(int mode, const float* tab, const uint8_t* a, const uint8_t* b, int batch, int H, int W, int ws,
                             int ov, const double* u2, const double* v2, const double* zero, double* u, double* v,
                             uint8_t* invalid, float* win, float* corr, void* work, size_t work_bytes, void* stream) {
    if (mode == TPIV_MODE_CWS_FAST) return fail(TPIV_EUNSUPPORTED, "weighting=: the CWS_Fast iteration has no weighted kernel");
    if (mode != 0 && mode != TPIV_MODE_DWS && mode != TPIV_MODE_CWS) return fail(TPIV_EKEY, "unknown multipass mode");
    if (!tpiv::win_size(ws))
        return fail(TPIV_EUNSUPPORTED, "weighting=: weighted passes cover window sizes 16, 32 and 64 (got " + std::to_string(ws) + ")");
    if (!tab) return fail(TPIV_EINVAL, "tpiv_debug_pass_weighted: tables missing");
    const tpiv::WinParams wp{tab};
    if (mode == 0)
        return pass1_impl(a, b, batch, H, W, ws, ov, 1.2, 3, TPIV_PREC_FAST, u, v, invalid, work, work_bytes, win, corr, stream,
                          nullptr, nullptr, &wp);
    if (!zero || !u2 || !v2) return fail(TPIV_EINVAL, "tpiv_debug_pass_weighted: shifted passes need u2, v2 and a zero field");
    return run_iter(mode, TPIV_PREC_FAST, a, b, batch, H, W, ws, ov, zero, zero, u2, v2, 1.2, 3, u, v, invalid, nullptr, nullptr,
                    win, corr, work, work_bytes, stream, nullptr, nullptr, &wp);
}

int tpiv_debug_iter_compact(int mode, const uint8_t* a, const uint8_t* b, int batch, int H, int W, int ws, int ov,
                            const double* u_raw, const double* v_raw, const uint8_t* mask, double val_ratio, int val_win,
                            int precision, double* u, double* v, uint8_t* invalid, double* du, double* dv, void* work,
                            size_t work_bytes, void* stream) {
    if (mode != TPIV_MODE_DWS && mode != TPIV_MODE_CWS)
        return fail(TPIV_EINVAL, "tpiv_debug_iter_compact: the compact hand-off exists for DWS and CWS only");
    if (!mask) return fail(TPIV_EINVAL, "tpiv_debug_iter_compact: mask missing");
    // the call of tpiv_plan_run: raw predictor + mask byte, no half-shift fields
    return run_iter(mode, precision, a, b, batch, H, W, ws, ov, u_raw, v_raw, nullptr, nullptr, val_ratio, val_win, u, v,
                    invalid, du, dv, nullptr, nullptr, work, work_bytes, stream, mask);
}

int tpiv_debug_peaks(const float* maps, int n_maps, int ws, int planar, double val_ratio, int val_win, double* u,
                     double* v, uint8_t* invalid, void* work, size_t work_bytes, void* stream) {
    if (ws != 8 && ws != 16 && ws != 32 && ws != 64 && ws != 128)
        return fail(TPIV_EUNSUPPORTED, "tpiv_debug_peaks handles 8, 16, 32, 64 and 128 pixel maps");
    if (n_maps <= 0) return TPIV_OK;
    tpiv::PassParams p{};
    p.batch = 1;
    p.ws = ws;
    p.n_rows = n_maps;
    p.n_cols = 1;
    p.u = u;
    p.v = v;
    p.val = invalid;
    p.val_ratio = val_ratio;
    p.val_win = val_win;
    int rc = check_work(work, work_bytes, (size_t)n_maps * 8 * sizeof(float));
    if (rc) return rc;
    p.peak_raw = static_cast<float*>(work);
    HIP_TRY(tpiv::launch_peaks_from_maps(p, maps, n_maps, planar, (hipStream_t)stream));
    return TPIV_OK;
}

int tpiv_plan_create(tpiv_plan** out, int H, int W, int ws, int ov, int n_pass, int mode,
                     double pass_scale, double val_ratio, int val_win, int max_batch, int precision) {
    if (!out) return fail(TPIV_EINVAL, "null plan pointer");
    *out = nullptr;
    if (n_pass < 1) n_pass = 1;     // range(multipass - 1) is empty for multipass <= 1 (B:855)
    if (n_pass > 1 && mode != TPIV_MODE_DWS && mode != TPIV_MODE_CWS)
        return fail(TPIV_EKEY, "unknown multipass mode");
    if (max_batch < 1) return fail(TPIV_EINVAL, "max_batch must be >= 1");
    if (!(pass_scale > 0)) return fail(TPIV_EINVAL, "multipass_scale must be positive");
    if (!valid_precision(precision)) return fail(TPIV_EINVAL, "precision must be TPIV_PREC_FAST, TPIV_PREC_REFERENCE, TPIV_PREC_F64 or TPIV_PREC_EXACT");
    tpiv_plan* pl = new tpiv_plan();
    pl->precision = precision;
    pl->H = H;
    pl->W = W;
    pl->n_pass = n_pass;
    pl->mode = mode;
    pl->max_batch = max_batch;
    pl->val_ratio = val_ratio;
    pl->val_win = val_win;
    int rc = TPIV_OK;
    hipError_t he = hipGetDevice(&pl->device);
    if (he != hipSuccess) {
        delete pl;
        return hip_fail(he, "hipGetDevice");
    }
    int w = ws, o = ov;
    for (int p = 0; p < n_pass && rc == TPIV_OK; ++p) {
        if (p > 0) {
            w = (int)std::floor((double)w / pass_scale);   // int(ws // scale), B:856-857
            o = (int)std::floor((double)o / pass_scale);
        }
        rc = check_window(H, W, w, o, val_win);
        if (rc) break;
        PassGeo g;
        g.ws = w;
        g.ov = o;
        field_shape(H, W, w, o, &g.n_rows, &g.n_cols);
        g.x.resize(g.n_cols);
        g.y.resize(g.n_rows);
        coords_1d(W, g.n_cols, w, o, g.x.data());
        coords_1d(H, g.n_rows, w, o, g.y.data());
        pl->geo.push_back(std::move(g));
    }
    size_t max_fine = 0, max_T = 0;
    pl->Wy32.assign(n_pass, nullptr);
    pl->Ax32.assign(n_pass, nullptr);
    pl->k0y32.assign(n_pass, nullptr);
    pl->k0x32.assign(n_pass, nullptr);
    pl->KY.assign(n_pass, 0);
    pl->KX.assign(n_pass, 0);
    pl->u.assign(n_pass, nullptr);
    pl->v.assign(n_pass, nullptr);
    pl->val.assign(n_pass, nullptr);
    for (int p = 0; p < n_pass && rc == TPIV_OK; ++p) {
        const PassGeo& g = pl->geo[p];
        const size_t N = (size_t)g.n_rows * g.n_cols;
        if (p < n_pass - 1) {
            rc = pl->alloc(&pl->u[p], N * max_batch);
            if (!rc) rc = pl->alloc(&pl->v[p], N * max_batch);
            if (!rc) rc = pl->alloc(&pl->val[p], N * max_batch);
        }
        if (p > 0 && rc == TPIV_OK) {
            const PassGeo& c = pl->geo[p - 1];
            std::vector<double> ay((size_t)g.n_rows * c.n_rows), ax((size_t)g.n_cols * c.n_cols);
            rc = spline_matrix(c.n_rows, c.y.data(), g.n_rows, g.y.data(), ay.data());
            if (!rc) rc = spline_matrix(c.n_cols, c.x.data(), g.n_cols, g.x.data(), ax.data());
            if (!rc) rc = build_banded(pl, p, c.n_rows, c.n_cols, g.n_rows, g.n_cols, ay, ax);
            if (N > max_fine) max_fine = N;
            // T1 of the banded predictor: three planes of [coarse columns][fine rows rounded up to 32] per pair.  The row
            // kernel of predict_mfma.hip stores at cc < ncc, rf < nrfp only, and the column kernel reads each plane through
            // a buffer descriptor of exactly that size, so no access leaves 3 * roundup32(nrf) * ncc doubles per pair.
            const size_t t = (size_t)3 * ((g.n_rows + 31) / 32 * 32) * c.n_cols;
            if (t > max_T) max_T = t;
        }
    }
    if (rc == TPIV_OK) {
        size_t raw = 0;
        for (size_t i = 0; i < pl->geo.size(); ++i) {
            const PassGeo& g = pl->geo[i];
            const size_t b = tpiv::peak_raw_bytes(g.ws, max_batch, g.n_rows * g.n_cols,
                                                  i == 0 ? precision : (int)TPIV_PREC_FAST);
            if (b > raw) raw = b;
        }
        pl->peak_raw_bytes = raw;
        if (raw) rc = pl->alloc(&pl->peak_raw, raw / sizeof(float) + 64);
        if (rc == TPIV_OK && precision == TPIV_PREC_EXACT && tpiv::exact_refine_size(pl->geo[0].ws))
            rc = pl->alloc(&pl->exact_count, 4);
    }
    if (rc == TPIV_OK && n_pass > 1) {
        rc = pl->alloc(&pl->u0, max_fine * max_batch);
        if (!rc) rc = pl->alloc(&pl->v0, max_fine * max_batch);
        if (!rc) rc = pl->alloc(&pl->pmask, max_fine * max_batch);
        if (!rc) rc = pl->alloc(&pl->T, max_T * max_batch);
    }
    if (rc) {
        const std::string keep = g_err;
        delete pl;
        g_err = keep;
        return rc;
    }
    *out = pl;
    return TPIV_OK;
}

void tpiv_plan_destroy(tpiv_plan* plan) { delete plan; }

int tpiv_plan_n_pass(const tpiv_plan* plan) { return plan ? plan->n_pass : 0; }

int tpiv_plan_pass_geometry(const tpiv_plan* plan, int pass, int* ws, int* ov, int* n_rows, int* n_cols) {
    if (!plan || pass < 0 || pass >= plan->n_pass) return fail(TPIV_EINVAL, "bad plan / pass index");
    const PassGeo& g = plan->geo[pass];
    if (ws) *ws = g.ws;
    if (ov) *ov = g.ov;
    if (n_rows) *n_rows = g.n_rows;
    if (n_cols) *n_cols = g.n_cols;
    return TPIV_OK;
}

const char* tpiv_plan_kernel_name(const tpiv_plan* plan, int pass, char* buf, int len) {
    if (!buf || len <= 0) return buf;
    buf[0] = 0;
    if (!plan || pass < 0 || pass >= plan->n_pass) return buf;
    const int mode = pass == 0 ? (int)tpiv::MODE_PASS1 : plan->mode;
    if (plan->wt_kind) return tpiv::xcorr_win_kernel_name(plan->geo[pass].ws, mode, buf, len);
    if (plan->corr_kind) return tpiv::xcorr_spec_kernel_name(plan->geo[pass].ws, mode, buf, len);
    return tpiv::xcorr_kernel_name(plan->geo[pass].ws, mode, plan->precision, buf, len);
}

int tpiv_plan_exact_fallbacks(tpiv_plan* plan, long long* n_windows) {
    if (!plan || !n_windows) return fail(TPIV_EINVAL, "null argument");
    if (!plan->exact_count)
        return fail(TPIV_EINVAL, "not a TPIV_PREC_EXACT plan with an even first-pass window size from 8 to 128");
    if (plan->last_batch <= 0) return fail(TPIV_EINVAL, "the plan has not run yet");
    if (plan->last_filtered)
        return fail(TPIV_EINVAL, "the last run's first pass was a filtered or weighted one (tpiv_plan_set_correlation, tpiv_plan_set_weighting): it takes no exact scheme");
    HIP_TRY(hipDeviceSynchronize());
    unsigned n = 0;
    HIP_TRY(hipMemcpy(&n, plan->exact_count, sizeof(n), hipMemcpyDeviceToHost));
    *n_windows = (long long)n;
    return TPIV_OK;
}

int tpiv_plan_pass_fields(const tpiv_plan* plan, int pass, double** u, double** v, uint8_t** invalid) {
    if (!plan || pass < 0 || pass >= plan->n_pass - 1)
        return fail(TPIV_EINVAL, "only the passes before the last keep their fields in the plan");
    if (u) *u = plan->u[pass];
    if (v) *v = plan->v[pass];
    if (invalid) *invalid = plan->val[pass];
    return TPIV_OK;
}

static int run_banded_predict(tpiv_plan* plan, int p, int batch, const double* u_c, const double* v_c,
                              const uint8_t* val_c, double* u0, double* v0, double* u2, double* v2,
                              hipStream_t st, uint8_t* mask_out = nullptr) {
    const PassGeo& g = plan->geo[p];
    const PassGeo& c = plan->geo[p - 1];
    tpiv::BandedPredictParams q{};
    q.batch = batch;
    q.mode = plan->mode;
    q.nrc = c.n_rows;
    q.ncc = c.n_cols;
    q.nrf = g.n_rows;
    q.ncf = g.n_cols;
    q.KY = plan->KY[p];
    q.KX = plan->KX[p];
    q.nrfp = (g.n_rows + 31) / 32 * 32;
    q.Wy32 = plan->Wy32[p];
    q.k0y32 = plan->k0y32[p];
    q.Ax32 = plan->Ax32[p];
    q.k0x32 = plan->k0x32[p];
    q.u_c = u_c;
    q.v_c = v_c;
    q.val_c = val_c;
    q.T1 = plan->T;
    q.u0 = u0;
    q.v0 = v0;
    q.u2 = u2;
    q.v2 = v2;
    q.mask_out = mask_out;
    hipError_t he = tpiv::launch_predict_mfma(q, st);
    return he == hipSuccess ? TPIV_OK : hip_fail(he, "launch_predict_mfma");
}

int tpiv_plan_debug_predict(tpiv_plan* plan, int pass, int batch, const double* u_c, const double* v_c,
                            const uint8_t* invalid_c, double* u0, double* v0, double* u2, double* v2,
                            void* stream) {
    if (!plan || pass < 1 || pass >= plan->n_pass) return fail(TPIV_EINVAL, "bad plan / pass index");
    if (batch < 1 || batch > plan->max_batch) return fail(TPIV_EINVAL, "batch exceeds the plan's max_batch");
    return run_banded_predict(plan, pass, batch, u_c, v_c, invalid_c, u0, v0, u2, v2, (hipStream_t)stream);
}

static int run_median_test(const double* u, const double* v, const uint8_t* invalid, int batch, int n_rows, int n_cols,
                           double threshold, double eps, int min_neighbours, uint8_t* status, double* out_u, double* out_v,
                           int replace, uint8_t* invalid_out, hipStream_t st) {
    tpiv::OutlierParams q{};
    q.u = u;
    q.v = v;
    q.invalid = invalid;
    q.batch = batch;
    q.n_rows = n_rows;
    q.n_cols = n_cols;
    q.threshold = threshold;
    q.eps = eps;
    q.min_neighbours = min_neighbours;
    q.status = status;
    q.out_u = out_u;
    q.out_v = out_v;
    q.replace = replace;
    q.invalid_out = invalid_out;
    hipError_t he = tpiv::launch_median_test(q, st);
    return he == hipSuccess ? TPIV_OK : hip_fail(he, "launch_median_test");
}

int tpiv_median_test(const double* u, const double* v, const uint8_t* invalid, int batch, int n_rows, int n_cols,
                     double threshold, double eps, int min_neighbours, uint8_t* status, double* med_u, double* med_v,
                     void* stream) {
    if (batch < 0 || n_rows < 1 || n_cols < 1) return fail(TPIV_EINVAL, "tpiv_median_test: empty grid");
    if (!(threshold > 0) || !(eps >= 0)) return fail(TPIV_EINVAL, "tpiv_median_test: threshold must be > 0 and eps >= 0");
    if (min_neighbours < 1 || min_neighbours > 8) return fail(TPIV_EINVAL, "tpiv_median_test: min_neighbours must be in 1..8");
    if (!u || !v || !invalid || !status) return fail(TPIV_EINVAL, "tpiv_median_test: null pointer");
    if ((long long)n_rows * n_cols >= (1LL << 31)) return fail(TPIV_EUNSUPPORTED, "field too large");
    if (batch == 0) return TPIV_OK;
    // no output may overlap an input or another output: every decision is taken on the fields as they came in
    const size_t cells = (size_t)batch * n_rows * n_cols;
    const Span in[3] = {{u, cells * 8}, {v, cells * 8}, {invalid, cells}};
    const Span out[3] = {{status, cells}, {med_u, cells * 8}, {med_v, cells * 8}};
    if (const int k = aliased(in, 3, out, 3))
        return fail(TPIV_EINVAL, k == 1 ? "tpiv_median_test: an output aliases an input" : "tpiv_median_test: two outputs overlap");
    return run_median_test(u, v, invalid, batch, n_rows, n_cols, threshold, eps, min_neighbours, status, med_u, med_v, 0,
                           nullptr, (hipStream_t)stream);
}

int tpiv_field_fit(const double* u, const double* v, const uint8_t* skip, int batch, int n_rows, int n_cols, int radius,
                   int order, double* fit, uint8_t* count, int8_t* order_out, void* stream) {
    if (batch < 0 || n_rows < 1 || n_cols < 1) return fail(TPIV_EINVAL, "tpiv_field_fit: empty grid");
    if (radius < 1 || radius > 3) return fail(TPIV_EINVAL, "tpiv_field_fit: radius must be 1, 2 or 3");
    if (order < 1 || order > 2) return fail(TPIV_EINVAL, "tpiv_field_fit: order must be 1 or 2");
    if (!u || !v || !fit || !count || !order_out) return fail(TPIV_EINVAL, "tpiv_field_fit: null pointer");
    if ((long long)batch * n_rows * n_cols >= (1LL << 31)) return fail(TPIV_EINVAL, "tpiv_field_fit: field stack too large");
    if (batch == 0) return TPIV_OK;
    const size_t cells = (size_t)batch * n_rows * n_cols;
    const Span in[3] = {{u, cells * 8}, {v, cells * 8}, {skip, cells}};
    const Span out[3] = {{fit, 6 * cells * 8}, {count, cells}, {order_out, cells}};
    if (const int k = aliased(in, 3, out, 3))
        return fail(TPIV_EINVAL, k == 1 ? "tpiv_field_fit: an output aliases an input" : "tpiv_field_fit: two outputs overlap");
    if (batch > 65535 || (n_rows + tpiv::FIELDFIT_TILE_ROWS - 1) / tpiv::FIELDFIT_TILE_ROWS > 65535)
        return fail(TPIV_EUNSUPPORTED, "tpiv_field_fit: more than 65535 pairs or tile rows in one call");
    tpiv::FieldFitParams q{};
    q.u = u;
    q.v = v;
    q.skip = skip;
    q.batch = batch;
    q.n_rows = n_rows;
    q.n_cols = n_cols;
    q.radius = radius;
    q.order_max = order;
    q.fit = fit;
    q.count = count;
    q.order = order_out;
    hipError_t he = tpiv::launch_field_fit(q, (hipStream_t)stream);
    return he == hipSuccess ? TPIV_OK : hip_fail(he, "launch_field_fit");
}

int tpiv_stereo_reconstruct(const double* u1, const double* v1, const double* u2, const double* v2, const double* su1,
                            const double* sv1, const double* su2, const double* sv2, const uint8_t* skip, const double* a1,
                            const double* b1, const double* a2, const double* b2, int batch, long long cells, double fill,
                            double* U, double* V, double* W, double* res, double* sU, double* sV, double* sW, uint8_t* status,
                            double* pair_rms, int32_t* pair_count, void* stream) {
    if (batch < 0 || cells < 1) return fail(TPIV_EINVAL, "tpiv_stereo_reconstruct: empty grid");
    if (!u1 || !v1 || !u2 || !v2 || !a1 || !b1 || !a2 || !b2 || !U || !V || !W || !res || !status || !pair_rms || !pair_count)
        return fail(TPIV_EINVAL, "tpiv_stereo_reconstruct: null pointer");
    const int n_sigma = (su1 != nullptr) + (sv1 != nullptr) + (su2 != nullptr) + (sv2 != nullptr);
    if (n_sigma != 0 && n_sigma != 4)
        return fail(TPIV_EINVAL, "tpiv_stereo_reconstruct: the sigmas su1, sv1, su2, sv2 come all four or not at all");
    if (n_sigma == 4 && (!sU || !sV || !sW)) return fail(TPIV_EINVAL, "tpiv_stereo_reconstruct: null pointer");
    if (cells >= (1LL << 31) || (long long)batch * cells >= (1LL << 31))
        return fail(TPIV_EINVAL, "tpiv_stereo_reconstruct: field stack too large");
    if (batch == 0) return TPIV_OK;
    const size_t n = (size_t)batch * cells, one = (size_t)cells;
    const bool sig = n_sigma == 4;
    const Span in[13] = {{u1, n * 8},  {v1, n * 8},  {u2, n * 8},  {v2, n * 8},  {su1, n * 8},  {sv1, n * 8}, {su2, n * 8},
                         {sv2, n * 8}, {skip, one},  {a1, one * 8}, {b1, one * 8}, {a2, one * 8}, {b2, one * 8}};
    const Span out[10] = {{U, n * 8},
                          {V, n * 8},
                          {W, n * 8},
                          {res, n * 8},
                          {sig ? sU : nullptr, n * 8},
                          {sig ? sV : nullptr, n * 8},
                          {sig ? sW : nullptr, n * 8},
                          {status, n},
                          {pair_rms, (size_t)batch * 8},
                          {pair_count, (size_t)batch * 4}};
    if (const int k = aliased(in, 13, out, 10))
        return fail(TPIV_EINVAL, k == 1 ? "tpiv_stereo_reconstruct: an output aliases an input"
                                        : "tpiv_stereo_reconstruct: two outputs overlap");
    if ((batch + tpiv::STEREO_BLOCK_PAIRS - 1) / tpiv::STEREO_BLOCK_PAIRS > 65535)
        return fail(TPIV_EUNSUPPORTED, "tpiv_stereo_reconstruct: too many pairs in one call");
    tpiv::StereoParams q{};
    q.u1 = u1;
    q.v1 = v1;
    q.u2 = u2;
    q.v2 = v2;
    q.su1 = su1;
    q.sv1 = sv1;
    q.su2 = su2;
    q.sv2 = sv2;
    q.skip = skip;
    q.a1 = a1;
    q.b1 = b1;
    q.a2 = a2;
    q.b2 = b2;
    q.batch = batch;
    q.cells = cells;
    q.fill = fill;
    q.U = U;
    q.V = V;
    q.W = W;
    q.res = res;
    q.sU = sig ? sU : nullptr;
    q.sV = sig ? sV : nullptr;
    q.sW = sig ? sW : nullptr;
    q.status = status;
    q.pair_rms = pair_rms;
    q.pair_count = pair_count;
    hipError_t he = tpiv::launch_stereo_reconstruct(q, (hipStream_t)stream);
    return he == hipSuccess ? TPIV_OK : hip_fail(he, "launch_stereo_reconstruct");
}

int tpiv_stereo_triangulate(const double* dx, const double* dy, const double* X, const double* Y, const uint8_t* skip,
                            int batch, long long cells, const double* cameras_host, double gap_max, const double* plane_host,
                            double tol, const double* centre_host, double* Mx, double* My, double* Mz, double* gap,
                            uint8_t* status, int32_t* count, double* sums, void* stream) {
    if (batch < 0 || cells < 1) return fail(TPIV_EINVAL, "tpiv_stereo_triangulate: empty grid");
    if (!dx || !dy || !X || !Y || !cameras_host || !plane_host || !centre_host || !status || !count || !sums)
        return fail(TPIV_EINVAL, "tpiv_stereo_triangulate: null pointer");
    const int n_points = (Mx != nullptr) + (My != nullptr) + (Mz != nullptr) + (gap != nullptr);
    if (n_points != 0 && n_points != 4)
        return fail(TPIV_EINVAL, "tpiv_stereo_triangulate: the points Mx, My, Mz, gap come all four or not at all");
    if (!(gap_max >= 0)) return fail(TPIV_EINVAL, "tpiv_stereo_triangulate: gap_max must be >= 0 (infinity: no test)");
    if (!(tol >= 0)) return fail(TPIV_EINVAL, "tpiv_stereo_triangulate: tol must be >= 0 (infinity: no test)");
    if (cells >= (1LL << 31) || (long long)batch * cells >= (1LL << 31))
        return fail(TPIV_EINVAL, "tpiv_stereo_triangulate: field stack too large");
    if (batch == 0) return TPIV_OK;
    const size_t n = (size_t)batch * cells, one = (size_t)cells;
    const Span in[5] = {{dx, n * 8}, {dy, n * 8}, {X, one * 8}, {Y, one * 8}, {skip, one}};
    const Span out[7] = {{Mx, n * 8}, {My, n * 8}, {Mz, n * 8}, {gap, n * 8}, {status, n}, {count, (size_t)batch * 4},
                         {sums, (size_t)batch * 9 * 8}};
    if (const int k = aliased(in, 5, out, 7))
        return fail(TPIV_EINVAL, k == 1 ? "tpiv_stereo_triangulate: an output aliases an input"
                                        : "tpiv_stereo_triangulate: two outputs overlap");
    if ((batch + tpiv::STEREO_BLOCK_PAIRS - 1) / tpiv::STEREO_BLOCK_PAIRS > 65535)
        return fail(TPIV_EUNSUPPORTED, "tpiv_stereo_triangulate: too many items in one call");
    tpiv::TriangulateParams q{};
    q.dx = dx;
    q.dy = dy;
    q.X = X;
    q.Y = Y;
    q.skip = skip;
    q.batch = batch;
    q.cells = cells;
    for (int k = 0; k < 3; ++k) {
        q.C1[k] = cameras_host[k];
        q.C2[k] = cameras_host[3 + k];
        q.plane[k] = plane_host[k];
        q.centre[k] = centre_host[k];
    }
    q.gap_max = gap_max;
    q.tol = tol;
    q.Mx = Mx;
    q.My = My;
    q.Mz = Mz;
    q.gap = gap;
    q.status = status;
    q.count = count;
    q.sums = sums;
    hipError_t he = tpiv::launch_stereo_triangulate(q, (hipStream_t)stream);
    return he == hipSuccess ? TPIV_OK : hip_fail(he, "launch_stereo_triangulate");
}

static int particle_frames(const char* who, const uint8_t* frames, int n, int H, int W, int level, int capacity) {
    const std::string w(who);
    if (n < 0 || H < 3 || W < 3) return fail(TPIV_EINVAL, w + ": frames of at least 3 x 3 pixels");
    if (level < 0 || level > 255) return fail(TPIV_EINVAL, w + ": level must be in 0..255");
    if (capacity < 0) return fail(TPIV_EINVAL, w + ": negative capacity");
    if (!frames) return fail(TPIV_EINVAL, w + ": null pointer");
    if ((long long)H * W >= (1LL << 31) || (long long)n * (H + 1) >= (1LL << 31) || (long long)n * capacity >= (1LL << 31))
        return fail(TPIV_EINVAL, w + ": frames or lists too large");
    if (n > 65535) return fail(TPIV_EUNSUPPORTED, w + ": more than 65535 frames in one call");
    return TPIV_OK;
}

int tpiv_particle_count(const uint8_t* frames, int n, int H, int W, int level, const uint8_t* mask, int32_t* row_start,
                        int32_t* count, void* stream) {
    if (const int rc = particle_frames("tpiv_particle_count", frames, n, H, W, level, 0)) return rc;
    if (!row_start || !count) return fail(TPIV_EINVAL, "tpiv_particle_count: null pointer");
    if (n == 0) return TPIV_OK;
    const size_t px = (size_t)H * W;
    const Span in[2] = {{frames, n * px}, {mask, px}};
    const Span out[2] = {{row_start, (size_t)n * (H + 1) * 4}, {count, (size_t)n * 4}};
    if (const int k = aliased(in, 2, out, 2))
        return fail(TPIV_EINVAL, k == 1 ? "tpiv_particle_count: an output aliases an input" : "tpiv_particle_count: two outputs overlap");
    tpiv::ParticleParams q{};
    q.frames = frames;
    q.n = n;
    q.H = H;
    q.W = W;
    q.level = level;
    q.mask = mask;
    q.row_start = row_start;
    q.count = count;
    hipError_t he = tpiv::launch_particle_count(q, (hipStream_t)stream);
    return he == hipSuccess ? TPIV_OK : hip_fail(he, "launch_particle_count");
}

int tpiv_particle_detect(const uint8_t* frames, int n, int H, int W, int level, const uint8_t* mask, const double* table,
                         const int32_t* row_start, int capacity, double* x, double* y, uint8_t* peak, void* stream) {
    if (const int rc = particle_frames("tpiv_particle_detect", frames, n, H, W, level, capacity)) return rc;
    if (!row_start || !table || (capacity > 0 && (!x || !y || !peak)))
        return fail(TPIV_EINVAL, "tpiv_particle_detect: null pointer");
    if (n == 0 || capacity == 0) return TPIV_OK;
    const size_t px = (size_t)H * W, cells = (size_t)n * capacity;
    const Span in[4] = {{frames, n * px}, {mask, px}, {table, 256 * 8}, {row_start, (size_t)n * (H + 1) * 4}};
    const Span out[3] = {{x, cells * 8}, {y, cells * 8}, {peak, cells}};
    if (const int k = aliased(in, 4, out, 3))
        return fail(TPIV_EINVAL, k == 1 ? "tpiv_particle_detect: an output aliases an input" : "tpiv_particle_detect: two outputs overlap");
    tpiv::ParticleParams q{};
    q.frames = frames;
    q.n = n;
    q.H = H;
    q.W = W;
    q.level = level;
    q.mask = mask;
    q.table = table;
    q.row_start = const_cast<int32_t*>(row_start);      // (read only by the writing launch)
    q.capacity = capacity;
    q.x = x;
    q.y = y;
    q.peak = peak;
    hipError_t he = tpiv::launch_particle_detect(q, (hipStream_t)stream);
    return he == hipSuccess ? TPIV_OK : hip_fail(he, "launch_particle_detect");
}

int tpiv_particle_match(const double* xa, const double* ya, const int32_t* rsa, int cap_a, const double* xb, const double* yb,
                        const int32_t* rsb, int cap_b, int n, int H, int W, const double* up, const double* vp, int n_rows,
                        int n_cols, const double* xc, const double* yc, double radius, int32_t* match, uint8_t* status,
                        double* d2, int32_t* matched, void* work, size_t work_bytes, void* stream) {
    if (n < 0 || H < 1 || W < 1 || n_rows < 1 || n_cols < 1) return fail(TPIV_EINVAL, "tpiv_particle_match: empty frame or grid");
    if (cap_a < 0 || cap_b < 0) return fail(TPIV_EINVAL, "tpiv_particle_match: negative capacity");
    if (!(radius > 0) || !std::isfinite(radius)) return fail(TPIV_EINVAL, "tpiv_particle_match: radius must be a positive finite number");
    if (!rsa || !rsb || !up || !vp || !xc || !yc || !matched || (cap_a > 0 && (!xa || !ya || !match || !status || !d2))
        || (cap_b > 0 && (!xb || !yb)))
        return fail(TPIV_EINVAL, "tpiv_particle_match: null pointer");
    const long long lim = 1LL << 31;
    if ((long long)n * (H + 1) >= lim || (long long)n * cap_a >= lim || (long long)n * cap_b >= lim
        || (long long)n * n_rows * n_cols >= lim)
        return fail(TPIV_EINVAL, "tpiv_particle_match: lists or field stack too large");
    if (n > 65535) return fail(TPIV_EUNSUPPORTED, "tpiv_particle_match: more than 65535 pairs in one call");
    if (n == 0) return TPIV_OK;
    const size_t na = (size_t)n * cap_a, nb = (size_t)n * cap_b, need = 16 * nb;
    if (need > 0 && (!work || work_bytes < need || ((uintptr_t)work & 7) != 0))
        return fail(TPIV_EINVAL, "tpiv_particle_match: work memory of 16 * n * cap_b bytes, 8-byte aligned");
    const size_t rs = (size_t)n * (H + 1) * 4, cells = (size_t)n * n_rows * n_cols * 8;
    const Span in[10] = {{xa, na * 8}, {ya, na * 8}, {rsa, rs}, {xb, nb * 8}, {yb, nb * 8}, {rsb, rs}, {up, cells}, {vp, cells},
                         {xc, (size_t)n_cols * 8}, {yc, (size_t)n_rows * 8}};
    const Span out[5] = {{match, na * 4}, {status, na}, {d2, na * 8}, {matched, (size_t)n * 4}, {work, need}};
    if (const int k = aliased(in, 10, out, 5))
        return fail(TPIV_EINVAL, k == 1 ? "tpiv_particle_match: an output aliases an input" : "tpiv_particle_match: two outputs overlap");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(matched, 0, (size_t)n * 4, st));
    if (need > 0) HIP_TRY(hipMemsetAsync(work, 0xff, need, st));
    tpiv::ParticleMatchParams q{};
    q.xa = xa;
    q.ya = ya;
    q.rsa = rsa;
    q.cap_a = cap_a;
    q.xb = xb;
    q.yb = yb;
    q.rsb = rsb;
    q.cap_b = cap_b;
    q.n = n;
    q.H = H;
    q.W = W;
    q.up = up;
    q.vp = vp;
    q.n_rows = n_rows;
    q.n_cols = n_cols;
    q.xc = xc;
    q.yc = yc;
    q.radius = radius;
    q.match = match;
    q.status = status;
    q.d2 = d2;
    q.matched = matched;
    q.claim_d2 = (unsigned long long*)work;
    q.claim_i = (unsigned*)((char*)work + 8 * nb);
    hipError_t he = tpiv::launch_particle_match(q, st);
    return he == hipSuccess ? TPIV_OK : hip_fail(he, "launch_particle_match");
}

int tpiv_plan_set_outlier(tpiv_plan* plan, int kind, double threshold, double eps, int min_neighbours) {
    if (!plan) return fail(TPIV_EINVAL, "null plan");
    if (kind != 0 && kind != 1) return fail(TPIV_EINVAL, "tpiv_plan_set_outlier: kind must be 0 (off) or 1 (normalized median)");
    if (kind == 0) {
        plan->outlier_kind = 0;
        return TPIV_OK;
    }
    if (!(threshold > 0) || !(eps >= 0)) return fail(TPIV_EINVAL, "tpiv_plan_set_outlier: threshold must be > 0 and eps >= 0");
    if (min_neighbours < 1 || min_neighbours > 8) return fail(TPIV_EINVAL, "tpiv_plan_set_outlier: min_neighbours must be in 1..8");
    if (plan->ostatus.empty()) {                     // first time on: the workspace (kept until the plan is destroyed)
        int rc = check_plan_device(plan);
        if (rc) return rc;
        std::vector<uint8_t*> status(plan->n_pass, nullptr);
        size_t spare = 0;
        for (int p = 0; p < plan->n_pass && !rc; ++p) {
            const size_t N = (size_t)plan->geo[p].n_rows * plan->geo[p].n_cols;
            rc = plan->alloc(&status[p], N * plan->max_batch);
            if (p < plan->n_pass - 1 && N > spare) spare = N;
        }
        const PassGeo& g = plan->geo[plan->n_pass - 1];
        if (!rc && spare) rc = plan->alloc(&plan->raw_u, spare * plan->max_batch);
        if (!rc && spare) rc = plan->alloc(&plan->raw_v, spare * plan->max_batch);
        if (!rc) rc = plan->alloc(&plan->raw_val, (size_t)g.n_rows * g.n_cols * plan->max_batch);
        if (rc) return rc;                           // (what was allocated stays in plan->allocs and goes with the plan)
        plan->ostatus = std::move(status);
    }
    plan->outlier_kind = kind;
    plan->outlier_threshold = threshold;
    plan->outlier_eps = eps;
    plan->outlier_min = min_neighbours;
    return TPIV_OK;
}

int tpiv_plan_pass_outliers(const tpiv_plan* plan, int pass, uint8_t** status) {
    if (!plan || !status || pass < 0 || pass >= plan->n_pass) return fail(TPIV_EINVAL, "bad plan / pass index");
    if (!plan->outlier_kind) return fail(TPIV_EINVAL, "the plan runs no outlier test (tpiv_plan_set_outlier)");
    *status = plan->ostatus[pass];
    return TPIV_OK;
}

int tpiv_apply_mask(const uint8_t* frames, int n, long long pixels, const uint8_t* mask, uint8_t* out, void* stream) {
    if (n < 0 || pixels <= 0) return fail(TPIV_EINVAL, "tpiv_apply_mask: bad shape");
    if (n == 0) return TPIV_OK;
    if (!frames || !mask || !out) return fail(TPIV_EINVAL, "tpiv_apply_mask: null pointer");
    if (out != frames && out < frames + (size_t)n * pixels && frames < out + (size_t)n * pixels)
        return fail(TPIV_EINVAL, "tpiv_apply_mask: out overlaps frames without being frames");
    HIP_TRY(tpiv::launch_apply_mask(frames, n, pixels, mask, out, (hipStream_t)stream));
    return TPIV_OK;
}

// the window sizes a plan accepts for a mask grid: check_window's, from 8 on
static int check_mask_window(int H, int W, int ws, int ov) {
    if (int rc = check_window(H, W, ws, ov, 0)) return rc;
    if (ws < 8) return fail(TPIV_EUNSUPPORTED, "mask: window size must be in 8..256 (got " + std::to_string(ws) + ")");
    return TPIV_OK;
}

int tpiv_mask_coverage(const uint8_t* mask, int H, int W, int ws, int ov, int32_t* count, void* stream) {
    if (!mask || !count) return fail(TPIV_EINVAL, "tpiv_mask_coverage: null pointer");
    if (int rc = check_mask_window(H, W, ws, ov)) return rc;
    int nr = 0, nc = 0;
    field_shape(H, W, ws, ov, &nr, &nc);
    HIP_TRY(tpiv::launch_mask_coverage(mask, H, W, ws, ov, nr, nc, count, nullptr, 0, (hipStream_t)stream));
    return TPIV_OK;
}

int tpiv_mask_fields(double* u, double* v, uint8_t* invalid, uint8_t* status, const uint8_t* grid, int batch, int n_rows,
                     int n_cols, int invalid_value, void* stream) {
    if (batch < 0 || n_rows < 1 || n_cols < 1) return fail(TPIV_EINVAL, "tpiv_mask_fields: empty grid");
    if (invalid_value != 0 && invalid_value != 1) return fail(TPIV_EINVAL, "tpiv_mask_fields: invalid_value must be 0 or 1");
    if ((long long)n_rows * n_cols >= (1LL << 31)) return fail(TPIV_EUNSUPPORTED, "field too large");
    if (batch == 0) return TPIV_OK;
    if (!u || !v || !invalid || !grid) return fail(TPIV_EINVAL, "tpiv_mask_fields: null pointer");
    HIP_TRY(tpiv::launch_mask_fields(u, v, invalid, status, grid, batch, n_rows, n_cols, invalid_value, (hipStream_t)stream));
    return TPIV_OK;
}

int tpiv_plan_set_mask(tpiv_plan* plan, const uint8_t* mask, double threshold, void* stream) {
    if (!plan) return fail(TPIV_EINVAL, "null plan");
    if (!mask) {
        plan->mask_on = false;
        return TPIV_OK;
    }
    if (!(threshold >= 0.0 && threshold <= 1.0)) return fail(TPIV_EINVAL, "tpiv_plan_set_mask: threshold must be in [0, 1]");
    if (int rc = check_plan_device(plan)) return rc;
    for (const PassGeo& g : plan->geo)
        if (int rc = check_mask_window(plan->H, plan->W, g.ws, g.ov)) return rc;
    if (plan->mgrid.empty()) {                       // first time on: the grids (kept until the plan is destroyed)
        std::vector<uint8_t*> grids(plan->n_pass, nullptr);
        for (int p = 0; p < plan->n_pass; ++p)
            if (int rc = plan->alloc(&grids[p], (size_t)plan->geo[p].n_rows * plan->geo[p].n_cols)) return rc;
        plan->mgrid = std::move(grids);
    }
    plan->mask_on = false;                           // (stays off if a launch below fails)
    for (int p = 0; p < plan->n_pass; ++p) {
        const PassGeo& g = plan->geo[p];
        const int limit = (int)(threshold * (double)(g.ws * g.ws));       // one float64 product, truncated
        HIP_TRY(tpiv::launch_mask_coverage(mask, plan->H, plan->W, g.ws, g.ov, g.n_rows, g.n_cols, nullptr, plan->mgrid[p],
                                           limit, (hipStream_t)stream));
    }
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));       // the caller may let go of the image
    plan->mask_on = true;
    return TPIV_OK;
}

int tpiv_plan_pass_mask(const tpiv_plan* plan, int pass, uint8_t** grid) {
    if (!plan || !grid || pass < 0 || pass >= plan->n_pass) return fail(TPIV_EINVAL, "bad plan / pass index");
    if (!plan->mask_on) return fail(TPIV_EINVAL, "the plan has no mask (tpiv_plan_set_mask)");
    *grid = plan->mgrid[pass];
    return TPIV_OK;
}

int tpiv_apply_mask_pairs(const uint8_t* frames, int n, long long pixels, const uint8_t* masks, uint8_t* out, void* stream) {
    if (n < 0 || pixels <= 0) return fail(TPIV_EINVAL, "tpiv_apply_mask_pairs: bad shape");
    if (n == 0) return TPIV_OK;
    if (!frames || !masks || !out) return fail(TPIV_EINVAL, "tpiv_apply_mask_pairs: null pointer");
    const size_t bytes = (size_t)n * pixels;
    if (out != frames && out < frames + bytes && frames < out + bytes)
        return fail(TPIV_EINVAL, "tpiv_apply_mask_pairs: out overlaps frames without being frames");
    if (out < masks + bytes && masks < out + bytes) return fail(TPIV_EINVAL, "tpiv_apply_mask_pairs: out overlaps the masks");
    HIP_TRY(tpiv::launch_apply_mask_pairs(frames, n, pixels, masks, out, (hipStream_t)stream));
    return TPIV_OK;
}

int tpiv_mask_coverage_pairs(const uint8_t* masks, int n, int H, int W, int ws, int ov, int32_t* count, void* stream) {
    if (n < 0) return fail(TPIV_EINVAL, "tpiv_mask_coverage_pairs: bad shape");
    if (int rc = check_mask_window(H, W, ws, ov)) return rc;
    if (n == 0) return TPIV_OK;
    if (!masks || !count) return fail(TPIV_EINVAL, "tpiv_mask_coverage_pairs: null pointer");
    int nr = 0, nc = 0;
    field_shape(H, W, ws, ov, &nr, &nc);
    HIP_TRY(tpiv::launch_mask_coverage_pairs(masks, n, H, W, ws, ov, nr, nc, count, nullptr, 0, (hipStream_t)stream));
    return TPIV_OK;
}

int tpiv_mask_fields_pairs(double* u, double* v, uint8_t* invalid, uint8_t* status, const uint8_t* grids, int batch,
                           int n_rows, int n_cols, int invalid_value, void* stream) {
    if (batch < 0 || n_rows < 1 || n_cols < 1) return fail(TPIV_EINVAL, "tpiv_mask_fields_pairs: empty grid");
    if (invalid_value != 0 && invalid_value != 1)
        return fail(TPIV_EINVAL, "tpiv_mask_fields_pairs: invalid_value must be 0 or 1");
    if ((long long)n_rows * n_cols >= (1LL << 31)) return fail(TPIV_EUNSUPPORTED, "field too large");
    if (batch == 0) return TPIV_OK;
    if (!u || !v || !invalid || !grids) return fail(TPIV_EINVAL, "tpiv_mask_fields_pairs: null pointer");
    HIP_TRY(tpiv::launch_mask_fields_pairs(u, v, invalid, status, grids, batch, n_rows, n_cols, invalid_value,
                                           (hipStream_t)stream));
    return TPIV_OK;
}

size_t tpiv_dynamic_mask_work_bytes(int n, int H, int W) {
    if (n <= 0 || H <= 0 || W <= 0 || H > (1 << 28) || W > (1 << 28)) return 0;
    return (size_t)n * H * W;
}

int tpiv_dynamic_mask(const uint8_t* a, const uint8_t* b, int n, int H, int W, int kind, int size, int level, int grow,
                      const uint8_t* fixed, uint8_t* masks, void* work, void* stream) {
    if (n < 0 || H <= 0 || W <= 0 || H > (1 << 28) || W > (1 << 28)) return fail(TPIV_EINVAL, "tpiv_dynamic_mask: bad shape");
    if ((H + tpiv::PREFILTER_TILE_ROWS - 1) / tpiv::PREFILTER_TILE_ROWS > 65535)
        return fail(TPIV_EINVAL, "tpiv_dynamic_mask: more than 65535 tile rows");
    if (kind != TPIV_DYNMASK_BRIGHT && kind != TPIV_DYNMASK_DARK)
        return fail(TPIV_EINVAL, "tpiv_dynamic_mask: kind must be TPIV_DYNMASK_BRIGHT or TPIV_DYNMASK_DARK");
    if (size < 3 || size > 63 || size % 2 == 0) return fail(TPIV_EINVAL, "tpiv_dynamic_mask: size must be odd and in 3..63");
    if (level < 0 || level > 255) return fail(TPIV_EINVAL, "tpiv_dynamic_mask: level must be in 0..255");
    if (grow < 0 || size / 2 + grow > 31) return fail(TPIV_EINVAL, "tpiv_dynamic_mask: grow must be >= 0 with size / 2 + grow <= 31");
    if (n == 0) return TPIV_OK;
    if (!a || !b || !masks || !work) return fail(TPIV_EINVAL, "tpiv_dynamic_mask: null pointer");
    const size_t bytes = (size_t)n * H * W, image = (size_t)H * W;
    uint8_t* core = static_cast<uint8_t*>(work);
    auto overlaps = [](const uint8_t* x, size_t nx, const uint8_t* y, size_t ny) { return x < y + ny && y < x + nx; };
    if (overlaps(masks, bytes, a, bytes) || overlaps(masks, bytes, b, bytes) || overlaps(core, bytes, a, bytes) ||
        overlaps(core, bytes, b, bytes) || overlaps(core, bytes, masks, bytes) ||
        (fixed && (overlaps(masks, bytes, fixed, image) || overlaps(core, bytes, fixed, image))))
        return fail(TPIV_EINVAL, "tpiv_dynamic_mask: the masks and the workspace overlap neither each other nor an input");
    HIP_TRY(tpiv::launch_dynamic_mask(a, b, n, H, W, kind, size, level, grow, fixed, masks, core, (hipStream_t)stream));
    return TPIV_OK;
}

int tpiv_plan_set_pair_masks(tpiv_plan* plan, int on) {
    if (!plan) return fail(TPIV_EINVAL, "null plan");
    if (!on) {
        plan->pair_on = false;
        return TPIV_OK;
    }
    if (int rc = refuse_combination(plan, F_PAIR_MASKS)) return rc;
    if (int rc = check_plan_device(plan)) return rc;
    for (const PassGeo& g : plan->geo)
        if (int rc = check_mask_window(plan->H, plan->W, g.ws, g.ov)) return rc;
    if (plan->pgrid.empty()) {                       // first time on: the grids (kept until the plan is destroyed)
        std::vector<uint8_t*> grids(plan->n_pass, nullptr);
        for (int p = 0; p < plan->n_pass; ++p)
            if (int rc = plan->alloc(&grids[p], (size_t)plan->geo[p].n_rows * plan->geo[p].n_cols * plan->max_batch)) return rc;
        plan->pgrid = std::move(grids);
    }
    plan->pair_on = true;
    return TPIV_OK;
}

int tpiv_plan_pass_pair_mask(const tpiv_plan* plan, int pass, uint8_t** grid) {
    if (!plan || !grid || pass < 0 || pass >= plan->n_pass) return fail(TPIV_EINVAL, "bad plan / pass index");
    if (!plan->pair_on) return fail(TPIV_EINVAL, "the plan has no per-pair masks (tpiv_plan_set_pair_masks)");
    *grid = plan->pgrid[pass];
    return TPIV_OK;
}

static int run_uncertainty(const uint8_t* a, const uint8_t* b, int batch, int H, int W, int ws, int ov, int n_rows,
                           int n_cols, const double* u, const double* v, const uint8_t* invalid, const uint8_t* exclude,
                           int radius, double* su, double* sv, long long* stats, hipStream_t st, bool exclude_pairs = false) {
    tpiv::UncertaintyParams q{};
    q.A = a;
    q.B = b;
    q.batch = batch;
    q.H = H;
    q.W = W;
    q.ws = ws;
    q.ov = ov;
    q.n_rows = n_rows;
    q.n_cols = n_cols;
    q.u = u;
    q.v = v;
    q.invalid = invalid;
    q.exclude = exclude;
    q.exclude_stride = exclude_pairs ? n_rows * n_cols : 0;
    q.radius = radius;
    q.su = su;
    q.sv = sv;
    q.stats = stats;
    hipError_t he = tpiv::launch_uncertainty(q, st);
    return he == hipSuccess ? TPIV_OK : hip_fail(he, "launch_uncertainty");
}

// the sizes tpiv_uncertainty covers: its integer bounds hold for ws <= 128 and radius <= 4
static int check_uncertainty(int H, int W, int ws, int ov, int radius) {
    if (ws < tpiv::UNCERTAINTY_MIN_WS || ws > tpiv::UNCERTAINTY_MAX_WS)
        return fail(TPIV_EINVAL, "uncertainty: window size must be in 4..128 (got " + std::to_string(ws) + ")");
    if (ov < 0 || ov >= ws) return fail(TPIV_EINVAL, "uncertainty: overlap must be in 0..ws-1");
    if (radius < 0 || radius > tpiv::UNCERTAINTY_MAX_RADIUS)
        return fail(TPIV_EINVAL, "uncertainty: radius must be in 0..4 (got " + std::to_string(radius) + ")");
    if (H < ws || W < ws) return fail(TPIV_EINVAL, "uncertainty: the frame holds no window");
    if (H >= (1 << 22) || W >= (1 << 22) || (long long)H * W >= (1LL << 30))
        return fail(TPIV_EINVAL, "uncertainty: frame too large");      // Q8 coordinates and flat indices in 32 bits
    return TPIV_OK;
}

int tpiv_uncertainty(const uint8_t* a, const uint8_t* b, int batch, int H, int W, int ws, int ov, const double* u,
                     const double* v, const uint8_t* invalid, int radius, double* su, double* sv, long long* stats,
                     void* stream) {
    if (batch < 0) return fail(TPIV_EINVAL, "tpiv_uncertainty: negative batch");
    if (int rc = check_uncertainty(H, W, ws, ov, radius)) return rc;
    if (batch == 0) return TPIV_OK;
    if (!a || !b || !u || !v || !su || !sv) return fail(TPIV_EINVAL, "tpiv_uncertainty: null pointer");
    int nr = 0, nc = 0;
    field_shape(H, W, ws, ov, &nr, &nc);
    if ((long long)batch * nr * nc >= (1LL << 31)) return fail(TPIV_EINVAL, "tpiv_uncertainty: batch of fields too large");
    const size_t cells = (size_t)batch * nr * nc, pixels = (size_t)batch * H * W;
    const Span in[5] = {{a, pixels}, {b, pixels}, {u, cells * 8}, {v, cells * 8}, {invalid, cells}};
    const Span out[3] = {{su, cells * 8}, {sv, cells * 8}, {stats, cells * 64}};
    if (const int k = aliased(in, 5, out, 3))
        return fail(TPIV_EINVAL, k == 1 ? "tpiv_uncertainty: an output overlaps an input" : "tpiv_uncertainty: two outputs overlap");
    return run_uncertainty(a, b, batch, H, W, ws, ov, nr, nc, u, v, invalid, nullptr, radius, su, sv, stats,
                           (hipStream_t)stream);
}

int tpiv_plan_set_uncertainty(tpiv_plan* plan, int kind, int radius) {
    if (!plan) return fail(TPIV_EINVAL, "null plan");
    if (kind != 0 && kind != 1)
        return fail(TPIV_EINVAL, "tpiv_plan_set_uncertainty: kind must be 0 (off) or 1 (correlation statistics)");
    if (kind == 0) {
        plan->unc_kind = 0;
        return TPIV_OK;
    }
    if (int rc = refuse_combination(plan, F_UNCERTAINTY)) return rc;
    const PassGeo& g = plan->geo[plan->n_pass - 1];
    if (int rc = check_uncertainty(plan->H, plan->W, g.ws, g.ov, radius)) return rc;
    if (!plan->unc_su) {                             // first time on: the two fields (kept until the plan is destroyed)
        if (int rc = check_plan_device(plan)) return rc;
        const size_t n = (size_t)g.n_rows * g.n_cols * plan->max_batch;
        double *su = nullptr, *sv = nullptr;
        if (int rc = plan->alloc(&su, n)) return rc;
        if (int rc = plan->alloc(&sv, n)) return rc;
        plan->unc_su = su;
        plan->unc_sv = sv;
    }
    plan->unc_kind = kind;
    plan->unc_radius = radius;
    return TPIV_OK;
}

int tpiv_plan_uncertainty(const tpiv_plan* plan, double** su, double** sv) {
    if (!plan || !su || !sv) return fail(TPIV_EINVAL, "bad plan / null pointer");
    if (!plan->unc_kind) return fail(TPIV_EINVAL, "the plan estimates no uncertainty (tpiv_plan_set_uncertainty)");
    *su = plan->unc_su;
    *sv = plan->unc_sv;
    return TPIV_OK;
}

// ---- iterative image deformation (deform.hip) ---------------------------------------------------------------------

namespace {
int check_deform_grid(const char* who, int batch, int n_rows, int n_cols) {
    if (batch < 0) return fail(TPIV_EINVAL, std::string(who) + ": negative batch");
    if (n_rows < 1 || n_cols < 1) return fail(TPIV_EINVAL, std::string(who) + ": empty grid");
    if (batch > 65535 || (n_rows + 15) / 16 > 65535) return fail(TPIV_EINVAL, std::string(who) + ": batch or grid too large");
    if ((long long)batch * n_rows * n_cols >= (1LL << 31)) return fail(TPIV_EINVAL, std::string(who) + ": batch of fields too large");
    return TPIV_OK;
}
// the frames and geometries tpiv_deform_warp covers
int check_deform_frame(int H, int W, int ws, int ov) {
    if (ws < 2 || ws > 256) return fail(TPIV_EINVAL, "deform: window size must be in 2..256 (got " + std::to_string(ws) + ")");
    if (ov < 0 || ov >= ws) return fail(TPIV_EINVAL, "deform: overlap must be in 0..ws-1");
    if (H < ws || W < ws) return fail(TPIV_EINVAL, "deform: the frame holds no window");
    if (H >= (1 << 22) || W >= (1 << 22) || (long long)H * W >= (1LL << 30))
        return fail(TPIV_EINVAL, "deform: frame too large");         // Q8 coordinates and flat indices in 32 bits
    if ((H + 31) / 32 > 65535) return fail(TPIV_EINVAL, "deform: frame too tall");
    return TPIV_OK;
}
}  // namespace

int tpiv_deform_nodes(const double* u, const double* v, const uint8_t* invalid, int batch, int n_rows, int n_cols, int smooth,
                      int16_t* nodes, void* stream) {
    if (int rc = check_deform_grid("tpiv_deform_nodes", batch, n_rows, n_cols)) return rc;
    if (batch == 0) return TPIV_OK;
    if (!u || !v || !invalid || !nodes) return fail(TPIV_EINVAL, "tpiv_deform_nodes: null pointer");
    if ((uintptr_t)nodes & 3u) return fail(TPIV_EINVAL, "tpiv_deform_nodes: nodes must be 4-byte aligned");
    const size_t cells = (size_t)batch * n_rows * n_cols;
    const Span in[3] = {{u, cells * 8}, {v, cells * 8}, {invalid, cells}};
    const Span out[1] = {{nodes, cells * 4}};
    if (aliased(in, 3, out, 1)) return fail(TPIV_EINVAL, "tpiv_deform_nodes: the nodes overlap an input");
    HIP_TRY(tpiv::launch_deform_nodes(u, v, invalid, batch, n_rows, n_cols, smooth != 0, nodes, (hipStream_t)stream));
    return TPIV_OK;
}

int tpiv_deform_warp(const uint8_t* a, const uint8_t* b, int batch, int H, int W, int ws, int ov, const int16_t* nodes,
                     const int16_t* table, int interp, uint8_t* wa, uint8_t* wb, int32_t* counter, void* stream) {
    const int kind = interp & ~TPIV_DEFORM_GATHER;
    if (kind != TPIV_DEWARP_LINEAR && kind != TPIV_DEWARP_CUBIC) return fail(TPIV_EINVAL, "tpiv_deform_warp: unknown interp");
    if (int rc = check_deform_frame(H, W, ws, ov)) return rc;
    int nr = 0, nc = 0;
    field_shape(H, W, ws, ov, &nr, &nc);
    if (int rc = check_deform_grid("tpiv_deform_warp", batch, nr, nc)) return rc;
    if (batch == 0) return TPIV_OK;
    if (!a || !b || !nodes || !wa || !wb || (kind == TPIV_DEWARP_CUBIC && !table))
        return fail(TPIV_EINVAL, "tpiv_deform_warp: null pointer");
    if ((uintptr_t)nodes & 3u) return fail(TPIV_EINVAL, "tpiv_deform_warp: nodes must be 4-byte aligned");
    if (((uintptr_t)table & 7u) || ((uintptr_t)counter & 3u)) return fail(TPIV_EINVAL, "tpiv_deform_warp: misaligned table or counter");
    const size_t cells = (size_t)batch * nr * nc, pixels = (size_t)batch * H * W;
    const Span in[4] = {{a, pixels}, {b, pixels}, {nodes, cells * 4}, {table, kind == TPIV_DEWARP_CUBIC ? (size_t)2048 : 0}};
    const Span out[3] = {{wa, pixels}, {wb, pixels}, {counter, 8}};
    if (aliased(in, 4, out, 3)) return fail(TPIV_EINVAL, "tpiv_deform_warp: an output overlaps an input or another output");
    tpiv::DeformWarpParams q{};
    q.A = a;
    q.B = b;
    q.batch = batch;
    q.H = H;
    q.W = W;
    q.ws = ws;
    q.ov = ov;
    q.n_rows = nr;
    q.n_cols = nc;
    q.nodes = nodes;
    q.table = table;
    q.interp = kind;
    q.force_gather = (interp & TPIV_DEFORM_GATHER) != 0;
    q.wa = wa;
    q.wb = wb;
    q.counter = counter;
    HIP_TRY(tpiv::launch_deform_warp(q, (hipStream_t)stream));
    return TPIV_OK;
}

int tpiv_deform_combine(const int16_t* nodes, const double* du, const double* dv, const uint8_t* dval, int batch, int n_rows,
                        int n_cols, double* u, double* v, uint8_t* invalid, void* stream) {
    if (int rc = check_deform_grid("tpiv_deform_combine", batch, n_rows, n_cols)) return rc;
    if (batch == 0) return TPIV_OK;
    if (!nodes || !du || !dv || !dval || !u || !v || !invalid) return fail(TPIV_EINVAL, "tpiv_deform_combine: null pointer");
    if ((uintptr_t)nodes & 3u) return fail(TPIV_EINVAL, "tpiv_deform_combine: nodes must be 4-byte aligned");
    const size_t cells = (size_t)batch * n_rows * n_cols;
    const Span in[4] = {{nodes, cells * 4}, {du, cells * 8}, {dv, cells * 8}, {dval, cells}};
    const Span out[3] = {{u, cells * 8}, {v, cells * 8}, {invalid, cells}};
    if (aliased(in, 4, out, 3)) return fail(TPIV_EINVAL, "tpiv_deform_combine: an output overlaps an input or another output");
    HIP_TRY(tpiv::launch_deform_combine(nodes, du, dv, dval, cells, u, v, invalid, (hipStream_t)stream));
    return TPIV_OK;
}

int tpiv_plan_set_deform(tpiv_plan* plan, int iterations, int interp, int smooth, const int16_t* table) {
    if (!plan) return fail(TPIV_EINVAL, "null plan");
    if (iterations < 0 || iterations > 8) return fail(TPIV_EINVAL, "tpiv_plan_set_deform: iterations must be in 0..8");
    if (iterations == 0) {
        plan->def_iters = 0;
        return TPIV_OK;
    }
    if (int rc = refuse_combination(plan, F_DEFORM)) return rc;
    if (interp != TPIV_DEWARP_LINEAR && interp != TPIV_DEWARP_CUBIC) return fail(TPIV_EINVAL, "tpiv_plan_set_deform: unknown interp");
    if (interp == TPIV_DEWARP_CUBIC && !table) return fail(TPIV_EINVAL, "tpiv_plan_set_deform: the cubic interpolation needs its table");
    const PassGeo& g = plan->geo[plan->n_pass - 1];
    if (check_window(plan->H, plan->W, g.ws, g.ov, plan->val_win)) {              // what tpiv_pass1 refuses
        const std::string why = g_err;
        return fail(TPIV_EINVAL, "tpiv_plan_set_deform: the first pass refuses the last pass's geometry: " + why);
    }
    if (int rc = check_deform_frame(plan->H, plan->W, g.ws, g.ov)) return rc;
    if (int rc = check_deform_grid("tpiv_plan_set_deform", plan->max_batch, g.n_rows, g.n_cols)) return rc;
    if (int rc = check_plan_device(plan)) return rc;
    if (!plan->def_nodes) {                          // first time on: the workspace (kept until the plan is destroyed)
        const size_t n = (size_t)g.n_rows * g.n_cols * plan->max_batch, px = (size_t)plan->H * plan->W * plan->max_batch;
        int16_t *nodes = nullptr, *tab = nullptr;
        uint8_t *wa = nullptr, *wb = nullptr, *dval = nullptr;
        double *du = nullptr, *dv = nullptr, *su = nullptr, *sv = nullptr;
        int rc = plan->alloc(&nodes, 2 * n);
        if (!rc) rc = plan->alloc(&tab, 1024);
        if (!rc) rc = plan->alloc(&wa, px);
        if (!rc) rc = plan->alloc(&wb, px);
        if (!rc) rc = plan->alloc(&du, n);
        if (!rc) rc = plan->alloc(&dv, n);
        if (!rc) rc = plan->alloc(&dval, n);
        if (!rc) rc = plan->alloc(&su, n);
        if (!rc) rc = plan->alloc(&sv, n);
        if (rc) return rc;                           // (what was allocated stays in plan->allocs and goes with the plan)
        const size_t need = tpiv::peak_raw_bytes(g.ws, plan->max_batch, g.n_rows * g.n_cols, plan->precision);
        if (need > plan->peak_raw_bytes) {           // pass 1 at the last geometry needs more than any pass of the plan
            float* raw = nullptr;
            if (int rc2 = plan->alloc(&raw, need / sizeof(float) + 64)) return rc2;
            plan->peak_raw = raw;
            plan->peak_raw_bytes = need;
        }
        for (hipEvent_t& e : plan->def_ev)
            if (!e) HIP_TRY(hipEventCreate(&e));
        plan->def_table = tab;
        plan->def_wa = wa;
        plan->def_wb = wb;
        plan->def_du = du;
        plan->def_dv = dv;
        plan->def_dval = dval;
        plan->def_su = su;
        plan->def_sv = sv;
        plan->def_nodes = nodes;
    }
    if (table) HIP_TRY(hipMemcpy(plan->def_table, table, 1024 * sizeof(int16_t), hipMemcpyDeviceToDevice));
    plan->def_iters = iterations;
    plan->def_interp = interp;
    plan->def_smooth = smooth != 0;
    plan->def_ran = false;
    return TPIV_OK;
}

int tpiv_plan_deform_stage(const tpiv_plan* plan, int16_t** nodes, uint8_t** wa, uint8_t** wb, double** du, double** dv,
                           uint8_t** dval) {
    if (!plan) return fail(TPIV_EINVAL, "null plan");
    if (!plan->def_iters) return fail(TPIV_EINVAL, "the plan deforms no images (tpiv_plan_set_deform)");
    if (nodes) *nodes = plan->def_nodes;
    if (wa) *wa = plan->def_wa;
    if (wb) *wb = plan->def_wb;
    if (du) *du = plan->def_du;
    if (dv) *dv = plan->def_dv;
    if (dval) *dval = plan->def_dval;
    return TPIV_OK;
}

int tpiv_plan_deform_ms(tpiv_plan* plan, double* ms) {
    if (!plan || !ms) return fail(TPIV_EINVAL, "bad plan / null pointer");
    if (!plan->def_iters) return fail(TPIV_EINVAL, "the plan deforms no images (tpiv_plan_set_deform)");
    if (!plan->def_ran) return fail(TPIV_EINVAL, "the plan has not run yet");
    HIP_TRY(hipEventSynchronize(plan->def_ev[1]));
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, plan->def_ev[0], plan->def_ev[1]));
    *ms = (double)t;
    return TPIV_OK;
}

namespace {
// What a plan enqueues behind a stage, a pass or a deformation round, at geometry p: the mask step, the median test, the
// mask step once more on what the test wrote (the header has the order and its reasons, at tpiv_plan_set_outlier,
// tpiv_plan_set_mask and tpiv_plan_set_deform).  Built before the stage, it also says where the stage writes: with the test
// on, what the test rewrites goes somewhere else, and the test puts it where the next reader or the caller expects it.
//   feeds:            another stage reads u, v next: the predictor behind a pass, the next round's nodes behind a round;
//                     the test then replaces the vectors, and otherwise only flags them in the caller's mask
//   excluded_invalid: cells that the mask excludes stay invalid in what the stage hands on
struct Settle {
    const tpiv_plan* plan;
    int p;
    bool test, feeds, excluded_invalid;
    double *u, *v;              // where the next reader or the caller expects the stage's fields ...
    uint8_t* invalid;
    double *wu, *wv;            // ... and where the stage writes them
    uint8_t* wval;

    Settle(const tpiv_plan* plan_, int p_, bool feeds_, bool excluded_invalid_, double* u_, double* v_, uint8_t* invalid_,
           double* spare_u, double* spare_v)
        : plan(plan_), p(p_), test(plan_->outlier_kind != 0), feeds(feeds_), excluded_invalid(excluded_invalid_), u(u_), v(v_),
          invalid(invalid_), wu(test && feeds ? spare_u : u_), wv(test && feeds ? spare_v : v_),
          wval(test && !feeds ? plan_->raw_val : invalid_) {}

    int run(int batch, hipStream_t st) const {
        const PassGeo& g = plan->geo[p];
        const bool pairs = plan->pair_run;      // a masked run: one grid per pair in the place of the static one
        const uint8_t* grid = pairs ? plan->pgrid[p] : plan->mask_on ? plan->mgrid[p] : nullptr;
        auto mask = [&](double* mu, double* mv, uint8_t* mval, uint8_t* status, bool invalid_value) {
            hipError_t he = pairs ? tpiv::launch_mask_fields_pairs(mu, mv, mval, status, grid, batch, g.n_rows, g.n_cols,
                                                                   invalid_value, st)
                                  : tpiv::launch_mask_fields(mu, mv, mval, status, grid, batch, g.n_rows, g.n_cols,
                                                             invalid_value, st);
            return he == hipSuccess ? TPIV_OK : hip_fail(he, "launch_mask_fields");
        };
        if (grid)                   // excluded cells: zero vectors, and always invalid to the test
            if (int rc = mask(wu, wv, wval, nullptr, test || excluded_invalid)) return rc;
        if (!test) return TPIV_OK;
        if (int rc = run_median_test(wu, wv, wval, batch, g.n_rows, g.n_cols, plan->outlier_threshold, plan->outlier_eps,
                                     plan->outlier_min, plan->ostatus[p], feeds ? u : nullptr, feeds ? v : nullptr, 1,
                                     feeds ? nullptr : invalid, st))
            return rc;
        return grid ? mask(u, v, invalid, plan->ostatus[p], excluded_invalid) : TPIV_OK;
    }
};
}  // namespace

// the rounds of a deforming plan behind its last pass (tpiv_plan_set_deform has the order of the steps)
static int run_deform(tpiv_plan* plan, const uint8_t* a, const uint8_t* b, int batch, double* u, double* v, uint8_t* invalid,
                      void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int last = plan->n_pass - 1;
    const PassGeo& g = plan->geo[last];
    const size_t cells = (size_t)batch * g.n_rows * g.n_cols;
    HIP_TRY(hipEventRecord(plan->def_ev[0], st));
    // a weighted plan's residual pass is the weighted first pass with the last pass's tables
    const tpiv::WinParams wp{plan->wt_kind ? plan->wt_tab[last] : nullptr};
    for (int k = 1; k <= plan->def_iters; ++k) {
        // excluded cells stay valid behind every round, so that they pull the warp to zero at a wall
        const Settle settle(plan, last, k < plan->def_iters, false, u, v, invalid, plan->def_su, plan->def_sv);
        HIP_TRY(tpiv::launch_deform_nodes(u, v, invalid, batch, g.n_rows, g.n_cols, plan->def_smooth, plan->def_nodes, st));
        tpiv::DeformWarpParams q{};
        q.A = a;
        q.B = b;
        q.batch = batch;
        q.H = plan->H;
        q.W = plan->W;
        q.ws = g.ws;
        q.ov = g.ov;
        q.n_rows = g.n_rows;
        q.n_cols = g.n_cols;
        q.nodes = plan->def_nodes;
        q.table = plan->def_table;
        q.interp = plan->def_interp;
        q.wa = plan->def_wa;
        q.wb = plan->def_wb;
        HIP_TRY(tpiv::launch_deform_warp(q, st));
        if (int rc = pass1_impl(plan->def_wa, plan->def_wb, batch, plan->H, plan->W, g.ws, g.ov, plan->val_ratio, plan->val_win,
                                plan->precision, plan->def_du, plan->def_dv, plan->def_dval, plan->peak_raw,
                                plan->peak_raw_bytes, nullptr, nullptr, stream, nullptr, nullptr, plan->wt_kind ? &wp : nullptr))
            return rc;
        HIP_TRY(tpiv::launch_deform_combine(plan->def_nodes, plan->def_du, plan->def_dv, plan->def_dval, cells, settle.wu,
                                            settle.wv, settle.wval, st));
        if (int rc = settle.run(batch, st)) return rc;
    }
    HIP_TRY(hipEventRecord(plan->def_ev[1], st));
    plan->def_ran = true;
    return TPIV_OK;
}

int tpiv_plan_run(tpiv_plan* plan, const uint8_t* a, const uint8_t* b, int batch, double* u, double* v,
                  uint8_t* invalid, void* stream) {
    if (!plan) return fail(TPIV_EINVAL, "null plan");
    if (batch < 0 || batch > plan->max_batch) return fail(TPIV_EINVAL, "batch exceeds the plan's max_batch");
    if (batch == 0) return TPIV_OK;
    if (int rc = check_plan_device(plan)) return rc;
    const int last = plan->n_pass - 1;
    plan->last_batch = batch;
    hipStream_t st = (hipStream_t)stream;
    auto mark = [&](int slot, int end) {
        hipEvent_t e = plan->ev(slot, end);
        if (e) (void)hipEventRecord(e, st);
    };
    for (int p = 0; p <= last; ++p) {
        const PassGeo& g = plan->geo[p];
        // a pass before the last keeps its fields in the plan for the predictor, to which excluded cells are invalid
        const Settle settle(plan, p, p < last, p < last, p == last ? u : plan->u[p], p == last ? v : plan->v[p],
                            p == last ? invalid : plan->val[p], plan->raw_u, plan->raw_v);
        double *const pu = settle.wu, *const pv = settle.wv;
        uint8_t* const pval = settle.wval;
        int rc;
        const tpiv::SpecParams sp = plan->corr_kind ? plan->spec(p) : tpiv::SpecParams{};
        const tpiv::SpecParams* const spec = plan->corr_kind ? &sp : nullptr;
        const tpiv::WinParams wp{plan->wt_kind ? plan->wt_tab[p] : nullptr};
        const tpiv::WinParams* const win = plan->wt_kind ? &wp : nullptr;
        if (p == 0) {
            mark(0, 0);
            rc = pass1_impl(a, b, batch, plan->H, plan->W, g.ws, g.ov, plan->val_ratio, plan->val_win,
                            plan->precision, pu, pv, pval, plan->peak_raw, plan->peak_raw_bytes, nullptr, nullptr,
                            stream, spec || win ? nullptr : plan->sub_events(), spec, win);
            mark(0, 1);
            if (!rc && plan->exact_count && !spec && !win) {
                const size_t off = tpiv::exact_fallback_count_offset(batch, g.n_rows * g.n_cols);
                HIP_TRY(hipMemcpyAsync(plan->exact_count, reinterpret_cast<const char*>(plan->peak_raw) + off,
                                       sizeof(unsigned), hipMemcpyDeviceToDevice, st));
            }
        } else {
            const PassGeo& c = plan->geo[p - 1];
            mark(2 * p - 1, 0);
            // compact hand-off: raw predictor (u0, v0) + mask byte; zeroing and half shift are formed by the readers
            rc = run_banded_predict(plan, p, batch, plan->u[p - 1], plan->v[p - 1], plan->val[p - 1], plan->u0,
                                    plan->v0, nullptr, nullptr, st, plan->pmask);
            mark(2 * p - 1, 1);
            mark(2 * p, 0);
            if (!rc)
                rc = run_iter(plan->mode, plan->precision, a, b, batch, plan->H, plan->W, g.ws, g.ov, plan->u0, plan->v0,
                              nullptr, nullptr, plan->val_ratio, plan->val_win, pu, pv, pval, nullptr,
                              nullptr, nullptr, nullptr, plan->peak_raw, plan->peak_raw_bytes, stream, plan->pmask, spec, win);
            mark(2 * p, 1);
        }
        if (rc) return rc;
        // (what follows goes behind the closing event of the pass's timing slot: the slots keep their meaning)
        rc = settle.run(batch, st);
        if (rc) return rc;
    }
    if (plan->def_iters) {   // behind the last pass, its mask and outlier steps and the closing event of its timing slot
        if (int rc = run_deform(plan, a, b, batch, u, v, invalid, stream)) return rc;
    }
    if (plan->unc_kind) {    // behind the last pass, its outlier and mask steps and the closing event of its timing slot
        const PassGeo& g = plan->geo[last];
        const double* uu = u;
        const double* vv = v;
        if (int rc = run_uncertainty(a, b, batch, plan->H, plan->W, g.ws, g.ov, g.n_rows, g.n_cols, uu, vv, invalid,
                                     plan->pair_run  ? plan->pgrid[last]
                                     : plan->mask_on ? plan->mgrid[last]
                                                     : nullptr,
                                     plan->unc_radius, plan->unc_su, plan->unc_sv, nullptr, st, plan->pair_run))
            return rc;
    }
    plan->last_filtered = plan->corr_kind != 0 || plan->wt_kind != 0;
    if (plan->timing && plan->runs_recorded < 512) {
        if (plan->sub_recorded.size() <= plan->runs_recorded) plan->sub_recorded.resize(plan->runs_recorded + 1, 0);
        plan->sub_recorded[plan->runs_recorded] = plan->exact_count != nullptr && !plan->last_filtered;
        plan->runs_recorded++;
    }
    return TPIV_OK;
}

int tpiv_plan_run_masked(tpiv_plan* plan, const uint8_t* a, const uint8_t* b, const uint8_t* masks, double threshold,
                         int batch, double* u, double* v, uint8_t* invalid, void* stream) {
    if (!plan) return fail(TPIV_EINVAL, "null plan");
    if (!plan->pair_on) return fail(TPIV_EINVAL, "the plan has no per-pair masks (tpiv_plan_set_pair_masks)");
    if (!(threshold >= 0.0 && threshold <= 1.0)) return fail(TPIV_EINVAL, "tpiv_plan_run_masked: threshold must be in [0, 1]");
    if (batch < 0 || batch > plan->max_batch) return fail(TPIV_EINVAL, "batch exceeds the plan's max_batch");
    if (batch == 0) return TPIV_OK;
    if (!masks) return fail(TPIV_EINVAL, "tpiv_plan_run_masked: null pointer");
    if (int rc = check_plan_device(plan)) return rc;
    for (int p = 0; p < plan->n_pass; ++p) {
        const PassGeo& g = plan->geo[p];
        const int limit = (int)(threshold * (double)(g.ws * g.ws));       // tpiv_plan_set_mask's rule
        HIP_TRY(tpiv::launch_mask_coverage_pairs(masks, batch, plan->H, plan->W, g.ws, g.ov, g.n_rows, g.n_cols, nullptr,
                                                 plan->pgrid[p], limit, (hipStream_t)stream));
    }
    plan->pair_run = true;
    const int rc = tpiv_plan_run(plan, a, b, batch, u, v, invalid, stream);
    plan->pair_run = false;
    return rc;
}

// ---- spectrally filtered passes and weighted windows: what their two setters share -----------------------------------

// The last step of tpiv_plan_set_correlation / _set_weighting, behind every refusal that needs no device.  Such a pass works in
// the float32 tile layout (records, item counters) whatever the plan's precision: a plan whose workspace was sized for
// float64 records alone gets a larger one (the old one is freed with the plan).  tabs (the plan's per-pass device tables,
// floats_of(ws) floats each) are allocated the first time and kept until the plan is destroyed; tables: all of them, pass
// after pass, on the host.  The plan's workspace changes only when everything else has succeeded.
static int install_pass_tables(tpiv_plan* plan, std::vector<float*>& tabs, const float* tables, size_t (*floats_of)(int ws)) {
    if (int rc = check_plan_device(plan)) return rc;
    size_t raw = 0;
    for (const PassGeo& g : plan->geo)
        raw = std::max(raw, tpiv::peak_raw_bytes(g.ws, plan->max_batch, g.n_rows * g.n_cols, TPIV_PREC_FAST));
    float* grown = nullptr;
    if (raw > plan->peak_raw_bytes)
        if (int rc = plan->alloc(&grown, raw / sizeof(float) + 64)) return rc;
    if (tabs.empty()) {
        std::vector<float*> fresh(plan->n_pass, nullptr);
        for (int p = 0; p < plan->n_pass; ++p)
            if (int rc = plan->alloc(&fresh[p], floats_of(plan->geo[p].ws))) return rc;
        tabs = std::move(fresh);
    }
    HIP_TRY(hipDeviceSynchronize());                 // no run in flight reads the tables while they change
    size_t off = 0;
    for (int p = 0; p < plan->n_pass; ++p) {
        const size_t n = floats_of(plan->geo[p].ws);
        HIP_TRY(hipMemcpy(tabs[p], tables + off, n * sizeof(float), hipMemcpyHostToDevice));
        off += n;
    }
    if (grown) {
        plan->peak_raw = grown;
        plan->peak_raw_bytes = raw;
    }
    return TPIV_OK;
}

// ---- spectrally filtered passes -------------------------------------------------------------------------------------

int tpiv_plan_set_correlation(tpiv_plan* plan, int kind, double dx, double dy, double floor, const float* tables,
                              size_t n_tables) {
    if (!plan) return fail(TPIV_EINVAL, "null plan");
    if (kind == TPIV_CORR_NONE) {
        plan->corr_kind = 0;
        return TPIV_OK;
    }
    if (int rc = check_correlation("tpiv_plan_set_correlation", kind, dx, dy, floor)) return rc;
    if (int rc = refuse_combination(plan, F_CORRELATION)) return rc;
    size_t need = 0;
    for (const PassGeo& g : plan->geo) {
        if (!tpiv::spec_size(g.ws))
            return fail(TPIV_EUNSUPPORTED, "correlation=: filtered passes cover window sizes 16, 32 and 64; this plan has a pass of " +
                                               std::to_string(g.ws));
        need += 2 * (size_t)(g.ws / 2 + 1);
    }
    if (!tables || n_tables != need)
        return fail(TPIV_EINVAL, "tpiv_plan_set_correlation: tables must hold g_y and g_x of every pass, " + std::to_string(need) +
                                     " floats in all");
    if (int rc = install_pass_tables(plan, plan->corr_tab, tables, [](int ws) { return 2 * (size_t)(ws / 2 + 1); })) return rc;
    plan->corr_kind = kind;
    plan->corr_floor = floor;
    return TPIV_OK;
}

// ---- weighted interrogation windows ---------------------------------------------------------------------------------

int tpiv_plan_set_weighting(tpiv_plan* plan, int kind, double sigma_x, double sigma_y, const float* tables, size_t n_tables) {
    if (!plan) return fail(TPIV_EINVAL, "null plan");
    if (kind == TPIV_WEIGHT_NONE) {
        plan->wt_kind = 0;
        return TPIV_OK;
    }
    if (kind != TPIV_WEIGHT_UNIFORM && kind != TPIV_WEIGHT_GAUSSIAN)
        return fail(TPIV_EINVAL, "tpiv_plan_set_weighting: kind must be TPIV_WEIGHT_NONE, TPIV_WEIGHT_UNIFORM or TPIV_WEIGHT_GAUSSIAN");
    if (kind == TPIV_WEIGHT_GAUSSIAN && (!(sigma_x >= 0.2 && sigma_x <= 4.0) || !(sigma_y >= 0.2 && sigma_y <= 4.0)))
        return fail(TPIV_EINVAL, "tpiv_plan_set_weighting: sigma must be in 0.2..4 (relative to the half window)");
    if (int rc = refuse_combination(plan, F_WEIGHTING)) return rc;
    size_t need = 0;
    for (const PassGeo& g : plan->geo) {
        if (!tpiv::win_size(g.ws))
            return fail(TPIV_EUNSUPPORTED, "weighting=: weighted passes cover window sizes 16, 32 and 64; this plan has a pass of " +
                                               std::to_string(g.ws));
        need += 2 * (size_t)g.ws;
    }
    if (!tables || n_tables != need)
        return fail(TPIV_EINVAL, "tpiv_plan_set_weighting: tables must hold g_y and g_x of every pass, " + std::to_string(need) +
                                     " floats in all");
    for (size_t i = 0; i < need; ++i)
        if (!(tables[i] > 0.0f && tables[i] <= 1.0f))       // (also refuses NaN)
            return fail(TPIV_EINVAL, "tpiv_plan_set_weighting: every table entry must be finite and in (0, 1]");
    if (kind == TPIV_WEIGHT_UNIFORM)
        for (size_t i = 0; i < need; ++i)
            if (tables[i] != 1.0f) return fail(TPIV_EINVAL, "tpiv_plan_set_weighting: the uniform weight's tables are all ones");
    if (int rc = install_pass_tables(plan, plan->wt_tab, tables, [](int ws) { return 2 * (size_t)ws; })) return rc;
    plan->wt_kind = kind;
    return TPIV_OK;
}

// ---- ensemble correlation -------------------------------------------------------------------------------------------

static int check_ensemble(const char* who, int mode, int H, int W, int ws, int ov, int val_win) {
    if (mode != 0 && mode != TPIV_MODE_DWS && mode != TPIV_MODE_CWS)
        return fail(TPIV_EKEY, std::string(who) + ": mode must be 0 (pass 1), TPIV_MODE_DWS or TPIV_MODE_CWS");
    if (int rc = check_window(H, W, ws, ov, val_win)) return rc;
    if (!tpiv::ensemble_size(ws))
        return fail(TPIV_EUNSUPPORTED, std::string(who) + ": ensemble correlation covers window sizes 16, 32 and 64 (got " +
                                           std::to_string(ws) + ")");
    return TPIV_OK;
}

size_t tpiv_ensemble_bytes(int H, int W, int ws, int ov) {
    if (ov >= ws || ws > H || ws > W || ws <= 0 || ov < 0 || !tpiv::ensemble_size(ws)) return 0;
    int nr, nc;
    field_shape(H, W, ws, ov, &nr, &nc);
    return (size_t)nr * nc * ws * ws * sizeof(float);
}

static int ensemble_add_impl(int mode, const uint8_t* a, const uint8_t* b, int batch, int H, int W, int ws, int ov,
                             const double* u0, const double* v0, const double* u2, const double* v2, const uint8_t* pmask,
                             float* acc, void* work, size_t work_bytes, void* stream) {
    if (int rc = check_ensemble("tpiv_ensemble_add", mode, H, W, ws, ov, 0)) return rc;
    if (batch < 0) return fail(TPIV_EINVAL, "tpiv_ensemble_add: negative batch");
    if (!acc || ((uintptr_t)acc & 15)) return fail(TPIV_EINVAL, "tpiv_ensemble_add: acc missing or not 16-byte aligned");
    if (batch == 0) return TPIV_OK;
    if (!a || !b) return fail(TPIV_EINVAL, "tpiv_ensemble_add: frames missing");
    if (mode != 0 && !pmask && (!u2 || !v2)) return fail(TPIV_EINVAL, "tpiv_ensemble_add: a shifted pass needs u2 / v2");
    tpiv::PassParams p = pass_params(a, b, batch, H, W, ws, ov, 1.2, 3, TPIV_PREC_FAST, nullptr, nullptr, nullptr, nullptr, nullptr);
    p.u0 = u0;
    p.v0 = v0;
    p.u2 = u2;
    p.v2 = v2;
    p.pmask = pmask;
    if (int rc = check_work(work, work_bytes, tpiv::ensemble_work_bytes(p.n_rows * p.n_cols))) return rc;
    p.peak_raw = static_cast<float*>(work);
    int n_cu;
    if (int rc = n_cu_of_current_device(&n_cu)) return rc;
    HIP_TRY(tpiv::launch_ensemble_add(p, mode, acc, n_cu, (hipStream_t)stream));
    return TPIV_OK;
}

static int ensemble_peaks_impl(int mode, const float* acc, long long n_pairs, int H, int W, int ws, int ov, const double* u0,
                               const double* v0, const double* u2, const double* v2, const uint8_t* pmask, double val_ratio,
                               int val_win, double* u, double* v, uint8_t* invalid, double* du, double* dv, void* work,
                               size_t work_bytes, void* stream) {
    if (int rc = check_ensemble("tpiv_ensemble_peaks", mode, H, W, ws, ov, val_win)) return rc;
    if (n_pairs < 1 || n_pairs > (1LL << 24))
        return fail(TPIV_EINVAL, "tpiv_ensemble_peaks: n_pairs must be in 1..2^24 (no pairs were added?)");
    if (!acc || ((uintptr_t)acc & 15)) return fail(TPIV_EINVAL, "tpiv_ensemble_peaks: acc missing or not 16-byte aligned");
    if (!u || !v || !invalid) return fail(TPIV_EINVAL, "tpiv_ensemble_peaks: output missing");
    if (mode != 0 && (!u0 || !v0 || (!pmask && (!u2 || !v2))))
        return fail(TPIV_EINVAL, "tpiv_ensemble_peaks: a shifted pass needs u0, v0, u2, v2");
    tpiv::PassParams p = pass_params(nullptr, nullptr, 1, H, W, ws, ov, val_ratio, val_win, TPIV_PREC_FAST, u, v, invalid, nullptr,
                                     nullptr);
    p.u0 = u0;
    p.v0 = v0;
    p.u2 = u2;
    p.v2 = v2;
    p.pmask = pmask;
    p.du = mode != 0 ? du : nullptr;
    p.dv = mode != 0 ? dv : nullptr;
    if (p.du && !p.dv) return fail(TPIV_EINVAL, "tpiv_ensemble_peaks: du without dv");
    if (int rc = check_work(work, work_bytes, tpiv::ensemble_work_bytes(p.n_rows * p.n_cols))) return rc;
    p.peak_raw = static_cast<float*>(work);
    int n_cu;
    if (int rc = n_cu_of_current_device(&n_cu)) return rc;
    HIP_TRY(tpiv::launch_ensemble_peaks(p, mode, acc, n_pairs, n_cu, (hipStream_t)stream));
    return TPIV_OK;
}

int tpiv_ensemble_add(int mode, const uint8_t* a, const uint8_t* b, int batch, int H, int W, int ws, int ov, const double* u2,
                      const double* v2, float* acc, void* work, size_t work_bytes, void* stream) {
    // the documented size (a plan hands its own buffer to the _impl, sized by ensemble_work_bytes)
    if (batch > 0)
        if (int rc = check_work(work, work_bytes, tpiv_work_bytes(H, W, ws, ov, 1))) return rc;
    return ensemble_add_impl(mode, a, b, batch, H, W, ws, ov, nullptr, nullptr, u2, v2, nullptr, acc, work, work_bytes, stream);
}

int tpiv_ensemble_peaks(int mode, const float* acc, long long n_pairs, int H, int W, int ws, int ov, const double* u0,
                        const double* v0, const double* u2, const double* v2, double val_ratio, int val_win, double* u, double* v,
                        uint8_t* invalid, double* du, double* dv, void* work, size_t work_bytes, void* stream) {
    if (int rc = check_work(work, work_bytes, tpiv_work_bytes(H, W, ws, ov, 1))) return rc;      // the documented size
    return ensemble_peaks_impl(mode, acc, n_pairs, H, W, ws, ov, u0, v0, u2, v2, nullptr, val_ratio, val_win, u, v, invalid, du,
                               dv, work, work_bytes, stream);
}

int tpiv_plan_set_ensemble(tpiv_plan* plan, int on) {
    if (!plan) return fail(TPIV_EINVAL, "null plan");
    if (!on) {                       // (the workspace stays: a plan frees at its destruction)
        plan->ens_on = false;
        plan->ens_pass = plan->ens_done = -1;
        return TPIV_OK;
    }
    if (int rc = refuse_combination(plan, F_ENSEMBLE)) return rc;
    size_t cells = 0, fine = 0;
    for (const PassGeo& g : plan->geo) {
        if (!tpiv::ensemble_size(g.ws))
            return fail(TPIV_EUNSUPPORTED, "ensemble correlation covers window sizes 16, 32 and 64; this plan has a pass of " +
                                               std::to_string(g.ws));
        const size_t N = (size_t)g.n_rows * g.n_cols;
        cells = std::max(cells, N * g.ws * g.ws);
        fine = std::max(fine, N);
    }
    if (int rc = check_plan_device(plan)) return rc;
    if (!plan->ens_acc) {
        if (tpiv::ensemble_work_bytes((int)fine) > plan->peak_raw_bytes)
            return fail(TPIV_EINVAL, "plan workspace smaller than the ensemble launches need");     // (never: same records)
        int rc = plan->alloc(&plan->ens_acc, cells);
        plan->ens_u.assign(plan->n_pass, nullptr);
        plan->ens_v.assign(plan->n_pass, nullptr);
        plan->ens_val.assign(plan->n_pass, nullptr);
        for (int p = 0; p < plan->n_pass && !rc; ++p) {
            const size_t N = (size_t)plan->geo[p].n_rows * plan->geo[p].n_cols;
            rc = plan->alloc(&plan->ens_u[p], N);
            if (!rc) rc = plan->alloc(&plan->ens_v[p], N);
            if (!rc) rc = plan->alloc(&plan->ens_val[p], N);
        }
        if (!rc && plan->n_pass > 1) {
            rc = plan->alloc(&plan->ens_u0, fine);
            if (!rc) rc = plan->alloc(&plan->ens_v0, fine);
            if (!rc) rc = plan->alloc(&plan->ens_pmask, fine);
        }
        if (rc) {
            plan->ens_acc = nullptr;       // (what was allocated stays in allocs and is freed with the plan)
            return rc;
        }
    }
    plan->ens_on = true;
    plan->ens_pass = plan->ens_done = -1;
    plan->ens_pairs = 0;
    return TPIV_OK;
}

int tpiv_plan_ensemble_begin(tpiv_plan* plan, int pass, void* stream) {
    if (!plan) return fail(TPIV_EINVAL, "null plan");
    if (!plan->ens_on) return fail(TPIV_EINVAL, "ensemble correlation is off (tpiv_plan_set_ensemble)");
    if (pass < 0 || pass >= plan->n_pass) return fail(TPIV_EINVAL, "bad pass index");
    if (pass > 0 && plan->ens_done < pass - 1)
        return fail(TPIV_EINVAL, "ensemble pass " + std::to_string(pass) + " begins before pass " + std::to_string(pass - 1) +
                                     " was ended");
    if (int rc = check_plan_device(plan)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const PassGeo& g = plan->geo[pass];
    HIP_TRY(hipMemsetAsync(plan->ens_acc, 0, (size_t)g.n_rows * g.n_cols * g.ws * g.ws * sizeof(float), st));
    if (pass > 0) {
        if (int rc = run_banded_predict(plan, pass, 1, plan->ens_u[pass - 1], plan->ens_v[pass - 1], plan->ens_val[pass - 1],
                                        plan->ens_u0, plan->ens_v0, nullptr, nullptr, st, plan->ens_pmask))
            return rc;
    }
    plan->ens_pass = pass;
    plan->ens_pairs = 0;
    return TPIV_OK;
}

int tpiv_plan_ensemble_add(tpiv_plan* plan, const uint8_t* a, const uint8_t* b, int batch, void* stream) {
    if (!plan) return fail(TPIV_EINVAL, "null plan");
    if (!plan->ens_on || plan->ens_pass < 0) return fail(TPIV_EINVAL, "tpiv_plan_ensemble_add before tpiv_plan_ensemble_begin");
    if (batch < 0 || batch > plan->max_batch) return fail(TPIV_EINVAL, "batch exceeds the plan's max_batch");
    if (batch == 0) return TPIV_OK;
    if (plan->ens_pairs + batch > (1LL << 24)) return fail(TPIV_EINVAL, "more than 2^24 pairs in one ensemble");
    if (int rc = check_plan_device(plan)) return rc;
    const int p = plan->ens_pass;
    const PassGeo& g = plan->geo[p];
    if (int rc = ensemble_add_impl(p == 0 ? 0 : plan->mode, a, b, batch, plan->H, plan->W, g.ws, g.ov, plan->ens_u0, plan->ens_v0,
                                   nullptr, nullptr, p == 0 ? nullptr : plan->ens_pmask, plan->ens_acc, plan->peak_raw,
                                   plan->peak_raw_bytes, stream))
        return rc;
    plan->ens_pairs += batch;
    return TPIV_OK;
}

int tpiv_plan_ensemble_end(tpiv_plan* plan, double* u, double* v, uint8_t* invalid, void* stream) {
    if (!plan) return fail(TPIV_EINVAL, "null plan");
    if (!plan->ens_on || plan->ens_pass < 0) return fail(TPIV_EINVAL, "tpiv_plan_ensemble_end before tpiv_plan_ensemble_begin");
    if (plan->ens_pairs < 1) return fail(TPIV_EINVAL, "tpiv_plan_ensemble_end: no pairs were added");
    if (!u || !v || !invalid) return fail(TPIV_EINVAL, "tpiv_plan_ensemble_end: output missing");
    if (int rc = check_plan_device(plan)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int p = plan->ens_pass, last = plan->n_pass - 1;
    const PassGeo& g = plan->geo[p];
    const size_t N = (size_t)g.n_rows * g.n_cols;
    // as in tpiv_plan_run, on a batch of one: a pass before the last keeps its field in the plan for the next begin
    const Settle settle(plan, p, p < last, p < last, p == last ? u : plan->ens_u[p], p == last ? v : plan->ens_v[p],
                        p == last ? invalid : plan->ens_val[p], plan->raw_u, plan->raw_v);
    if (int rc = ensemble_peaks_impl(p == 0 ? 0 : plan->mode, plan->ens_acc, plan->ens_pairs, plan->H, plan->W, g.ws, g.ov,
                                     plan->ens_u0, plan->ens_v0, nullptr, nullptr, p == 0 ? nullptr : plan->ens_pmask,
                                     plan->val_ratio, plan->val_win, settle.wu, settle.wv, settle.wval, nullptr, nullptr,
                                     plan->peak_raw, plan->peak_raw_bytes, stream))
        return rc;
    if (int rc = settle.run(1, st)) return rc;
    if (p < last) {
        HIP_TRY(hipMemcpyAsync(u, plan->ens_u[p], N * sizeof(double), hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(v, plan->ens_v[p], N * sizeof(double), hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(invalid, plan->ens_val[p], N, hipMemcpyDeviceToDevice, st));
    }
    plan->ens_done = p;
    plan->ens_pass = -1;
    return TPIV_OK;
}

int tpiv_plan_ensemble_maps(tpiv_plan* plan, float** acc, long long* n_pairs) {
    if (!plan || !plan->ens_on) return fail(TPIV_EINVAL, "ensemble correlation is off (tpiv_plan_set_ensemble)");
    if (acc) *acc = plan->ens_acc;
    if (n_pairs) *n_pairs = plan->ens_pairs;
    return TPIV_OK;
}

int tpiv_postval(double* u, double* v, const uint8_t* invalid, int batch, int n_rows, int n_cols, uint8_t* cls,
                 int32_t* counts, void* stream) {
    if (batch < 0 || n_rows < 1 || n_cols < 1) return fail(TPIV_EINVAL, "tpiv_postval: empty grid");
    if ((long long)n_rows * n_cols >= (1LL << 31)) return fail(TPIV_EUNSUPPORTED, "field too large");
    if (batch == 0) return TPIV_OK;
    if (!u || !v || !invalid || !cls || !counts) return fail(TPIV_EINVAL, "tpiv_postval: null pointer");
    tpiv::PostvalParams q{};
    q.u = u;
    q.v = v;
    q.invalid = invalid;
    q.cls = cls;
    q.counts = counts;
    q.batch = batch;
    q.n_rows = n_rows;
    q.n_cols = n_cols;
    HIP_TRY(tpiv::launch_postval(q, (hipStream_t)stream));
    return TPIV_OK;
}

int tpiv_postval_compact(const double* u, const double* v, const uint8_t* cls, const int32_t* counts, int batch, int n_rows,
                         int n_cols, int32_t* offsets, int32_t* ring_rc, double* ring_uv, int32_t* hole_rc, void* stream) {
    if (batch < 0 || n_rows < 1 || n_cols < 1) return fail(TPIV_EINVAL, "tpiv_postval_compact: empty grid");
    if ((long long)batch * n_rows * n_cols >= (1LL << 30)) return fail(TPIV_EUNSUPPORTED, "batch of fields too large");
    if (batch == 0) return TPIV_OK;
    if (!u || !v || !cls || !counts || !offsets || !ring_rc || !ring_uv || !hole_rc)
        return fail(TPIV_EINVAL, "tpiv_postval_compact: null pointer");
    HIP_TRY(tpiv::launch_postval_compact(u, v, cls, counts, batch, n_rows, n_cols, offsets, ring_rc, ring_uv, hole_rc,
                                         (hipStream_t)stream));
    return TPIV_OK;
}

int tpiv_finish_fields(const double* u, const double* v, int batch, int n_rows, int n_cols, double scale, double dt,
                       double* fu, double* fv, void* stream) {
    if (batch < 0 || n_rows < 1 || n_cols < 1) return fail(TPIV_EINVAL, "tpiv_finish_fields: empty grid");
    if (batch == 0) return TPIV_OK;
    if (!u || !v || !fu || !fv) return fail(TPIV_EINVAL, "tpiv_finish_fields: null pointer");
    HIP_TRY(tpiv::launch_finish_fields(u, v, batch, n_rows, n_cols, scale, dt, fu, fv, (hipStream_t)stream));
    return TPIV_OK;
}

int tpiv_ensemble_moments(const double* u, const double* v, int n, long long cells, double* out, void* stream) {
    if (n <= 0 || cells <= 0) return fail(TPIV_EINVAL, "tpiv_ensemble_moments: needs at least one field");
    if (!u || !v || !out) return fail(TPIV_EINVAL, "tpiv_ensemble_moments: null pointer");
    HIP_TRY(tpiv::launch_ensemble_moments(u, v, n, cells, out, (hipStream_t)stream));
    return TPIV_OK;
}

int tpiv_bmp_unpack(const uint8_t* raw, const int64_t* desc, const uint8_t* lut, int n_files, int H, int W,
                    uint8_t* out, void* stream) {
    if (n_files < 0 || H <= 0 || W <= 0) return fail(TPIV_EINVAL, "tpiv_bmp_unpack: bad shape");
    if (n_files == 0) return TPIV_OK;
    if (!raw || !desc || !lut || !out) return fail(TPIV_EINVAL, "tpiv_bmp_unpack: null pointer");
    HIP_TRY(tpiv::launch_bmp_unpack(raw, reinterpret_cast<const long long*>(desc), lut, n_files, H, W, out,
                                    (hipStream_t)stream));
    return TPIV_OK;
}

int tpiv_bmp_unpack_bg(const uint8_t* raw, const int64_t* desc, const uint8_t* lut, int n_files, int H, int W,
                       const uint8_t* bg, uint8_t* out, void* stream) {
    if (n_files < 0 || H <= 0 || W <= 0) return fail(TPIV_EINVAL, "tpiv_bmp_unpack_bg: bad shape");
    if (n_files == 0) return TPIV_OK;
    if (!raw || !desc || !lut || !bg || !out) return fail(TPIV_EINVAL, "tpiv_bmp_unpack_bg: null pointer");
    HIP_TRY(tpiv::launch_bmp_unpack_bg(raw, reinterpret_cast<const long long*>(desc), lut, n_files, H, W, bg, out,
                                       (hipStream_t)stream));
    return TPIV_OK;
}

int tpiv_frame_min(const uint8_t* frames, int n, long long pixels, uint8_t* acc, void* stream) {
    if (n < 0 || pixels <= 0) return fail(TPIV_EINVAL, "tpiv_frame_min: bad shape");
    if (n == 0) return TPIV_OK;
    if (!frames || !acc) return fail(TPIV_EINVAL, "tpiv_frame_min: null pointer");
    HIP_TRY(tpiv::launch_frame_min(frames, n, pixels, acc, (hipStream_t)stream));
    return TPIV_OK;
}

// single-pixel ensemble correlation: the geometry every entry refuses alike (bins, radius, shift)
static bool pixel_corr_geometry(int H, int W, int bin_y, int bin_x, int radius, int shift_y, int shift_x) {
    return H >= 1 && W >= 1 && bin_y >= 1 && bin_x >= 1 && (long long)bin_y * bin_x <= tpiv::kPixelCorrMaxBin && bin_y <= H &&
           bin_x <= W && radius >= tpiv::kPixelCorrMinRadius && radius <= tpiv::kPixelCorrMaxRadius &&
           std::abs(shift_y) <= tpiv::kPixelCorrMaxShift && std::abs(shift_x) <= tpiv::kPixelCorrMaxShift &&
           (long long)H * W <= 0x7fffffffLL;
}

size_t tpiv_pixel_corr_bytes(int H, int W, int bin_y, int bin_x, int radius) {
    if (!pixel_corr_geometry(H, W, bin_y, bin_x, radius, 0, 0)) return 0;
    const size_t D = 2 * (size_t)radius + 1;
    return (size_t)(H / bin_y) * (size_t)(W / bin_x) * D * D * sizeof(int64_t);
}

int tpiv_pixel_corr_add(const uint8_t* a, const uint8_t* b, int batch, int H, int W, int bin_y, int bin_x, int radius,
                        int shift_y, int shift_x, int64_t* acc, int64_t* mom, void* stream) {
    if (!pixel_corr_geometry(H, W, bin_y, bin_x, radius, shift_y, shift_x))
        return fail(TPIV_EINVAL, "tpiv_pixel_corr_add: bin_y, bin_x >= 1 with bin_y * bin_x <= 256 inside the frame, radius in "
                                 "3..16, |shift| <= 64");
    if (batch < 0 || batch > tpiv::kPixelCorrMaxBatch)
        return fail(TPIV_EINVAL, "tpiv_pixel_corr_add: batch must be in 0..256 (the 32-bit partial sums of one call)");
    if (!acc || !mom || ((uintptr_t)acc & 7u) || ((uintptr_t)mom & 7u))
        return fail(TPIV_EINVAL, "tpiv_pixel_corr_add: acc and mom must be 8-byte aligned device pointers");
    if (batch == 0) return TPIV_OK;
    if (!a || !b) return fail(TPIV_EINVAL, "tpiv_pixel_corr_add: null pointer");
    HIP_TRY(tpiv::launch_pixel_corr_add(a, b, batch, H, W, bin_y, bin_x, radius, shift_y, shift_x,
                                        reinterpret_cast<long long*>(acc), reinterpret_cast<long long*>(mom), (hipStream_t)stream));
    return TPIV_OK;
}

int tpiv_pixel_corr_peaks(const int64_t* acc, const int64_t* mom, int n_pairs, int H, int W, int bin_y, int bin_x, int radius,
                          int shift_y, int shift_x, double* u, double* v, double* peak, double* ratio, uint8_t* status,
                          double* corr, void* stream) {
    if (!pixel_corr_geometry(H, W, bin_y, bin_x, radius, shift_y, shift_x))
        return fail(TPIV_EINVAL, "tpiv_pixel_corr_peaks: bin_y, bin_x >= 1 with bin_y * bin_x <= 256 inside the frame, radius "
                                 "in 3..16, |shift| <= 64");
    if (n_pairs < 1 || n_pairs > tpiv::kPixelCorrMaxPairs)
        return fail(TPIV_EINVAL, "tpiv_pixel_corr_peaks: n_pairs must be in 1..65536");
    if (!acc || !mom || ((uintptr_t)acc & 7u) || ((uintptr_t)mom & 7u))
        return fail(TPIV_EINVAL, "tpiv_pixel_corr_peaks: acc and mom must be 8-byte aligned device pointers");
    if (!u || !v || !peak || !ratio || !status) return fail(TPIV_EINVAL, "tpiv_pixel_corr_peaks: null output pointer");
    if (((uintptr_t)u | (uintptr_t)v | (uintptr_t)peak | (uintptr_t)ratio | (uintptr_t)corr) & 7u)
        return fail(TPIV_EINVAL, "tpiv_pixel_corr_peaks: float64 outputs must be 8-byte aligned");
    HIP_TRY(tpiv::launch_pixel_corr_peaks(reinterpret_cast<const long long*>(acc), reinterpret_cast<const long long*>(mom),
                                          n_pairs, H, W, bin_y, bin_x, radius, shift_y, shift_x, u, v, peak, ratio, status, corr,
                                          (hipStream_t)stream));
    return TPIV_OK;
}

int tpiv_subtract_background(const uint8_t* frames, int n, long long pixels, const uint8_t* bg, uint8_t* out,
                             void* stream) {
    if (n < 0 || pixels <= 0) return fail(TPIV_EINVAL, "tpiv_subtract_background: bad shape");
    if (n == 0) return TPIV_OK;
    if (!frames || !bg || !out) return fail(TPIV_EINVAL, "tpiv_subtract_background: null pointer");
    if (out != frames && out < frames + (size_t)n * pixels && frames < out + (size_t)n * pixels)
        return fail(TPIV_EINVAL, "tpiv_subtract_background: out overlaps frames without being frames");
    HIP_TRY(tpiv::launch_subtract_background(frames, n, pixels, bg, out, (hipStream_t)stream));
    return TPIV_OK;
}

int tpiv_prefilter(const uint8_t* frames, int n, int H, int W, const uint8_t* bg, int kind, int size, int cap,
                   uint8_t* out, void* stream) {
    if (n < 0 || H <= 0 || W <= 0) return fail(TPIV_EINVAL, "tpiv_prefilter: bad shape");
    if (kind != TPIV_PREFILTER_NONE && kind != TPIV_PREFILTER_MIN && kind != TPIV_PREFILTER_MEAN)
        return fail(TPIV_EINVAL, "tpiv_prefilter: kind must be TPIV_PREFILTER_NONE, _MIN or _MEAN");
    if (kind != TPIV_PREFILTER_NONE && (size < 3 || size > 63 || size % 2 == 0))
        return fail(TPIV_EINVAL, "tpiv_prefilter: size must be odd and in 3..63");
    if (cap < 1 || cap > 255) return fail(TPIV_EINVAL, "tpiv_prefilter: cap must be in 1..255 (255: none)");
    if (n == 0) return TPIV_OK;
    if (!frames || !out) return fail(TPIV_EINVAL, "tpiv_prefilter: null pointer");
    const size_t bytes = (size_t)n * H * W;
    if (out < frames + bytes && frames < out + bytes)
        return fail(TPIV_EINVAL, "tpiv_prefilter: out overlaps frames (the filter is a stencil: not in place)");
    if (bg && out < bg + (size_t)H * W && bg < out + bytes)
        return fail(TPIV_EINVAL, "tpiv_prefilter: out overlaps the background");
    HIP_TRY(tpiv::launch_prefilter(frames, n, H, W, bg, kind, size, cap, out, (hipStream_t)stream));
    return TPIV_OK;
}

int tpiv_depth_map(const uint16_t* src, const long long* src_off, int n, int H, int W, const uint8_t* lut, uint8_t* out,
                   void* stream) {
    if (n < 0 || H <= 0 || W <= 0) return fail(TPIV_EINVAL, "tpiv_depth_map: bad shape");
    if (n == 0) return TPIV_OK;
    if (!src || !lut || !out) return fail(TPIV_EINVAL, "tpiv_depth_map: null pointer");
    if ((uintptr_t)src % 2 != 0) return fail(TPIV_EINVAL, "tpiv_depth_map: src must be 2-byte aligned");
    const size_t px = (size_t)n * H * W;
    const uint8_t* s8 = reinterpret_cast<const uint8_t*>(src);
    if (!src_off && out < s8 + 2 * px && s8 < out + px) return fail(TPIV_EINVAL, "tpiv_depth_map: out overlaps src");
    if (out < lut + 65536 && lut < out + px) return fail(TPIV_EINVAL, "tpiv_depth_map: out overlaps the table");
    int n_cu = 0;
    if (int rc = n_cu_of_current_device(&n_cu)) return rc;
    HIP_TRY(tpiv::launch_depth_map(src, src_off, n, H, W, lut, out, n_cu, (hipStream_t)stream));
    return TPIV_OK;
}

int tpiv_dewarp(const uint8_t* frames, const long long* src_off, int n, int H, int W, const int32_t* map, const int16_t* table,
                int interp, int fill, uint8_t* out, void* stream) {
    if (n < 0 || H <= 0 || W <= 0 || H > (1 << 22) || W > (1 << 22) || (long long)H * W >= (1LL << 31))
        return fail(TPIV_EINVAL, "tpiv_dewarp: bad shape");
    if (interp != TPIV_DEWARP_LINEAR && interp != TPIV_DEWARP_CUBIC)
        return fail(TPIV_EINVAL, "tpiv_dewarp: interp must be TPIV_DEWARP_LINEAR or TPIV_DEWARP_CUBIC");
    if (fill < 0 || fill > 255) return fail(TPIV_EINVAL, "tpiv_dewarp: fill must be in 0..255");
    if (n == 0) return TPIV_OK;
    if (!frames || !map || !out || (interp == TPIV_DEWARP_CUBIC && !table)) return fail(TPIV_EINVAL, "tpiv_dewarp: null pointer");
    if ((uintptr_t)map % 4 != 0 || (uintptr_t)table % 2 != 0)
        return fail(TPIV_EINVAL, "tpiv_dewarp: the map must be 4-byte and the table 2-byte aligned");
    const size_t px = (size_t)n * H * W;
    const uint8_t* m8 = reinterpret_cast<const uint8_t*>(map);
    const uint8_t* t8 = reinterpret_cast<const uint8_t*>(table);
    if (!src_off && out < frames + px && frames < out + px)
        return fail(TPIV_EINVAL, "tpiv_dewarp: out overlaps frames (a gather: not in place)");
    if (out < m8 + (size_t)H * W * 8 && m8 < out + px) return fail(TPIV_EINVAL, "tpiv_dewarp: out overlaps the map");
    if (t8 && out < t8 + 2048 && t8 < out + px) return fail(TPIV_EINVAL, "tpiv_dewarp: out overlaps the table");
    HIP_TRY(tpiv::launch_dewarp(frames, src_off, n, H, W, map, table, interp, fill, out, (hipStream_t)stream));
    return TPIV_OK;
}

size_t tpiv_equalize_work_bytes(int n, int H, int W, int tile) {
    if (n <= 0 || H <= 0 || W <= 0 || H > (1 << 28) || W > (1 << 28) || tile < tpiv::EQUALIZE_TILE_MIN ||
        tile > tpiv::EQUALIZE_TILE_MAX)
        return 0;
    return (size_t)n * tpiv::equalize_tiles(H, tile) * tpiv::equalize_tiles(W, tile) * 256;
}

int tpiv_equalize(const uint8_t* frames, int n, int H, int W, int tile, int clip_q8, uint8_t* out, void* work,
                  size_t work_bytes, void* stream) {
    if (n < 0 || H <= 0 || W <= 0 || H > (1 << 28) || W > (1 << 28)) return fail(TPIV_EINVAL, "tpiv_equalize: bad shape");
    if (tile < tpiv::EQUALIZE_TILE_MIN || tile > tpiv::EQUALIZE_TILE_MAX)
        return fail(TPIV_EINVAL, "tpiv_equalize: tile must be in 8..256");
    if (clip_q8 < tpiv::EQUALIZE_CLIP_Q8_MIN || clip_q8 > tpiv::EQUALIZE_CLIP_Q8_MAX)
        return fail(TPIV_EINVAL, "tpiv_equalize: clip_q8 must be in 256..65536");
    if (n == 0) return TPIV_OK;
    if (!frames || !out || !work) return fail(TPIV_EINVAL, "tpiv_equalize: null pointer");
    const size_t need = tpiv_equalize_work_bytes(n, H, W, tile);
    if (work_bytes < need) return fail(TPIV_EINVAL, "tpiv_equalize: workspace too small (tpiv_equalize_work_bytes)");
    if (tpiv::equalize_tiles(H, tile) > 65535) return fail(TPIV_EINVAL, "tpiv_equalize: more than 65535 tile rows");
    const size_t bytes = (size_t)n * H * W;
    if (out != frames && out < frames + bytes && frames < out + bytes)
        return fail(TPIV_EINVAL, "tpiv_equalize: out overlaps frames in part (in place means out == frames)");
    const uint8_t* w8 = static_cast<const uint8_t*>(work);
    if ((w8 < frames + bytes && frames < w8 + need) || (w8 < out + bytes && out < w8 + need))
        return fail(TPIV_EINVAL, "tpiv_equalize: the workspace overlaps the frames or out");
    HIP_TRY(tpiv::launch_equalize(frames, n, H, W, tile, clip_q8, out, static_cast<uint8_t*>(work), (hipStream_t)stream));
    return TPIV_OK;
}

int tpiv_depth_histogram(const uint16_t* src, int n, long long pixels_per_frame, unsigned long long* hist, void* stream) {
    if (n < 0 || pixels_per_frame <= 0) return fail(TPIV_EINVAL, "tpiv_depth_histogram: bad shape");
    if (n == 0) return TPIV_OK;
    if (!src || !hist) return fail(TPIV_EINVAL, "tpiv_depth_histogram: null pointer");
    if ((uintptr_t)src % 2 != 0 || (uintptr_t)hist % 8 != 0)
        return fail(TPIV_EINVAL, "tpiv_depth_histogram: src must be 2-byte aligned, hist 8-byte aligned");
    if (pixels_per_frame > (1LL << 62) / n) return fail(TPIV_EINVAL, "tpiv_depth_histogram: bad shape");
    int n_cu = 0;
    if (int rc = n_cu_of_current_device(&n_cu)) return rc;
    HIP_TRY(tpiv::launch_depth_histogram(src, (long long)n * pixels_per_frame, hist, n_cu, (hipStream_t)stream));
    return TPIV_OK;
}

namespace {
// One file into a slot of at most slot_bytes: bytes read, or -1 (cannot open / not a regular file / too big / short read).
int64_t read_one_file(const char* path, uint8_t* out, size_t slot_bytes) {
    const int fd = path ? ::open(path, O_RDONLY | O_CLOEXEC) : -1;
    if (fd < 0) return -1;
    int64_t res = -1;
    struct stat st;
    if (::fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && (size_t)st.st_size <= slot_bytes) {
        size_t got = 0;
        const size_t want = (size_t)st.st_size;
        while (got < want) {
            const ssize_t r = ::read(fd, out + got, want - got);
            if (r <= 0) break;
            got += (size_t)r;
        }
        if (got == want) res = (int64_t)want;
    }
    ::close(fd);
    return res;
}
}  // namespace

// Read-ahead ring of the file path: the whole run's file list is handed over once, reader threads fill the caller's
// staging buffers batch by batch (in order, up to n_bufs batches ahead of the consumer) and the consumer blocks in
// tpiv_reader_next without holding any interpreter lock.
struct tpiv_reader {
    std::vector<std::string> paths;
    std::vector<uint8_t*> bufs;
    std::vector<int64_t> sizes;          // per file
    std::vector<int> done;               // per batch: files finished
    size_t slot_bytes = 0;
    long files_per_batch = 0, n_batches = 0;
    std::atomic<long> next_file{0};
    long released = 0;                   // batches handed back by the consumer (in order)
    long cursor = 0;                     // next batch tpiv_reader_next hands out
    bool stop = false;
    std::mutex m;
    std::condition_variable cv;
    std::vector<std::thread> pool;

    long files_in(long b) const {
        const long n = (long)paths.size();
        return std::min(files_per_batch, n - b * files_per_batch);
    }
    void work() {
        const long n = (long)paths.size();
        for (;;) {
            const long i = next_file.fetch_add(1);
            if (i >= n) return;
            const long b = i / files_per_batch;
            {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return stop || b < released + (long)bufs.size(); });
                if (stop) return;
            }
            uint8_t* out = bufs[b % (long)bufs.size()] + (size_t)(i - b * files_per_batch) * slot_bytes;
            const int64_t got = read_one_file(paths[i].c_str(), out, slot_bytes);
            std::lock_guard<std::mutex> lk(m);
            sizes[i] = got;
            if (++done[b] == files_in(b)) cv.notify_all();
        }
    }
};

tpiv_reader* tpiv_reader_open(const char* const* paths, int64_t n_files, int files_per_batch, uint8_t* const* bufs,
                              int n_bufs, size_t slot_bytes, int n_threads) {
    if (n_files < 0 || files_per_batch < 1 || n_bufs < 1 || slot_bytes == 0 || !bufs || (n_files > 0 && !paths)) {
        fail(TPIV_EINVAL, "tpiv_reader_open: bad arguments");
        return nullptr;
    }
    auto* r = new tpiv_reader;
    for (int64_t i = 0; i < n_files; ++i) r->paths.emplace_back(paths[i] ? paths[i] : "");
    for (int k = 0; k < n_bufs; ++k) {
        if (!bufs[k]) {
            delete r;
            fail(TPIV_EINVAL, "tpiv_reader_open: null staging buffer");
            return nullptr;
        }
        r->bufs.push_back(bufs[k]);
    }
    r->slot_bytes = slot_bytes;
    r->files_per_batch = files_per_batch;
    r->n_batches = (long)((n_files + files_per_batch - 1) / files_per_batch);
    r->sizes.assign((size_t)n_files, -1);
    r->done.assign((size_t)r->n_batches, 0);
    if (n_threads < 1) n_threads = 1;
    for (int t = 0; t < n_threads; ++t) r->pool.emplace_back([r] { r->work(); });
    return r;
}

int tpiv_reader_next(tpiv_reader* r, int* n_files, int* buf_index, int64_t* sizes) {
    if (!r || !n_files || !buf_index || !sizes) return fail(TPIV_EINVAL, "tpiv_reader_next: null argument");
    std::unique_lock<std::mutex> lk(r->m);
    *n_files = 0;
    if (r->cursor >= r->n_batches) return TPIV_OK;
    const long b = r->cursor;
    const long cnt = r->files_in(b);
    if (b >= r->released + (long)r->bufs.size())
        return fail(TPIV_EINVAL, "tpiv_reader_next: every staging buffer is held (release one first)");
    r->cv.wait(lk, [&] { return r->done[b] == cnt; });
    for (long k = 0; k < cnt; ++k) sizes[k] = r->sizes[(size_t)(b * r->files_per_batch + k)];
    *buf_index = (int)(b % (long)r->bufs.size());
    *n_files = (int)cnt;
    r->cursor = b + 1;
    return TPIV_OK;
}

int tpiv_reader_release(tpiv_reader* r) {
    if (!r) return fail(TPIV_EINVAL, "tpiv_reader_release: null reader");
    {
        std::lock_guard<std::mutex> lk(r->m);
        if (r->released >= r->cursor) return fail(TPIV_EINVAL, "tpiv_reader_release: nothing handed out");
        ++r->released;
    }
    r->cv.notify_all();
    return TPIV_OK;
}

void tpiv_reader_close(tpiv_reader* r) {
    if (!r) return;
    {
        std::lock_guard<std::mutex> lk(r->m);
        r->stop = true;
    }
    r->cv.notify_all();
    for (auto& t : r->pool) t.join();
    delete r;
}

int tpiv_read_files(const char* const* paths, int n_files, uint8_t* dst, size_t slot_bytes, int n_threads,
                    int64_t* sizes) {
    if (n_files < 0 || (n_files > 0 && (!paths || !dst || !sizes)) || slot_bytes == 0)
        return fail(TPIV_EINVAL, "tpiv_read_files: bad arguments");
    if (n_files == 0) return TPIV_OK;
    if (n_threads < 1) n_threads = 1;
    if (n_threads > n_files) n_threads = n_files;
    std::atomic<int> next{0};
    auto worker = [&]() {
        for (;;) {
            const int i = next.fetch_add(1);
            if (i >= n_files) return;
            sizes[i] = read_one_file(paths[i], dst + (size_t)i * slot_bytes, slot_bytes);
        }
    };
    std::vector<std::thread> pool;
    for (int t = 1; t < n_threads; ++t) pool.emplace_back(worker);
    worker();
    for (auto& t : pool) t.join();
    return TPIV_OK;
}

#ifdef TPIV_STAMPS
// Diagnostic builds only (make stamps): device buffer of 32 uint64 that the tile kernels add their
// per-phase s_memtime deltas to.  The production library has neither this setter nor any other state.
int tpiv_debug_set_stamps(void* dev_buffer) {
    g_stamps = static_cast<unsigned long long*>(dev_buffer);
    return TPIV_OK;
}
#endif

int tpiv_plan_set_timing(tpiv_plan* plan, int enable) {
    if (!plan) return fail(TPIV_EINVAL, "null plan");
    plan->timing = enable != 0;
    plan->runs_recorded = 0;
    return TPIV_OK;
}

int tpiv_plan_get_timing(tpiv_plan* plan, double* avg_ms, int n_slots, int* n_runs) {
    if (!plan || !avg_ms || n_slots != plan->n_slots()) return fail(TPIV_EINVAL, "bad timing query");
    for (int s = 0; s < n_slots; ++s) avg_ms[s] = 0.0;
    const size_t n = plan->runs_recorded;
    for (size_t r = 0; r < n; ++r) {
        for (int s = 0; s < n_slots; ++s) {
            float ms = 0.f;
            HIP_TRY(hipEventSynchronize(plan->events[r][2 * s + 1]));
            HIP_TRY(hipEventElapsedTime(&ms, plan->events[r][2 * s], plan->events[r][2 * s + 1]));
            avg_ms[s] += ms;
        }
    }
    if (n)
        for (int s = 0; s < n_slots; ++s) avg_ms[s] /= (double)n;
    for (double& m : plan->exact_ms) m = 0.0;
    size_t n_sub = 0;                    // runs whose first pass was the exact scheme (a filtered run records no sub-events)
    for (size_t r = 0; r < n; ++r) n_sub += r < plan->sub_recorded.size() && plan->sub_recorded[r];
    if (plan->exact_count && n_sub) {
        for (size_t r = 0; r < n; ++r) {
            if (!plan->sub_recorded[r]) continue;
            const hipEvent_t* sub = plan->events[r].data() + 2 * n_slots;
            const hipEvent_t chain[5] = {plan->events[r][0], sub[0], sub[1], sub[2], plan->events[r][1]};
            for (int s = 0; s < 4; ++s) {
                float ms = 0.f;
                HIP_TRY(hipEventElapsedTime(&ms, chain[s], chain[s + 1]));
                plan->exact_ms[s] += ms / (double)n_sub;
            }
        }
    }
    if (n_runs) *n_runs = (int)n;
    plan->runs_recorded = 0;
    return TPIV_OK;
}

int tpiv_plan_exact_timing(const tpiv_plan* plan, double* ms4) {
    if (!plan || !ms4) return fail(TPIV_EINVAL, "null argument");
    if (!plan->exact_count) return fail(TPIV_EINVAL, "not a TPIV_PREC_EXACT plan with an even first-pass window size from 8 to 128");
    for (int s = 0; s < 4; ++s) ms4[s] = plan->exact_ms[s];
    return TPIV_OK;
}

}  // extern "C"
