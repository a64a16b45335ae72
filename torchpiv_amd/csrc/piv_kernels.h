// Internal launch interface between the C-ABI layer (c_api.cpp) and the kernels
// (the .hip units of this directory; dispatch in piv_launch.hip).  Not part of the public boundary (include/torchpiv_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tpiv {

// MODE_CWSF: the reference's piv_iteration_CWS_Fast (B:599-675): bicubic resampling of every window inside
// itself; runs the generic-size kernel only
enum { MODE_PASS1 = 0, MODE_DWS = 1, MODE_CWS = 2, MODE_CWSF = 3 };

struct PassParams {
    const uint8_t* A;      // [batch, H, W] frame a
    const uint8_t* B;      // [batch, H, W] frame b
    int batch, H, W;
    int ws, ov, n_rows, n_cols;
    // predictor inputs of passes >= 2, [batch, n_rows, n_cols] float64
    const double* u0;      // predictor after invalid-zeroing (fallback value)
    const double* v0;
    const double* u2;      // window half-shift: DWS rint(u0/2), CWS u0_prezero/2
    const double* v2;
    // Compact hand-off from the plan's predictor (tpiv_plan_run): pmask != nullptr means u0 / v0 hold the RAW
    // predictor (before the invalid-zeroing), pmask its thresholded mask, and u2 / v2 are not used -- the
    // zeroing and the half shift are formed where they are read (pred_half_shift / pred_fallback below): two
    // float64 fields and a byte per window cross HBM instead of four fields.
    const uint8_t* pmask;
    // outputs [batch, n_rows, n_cols]
    double* u;
    double* v;
    uint8_t* val;          // 1 = invalid (peak ratio below val_ratio)
    double* du;            // optional: raw displacement of this pass (passes >= 2)
    double* dv;
    double val_ratio;
    int val_win;
    int precision;         // pass 1 only: 0 = float32 kernels, 1 = float64 (TPIV_PREC_REFERENCE), 3 = exact sums (every even size from 8 to 128)
    // test hooks (nullptr in production)
    float* dbg_win;        // [batch, N, 2, ws, ws] staged windows (after the shift)
    float* dbg_corr;       // [batch, N, ws, ws] corr - min + eps, fftshift layout
    unsigned long long* stamps;   // diagnostic build (-DTPIV_STAMPS) only: per-phase cycle sums
    // workspace [batch, N, 8] float32 between the tile kernel and finalize_kernel:
    // {c[m], c[left], c[right], c[top], c[bot], c[m2], bits(m), bits(dead)} per window
    // (float64 pass 1: 8 doubles per window, m and dead stored as values)
    float* peak_raw;
    unsigned* work_ctr;      // 8 x 16 dwords: per-XCD item counters of the tile kernel (set by launch_xcorr)
    // 64x64 CWS pass in two launches (round 5): the fast-path-only kernel appends the items that need the per-pixel staging
    // path to slow_list (count: slow_count); the full kernel then runs with list_mode = 1 over exactly those items
    int* slow_list;
    unsigned* slow_count;
    int list_mode;
    // precision "exact" (pass 1 at every even size from 8 to 128, xcorr_exact.hip; all set by launch_xcorr): the float32 kernel's candidate cells
    // per window (8 x int16: arg-max, 3 second-peak cells, 4 minimum cells; -1 = none, arg-max -1 = undecided, -2 = dead),
    // and the windows that go to the float64 kernel instead (undecided ones)
    uint4* cand;
    int* fb_list;
    unsigned* fb_count;
    float exact_band;        // width of the decision band of the locating pass per unit of E+ (exact_band_coef(ws); "The band" below)
    float exact_band_range;  // optional floor of the band relative to the map range (TPIV_EXACT_BAND_RANGE experiments; 0 by default)
    hipEvent_t* sub_events;  // host side only, optional: [3] recorded behind the locating pass, the refinement, the float64 list pass
    // n / d for n < 2^31 as (n * magic) >> shift (set by the tile launcher; keeps the per-item index
    // arithmetic in the scalar unit instead of a hoisted float reciprocal that occupies a VGPR)
    unsigned groups_magic, ncols_magic;
    int groups_shift, ncols_shift;
};

// ---- precision "exact": constants shared by the locating passes (xcorr_tile.hpp peak_candidates, xcorr_big.hpp,
// xcorr_generic.hip map_candidates), the refinement (xcorr_exact.hip) and the launcher
// The band.  A decision of the locating pass is right whenever every cell of its float32 map is within band / 2 of the
// exact one (up to a common offset and a common factor 1 + O(u), which change no order).  The float32 map's cell error is
// BOUNDED -- DESIGN.md 3.4b derives it from the standard FFT error analysis (Higham, Accuracy and Stability of Numerical
// Algorithms, 2nd ed., Thm 24.2), u = 2^-24:
//     |map32(d) - map(d)|  <=  Gamma E+,     E+ = (|a'|^2 + |b'|^2) / 2  >=  |a'| |b'|,     a' = a / mean(a) - 1,
//     Gamma = 2 (F + 1) u + 5 u + I u
//   F u: normwise relative error of the forward 2-D transform of a' + i b' (+ 1 u for the rounding of its inputs), carried
//        through the bilinear cross-spectrum by Cauchy-Schwarz: sum_k |dP_k| <= |dZ| |Z| = (F + 1) u N (|a'|^2 + |b'|^2);
//   5 u: the cross-spectrum's own arithmetic (re = 2 (ad + bc), im = (c^2 - a^2) + (d^2 - b^2): <= 5 u (|z_k|^2 + |z_-k|^2) / 4 per bin);
//   I u: the inverse 2-D transform, componentwise: |dy_d| <= I u sum_k |P_k| <= I u N |a'| |b'|.
// Per 1-D transform of length n (a 2-D transform is two of them):
//   radix-2/4 codelets (fft_inreg.hpp; tile kernels and 128x128): F = I = eta log2 n, eta = 6.66 per radix-2 level
//       (twiddle error + 4 roundings; a radix-4 butterfly with its one twiddle per two levels is below two radix-2 levels);
//   two-factor mixed-radix transforms (fft_mixed.hpp, radix_pass: n = n1 n2, direct small DFTs of radix r <= 8, each
//       (r + 3) sqrt(r) u normwise, + 4 u for the twiddle between them): F = I <= 64 for every pair;
//   plain O(n^2) DFTs (first-generation generic kernel): componentwise (n + 3) u sum |x|: I = n + 3, F = (n + 3) sqrt(n).
// 64 x 64: Gamma = 247 u = 1.47e-5 (measured over tools/research/exact_band.py's families and its adversarial search: <= 8e-7).
// The locating pass forms E+ from the exact integer window sums (sum a, sum a^2: v_sad_u8 / v_dot4_u32_u8 on the bytes it
// staged) and uses band = 2 Gamma (1 + 1/16) E+ -- the 1/16 covers the float32 rounding of E+ itself and of the band
// comparisons.
constexpr double EXACT_ETA = 6.66;
enum { EXACT_FFT_RADIX2 = 0, EXACT_FFT_MIXED = 1, EXACT_FFT_PLAIN = 2 };
inline double exact_gamma_u(int ws, int kind) {       // Gamma in units of u = 2^-24
    double lg = 0.0, rt = 1.0;
    for (int n = 1; n < ws; n *= 2) lg += 1.0;         // ceil(log2 ws)
    while ((rt + 1.0) * (rt + 1.0) <= (double)ws) rt += 1.0;
    rt += 1.0;                                         // >= sqrt(ws)
    const double f1 = kind == EXACT_FFT_PLAIN ? (ws + 3) * rt : (kind == EXACT_FFT_MIXED ? 64.0 : lg * EXACT_ETA);
    const double i1 = kind == EXACT_FFT_PLAIN ? (double)(ws + 3) : f1;
    return 2.0 * (2.0 * f1 + 1.0) + 5.0 + 2.0 * i1;
}
inline float exact_band_coef(int ws, int kind = EXACT_FFT_RADIX2) {
    return (float)(2.0 * exact_gamma_u(ws, kind) * (1.0 + 1.0 / 16) * 5.9604644775390625e-08);
}
constexpr int EXACT_MAX_SECOND = 3, EXACT_MAX_MIN = 4;

struct PredictParams {
    int batch, mode;
    int nrc, ncc, nrf, ncf;       // coarse / fine grid
    const double* Ay;             // [nrf, nrc]
    const double* Ax;             // [ncf, ncc]
    const double* u_c;            // [batch, nrc, ncc]
    const double* v_c;
    const uint8_t* val_c;
    double* T;                    // workspace [batch, 3, nrc, ncf]
    double* u0;                   // [batch, nrf, ncf]
    double* v0;
    double* u2;
    double* v2;
};

// Banded form of the predictor (plan path, predict_mfma.hip).  The rows of the spline operator decay like
// 0.268^|j - j0|, so everything outside a 65-tap band is below float64 rounding of the sum.  Per block of
// 32 fine rows / columns: a dense K x 32 weight tile over the union of the block's bands (zero elsewhere),
// K a multiple of 8.
struct BandedPredictParams {
    int batch, mode;
    int nrc, ncc, nrf, ncf;
    int KY, KX;                   // taps per row / column block
    int nrfp;                     // nrf rounded up to a multiple of 32: pitch of the transposed T1
    const double* Wy32;           // [ceil(nrf / 32)][KY][32]
    const int* k0y32;             // first coarse row of the block's tile
    const double* Ax32;           // [ceil(ncf / 32)][KX][32]
    const int* k0x32;             // first coarse column of the block's tile
    const double* u_c;            // [batch, nrc, ncc]
    const double* v_c;
    const uint8_t* val_c;
    double* T1;                   // workspace [batch, 3, ncc, nrfp]: the row operator's result, transposed
    double* u0;                   // [batch, nrf, ncf]
    double* v0;
    double* u2;
    double* v2;
    uint8_t* mask_out;            // compact output (PassParams::pmask): u0 / v0 receive the RAW predictor, u2 / v2 nothing
};

// post-validation on the device (postval.hip)
struct PostvalParams {
    double* u;               // [batch, n_rows, n_cols], modified in place (border interpolation, determined fills)
    double* v;
    const uint8_t* invalid;  // [batch, n_rows, n_cols] 1 = invalid vector
    uint8_t* cls;            // out [batch, n_rows, n_cols]: 0 valid, 2 hole filled here, 3 ambiguous hole,
                             //     4 general hole, 5 ring (valid cell next to a hole)
    int* counts;             // out [batch, 4]: holes, ring cells, ambiguous holes, general holes
    int batch, n_rows, n_cols;
};
hipError_t launch_postval(const PostvalParams& p, hipStream_t stream);
// ring / hole lists of the pairs that need the host triangulation, packed pair after pair in np.argwhere order
hipError_t launch_postval_compact(const double* u, const double* v, const uint8_t* cls, const int* counts, int batch, int n_rows,
                                  int n_cols, int* offsets, int* ring_rc, double* ring_uv, int* hole_rc, hipStream_t stream);
// B:894-898 for a batch: flip along the rows, sign of v, unit scaling (the reference's expression, bit-identical)
hipError_t launch_finish_fields(const double* u, const double* v, int batch, int n_rows, int n_cols, double scale, double dt,
                                double* fu, double* fv, hipStream_t stream);
// ensemble statistics (postval.hip): out [5][cells] = mean u, mean v, <u'u'>, <v'v'>, <u'v'> of n stacked fields
hipError_t launch_ensemble_moments(const double* U, const double* V, int n, long long cells, double* out, hipStream_t stream);

// image ingest (ingest.hip): raw uncompressed BMP files -> uint8 frames
hipError_t launch_bmp_unpack(const uint8_t* raw, const long long* desc, const uint8_t* lut, int n_files, int H, int W,
                             uint8_t* out, hipStream_t stream);
// the same with the ensemble-minimum background subtracted (bg2 [2, H, W]: desc[f][5] picks the slot)
hipError_t launch_bmp_unpack_bg(const uint8_t* raw, const long long* desc, const uint8_t* lut, int n_files, int H, int W,
                                const uint8_t* bg2, uint8_t* out, hipStream_t stream);
// static background (background.hip): acc = min(acc, frames[0..n)) per pixel; out = max(frames, bg) - bg (out may be frames)
hipError_t launch_frame_min(const uint8_t* frames, int n, long long pixels, uint8_t* acc, hipStream_t stream);
hipError_t launch_subtract_background(const uint8_t* frames, int n, long long pixels, const uint8_t* bg, uint8_t* out,
                                      hipStream_t stream);
// spatial pre-filters (prefilter.hip): out = filter(max(frames, bg) - bg), bg [H, W] or nullptr; kind PREFILTER_MIN: minus the
// minimum of the size x size neighbourhood, PREFILTER_MEAN: minus its rounded mean (clamped at 0), PREFILTER_NONE: nothing; then
// min(., cap) (cap 255: none).  One workgroup per PREFILTER_TILE_COLS x PREFILTER_TILE_ROWS tile of a frame, the tile and its
// halo staged in LDS; out must not overlap frames (a stencil).
constexpr int PREFILTER_NONE = 0, PREFILTER_MIN = 1, PREFILTER_MEAN = 2;
constexpr int PREFILTER_TILE_COLS = 128, PREFILTER_TILE_ROWS = 64;
hipError_t launch_prefilter(const uint8_t* frames, int n, int H, int W, const uint8_t* bg, int kind, int size, int cap,
                            uint8_t* out, hipStream_t stream);

// deep frames (depth.hip).  Tone map: out[f][p] = lut[src[src_off[f] + p]] for n frames of H x W uint16 samples (src_off:
// n element offsets on the device, nullptr: f * H * W), the 64 KiB table staged in LDS once per persistent workgroup, two
// workgroups per CU.  Histogram: hist[v] += count of v among src[0 .. total), exact, privatised in LDS as packed 16-bit
// counters (one workgroup per CU) and flushed with 64-bit atomics; src must be 2-byte aligned, hist 8-byte aligned.
hipError_t launch_depth_map(const uint16_t* src, const long long* src_off, int n, int H, int W, const uint8_t* lut,
                            uint8_t* out, int n_cu, hipStream_t stream);
hipError_t launch_depth_histogram(const uint16_t* src, long long total, unsigned long long* hist, int n_cu,
                                  hipStream_t stream);

// tile-wise adaptive histogram equalization (equalize.hip, defined in include/torchpiv_hip.h): a table kernel, one workgroup
// per (frame, tile), writes luts [n, ky, kx, 256]; a map kernel, one workgroup per rectangle between tile centres, blends the
// four neighbour tables into out, which may be frames itself.  equalize_tiles: the tiles k of an axis of n pixels.
constexpr int EQUALIZE_TILE_MIN = 8, EQUALIZE_TILE_MAX = 256, EQUALIZE_CLIP_Q8_MIN = 256, EQUALIZE_CLIP_Q8_MAX = 65536;
inline int equalize_tiles(int n, int tile) {
    const long long k = (2LL * n + tile) / (2LL * tile);
    return k < 1 ? 1 : (int)k;
}
hipError_t launch_equalize(const uint8_t* frames, int n, int H, int W, int tile, int clip_q8, uint8_t* out, uint8_t* luts,
                           hipStream_t stream);

// normalized median test (outlier.hip): one lane per cell, one workgroup per OUTLIER_TILE_COLS x OUTLIER_TILE_ROWS tile
// (a wavefront per tile row), the tile and its one-cell halo staged in LDS
constexpr int OUTLIER_TILE_COLS = 64, OUTLIER_TILE_ROWS = 8;
struct OutlierParams {
    const double* u;         // [batch, n_rows, n_cols]
    const double* v;
    const uint8_t* invalid;  // the mask as the peak-ratio test left it; read as a snapshot
    int batch, n_rows, n_cols;
    double threshold, eps;
    int min_neighbours;      // 1..8
    uint8_t* status;         // out: bit 0 = flagged here, bit 1 = invalid on input
    double* out_u;           // optional; replace == 0: the neighbourhood medians, replace != 0: the field with its
    double* out_v;           //   flagged cells at their medians (the plan's passes before the last)
    int replace;
    uint8_t* invalid_out;    // optional: invalid | flag (the plan's last pass); none of the outputs may alias an input
};
hipError_t launch_median_test(const OutlierParams& p, hipStream_t stream);

// local least-squares fit of vector fields (fieldfit.hip, defined in include/torchpiv_hip.h: tpiv_field_fit): one lane per
// cell, one workgroup per FIELDFIT_TILE_COLS x FIELDFIT_TILE_ROWS tile, the tile and its `radius` halo staged in LDS
constexpr int FIELDFIT_TILE_COLS = 64, FIELDFIT_TILE_ROWS = 8;
struct FieldFitParams {
    const double* u;         // [batch, n_rows, n_cols]
    const double* v;
    const uint8_t* skip;     // optional: non-zero = not data
    int batch, n_rows, n_cols;
    int radius;              // 1..3
    int order_max;           // 1 or 2: the order asked for
    double* fit;             // out [6, batch, n_rows, n_cols]: U, Ux, Uy, V, Vx, Vy
    uint8_t* count;          // out: data cells used
    int8_t* order;           // out: the order fitted, 2 / 1 / 0 / -1; none of the outputs may alias an input
};
hipError_t launch_field_fit(const FieldFitParams& p, hipStream_t stream);

// particle images and their pairing (particles.hip, defined in include/torchpiv_hip.h: tpiv_particle_count / _detect /
// _match).  Detection: a wavefront per image row, PARTICLE_BLOCK_ROWS adjacent rows per workgroup, a lane per
// PARTICLE_LANE_PIXELS adjacent pixels of a 256-pixel step along the row; launch_particle_count leaves the per-row counts
// scanned in row_start, launch_particle_detect walks the rows again and writes the list in raster order.  Matching: a
// lane per particle of frame a, three launches (nearest candidate, claim by distance, claim by index and verdict).
constexpr int PARTICLE_BLOCK_ROWS = 4, PARTICLE_LANE_PIXELS = 4;
struct ParticleParams {
    const uint8_t* frames;   // [n, H, W]
    int n, H, W;
    int level;               // 0..255
    const uint8_t* mask;     // optional [H, W]: non-zero = no particle image here
    const double* table;     // [256] ln(max(i, 1)) (detect only)
    int32_t* row_start;      // [n, H + 1]: out of count, in of detect
    int32_t* count;          // out of count [n]
    int capacity;            // detect: entries per frame of x, y, peak
    double *x, *y;           // out of detect [n, capacity]
    uint8_t* peak;           // out of detect [n, capacity]
};
hipError_t launch_particle_count(const ParticleParams& p, hipStream_t stream);
hipError_t launch_particle_detect(const ParticleParams& p, hipStream_t stream);
struct ParticleMatchParams {
    const double *xa, *ya;   // [n, cap_a]
    const int32_t* rsa;      // [n, H + 1]
    int cap_a;
    const double *xb, *yb;   // [n, cap_b]
    const int32_t* rsb;      // [n, H + 1]
    int cap_b;
    int n, H, W;
    const double *up, *vp;   // [n, n_rows, n_cols]
    int n_rows, n_cols;
    const double *xc, *yc;   // [n_cols], [n_rows], ascending
    double radius;
    int32_t* match;          // out [n, cap_a]
    uint8_t* status;         // out [n, cap_a]
    double* d2;              // out [n, cap_a]
    int32_t* matched;        // out [n], zero on entry
    unsigned long long* claim_d2;    // work [n, cap_b], all bits set on entry
    unsigned* claim_i;               // work [n, cap_b], all bits set on entry
};
hipError_t launch_particle_match(const ParticleMatchParams& p, hipStream_t stream);

// stereoscopic reconstruction (stereo.hip, defined in include/torchpiv_hip.h: tpiv_stereo_reconstruct): a workgroup of
// STEREO_BLOCK_THREADS lanes keeps the geometry of its cells in registers and walks STEREO_BLOCK_PAIRS pairs of the
// stack; a lane owns one cell (8-byte accesses) or, where every plane allows it, two adjacent ones (16-byte accesses).
// The per-pair summary is a second launch, one workgroup of STEREO_SUM_THREADS lanes per pair.
constexpr int STEREO_BLOCK_THREADS = 256, STEREO_BLOCK_PAIRS = 8, STEREO_SUM_THREADS = 1024;
struct StereoParams {
    const double *u1, *v1, *u2, *v2;         // [batch, cells]
    const double *su1, *sv1, *su2, *sv2;     // optional, all four or none
    const uint8_t* skip;                     // optional [cells]
    const double *a1, *b1, *a2, *b2;         // [cells]
    int batch;
    long long cells;
    double fill;
    double *U, *V, *W, *res;                 // out [batch, cells]
    double *sU, *sV, *sW;                    // out with the sigmas
    uint8_t* status;                         // out [batch, cells]
    double* pair_rms;                        // out [batch]
    int32_t* pair_count;                     // out [batch]; none of the outputs may alias an input
};
hipError_t launch_stereo_reconstruct(const StereoParams& p, hipStream_t stream);

// stereo self-calibration (stereo.hip, defined in include/torchpiv_hip.h: tpiv_stereo_triangulate): the same streaming
// layout -- STEREO_BLOCK_THREADS lanes, one or two cells per lane, STEREO_BLOCK_PAIRS items of the stack per workgroup --
// writes the points and the status; the sums of the plane fit are a second launch, one workgroup of STEREO_SUM_THREADS
// lanes per item, that triangulates its cells again instead of reading the points back (they are optional).
struct TriangulateParams {
    const double *dx, *dy;                   // [batch, cells]
    const double *X, *Y;                     // [cells]
    const uint8_t* skip;                     // optional [cells]
    int batch;
    long long cells;
    double C1[3], C2[3];                     // the camera centres
    double gap_max;
    double plane[3], tol;                    // c0, c1, c2
    double centre[3];                        // Xm, Ym, Zm of the sums
    double *Mx, *My, *Mz, *gap;              // out [batch, cells], all four or none
    uint8_t* status;                         // out [batch, cells]
    int32_t* count;                          // out [batch]
    double* sums;                            // out [batch, 9]; none of the outputs may alias an input
};
hipError_t launch_stereo_triangulate(const TriangulateParams& p, hipStream_t stream);

// geometric mask (mask.hip, defined in include/torchpiv_hip.h).  apply: out = mask ? 0 : frames for n frames against one
// image (out may be frames itself).  coverage: a wavefront per window of the (ws, ov) grid counts its masked pixels into count
// (optional) and writes grid = count > limit (optional).  fields: u = v = +0.0, invalid = invalid_value, status = 2 (optional)
// at the cells of every pair where grid != 0.
hipError_t launch_apply_mask(const uint8_t* frames, int n, long long pixels, const uint8_t* mask, uint8_t* out,
                             hipStream_t stream);
hipError_t launch_mask_coverage(const uint8_t* mask, int H, int W, int ws, int ov, int n_rows, int n_cols, int32_t* count,
                                uint8_t* grid, int limit, hipStream_t stream);
hipError_t launch_mask_fields(double* u, double* v, uint8_t* invalid, uint8_t* status, const uint8_t* grid, int batch,
                              int n_rows, int n_cols, int invalid_value, hipStream_t stream);
// the per-pair forms: masks [n, pixels] (mask f for frame f), count and grid [n, n_rows, n_cols], grids [batch, n_rows, n_cols]
hipError_t launch_apply_mask_pairs(const uint8_t* frames, int n, long long pixels, const uint8_t* masks, uint8_t* out,
                                   hipStream_t stream);
hipError_t launch_mask_coverage_pairs(const uint8_t* masks, int n, int H, int W, int ws, int ov, int n_rows, int n_cols,
                                      int32_t* count, uint8_t* grid, int limit, hipStream_t stream);
hipError_t launch_mask_fields_pairs(double* u, double* v, uint8_t* invalid, uint8_t* status, const uint8_t* grids, int batch,
                                    int n_rows, int n_cols, int invalid_value, hipStream_t stream);

// per-pair masks of moving bodies (dynmask.hip, defined in include/torchpiv_hip.h: tpiv_dynamic_mask): an erosion kernel
// (core = erode(a) | erode(b) into `core`, [n, H, W] bytes of the caller's workspace) and a dilation kernel
// (out = dilate(core) | fixed != 0), both on the tiles of the pre-filter.  out and core overlap neither each other nor an input.
constexpr int DYNMASK_BRIGHT = 0, DYNMASK_DARK = 1;
hipError_t launch_dynamic_mask(const uint8_t* a, const uint8_t* b, int n, int H, int W, int kind, int size, int level,
                               int grow, const uint8_t* fixed, uint8_t* out, uint8_t* core, hipStream_t stream);

// geometric rectification (dewarp.hip, defined in include/torchpiv_hip.h): out[f] = frame f (at element offset src_off[f] on
// the device, nullptr: f * H * W) sampled through map int32 [H, W, 2] (signed Q8, x first), bilinear or Catmull-Rom with the
// Q10 weight table int16 [256, 4] (read by DEWARP_CUBIC only); a lane per four adjacent output pixels, the frames of a
// launch in chunks of DEWARP_FRAME_CHUNK along the grid's second dimension.  Out of place only; H * W < 2^31.
constexpr int DEWARP_LINEAR = 0, DEWARP_CUBIC = 1, DEWARP_FRAME_CHUNK = 8;
hipError_t launch_dewarp(const uint8_t* frames, const long long* src_off, int n, int H, int W, const int32_t* map,
                         const int16_t* table, int interp, int fill, uint8_t* out, hipStream_t stream);

// correlation-statistics uncertainty (uncertainty.hip, defined in include/torchpiv_hip.h: tpiv_uncertainty): one workgroup
// per window; the two half-shifted patches as int16 and one component's asymmetry contributions as int32 in LDS (150 KB at
// ws = 128, R = 4), exact 64-bit integer sums, a float64 epilogue in one lane.  batch * n_rows * n_cols < 2^31.
constexpr int UNCERTAINTY_MIN_WS = 4, UNCERTAINTY_MAX_WS = 128, UNCERTAINTY_MAX_RADIUS = 4;
struct UncertaintyParams {
    const uint8_t* A;        // [batch, H, W]
    const uint8_t* B;
    int batch, H, W, ws, ov, n_rows, n_cols;
    const double* u;         // [batch, n_rows, n_cols], pixels from a to b
    const double* v;
    const uint8_t* invalid;  // optional [batch, n_rows, n_cols]: non-zero = no estimate (NaN, zero stats row)
    const uint8_t* exclude;  // optional [n_rows, n_cols], one grid for every pair: the same (a plan's mask grid)
    int exclude_stride;      // 0: that one grid; n_rows * n_cols: a grid per pair (a plan's per-pair grids)
    int radius;              // 0..UNCERTAINTY_MAX_RADIUS
    double* su;              // out [batch, n_rows, n_cols]
    double* sv;
    long long* stats;        // optional out [batch, n_rows, n_cols, 8]
};
hipError_t launch_uncertainty(const UncertaintyParams& p, hipStream_t stream);

// iterative image deformation (deform.hip, defined in include/torchpiv_hip.h: tpiv_deform_nodes / _warp / _combine).
// Nodes: int16 [batch, n_rows, n_cols, 2], the Q8 half shift (x first), 4-byte aligned.  The warp kernel owns a tile of
// 64 x 32 output pixels per workgroup, both frames of a pair; its source footprints come from LDS patches where they fit
// and from the per-pixel gather where they do not (force_gather != 0: everywhere) -- the same bytes either way.
// H, W < 2^22, H * W < 2^30 (Q8 coordinates and flat indices in 32 bits); batch and H / 32 at most 65535 (the grid).
struct DeformWarpParams {
    const uint8_t* A;        // [batch, H, W]
    const uint8_t* B;
    int batch, H, W, ws, ov, n_rows, n_cols;
    const int16_t* nodes;    // [batch, n_rows, n_cols, 2]
    const int16_t* table;    // int16 [256, 4], Q10 (read by DEWARP_CUBIC only)
    int interp;              // DEWARP_LINEAR / DEWARP_CUBIC
    int force_gather;
    uint8_t* wa;             // out [batch, H, W]
    uint8_t* wb;
    int* counter;            // optional int32 [2]: += tiles sampled from LDS, tiles gathered
};
hipError_t launch_deform_nodes(const double* u, const double* v, const uint8_t* invalid, int batch, int n_rows, int n_cols,
                               int smooth, int16_t* nodes, hipStream_t stream);
hipError_t launch_deform_warp(const DeformWarpParams& p, hipStream_t stream);
hipError_t launch_deform_combine(const int16_t* nodes, const double* du, const double* dv, const uint8_t* dval, size_t cells,
                                 double* u, double* v, uint8_t* invalid, hipStream_t stream);

hipError_t launch_xcorr(const PassParams& p, int mode, int n_cu, hipStream_t stream);
// bytes of the tile kernels' work-queue counters (8 x one 64-byte line), and of the slow-item list header behind them
constexpr size_t TILE_CTR_BYTES = 8 * 16 * sizeof(unsigned), TILE_SLOW_HDR_BYTES = 256;
// 64x64 CWS pass at the fast operation order: fast-path-only kernel at three wavefronts per SIMD + a second launch of the full
// kernel over the items it set aside
constexpr bool tile_split64(int ws, int mode) { return ws == 64 && mode == MODE_CWS; }
// wavefronts per SIMD the tile kernel of (ws, mode) is built for (the OCC template argument of xcorr_tile_kernel;
// 8x8: of xcorr_tile_cand_kernel only, its passes run xcorr_w8.hip); 0 for sizes that run another kernel.
// The full 64x64 CWS kernel stays at two: built for three it spills 97 registers.
constexpr int tile_occ_c(int ws, int mode) {
    return (ws != 8 && ws != 16 && ws != 32 && ws != 64) ? 0
           : (ws == 16 ? 4 : ((ws == 32 || (ws == 64 && mode != MODE_CWS)) ? 3 : 2));
}
inline int tile_occ(int ws, int mode) { return tile_occ_c(ws, mode); }
#ifdef __HIPCC__
// The predictor as the kernels of a shifted pass read it.  MODE is MODE_DWS or MODE_CWS.
//   half shift (B:705-706 CWS: halves taken BEFORE the zeroing; B:782-785 DWS: rint(u0 / 2) AFTER it)
// (The loads are unconditional -- the form is chosen by selecting POINTERS, wave-uniformly: the kernels fetch the
//  next item's shift one iteration ahead, and a load under `if` makes the compiler wait right behind it.)
template <int MODE>
__device__ __forceinline__ void pred_half_shift(const PassParams& p, size_t i, double& sx, double& sy) {
    const bool compact = p.pmask != nullptr;
    const double* __restrict__ us = compact ? p.u0 : p.u2;
    const double* __restrict__ vs = compact ? p.v0 : p.v2;
    double u = us[i], v = vs[i];
    if constexpr (MODE == MODE_DWS) {
        const uint8_t* mp = compact ? p.pmask + i : reinterpret_cast<const uint8_t*>(us + i);    // (any readable byte)
        const bool zero = *mp != 0 && compact;
        const double uz = zero ? 0.0 : u, vz = zero ? 0.0 : v;
        sx = compact ? rint(uz / 2) : u;
        sy = compact ? rint(vz / 2) : v;
    } else {
        sx = compact ? u / 2 : u;
        sy = compact ? v / 2 : v;
    }
}
//   the CWS half shift as the float32 the staging uses (B:714-715 casts u2, v2 to float32): halving is exact in
//   either precision, so float(u / 2) == float(u) * 0.5f -- one float32 multiply instead of float64 work
__device__ __forceinline__ void pred_half_shift_cws_f32(const PassParams& p, size_t i, float& vx, float& vy) {
    const bool compact = p.pmask != nullptr;
    const double* __restrict__ us = compact ? p.u0 : p.u2;
    const double* __restrict__ vs = compact ? p.v0 : p.v2;
    const float k = compact ? 0.5f : 1.0f;
    vx = (float)us[i] * k;
    vy = (float)vs[i] * k;
}
//   fallback value: the predictor after the invalid-zeroing (B:711-713 / B:778-780)
__device__ __forceinline__ void pred_fallback(const PassParams& p, size_t i, double& u0, double& v0) {
    const bool compact = p.pmask != nullptr;
    const uint8_t* mp = compact ? p.pmask + i : reinterpret_cast<const uint8_t*>(p.u0 + i);
    const bool zero = *mp != 0 && compact;
    u0 = zero ? 0.0 : p.u0[i];
    v0 = zero ? 0.0 : p.v0[i];
}
#endif

// symbol-like name of the kernel launch_xcorr picks for (ws, mode) -- for bench / profile labels
const char* xcorr_kernel_name(int ws, int mode, int precision, char* buf, int len);
// bytes of PassParams::peak_raw a pass needs (records, work-queue counters, generic-size DFT scratch)
size_t peak_raw_bytes(int ws, int batch, int n_windows, int precision, bool force_generic = false);
// precision "exact": window sizes whose first pass runs the exact scheme (every even size from 8 to 128; xcorr_exact.hip)
bool exact_refine_size(int ws);
// precision "exact": byte offset of the float64-list counter (one unsigned) inside PassParams::peak_raw
size_t exact_fallback_count_offset(int batch, int n_windows);
// test hook: peak stage + finalize on caller-made maps; planar selects the LDS layout variant of the tile kernel
hipError_t launch_peaks_from_maps(const PassParams& p, const float* maps, int n_maps, int planar, hipStream_t stream);
// ensemble correlation (xcorr_ens.hip, defined in include/torchpiv_hip.h: tpiv_ensemble_add / _peaks): window sizes 16, 32, 64;
// both launches work in PassParams::peak_raw of ensemble_work_bytes(n_windows) bytes
bool ensemble_size(int ws);
size_t ensemble_work_bytes(int n_windows);
hipError_t launch_ensemble_add(const PassParams& p, int mode, float* acc, int n_cu, hipStream_t stream);
hipError_t launch_ensemble_peaks(const PassParams& p, int mode, const float* acc, long long n_pairs, int n_cu,
                                 hipStream_t stream);
// spectrally filtered passes (xcorr_spec.hip, defined in include/torchpiv_hip.h: tpiv_plan_set_correlation): window sizes 16,
// 32 and 64, pass 1 / DWS / CWS.  The filter travels as a second kernel argument: PassParams keeps its layout.
struct SpecParams {
    const float* tab;        // device: g_y[0 .. ws/2], then g_x[0 .. ws/2] (all ones: phase-only correlation)
    float floor;             // tau = floor x mean |P|
};
bool spec_size(int ws);
// the pass with its finalize step; p.peak_raw: peak_raw_bytes(ws, batch, n_windows, 0)
hipError_t launch_xcorr_spec(const PassParams& p, int mode, const SpecParams& s, int n_cu, hipStream_t stream);
const char* xcorr_spec_kernel_name(int ws, int mode, char* buf, int len);
// weighted interrogation windows (xcorr_win.hip, defined in include/torchpiv_hip.h: tpiv_plan_set_weighting): window sizes 16,
// 32 and 64, pass 1 / DWS / CWS.  The tables travel as a second kernel argument: PassParams keeps its layout.
struct WinParams {
    const float* tab;        // device: g_y[0 .. ws-1], then g_x[0 .. ws-1] (all ones: the top-hat through these kernels)
};
bool win_size(int ws);
// the pass with its finalize step; p.peak_raw: peak_raw_bytes(ws, batch, n_windows, 0)
hipError_t launch_xcorr_win(const PassParams& p, int mode, const WinParams& s, int n_cu, hipStream_t stream);
const char* xcorr_win_kernel_name(int ws, int mode, char* buf, int len);
// single-pixel ensemble correlation (pixelcorr.hip, defined in include/torchpiv_hip.h: tpiv_pixel_corr_add / _peaks).  The
// add kernel keeps a bin's sum of one call in 32 bits: 256 pixels x 256 pairs x 255^2 < 2^32, hence the batch bound.
constexpr int kPixelCorrMinRadius = 3, kPixelCorrMaxRadius = 16, kPixelCorrMaxBin = 256, kPixelCorrMaxShift = 64;
constexpr int kPixelCorrMaxBatch = 256, kPixelCorrMaxPairs = 65536;
hipError_t launch_pixel_corr_add(const uint8_t* a, const uint8_t* b, int batch, int H, int W, int ky, int kx, int radius,
                                 int sy, int sx, long long* acc, long long* mom, hipStream_t stream);
hipError_t launch_pixel_corr_peaks(const long long* acc, const long long* mom, int n_pairs, int H, int W, int ky, int kx,
                                   int radius, int sy, int sx, double* u, double* v, double* peak, double* ratio,
                                   uint8_t* status, double* corr, hipStream_t stream);
hipError_t launch_predict_mfma(const BandedPredictParams& q, hipStream_t stream);
hipError_t launch_predict(const PredictParams& q, hipStream_t stream);

}  // namespace tpiv
