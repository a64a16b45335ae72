/* torchpiv_hip.h -- C ABI of the MI355X-native PIV cross-correlation engine.
 *
 * The reference (NikNazarov/TorchPIV) has no FFI layer: its boundary is the Python
 * class OfflinePIV (src/torchPIV/PIVbackend.py:824-903) calling pure functions on
 * torch tensors.  This library replaces the device part of those functions; the
 * Python host (torchpiv_amd/backend.py) binds it with ctypes and keeps the
 * reference's class / function signatures.  Each entry point cites the reference
 * code it replaces (B: = src/torchPIV/PIVbackend.py).
 *
 * Conventions
 *   - every pointer named *_dev is device memory on the CURRENT HIP device, owned by
 *     the caller (PyTorch-ROCm tensors: tensor.data_ptr()); the run functions only enqueue
 *     work on `stream` (a hipStream_t passed as void*; NULL = the null stream) and return at
 *     once.  No run function allocates device memory or synchronises: a plan owns its workspace
 *     (allocated by tpiv_plan_create and, for the outlier test, by tpiv_plan_set_outlier -- both at
 *     the call, never during a run), and the function-level entry points (tpiv_pass1 /
 *     tpiv_iter) take a caller-provided work buffer of tpiv_work_bytes() bytes (hand-off records
 *     between the tile kernel and the finalize kernel).  The library keeps no state between
 *     calls, so calls on different streams (with different work buffers) may overlap;
 *   - fields are row-major [batch, n_rows, n_cols]; frames are uint8 [batch, H, W];
 *   - return value: TPIV_OK or an error code; tpiv_last_error() gives the message
 *     of the calling thread's last failure.  Nothing is thrown across the ABI.
 */
#ifndef TORCHPIV_HIP_H
#define TORCHPIV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TPIV_VERSION 2

enum tpiv_status {
    TPIV_OK = 0,
    TPIV_EINVAL = 1,  /* bad window / overlap / shape: the reference raises ValueError (B:503-507) */
    TPIV_EKEY = 2,    /* unknown multipass mode: the reference raises KeyError (B:850) */
    TPIV_EHIP = 3,    /* a HIP runtime call failed */
    TPIV_ENOMEM = 4,
    TPIV_EUNSUPPORTED = 5 /* valid for the reference but outside what the kernels cover */
};

enum tpiv_mode {
    TPIV_MODE_DWS = 1, /* discrete window shift,  piv_iteration_DWS  B:744-812 */
    TPIV_MODE_CWS = 2, /* continuous window shift, piv_iteration_CWS B:677-740 */
    TPIV_MODE_CWS_FAST = 3 /* piv_iteration_CWS_Fast B:599-675 (bicubic grid_sample of every window inside itself,
                              u = u0 + du); the reference's OfflinePIV cannot reach it (absent from IterModMap):
                              tpiv_iter only, generic-size kernel; u2 / v2 unused (may be NULL), u0 / v0 are the
                              predictor AFTER the invalid-zeroing (tpiv_predict's u0 / v0) */
};

enum tpiv_precision {
    TPIV_PREC_FAST = 0,      /* pass 1 in float32 (observed deviation ~1e-6 px); shifted passes form the CWS
                                sample as row lerps + a column lerp with the reference's float32 weights
                                (float32 rounding differences against B:187-193) */
    TPIV_PREC_REFERENCE = 1, /* pass 1 in float64 like the reference (B:513-514 promotes the windows to
                                float64 before the FFT); shifted passes evaluate B:187-193 operation by
                                operation, so the staged windows are bit-identical to the reference's
                                (the transforms of passes >= 2 are float32 in the reference itself,
                                B:249-257, with a float64 epilogue, B:382) */
    TPIV_PREC_F64 = 2,       /* the reference's ARITHMETIC TYPES in every pass -- pass 1 in float64 (as
                                TPIV_PREC_REFERENCE), shifted passes in float32 with the float64 epilogue -- with
                                the cheaper operation order of TPIV_PREC_FAST in the shifted passes (row lerps +
                                column lerp of the CWS sample: float32 rounding differences, <= 1e-4 grey levels,
                                against B:187-193). */
    TPIV_PREC_EXACT = 3      /* as TPIV_PREC_F64, with the map cells that reach the result of pass 1 (arg-max, its
                                neighbours, second peak, minimum: B:383-411, B:518) evaluated as EXACT integer
                                correlation sums of the uint8 windows instead of through a float64 FFT: a float32
                                FFT pass locates the cells inside an error band (the proven bound on its rounding
                                error), windows it cannot decide run the float64 transform
                                (xcorr_exact.hip).  Every even first-pass window size from 8 to 128; other sizes run
                                as TPIV_PREC_F64.  Within ~1e-14 px of the reference's float64
                                pass 1 (whose own transform rounding is the difference).  The default of the Python
                                drop-in (OfflinePIV). */
};

typedef struct tpiv_plan tpiv_plan;

int tpiv_version(void);
const char* tpiv_last_error(void);

/* ---- host-side geometry (no GPU needed) -------------------------------------- */

/* get_field_shape, B:425-456: (size - ws)//(ws - ov) + 1 per axis. */
int tpiv_field_shape(int H, int W, int ws, int ov, int* n_rows, int* n_cols);

/* get_coordinates, B:522-597: window-centre coordinates along each axis
 * (x: n_cols values, y: n_rows values); the reference returns their meshgrid. */
int tpiv_coordinates(int H, int W, int ws, int ov, double* x, double* y);

/* The predictor operator of scipy.interpolate.RectBivariateSpline(kx=ky=3, s=0)
 * as the reference calls it (B:700-704, 710-711, 769-773, 777-778): row-major
 * A[nf, nc] such that fine = A_y * coarse * A_x^T.  1-D not-a-knot cubic spline
 * interpolation from the nc coarse coordinates xc to the nf fine coordinates xf,
 * evaluation points clamped to [xc[0], xc[nc-1]] (FITPACK does not extrapolate).
 * Needs nc >= 4 (as scipy does). */
int tpiv_spline_matrix(int nc, const double* xc, int nf, const double* xf, double* A);

/* ---- function-level seam (device pointers) ---------------------------------- */

/* Memory contract of every entry point that takes device pointers (tests/test_gpu_memory_contract.py holds each of them
 * to it under guard bands and three fill patterns):
 *   - frames (uint8, and the uint16 samples of tpiv_depth_*) may sit at ANY byte address a multiple of their element size:
 *     the staging's wide loads take any alignment, and no entry point of the correlation seam (tpiv_pass1, tpiv_iter,
 *     tpiv_debug_*, tpiv_ensemble_add, tpiv_uncertainty, tpiv_plan_run*) asks more of a frame than that.  A buffer that needs
 *     more says so at its entry point (the accumulator of tpiv_ensemble_*, the nodes of tpiv_deform_warp, the map of
 *     tpiv_dewarp, the work memory of tpiv_particle_match): a misaligned one is TPIV_EINVAL and nothing is written;
 *   - typed inputs and outputs (double, float, int32, int16, ...) sit at their natural alignment, the work buffer at 256 bytes;
 *   - the prior contents of a work buffer and of every pure output are irrelevant: the library zeroes what it needs zeroed,
 *     and the same call gives the same bits whatever the buffers held;
 *   - every cell of every output is written -- those of masked, dead, invalid and listed windows and of the partial last
 *     wavefront too -- except where an entry point names a part it leaves alone (list entries behind a count or a total,
 *     rows >= batch of a larger output array);
 *   - nothing outside [0, bytes) of any buffer is written, and nothing outside an input reaches a result: a call reads
 *     frame bytes of the pair it works on only, a work buffer of exactly the documented size suffices for every precision
 *     and mode, and a refused call (TPIV_EINVAL: a NULL or short work buffer included) writes nothing at all. */

/* Tensor part of extended_search_area_piv(frame_a, frame_b, window_size, overlap,
 * validate=True, validation_ratio), B:459-520 (+ correalte_fft B:249-257,
 * correlation_to_displacement B:360-422, peak2peak_secondpeak B:346-358).
 * Outputs: u, v float64 and invalid uint8 (1 = peak ratio < val_ratio). */
int tpiv_pass1(const uint8_t* a_dev, const uint8_t* b_dev, int batch, int H, int W,
               int ws, int ov, double val_ratio, int val_win, int precision,
               double* u_dev, double* v_dev, uint8_t* invalid_dev,
               void* work_dev, size_t work_bytes, void* stream);

/* Bytes of device work buffer tpiv_pass1 / tpiv_iter / tpiv_debug_pass need for `batch` pairs of
 * H x W frames at (ws, ov) (either precision); 0 if the geometry is invalid. */
size_t tpiv_work_bytes(int H, int W, int ws, int ov, int batch);

/* Predictor of one multipass iteration (host-side scipy calls in the reference,
 * B:700-717 CWS / B:769-790 DWS): spline-upsample u, v and the invalid mask from
 * the coarse grid [nrc, ncc] to the fine grid [nrf, ncf] with the operators of
 * tpiv_spline_matrix (Ay [nrf, nrc], Ax [ncf, ncc], device memory), threshold the
 * mask at 0.5, zero the predictor where invalid and form the window half-shift
 * (CWS: u0/2 taken before the zeroing; DWS: rint(u0/2) after it).
 * work_dev: batch*3*nrc*ncf float64 of scratch. */
int tpiv_predict(int mode, int batch, int nrc, int ncc, int nrf, int ncf,
                 const double* Ay_dev, const double* Ax_dev,
                 const double* u_c_dev, const double* v_c_dev, const uint8_t* invalid_c_dev,
                 double* work_dev, double* u0_dev, double* v0_dev, double* u2_dev, double* v2_dev,
                 void* stream);

/* Tensor part of piv_iteration_DWS.__call__ (B:791-810, interpolation_DWS B:197-216)
 * or piv_iteration_CWS.__call__ (B:719-738, biliniar_interpolation_CWS B:147-194):
 * shift the windows of frame a by -(u2, v2) and of frame b by +(u2, v2), correlate,
 * find the peak, validate and combine with the predictor
 * (u = 2*u2 + du, fallback to u0 where (du > u0 and rint(u0) > 0) or invalid).
 * du_dev / dv_dev (optional, may be NULL) receive the raw displacement of this pass. */
int tpiv_iter(int mode, const uint8_t* a_dev, const uint8_t* b_dev, int batch, int H, int W,
              int ws, int ov,
              const double* u0_dev, const double* v0_dev, const double* u2_dev, const double* v2_dev,
              double val_ratio, int val_win, int precision,
              double* u_dev, double* v_dev, uint8_t* invalid_dev,
              double* du_dev, double* dv_dev, void* work_dev, size_t work_bytes, void* stream);

/* ---- plan: the whole multipass pipeline of OfflinePIV.__call__ for a batch ---- */

/* Mirrors OfflinePIV.__init__ (B:825-858): pass p > 0 uses ws_p = int(ws_{p-1} // pass_scale),
 * ov_p = int(ov_{p-1} // pass_scale).  Allocates (on the current device) the spline
 * operators and the per-pass field workspace for up to max_batch pairs.
 * precision: enum tpiv_precision (arithmetic of pass 1). */
int tpiv_plan_create(tpiv_plan** out, int H, int W, int ws, int ov, int n_pass, int mode,
                     double pass_scale, double val_ratio, int val_win, int max_batch, int precision);
void tpiv_plan_destroy(tpiv_plan* plan);
int tpiv_plan_n_pass(const tpiv_plan* plan);
int tpiv_plan_pass_geometry(const tpiv_plan* plan, int pass, int* ws, int* ov, int* n_rows, int* n_cols);

/* Name of the cross-correlation kernel pass `pass` launches (for bench / profile labels), e.g.
 * "xcorr_tile_kernel<32, 2, 3, true>" (the demangled form profilers print; second argument: 0 pass 1, 1 DWS, 2 CWS; last: fast arithmetic).  Returns buf. */
const char* tpiv_plan_kernel_name(const tpiv_plan* plan, int pass, char* buf, int len);

/* Pass 1 and every further pass (B:873-882) for `batch` <= max_batch pairs; the last
 * pass writes straight into u_dev / v_dev / invalid_dev ([batch, n_rows_last, n_cols_last]). */
int tpiv_plan_run(tpiv_plan* plan, const uint8_t* a_dev, const uint8_t* b_dev, int batch,
                  double* u_dev, double* v_dev, uint8_t* invalid_dev, void* stream);

/* Device pointers to the fields pass `pass` (< n_pass - 1) left in the plan's workspace
 * during the last run (for parity tests of the intermediate passes). */
int tpiv_plan_pass_fields(const tpiv_plan* plan, int pass, double** u_dev, double** v_dev,
                          uint8_t** invalid_dev);

/* ---- normalized median test (extension; the reference validates by the peak ratio alone) ---------- */

/* The normalized median test of Westerweel & Scarano (Exp. Fluids 39, 2005) on fields u, v float64 and the mask
 * invalid uint8 [batch, n_rows, n_cols] (read as a snapshot).  Per cell: N = the up to 8 cells around it that lie in
 * the grid and have invalid == 0, k = |N| (the cell's own mask byte plays no part).  k < min_neighbours: not flagged,
 * medians = the cell's own u, v.  Otherwise, per component w of (u, v): sort the k neighbour values (the order of <,
 * -0.0 before +0.0); med = s[(k-1)/2] for odd k, (s[k/2-1] + s[k/2]) * 0.5 for even k; rmed = the same pick from the
 * sorted residuals |w_i - med|; out_w = |w_centre - med| > threshold * (rmed + eps); flag = out_u | out_v.  Every
 * operation is one IEEE float64 operation in the order written (no contraction, no division), so a host model that
 * does the same gives the same bits.  Inputs are finite; with NaN / inf nothing is promised except that nothing faults.
 * status_dev uint8: bit 0 = flagged, bit 1 = the cell was invalid on input.  med_u_dev / med_v_dev (float64, either
 * may be NULL): the medians.  No output may overlap an input or another output (TPIV_EINVAL), as are n_rows or
 * n_cols < 1, threshold <= 0, eps < 0 and min_neighbours outside 1..8.  Enqueues only; allocates nothing. */
int tpiv_median_test(const double* u_dev, const double* v_dev, const uint8_t* invalid_dev, int batch, int n_rows,
                     int n_cols, double threshold, double eps, int min_neighbours, uint8_t* status_dev,
                     double* med_u_dev, double* med_v_dev, void* stream);

/* Outlier test of a plan: kind 0 = off (every plan's default: tpiv_plan_run enqueues exactly what it does without this
 * call), 1 = tpiv_median_test with the given parameters after the tile kernels of EVERY pass, on that pass's u, v, invalid:
 *   pass before the last: a flagged cell gets u, v := the medians (out of place: from the fields as the pass left
 *     them); its mask byte stays as the peak-ratio test left it -- the next predictor follows the neighbourhood
 *     where a vector was spurious and still zeroes where the correlation itself was poor;
 *   last pass: invalid |= flag, u and v untouched -- the post-validation treats these cells like peak-ratio holes.
 * The launches go behind the closing event of the pass's timing slot (tpiv_plan_get_timing keeps its meaning).
 * Allocates, at this call, a status map per pass and the spare fields of the out-of-place step for max_batch pairs. */
int tpiv_plan_set_outlier(tpiv_plan* plan, int kind, double threshold, double eps, int min_neighbours);

/* Device pointer to the status map (as tpiv_median_test's) pass `pass` -- the last included -- left during the last
 * run, [batch, n_rows, n_cols] of that pass.  TPIV_EINVAL when the test is off. */
int tpiv_plan_pass_outliers(const tpiv_plan* plan, int pass, uint8_t** status_dev);

/* ---- local least-squares fit: denoised vectors and derivatives (extension; the reference has none) ---------- */

/* Local polynomial regression of fields u, v float64 [batch, n_rows, n_cols] (Raffel et al., "least-squares operators"):
 * per cell the fit's constant term is the denoised vector and its linear terms are the derivatives per cell spacing.
 * skip_dev uint8 of the same shape or NULL: non-zero = the cell is not data.  radius in {1, 2, 3}, order in {1, 2}.
 *
 * A cell is DATA when its skip byte is 0 and both u and v are finite.  Per cell (R, C): S = the data cells (R + j, C + i)
 * with |i|, |j| <= radius inside the grid (the centre included when it is data).  Basis, in this order:
 *   phi_0 .. phi_5 = 1, i, j, i*i, i*j, j*j     (i: column offset, j: row offset, integers); n = 3 at order 1, 6 at order 2.
 * Moments: the integers sum_S i^a j^b, summed in int32, each converted to float64 once (exact); M[p][q] = sum_S phi_p phi_q.
 * Right-hand sides, per component w of (u, v): b[q] starts at +0.0 and takes b[q] = b[q] + w * (double)phi_q(i, j) -- one
 * product, one add -- for the cells of S in row-major order (j outer, i inner, both ascending).
 * LDL^T of M without pivoting, the right-hand sides riding along, A = M, on the lower triangle:
 *   for k = 0 .. n-1:  d[k] = A[k][k];   pivot k is accepted when d[k] > 2^-30 * M[k][k] (one product, one compare);
 *     for q = k+1 .. n-1:  l = A[q][k] / d[k];   for s = k+1 .. q: A[q][s] = A[q][s] - l * A[s][k];
 *                          b[q] = b[q] - l * b[k];   L[q][k] = l;
 *   y[k] = b[k] / d[k];
 *   back substitution over m unknowns, k = m-1 .. 0:  t = y[k];  for q = k+1 .. m-1: t = t - L[q][k] * c[q];  c[k] = t.
 * The ladder: order 2 asked and pivots 0..5 all accepted -> m = 6, order_dev = 2; else pivots 0..2 all accepted -> m = 3 on
 * the shared leading block, order_dev = 1; else |S| >= 1 -> c0 = b[0] / (double)|S| (b[0] as summed, one division), order_dev
 * = 0; else order_dev = -1.  (Over 5 000 random validity patterns per radius a full-rank M keeps every d[k] / M[k][k]
 * >= 7.7e-6 and a rank-deficient one has its first failing pivot <= 3.3e-14: the threshold sits in the gap)
 * fit_dev float64 [6, batch, n_rows, n_cols] = the planes U, Ux, Uy, V, Vx, Vy = c0, c1, c2 of u, then of v; the slopes are
 * NaN at order_dev <= 0 and everything is NaN at -1 (the NaN written is 0x7ff8000000000000).  count_dev uint8 = |S|.
 * order_dev int8.  The fit is evaluated at every cell, skipped ones included (from their neighbours).
 * Every floating-point operation is one IEEE float64 + - * / in the order written (no contraction, no square root), so a
 * host model that does the same gives the same bits -- for data whose sums stay finite; beyond that nothing is promised
 * except that nothing faults.  TPIV_EINVAL, nothing launched: a null u, v, fit, count or order pointer, n_rows or n_cols < 1,
 * batch < 0, radius or order outside their sets, an output that overlaps an input or another output, batch * n_rows * n_cols
 * >= 2^31.  batch == 0 succeeds and launches nothing.  Enqueues only; allocates nothing. */
int tpiv_field_fit(const double* u_dev, const double* v_dev, const uint8_t* skip_dev, int batch, int n_rows, int n_cols,
                   int radius, int order, double* fit_dev, uint8_t* count_dev, int8_t* order_dev, void* stream);

/* ---- stereoscopic reconstruction: three components from two cameras (extension; the reference has none) ------ */

/* Two cameras look at the light sheet z = 0 from different sides; each delivers an in-plane field on the SAME grid of
 * cells, in the same unit: u1, v1 and u2, v2 float64 [batch, cells].  To first order a particle that moves by (U, V, W)
 * is seen by camera c moving by (U + a_c W, V + b_c W), a_c, b_c the viewing tangents of that camera at the cell (a1, b1,
 * a2, b2 float64 [cells], the same for every pair).  Per cell, the least-squares solution of the four equations and the
 * root of the sum of their squared residuals, in float64, every operation rounded once, left to right as written:
 *   du = u1 - u2;  dv = v1 - v2;  da = a1 - a2;  db = b1 - b2;  g = da*da + db*db
 *   W  = (da*du + db*dv) / g
 *   U  = ((u1 + u2) - (a1 + a2)*W) * 0.5
 *   V  = ((v1 + v2) - (b1 + b2)*W) * 0.5
 *   eu = du - da*W;  ev = dv - db*W;  res = sqrt((eu*eu + ev*ev) * 0.5)
 * With the four 1-sigma fields su1, sv1, su2, sv2 [batch, cells] (all four or none), the propagated 1-sigma errors, the
 * four components' errors taken as independent:
 *   q1 = su1*su1;  q2 = su2*su2;  r1 = sv1*sv1;  r2 = sv2*sv2;  qs = q1 + q2;  rs = r1 + r2
 *   sW = sqrt(((da*da)*qs + (db*db)*rs) / (g*g))
 *   ma = (a1 + a2)*0.5;  mb = (b1 + b2)*0.5
 *   ka = ma*da/g;  kb = ma*db/g;  la = mb*db/g;  lb = mb*da/g                       (product, then quotient)
 *   cu1 = 0.5 - ka;  cu2 = 0.5 + ka;  cv1 = 0.5 - la;  cv2 = 0.5 + la
 *   sU = sqrt((cu1*cu1)*q1 + (cu2*cu2)*q2 + (kb*kb)*rs)
 *   sV = sqrt((cv1*cv1)*r1 + (cv2*cv2)*r2 + (lb*lb)*qs)
 * status_dev uint8 [batch, cells], the tests in this order:
 *   1  skip_dev (uint8 [cells] or NULL) is non-zero: U = V = W = fill; res and the sigmas NaN
 *   3  a1, b1, a2 or b2 is not finite, or g == 0 (the two views cannot tell W from U): everything NaN
 *   2  u1, v1, u2 or v2 is not finite: everything NaN
 *   0  otherwise: the reconstruction; a non-finite input sigma makes sU, sV, sW of that cell NaN and nothing else.
 * The NaN written is 0x7ff8000000000000.  Per pair: pair_count_dev int32 [batch] = the status-0 cells; pair_rms_dev
 * float64 [batch] = sqrt(S / (double)count), NaN at count 0, with S = the sum of res*res over the status-0 cells in a
 * fixed order: lane t of 1024 sums the cells t, t + 1024, ... in ascending order from +0.0, then acc[t] = acc[t] +
 * acc[t + s] for s = 512, 256, ..., 1.  No floating-point atomics: the same call gives the same bytes.
 * A host model that does the same operations gives the same bits in U, V, W, res, the sigmas and the status -- for data
 * whose intermediate values stay finite; beyond that nothing is promised except that nothing faults.
 * TPIV_EINVAL, nothing launched: a null field, tangent or output pointer (sU, sV, sW are needed only with the sigmas),
 * batch < 0, cells < 1, a partial set of sigmas, an output that overlaps an input or another output, batch * cells >= 2^31.
 * TPIV_EUNSUPPORTED: more than 524 280 pairs.  batch == 0 succeeds and launches nothing.  The inputs are not written.
 * Enqueues only (two launches); allocates nothing and needs no work memory. */
int tpiv_stereo_reconstruct(const double* u1_dev, const double* v1_dev, const double* u2_dev, const double* v2_dev,
                            const double* su1_dev, const double* sv1_dev, const double* su2_dev, const double* sv2_dev,
                            const uint8_t* skip_dev, const double* a1_dev, const double* b1_dev, const double* a2_dev,
                            const double* b2_dev, int batch, long long cells, double fill, double* U_dev, double* V_dev,
                            double* W_dev, double* res_dev, double* sU_dev, double* sV_dev, double* sW_dev,
                            uint8_t* status_dev, double* pair_rms_dev, int32_t* pair_count_dev, void* stream);

/* Self-calibration: where the light sheet really lies, from the disparity between the two rectified views of the SAME
 * instant.  dx, dy float64 [batch, cells], in mm: camera 2's rectified position of a particle minus camera 1's, along X and
 * along Y (up).  X, Y float64 [cells]: the world position of each cell on z = 0.  The disparity belongs to the midpoint of
 * the two rectified positions (symmetric assignment), so camera 1 saw the particle at q1 and camera 2 at q2 below; the
 * point of the sheet is the midpoint M of the shortest segment between the two lines of sight, gap its length.  Host
 * values, read during the call: cameras_host[6] = the centres C1, C2; plane_host[3] = (c0, c1, c2) of a plane Z = c0 + c1 X +
 * c2 Y with the tolerance tol; centre_host[3] = (Xm, Ym, Zm), subtracted before the sums.  Per cell, in float64, every
 * operation rounded once, left to right as written, a dot product its x, then y, then z term:
 *   hx = dx*0.5;  hy = dy*0.5
 *   q1 = (X - hx, Y - hy, 0);  q2 = (X + hx, Y + hy, 0)
 *   d1 = q1 - C1;  d2 = q2 - C2  (their z: 0.0 - C.z);  w = C1 - C2
 *   a = d1.d1;  b = d1.d2;  c = d2.d2;  d = d1.w;  e = d2.w
 *   den = a*c - b*b
 *   s = (b*e - c*d)/den;  t = (a*e - b*d)/den
 *   p1 = C1 + s*d1;  p2 = C2 + t*d2
 *   M = (p1 + p2)*0.5;  g = p1 - p2;  gap = sqrt(g.g)
 *   r = M.z - ((c0 + c1*M.x) + c2*M.y)
 * status_dev uint8 [batch, cells], the tests in this order:
 *   1  skip_dev (uint8 [cells] or NULL) is non-zero
 *   3  one of the six centre coordinates is not finite
 *   2  dx or dy is not finite
 *   3  den is not finite or den <= 0 (parallel lines of sight; a non-finite X or Y) -- tested behind 2 because a
 *      non-finite dx or dy makes den a NaN: with the centres' test before it, 3 precedes 2 wherever both can be told apart
 *   4  gap > gap_max
 *   5  |r| > tol
 *   0  otherwise.
 * An infinite gap_max or tol switches its test off (the comparison is false).  Mx, My, Mz, gap float64 [batch, cells] --
 * all four or all four NULL -- hold M and gap at status 0, 4 and 5 and NaN (0x7ff8000000000000) at 1, 2 and 3.
 * Per item of the batch, over its status-0 cells: count_dev int32 [batch]; sums_dev float64 [batch, 9] = the sums of
 *   x, y, z, x*x, x*y, y*y, x*z, y*z, z*z    with x = M.x - Xm, y = M.y - Ym, z = M.z - Zm  (one subtraction, one product),
 * each in pair_rms's fixed order: lane t of 1024 sums the cells t, t + 1024, ... in ascending order from +0.0, then acc[t] =
 * acc[t] + acc[t + s] for s = 512, 256, ..., 1.  No floating-point atomics, no contraction: the same call gives the same
 * bytes, and a host model that does the same operations gives the same bits in the points, the status, the count and the
 * sums -- for data whose intermediate values stay finite; beyond that nothing is promised except that nothing faults.
 * TPIV_EINVAL, nothing launched: a null dx, dy, X, Y, host array, status, count or sums pointer, a partial set of Mx, My,
 * Mz, gap, batch < 0, cells < 1, an output that overlaps an input or another output, batch * cells >= 2^31, a gap_max or tol
 * that is negative or NaN.  TPIV_EUNSUPPORTED: more than 524 280 items.  batch == 0 succeeds and launches nothing.  The
 * inputs are not written.  Enqueues only (two launches; the second, one workgroup per item, triangulates again and reads
 * no output of the first); allocates nothing and needs no work memory. */
int tpiv_stereo_triangulate(const double* dx_dev, const double* dy_dev, const double* X_dev, const double* Y_dev,
                            const uint8_t* skip_dev, int batch, long long cells, const double* cameras_host,
                            double gap_max, const double* plane_host, double tol, const double* centre_host,
                            double* Mx_dev, double* My_dev, double* Mz_dev, double* gap_dev, uint8_t* status_dev,
                            int32_t* count_dev, double* sums_dev, void* stream);

/* ---- particle images and their pairing: hybrid PIV / PTV (extension; the reference has none) ------- */

/* Particle images of n frames frames_dev uint8 [n, H, W], H, W >= 3.  Pixel (r, c) with 1 <= r <= H - 2 and 1 <= c <= W - 2
 * and intensity I is a particle image iff
 *   I >= level (0..255),
 *   mask_dev (uint8 [H, W] or NULL, one image for every frame) is zero there,
 *   I >  the pixels (r-1, c-1), (r-1, c), (r-1, c+1), (r, c-1)   -- the four neighbours before it in raster order,
 *   I >= the pixels (r, c+1), (r+1, c-1), (r+1, c), (r+1, c+1)   -- the four behind it;
 * so a plateau of equal pixels gives its raster-first pixel alone, and two horizontally, vertically or diagonally
 * adjacent pixels are never both reported.  Border pixels are never reported, however bright.
 * tpiv_particle_count writes, per frame f, row_start_dev int32 [n, H + 1]: entry r = how many particle images lie in the
 * rows before r (entry 0 = 0, entry H = the total), and count_dev int32 [n] = that total.  Enqueues only (two launches);
 * allocates nothing.
 * tpiv_particle_detect takes row_start_dev as tpiv_particle_count (same frames, level, mask) left it and writes the list of
 * each frame in RASTER ORDER of the peak pixel -- list index = row_start[r] + the particle images of row r left of c; the
 * order is a property of the index, not of scheduling, and no atomic operation takes part -- into x_dev, y_dev float64
 * [n, capacity] and peak_dev uint8 [n, capacity]: peak = I, and with T = table_dev float64 [256] (the caller's table of
 * ln(max(i, 1))), per axis in float64, every operation rounded once, as written:
 *   den = (L - 2*C) + R;  off = den < 0 ? (L - R) / (2*den) : 0
 *   x = c + off   with L = T[I(r, c-1)], C = T[I], R = T[I(r, c+1)]
 *   y = r + off   with L = T[I(r-1, c)], C = T[I], R = T[I(r+1, c)]
 * (image coordinates: x along the columns, y along the rows downward, pixel (0, 0) centred at the origin; |off| <= 1/2 up
 * to rounding).  A host model that does the same operations on the same table gives the same bits.  Capacity: the
 * first `capacity` particle images of a frame are stored; entries at list index >= capacity are not written, nor are the
 * entries of a frame behind its last particle image; row_start and count stay those of the whole list.  capacity == 0
 * writes nothing (x_dev, y_dev, peak_dev may be NULL).  Enqueues only (one launch); allocates nothing.
 * TPIV_EINVAL, nothing launched: a null frames, row_start, count, table or (capacity > 0) list pointer, n < 0, H or W < 3,
 * level outside 0..255, capacity < 0, H * W >= 2^31, n * (H + 1) or n * capacity >= 2^31, an output that overlaps an input
 * or another output.  TPIV_EUNSUPPORTED: more than 65535 frames.  n == 0 succeeds and launches nothing.  The frames, the
 * mask and the table are not written. */
int tpiv_particle_count(const uint8_t* frames_dev, int n, int H, int W, int level, const uint8_t* mask_dev,
                        int32_t* row_start_dev, int32_t* count_dev, void* stream);
int tpiv_particle_detect(const uint8_t* frames_dev, int n, int H, int W, int level, const uint8_t* mask_dev,
                         const double* table_dev, const int32_t* row_start_dev, int capacity, double* x_dev, double* y_dev,
                         uint8_t* peak_dev, void* stream);

/* Pairs the particle images of frame a with those of frame b, for n pairs of frames [H, W].  xa_dev, ya_dev float64
 * [n, cap_a] and rsa_dev int32 [n, H + 1], xb_dev, yb_dev [n, cap_b] and rsb_dev: lists as tpiv_particle_detect writes them
 * (raster order; the stored length of a list is min(row_start[H], capacity)).  up_dev, vp_dev float64 [n, n_rows, n_cols]:
 * the predicted displacement in pixels in image orientation (u along the columns, v along the rows downward, row 0 the
 * top row of windows) at the window centres xc_dev float64 [n_cols], yc_dev [n_rows] (image coordinates, strictly
 * ascending).  radius: R > 0, finite.  For particle i of a at (x, y), in float64, every operation rounded once, as written:
 *   per axis, with k = how many centres are <= the coordinate:  j0 = max(k - 1, 0);  j1 = min(k, n - 1);
 *     t = j1 > j0 ? (coordinate - c[j0]) / (c[j1] - c[j0]) : 0          -- constant outside the centres; a 1-wide grid works
 *   g(x, y) = a + ty*(b - a)   with a = g[y0][x0] + tx*(g[y0][x1] - g[y0][x0]),  b = g[y1][x0] + tx*(g[y1][x1] - g[y1][x0])
 *   px = x + up(x, y);  py = y + vp(x, y)
 *   status 3 unless 0 <= px <= W - 1 and 0 <= py <= H - 1  (a NaN is outside)
 *   candidates: the stored particles j of b in the rows max(ceil(py - R - 0.5), 0) .. min(floor(py + R + 0.5), H - 1) (through
 *     rsb) with  d2 = dx*dx + dy*dy <= R*R,  dx = px - xb[j],  dy = py - yb[j]  (the bound inclusive)
 *   fwd = the candidate of smallest d2, of equal ones the lowest j;  status 1 without a candidate
 *   one-to-one: j goes to the claimant (i with fwd = j) of smallest d2, of equal ones the lowest i; the others get status 2.
 * match_dev int32 [n, cap_a]: j at status 0, else -1.  status_dev uint8 [n, cap_a]: 0 matched, 1 no candidate, 2 lost
 * the candidate to a nearer claimant, 3 predicted outside the frame, 255 for the entries behind the stored list.  d2_dev
 * float64 [n, cap_a]: the d2 to fwd at status 0 and 2, NaN (0x7ff8000000000000) otherwise.  matched_dev int32 [n]: how
 * many have status 0.  The claims are decided by unsigned integer atomic minima (on the bit pattern of d2, which orders
 * like d2 >= +0.0, then on i) between launches, the count by integer atomic adds: nothing depends on scheduling, and a host
 * model that does the same operations gives the same bits.  work_dev: work_bytes >= 16 * n * cap_b bytes, 8-byte aligned,
 * contents ignored and overwritten.  TPIV_EINVAL, nothing launched: a null pointer (lists of capacity 0 and their work
 * memory may be NULL), n < 0, H, W, n_rows or n_cols < 1, a negative capacity, a radius that is not a positive finite
 * number, work memory too small or misaligned, n * (H + 1), n * cap_a, n * cap_b or n * n_rows * n_cols >= 2^31, an output that
 * overlaps an input, the work memory or another output.  TPIV_EUNSUPPORTED: more than 65535 pairs.  n == 0 succeeds and
 * launches nothing.  The inputs are not written.  Enqueues only (two memsets, three launches); allocates nothing. */
int tpiv_particle_match(const double* xa_dev, const double* ya_dev, const int32_t* rsa_dev, int cap_a, const double* xb_dev,
                        const double* yb_dev, const int32_t* rsb_dev, int cap_b, int n, int H, int W, const double* up_dev,
                        const double* vp_dev, int n_rows, int n_cols, const double* xc_dev, const double* yc_dev,
                        double radius, int32_t* match_dev, uint8_t* status_dev, double* d2_dev, int32_t* matched_dev,
                        void* work_dev, size_t work_bytes, void* stream);

/* ---- geometric mask (extension; the reference has none) ------------------------------------------ */

/* Pixel step: out_dev[f][p] = mask_dev[p] != 0 ? 0 : frames_dev[f][p] for n frames [n, pixels] uint8 against one image
 * mask_dev [pixels] uint8 -- any non-zero byte masks, not only 1.  The result is frames & keep with keep = 0x00 on masked
 * pixels and 0xFF elsewhere: a uint8 frame like any other.  out_dev may be frames_dev itself; a partial overlap is
 * TPIV_EINVAL, like a null pointer, n < 0 or pixels < 1.  n == 0 succeeds and launches nothing.  Enqueues only; allocates
 * nothing. */
int tpiv_apply_mask(const uint8_t* frames_dev, int n, long long pixels, const uint8_t* mask_dev, uint8_t* out_dev,
                    void* stream);

/* count_dev [n_rows, n_cols] int32 (the grid of tpiv_field_shape(H, W, ws, ov)) = the number of non-zero bytes of
 * mask_dev [H, W] inside window (i, j), which covers rows i (ws - ov) ... + ws and columns j (ws - ov) ... + ws: the nominal
 * window of a pass, whatever shift a later pass applies to it.  Any ws in 8..256 -- odd and non-power-of-two sizes
 * included -- with any overlap below ws that the passes accept.  Enqueues only; allocates nothing. */
int tpiv_mask_coverage(const uint8_t* mask_dev, int H, int W, int ws, int ov, int32_t* count_dev, void* stream);

/* Excluded cells into the fields of a pass: wherever grid_dev [n_rows, n_cols] uint8 is non-zero, in every pair of
 * u_dev, v_dev float64 and invalid_dev uint8 [batch, n_rows, n_cols]: u = v = +0.0 (whatever was there, a NaN included),
 * invalid = invalid_value (0 or 1), and status = 2 -- tpiv_median_test's "invalid on input, not flagged" -- when status_dev
 * is not NULL.  Every other cell is untouched.  batch == 0 succeeds and launches nothing.  Enqueues only; allocates nothing. */
int tpiv_mask_fields(double* u_dev, double* v_dev, uint8_t* invalid_dev, uint8_t* status_dev, const uint8_t* grid_dev,
                     int batch, int n_rows, int n_cols, int invalid_value, void* stream);

/* Mask of a plan.  mask_dev [H, W] uint8, non-zero = masked; threshold in [0, 1].  For every pass with (ws, ov) the cell
 * (i, j) is EXCLUDED if and only if tpiv_mask_coverage's count > limit, limit = (int)(threshold * (double)(ws * ws)): one
 * float64 product, truncated (limit == ws * ws excludes nothing).  The grids are computed here, once, and kept -- one
 * uint8 [n_rows, n_cols] per pass, allocated at the first call; the image is not needed after the call returns (it waits
 * for the stream).  tpiv_plan_run then, behind the closing event of the pass's timing slot as the median test:
 *   pass before the last: excluded cells read u = v = +0.0, invalid = 1 -- the predictor zeroes them as it zeroes any
 *     invalid vector (no slip at a wall) and the median test does not count them as neighbours;
 *   last pass: u = v = +0.0, invalid = 0 -- to the post-validation an excluded cell is a valid zero vector, never a hole;
 *   with tpiv_plan_set_outlier: one tpiv_mask_fields call with invalid = 1 before the test of every pass (the test runs
 *     on the masked fields), one more on what the test wrote (invalid as above) with the status map, where every excluded
 *     cell then reads exactly 2.  Without the test: one call per pass.
 * The plan does not touch the frames: the pixel step is tpiv_apply_mask, the caller's.  mask_dev NULL switches the mask
 * off (every plan's default): tpiv_plan_run again enqueues exactly what it does without this call. */
int tpiv_plan_set_mask(tpiv_plan* plan, const uint8_t* mask_dev, double threshold, void* stream);

/* Device pointer to the grid of pass `pass`, uint8 [n_rows, n_cols], 1 = excluded.  TPIV_EINVAL when the mask is off. */
int tpiv_plan_pass_mask(const tpiv_plan* plan, int pass, uint8_t** grid_dev);

/* ---- per-pair masks of moving bodies (extension; the reference has none) ------------------------- */

enum tpiv_dynmask_kind {
    TPIV_DYNMASK_BRIGHT = 0, /* a lit body: core where the whole neighbourhood is >= level */
    TPIV_DYNMASK_DARK = 1    /* a shadow: core where the whole neighbourhood is <= level */
};

/* Segments one mask per pair from the frames a_dev, b_dev [n, H, W] uint8 themselves, in integer arithmetic (every
 * implementation of these lines gives the same bytes).  size = 2 r + 1 odd in 3..63, level in 0..255, grow >= 0 with
 * r + grow <= 31.  N_q(y, x) is the (2 q + 1) x (2 q + 1) square around a pixel clipped to the image (no padding value), as
 * in tpiv_prefilter.  Per frame g:
 *   BRIGHT: core(y, x) = [min over N_r(y, x) of g >= level]
 *   DARK:   core(y, x) = [max over N_r(y, x) of g <= level]
 *   obj(y, x) = [core is set somewhere in N_(r + grow)(y, x)]
 * -- the morphological opening of {g >= level} ({g <= level}) by the size x size square, grown by `grow`: anything
 * narrower than size in either direction vanishes, what survives comes back at full width.
 *   masks_dev[f] = obj(a[f]) | obj(b[f]) | (static_dev != 0), bytes 0 / 1, [n, H, W]; static_dev [H, W] uint8 or NULL.
 * work_dev: at least tpiv_dynamic_mask_work_bytes(n, H, W) bytes on the device (0 for a shape the call refuses);
 * afterwards it holds the union of both frames' cores, one byte (0x00 / 0xFF) per pixel and pair.  masks_dev and work_dev
 * overlap neither each other nor an input; the inputs are not written.  TPIV_EINVAL for a bad kind, size, level, grow or
 * shape (n < 0, H or W outside 1..2^28, H above 65535 * 64), a null pointer or such an overlap: decided on the host, nothing is launched then.
 * n == 0 succeeds and launches nothing.  Enqueues two kernels; allocates nothing and never synchronises. */
size_t tpiv_dynamic_mask_work_bytes(int n, int H, int W);
int tpiv_dynamic_mask(const uint8_t* a_dev, const uint8_t* b_dev, int n, int H, int W, int kind, int size, int level,
                      int grow, const uint8_t* static_dev, uint8_t* masks_dev, void* work_dev, void* stream);

/* tpiv_apply_mask with mask f for frame f: out_dev[f][p] = masks_dev[f][p] != 0 ? 0 : frames_dev[f][p], all [n, pixels]
 * uint8.  out_dev may be frames_dev itself; a partial overlap, or any overlap of out_dev with the masks, is TPIV_EINVAL,
 * like a null pointer, n < 0 or pixels < 1.  n == 0 succeeds and launches nothing.  Enqueues only; allocates nothing. */
int tpiv_apply_mask_pairs(const uint8_t* frames_dev, int n, long long pixels, const uint8_t* masks_dev, uint8_t* out_dev,
                          void* stream);

/* tpiv_mask_coverage for n masks masks_dev [n, H, W]: count_dev [n, n_rows, n_cols] int32, count[f][i][j] = the non-zero
 * bytes of mask f inside window (i, j).  Any ws in 8..256 and any overlap, like the static one.  n == 0 succeeds and
 * launches nothing.  Enqueues only; allocates nothing. */
int tpiv_mask_coverage_pairs(const uint8_t* masks_dev, int n, int H, int W, int ws, int ov, int32_t* count_dev,
                             void* stream);

/* tpiv_mask_fields with one grid per pair: wherever grids_dev [batch, n_rows, n_cols] uint8 is non-zero, the same cell of
 * the same pair reads u = v = +0.0, invalid = invalid_value (0 or 1) and status = 2 (status_dev not NULL).  Every other cell
 * is untouched.  batch == 0 succeeds and launches nothing.  Enqueues only; allocates nothing. */
int tpiv_mask_fields_pairs(double* u_dev, double* v_dev, uint8_t* invalid_dev, uint8_t* status_dev,
                           const uint8_t* grids_dev, int batch, int n_rows, int n_cols, int invalid_value, void* stream);

/* Per-pair grids of a plan.  on != 0 allocates, at this call (the first such call), one uint8 [max_batch, n_rows, n_cols]
 * grid per pass; on == 0 switches them off again.  TPIV_EINVAL for a plan with tpiv_plan_set_ensemble on (and
 * tpiv_plan_set_ensemble refuses a plan with these grids on); a pass with a window size outside 8..256 is refused as
 * tpiv_plan_set_mask refuses it.  tpiv_plan_run is not affected. */
int tpiv_plan_set_pair_masks(tpiv_plan* plan, int on);

/* tpiv_plan_run with one mask per pair, masks_dev [batch, H, W] uint8 (non-zero = masked; the device reads them
 * when the enqueued work runs, so they stay valid until then).  First, for every
 * pass with (ws, ov), one tpiv_mask_coverage_pairs-like launch writes the plan's grids of this batch: cell (i, j) of pair f
 * is EXCLUDED if and only if count[f][i][j] > limit, limit = (int)(threshold * (double)(ws * ws)) -- tpiv_plan_set_mask's
 * rule, threshold in [0, 1].  Then everything tpiv_plan_run enqueues, with pair f's grid wherever a plan with a static
 * mask reads its one grid: the mask steps behind every pass and every deformation round, with and without the median
 * test (tpiv_mask_fields_pairs in the place of tpiv_mask_fields), and the grid the uncertainty kernel reads.  A static mask
 * set with tpiv_plan_set_mask is superseded for this run (callers OR the static image into masks_dev) and applies again to
 * the next tpiv_plan_run.  The plan does not touch the frames: the pixel step is tpiv_apply_mask_pairs, the caller's.
 * TPIV_EINVAL without tpiv_plan_set_pair_masks, for a bad threshold or batch, or a null mask pointer.  Enqueues only;
 * allocates nothing. */
int tpiv_plan_run_masked(tpiv_plan* plan, const uint8_t* a_dev, const uint8_t* b_dev, const uint8_t* masks_dev,
                         double threshold, int batch, double* u_dev, double* v_dev, uint8_t* invalid_dev, void* stream);

/* Device pointer to the grids of pass `pass` that the last tpiv_plan_run_masked used, uint8 [batch, n_rows, n_cols] of that
 * run, 1 = excluded.  TPIV_EINVAL when the per-pair grids are off. */
int tpiv_plan_pass_pair_mask(const tpiv_plan* plan, int pass, uint8_t** grid_dev);

/* ---- per-vector uncertainty (extension; the reference has none) ---------------------------------- */

/* Correlation-statistics uncertainty (B. Wieneke, Meas. Sci. Technol. 26 (2015) 074002): the 1-sigma random error, in
 * pixels, of every vector of a field u, v float64 [batch, n_rows, n_cols] at geometry (ws, ov) measured on frames a, b
 * uint8 [batch, H, W].  u is the displacement along x (columns), v along y (rows), from a to b.  st = ws - ov; window
 * (r, c) starts at y0 = r st, x0 = c st.  Supported: 4 <= ws <= 128 of any parity, 0 <= ov < ws, 0 <= radius R <= 4, a
 * frame that holds at least one window.  Per window, in integers:
 *   1. hx = clamp(rint(u * 128), -32767, 32767) (ties to even; the product is exact), hy likewise from v: the half shift
 *      in Q8.  A non-finite u or v: su = sv = NaN and an all-zero stats row.
 *   2. Two patches, indices i, j = -R ... ws + R (P = ws + 2R + 1 a side).  a*[i][j] is frame a at qy = ((y0 + i) << 8)
 *      - hy, qx = ((x0 + j) << 8) - hx, b*[i][j] frame b at + hy, + hx: iy = qy >> 8 (arithmetic), fy = qy & 255, ix, fx
 *      likewise; taps at rows clamp(iy, 0, H-1), clamp(iy + 1, 0, H-1) and the columns alike; value = (sum wy wx p +
 *      8192) >> 14 with weights (256 - f, f): 0 ... 1020, grey levels in Q2.
 *   3. N = ws^2, core = 0 <= i, j < ws.  ma = (sum_core a* + N/2) / N (integer division), mb likewise; a' = a* - ma,
 *      b' = b* - mb everywhere.
 *   4. C0 = sum_core a'[i][j] b'[i][j].  Component x: d[i][j] = a'[i][j] b'[i][j+1] - a'[i][j+1] b'[i][j], s the same with
 *      +; component y with [i+1][j] for [i][j+1].  S2 = sum_core s (= C(+1) + C(-1)); S(k,l) = sum_core d[i][j] d[i+k][j+l];
 *      S00 = S(0,0); the lags of the half plane {1 <= k <= R, -R <= l <= R} and {k = 0, 1 <= l <= R} count iff
 *      20 S(k,l) > S00; var = S00 + 2 sum_counted S(k,l); n = the number counted.  |d| < 2^21 and every sum stays below
 *      2^63 inside the supported range.
 *   5. In float64, every operation rounded on its own: sd = sqrt((double)var), s2 = (double)S2, c0 = (double)C0,
 *      cp = (s2 + sd) * 0.5, cm = (s2 - sd) * 0.5.  sigma = NaN when C0 <= 0, !(cm > 0) or !(c0 c0 > cp cm); otherwise
 *      sigma = (log cp - log cm) / (4 log c0 - 2 log cm - 2 log cp): unsigned, > 0 when finite.
 * su_dev, sv_dev float64 [batch, n_rows, n_cols]; stats_dev (may be NULL) int64 [batch, n_rows, n_cols, 8] = C0, S2x, S00x,
 * varx, S2y, S00y, vary, nx + 256 ny.  invalid_dev (may be NULL) uint8 [batch, n_rows, n_cols]: a non-zero byte gives NaN
 * in both components and an all-zero stats row.  The integers are the same in every implementation of these lines; only
 * the logarithms carry a tolerance.  TPIV_EINVAL, with nothing launched: a size outside the ranges above, a null pointer,
 * an output that overlaps an input or another output, H or W >= 2^22 or H * W >= 2^30 (the Q8 coordinates and the flat
 * pixel indices are 32-bit), batch * n_rows * n_cols >= 2^31.  batch == 0 succeeds and launches nothing.  Enqueues only; allocates
 * nothing and needs no work memory. */
int tpiv_uncertainty(const uint8_t* a_dev, const uint8_t* b_dev, int batch, int H, int W, int ws, int ov,
                     const double* u_dev, const double* v_dev, const uint8_t* invalid_dev, int radius, double* su_dev,
                     double* sv_dev, long long* stats_dev, void* stream);

/* Uncertainty of a plan: kind 0 = off (every plan's default: tpiv_plan_run enqueues exactly what it does without this
 * call), 1 = tpiv_uncertainty with the given radius behind the last pass -- behind its outlier and mask steps and behind the
 * closing event of its timing slot (tpiv_plan_get_timing keeps its meaning) -- on the frames the run was given and on the
 * u, v, invalid it returns: cells the run returns as invalid (median-flagged ones included) are NaN, and so are the cells
 * of the last pass's mask grid.  Allocates, at this call, su and sv for max_batch pairs at the last pass's geometry.  A
 * last pass with ws > 128 or ws < 4, or a radius outside 0..4: TPIV_EINVAL. */
int tpiv_plan_set_uncertainty(tpiv_plan* plan, int kind, int radius);

/* Device pointers to su, sv of the last run, [batch, n_rows, n_cols] of the last pass.  TPIV_EINVAL when it is off. */
int tpiv_plan_uncertainty(const tpiv_plan* plan, double** su_dev, double** sv_dev);

/* ---- iterative image deformation (extension; the reference shifts windows rigidly) ---------------- */

/* OR-ed into tpiv_deform_warp's interp: every tile takes the per-pixel gather (the same bytes; measurements and tests). */
#define TPIV_DEFORM_GATHER 0x100

/* Image deformation behind the last pass (Scarano, Meas. Sci. Technol. 13 (2002) R1; predictor smoothing after Schrijer &
 * Scarano, Exp. Fluids 45 (2008) 927): the field u, v of the last pass, geometry (ws, ov), st = ws - ov, grid n_rows x n_cols
 * of tpiv_field_shape, window (r, c) at row r st and column c st, becomes a dense half shift; frame a is resampled at -h and
 * frame b at +h into uint8 frames; tpiv_pass1 measures the residual on them; the sum is the new field.  u runs along x
 * (columns), v along y (rows), from a to b.  Everything is integer except the last addition, so every implementation of
 * these lines gives the same bytes.
 *   Nodes (tpiv_deform_nodes): int16 [batch, n_rows, n_cols, 2], x first, the half shift in Q8.
 *     A cell is VALID when its invalid byte is 0 and u and v are both finite: q = clamp(rint(w * 128), -16383, 16383) per
 *     component w (the product is exact, ties to even).  Any other cell: s, k = the sum and the count of q over those of its
 *     up to 8 neighbours that lie in the grid and are valid; q = floor((2 s + k) / (2 k)) per component, 0 when k == 0 (the
 *     neighbours are read as a snapshot: substituted values never feed a substitution).  smooth != 0: afterwards the 3 x 3
 *     binomial [[1,2,1],[2,4,2],[1,2,1]] over the substituted values with edge replicate, out of place, q = (sum + 8) >> 4
 *     (arithmetic shift).
 *   Dense half shift of pixel (y, x).  Per axis, shown for rows (n = n_rows): n == 1: r = 0, wy = 0; otherwise
 *     r = clamp(floor((2 y - (ws - 1)) / (2 st)), 0, n - 2), t = clamp(2 y - (ws - 1) - 2 r st, 0, 2 st),
 *     wy = (256 t + st) / (2 st) (integer division, 0 .. 256): bilinear between the window centres r st + (ws - 1) / 2,
 *     constant outside their hull.  h = ((256 - wy) ((256 - wx) n00 + wx n01) + wy ((256 - wx) n10 + wx n11) + 32768) >> 16
 *     per component (arithmetic shift; node indices r + 1, c + 1 clamped to the grid; |sum| < 2^31 by the node clamp).
 *   Warp (tpiv_deform_warp): wa[y][x] = frame a sampled at qx = clamp((x << 8) - hx, 0, (W - 1) << 8), qy = clamp((y << 8) -
 *     hy, 0, (H - 1) << 8); wb[y][x] = frame b at + hx, + hy.  Sampling is tpiv_dewarp's TPIV_DEWARP_LINEAR or
 *     TPIV_DEWARP_CUBIC -- the same Q8 weights, the same Q10 table int16 [256, 4], the same rounding and clamp, tap indices
 *     clamped to the frame -- without its outside case: there is no fill.  Out of place: uint8 [batch, H, W] each.
 *   Combine (tpiv_deform_combine): u = (double)qx * (1.0 / 128) + du (the product is exact: one rounding), v likewise from
 *     qy and dv, invalid = dval, where du, dv, dval are tpiv_pass1's outputs on (wa, wb) at (ws, ov).  2 h / 256 at a window
 *     centre is the node itself: the smoothed, quantised predictor is the shift that was applied, so smoothing and
 *     quantisation cost no accuracy.  The reference's `du > u0` fix-up of the shifted passes (B:236-242) is NOT
 *     reproduced: the residual is added as measured.
 * The three entries enqueue only and allocate nothing; batch == 0 succeeds and launches nothing.  TPIV_EINVAL, with nothing
 * launched: a null pointer (table_dev may be NULL for TPIV_DEWARP_LINEAR, counter_dev always), n_rows or n_cols < 1, ws
 * outside 2..256, ov outside 0..ws-1, a frame that holds no window, H or W >= 2^22 or H * W >= 2^30 (Q8 coordinates and flat
 * pixel indices are 32-bit), batch or (H + 31) / 32 above 65535, batch * n_rows * n_cols >= 2^31, an unknown interp, nodes
 * that are not 4-byte aligned, an output that overlaps an input or another output.
 * counter_dev (optional): int32 [2] on the device, += the number of 64 x 32 pixel tiles whose source footprints were
 * sampled from LDS patches, and of those that took the per-pixel gather because a footprint did not fit (a predictor
 * discontinuity, a huge gradient); both forms give the same bytes. */
int tpiv_deform_nodes(const double* u_dev, const double* v_dev, const uint8_t* invalid_dev, int batch, int n_rows,
                      int n_cols, int smooth, int16_t* nodes_dev, void* stream);
int tpiv_deform_warp(const uint8_t* a_dev, const uint8_t* b_dev, int batch, int H, int W, int ws, int ov,
                     const int16_t* nodes_dev, const int16_t* table_dev, int interp, uint8_t* wa_dev, uint8_t* wb_dev,
                     int32_t* counter_dev, void* stream);
int tpiv_deform_combine(const int16_t* nodes_dev, const double* du_dev, const double* dv_dev, const uint8_t* dval_dev,
                        int batch, int n_rows, int n_cols, double* u_dev, double* v_dev, uint8_t* invalid_dev, void* stream);

/* Deformation of a plan: iterations 0 = off (every plan's default: tpiv_plan_run enqueues exactly what it does without this
 * call), 1..8 = that many rounds behind the last pass -- behind its mask and outlier steps and the closing event of its
 * timing slot (tpiv_plan_get_timing keeps its meaning).  Round k = 1..n: tpiv_deform_nodes on the current u, v, invalid (what
 * the last pass, or round k - 1, left in the caller's fields), tpiv_deform_warp of the run's frames, the first pass
 * (tpiv_pass1 at the last pass's geometry with the plan's precision, val_ratio and val_win) on the warped frames,
 * tpiv_deform_combine into u, v, invalid.  Then, as behind a last pass:
 *   with tpiv_plan_set_mask: excluded cells read u = v = +0.0 and are valid, so they pull the warp to zero at a wall;
 *   with tpiv_plan_set_outlier: rounds before the last take the test's "pass before the last" form (a flagged cell gets the
 *     medians, out of place; its mask byte stays), the last round the "last pass" form (invalid |= flag, u and v untouched);
 *     the status map of the last pass is then that of the last round's test.  With both, the mask goes in front of the test
 *     with invalid = 1 and behind it with invalid = 0 and the status map, in every round.
 * tpiv_plan_set_uncertainty runs behind the rounds, on the original frames and the final fields.  The residual pass records
 * nothing in the timing slots and leaves tpiv_plan_exact_fallbacks alone (it keeps meaning pass 1).  interp:
 * TPIV_DEWARP_LINEAR or TPIV_DEWARP_CUBIC; table_dev: the Q10 table (copied into the plan at this call; may be NULL for
 * linear).  Allocates, at the first call with iterations > 0: the nodes, wa and wb for max_batch pairs, du, dv, dval, the
 * spare fields of the out-of-place median step, the table, and a larger pass-1 work buffer if the last geometry needs one.
 * TPIV_EINVAL: iterations outside 0..8, an unknown interp, a missing cubic table, a last-pass geometry tpiv_pass1 refuses, H
 * or W >= 2^22, H * W >= 2^30. */
int tpiv_plan_set_deform(tpiv_plan* plan, int iterations, int interp, int smooth, const int16_t* table_dev);

/* Device pointers to what the last round of the last run left: nodes int16 [batch, n_rows, n_cols, 2], wa, wb uint8
 * [batch, H, W], du, dv float64 and dval uint8 [batch, n_rows, n_cols].  Any pointer argument may be NULL.  TPIV_EINVAL when
 * the deformation is off. */
int tpiv_plan_deform_stage(const tpiv_plan* plan, int16_t** nodes_dev, uint8_t** wa_dev, uint8_t** wb_dev, double** du_dev,
                           double** dv_dev, uint8_t** dval_dev);

/* Milliseconds all rounds of the last run took together (an event pair around them on the run's stream, recorded in every
 * run of a deforming plan).  Waits for the closing event.  TPIV_EINVAL when the deformation is off or before the first run. */
int tpiv_plan_deform_ms(tpiv_plan* plan, double* ms);

/* ---- ensemble correlation (extension; the reference correlates pair by pair) -------------------------- */

/* Sum-of-correlation PIV (Meinhart, Wereley & Santiago, J. Fluids Eng. 122 (2000) 285): the correlation maps of all pairs
 * of a recording are added window by window and the peak of the summed map is taken once.  Window sizes 16, 32 and 64 (the
 * tile kernels), mode 0 (first pass), TPIV_MODE_DWS or TPIV_MODE_CWS; any other size: TPIV_EUNSUPPORTED.
 *   Map of pair i, window w, C_i[w], float32 [ws, ws] in fftshift layout, RAW -- before any minimum subtraction and before the
 *   1e-7 of B:381: mode 0: the circular cross-correlation of a / mean(a) - 1 and b / mean(b) - 1 (B:513-514 without the
 *   pedestal, which is a constant of the map), the ZERO map when the pixel sum of either window is 0; shifted modes: of the
 *   windows staged at the half shift (u2, v2) exactly as tpiv_iter stages them at TPIV_PREC_FAST (flat-index clamp and
 *   nearest-sample quirk included), minus their means, not normalised.  u2_dev, v2_dev float64 [n_rows, n_cols]: ONE half
 *   shift per window for every pair (DWS: integral values); NULL for mode 0.
 *   tpiv_ensemble_add: acc_dev float32 [n_rows * n_cols, ws, ws] (tpiv_ensemble_bytes bytes, 16-byte aligned, zeroed by the
 *   caller before the first call) += C_0 + C_1 + ... + C_(batch-1), summed in float32 in ascending pair order by the one
 *   wavefront that owns the window: no atomics, so the same sequence of calls gives the same bits.  16 x 16, 32 x 32 and
 *   64 x 64 mode 0 / DWS form T = C_0 + ... + C_(batch-1) first and then acc <- acc + T; 64 x 64 CWS adds pair by pair,
 *   acc <- (...((acc + C_0) + C_1)...).  batch == 0 succeeds and launches nothing.
 *   tpiv_ensemble_peaks: M = acc / n_pairs (one float32 division per cell; n_pairs in 1..2^24) through the peak stage of
 *   every pass -- M - min M + 1e-7, first arg-max, three-point log-Gaussian fit, peak-to-second-peak ratio against val_ratio
 *   over the val_win neighbourhood, float64 epilogue: correlation_to_displacement (B:360-422) on M - min M.  Mode 0 writes
 *   the displacement as u, v [n_rows, n_cols]; a shifted mode combines it with the predictor like tpiv_iter, u = 2 u2 + du
 *   with the fallback to u0 where (du > u0 and rint(u0) > 0) or invalid; u0_dev .. v2_dev are tpiv_predict's outputs for a
 *   batch of one, du_dev / dv_dev (optional) receive the raw displacement.  No window counts as dead here: a window whose
 *   every contribution was the zero map has a constant M and comes out invalid with u = v = 0 (mode 0).
 * work_dev: tpiv_work_bytes(H, W, ws, ov, 1) bytes, for either call.  Both enqueue only and allocate nothing.  TPIV_EINVAL:
 * a null or misaligned accumulator, missing predictor fields, n_pairs out of range, a work buffer that is too small. */
size_t tpiv_ensemble_bytes(int H, int W, int ws, int ov);
int tpiv_ensemble_add(int mode, const uint8_t* a_dev, const uint8_t* b_dev, int batch, int H, int W, int ws, int ov,
                      const double* u2_dev, const double* v2_dev, float* acc_dev, void* work_dev, size_t work_bytes,
                      void* stream);
int tpiv_ensemble_peaks(int mode, const float* acc_dev, long long n_pairs, int H, int W, int ws, int ov,
                        const double* u0_dev, const double* v0_dev, const double* u2_dev, const double* v2_dev,
                        double val_ratio, int val_win, double* u_dev, double* v_dev, uint8_t* invalid_dev,
                        double* du_dev, double* dv_dev, void* work_dev, size_t work_bytes, void* stream);

/* Ensemble correlation of a plan: on != 0 allocates, at the first such call, one accumulator sized for the largest pass, a
 * batch-1 field per pass and a predictor hand-off of its own (tpiv_plan_run in between disturbs nothing, and runs exactly
 * as without this call).  TPIV_EUNSUPPORTED when a pass has a window size other than 16, 32, 64 (the message names it);
 * TPIV_EINVAL on a plan with tpiv_plan_set_uncertainty or tpiv_plan_set_deform on -- and those refuse a plan with this on.
 * The plan's precision has no effect on these calls: maps are float32, the peak epilogue float64.  Per pass p = 0 .. n_pass - 1:
 *   tpiv_plan_ensemble_begin(p): zeroes the accumulator; p > 0: runs the plan's banded predictor ONCE, for a batch of one, on
 *     the ensemble field of pass p - 1 -- one predictor, one mask, one half shift shared by every pair.  TPIV_EINVAL when pass
 *     p - 1 has not been ended.
 *   tpiv_plan_ensemble_add: tpiv_ensemble_add of batch <= max_batch pairs at the pass's geometry and mode, any number of times.
 *   tpiv_plan_ensemble_end: tpiv_ensemble_peaks with the plan's val_ratio / val_win, then the settle step of tpiv_plan_run on
 *     the batch of one -- tpiv_plan_set_mask and tpiv_plan_set_outlier act on an ensemble field exactly as on a pair's field
 *     of that pass (a pass before the last: excluded cells invalid, flagged vectors replaced by the medians; last pass:
 *     excluded cells valid zeros, invalid |= flag).  u_dev, v_dev, invalid_dev [n_rows, n_cols] of that pass receive the
 *     field; a pass before the last also keeps it in the plan for the next begin.  TPIV_EINVAL with no pair added, or before
 *     begin.
 * A failed call changes nothing.  tpiv_plan_ensemble_maps (tests): the accumulator and the pairs added since begin. */
int tpiv_plan_set_ensemble(tpiv_plan* plan, int on);
int tpiv_plan_ensemble_begin(tpiv_plan* plan, int pass, void* stream);
int tpiv_plan_ensemble_add(tpiv_plan* plan, const uint8_t* a_dev, const uint8_t* b_dev, int batch, void* stream);
int tpiv_plan_ensemble_end(tpiv_plan* plan, double* u_dev, double* v_dev, uint8_t* invalid_dev, void* stream);
int tpiv_plan_ensemble_maps(tpiv_plan* plan, float** acc_dev, long long* n_pairs);

/* ---- single-pixel ensemble correlation (extension; the reference has none) ------------------------------ */

/* Single-pixel ensemble correlation (Westerweel, Geelhoed & Lindken, Exp. Fluids 37 (2004) 375; Kaehler, Scholz & Ortmanns,
 * Exp. Fluids 41 (2006) 327; Scharnowski, Hain & Kaehler, Exp. Fluids 52 (2012) 985): the correlation at one pixel, or at a
 * small rectangular bin of pixels, is summed over the pairs of a recording instead of over an interrogation window.
 * Everything up to the coefficient is exact integer arithmetic.
 *   Inputs: prepared frames a_i, b_i, uint8 [H, W] (H * W < 2^31), i = 0 .. N - 1, N <= 65536 pairs in all.
 *   Parameters: search radius R in 3..16, D = 2 R + 1; bin (bin_y, bin_x) = (k_y, k_x), both >= 1, k_y * k_x <= 256, k_y <= H,
 *     k_x <= W; ONE integer pre-shift s = (shift_y, shift_x) for every bin, |s| <= 64 on each axis.
 *   Bins: n_by = H / k_y by n_bx = W / k_x (integer division; the rows and columns left over belong to no bin); bin (r, c)
 *     holds the pixels p = (y, x) with r k_y <= y < (r + 1) k_y and c k_x <= x < (c + 1) k_x.  b counts as 0 outside the frame.
 *   Accumulated, all int64:
 *     acc[r, c, j, i] = sum_i sum_{p in bin} a_i(p) b_i(p + s + d), d = (j - R, i - R)          [n_by, n_bx, D, D]
 *     mom[0..3, y, x] = sum_i a_i, sum_i a_i^2, sum_i b_i, sum_i b_i^2 per pixel, each frame's own coordinates  [4, H, W]
 *   Exact int64 numerators (N <= 2^16, a bin <= 2^8 pixels and bytes < 2^8 keep N acc < 2^56 and every sum of products of
 *   two moments < 2^56, so each of these is below 2^57 in magnitude):
 *     num[d] = N acc[d] - sum_{p in bin} mom0[p] mom2[p + s + d]
 *     va     = N sum_p mom1[p] - sum_p mom0[p]^2
 *     vb[d]  = N sum_p mom3[p + s + d] - sum_p mom2[p + s + d]^2
 *   Coefficient: C[d] = double(num[d]) / sqrt(double(va) * double(vb[d])) -- each conversion and each operation ONE IEEE
 *     float64 operation, in this order, no contraction.
 *   Peak: M = (C - min C) + 1e-7 (the peak stage's recipe); the first arg-max (j, i) in raster order; three-point
 *     log-Gaussian fit per axis, dx = (ln M[j, i-1] - ln M[j, i+1]) / (2 (ln M[j, i+1] + ln M[j, i-1]) - 4 ln M[j, i]), dy
 *     alike along j; u = shift_x + i - R + dx, v = shift_y + j - R + dy; peak = C at the arg-max; ratio = M(peak) / (the
 *     largest M outside the 5 x 5 cells around the peak, clipped to the plane).
 *   Status, uint8, the first that applies: 1 border -- some p + s + d of the bin, d over the whole D x D plane, leaves the
 *     frame; 2 flat -- va = 0 or some vb[d] = 0; 3 range -- the first arg-max over the whole plane lies on its outer ring
 *     (|d_y| = R or |d_x| = R; otherwise it is the first arg-max of the interior); 4 fit -- dx or dy not finite, or |dx| > 1 or
 *     |dy| > 1; 0 valid.  A bin with a non-zero status gets u = v = peak = ratio = NaN; border and flat bins also get an
 *     all-zero plane.  Every output cell is written in every case.
 * tpiv_pixel_corr_bytes: the bytes of acc, n_by n_bx D^2 8; 0 for a refused geometry.  mom is 4 H W 8 bytes.
 * tpiv_pixel_corr_add: acc += and mom += over the pairs a_dev, b_dev uint8 [batch, H, W] (any alignment; 4-byte aligned
 *   frames of a width divisible by 4 load fastest).  The caller zeroes both accumulators before the first call.  One int64
 *   read-modify-write of every cell per call, by the one workgroup that owns the bin: no atomics, and integer sums, so any
 *   split of a recording into calls gives the same bits.  batch <= 256: inside one call a bin's sum is kept in 32 bits, and
 *   256 pixels x 256 pairs x 255^2 = 4 261 478 400 < 2^32.  batch == 0 succeeds and launches nothing.  The frames are not
 *   written; acc and mom may overlap neither each other nor the frames.
 * tpiv_pixel_corr_peaks: u_dev, v_dev, peak_dev, ratio_dev float64 and status_dev uint8 [n_by, n_bx]; corr_dev (optional,
 *   may be NULL) float64 [n_by, n_bx, D, D]: the planes C.  acc_dev and mom_dev are not written.
 * All three enqueue only, allocate nothing and keep no state.  TPIV_EINVAL, with nothing launched and nothing written: a null
 * or not 8-byte aligned accumulator, a null frame pointer (batch > 0) or output pointer, a parameter outside the ranges
 * above, n_pairs outside 1..65536, batch outside 0..256. */
size_t tpiv_pixel_corr_bytes(int H, int W, int bin_y, int bin_x, int radius);
int tpiv_pixel_corr_add(const uint8_t* a_dev, const uint8_t* b_dev, int batch, int H, int W, int bin_y, int bin_x, int radius,
                        int shift_y, int shift_x, int64_t* acc_dev, int64_t* mom_dev, void* stream);
int tpiv_pixel_corr_peaks(const int64_t* acc_dev, const int64_t* mom_dev, int n_pairs, int H, int W, int bin_y, int bin_x,
                          int radius, int shift_y, int shift_x, double* u_dev, double* v_dev, double* peak_dev,
                          double* ratio_dev, uint8_t* status_dev, double* corr_dev, void* stream);

/* ---- spectrally filtered passes: phase-only and robust phase correlation ----------------------------------------------
 * (A. Eckstein, P. Vlachos, Digital particle image velocimetry (DPIV) robust phase correlation, Meas. Sci. Technol. 20
 * (2009) 055401.)  Every pass of a plan with this on takes its peak from a filtered map instead of the plain
 * cross-correlation.  Take a window pair as the pass stages it -- first pass, DWS or CWS staging, quirks included, exactly
 * the windows tpiv_debug_pass reports -- call the staged windows wa, wb (ws x ws) and subtract each window's own mean.
 *   1. P(ky, kx) = conj(F wa) (F wb), F the unnormalised 2-D DFT.  The first pass does NOT divide by the window mean: the
 *      filter is invariant to a scale factor in either frame.
 *   2. m = the mean of |P| over all ws^2 bins, tau = floor x m (floor: 2^-20 .. 2^-4, by default 2^-10).
 *   3. g_x[j] = float32(exp(-(pi d_x / (2 ws))^2 j^2)), j = 0 .. ws/2, and g_y likewise with d_y: evaluated in float64 on
 *      the host, rounded once.  W(ky, kx) = g_y[|ky~|] g_x[|kx~|] as one float32 product, k~ = k for k <= ws/2 and k - ws
 *      otherwise.  With d in e^-2 diameters (0 .. 16 pixels) this is the spectrum exp(-pi^2 f^2 d^2 / 4) of the correlation
 *      of two Gaussian particle images.  TPIV_CORR_PHASE: d_x = d_y = 0, W = 1.
 *   4. Q = W P / max(|P|, tau), and Q = 0 where |P| = 0.  The floor is what makes the filter well defined: a window with
 *      periodic content has bins that are exactly 0, and unfloored rounding noise would be normalised to full weight there.
 *   5. C = fftshift(sum_k Q_k exp(+2 pi i k x / ws)), the UNNORMALISED inverse: a pure circular shift peaks at sum W, and the
 *      1e-7 of the peak stage keeps the relative size it has in a first-pass map.
 *   6. The peak stage of every pass follows unchanged: minimum subtraction, + 1e-7, first arg-max, three-point log-Gaussian
 *      fit, peak-to-second-peak test with the plan's val_ratio / val_win, float64 epilogue; a shifted pass then combines
 *      with the predictor as tpiv_iter does.
 *   7. A window whose mean-free energy is 0 in either frame (a zero, masked or constant window) has m = 0: in the first pass
 *      it is dead exactly as a zero-sum window of the float32 first pass (u = v = 0, valid); in a shifted pass it hands the
 *      zero map to the peak stage, whose peak ratio makes it invalid.  No NaN comes out of 0 x (1 / tau).  The kernels
 *      decide this by exact equality of the float32 energy with 0: exact for integer-valued staged windows (first pass,
 *      DWS, zeroed or masked pixels, constant regions under CWS); a CWS window that is constant only up to the rounding of
 *      its bilinear samples is not empty -- its map is filtered rounding noise, which the peak ratio has to reject.
 * tables (host): for pass 0, 1, ... in turn g_y[0 .. ws/2] then g_x[0 .. ws/2] of that pass's window size, n_tables floats
 * in all; the plan uploads them once.  d_x, d_y and floor are checked against their ranges and floor is what the kernels use;
 * the weights are the tables' (d_x, d_y are not kept).  A plan whose workspace was sized for float64 records alone
 * (TPIV_PREC_REFERENCE / _F64 with few windows) gets a larger one here: a filtered pass works in the float32 layout.
 * tpiv_plan_exact_fallbacks returns TPIV_EINVAL after a filtered run, and tpiv_plan_exact_timing averages over the unfiltered
 * runs alone.  kind = TPIV_CORR_NONE: off, every pass is byte for byte what it was (tables may be NULL).
 * TPIV_EUNSUPPORTED, with a message naming the size, when a pass has a window size other than 16, 32 or 64 (multipass modes
 * of a plan are DWS and CWS; the CWS_Fast iteration has no filtered kernel: tpiv_debug_pass_spec).  TPIV_EINVAL on a plan
 * with tpiv_plan_set_uncertainty, tpiv_plan_set_deform or tpiv_plan_set_ensemble on -- and those refuse a plan with this on.
 * The plan's precision has no effect on a filtered pass: the first pass is the float32 spectral kernel -- the exact integer
 * scheme decides plain correlation sums, not a normalised spectrum.  tpiv_plan_set_mask and tpiv_plan_set_outlier act as
 * on any plan.  tpiv_plan_kernel_name names the spectral kernels for such a plan.  A failed call changes nothing. */
enum { TPIV_CORR_NONE = 0, TPIV_CORR_PHASE = 1, TPIV_CORR_RPC = 2 };
int tpiv_plan_set_correlation(tpiv_plan* plan, int kind, double d_x, double d_y, double floor, const float* tables,
                              size_t n_tables);

/* ---- weighted interrogation windows ------------------------------------------------------------------------------------
 * Every pass of a plan with this on multiplies its windows by a separable weight in front of the transform; the top-hat
 * window of the plain passes has a sinc-shaped frequency response with negative lobes (F. Schrijer, F. Scarano, Effect of
 * predictor-corrector filtering on the stability and spatial resolution of iterative PIV interrogation, Exp. Fluids 45
 * (2008) 927), a Gaussian weight a positive one and a smaller effective footprint.  Take a window pair as the pass stages
 * it -- first pass, DWS or CWS staging, quirks included, exactly the windows tpiv_debug_pass reports -- and call the staged
 * windows wa, wb (ws x ws, float32).
 *   1. W(y, x) = g_y[y] g_x[x], one float32 product; both tables have ws entries and are strictly positive.
 *      TPIV_WEIGHT_GAUSSIAN: g[i] = float32(exp(-t^2 / (2 sigma^2))), t = (2 i - (ws - 1)) / ws, evaluated in float64 on the
 *      host and rounded once; sigma is relative to the half window, 0.2 <= sigma <= 4 (sigma_x for g_x, sigma_y for g_y).
 *      TPIV_WEIGHT_UNIFORM: g = 1, the top-hat window through the weighted kernels.
 *   2. a' = wa - mean(wa), the plain mean: exactly 0 for a constant integer-valued window.
 *   3. mu = sum W a' / sum W, the W-weighted mean of the remainder: the weighted signal has no DC, or the map would carry
 *      the pedestal W * W centred at zero displacement.
 *   4. x_a = W (a' - mu); in the first pass x_a is additionally divided by mean(wa), which keeps the scale of the plain first
 *      pass (B:513-514), so the peak stage's 1e-7 keeps its relative size.  The shifted passes divide by nothing.  x_b
 *      likewise.
 *   5. C = fftshift of the circular cross-correlation of x_a and x_b, as every float32 pass forms it.  The peak stage of
 *      every pass follows unchanged: minimum subtraction, + 1e-7, first arg-max, three-point log-Gaussian fit,
 *      peak-to-second-peak test with the plan's val_ratio / val_win, float64 epilogue; a shifted pass then combines with the
 *      predictor as tpiv_iter does.
 *   6. A window whose energy sum x^2 is exactly 0 in float32 in either frame (a zero, masked or constant window) is handled
 *      as rule 7 of tpiv_plan_set_correlation has it: in the first pass it is dead (u = v = 0, valid), as is a first-pass
 *      window whose pixel sum is 0; in a shifted pass it hands the zero map to the peak stage, whose peak ratio makes it
 *      invalid.  No NaN.  A CWS window that is constant only up to the rounding of its bilinear samples is not empty: its
 *      map is rounding noise, which the peak ratio has to reject.
 *   7. The bias of the weighted correlation toward zero displacement (the envelope W * W) is NOT corrected, as the reference
 *      does not correct the top-hat's triangle; it vanishes as the residual does under predictor passes and
 *      tpiv_plan_set_deform.
 * tables (host): for pass 0, 1, ... in turn g_y[0 .. ws-1] then g_x[0 .. ws-1] of that pass's window size, n_tables floats
 * in all; the plan uploads them once.  The weights are the tables' (sigma_x, sigma_y are checked against their range and not
 * kept).  kind = TPIV_WEIGHT_NONE: off, every pass is byte for byte what it was (tables may be NULL).
 * TPIV_EINVAL: a table entry that is not finite or not in (0, 1], a uniform table that is not all ones, sigma out of range, a
 * wrong n_tables.  TPIV_EUNSUPPORTED, with a message naming the size, when a pass has a window size other than 16, 32 or 64
 * (multipass modes of a plan are DWS and CWS; the CWS_Fast iteration has no weighted kernel: tpiv_debug_pass_weighted).
 * TPIV_EINVAL on a plan with tpiv_plan_set_uncertainty (its estimator sums over a top-hat window), tpiv_plan_set_ensemble or
 * tpiv_plan_set_correlation on -- and those refuse a plan with this on.  It combines with tpiv_plan_set_deform, in either
 * order of the two calls: the residual pass of every round is the weighted first pass at the last pass's geometry with that
 * pass's tables.  The plan's precision has no effect on a weighted pass (float32 kernel, float64 epilogue); a plan whose
 * workspace was sized for float64 records alone gets a larger one here.  tpiv_plan_exact_fallbacks returns TPIV_EINVAL after
 * a weighted run, and tpiv_plan_exact_timing averages over the other runs alone.  tpiv_plan_set_mask and
 * tpiv_plan_set_outlier act as on any plan.  tpiv_plan_kernel_name names the weighted kernels for such a plan.  A failed
 * call changes nothing. */
enum { TPIV_WEIGHT_NONE = 0, TPIV_WEIGHT_UNIFORM = 1, TPIV_WEIGHT_GAUSSIAN = 2 };
int tpiv_plan_set_weighting(tpiv_plan* plan, int kind, double sigma_x, double sigma_y, const float* tables, size_t n_tables);

/* ---- post-validation (B:884-892) ------------------------------------------------- */

/* Device part of the reference's per-pair host post-processing, for a whole batch:
 *   u[val] = v[val] = NaN (B:885-886; `invalid_dev` plays the NaN mask, u/v are not overwritten with NaN),
 *   interpolate_boarders (B:328-344) on u and v in place,
 *   the ring / hole census of getPixelsForInterp (B:266-282) -> counts_dev [batch, 4] int32 =
 *   {holes, ring cells, ambiguous holes, general holes}.  Both drop decisions of fillMissingValues
 *   (B:284-308) follow from the counts: ring == 0 (nothing to interpolate from: the interpolator raises ->
 *   pair dropped, including the "no invalid vector" quirk) and 4 * ring >= n_rows * n_cols ("to many false
 *   vectors").
 *   Holes whose Delaunay-linear value does not depend on the triangulation (both N and S, or both E and W,
 *   neighbours valid, but not all four) are filled in place: (N + S) / 2 resp. (E + W) / 2.  Holes with all
 *   four neighbours valid (co-circular diamond: Qhull's tie-break decides between the two) and holes inside
 *   wider gaps are only classified; a pair with ambiguous + general > 0 needs the host triangulation.
 * cls_dev [batch, n_rows, n_cols] uint8: 0 valid, 2 hole filled here, 3 ambiguous hole, 4 general hole,
 * 5 ring cell.  Needs n_rows, n_cols >= 2. */
int tpiv_postval(double* u_dev, double* v_dev, const uint8_t* invalid_dev, int batch, int n_rows, int n_cols,
                 uint8_t* cls_dev, int32_t* counts_dev, void* stream);

/* What fillMissingValues (B:296-302) hands to the interpolator, cut out of a batch on the device after tpiv_postval: for
 * every pair that is kept (ring > 0, 4 ring < cells) AND holds an ambiguous or general hole, the ring cells
 * (np.argwhere(neighbours), B:298: row-major order -- Qhull's triangulation depends on the insertion order, so the
 * compaction preserves it) with their values, and all hole cells (np.argwhere(invalid_mask), B:297), packed pair after
 * pair into flat lists:
 *   offsets_dev [2, batch + 1] int32: row 0 = start of every pair's ring cells (last entry: total), row 1 = holes;
 *   ring_rc_dev [total ring, 2] int32 (row, column), ring_uv_dev [total ring, 2] float64 (u, v), hole_rc_dev
 *   [total holes, 2] int32.  The caller sizes ring_* for batch * ceil(cells / 4) entries and hole_rc for batch * cells. */
int tpiv_postval_compact(const double* u_dev, const double* v_dev, const uint8_t* cls_dev, const int32_t* counts_dev,
                         int batch, int n_rows, int n_cols, int32_t* offsets_dev, int32_t* ring_rc_dev,
                         double* ring_uv_dev, int32_t* hole_rc_dev, void* stream);

/* B:894-898 for a batch of final fields [batch, n_rows, n_cols]: fu = flip(u, axis 0) * scale / dt * 1000,
 * fv = -flip(v, axis 0) * scale / dt * 1000 -- the reference's float64 expression, left to right, three correctly
 * rounded operations per value: bit-identical to numpy's.  (x, y are not flipped, B:899-900.) */
int tpiv_finish_fields(const double* u_dev, const double* v_dev, int batch, int n_rows, int n_cols, double scale,
                       double dt, double* fu_dev, double* fv_dev, void* stream);

/* ---- ensemble statistics (workers.py:85-96 of the reference's job runner) ------------ */

/* Mean and two-pass central moments of n stacked fields u_dev, v_dev [n, cells] float64 (dataset
 * order): out_dev [5, cells] = mean(u), mean(v), mean((u-U)^2), mean((v-V)^2), mean((u-U)(v-V)),
 * accumulated along the stack IN ORDER like numpy's np.mean(axis=0) -- bit-identical to the reference's
 * np.mean(u_inst, axis=0), np.mean((u_inst - avg_u)**2, axis=0), ... */
int tpiv_ensemble_moments(const double* u_dev, const double* v_dev, int n, long long cells, double* out_dev,
                          void* stream);

/* ---- image ingest (PIVDataset.__getitem__, B:129-144) ------------------------------- */

/* Unpacks n_files uncompressed BMP files that were uploaded as RAW FILE BYTES into uint8 frames
 * out_dev [n_files, H, W] (top-down rows, what cv2.imdecode(..., IMREAD_GRAYSCALE) returns): header
 * skip, bottom-up row flip, row-padding strip, palette look-up (1 byte per pixel) or OpenCV's
 * fixed-point BGR -> gray weights (3 / 4 bytes per pixel).  The host parses the 54-byte headers
 * (torchpiv_amd/io.py) and passes, per file, desc_dev[f][6] int64 = {offset of the file in raw_dev,
 * offset of the pixel data in the file, row stride in bytes, bytes per pixel (1, 3, 4), rows stored
 * bottom-up (0/1), reserved} and lut_dev[f][256] (palette entries already converted to gray). */
int tpiv_bmp_unpack(const uint8_t* raw_dev, const int64_t* desc_dev, const uint8_t* lut_dev, int n_files,
                    int H, int W, uint8_t* out_dev, void* stream);

/* tpiv_bmp_unpack with the static background subtracted in the same pass: out = max(px, bg) - bg per pixel, where
 * bg_dev [2, H, W] uint8 holds two backgrounds (frames a, frames b of a pair) and desc_dev[f][5] picks the one of file f
 * (0: bg_dev[0], otherwise bg_dev[1]).  Bit-identical to tpiv_bmp_unpack followed by tpiv_subtract_background. */
int tpiv_bmp_unpack_bg(const uint8_t* raw_dev, const int64_t* desc_dev, const uint8_t* lut_dev, int n_files,
                       int H, int W, const uint8_t* bg_dev, uint8_t* out_dev, void* stream);

/* ---- static background (ensemble minimum) --------------------------------------------- */

/* acc_dev[p] = min(acc_dev[p], frames_dev[f][p]) over the n frames frames_dev [n, pixels] uint8: one call or several
 * over parts of a recording give the per-pixel minimum of all of them (start from an acc of 255s). */
int tpiv_frame_min(const uint8_t* frames_dev, int n, long long pixels, uint8_t* acc_dev, void* stream);

/* out_dev[f][p] = max(frames_dev[f][p], bg_dev[p]) - bg_dev[p] (frame minus background, clamped at 0) for n frames
 * [n, pixels] uint8.  out_dev may be frames_dev itself; other overlaps are not supported. */
int tpiv_subtract_background(const uint8_t* frames_dev, int n, long long pixels, const uint8_t* bg_dev,
                             uint8_t* out_dev, void* stream);

/* ---- spatial pre-filters ------------------------------------------------------------------ */

enum tpiv_prefilter_kind {
    TPIV_PREFILTER_NONE = 0, /* background and cap only */
    TPIV_PREFILTER_MIN = 1,  /* minus the minimum of the size x size neighbourhood */
    TPIV_PREFILTER_MEAN = 2  /* minus the rounded mean of the size x size neighbourhood, clamped at 0 */
};

/* Filters n frames frames_dev [n, H, W] uint8 into out_dev, one launch for all of them, in integer arithmetic (every
 * implementation of these lines gives the same bytes).  g = max(f, bg) - bg with bg_dev [H, W], g = f with bg_dev NULL.
 * The neighbourhood of a pixel is the size x size square around it clipped to the image (no padding value), c its
 * pixel count, size odd in 3..63.  MIN: out = g - min(neighbourhood of g).  MEAN: S = the neighbourhood's sum,
 * m = (2 S + c) / (2 c) (integer division: the mean rounded half up), out = max(g - m, 0).  NONE: out = g, size is not
 * read.  Then out = min(out, cap), cap in 1..255 (255: no capping).  out_dev must not overlap frames_dev, not even as
 * frames_dev itself (the filter is a stencil): TPIV_EINVAL, like a bad kind, size, cap or shape; nothing is launched
 * then.  Enqueues only; allocates nothing. */
int tpiv_prefilter(const uint8_t* frames_dev, int n, int H, int W, const uint8_t* bg_dev, int kind, int size, int cap,
                   uint8_t* out_dev, void* stream);

/* ---- deep (10..16-bit) frames ---------------------------------------------------------------- */

/* Tone map: out_dev[f][y][x] = lut_dev[src_dev[src_off_dev[f] + y * W + x]] for n frames of uint16 samples, one launch.
 * lut_dev: uint8 [65536] on the device (torchpiv_amd.engine.depth_lut builds the linear and the square-root curve on the
 * host; any table is allowed).  src_off_dev: n element offsets into src_dev, on the device, each frame inside memory of
 * the caller (not checked: they live on the device); NULL: frame f starts at f * H * W.  One launch so turns the
 * interleaved a / b slots of a staged batch into the contiguous stacks the plan reads.  out_dev [n, H, W] must overlap
 * neither the source nor the table; src_dev is not written and no byte outside out_dev's n * H * W is.  src_dev needs
 * 2-byte alignment only (16-byte aligned frames with 8-byte aligned outputs move fastest).  TPIV_EINVAL for a null
 * pointer, n < 0, H or W < 1, an overlap that can be seen from the host; n == 0 succeeds and launches nothing.
 * Enqueues only; allocates nothing. */
int tpiv_depth_map(const uint16_t* src_dev, const long long* src_off_dev, int n, int H, int W, const uint8_t* lut_dev,
                   uint8_t* out_dev, void* stream);

/* hist_dev[v] += the number of samples equal to v among the n frames src_dev [n, pixels_per_frame] uint16, for all 65536
 * values, exactly.  hist_dev: uint64 [65536] on the device, accumulated (start from zeros): one call or several over
 * parts of a recording give the histogram of all of them.  Same error rules as tpiv_depth_map. */
int tpiv_depth_histogram(const uint16_t* src_dev, int n, long long pixels_per_frame, unsigned long long* hist_dev,
                         void* stream);

/* ---- geometric rectification (extension; the reference has none) ------------------------------- */

#define TPIV_DEWARP_LINEAR 0
#define TPIV_DEWARP_CUBIC 1

/* Rectifies n frames through one backward map, in integer arithmetic (every implementation of these lines gives the same
 * bytes), one launch: out_dev[f][r][c] = frame f sampled at the source position map_dev holds for output pixel (r, c).
 *   Frames: uint8, frame f = the H * W bytes from frames_dev + src_off_dev[f] on (src_off_dev: n element offsets on the
 *   device, each frame inside memory of the caller -- not checked: they live on the device; NULL: f * H * W).
 *   Map: int32 [H, W, 2], source x then source y in signed Q8, q = floor(s * 256 + 0.5), pixel centres at the integers.
 *   A pixel is OUTSIDE when qx < 0, qy < 0, qx > (W - 1) << 8 or qy > (H - 1) << 8 (torchpiv_amd.engine.dewarp_map stores
 *   such entries as (-1, -1)): out = fill.  Else ix = qx >> 8, fx = qx & 255, likewise y, every tap coordinate clamped to
 *   0 .. W - 1 / 0 .. H - 1 (edge replicate; the kernel clamps unconditionally, whatever the map holds), and
 *     TPIV_DEWARP_LINEAR: out = (sum wy wx p + 32768) >> 16 over the taps (iy, iy + 1) x (ix, ix + 1), weights (256 - f, f);
 *     TPIV_DEWARP_CUBIC: out = clamp((sum Ty[a] Tx[b] p + (1 << 19)) >> 20, 0, 255) over the taps iy - 1 .. iy + 2, ix - 1 ..
 *       ix + 2, arithmetic shift, T = table_dev[f]: int16 [256, 4] in Q10, the Catmull-Rom weights (a = -0.5) of t = f / 256
 *       as floor(c * 1024 + 0.5) with the remainder to 1024 added to weight 1 (f < 128) or 2 (f >= 128)
 *       (torchpiv_amd.engine.dewarp_cubic_table; any table whose rows keep sum |w| <= 1280 stays inside int32).
 *   table_dev is read by TPIV_DEWARP_CUBIC only and may be NULL otherwise.
 * out_dev [n, H, W] must overlap neither the frames nor the map nor the table (a gather: never in place); the frames are
 * not written and no byte outside out_dev's n * H * W is.  TPIV_EINVAL for a null pointer, n < 0, H or W outside 1..2^22,
 * H * W >= 2^31, an unknown interp, fill outside 0..255, a map that is not 4-byte aligned, an overlap that can be seen
 * from the host; nothing is launched then.  n == 0 succeeds and launches nothing.  Enqueues only; allocates nothing. */
int tpiv_dewarp(const uint8_t* frames_dev, const long long* src_off_dev, int n, int H, int W, const int32_t* map_dev,
                const int16_t* table_dev, int interp, int fill, uint8_t* out_dev, void* stream);

/* ---- tile-wise adaptive histogram equalization (CLAHE) ----------------------------------------- */

/* Equalizes n frames frames_dev [n, H, W] uint8 into out_dev, in integer arithmetic (every implementation of these lines
 * gives the same bytes).  tile in 8..256; clip_q8 in 256..65536, the clip limit in 1/256 of the uniform bin height.
 *   Tile grid, per axis of n pixels: k = max(1, (2 n + tile) / (2 tile)) tiles with the edges e_i = (i n) / k, i = 0..k.
 *   Per tile with N pixels and the histogram h[256]: L = max(1, (clip_q8 N) >> 16) (64-bit product), E = sum max(h - L, 0),
 *   r = E % 256, h'[b] = min(h[b], L) + E / 256 + ((b + 1) r / 256 - b r / 256) (one redistribution, sum h' = N),
 *   C[b] = h'[0] + .. + h'[b], b0 = the lowest bin with h > 0, d = N - C[b0],
 *   lut[b] = (510 max(C[b] - C[b0], 0) + d) / (2 d), 0 for every b when d == 0: the darkest level of a tile maps to 0.
 *   Per pixel p of an axis, doubled coordinates: P = 2 p + 1, tile centres c_i = e_i + e_(i+1), i = the last i with
 *   c_i <= P clamped to 0..k-2, D = c_(i+1) - c_i, w1 = clamp(P - c_i, 0, D), w0 = D - w1 (k == 1: one tile, weight 1, D = 1).
 *   out = (2 s + Dy Dx) / (2 Dy Dx), s = the sum over the four neighbour tiles of wy wx lut_tile[g].
 * work_dev: at least tpiv_equalize_work_bytes(n, H, W, tile) bytes on the device; afterwards it starts with the tables,
 * uint8 [n, ky, kx, 256].  out_dev may be frames_dev itself (the map is pointwise once the tables exist); any other overlap
 * of out_dev with frames_dev, or of work_dev with either, is TPIV_EINVAL, like tile or clip_q8 out of range, a null
 * pointer, a workspace that is too small, n < 0, H or W outside 1..2^28: decided on the host, nothing is launched then.
 * n == 0 succeeds and launches nothing.  Enqueues two kernels; allocates nothing and never synchronises. */
size_t tpiv_equalize_work_bytes(int n, int H, int W, int tile);
int tpiv_equalize(const uint8_t* frames_dev, int n, int H, int W, int tile, int clip_q8, uint8_t* out_dev, void* work_dev,
                  size_t work_bytes, void* stream);

/* Host side of the ingest (no GPU involved): reads n_files files into dst + i * slot_bytes (page-locked staging memory
 * of the caller, at most slot_bytes each) with up to n_threads native reader threads -- what PIVDataset.__getitem__
 * (B:129-144) does file by file with np.fromfile, here for a whole batch without the interpreter in the loop.
 * sizes[i] = bytes read, or -1 when the file cannot be opened / read or does not fit the slot (the caller then takes
 * its per-file path, which skips an undecodable pair like B:138-139).  Returns TPIV_OK (per-file failures are not errors). */
int tpiv_read_files(const char* const* paths, int n_files, uint8_t* dst, size_t slot_bytes, int n_threads,
                    int64_t* sizes);

/* Read-ahead form of the same for a whole run (the loader of OfflinePIV.batched): the file list is handed over once;
 * n_threads reader threads fill the caller's n_bufs page-locked staging buffers batch after batch -- batch k (files
 * [k * files_per_batch, (k + 1) * files_per_batch), file j of it at bufs[k % n_bufs] + j * slot_bytes) -- running at most
 * n_bufs batches ahead of the consumer.  tpiv_reader_next blocks until the next batch is complete and gives its number
 * of files in *n_files (0: end of the list) with *buf_index and sizes[j] (bytes, or -1 as for tpiv_read_files);
 * tpiv_reader_release hands the OLDEST outstanding batch's buffer back for refilling (call it once the upload of that
 * buffer is through); tpiv_reader_close stops the threads (also mid-run) and frees the handle. */
typedef struct tpiv_reader tpiv_reader;
tpiv_reader* tpiv_reader_open(const char* const* paths, int64_t n_files, int files_per_batch, uint8_t* const* bufs,
                              int n_bufs, size_t slot_bytes, int n_threads);
int tpiv_reader_next(tpiv_reader* reader, int* n_files, int* buf_index, int64_t* sizes);
int tpiv_reader_release(tpiv_reader* reader);
void tpiv_reader_close(tpiv_reader* reader);

/* ---- measurement ------------------------------------------------------------------ */

/* Per-kernel timing with hipEvents recorded on the run's own stream (torch.cuda.Event only
 * sees torch's current stream).  While enabled, every tpiv_plan_run brackets each launch
 * with an event pair (no host synchronisation; up to 512 runs are kept).  Slots:
 * 0 = pass-1 tile kernel; for pass p >= 1: 2p-1 = predictor kernels, 2p = tile kernel. */
int tpiv_plan_set_timing(tpiv_plan* plan, int enable);
/* Waits for the recorded events, writes the MEAN duration in milliseconds of every slot over
 * the runs recorded since the last call into avg_ms[0..n_slots) and the number of runs into
 * n_runs, then clears the record.  n_slots must be 2*n_pass - 1. */
int tpiv_plan_get_timing(tpiv_plan* plan, double* avg_ms, int n_slots, int* n_runs);
/* TPIV_PREC_EXACT plans with an even first-pass window size from 8 to 128: the number of windows of the LAST tpiv_plan_run whose first pass
 * went through the float64 transform (undecided by the float32 locating pass).  Waits for the device.  TPIV_EINVAL for
 * other plans or before the first run.  (Diagnostics: bench.py reports the share.) */
int tpiv_plan_exact_fallbacks(tpiv_plan* plan, long long* n_windows);
/* The same plans: slot 0 of tpiv_plan_get_timing taken apart, as of the last call of
 * that function: ms4 = mean milliseconds of {float32 locating pass, exact refinement, float64 pass of the undecided
 * windows, finalize}. */
int tpiv_plan_exact_timing(const tpiv_plan* plan, double* ms4);

/* ---- test hook ------------------------------------------------------------------ */

/* Runs one pass like tpiv_pass1 (mode 0: float32, or the exact first pass when precision is
 * TPIV_PREC_EXACT) / tpiv_iter (mode DWS/CWS/CWS_Fast at `precision`; zero_dev = [batch, n_rows, n_cols]
 * float64 zeros) and additionally writes the staged windows win_dev
 * [batch, N, 2, ws, ws] float32 (frame a, frame b, after the shift) and the correlation maps
 * corr_dev [batch, N, ws, ws] float32 (corr - min + 1e-7, fftshift layout; odd window sizes write none).
 * DWS / CWS: u2_dev, v2_dev are the half shift as tpiv_iter takes it (DWS: integral values) and u0 = v0 = 0, so the
 * outputs are u = 2 u2 + du, v = 2 v2 + dv with the pass's raw displacement du, dv where the window is valid, and 0
 * where invalid_dev says it is not.  CWS_Fast: u2_dev, v2_dev are the predictor itself, passed as u0, v0 (the windows
 * are resampled by -/+ u0 / 2 inside themselves) and the outputs are tpiv_iter's, u = u0 + du unless masked.  Mode 0 with
 * TPIV_PREC_EXACT: the maps of the float32 locating kernel, the one whose decisions the exact
 * pass takes (also for the windows it then sends to the float64 transform).  Either may be NULL. */
int tpiv_debug_pass(int mode, int precision, const uint8_t* a_dev, const uint8_t* b_dev, int batch, int H, int W,
                    int ws, int ov, const double* u2_dev, const double* v2_dev, const double* zero_dev,
                    double* u_dev, double* v_dev, uint8_t* invalid_dev,
                    float* win_dev, float* corr_dev, void* work_dev, size_t work_bytes, void* stream);

/* tpiv_debug_pass of a spectrally filtered pass (tpiv_plan_set_correlation): mode 0, TPIV_MODE_DWS or TPIV_MODE_CWS at
 * ws = 16, 32 or 64 (anything else, TPIV_MODE_CWS_FAST included: TPIV_EUNSUPPORTED); tab_dev = g_y[0 .. ws/2] then
 * g_x[0 .. ws/2] on the device.  win_dev receives the staged windows (before the mean removal), corr_dev the map the
 * decisions are taken on, C - min + 1e-7 in fftshift layout. */
int tpiv_debug_pass_spec(int mode, int kind, double floor, const float* tab_dev, const uint8_t* a_dev, const uint8_t* b_dev,
                         int batch, int H, int W, int ws, int ov, const double* u2_dev, const double* v2_dev,
                         const double* zero_dev, double* u_dev, double* v_dev, uint8_t* invalid_dev, float* win_dev,
                         float* corr_dev, void* work_dev, size_t work_bytes, void* stream);

/* tpiv_debug_pass of a weighted pass (tpiv_plan_set_weighting): mode 0, TPIV_MODE_DWS or TPIV_MODE_CWS at ws = 16, 32 or 64
 * (anything else, TPIV_MODE_CWS_FAST included: TPIV_EUNSUPPORTED); tab_dev = g_y[0 .. ws-1] then g_x[0 .. ws-1] on the
 * device.  win_dev receives the staged windows (before step 2), corr_dev the map the decisions are taken on, C - min + 1e-7
 * in fftshift layout. */
int tpiv_debug_pass_weighted(int mode, const float* tab_dev, const uint8_t* a_dev, const uint8_t* b_dev, int batch, int H,
                             int W, int ws, int ov, const double* u2_dev, const double* v2_dev, const double* zero_dev,
                             double* u_dev, double* v_dev, uint8_t* invalid_dev, float* win_dev, float* corr_dev,
                             void* work_dev, size_t work_bytes, void* stream);

/* Runs one shifted pass (mode DWS or CWS) from the COMPACT predictor hand-off, exactly as tpiv_plan_run does after its
 * predictor: u_raw_dev, v_raw_dev [batch, n_rows, n_cols] float64 are the raw predictor (before the invalid-zeroing) and
 * mask_dev [batch, n_rows, n_cols] uint8 its thresholded mask (non-zero = the interpolated mask reached 0.5); the zeroing,
 * the halving and DWS's rint are formed by the kernels where they read them.  Everything else -- outputs, du_dev / dv_dev
 * (either may be NULL), work buffer -- is tpiv_iter's.  Lets the tests plant a predictor and compare the compact form with
 * the four fields of tpiv_iter bit for bit.  TPIV_EINVAL for CWS_Fast (which has no compact form) and for a NULL mask. */
int tpiv_debug_iter_compact(int mode, const uint8_t* a_dev, const uint8_t* b_dev, int batch, int H, int W,
                            int ws, int ov, const double* u_raw_dev, const double* v_raw_dev, const uint8_t* mask_dev,
                            double val_ratio, int val_win, int precision,
                            double* u_dev, double* v_dev, uint8_t* invalid_dev, double* du_dev, double* dv_dev,
                            void* work_dev, size_t work_bytes, void* stream);

/* Peak analysis alone -- correlation_to_displacement (B:360-422) + peak2peak_secondpeak
 * (B:346-358) -- on caller-supplied correlation maps [n_maps, ws, ws] float32 in fftshift layout
 * (ws = 8, 16, 32, 64 or 128): runs the kernels' peak stage and finalize on them.  planar != 0
 * selects the LDS layout of the three-wavefront tile kernels (64x64: the three-row map); planar = 2 with
 * ws = 8 the peak stage of the one-window-per-lane kernel; ignored for ws = 128.  The kernel subtracts the map minimum first (B:518), so feed maps whose minimum is
 * 0 to compare with the reference function.  work_dev: n_maps * 32 bytes. */
int tpiv_debug_peaks(const float* maps_dev, int n_maps, int ws, int planar, double val_ratio, int val_win,
                     double* u_dev, double* v_dev, uint8_t* invalid_dev,
                     void* work_dev, size_t work_bytes, void* stream);

/* Runs the plan's own (banded) predictor of pass `pass` (1 <= pass < n_pass) on caller-supplied
 * coarse fields, exactly as tpiv_plan_run does between passes; same outputs as tpiv_predict.
 * Lets the tests compare the banded operator with the dense one. */
int tpiv_plan_debug_predict(tpiv_plan* plan, int pass, int batch,
                            const double* u_c_dev, const double* v_c_dev, const uint8_t* invalid_c_dev,
                            double* u0_dev, double* v0_dev, double* u2_dev, double* v2_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TORCHPIV_HIP_H */
