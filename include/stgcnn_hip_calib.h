/* stgcnn_hip_calib.h -- calibration of the predicted Gaussians, fit and apply: part of the C ABI of libstgcnn_hip.so,
 * included by stgcnn_hip.h (inside its extern "C" block; it relies on that header's types, limits and status codes) and
 * not meant to be included on its own.  The binding of these entry points is social_stgcnn_amd/_lib.py's
 * _SIGNATURES_CALIB; tests/test_calib_cpu.py holds the two copies against each other.                                */
#ifndef STGCNN_HIP_CALIB_H
#define STGCNN_HIP_CALIB_H
#ifndef STGCNN_HIP_H
#error "include stgcnn_hip.h, which includes this file"
#endif

/* N15  one positive factor g_t on the covariance of every predicted step t, fitted on held-out predictions and applied
 *      in front of every consumer of V_pred (added entry points, the ABI version stays).  The sampler
 *      draws the steps independently and sums them, so the factors change the absolute covariance at horizon h to
 *      C'_h = sum_{t<=h} g_t sig_t, sig_t = [sx^2, rho sx sy, sy^2]_t: a shift of 0.5 log g_t on the two log-sigma
 *      channels of V_pred at step t.  Means and correlations stay.
 *   stg_calib_fit.  Inputs as N14: v_pred (N,5,P,V) with strides, mean (N,P,V,2), truth (N,P,V,2) absolute, num_peds
 *     int32[N] or NULL (every scene holds V; values are clamped to 0 .. V).  float32, DEVICE memory.  An element is
 *     (n, v) with v < num_peds[n]; the elements are numbered in ascending (n, v).
 *     Per element, float32 as written (no fused multiply-add): sig_t from expf, expf, tanhf (the term N8 sums),
 *     off_h = mean_h - truth_h.  Horizons h = 1 .. P are fitted in ascending order: base_h = sum_{t<h} g_t sig_t
 *     (ascending t, multiply, then add), a candidate g gives C = base_h + g sig_h, and d2 is N8's value of off_h under C
 *     (determinant floored at 2^-15 cxx cyy).  ok(g) over all elements:
 *       STG_CALIB_MOMENT    sum d2 <= 2 count, the sum in float64: a wave's 64 elements by the xor butterfly 32 .. 1, the
 *                           four waves of a 256-element workgroup in ascending order, the workgroups in ascending order;
 *       STG_CALIB_COVERAGE  #(d2 <= thr) >= (double)level count, thr = (float)(-2 log1p(-(double)level)), float32 d2
 *                           against float32 thr.
 *     Round 0 tests 2^e, e = -10 .. 21, ascending: 2^-10 ok -> g_h = 2^-10, STG_CALIB_LOW; none ok -> g_h = 2^21,
 *     STG_CALIB_HIGH; otherwise hi = the first ok candidate, lo = its predecessor.  Three rounds refine: candidates
 *     lo + (hi - lo) (c 2^-5), c = 1 .. 31, and hi itself as c = 32; the first ok one is the new hi, its predecessor the
 *     new lo (the old lo for c = 1); then g_h = hi.  "First ok in ascending order" is the definition: nothing relies on
 *     d2 being monotone in g.  A horizon without elements: g_h = 1, STG_CALIB_EMPTY.
 *     Outputs (DEVICE): g float32[P]; bracket float32[P,2], the final (lo, hi) -- both g_h where a flag is set; flags
 *     int32[P]; stats float64[P,3] = {count, sum d2 at g_h, #(d2 <= thr) at g_h} (zeros where EMPTY); sig (N,P,V,3), the
 *     terms sig_t as computed (zeros where v >= num_peds[n]).
 *     ws: stg_calib_fit_ws_bytes(N, P, V) bytes of DEVICE scratch, 8-byte aligned; ws_bytes: what the caller holds.
 *     2 + 8 P launches of 256-thread workgroups over the live elements (not one workgroup per scene) and one-workgroup
 *     picks; no atomics, no cooperative launch, no host synchronisation, capturable, bitwise repeatable.
 *   stg_calib_apply: out[n,f,t,v] = v_pred[n,f,t,v] + (f == 2 || f == 3 ? shift[t] : 0), every V slot, one launch.
 *     shift float32[P] DEVICE, the caller's (float)(0.5 log((double)g_t)).  out NULL (or v_pred itself with the same
 *     strides): in place, only fields 2 and 3 are touched; else out has its own strides and receives all five fields.
 *   1 <= P <= STG_SCORE_MAX_P, 1 <= V <= STG_SCORE_MAX_V, N V <= 2^30: above a limit STG_EUNSUPPORTED.  Bad sizes, NULL
 *   required pointers, mean / truth / ws not 8-byte aligned, an unknown mode, a level outside (0, 1), ws_bytes below
 *   stg_calib_fit_ws_bytes, out == v_pred with other strides: STG_EINVAL; both decided before any launch.  N == 0 is
 *   a no-op that launches nothing: the caller sets g = 1 and STG_CALIB_EMPTY (ops.calib_fit does).
 *   stg_calib_fit_ws_bytes returns the size, or a negative status for sizes the fit refuses.                           */
#define STG_CALIB_MOMENT 0
#define STG_CALIB_COVERAGE 1
#define STG_CALIB_LOW 1   /* 2^-10 was already ok: g_h = 2^-10 */
#define STG_CALIB_HIGH 2  /* no candidate up to 2^21 was ok: g_h = 2^21 */
#define STG_CALIB_EMPTY 4 /* no element: g_h = 1 */
int64_t stg_calib_fit_ws_bytes(int N, int P, int V);
int stg_calib_fit(const float *v_pred, int64_t p_sn, int64_t p_sf, int64_t p_sp, int64_t p_sv, const float *mean,
                  const float *truth, const int32_t *num_peds, int N, int P, int V, int mode, float level, float *g,
                  float *bracket, int32_t *flags, double *stats, float *sig, void *ws, int64_t ws_bytes, void *stream);
int stg_calib_apply(const float *v_pred, int64_t p_sn, int64_t p_sf, int64_t p_sp, int64_t p_sv, const float *shift,
                    int N, int P, int V, float *out, int64_t o_sn, int64_t o_sf, int64_t o_sp, int64_t o_sv,
                    void *stream);

#endif /* STGCNN_HIP_CALIB_H */
