/*
 * stgcnn_hip.h -- C ABI of libstgcnn_hip.so: the MI355X (gfx950) Social-STGCNN hot path.
 *
 * The reference (GRatTWCU/Social-STGCNN) has no FFI: its hot path is Python on torch
 * (model.py, utils.py, metrics.py).  This library is what a binding for that path binds
 * (ctypes stub: social_stgcnn_amd/_lib.py).  Each entry point cites the
 * reference code it replaces (file:line under /root/reference).
 *
 * Conventions
 *  - plain pointers (DEVICE memory unless stated) and sizes; fp32 data, int32 counts.
 *  - every function returns 0 on success, a negative STG_E* code for invalid arguments, or a
 *    positive hipError_t; it never aborts, allocates nothing, does not synchronise the host,
 *    reads no environment variable and keeps no mutable global state (re-entrant across
 *    streams; the only per-thread state is the text behind stg_last_error()).  Every choice a
 *    caller can make -- kernel path, waves per scene, storage type -- is an explicit argument
 *    (stg_model_desc.flags / .wg_waves).  Work is enqueued on `stream` (a hipStream_t passed as
 *    void*; NULL = the default stream).
 *  - a batch holds N scene-windows padded to V pedestrian slots; `num_peds` (int32[N], may be
 *    NULL = all V valid) gives the real count V_i of each scene.  Slots >= V_i are ignored on
 *    input and written as zeros on output.
 *  - tensors are contiguous in the layouts named below unless explicit strides (in elements)
 *    are part of the signature.
 */
#ifndef STGCNN_HIP_H
#define STGCNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define STG_OK 0
#define STG_EINVAL (-1)      /* bad size / null pointer / inconsistent arguments          */
#define STG_EUNSUPPORTED (-2) /* configuration outside what the kernels are built for      */
#define STG_ELDS (-3)        /* scene too large for the 160 KiB LDS of one CU             */

#define STG_ABI_VERSION 8
#define STG_MAX_BLOCKS 4     /* st_gcn blocks in one fused model                          */

int stg_abi_version(void);
/* Human-readable description of the last error raised on the calling thread. */
const char *stg_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * R1/R2  utils.anorm + utils.seq_to_graph (utils.py:23-53) incl. networkx
 *        normalized_laplacian_matrix (call site utils.py:48-50).
 * rel:   relative displacements, element (n, v, c, t) at rel[n*rel_sn + v*rel_sv + c*rel_sc + t*rel_st]
 *        (the reference layout (V,2,T) is rel_sv=2T, rel_sc=T, rel_st=1).
 * nodes: out (N,T,V,2)  node features  V[s,h,:] = rel[h,:,s]            (may be NULL)
 * adj:   out (N,T,V,V)  A[s,h,k] = 1/||rel_h - rel_k|| (0 if equal), A[s,h,h] = 1;
 *        if normalize != 0 the symmetric normalised Laplacian D^-1/2 (D - A) D^-1/2.
 */
int stg_adj_build(const float *rel, int64_t rel_sn, int64_t rel_sv, int64_t rel_sc, int64_t rel_st,
                  const int32_t *num_peds, int N, int V, int T, int normalize,
                  float *nodes, float *adj, void *stream);

/* ---------------------------------------------------------------------------------------------
 * R3  the einsum of ConvTemporalGraphical.forward (model.py:67):
 *        y[n,c,t,w] = sum_v x[n,c,t,v] * A[n,t,v,w]         ('nctv,ntvw->nctw')
 * x (N,C,T,V) with strides; A (N,T,V,V) contiguous per scene with batch stride a_sn
 * (a_sn = 0 shares one (T,V,V) adjacency over the batch: the reference's 'nctv,tvw->nctw').
 * y (N,C,T,V) contiguous.  Backward: dx[n,c,t,v] = sum_w dy[n,c,t,w] * A[n,t,v,w] (A is data:
 * no dA).
 */
int stg_spatial_agg_fwd(const float *x, int64_t x_sn, int64_t x_sc, int64_t x_st, int64_t x_sv,
                        const float *adj, int64_t a_sn, const int32_t *num_peds,
                        int N, int C, int T, int V, float *y, void *stream);
int stg_spatial_agg_bwd(const float *dy, const float *adj, int64_t a_sn, const int32_t *num_peds,
                        int N, int C, int T, int V, float *dx, void *stream);

/* ---------------------------------------------------------------------------------------------
 * R3/R4  nn.Conv2d(Cin, Cout, (kt,1), padding=(pad,0)) as built at model.py:55-62 and
 *        model.py:116-122,135-139 (stride 1, dilation 1).
 * x (N,Cin,T,V) strided, w (Cout,Cin,kt,1), b (Cout) or NULL, y (N,Cout,To,V), To = T+2*pad-kt+1.
 * bwd: dx (N,Cin,T,V) (may be NULL), dw/db are ACCUMULATED into (+=) and must be zeroed by the
 * caller (db may be NULL).
 */
int stg_conv_t_fwd(const float *x, int64_t x_sn, int64_t x_sc, int64_t x_st, int64_t x_sv,
                   const float *w, const float *b, const int32_t *num_peds,
                   int N, int Cin, int Cout, int T, int V, int kt, int pad, float *y, void *stream);
int stg_conv_t_bwd(const float *x, int64_t x_sn, int64_t x_sc, int64_t x_st, int64_t x_sv,
                   const float *w, const float *dy, const int32_t *num_peds,
                   int N, int Cin, int Cout, int T, int V, int kt, int pad,
                   float *dx, float *dw, float *db, void *stream);

/* ---------------------------------------------------------------------------------------------
 * R4/R5  st_gcn.forward (model.py:145-155) and social_stgcnn.forward (model.py:182-198) as ONE
 *        scene-resident kernel per direction.
 *
 * Parameters live in one flat fp32 buffer in the reference's named_parameters() order
 * (st_gcns.j: gcn.conv.weight, gcn.conv.bias, tcn.0.{weight,bias}, tcn.1.weight,
 * tcn.2.{weight,bias}, tcn.3.{weight,bias}, [residual.0.{weight,bias}, residual.1.{weight,bias}],
 * prelu.weight; tpcnns.k.{weight,bias}; tpcnn_ouput.{weight,bias}; prelus.k.weight), BatchNorm
 * running statistics in a second flat buffer (per block: tcn.0 mean,var; tcn.3 mean,var;
 * [residual.1 mean,var]).  stg_model_param_count()/stg_model_buffer_count() give the sizes.
 */
typedef struct {
    int32_t n_stgcnn;      /* number of st_gcn blocks (model.py:163-166), 1..STG_MAX_BLOCKS      */
    int32_t n_txpcnn;      /* 0 = no TXP-CNN (stand-alone st_gcn module); else model.py:168-172 */
    int32_t c_in;          /* input_feat                                                        */
    int32_t c_out;         /* output_feat                                                       */
    int32_t t_obs;         /* seq_len                                                           */
    int32_t t_pred;        /* pred_seq_len                                                      */
    int32_t kt;            /* temporal kernel size (odd)                                        */
    int32_t residual0;     /* first block: 0 none (residual=False), 1 identity, 2 conv+BN       */
    int32_t use_mdn;       /* skip the block-final PReLU (model.py:152)                         */
    int32_t bn_mode;       /* 0 eval (running stats), 1 train with per-scene statistics (the     */
                           /* reference's N=1 training loop, train.py:36-77)                    */
    float bn_eps;          /* 1e-5                                                              */
    float bn_momentum;     /* 0.1                                                               */
    int32_t flags;         /* STG_OPT_* bit set, 0 = defaults.  Part of the descriptor because it decides  */
                           /* the workspace / scratch layouts the size queries report                      */
    int32_t wg_waves;      /* 0 = auto; 1, 2, 4 or 8: waves per scene of the workgroup-per-scene kernels   */
} stg_model_desc;

#define STG_OPT_WG_PATH 1     /* run the workgroup-per-scene kernels even where the wave-per-scene path fits */
#define STG_OPT_SPLIT_BF16 2  /* TXP input-gradient GEMMs on bf16 MFMAs with hi/lo-split operands (fp32 in/out) */
#define STG_OPT_BF16_STORE 8  /* bf16 STORAGE of what the forward saves for the backward and of the hand-offs between the  */
                              /* backward's kernels (TXP planes a_l, pre-activations z_l, dz_l): half the bytes; compute,    */
                              /* accumulation, parameters, inputs and V_pred stay fp32 (the forward result is unchanged).    */
                              /* Wave-per-scene path only (one st_gcn block, V <= 68).                                       */
#define STG_OPT_F32_MFMA 16   /* run the TXP convolutions and the weight-gradient GEMM on v_mfma_f32_16x16x4_f32 (the round-1 kernels)
                               * where the default uses v_mfma_f32_16x16x32_bf16 with exact three-piece operands (V <= 32, fp32
                               * storage): same accuracy class, for A/B measurements                                            */
#define STG_OPT_SEPARATE_FB 32 /* stg_model_step: run the forward and the backward scene kernels as two launches also where
                               * one launch serves both (same results bit for bit: A/B measurements and tests)           */
#define STG_OPT_GENERIC_WGRAD 64 /* keep the generic weight-gradient kernel also where the one compiled for the canonical model
                                 * with uniform scenes of 32 pedestrians serves the batch (same results bit for bit: A/B
                                 * measurements and tests)                                                              */
#define STG_OPT_WAVE_PATH 4   /* keep the wave-per-scene kernels for small batches too (default: batches of fewer than  */
                              /* 288 scenes of <= 40 pedestrians run the workgroup kernels, several waves per scene)     */

int64_t stg_model_param_count(const stg_model_desc *d);
int64_t stg_model_buffer_count(const stg_model_desc *d);
/* Per-scene activation workspace (floats) the forward writes for the backward when save != 0. */
int64_t stg_model_ws_floats(const stg_model_desc *d, int V);
/* floats of the BATCH tail of the training workspace, behind the N per-scene blocks: the forward leaves there what the
 * backward needs once per batch (the prepared bf16 operands of the input-gradient GEMMs, written by extra workgroups
 * of the forward's first launch; the scene order of a ragged batch, so that the backward does not sort again -- it
 * must be given the forward's num_peds).  ws holds N * stg_model_ws_floats + stg_model_ws_tail_floats floats.      */
int64_t stg_model_ws_tail_floats(const stg_model_desc *d, int N, int V);
/* Per-scene batch statistics the forward emits in bn_mode 1: (N, stat_floats) =
 * per block, per BatchNorm: mean[C], unbiased var[C].                                           */
int64_t stg_model_stat_floats(const stg_model_desc *d);
/* Scratch floats stg_model_fwd needs (hand-off between its block kernel and its TXP-CNN kernel; 0 when
 * one kernel does both). */
int64_t stg_model_fwd_scratch_floats(const stg_model_desc *d, int N, int V);
/* Scratch floats stg_model_bwd needs (partial-gradient slab rows of its kernels + the dz hand-off
 * between the input-gradient kernel and the weight-gradient kernel). */
int64_t stg_model_bwd_scratch_floats(const stg_model_desc *d, int N, int V);
/* Diagnostic build with STG_STAMPS=1: where in the forward's / the backward's scratch buffer (in floats) the scene
 * kernels leave their N x 16 64-bit time stamps.  STG_EUNSUPPORTED where none are written (every other build).  */
int64_t stg_model_fwd_stamps_offset(const stg_model_desc *d, int N, int V);
int64_t stg_model_bwd_stamps_offset(const stg_model_desc *d, int N, int V);

/* x (N,c_in,t_obs,V) strided; adj (N,t_obs,V,V), batch stride a_sn (0 = shared);
 * y: (N,c_out,t_pred,V) when n_txpcnn>0, else the block output (N,c_out,t_obs,V).
 * ws: N * stg_model_ws_floats + stg_model_ws_tail_floats floats (16-byte aligned) or NULL (inference).  stats: N * stg_model_stat_floats
 * or NULL.  scratch: stg_model_fwd_scratch_floats floats, 16-byte aligned (may be NULL when that is 0).     */
int stg_model_fwd(const stg_model_desc *d, const float *params, const float *buffers,
                  const float *x, int64_t x_sn, int64_t x_sc, int64_t x_st, int64_t x_sv,
                  const float *adj, int64_t a_sn, const int32_t *num_peds, int N, int V,
                  float *y, float *ws, float *stats, float *scratch, void **events, int n_events, void *stream);
/* events (may be NULL): n_events hipEvent_t handles for per-kernel device timing -- the entry point records
 * events[0] on `stream` before its first kernel and events[k] after its k-th kernel, as far as n_events reaches
 * (stg_model_fwd / stg_model_bwd kernel order: see DESIGN.md section 5).                                      */
/* dy like y.  grad_params (param_count) is OVERWRITTEN with the gradient summed over the batch;
 * dx (N,c_in,t_obs,V) may be NULL (the reference never needs it: x is data); a non-NULL dx needs STG_OPT_WG_PATH in
 * the descriptor of BOTH passes (STG_EUNSUPPORTED otherwise: the wave-per-scene kernels compute no input gradient).  scratch: stg_model_bwd_scratch_floats floats, 16-byte aligned
 * (ws must be 16-byte aligned too).                                                               */
int stg_model_bwd(const stg_model_desc *d, const float *params, const float *buffers,
                  const float *x, int64_t x_sn, int64_t x_sc, int64_t x_st, int64_t x_sv,
                  const float *adj, int64_t a_sn, const int32_t *num_peds, int N, int V,
                  const float *dy, const float *ws, float *scratch, float *grad_params, float *dx,
                  void **events, int n_events, void *stream);

/* stg_model_bwd fused with the loss (train.py:52-74: l = graph_loss(V_pred, V_tr); loss += l; loss.backward()): the
 * backward starts from V_pred itself -- y, the (N, 5, pred, V) output of stg_model_fwd -- and the (N, pred, V, 2)
 * target, computes d(sum_n weights[n] * loss_n)/dV_pred in its input stage (metrics.py:84-113, as stg_nll_fwd does)
 * and writes losses[n] = bivariate_loss of scene n.  weights may be NULL (all ones).  Served by the wave-per-scene
 * and the workgroup-per-scene kernels alike; STG_EUNSUPPORTED (nothing launched, no error message) with
 * STG_OPT_SPLIT_BF16 or without a TXP-CNN -- call stg_nll_fwd + stg_model_bwd then.  No input gradient.            */
int stg_model_bwd_nll(const stg_model_desc *d, const float *params, const float *buffers, const float *x, int64_t x_sn,
                      int64_t x_sc, int64_t x_st, int64_t x_sv, const float *adj, int64_t a_sn, const int32_t *num_peds,
                      int N, int V, const float *y, const float *target, const float *weights, float *losses,
                      const float *ws, float *scratch, float *grad_params, void **events, int n_events, void *stream);

/* The whole tail of a single-rank training step behind the fused loss + backward (train.py:58-76,197 + the
 * running-statistics updates of model.py:114,123,140 for the scenes just forwarded): stg_model_bwd_nll whose last launch
 * -- the fixed-order reduction of the partial gradients -- also applies SGD without clipping, p -= lr * grad (grad is
 * still written), folds the forward's per-scene BatchNorm statistics into the running ones (= stg_bn_fold) and writes
 * total[0] = sum_n weights[n] * losses[n] (= stg_weighted_sum), in extra workgroups of the same grid.  With
 * clip_grad_norm_ the update depends on the norm of the complete gradient: use stg_model_bwd_nll + stg_train_tail.   */
typedef struct stg_step_tail {
    float *params;          /* the flat parameters (the same buffer as `params`), updated in place               */
    const float *lr_dev;    /* learning rate in device memory (captured graphs follow StepLR), or NULL: use lr   */
    float lr;
    const float *stats;     /* per-scene batch statistics written by stg_model_fwd, or NULL: no fold             */
    float *buffers;         /* running statistics, updated in place                                              */
    int64_t *const *nbt;    /* num_batches_tracked counters (device pointers), n_bn of them, or NULL             */
    int n_bn;
    float *total;           /* out, 1 float, or NULL                                                             */
} stg_step_tail;
int stg_model_bwd_step(const stg_model_desc *d, const float *params, const float *buffers, const float *x, int64_t x_sn,
                       int64_t x_sc, int64_t x_st, int64_t x_sv, const float *adj, int64_t a_sn, const int32_t *num_peds,
                       int N, int V, const float *y, const float *target, const float *weights, float *losses,
                       const float *ws, float *scratch, float *grad_params, const stg_step_tail *tail, void **events,
                       int n_events, void *stream);
/* One single-rank training step without clipping in ONE call: stg_model_fwd (training: ws and stats as there) followed by
 * stg_model_bwd_step on its output, with the arguments of both -- y is written by the forward and read by the backward,
 * fwd_scratch / bwd_scratch are the two calls' scratch buffers, fwd_events / bwd_events their event lists.  Results
 * are those of the two calls bit for bit.  Where both passes run the scene kernels compiled for the canonical model on
 * uniform scenes of 32 pedestrians (one st_gcn block, five TXP layers, V = 32, num_peds NULL, a batch of more than 1024
 * scenes), the forward and the backward scene kernels are ONE launch: a wave runs the backward of its scene straight
 * behind the forward.  The step is then four launches, not five; bwd_events[1] closes the interval of that launch and
 * the forward scene kernel's own interval (fwd_events[1] .. fwd_events[2]) is empty.  STG_OPT_SEPARATE_FB in the
 * descriptor keeps the two launches; every other batch runs them as the two calls do.  STG_EUNSUPPORTED, nothing
 * launched, where stg_model_bwd_step is (STG_OPT_SPLIT_BF16, no TXP-CNN, N == 0).                                   */
int stg_model_step(const stg_model_desc *d, const float *params, const float *buffers, const float *x, int64_t x_sn,
                   int64_t x_sc, int64_t x_st, int64_t x_sv, const float *adj, int64_t a_sn, const int32_t *num_peds,
                   int N, int V, float *y, float *ws, float *stats, float *fwd_scratch, const float *target,
                   const float *weights, float *losses, float *bwd_scratch, float *grad_params,
                   const stg_step_tail *tail, void **fwd_events, int n_fwd_events, void **bwd_events,
                   int n_bwd_events, void *stream);
/* Sequential-fold update of the BatchNorm running statistics with the per-scene statistics of a
 * batch, exactly as N successive reference forwards would (momentum update per scene,
 * model.py:114,123,140; SURVEY 7 'BatchNorm semantics').  Scenes with num_peds[n] == 0 are skipped.
 * nbt: HOST array of n_bn DEVICE pointers to the int64 num_batches_tracked counters (may be NULL);
 * each is incremented by the number of non-empty scenes.                                          */
int stg_bn_fold(const stg_model_desc *d, const float *stats, const int32_t *num_peds, int N,
                float *buffers, int64_t *const *nbt, int n_bn, void *stream);

/* ---------------------------------------------------------------------------------------------
 * R6  metrics.bivariate_loss (metrics.py:84-113), batched: loss[n] = mean over (P, V_n) of
 *     -log(clamp(pdf, 1e-20)).  pred element (n,f,p,v) at pred[n*p_sn + f*p_sf + p*p_sp + v*p_sv]
 *     (f = mux,muy,log sx,log sy,atanh rho; the model output (N,5,P,V) is p_sf=P*V, p_sp=V, p_sv=1);
 *     target (N,P,V,2) contiguous.  grad (N,5,P,V) contiguous receives grad_scale[n] * d loss[n] / d pred
 *     (grad may be NULL; grad_scale float[N] may be NULL = 1: the caller's per-scene loss weights, so that
 *     grad is directly d(sum_n w_n loss_n)/d pred).
 */
int stg_nll_fwd(const float *pred, int64_t p_sn, int64_t p_sf, int64_t p_sp, int64_t p_sv,
                const float *target, const int32_t *num_peds, const float *grad_scale, int N, int P, int V,
                float *loss, float *grad, void *stream);
/* out[n,f,p,v] = grad[n,f,p,v] * gloss[n]  (chain rule with the upstream gradient of loss[n]). */
int stg_nll_bwd(const float *grad, const float *gloss, int N, int P, int V, float *out, void *stream);

/* N3  optim.SGD(lr) step without momentum / weight decay (train.py:197): p -= lr * g.          */
int stg_sgd_step(float *params, const float *grads, int64_t count, float lr, void *stream);

/* Ragged batches (the reference's DataLoader yields scenes of 2..57 pedestrians, utils.py:121-193): order[0..N) =
 * scene indices sorted by clamp(num_peds[n], 0, V) descending, stable.  stg_model_fwd / stg_model_bwd run this
 * themselves when num_peds is given (into their scratch buffers) and deal the sorted scenes to their persistent
 * waves boustrophedon, so a padded ragged batch is load-balanced; exported for callers that schedule their own
 * work the same way.  key_start (V+2 ints, may be NULL): key_start[k] = number of scenes with more than V-k
 * pedestrians, so the scenes with at most x pedestrians are order[key_start[V-x] .. N).
 * 2 <= N <= 65536, V <= 1023 (one workgroup, per-wave key histograms in LDS).                                                   */
int stg_scene_order(const int32_t *num_peds, int N, int V, int32_t *order, int32_t *key_start, void *stream);

/* N3  torch.nn.utils.clip_grad_norm_ (train.py:71-73) + optim.SGD step (train.py:197) + the StepLR-scheduled
 *     learning rate (train.py:200) over the flat parameter / gradient buffers in one launch:
 *       total = ||grads||_2;  if max_norm > 0: grads *= min(1, max_norm / (total + 1e-6)) (in place);
 *       params -= lr * grads.   lr is read from device memory when lr_dev != NULL (so that a captured hipGraph
 *     follows the schedule), else the host value `lr`.  grad_norm (1 float, may be NULL) receives `total`.
 *     count <= 2^22 (single-workgroup kernel; the model has 7,563 parameters).                              */
int stg_optim_step(float *params, float *grads, int64_t count, const float *lr_dev, float lr, float max_norm,
                   float *grad_norm, void *stream);

/* ---------------------------------------------------------------------------------------------
 * N1  TrajectoryDataset / DataLoader collation (utils.py:121-193, train.py:167-177) with the windowed dataset resident
 *     in HBM: seq_rel_all = ragged concatenation of every window's relative trajectories (total_peds, 2, T_obs+T_pred);
 *     win_start int32[n_windows+1] = pedestrian offsets of the windows; index int32[N] (DEVICE memory, NULL = windows
 *     0..N-1) = the windows of this batch.  Writes obs_rel (N,V,2,T_obs) -- the input of stg_adj_build --, target
 *     (N,T_pred,V,2) and num_peds (N), zero-padded to V slots (a window with more than V pedestrians is truncated:
 *     pad to the dataset's largest crowd).  No host synchronisation: the whole training step can be captured with the
 *     index refreshed in place.                                                                                     */
int stg_gather_windows(const float *seq_rel_all, const int32_t *win_start, const int32_t *index, int n_windows, int N,
                       int V, int T_obs, int T_pred, float *obs_rel, float *target, int32_t *num_peds, void *stream);

/* Data-parallel training over scene-windows (the reference has no multi-GPU path): ONE all-reduce(sum) per
 * optimizer step carries the flat gradient AND the exact sequential fold of the BatchNorm running statistics over the
 * ranks ("R ranks x B scenes == one rank on the concatenated batch").
 *   stg_dp_pack : pack = [ grads (n_params) | world slots of (n_buffers + 1) floats ]; the slot of `rank` receives
 *                 acc = bn_after - (1-momentum)^{n_r} * bn_before and n_r = the rank's non-empty scenes (num_peds[i] > 0;
 *                 num_peds NULL = N), every other slot 0.  bn_before / bn_after: the flat running statistics before /
 *                 after this rank's stg_bn_fold.  pack holds n_params + world * (n_buffers + 1) floats.
 *   (the caller all-reduces `pack` with SUM over the ranks: RCCL on MI355X)
 *   stg_dp_fold : buffers = bn_before * keep^{sum_r n_r} + sum_r acc_r * keep^{sum_{j>r} n_j}, keep = 1 - momentum;
 *                 the first n_params floats of `pack` are the summed gradient (feed them to stg_optim_step).
 *                 nbt (HOST array of n_bn DEVICE pointers to the int64 num_batches_tracked counters, may be NULL): each
 *                 counter, already advanced by this rank's own scenes (stg_bn_fold), also receives the scene counts of
 *                 the OTHER ranks from the pack -- afterwards every rank holds the single-process value.              */
int stg_dp_pack(const float *grads, const float *bn_before, const float *bn_after, const int32_t *num_peds, int N,
                float momentum, int rank, int world, int n_params, int n_buffers, float *pack, void *stream);
int stg_dp_fold(const float *pack, const float *bn_before, float momentum, int rank, int world, int n_params,
                int n_buffers, float *buffers, int64_t *const *nbt, int n_bn, void *stream);
/* out[0] = sum_n weights[n] * values[n] (weights NULL: plain sum), fixed summation order: the reported group loss of
 * train.train (train.py:58-67,76) from the per-scene losses of stg_nll_fwd.                                          */
int stg_weighted_sum(const float *values, const float *weights, int N, float *out, void *stream);

/* The tail of a single-rank training step in ONE launch (the three jobs do not depend on each other; they run in
 * different workgroups): the BatchNorm running-statistics fold of the forward just done (= stg_bn_fold; stats NULL
 * skips it), total[0] = sum_n weights[n] * losses[n] (= stg_weighted_sum; losses or total NULL skips it) and
 * clip_grad_norm_ + SGD on the flat parameters (= stg_optim_step).  Replaces train.py:58-76 + the per-forward
 * running-statistics updates of model.py:114,123,140 for one group of scenes.                                        */
int stg_train_tail(const stg_model_desc *d, const float *stats, const int32_t *num_peds, int N, float *buffers,
                   int64_t *const *nbt, int n_bn, const float *losses, const float *weights, float *total,
                   float *params, float *grads, int64_t count, const float *lr_dev, float lr, float max_norm,
                   float *grad_norm, void *stream);

/* ---------------------------------------------------------------------------------------------
 * N2  evaluation tail of test.test (test.py:59-123) + metrics.ade/fde/nodes_rel_to_nodes_abs
 *     (metrics.py:21-75): per pedestrian the best-of-K average / final displacement error of K trajectories
 *     sampled from the predicted bivariate Gaussians.  pred as in stg_nll_fwd; target_rel (N,P,V,2) ground-truth
 *     displacements; obs_last (N,V,2) last observed absolute position (may be NULL: the errors are translation
 *     invariant up to fp32 rounding); noise: K*N*P*V*2 standard normals laid out (K,N,P,V,2), or NULL to draw
 *     them in the kernel (Philox4x32-10 keyed by `seed`, counter = (scene*V + ped, k*P + t)).
 *     sample = mean + chol(cov) * eps, trajectory = cumsum_t(sample) + obs_last; ade/fde (N,V) receive
 *     min_k mean_t |traj - truth| and min_k |traj_P - truth_P| (0 for padded pedestrians).
 */
int stg_bestofk_eval(const float *pred, int64_t p_sn, int64_t p_sf, int64_t p_sp, int64_t p_sv,
                     const float *target_rel, const float *obs_last, const int32_t *num_peds, const float *noise,
                     uint64_t seed, int N, int P, int V, int K, float *ade, float *fde, void *stream);

/* ---------------------------------------------------------------------------------------------
 * N5  the sampled trajectories of test.test (test.py:59-91, raw_data_dict[step]['pred']) for a whole batch: the K
 *     draws of stg_bestofk_eval written out instead of reduced.  pred, obs_last, num_peds and noise as there (obs_last
 *     NULL: trajectories relative to the origin; noise NULL: the in-kernel Philox stream, counter
 *     (scene*V + ped, k*P + t) under the padded width V, keyed by `seed`, or by the device uint64 *seed_dev read at
 *     execution time when seed_dev is not NULL -- a captured graph then draws afresh after the caller updates it).
 *     samples (K,N,P,V,2) contiguous (the noise layout): obs_last + cumsum_t(mean_t + chol(cov_t) eps_{k,t}); may be
 *     NULL only when K == 0.  mean (N,P,V,2) or NULL: obs_last + cumsum_t(mean_t), the zero-noise trajectory.  Same
 *     draws and Cholesky arithmetic as stg_bestofk_eval: best-of-K over samples is its ade / fde for the same seed.
 *     Padded slots are zeros in both outputs; N == 0 is a no-op.  samples, mean, noise and obs_last must be 8-byte
 *     aligned (16-byte alignment and an even V select the two-pedestrians-per-lane float4 stores).
 */
int stg_sample_trajectories(const float *pred, int64_t p_sn, int64_t p_sf, int64_t p_sp, int64_t p_sv,
                            const float *obs_last, const int32_t *num_peds, const float *noise, uint64_t seed,
                            const uint64_t *seed_dev, int N, int P, int V, int K, float *samples, float *mean,
                            void *stream);

/* ---------------------------------------------------------------------------------------------
 * N6  per-frame prediction scenes from raw tracks: the reference's windowing (utils.py:123-165) without the future.
 *     At frame index f >= T_obs - 1 (frames = the recording's distinct frame numbers in ascending order, utils.py:123)
 *     the scene is every pedestrian id with a row in each of the frames f-T_obs+1 .. f, in ascending id order; the
 *     positions are rounded as np.around(x, d) (utils.py:145): rint(x * scale) / scale in float64, scale = 10^d
 *     (scale <= 0: no rounding).  Outputs are float64 obs_abs (., T_obs, V, 2) oldest frame first, int64 ids (., V)
 *     (-1 in padded slots) and int32 num_peds; padded slots are zeros.
 *
 *   Recording: rows sorted by (frame index, id) and uploaded once -- ids int64[M], xy float64 (M,2) -- with
 *   frame_start int32[F+1] (rows of frame f are frame_start[f] .. frame_start[f+1]-1; no duplicate id in a frame).
 *   stg_frame_scene_counts: count int32[F] = the scene size at every frame (0 for f < T_obs - 1).
 *   stg_frame_scenes: the scenes of the N frame indices frames int32[N] into obs_abs (N,T_obs,V,2), ids (N,V),
 *   num_peds (N); a scene larger than V keeps its V smallest ids (size V to the largest count).
 *
 *   Live stream: stg_track_push turns one frame of detections into that frame's scene (N = 1) with the track state on
 *   the device: slot_id int64[S] (-1 = free), mask uint32[S] (bit t = seen t frames ago), ring float64 (T_obs,S,2) of
 *   rounded positions, head_flags int32[2] = {ring row of the last frame, STG_TRACK_* flags of the last push}.  Zero
 *   mask / head_flags and slot_id = -1 start a new stream.  Inputs: det_id int64[M_max], det_xy float64 (M_max,2) and
 *   the detection count det_count int32[1], all DEVICE memory (a captured graph replays with another count).  A
 *   repeated id within a push: the first detection wins.  A new id takes a free slot -- one not seen in the last
 *   T_obs - 1 frames --, the i-th new detection (detection order) the i-th free slot (slot order); without a free slot
 *   it is dropped for this frame.  The scene keeps the V smallest ids.  M_max <= STG_TRACK_MAX_DETECTIONS,
 *   S <= STG_TRACK_MAX_SLOTS, T_obs <= 32.  One workgroup; no host synchronisation.
 */
#define STG_TRACK_MAX_DETECTIONS 2048
#define STG_TRACK_MAX_SLOTS 2048
#define STG_TRACK_DUPLICATE 1 /* a repeated id in the push (later detections dropped)                 */
#define STG_TRACK_OVERFLOW 2  /* no free slot for a new id (dropped for this frame)                   */
#define STG_TRACK_TRUNCATED 4 /* det_count > M_max (the first M_max detections used)                  */
#define STG_TRACK_TOO_MANY 8  /* more than V fully observed pedestrians (the V smallest ids kept)      */
int stg_frame_scene_counts(const int32_t *frame_start, const int64_t *ids, int F, int T_obs, int32_t *count,
                           void *stream);
int stg_frame_scenes(const int32_t *frame_start, const int64_t *ids, const double *xy, const int32_t *frames, int N,
                     int V, int T_obs, double scale, double *obs_abs, int64_t *out_ids, int32_t *num_peds,
                     void *stream);
int stg_track_push(const int64_t *det_id, const double *det_xy, const int32_t *det_count, int M_max, int64_t *slot_id,
                   uint32_t *mask, double *ring, int32_t *head_flags, int S, int T_obs, double scale, int V,
                   double *obs_abs, int64_t *out_ids, int32_t *num_peds, void *stream);

/* NS independent live streams in ONE launch, one workgroup per stream: stream b runs exactly stg_track_push on its own
 * state slices -- slot_id (NS,S), mask (NS,S), ring (NS,T_obs,S,2), head_flags (NS,2) -- and its own range of one
 * packed tick of detections, writing obs_abs (NS,T_obs,V,2), out_ids (NS,V), num_peds (NS) and out_flags (NS) (the
 * STG_TRACK_* flags of the push; may be NULL).  All DEVICE memory, read when the kernel runs, so one captured graph
 * serves every tick whatever its counts:
 *   det_id int64 and det_xy float64 hold M_total detections; detection j of the tick is det_id[j*id_stride],
 *   (det_xy[j*xy_stride], det_xy[j*xy_stride+1]) -- id_stride 1, xy_stride 2 is the contiguous (M_total), (M_total,2)
 *   layout; packed (id, x, y) records are id_stride = xy_stride = 3 (det_xy = the record's second element).
 *   det_start int32[NS+1]: stream b owns detections det_start[b] .. det_start[b+1]-1, clamped to [0, M_total); more than
 *   M_max of them: the first M_max, flag STG_TRACK_TRUNCATED.  pushed int32[NS]: 0 = stream b is not pushed this
 *   tick -- its state is left bit for bit as it was and its scene is empty (num_peds 0, ids -1, zero positions,
 *   out_flags 0).  A push with no detections is a push (it ages the tracks).
 * block_threads: 0 (the measured default), 64, 256 or 1024 -- the same results at every size.
 * Limits: NS <= STG_TRACK_MAX_STREAMS: 4096 streams are 8 rounds of the chip's concurrent push workgroups at the
 * largest block (512 on 256 CUs), their state at the 2048-slot limit stays inside int64 offsets and every per-stream
 * index in int32; more streams are better served by a second launch.  M_total <= STG_TRACK_MAX_TOTAL_DETECTIONS =
 * STG_TRACK_MAX_STREAMS * STG_TRACK_MAX_DETECTIONS (every stream at its own limit); det_start stays in int32.         */
#define STG_TRACK_MAX_STREAMS 4096
#define STG_TRACK_MAX_TOTAL_DETECTIONS (STG_TRACK_MAX_STREAMS * STG_TRACK_MAX_DETECTIONS)
int stg_track_push_streams(const int64_t *det_id, int64_t id_stride, const double *det_xy, int64_t xy_stride,
                           int M_total, const int32_t *det_start, const int32_t *pushed, int NS, int M_max,
                           int64_t *slot_id, uint32_t *mask, double *ring, int32_t *head_flags, int S, int T_obs,
                           double scale, int V, double *obs_abs, int64_t *out_ids, int32_t *num_peds,
                           int32_t *out_flags, int block_threads, void *stream);

/* Partially observed tracks: the N6 scenes for pedestrians with a short history or tracker gaps (added entry points).
 * A rule is (min_seen in [2, T_obs], max_gap in [0, T_obs - 2]).  The window of a frame has steps t = 0 .. T_obs-1,
 * oldest first, the last one the frame itself; frames before the first one count as missed.  An id is in the scene iff
 * it is seen at step T_obs-1, seen in at least min_seen steps, and every run of missed steps between two seen steps is
 * at most max_gap long (missed steps ahead of the first seen one are no gap).  min_seen = T_obs, max_gap = 0 is the
 * strict rule of N6.  Order, the V smallest ids, STG_TRACK_TOO_MANY and the lifetime of a slot are those of N6.
 *   Fill, in float64 with IEEE operations as written (no fused multiply-add), round = the rounding of N6:
 *     interior step t between the nearest seen steps a < t < b:  p[t] = round(p[a] + (p[b]-p[a]) * ((double)(t-a) / (double)(b-a)))
 *     leading step t < a0 (the first seen step), q = the window after the interior fill:
 *                                                              p[t] = round(q[a0] - (double)(a0-t) * (q[a0+1] - q[a0]))
 *   seen: int32 per scene slot, bit t set = observed t frames ago (bit 0 = this frame, the orientation of the state's
 *   masks), 0 in padded slots.
 * The fill on a batch in place: obs_abs (N,T_obs,V,2) float64, seen (N,V), num_peds int32[N] or NULL (all V columns); one
 * lane per (scene, pedestrian).  A column's seen steps are rounded and its missed steps filled; a column at or past
 * num_peds, with bit 0 clear or with fewer than two bits set is left untouched.  2 <= T_obs <= 32.
 * The two recording kernels and the two pushes of N6 under a rule take (min_seen, max_gap) after their sizes and write
 * seen (N,V) / (V) / (NS,V) beside their other outputs; every other argument is as in the strict entry point, which
 * keeps its own code.  The recording scenes start at frame index min_seen - 1.  The pushes read only the ring rows of
 * seen frames.                                                                                                        */
int stg_fill_tracks(double *obs_abs, const int32_t *seen, const int32_t *num_peds, int N, int T_obs, int V,
                    double scale, void *stream);
int stg_frame_scene_counts_rule(const int32_t *frame_start, const int64_t *ids, int F, int T_obs, int min_seen,
                                int max_gap, int32_t *count, void *stream);
int stg_frame_scenes_rule(const int32_t *frame_start, const int64_t *ids, const double *xy, const int32_t *frames,
                          int N, int V, int T_obs, double scale, int min_seen, int max_gap, double *obs_abs,
                          int64_t *out_ids, int32_t *num_peds, int32_t *seen, void *stream);
int stg_track_push_rule(const int64_t *det_id, const double *det_xy, const int32_t *det_count, int M_max,
                        int64_t *slot_id, uint32_t *mask, double *ring, int32_t *head_flags, int S, int T_obs,
                        double scale, int V, int min_seen, int max_gap, double *obs_abs, int64_t *out_ids,
                        int32_t *num_peds, int32_t *seen, void *stream);
int stg_track_push_streams_rule(const int64_t *det_id, int64_t id_stride, const double *det_xy, int64_t xy_stride,
                                int M_total, const int32_t *det_start, const int32_t *pushed, int NS, int M_max,
                                int64_t *slot_id, uint32_t *mask, double *ring, int32_t *head_flags, int S, int T_obs,
                                double scale, int V, int min_seen, int max_gap, double *obs_abs, int64_t *out_ids,
                                int32_t *num_peds, int32_t *out_flags, int32_t *seen, int block_threads,
                                void *stream);

/* Timestamped pushes at the tracker's own rate (added entry points, the ABI version stays).  Time is
 * integer ticks (int64: a frame number, microseconds, whatever the caller's clock counts; differences must not overflow)
 * and `step` the model's step in ticks.  A push carries its time det_time int64[1] in DEVICE memory, strictly greater
 * than the stream's last push (the first push takes any time); a push that is not changes no state but the flags word
 * head_flags[1] and returns the empty scene with STG_TRACK_TIME_ORDER.
 *   State: slot_id int64[S] (-1 = free); per slot the ring of its newest R samples, t_ring int64 (S,R) and xy_ring
 *   float64 (S,R,2) (rounded positions, ring order = time order, the oldest overwritten); slot_head int32 (S,2) = {next
 *   write index, samples held}; clock int64[2] = {time of the last accepted push, accepted pushes so far}; head_flags
 *   int32[2] = {unused, STG_TRACK_* flags of the last push}.  Zero slot_head / clock / head_flags and slot_id = -1 start
 *   a stream.  2 <= R <= STG_TRACK_MAX_HISTORY (above: STG_EUNSUPPORTED).
 *   Samples: a detection is recorded as (t_now, round(x), round(y)).  Duplicate ids, TRUNCATED, OVERFLOW, the order in
 *   which new ids take free slots, TOO_MANY and the V smallest ids are those of stg_track_push.  A slot is live while
 *   t_now - t_newest <= (T_obs-1) * step; it is freed, its ring emptied, at the start of the first push for which that
 *   fails (on a feed of one push per step: the lifetime of stg_track_push).
 *   Window: step k (oldest first) is the instant tau = t_now - (T_obs-1-k) * step.  It is observed iff the track has a
 *   sample at exactly tau -- that position is taken, no arithmetic is done -- or samples ta < tau < tb adjacent in its
 *   ring with tb - ta <= max_dt (1 <= max_dt <= (T_obs-1) * step): the position is then, per coordinate, in float64
 *   with IEEE operations as written,  round(pa + (pb - pa) * ((double)(tau - ta) / (double)(tb - ta))).
 *   step >= 1 and step * T_obs < 2^31 (above: STG_EUNSUPPORTED), so every difference is exact in a double.  The observed
 *   steps are the presence bits (`seen`: bit j = step T_obs-1-j); membership (min_seen, max_gap) and the fill of the
 *   missed steps, from observed steps that may themselves be interpolated, are those of the *_rule entry points.  Fed
 *   pushes at t = f * step with max_dt = step and R >= T_obs, the scenes, seen and flags are those of
 *   stg_track_push_rule bit for bit.
 * stg_track_push_streams_timed: one workgroup per stream on the (NS, ...) slices of all of the above, det_time int64[NS],
 * with det_start, pushed, out_flags and block_threads as stg_track_push_streams_rule takes them; a stream not pushed
 * keeps its state bit for bit, its clock included.  Bad sizes, rules, R, step, max_dt or NULL pointers are refused before
 * any launch.  No host synchronisation; everything is read when the kernel runs, so one captured graph serves every push
 * whatever its time and count.                                                                                        */
#define STG_TRACK_MAX_HISTORY 256
#define STG_TRACK_TIME_ORDER 16 /* the push's time is not after the stream's last push (nothing recorded)       */
int stg_track_push_timed(const int64_t *det_id, const double *det_xy, const int32_t *det_count,
                         const int64_t *det_time, int M_max, int64_t *slot_id, int64_t *t_ring, double *xy_ring,
                         int32_t *slot_head, int64_t *clock, int32_t *head_flags, int S, int R, int T_obs, double scale,
                         int V, int64_t step, int64_t max_dt, int min_seen, int max_gap, double *obs_abs,
                         int64_t *out_ids, int32_t *num_peds, int32_t *seen, void *stream);
int stg_track_push_streams_timed(const int64_t *det_id, int64_t id_stride, const double *det_xy, int64_t xy_stride,
                                 int M_total, const int32_t *det_start, const int32_t *pushed, const int64_t *det_time,
                                 int NS, int M_max, int64_t *slot_id, int64_t *t_ring, double *xy_ring,
                                 int32_t *slot_head, int64_t *clock, int32_t *head_flags, int S, int R, int T_obs,
                                 double scale, int V, int64_t step, int64_t max_dt, int min_seen, int max_gap,
                                 double *obs_abs, int64_t *out_ids, int32_t *num_peds, int32_t *out_flags,
                                 int32_t *seen, int block_threads, void *stream);

/* ---------------------------------------------------------------------------------------------
 * N7  what a caller acts on, reduced from the K samples of N5 without writing them out: conflict and zone-occupancy
 *     counts.  pred, strides, obs_last, num_peds (clamped to [0, V]), noise, seed and seed_dev exactly as in
 *     stg_sample_trajectories; with s[k,n,t,v] the position it would write for the same arguments and vi the scene's
 *     clamped count, every output is an int32 count over the K samples (integers only: bitwise repeatable).
 *
 *   Conflicts (radius > 0): hit[k,n,t,i,j] = i != j, both below vi, dx*dx + dy*dy < radius*radius in float32 (strict).
 *     conflict (N,P,V)   #k with any_j hit[k,n,t,i,j]
 *     conflict_any (N,V) #k with any_{t,j} hit
 *     pair (N,V,V)       #k with any_t hit[k,n,t,i,j]: symmetric, zero diagonal; may be NULL
 *     partner (N,V)      argmax_j pair[n,i,j], the smallest j on ties, -1 when the row is all zero (computed whether or
 *                        not pair is written)
 *   Zones (Z > 0): zones (N,Z,4) float32 [x0,y0,x1,y1] with scene stride z_sn floats (0: one set shared by every
 *   scene); a sample is inside when x0 <= x < x1 && y0 <= y < y1, by comparison only (an inverted rectangle is empty).
 *     zone_any (N,P,Z)   #k with some pedestrian below vi inside at step t
 *     zone_count (N,P,Z) sum over k of the number inside
 *     ped_zone (N,V,Z)   #k in which pedestrian v is inside at any step
 *   Padded slots are 0 (-1 in partner).  radius <= 0 skips the conflict outputs, Z == 0 the zone outputs (their
 *   pointers may then be NULL); both at once is STG_EINVAL, as are a NULL pred or required output, P, V or K below 1 and
 *   noise / obs_last that are not 8-byte aligned.  N == 0 is a no-op.  One workgroup per scene with the samples of a
 *   few k at a time in LDS; sizes above the STG_RISK_MAX_* limits are refused with STG_EUNSUPPORTED before any launch
 *   (every size inside them fits the 160 KiB of LDS).                                                                */
#define STG_RISK_MAX_V 256
#define STG_RISK_MAX_K 64
#define STG_RISK_MAX_Z 16
#define STG_RISK_MAX_P 32
int stg_sample_risk(const float *pred, int64_t p_sn, int64_t p_sf, int64_t p_sp, int64_t p_sv, const float *obs_last,
                    const int32_t *num_peds, const float *noise, uint64_t seed, const uint64_t *seed_dev, int N, int P,
                    int V, int K, float radius, const float *zones, int64_t z_sn, int Z, int32_t *conflict,
                    int32_t *conflict_any, int32_t *partner, int32_t *pair, int32_t *zone_any, int32_t *zone_count,
                    int32_t *ped_zone, void *stream);

/* ---------------------------------------------------------------------------------------------
 * N8  live predictions scored against the tracks that follow (added entry points, the ABI version
 *     stays).  Per stream, pushes numbered 0, 1, ... since the state was cleared.  Push m leaves a record in ring row
 *     m mod P: the scene's ids and num_peds (clamped to [0, V]), mean (P,V,2), the K samples (K,P,V,2) and the cumulative
 *     covariance C_h = sum_{t<=h} [sx^2, rho sx sy, sy^2]_t, sx = expf(v_pred[2]), sy = expf(v_pred[3]),
 *     rho = tanhf(v_pred[4]), summed in float32 in ascending t.  At push m the record of push m-h (h = 1..P, as far as
 *     pushes exist) is scored at its step h against the truth: the first detection of the pedestrian's id among the
 *     first min(count, M_max) detections of the push, rounded as N6 rounds (scale) and converted to float32 -- taken
 *     from the detections, whatever the track state did with them.  For a matched pedestrian v < num_peds, in float32
 *     as written (no fused multiply-add), dx, dy = mean_h - truth, (cxx, cxy, cyy) = C_h:
 *       err = sqrtf(dx*dx + dy*dy)          det = fmaxf(cxx*cyy - cxy*cxy, (cxx*cyy) * 2^-15)
 *       d2  = (cyy*(dx*dx) - 2*cxy*dx*dy + cxx*(dy*dy)) / det
 *       nll = 0.5*d2 + 0.5*log(det) + log(2 pi)   (log(det): the correctly rounded float32 logarithm)
 *       best = min_k |samples[k,h] - truth|;   acc[k] += |samples[k,h] - truth|, acc_mean += err, steps += 1
 *     Order within a push: score the pending records, retire the one that turns P pushes old, then write this push's
 *     record into the retired row and zero its accumulators.
 *
 *   State (stg_score_state, NS leading, all DEVICE memory; zero head and totals start a stream):
 *     rec_ids int64 (NS,P,V), rec_peds int32 (NS,P), rec_mean (NS,P,P,V,2), rec_cov (NS,P,P,V,3),
 *     rec_samples (NS,P,K,P,V,2), acc (NS,P,K,V), acc_mean (NS,P,V) float32, steps int32 (NS,P,V),
 *     head int32 (NS,2) = {ring row of the next push, records that exist (<= P)},
 *     totals float64 (NS,P,5+Q) = per horizon {matched, sum err, sum d2, sum nll, sum best, #(d2 <= thr_q) for q < Q},
 *     traj_totals float64 (NS,5) = {trajectories with steps == P, the sums of their traj_ade, traj_fde, traj_ade_mean,
 *     traj_fde_mean}.  Each workgroup owns its stream's totals and sums them in a fixed order (no atomics).
 *     P*V*(8 + 20P + 8KP + 4K + 8) bytes per stream beside the totals.
 *   Outputs (stg_score_out, NS leading): rec_ids int64 (NS,P,V) (row h-1: the id where matched, else -1), matched int32,
 *     err, d2, nll, best float32 (NS,P,V); from the retired record traj_steps int32 (NS,V), traj_ade = min_k acc[k] /
 *     steps, traj_fde = best at h = P (0 if unmatched there), traj_ade_mean = acc_mean / steps, traj_fde_mean = err at
 *     h = P, float32 (NS,V).  Unmatched, padded and not yet existing entries are 0.  With traj_steps == P, traj_ade /
 *     traj_fde are the reference's per-pedestrian best-of-K ADE / FDE (test.py:93-123).
 *   Inputs: the prediction as the chain leaves it -- mean (NS,P,V,2), v_pred (NS,5,P,V) with its strides as in N5,
 *     samples (K,NS,P,V,2) or NULL, ids int64 (NS,V), num_peds int32 (NS) -- and thr float32[Q].  NULL samples or K == 0
 *     skips every sample-based value: rec_samples, acc, best, traj_ade and traj_fde may then be NULL.
 *   stg_score_push: one stream (NS = 1), det_id / det_xy / det_count as stg_track_push reads them.
 *   stg_score_push_streams: det_id / det_xy with strides, M_total, det_start and pushed as stg_track_push_streams reads
 *     them (the same clamping and M_max truncation); a stream not pushed keeps its state bit for bit and gets all-zero
 *     outputs (ids -1).  NS == 0 is a no-op.
 *   One workgroup per stream, 12 bytes of LDS per detection slot (24 KB at the limit), plain stores, no host
 *   synchronisation.  Sizes above STG_SCORE_MAX_* or the STG_TRACK_MAX_* limits: STG_EUNSUPPORTED; bad sizes, NULL
 *   required pointers or mean / samples not 8-byte aligned: STG_EINVAL; both decided before any launch.             */
#define STG_SCORE_MAX_V 256
#define STG_SCORE_MAX_K 64
#define STG_SCORE_MAX_P 32
#define STG_SCORE_MAX_Q 4
typedef struct stg_score_state {
    int64_t *rec_ids;
    int32_t *rec_peds;
    float *rec_mean, *rec_cov, *rec_samples, *acc, *acc_mean;
    int32_t *steps, *head;
    double *totals, *traj_totals;
} stg_score_state;
typedef struct stg_score_out {
    int64_t *rec_ids;
    int32_t *matched;
    float *err, *d2, *nll, *best;
    int32_t *traj_steps;
    float *traj_ade, *traj_fde, *traj_ade_mean, *traj_fde_mean;
} stg_score_out;
int stg_score_push(const int64_t *det_id, const double *det_xy, const int32_t *det_count, int M_max, double scale,
                   const float *mean, const float *v_pred, int64_t p_sn, int64_t p_sf, int64_t p_sp, int64_t p_sv,
                   const float *samples, const int64_t *ids, const int32_t *num_peds, int P, int V, int K,
                   const stg_score_state *state, const float *thr, int Q, const stg_score_out *out, void *stream);
int stg_score_push_streams(const int64_t *det_id, int64_t id_stride, const double *det_xy, int64_t xy_stride,
                           int M_total, const int32_t *det_start, const int32_t *pushed, int NS, int M_max,
                           double scale, const float *mean, const float *v_pred, int64_t p_sn, int64_t p_sf,
                           int64_t p_sp, int64_t p_sv, const float *samples, const int64_t *ids,
                           const int32_t *num_peds, int P, int V, int K, const stg_score_state *state,
                           const float *thr, int Q, const stg_score_out *out, void *stream);

/* Timed predictions scored by TIME (added entry points, the ABI version stays): the structs, limits and
 * the two entry points are declared in stgcnn_hip_score_time.h, included at the end of this header.                  */

/* ---------------------------------------------------------------------------------------------
 * N9  unlabelled detections -> track ids, the front end of the live pushes (added entry points, the ABI
 *     version stays).  A per-stream tracker with constant-velocity prediction and gated, globally greedy
 *     nearest-neighbour matching; exact and deterministic.
 *   State (all DEVICE memory; zeros and trk_id = -1 start a stream): C track slots -- trk_id int64[C] (-1 = free),
 *     trk_pos float64 (C,2) the last matched rounded position, trk_vel float64 (C,2) displacement per push, trk_miss
 *     int32[C] pushes since the last match, trk_hits int32[C] matches so far (>= 1 for a live track) --, next_id
 *     int64[1] and assoc_flags int32[1], the STG_ASSOC_* flags of the last push.
 *   One push with m = min(count, M_max) detections at p_j = round(xy_j) (the rounding of N6, scale), float64 with one
 *   IEEE operation at a time (no fused multiply-add):
 *     1. every live slot s predicts q_s = pos_s + vel_s * (double)(miss_s + 1);
 *     2. cost(s,j) = dx*dx + dy*dy, dx = q_s.x - p_j.x, dy = q_s.y - p_j.y; the pair is a candidate iff cost <= g2_s,
 *        g2_s = gate2 when hits_s >= 2 (the track has a velocity), gate_new2 when hits_s == 1;
 *     3. the candidates are taken in ascending order of (cost, s, j), each accepted when its track and its detection
 *        are both still free;
 *     4. a matched pair: id_j = trk_id_s, vel_s = (p_j - pos_s) / (double)(miss_s + 1), pos_s = p_j, miss_s = 0,
 *        hits_s += 1;
 *     5. a live slot not matched: miss_s += 1; once miss_s > max_miss the slot is freed (trk_id -1, the rest zero);
 *     6. the detections not matched, in detection order: the i-th gets id next_id + i and the i-th free slot in slot
 *        order (the slots freed in 5 included) with pos = p_j, vel = 0, miss = 0, hits = 1; when the free slots run
 *        out the others still get their ids, no slot, and STG_ASSOC_FULL is set; next_id advances by their number.
 *   The ids are written to det_id[j * id_stride], j < m: the array the push and score launches behind it read.
 *   Detections past M_max are not touched (the push drops them, STG_TRACK_TRUNCATED).  Ids are >= 0 and distinct within
 *   a push.  gate2 and gate_new2 are the SQUARED gates: finite, gate2 > 0, gate_new2 >= gate2; max_miss >= 0.
 *   stg_associate: one workgroup; det_xy float64 (M_max,2), det_count int32[1], det_id int64[M_max].
 *   stg_associate_streams: one workgroup per stream on the (NS, ...) slices of the state, det_id / det_xy with strides,
 *     M_total, det_start and pushed as stg_track_push_streams reads them; a stream not pushed keeps its state bit for
 *     bit and its ids are not written.
 *   LDS: 28 bytes per track slot and 20 per detection, 98,304 bytes at both limits.  Sizes above STG_ASSOC_MAX_*:
 *   STG_EUNSUPPORTED; bad sizes, gates, max_miss or NULL pointers: STG_EINVAL; both decided before any launch.  Every
 *   count, range and state word is read when the kernel runs, so one captured graph serves every push.  No host
 *   synchronisation.                                                                                                 */
#define STG_ASSOC_MAX_SLOTS STG_TRACK_MAX_SLOTS
#define STG_ASSOC_MAX_DETECTIONS STG_TRACK_MAX_DETECTIONS
#define STG_ASSOC_FULL 1 /* no free slot for a new track (the detection has its fresh id, nothing is remembered) */
int stg_associate(int64_t *det_id, const double *det_xy, const int32_t *det_count, int M_max, int64_t *trk_id,
                  double *trk_pos, double *trk_vel, int32_t *trk_miss, int32_t *trk_hits, int64_t *next_id,
                  int32_t *assoc_flags, int C, double scale, double gate2, double gate_new2, int max_miss,
                  void *stream);
int stg_associate_streams(int64_t *det_id, int64_t id_stride, const double *det_xy, int64_t xy_stride, int M_total,
                          const int32_t *det_start, const int32_t *pushed, int NS, int M_max, int64_t *trk_id,
                          double *trk_pos, double *trk_vel, int32_t *trk_miss, int32_t *trk_hits, int64_t *next_id,
                          int32_t *assoc_flags, int C, double scale, double gate2, double gate_new2, int max_miss,
                          void *stream);

/* Self-test helper: C(16x16) = A(16xK) * B(Kx16) through v_mfma_f32_16x16x4_f32 with the operand
 * maps the TXP-CNN kernels rely on (K multiple of 4).                                           */
int stg_selftest_mfma(const float *a, const float *b, int K, float *c, void *stream);

/* N8 continued: the time-indexed score (inside the extern "C" block above) */
#include "stgcnn_hip_score_time.h"

/* N10: training windows harvested from the live tracks (added entry points, the ABI version stays),
 * declared in stgcnn_hip_harvest.h like the timed score above */
#include "stgcnn_hip_harvest.h"

/* N11: ... from timestamped pushes, the tracks resampled on the model's step grid (added entry points,
 * the ABI version stays), declared in stgcnn_hip_harvest_time.h the same way */
#include "stgcnn_hip_harvest_time.h"

/* N12: N9 on timestamped pushes, ahead of the timed push (added entry points, the ABI version stays),
 * declared in stgcnn_hip_assoc_time.h the same way */
#include "stgcnn_hip_assoc_time.h"

/* N13: N12 with a filtered track state and a gate that follows the predicted uncertainty (added entry
 * points, the ABI version stays), declared in stgcnn_hip_assoc_filter.h the same way */
#include "stgcnn_hip_assoc_filter.h"

/* N14: distribution metrics of a batch of predictions against the truth, beside stg_bestofk_eval (an
 * added entry point, the ABI version stays), declared in stgcnn_hip_metrics.h the same way */
#include "stgcnn_hip_metrics.h"

/* N15: calibration of the predicted Gaussians, fit and apply (added entry points, the ABI version
 * stays), declared in stgcnn_hip_calib.h the same way */
#include "stgcnn_hip_calib.h"

#ifdef __cplusplus
}
#endif
#endif /* STGCNN_HIP_H */
