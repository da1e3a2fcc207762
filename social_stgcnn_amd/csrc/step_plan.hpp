// The host-side plan of one model step (model_layout.hip): which kernels serve a batch, and where the buffers that the
// forward and the backward share keep their parts.  Entry points and size queries compute it once per call from
// (layout, N, V), plan_step, and nothing else decides a path or adds up an offset; beside it, the records of a call.
#pragma once
#include "model_common.hpp"

namespace stg {

struct TxpFwdArgs;
struct TxpBwdArgs;

// SceneX6: the exact-bf16 scene kernels in both passes (txp_x6.hip; one wave per scene or the team launch: team_wanted).
// WaveF32: a wave per scene with the round-1 fp32-MFMA kernels (txp_wave.hip) in at least one pass -- STG_OPT_F32_MFMA,
//   STG_OPT_SPLIT_BF16 (forward x6, backward two-piece bf16), the diagnostic STG_FWD_F32 / STG_BWD_F32.
// Workgroup: the workgroup-per-scene kernels of model_fwd.hip / model_bwd.hip, `wg_waves` waves per scene (0: by V).
struct StepPath {
    enum Kind { SceneX6, WaveF32, Workgroup } kind;
    int wg_waves;
    bool fwd_x6, bwd_x6;   // the exact-bf16 kernels fit this pass at (layout, V): they run it unless kind == Workgroup,
                           // and their prepared operands have room in the buffers whatever the kind
    bool scene() const { return kind != Workgroup; }
};

// Scratch of stg_model_fwd (offsets in floats; -1: not in use on this path):
//   agg     aggregated input of block 0, N x (cin + 1) T V -- inference only (training: straight into the workspace)
//   order   sorted scene list + tier offsets + sorted counts -- inference, and training on the Workgroup path
//   stamps  [N][16] 64-bit cycle stamps of the scene kernels (diagnostic build with STG_STAMPS=1)
//   wp_fwd  prepared forward operands of the exact-bf16 convs: written by the aggregation launch, read by the scene
//           launch behind it, when path.scene() && path.fwd_x6
struct FwdCarve {
    int64_t agg, order, stamps, wp_fwd, total;
};

// Batch tail of the training workspace, `base` floats behind its start: the N per-scene blocks (offsets in floats from
// ws + base; -1: not in use):
//   wp      prepared input-gradient operands of the exact-bf16 convs: written by the forward's aggregation launch, read
//           by the backward's scene launch, when path.scene() && path.bwd_x6
//   order   sorted scene list + tier offsets + sorted counts: written by the forward (aggregation launch or
//           scene_order_kernel), read by the backward, when tail_has_order() -- the backward takes it on trust, so both
//           passes must be given the same descriptor, N, V and num_peds
// `total` (stg_model_ws_tail_floats, ABI) reserves the operands wherever path.bwd_x6 holds, also on the Workgroup path
// that does not use them: the reservation is wider than the use.
struct WsTail {
    int64_t base, wp, order, total;
};
inline bool tail_has_order(const StepPath &path, const int32_t *num_peds, int N, int V) {
    return path.scene() && scene_order_applies(num_peds, N, V);
}

// the scene launch of a pass on a path with scene(): exact-bf16 or fp32-MFMA kernels as the path says
int launch_scene_fwd(const StepPath &path, const TxpFwdArgs &a, hipStream_t st);
int launch_scene_bwd(const StepPath &path, const TxpBwdArgs &a, hipStream_t st);

// The training step in one call (stg_model_step), StepPlan::one_launch: whether the forward and the backward scene
// kernels run as ONE launch (txp_x6.hip, txp_step_x6_kernel).  Exactly where both passes would run their solo kernels
// compiled for the canonical model and uniform scenes of 32 pedestrians (Shape::Canon32): the SceneX6 path with both
// passes on the exact-bf16 kernels, a canonical layout, V = 32 without num_peds, a batch large enough that no team launch
// is wanted -- and the caller has not asked for separate launches (STG_OPT_SEPARATE_FB), nor the diagnostic build for one
// of the solo kernels' timing switches (txp_step_x6_fits).  Everything the launch itself requires is decided here: where
// this holds the launch goes through, where it does not the step runs its two launches.
int launch_scene_step(const TxpFwdArgs &f, const TxpBwdArgs &b, hipStream_t st);

// The plan of one call: all of the above, computed ONCE per entry-point call or size query and handed to both passes.
// `sized` is N >= 0 && V > 0: without it only `lay` is filled in, and plan_sized refuses under the caller's name.
struct StepPlan {
    ModelLayout lay;
    bool sized, one_launch;
    StepPath path;
    int64_t ws_stride;               // ws_floats_per_scene
    WsTail tail;
    FwdCarve fwd;
};
int plan_step(const stg_model_desc *d, const int32_t *num_peds, int N, int V, StepPlan *p);   // STG_OK or make_layout's
// ... and N < min_N or V <= 0 refused as "<what> N=%d V=%d" (what: "stg_model_fwd: bad sizes", "stg_model_ws_tail_floats:")
int plan_sized(const char *what, const stg_model_desc *d, const int32_t *num_peds, int N, int V, int min_N, StepPlan *p);

// One call of the model step, as the C entry points fill it from their arguments: the batch (x with its four strides, A,
// the crowd sizes or null), the model, and what each pass reads and writes beside them.
struct SceneInput {
    const float *x; int64_t x_sn, x_sc, x_st, x_sv; const float *adj; int64_t a_sn; const int32_t *num_peds; int N, V;
};
struct ModelCall { const stg_model_desc *d; const float *params, *buffers; SceneInput in; void *stream; };
struct FwdBuffers { float *y, *ws, *stats, *scratch; void **events; int n_events; };
struct BwdBuffers {
    const float *dy, *nll_target, *nll_weights; float *nll_losses;   // dy: dV_pred, or with nll_target V_pred itself
    const stg_step_tail *tail;                                       // the step tail in the reduction launch, or null
    const float *ws; float *scratch, *grad_params, *dx; void **events; int n_events;
};

// The members that the device argument structs (FwdArgs, BwdArgs, TxpFwdArgs, TxpBwdArgs, WgradArgs) have in common with
// a call, by name: the crowd and the sizes in all five; the parameters and the batch in the four that have an `x`.
template <class A> constexpr auto has_batch(int) -> decltype(A::x, true) { return true; }
template <class A> constexpr bool has_batch(...) { return false; }
template <class A>
void set_input(A &a, const ModelCall &c) {
    const SceneInput &in = c.in;
    a.num_peds = in.num_peds; a.N = in.N; a.V = in.V;
    if constexpr (has_batch<A>(0)) {
        a.params = c.params; a.x = in.x; a.x_sn = in.x_sn; a.x_sc = in.x_sc; a.x_st = in.x_st; a.x_sv = in.x_sv;
        a.adj = in.adj; a.a_sn = in.a_sn;
    }
}

// the two passes behind the C entry points (model_fwd.hip, model_bwd.hip), given a plan with `sized`.  `defer` /
// `deferred`: the forward leaves its scene launch to the backward's (plan.one_launch holds), which runs both as one.
int model_fwd_impl(const ModelCall &c, const FwdBuffers &b, const StepPlan &p, TxpFwdArgs *defer);
int model_bwd_impl(const ModelCall &c, const BwdBuffers &b, const StepPlan &p, const TxpFwdArgs *deferred);

}  // namespace stg
