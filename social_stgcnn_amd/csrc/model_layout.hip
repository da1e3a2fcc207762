// Host-side layout arithmetic for the fused model kernels + the public size queries.
#include <cstring>
#include <type_traits>
#include "model_common.hpp"
#include "scene_order.hpp"
#include "step_plan.hpp"
#include "txp_wave.hpp"

namespace stg {

int make_layout(const stg_model_desc *d, ModelLayout *lay) {
    STG_REQUIRE(d && lay, STG_EINVAL, "model descriptor is null");
    STG_REQUIRE(d->n_stgcnn >= 1 && d->n_stgcnn <= STG_MAX_BLOCKS, STG_EUNSUPPORTED,
                "n_stgcnn=%d outside 1..%d", d->n_stgcnn, STG_MAX_BLOCKS);
    STG_REQUIRE(d->n_txpcnn >= 0 && d->n_txpcnn <= kMaxTxp, STG_EUNSUPPORTED, "n_txpcnn=%d outside 0..%d",
                d->n_txpcnn, kMaxTxp);
    STG_REQUIRE(d->c_out == Cfg::C && d->t_obs == Cfg::T && d->kt == Cfg::KT, STG_EUNSUPPORTED,
                "fused kernels are built for output_feat=%d seq_len=%d kernel_size=%d (got %d,%d,%d)", Cfg::C,
                Cfg::T, Cfg::KT, d->c_out, d->t_obs, d->kt);
    STG_REQUIRE(d->c_in == Cfg::CIN0 || d->c_in == Cfg::C, STG_EUNSUPPORTED,
                "fused kernels are built for input_feat %d or %d (got %d)", Cfg::CIN0, Cfg::C, d->c_in);
    STG_REQUIRE(d->n_txpcnn == 0 || d->t_pred == Cfg::P, STG_EUNSUPPORTED,
                "fused kernels are built for pred_seq_len=%d (got %d)", Cfg::P, d->t_pred);
    STG_REQUIRE(d->bn_mode == 0 || d->bn_mode == 1, STG_EINVAL, "bn_mode=%d (0 eval, 1 per-scene train)", d->bn_mode);
    STG_REQUIRE(d->residual0 >= 0 && d->residual0 <= 2, STG_EINVAL, "residual0=%d", d->residual0);
    STG_REQUIRE(d->residual0 != 1 || d->c_in == d->c_out, STG_EINVAL, "identity residual needs c_in == c_out");
    STG_REQUIRE((d->flags & ~(STG_OPT_WG_PATH | STG_OPT_SPLIT_BF16 | STG_OPT_WAVE_PATH | STG_OPT_BF16_STORE | STG_OPT_F32_MFMA |
                              STG_OPT_SEPARATE_FB | STG_OPT_GENERIC_WGRAD)) == 0, STG_EINVAL,
                "unknown flags 0x%x", d->flags);
    STG_REQUIRE(d->wg_waves == 0 || d->wg_waves == 1 || d->wg_waves == 2 || d->wg_waves == 4 || d->wg_waves == 8,
                STG_EINVAL, "wg_waves=%d (0 auto, 1, 2, 4, 8)", d->wg_waves);
    ModelLayout &l = *lay;
    l = layout_of(ModelShape{d->n_stgcnn, d->n_txpcnn, d->c_in, d->residual0, d->use_mdn});
    l.bn_mode = d->bn_mode;
    l.eps = d->bn_eps;
    l.momentum = d->bn_momentum;
    l.flags = d->flags;
    l.wg_waves = d->wg_waves;
    return STG_OK;
}

bool is_canonical(const ModelLayout &L) {
    ModelLayout c = L;
    c.eps = kCanonLayout.eps;
    c.momentum = kCanonLayout.momentum;
    c.bn_mode = kCanonLayout.bn_mode;
    c.flags = kCanonLayout.flags;
    c.wg_waves = kCanonLayout.wg_waves;
    static_assert(std::is_trivially_copyable<ModelLayout>::value && sizeof(ModelLayout) % 4 == 0, "compared bytewise");
    return std::memcmp(&c, &kCanonLayout, sizeof c) == 0;
}

// ---- the plan of a model step (step_plan.hpp) ------------------------------------------------------------------
// A small batch of small scenes (fewer scenes than resident wave slots: every scene's latency chain is the step) runs
// the workgroup-per-scene kernels with several waves per scene instead of the fp32-MFMA wave kernels (measured: N = 512
// x 4 waves 2.9 vs 2.5 M scene-windows/s, N = 128 x 8 waves 0.95 vs 0.70).  The exact-bf16 kernels cut the scenes of a
// small batch into finer teams themselves (team_geom) and keep every batch they fit.
constexpr int kSmallBatch = 288;      // measured: 256 scenes 1.89 (workgroup kernels) vs 1.79 M/s (a wave per scene), 320 scenes 2.10 vs 2.19

static StepPath choose_path(const ModelLayout &L, int N, int V) {
    StepPath p{StepPath::Workgroup, L.wg_waves, txp_fwd_x6_fits(L, V), txp_bwd_x6_fits(L, V)};
    // a wave (or a team of waves) per scene: the whole model with one st_gcn block on the two input features
    if (L.n_txp < 1 || L.n_blocks != 1 || L.blk[0].cin != Cfg::CIN0 || (L.flags & STG_OPT_WG_PATH)) return p;
    if (p.fwd_x6 && p.bwd_x6) {
        p.kind = StepPath::SceneX6;
    } else if (txp_wave_f32_fits(V)) {
        if (N >= kSmallBatch || L.wg_waves != 0 || V > 40 || (L.flags & (STG_OPT_WAVE_PATH | STG_OPT_BF16_STORE)))
            p.kind = StepPath::WaveF32;
        else
            p.wg_waves = N <= 192 ? 8 : 4;     // 2048 resident wave slots / N scenes, at most the 8 waves a scene's tiles can use
    }
    return p;
}

static FwdCarve fwd_carve(const ModelLayout &L, const StepPath &path, int N, int V) {
    const bool stamps = diag_env("STG_STAMPS", 0) != 0;
    FwdCarve c;
    c.agg = 0;
    c.order = (((int64_t)N * (L.blk[0].cin + 1) * Cfg::T * V + 3) & ~(int64_t)3) + 4;
    c.stamps = stamps ? c.order + order_floats(N, V) : -1;
    const int64_t wp = (c.order + order_floats(N, V) + (stamps ? (int64_t)N * 32 : 0) + 3) & ~(int64_t)3;   // (16-byte vectors)
    c.wp_fwd = path.scene() && path.fwd_x6 ? wp : -1;
    c.total = wp + (path.fwd_x6 ? txp_bwd_x6_wp_floats(L) : 0);
    return c;
}

static WsTail ws_tail(const ModelLayout &L, const StepPath &path, int N, int V) {
    WsTail t;
    t.base = (int64_t)N * ws_floats_per_scene(L, V);
    t.wp = path.scene() && path.bwd_x6 ? 0 : -1;
    t.order = path.bwd_x6 ? txp_bwd_x6_wp_floats(L) : 0;
    t.total = t.order + order_floats(N, V);
    return t;
}

int launch_scene_fwd(const StepPath &path, const TxpFwdArgs &a, hipStream_t st) {
    return path.fwd_x6 ? launch_txp_fwd_x6(a, st) : launch_txp_fwd_wave(a, st);
}
int launch_scene_bwd(const StepPath &path, const TxpBwdArgs &a, hipStream_t st) {
    return path.bwd_x6 ? launch_txp_bwd_x6(a, st) : launch_txp_bwd_wave(a, st);
}

static bool step_one_launch(const ModelLayout &L, const StepPath &path, const int32_t *num_peds, int N, int V) {
    return path.kind == StepPath::SceneX6 && path.fwd_x6 && path.bwd_x6 && !(L.flags & STG_OPT_SEPARATE_FB) &&
           txp_step_x6_fits(L, num_peds, N, V);
}
int launch_scene_step(const TxpFwdArgs &f, const TxpBwdArgs &b, hipStream_t st) { return launch_txp_step_x6(f, b, st); }

int plan_step(const stg_model_desc *d, const int32_t *num_peds, int N, int V, StepPlan *p) {
    const int rc = make_layout(d, &p->lay);
    p->sized = rc == STG_OK && N >= 0 && V > 0;
    if (!p->sized) return rc;
    const ModelLayout &L = p->lay;
    p->path = choose_path(L, N, V);
    p->ws_stride = ws_floats_per_scene(L, V);
    p->tail = ws_tail(L, p->path, N, V);
    p->fwd = fwd_carve(L, p->path, N, V);
    p->one_launch = step_one_launch(L, p->path, num_peds, N, V);
    return STG_OK;
}
int plan_sized(const char *what, const stg_model_desc *d, const int32_t *num_peds, int N, int V, int min_N, StepPlan *p) {
    const int rc = plan_step(d, num_peds, N, V, p);
    if (rc != STG_OK) return rc;
    STG_REQUIRE(p->sized && N >= min_N, STG_EINVAL, "%s N=%d V=%d", what, N, V);
    return STG_OK;
}

__global__ __launch_bounds__(1024) void scene_order_kernel(const int32_t *__restrict__ num_peds, int N, int V,
                                                           int32_t *__restrict__ order,
                                                           int32_t *__restrict__ key_start,
                                                           int32_t *__restrict__ order_peds) {
    extern __shared__ int hist[];      // [K][16]
    __shared__ int wave_tot[16];
    scene_order_body<16>(num_peds, N, V, order, key_start, order_peds, hist, wave_tot);
}

bool launch_scene_order(const int32_t *num_peds, int N, int V, const SceneOrder &o, hipStream_t st) {
    if (!o.order || !scene_order_applies(num_peds, N, V)) return false;
    const size_t lds = (size_t)(V + 1) * 16 * sizeof(int);
    if (lds > 48 * 1024 &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(&scene_order_kernel),
                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return false;
    hipLaunchKernelGGL(scene_order_kernel, dim3(1), dim3(1024), lds, st, num_peds, N, V, o.order, o.key_start, o.order_peds);
    return hipGetLastError() == hipSuccess;
}

}  // namespace stg

extern "C" {

static int64_t layout_query(const stg_model_desc *d, int32_t stg::ModelLayout::*count) {
    stg::ModelLayout l;
    const int rc = stg::make_layout(d, &l);
    return rc == STG_OK ? l.*count : rc;
}
int64_t stg_model_param_count(const stg_model_desc *d) { return layout_query(d, &stg::ModelLayout::n_params); }
int64_t stg_model_buffer_count(const stg_model_desc *d) { return layout_query(d, &stg::ModelLayout::n_buffers); }
int64_t stg_model_stat_floats(const stg_model_desc *d) { return layout_query(d, &stg::ModelLayout::stat_floats); }
int64_t stg_model_ws_floats(const stg_model_desc *d, int V) {
    stg::ModelLayout l;
    const int rc = stg::make_layout(d, &l);
    if (rc != STG_OK) return rc;
    if (V <= 0) return stg::fail(STG_EINVAL, "stg_model_ws_floats: V=%d", V);
    return stg::ws_floats_per_scene(l, V);
}
int64_t stg_model_ws_tail_floats(const stg_model_desc *d, int N, int V) {
    stg::StepPlan p;
    const int rc = stg::plan_sized("stg_model_ws_tail_floats:", d, nullptr, N, V, 0, &p);
    return rc == STG_OK ? p.tail.total : rc;
}
int64_t stg_model_fwd_scratch_floats(const stg_model_desc *d, int N, int V) {
    stg::StepPlan p;
    const int rc = stg::plan_sized("stg_model_fwd_scratch_floats:", d, nullptr, N, V, 0, &p);
    return rc == STG_OK ? p.fwd.total : rc;
}
int64_t stg_model_fwd_stamps_offset(const stg_model_desc *d, int N, int V) {
    stg::StepPlan p;
    const int rc = stg::plan_sized("stg_model_fwd_stamps_offset:", d, nullptr, N, V, 0, &p);
    return rc != STG_OK ? rc : p.fwd.stamps >= 0 ? p.fwd.stamps : STG_EUNSUPPORTED;
}
int stg_scene_order(const int32_t *num_peds, int N, int V, int32_t *order, int32_t *key_start, void *stream) {
    STG_REQUIRE(N >= 0 && V > 0, STG_EINVAL, "stg_scene_order: bad sizes N=%d V=%d", N, V);
    if (N == 0) return STG_OK;
    STG_REQUIRE(num_peds && order, STG_EINVAL, "stg_scene_order: null pointer");
    STG_REQUIRE(N >= 2, STG_EUNSUPPORTED, "stg_scene_order: a single scene needs no order");
    STG_REQUIRE(N <= stg::kOrderMaxN && V <= stg::kOrderMaxV, STG_EUNSUPPORTED,
                "stg_scene_order: N=%d V=%d outside the single-workgroup sort (N <= %d, V <= %d)", N, V,
                stg::kOrderMaxN, stg::kOrderMaxV);
    STG_REQUIRE(stg::launch_scene_order(num_peds, N, V, stg::SceneOrder{order, key_start, nullptr}, stg::as_stream(stream)),
                STG_EINVAL, "stg_scene_order: launch failed");
    return STG_OK;
}

}  // extern "C"
