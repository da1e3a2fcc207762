// Shared by the wave-per-scene kernel families: the fp32-MFMA generation (txp_wave.hip) and the exact-bf16 kernels with
// their team forms (txp_x6.hip) -- the argument blocks of a scene launch, position tables, the workgroup's LDS copy of the
// st_gcn parameters, persistent-grid sizes.
#pragma once
#include "model_common.hpp"
#include "stgcn_block.hpp"

namespace stg {

// Mixed-V launch (ragged batches padded beyond V = 32, sorted scene list available): ONE launch of 4-wave
// workgroups whose LDS is sized for four scenes of up to 32 pedestrians.  The workgroups split themselves (on the
// device, from the tier offsets of the sorted list -- no host sync) into three classes: small scenes run four to a
// workgroup, scenes up to `v_mid` two to a workgroup (two waves idle), larger ones one to a workgroup; the class
// sizes follow the summed crowd sizes, large classes take the lowest block indices (dispatched first).
struct MixGeom {
    int on;               // 0: uniform launch (Vl / tier as given)
    int v_small, v_mid;   // class bounds: V_n <= v_small | <= v_mid | <= V
    int block_floats;     // LDS floats of one workgroup = 4 * per-wave floats at v_small
};

// Team launch of the exact-bf16 kernels (batches padded beyond 32 pedestrians; small batches): ONE launch of 4-wave
// workgroups in which a scene-window is worked on by one, two or four waves (scene_team.hpp) according to its crowd:
// V_n <= v1 one wave (four scenes per workgroup round), V_n <= v2 two waves (two scenes per round), larger ones four.
// The workgroups read the class sizes from the tier offsets of the sorted scene list on the device (no host sync).
constexpr int kTeamMaxV = 128;       // four chunks of 32 columns
struct TeamGeom {
    int on;
    int v1, v2;           // class bounds (v1 <= 32, v2 <= 64)
    int region_floats;    // LDS floats of a workgroup's image region: one four-wave scene, two two-wave scenes, four solo scenes
};

// forward: the WHOLE model per scene -- st_gcn block (from the aggregated input stgcn_agg_kernel left) + TXP-CNN
struct TxpFwdArgs {
    ModelLayout lay;
    const float *params, *buffers;
    const int32_t *num_peds;
    SceneTier tier;        // which scenes this launch serves (ragged batches: sorted, walked boustrophedon)
    int Vl;                // LDS geometry of the launch: >= every V_n of the tier (<= V)
    MixGeom mix;
    TeamGeom team;
    int N, V;
    const float *x;        // (N, c_in, T, V) strided block input (residual branch)
    int64_t x_sn, x_sc, x_st, x_sv;
    const float *adj;      // (unused by the wave kernels: A was consumed by stgcn_agg_kernel)
    int64_t a_sn;
    const float *agg;      // per scene [agg_stride]: ax at agg_ax ([c_in][T][V_n]), cs at agg_cs ([T][V_n])
    int64_t agg_stride, agg_ax, agg_cs;
    float *y;              // (N, C, P, V)
    const unsigned *wpf;   // prepared forward A operands (txp_conv_bf16.hpp), [L+1][cv::kWpDwords], or null
    float *ws;             // per-scene workspace or null (inference)
    int64_t ws_stride;
    float *stats;          // (N, stat_floats) per-scene BatchNorm statistics (bn_mode 1) or null
    unsigned long long *stamps;   // diagnostic build only (STG_STAMPS=1), else null: [N][16] stamps per scene -- the
                                  // exact-bf16 kernels write s_memrealtime into slots 0 and 8 (scene taken up / done,
                                  // txp_x6.hip), the fp32-MFMA kernels and the block phases s_memtime (another counter,
                                  // another rate: never subtract one kind from the other)
    int debug_skip;        // diagnostic builds only
    int stagger;           // start delay of the second half of every workgroup's waves (stagger_start units)
};

// backward: TXP-CNN input-gradient chain + the st_gcn block backward per scene (everything but the TXP weight gradients)
struct TxpBwdArgs {
    ModelLayout lay;
    const float *params;
    const int32_t *num_peds;
    SceneTier tier;        // which scenes this launch serves (ragged batches: sorted, walked boustrophedon)
    int Vl;                // LDS geometry of the launch: >= every V_n of the tier (<= V)
    MixGeom mix;
    TeamGeom team;
    int N, V;
    const float *x;        // (N, c_in, T, V) strided block input (residual branch)
    int64_t x_sn, x_sc, x_st, x_sv;
    const float *adj;      // (unused: no dx on this path, A is not needed)
    int64_t a_sn;
    const float *dy;       // (N, C, P, V): dV_pred -- or, with nll_target, V_pred itself
    // fused loss (stg_model_bwd_nll): the input stage computes d(sum_n w_n loss_n)/dV_pred from V_pred and the
    // target instead of reading it, and writes the per-scene losses
    const float *nll_target;   // (N, P, V, 2) or null
    const float *nll_weights;  // (N) or null (all ones)
    float *nll_losses;         // (N)
    const float *ws;
    int64_t ws_stride;
    float *dzg;            // [N][L][dz_slot(V)]   dz_l of the hidden layers for the weight-gradient GEMM
    const unsigned *wp;    // prepared input-gradient A operands (txp_conv_bf16.hpp), [L+1][cv::kWpDwords] -- the batch
                           // tail of the workspace, written by the forward's aggregation launch -- or null
    float *rows;           // [N][n_blk_params + n_txp]  per-scene small-parameter gradients: st_gcn block, PReLU slopes
    unsigned long long *stamps;   // diagnostic build only (STG_STAMPS=1), else null: [N][16], as TxpFwdArgs::stamps
    int debug_skip;        // timing-only diagnostic (STG_DEBUG_SKIP): 512 dz build, 1024 dgrad tile loops -- wrong results
    int split_bf16;        // 1: the input-gradient GEMMs run on bf16 MFMAs with hi/lo-split operands (see txp_wave.hip)
    int stagger;           // start delay of the second half of every workgroup's waves (stagger_start units)
};

// txp_x6.hip: the exact-bf16 kernels (txp_fwd_x6 / txp_bwd_x6, one wave per scene, and their team forms): V <= kTeamMaxV.
// The two predicates are asked by the planner only (step_plan.hpp); the launchers need the prepared operands (wpf / wp).
bool txp_fwd_x6_fits(const ModelLayout &L, int V);
bool txp_bwd_x6_fits(const ModelLayout &L, int V);
int64_t txp_bwd_x6_wp_floats(const ModelLayout &L);
int launch_txp_fwd_x6(const TxpFwdArgs &a, hipStream_t st);
int launch_txp_bwd_x6(const TxpBwdArgs &a, hipStream_t st);
// both passes of a training step as one launch (txp_step_x6_kernel): where each pass would run its solo Canon32 kernel
bool txp_step_x6_fits(const ModelLayout &L, const int32_t *num_peds, int N, int V);
int launch_txp_step_x6(const TxpFwdArgs &f, const TxpBwdArgs &b, hipStream_t st);

// LDS floats of one wave's position table (16-bit entries, Cfg::T * v of them) [+ the st_gcn tail's 32 reduction totals]
__host__ __device__ inline int ptab_floats(int v) { return ((Cfg::T * v + 1) / 2 + 3) & ~3; }
__host__ __device__ inline int bwd_ptab_floats(int v) { return ptab_floats(v) + kRedMax; }
// LDS floats of the workgroup's copy of the st_gcn block parameters and BatchNorm running statistics: the block code
// of the wave kernels reads them with broadcast LDS reads (no SGPR pressure, no scalar-load waits inside its passes)
__host__ __device__ inline int wave_param_floats(const ModelLayout &L) {
    return ((L.n_blk_params + 3) & ~3) + ((L.n_buffers + 3) & ~3);
}

// position -> (h << 8 | w) table of the scene, T * vi entries of 16 bits: p < C * vi are the positions of the TXP
// plane, q < T * vi the (t, w) columns of the st_gcn block -- no integer divisions per tile / column
__device__ __forceinline__ void build_ptab(ptab_t *ptab, int vi) {
    const int lane = threadIdx.x & 63;
    for (int p = lane; p < Cfg::T * vi; p += 64) {
        const int h = p / vi;
        ptab[p] = (ptab_t)((h << 8) | (p - h * vi));
    }
}
// the same for a wave that owns the column chunk [w0, w0 + wc) of a scene: position p of the chunk is (row p / wc, column
// w0 + p % wc) of the scene
__device__ __forceinline__ void build_ptab(ptab_t *ptab, int w0, int wc) {
    const int lane = threadIdx.x & 63;
    if (wc <= 0 && lane == 0) ptab[0] = 0;            // (an empty chunk: entry 0 is still read, never used)
    for (int p = lane; p < Cfg::T * wc; p += 64) {
        const int h = p / wc;
        ptab[p] = (ptab_t)((h << 8) | (w0 + p - h * wc));
    }
}


// "Every vector-memory operation issued so far has completed", stated where the compiler can see it (an S_WAITCNT it
// models).  vmcnt counts loads AND stores in order; wherever a register MAY still be waiting for a load on some path of
// the control-flow graph (a tile loop whose iterations are guarded by runtime tile counts is enough), the compiler puts
// s_waitcnt vmcnt(0) in front of its use -- which also waits for the acknowledgement of every store issued since: one
// HBM round trip per tile.  Draining once, right after the loads and before the guarded code, leaves nothing pending,
// and the tiles' stores are fire-and-forget again.  (Found in the ISA, not in a counter: DESIGN 5.2.)
__device__ __forceinline__ void vm_drain() { __builtin_amdgcn_s_waitcnt(0x0F70); }   // vmcnt(0), expcnt / lgkmcnt free

// Workgroup prologue of the wave kernels: the st_gcn block's parameters (and running statistics) into LDS, once.
__device__ __forceinline__ void stage_block_params(const ModelLayout &L, const float *__restrict__ params,
                                                   const float *__restrict__ buffers, float *blk_p, float *blk_b, int nt) {
    for (int e = threadIdx.x; e < L.n_blk_params; e += nt) blk_p[e] = params[e];
    if (buffers)
        for (int e = threadIdx.x; e < L.n_buffers; e += nt) blk_b[e] = buffers[e];
    __syncthreads();
}

// ---- persistent grids (host) ----------------------------------------------------------------------------
inline int wave_wpb(size_t per_wave) {
    // 4 waves per workgroup: the LDS footprint then admits either one workgroup (forward: 4 waves per CU,
    // one per SIMD) or two (backward: 8 per CU, two per SIMD) -- BALANCED over the four SIMDs.  Odd
    // residencies (6 waves per CU) measured 1.5x slower per wave (tools/micro/conv_tile_bench.hip).
    int wpb = diag_env("STG_TXP_WPB", 4);
    if (wpb != 1 && wpb != 2 && wpb != 8) wpb = 4;
    while (wpb > 1 && per_wave * wpb > (size_t)kLdsBytes) wpb >>= 1;
    return wpb;
}

// persistent grid: as many workgroups as the chip holds at once (LDS-limited, 2 waves per SIMD)
inline int wave_grid(size_t lds, int wpb, int N) {
    int per_cu = (int)(kLdsBytes / lds);
    if (per_cu * wpb > 8) per_cu = 8 / wpb;
    if (per_cu < 1) per_cu = 1;
    const int need = (N + wpb - 1) / wpb;
    const int g = kNumCU * per_cu;
    if (g >= need) return need;
    // equal shares: the smallest number of rounds that fits, then just enough workgroups for it
    const int rounds = (need + g - 1) / g;
    return (need + rounds - 1) / rounds;
}

}  // namespace stg
