// Shared host/device helpers for libstgcnn_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <cstdint>

#include "../../include/stgcnn_hip.h"

namespace stg {

// ---- error reporting -------------------------------------------------------------------
char *last_error_buf();
int fail(int code, const char *fmt, ...);
int hip_fail(hipError_t e, const char *what);

#define STG_REQUIRE(cond, code, ...)            \
    do {                                        \
        if (!(cond)) return stg::fail((code), __VA_ARGS__); \
    } while (0)

#define STG_LAUNCH_CHECK(what)                           \
    do {                                                 \
        hipError_t e_ = hipGetLastError();               \
        if (e_ != hipSuccess) return stg::hip_fail(e_, what); \
    } while (0)

static inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }
// p is a multiple of `bytes` (a power of two); NULL is
static inline bool aligned(const void *p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) == 0; }

// One kernel launch with dynamic LDS: raise the kernel's hipFuncAttributeMaxDynamicSharedMemorySize to `lds` (only
// when lds > raise_above: 0 = always; a site that stays under the runtime's own limit on most batches names that limit
// and makes no runtime call for them), launch, check.  Returns STG_OK or the HIP error, recorded under `what`.
struct Launch {
    const char *what;
    dim3 grid, block;
    size_t lds;
    hipStream_t st;
    size_t raise_above = 0;
};
int raise_lds_limit(const void *kernel, size_t lds, const char *what);      // common.hip
template <typename... Params, typename... Args>
inline int launch(const Launch &l, void (*kernel)(Params...), const Args &...args) {
    if (l.lds > l.raise_above) {
        const int rc = raise_lds_limit(reinterpret_cast<const void *>(kernel), l.lds, l.what);
        if (rc != STG_OK) return rc;
    }
    hipLaunchKernelGGL(kernel, l.grid, l.block, l.lds, l.st, args...);
    STG_LAUNCH_CHECK(l.what);
    return STG_OK;
}

// The product library reads NO environment variable.  A diagnostic build (make DIAG=1 -> -DSTG_DIAG,
// libstgcnn_hip_diag.so, used by tools/ only) can override tuning constants and skip kernel phases for timing.
#ifdef STG_DIAG
int diag_env(const char *name, int dflt);
#define STG_SKIP(args, bit) (((args).debug_skip & (bit)) != 0)
#else
static inline int diag_env(const char *, int dflt) { return dflt; }
#define STG_SKIP(args, bit) false
#endif

// Desynchronise the two waves that share a SIMD: every wave of a persistent wave-per-item kernel walks the same
// phases (stage / VALU, then MFMA) on equally sized items, so SIMD partners that start together stay in lockstep --
// both stage, then both fight for the matrix pipe -- and nothing overlaps.  The second half of a workgroup's waves
// (wave >= waves/2 shares a SIMD with wave - waves/2: waves are dealt to the SIMDs cyclically) starts `units` x 64 x 127
// cycles late, about half a phase period, and from then on one partner stages while the other computes.
__device__ __forceinline__ void stagger_start(int wave, int waves, int units) {
    // units < 0: no delay, the second half of the waves gets issue priority instead (-1 -> prio 1, ... -3 -> prio 3)
    if (waves >= 2 && wave >= waves / 2) {
        if (units == -1) __builtin_amdgcn_s_setprio(1);
        else if (units == -2) __builtin_amdgcn_s_setprio(2);
        else if (units <= -3) __builtin_amdgcn_s_setprio(3);
        for (int i = 0; i < units; ++i) __builtin_amdgcn_s_sleep(127);
    }
}

// per-kernel device timing requested by the caller (stg_model_fwd / stg_model_bwd `events`)
struct EventList {
    void **ev;
    int n, next;
    hipStream_t st;
    void mark() {
        if (ev && next < n) (void)hipEventRecord(reinterpret_cast<hipEvent_t>(ev[next]), st);
        ++next;
    }
    // record the events the entry point did not reach, so that every handle the caller passed can be read back
    void finish() {
        while (ev && next < n) mark();
    }
};

constexpr int kWave = 64;           // gfx950 wavefront
constexpr int kLdsBytes = 160 * 1024;
constexpr int kNumCU = 256;

// ---- device helpers --------------------------------------------------------------------
// v += the value of the lane that the DPP control CTRL names (rows outside ROW_MASK add 0): one DPP-modified v_add
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ void dpp_add(float &v) {
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}
// Sum over the 64 lanes of the wave, result in every lane.  Six DPP-modified v_add (quad swaps, row
// mirrors, row broadcasts -- pure VALU, no LDS crossbar, no s_waitcnt) leave the total in lane 63;
// v_readlane broadcasts it.  Needs all 64 lanes active (call from wave-uniform control flow).
__device__ __forceinline__ float wave_sum(float v) {
    dpp_add<0xB1>(v);          // quad_perm [1,0,3,2]
    dpp_add<0x4E>(v);          // quad_perm [2,3,0,1]
    dpp_add<0x141>(v);         // row_half_mirror
    dpp_add<0x140>(v);         // row_mirror            -> every lane holds its 16-lane row sum
    dpp_add<0x142, 0xa>(v);    // row_bcast15 into rows 1, 3
    dpp_add<0x143, 0xc>(v);    // row_bcast31 into rows 2, 3 -> lane 63 holds the wave sum
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
// one DPP stage applied to K values
template <int CTRL, int ROW_MASK = 0xf, int K>
__device__ __forceinline__ void dpp_stage(float (&v)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) dpp_add<CTRL, ROW_MASK>(v[k]);
}
// K independent wave sums at once: every DPP stage is applied to all K values before the next stage, so the
// dependent-DPP wait states of one chain are filled by the other chains (a lone wave_sum costs ~350 cycles of
// nops and readlane hazards at two waves per SIMD; K at once ~30 cycles per value).
// the DPP stages alone: lane 63 ends up with the K wave totals (the other lanes hold partial sums)
template <int K>
__device__ __forceinline__ void wave_sum_to_last(float (&v)[K]) {
    dpp_stage<0xB1>(v);
    dpp_stage<0x4E>(v);
    dpp_stage<0x141>(v);
    dpp_stage<0x140>(v);
    dpp_stage<0x142, 0xa>(v);
    dpp_stage<0x143, 0xc>(v);
}
template <int K>
__device__ __forceinline__ void wave_sum_n(float (&v)[K]) {
    wave_sum_to_last<K>(v);
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[k]), 63));
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

}  // namespace stg
