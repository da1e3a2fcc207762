// The round-1 fp32-MFMA wave-per-scene kernels (txp_wave.hip): launchers.  Included by the planner (model_layout.hip) only.
#pragma once
#include "txp_scene_common.hpp"

namespace stg {

// the fp32-MFMA wave kernels and their mixed-V launch; a.wpf / a.wp are not used
int launch_txp_fwd_wave(const TxpFwdArgs &a, hipStream_t st);
int launch_txp_bwd_wave(const TxpBwdArgs &a, hipStream_t st);
// whether their LDS images leave at least three waves per CU at this V
bool txp_wave_f32_fits(int V);

}  // namespace stg
