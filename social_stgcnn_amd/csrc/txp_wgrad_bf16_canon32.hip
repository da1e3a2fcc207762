// The Canon32 instantiations of the weight-gradient kernel (txp_wgrad_bf16.hip: the canonical model, uniform scenes of 32
// pedestrians) and their launcher, a translation unit of their own.
#define STG_K2_CANON32_TU
#include "txp_wgrad_bf16.hip"
