// The hard quantiser's key of one (value, centre) pair: the ONE expression that quantize_hard (quantize.hip) and the rate-aware
// symbol chooser (pc_decode.hip, IC_PC_DECODE_RDO) share.
#pragma once
#include "common.h"

#define HARD_SIGMA 1e7f

// fl(-1e7 * fl(fl(|z - c|)^2)), the products un-fused: the reference's argmax logit (quantize.hip has the contract).  Its negation
// is exact, so -ic_hard_logit(z, c) is the distortion key k = fl(1e7 * fl(t * t)), t = fl(|z - c|), bit for bit.
__device__ __forceinline__ float ic_hard_logit(float z, float c) {
    const float t = fabsf(z - c);
    return __fmul_rn(-HARD_SIGMA, __fmul_rn(t, t));
}
