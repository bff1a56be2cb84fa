// The arithmetic coder's integer frequency table of one context: the ONE expression that the parallel table pass
// (logits_to_freqs_kernel), the device decoder (pc_decode.hip) and the device encoder (pc_encode.hip) share.
#pragma once
#include "common.h"

// ---- logits -> integer frequency tables for the arithmetic coder (probclass.py:443-444, :474) ----
// pr = softmax(logits); freqs = max(int64(pr * resolution), 1).  One lane per context; a fixed per-row fp32
// expression (max, exp, sequential sum, divide, multiply, truncate), so the encoder (all contexts at once) and
// the decoder (one context at a time) derive IDENTICAL tables from identical logits.
__device__ __forceinline__ void pc_table_row(const float* __restrict__ l, int L, float resolution, long long* __restrict__ freqs,
                                             float* __restrict__ pr) {
    float m = l[0];
    for (int j = 1; j < L; ++j) m = fmaxf(m, l[j]);
    float e[16];
    float s = 0.f;
    for (int j = 0; j < L; ++j) { e[j] = expf(l[j] - m); s += e[j]; }
    for (int j = 0; j < L; ++j) {
        const float p = e[j] / s;
        if (pr) pr[j] = p;
        long long f = (long long)__fmul_rn(p, resolution);
        freqs[j] = f < 1 ? 1 : f;
    }
}
