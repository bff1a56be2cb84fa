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

// ---- the interleaved rANS coder's table of one context (container format 12) ----
// An integer function of pc_table_row's integers f (no second float rule): T = sum f, M = 2^16, g_j = max(1, f_j (M - L) / T), and
// the deficit D = M - sum g added to the first entry with the largest f_j.  D >= 1: the largest f_j is >= T / L, so its quotient is
// >= (M - L) / L >= 1 for L <= 16 and at most L - 1 entries are raised to 1, while sum floor(f_j (M - L) / T) <= M - L.
// -> cum[j] = g_0 + ... + g_(j-1), strictly increasing, cum[L] would be M; false for a total above 2^30 + 2 (status 1: cum is then
// still a valid table, the quotients may be off).  L is a compile-time number: every array here stays in registers.
#define PC_RANS_M 65536u
#define PC_RANS_MAX_TOTAL ((1ull << 30) + 2ull)
template <int LC>
__device__ __forceinline__ bool pc_rans_row(const float (&l)[LC], float resolution, unsigned (&cum)[LC]) {
    static_assert(LC >= 1 && LC <= 16, "the coders cover 1 .. 16 centres");
    long long fr[LC];
    pc_table_row(l, LC, resolution, fr, nullptr);
    unsigned long long T = 0;
    bool big = false;
    long long fmax = fr[0];
    int jmax = 0;
#pragma unroll
    for (int j = 0; j < LC; ++j) {
        big |= (unsigned long long)fr[j] > PC_RANS_MAX_TOTAL;             // also keeps the sum and the products below from wrapping
        T += (unsigned long long)fr[j];
        if (j > 0 && fr[j] > fmax) { fmax = fr[j]; jmax = j; }
    }
    big |= T > PC_RANS_MAX_TOTAL;
    if (big) {                                                            // any valid table: one slot each, the rest to entry 0
#pragma unroll
        for (int j = 0; j < LC; ++j) cum[j] = j == 0 ? 0u : PC_RANS_M - (unsigned)(LC - j);
        return false;
    }
    unsigned g[LC], sum = 0;
#pragma unroll
    for (int j = 0; j < LC; ++j) {
        // n / d for n < 2^47, d <= 2^30 + 2, n / d < 2^16: the double quotient is within 2^-36 of the true one, its integer part off by
        // at most one, and the exact remainder decides
        const unsigned long long n = (unsigned long long)fr[j] * (PC_RANS_M - (unsigned)LC);
        unsigned long long q = (unsigned long long)((double)n / (double)T);
        const long long rem = (long long)(n - q * T);
        if (rem < 0) --q; else if ((unsigned long long)rem >= T) ++q;
        g[j] = q < 1 ? 1u : (unsigned)q;
        sum += g[j];
    }
    const unsigned D = PC_RANS_M - sum;
    unsigned run = 0;
#pragma unroll
    for (int j = 0; j < LC; ++j) {
        cum[j] = run;
        run += g[j] + (j == jmax ? D : 0u);
    }
    return true;
}
