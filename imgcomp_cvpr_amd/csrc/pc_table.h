// The arithmetic coder's integer frequency table of one context: the ONE expression that the parallel table pass
// (logits_to_freqs_kernel), the device decoder (pc_decode.hip) and the device encoder (pc_encode.hip) share.
#pragma once
#include "common.h"
#include "quant_key.h"

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

// ---- the rate-aware symbol chooser's rule of one position (IC_PC_DECODE_RDO; tests/rdo_rule.py and codec.py have it in integers) ----
// floor-ish log2 in 2^-16 units, integers only: e = the top bit of v, m = v << (31 - e) the mantissa in [2^31, 2^32); 16 times the
// mantissa is squared (a square below 2^64, >> 31 back into [2^31, 2^33)) and the result's next bit is whether the square reached 2.
__device__ __forceinline__ int pc_ilog2_q16(unsigned v) {                  // 1 <= v < 2^32
    const int e = 31 - __clz((int)v);
    unsigned long long m = (unsigned long long)v << (31 - e);
    int r = e;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        m = (m * m) >> 31;
        r <<= 1;
        if (m >> 32) { m >>= 1; r |= 1; }
    }
    return r;
}

// cost = k + fl(lam * r): one rounded multiply, one rounded add.  (__dmul_rn / __dadd_rn are plain * and + in this toolchain and
// hipcc contracts those into an fma by default; the pragma takes the `contract` flag off these two operations, also once they are
// inlined.  The build's disassembly shows v_mul_f64 and v_add_f64 per cost and no f64 fma in the chooser.)
__device__ __forceinline__ double pc_rdo_cost(double k, double lam, double r) {
#pragma clang fp contract(off)
    const double p = lam * r;
    return k + p;
}

// The symbol of one position: the first j that attains min_j cost_j under `<`, cost_j = (double)k_j + lam * (double)R_j -- one
// rounded multiply, one rounded add, never an fma --, k_j = fl(1e7 fl(t t)), t = fl(|z - c_j|), the quantiser's own key, and
// R_j = ilog2_q16(T) - ilog2_q16(f_j) over the coder's table row f of the position (pc_table_row of its logits), T = sum f.
// rated = false (the tile's first position, which every format stores raw): all R_j = 0, the row is not read.  A total above
// 2^30 + 2: ok = false (status 1), all R_j = 0.  lam = 0 is quantize_hard whatever the row.  L is a compile-time number: every
// array here stays in registers.
template <int LC>
__device__ __forceinline__ int pc_rdo_pick(const float* __restrict__ logits, bool rated, float resolution, float z,
                                           const float* __restrict__ centers, double lam, bool& ok) {
    static_assert(LC >= 1 && LC <= 16, "the coders cover 1 .. 16 centres");
    int R[LC];
#pragma unroll
    for (int j = 0; j < LC; ++j) R[j] = 0;
    if (rated) {
        float l[LC];
#pragma unroll
        for (int j = 0; j < LC; ++j) l[j] = logits[j];
        long long fr[LC];
        pc_table_row(l, LC, resolution, fr, nullptr);
        unsigned long long T = 0;
        bool big = false;
#pragma unroll
        for (int j = 0; j < LC; ++j) {
            big |= (unsigned long long)fr[j] > PC_RANS_MAX_TOTAL;         // also keeps the sum from wrapping
            T += (unsigned long long)fr[j];
        }
        big |= T > PC_RANS_MAX_TOTAL;
        if (big) {
            ok = false;
        } else {
            const int lT = pc_ilog2_q16((unsigned)T);
#pragma unroll
            for (int j = 0; j < LC; ++j) R[j] = lT - pc_ilog2_q16((unsigned)fr[j]);
        }
    }
    double best = __builtin_inf();
    int sym = 0;
#pragma unroll
    for (int j = 0; j < LC; ++j) {
        const double k = (double)-ic_hard_logit(z, centers[j]);
        const double cost = pc_rdo_cost(k, lam, (double)R[j]);
        if (cost < best) { best = cost; sym = j; }
    }
    return sym;
}
