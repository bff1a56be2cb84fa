// Sequential decoder of the context model: the range decoder on the device, one symbol after the other, with the logits of
// probclass.hip reproduced bit for bit -- the launch-per-layer loop (any k), the persistent kernels for k = 24 (whole context
// recomputed; activation caches), tiles of one or several volumes in one launch, tiles coded in wavefront order.
//   reference: code/bit_counter.py:137-164 (decode loop), fjcommon arithmetic_coding.py (ArithmeticDecoder)
// Host entry points: ic_pc_decode_f32, ic_pc_decode_tiles_f32, ic_pc_decode_tiles_batch_f32 and their *_workspace_bytes;
// ic_pc_decode_channels_f32 and ic_pc_decode_tiles_batch_channels_f32 decode only the first channels of every stream (preview);
// ic_pc_decode_tiles_batch_layers_f32 reads every tile's stream as segments cut at channel planes (container format 6);
// ic_pc_decode_tiles_batch_layers_pertile_f32 does so with a channel limit per tile (recovery of damaged or cut layered files);
// ic_pc_decode_tiles_batch_layers_resume_f32 continues every tile at the layer where an earlier call on the same workspace stopped;
// ic_pc_decode_tiles_batch_fronts_f32 and ic_pc_decode_tiles_batch_fronts_pertile_f32 read every tile's wavefront-ordered stream as
// segments cut at fronts (container format 8), with one channel limit or one per tile;
// ic_pc_decode_tiles_batch_fronts_resume_f32 continues every tile's front sweep at the layer end where an earlier call stopped.
// ic_pc_decode_tiles_batch_channels_f32 with IC_PC_DECODE_RDO is the encoder's: the front sweep over records of (lambda, z) CHOOSES
// every tile's symbols by distortion + lambda * rate where the decoder reads them from a stream (pc_rdo_tiles_batch_kernel).
#include "common.h"
#include "pc_table.h"
#include "pc_internal.h"

// ---- sequential decoder (row N3: bit_counter.py:137-164 without the host in the loop) ----------------------------------
// A symbol's frequency table depends on the symbols decoded before it, so decoding is one context at a time by nature.
// The reference (and bit_counter._decode here) does a host round trip per symbol: gather the 5x9x9 context, run the
// network, fetch the table, step the arithmetic decoder in Python -- ~160 us per symbol.  Here the whole loop is
// enqueued on the stream: per symbol the SAME four context-model kernels as the parallel encoder side run on the
// gathered context (identical fp32 expression per logit -> identical tables, the property tested by
// test_blockwise_logits_bit_identical_to_full_volume), then ONE small kernel turns the logits into the integer table
// (pc_table_row, shared with logits_to_freqs_kernel), steps the arithmetic decoder (32-bit range coder, the reference's
// arithmetic_coding.py:ArithmeticDecoder restated for the device), stores the symbol, writes its centre into the padded
// volume and gathers the next context.  No host synchronisation until the end.
#define PC_AC_BITS 32
struct PcDecState {
    unsigned long long low, high, code;
    long long byte_pos;        // index of cur_byte (-1 before the first byte)
    int bit_left, cur_byte;
    int nxt_byte;              // byte byte_pos + 1, requested one byte early so that its load latency is off the path
    int error;                 // 1: frequency total too large, 2: internal
    long long next;            // raster index of the next symbol to decode
};

struct PcDecArgs {
    const unsigned char* bits; long long nbytes;
    PcDecState* st;
    const float* centers; const float* logits;
    float* vol;                // padded volume (C+4, h+8, w+8) of centre values
    float* ctx;                // (5, 9, 9) context of the next symbol
    long long* symbols;        // (C, h, w)
    int C, h, w, L, first_sym;
    float resolution;
};

__device__ __forceinline__ int pc_dec_bit(const unsigned char* bits, long long nbytes, PcDecState& s) {
    if (s.bit_left == 0) {
        s.cur_byte = s.nxt_byte;
        s.byte_pos += 1;
        const long long np = s.byte_pos + 1;
        s.nxt_byte = np < nbytes ? bits[np] : 0;       // past the end the stream reads as zeros (arithmetic_coding.py)
        s.bit_left = 8;
    }
    --s.bit_left;
    return (s.cur_byte >> s.bit_left) & 1;
}
__device__ __forceinline__ int pc_dec_bit(const PcDecArgs& a, PcDecState& s) { return pc_dec_bit(a.bits, a.nbytes, s); }

// a coder before its first bit: the whole range, no byte consumed, byte 0 requested.  The 32 priming bits of `code` are the
// caller's to read (pc_dec_bit), by the one thread or wave that keeps the state.
__device__ __forceinline__ void pc_dec_state_init(PcDecState& s, const unsigned char* bits, long long nbytes) {
    s.low = 0; s.high = (1ull << PC_AC_BITS) - 1; s.code = 0;
    s.byte_pos = -1; s.bit_left = 0; s.cur_byte = 0; s.nxt_byte = nbytes > 0 ? bits[0] : 0; s.error = 0; s.next = 1;
}

__device__ void pc_dec_gather(const PcDecArgs& a, long long idx) {
    // context of symbol idx = padded block [c, c+5) x [y, y+9) x [x, x+9)
    const int HW = a.h * a.w;
    const int c = (int)(idx / HW), r = (int)(idx - (long long)c * HW);
    const int y = r / a.w, x = r - y * a.w;
    const int PH = a.h + 8, PW = a.w + 8;
    for (int e = threadIdx.x; e < 5 * 9 * 9; e += blockDim.x) {
        const int d = e / 81, r2 = e - d * 81;
        a.ctx[e] = a.vol[((size_t)(c + d) * PH + y + r2 / 9) * PW + x + r2 % 9];
    }
}

__global__ __launch_bounds__(256) void pc_dec_fill_kernel(float* __restrict__ vol, long long n, const float* __restrict__ centers) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) vol[i] = centers[0];                       // symbol 0 everywhere: pad_symbols_volume pads with 0
}

__global__ __launch_bounds__(256) void pc_dec_init_kernel(const PcDecArgs a) {
    if (threadIdx.x == 0) {
        PcDecState s;
        pc_dec_state_init(s, a.bits, a.nbytes);
        for (int i = 0; i < PC_AC_BITS; ++i) s.code = (s.code << 1) | (unsigned)pc_dec_bit(a, s);
        *a.st = s;
        a.symbols[0] = a.first_sym;                       // the first symbol is not coded (bit_counter.py:117-121,152)
        a.vol[((size_t)4 * (a.h + 8) + 4) * (a.w + 8) + 4] = a.centers[a.first_sym];
    }
    __syncthreads();
    if ((long long)a.C * a.h * a.w > 1) pc_dec_gather(a, 1);
}

// one symbol: integer table from the logits, range-decoder step (arithmetic_coding.py:ArithmeticDecoder.read + _narrow)
__device__ int pc_dec_symbol(const PcDecArgs& a, PcDecState& s, const float* logits) {
    const unsigned long long MASK = (1ull << PC_AC_BITS) - 1, TOP = 1ull << (PC_AC_BITS - 1), SECOND = TOP >> 1;
    const unsigned long long MAX_TOTAL = (1ull << (PC_AC_BITS - 2)) + 2;
    long long fr[16];
    pc_table_row(logits, a.L, a.resolution, fr, nullptr);
    unsigned long long total = 0;
    for (int j = 0; j < a.L; ++j) total += (unsigned long long)fr[j];
    if (total > MAX_TOTAL) s.error = 1;
    const unsigned long long r = s.high - s.low + 1;
    const unsigned long long value = ((s.code - s.low + 1) * total - 1) / r;
    int sym = 0;
    unsigned long long cum = 0;
    while (sym + 1 < a.L && cum + (unsigned long long)fr[sym] <= value) { cum += (unsigned long long)fr[sym]; ++sym; }
    const unsigned long long cum_lo = cum, cum_hi = cum + (unsigned long long)fr[sym];
    s.high = s.low + cum_hi * r / total - 1;
    s.low = s.low + cum_lo * r / total;
    while (((s.low ^ s.high) & TOP) == 0) {
        s.code = ((s.code << 1) & MASK) | (unsigned)pc_dec_bit(a, s);
        s.low = (s.low << 1) & MASK;
        s.high = ((s.high << 1) & MASK) | 1;
    }
    while ((s.low & ~s.high & SECOND) != 0) {
        s.code = (s.code & TOP) | ((s.code << 1) & (MASK >> 1)) | (unsigned)pc_dec_bit(a, s);
        s.low = (s.low << 1) & (MASK >> 1);
        s.high = ((s.high << 1) & (MASK >> 1)) | TOP | 1;
    }
    return sym;
}

// n / d for n < 2^63, d < 2^34, n / d < 2^34: the double-precision quotient is within 2^-18 of the true one, so its integer
// part is off by at most one; one exact 64-bit multiply decides.  (The 64-bit integer division the compiler expands to is
// ~4x the instructions, and the sequential decoder does three per symbol on its critical path.)
__device__ __forceinline__ unsigned long long pc_udiv(unsigned long long n, unsigned long long d) {
    unsigned long long q = (unsigned long long)((double)n / (double)d);
    const long long rem = (long long)(n - q * d);
    if (rem < 0) --q; else if ((unsigned long long)rem >= d) ++q;
    return q;
}

// pc_dec_symbol for a whole wave: lane 48 + j holds logit j (0 beyond L -- logits are >= 0 after the ReLU, so the extra
// lanes do not move the maximum), the coder state is identical in every lane.  The per-symbol table is the expression of
// pc_table_row with its L exponentials, divisions and conversions spread over L lanes; the sum runs over readlane values in
// j order (0 + e0 + e1 + ...: the same fp32 sequence).  Returns the symbol (uniform).
template <int LC>       // LC = number of centres when known at compile time (the loops over readlane unroll), 0 = a.L
__device__ __forceinline__ int pc_dec_symbol_wave(const unsigned char* bits, long long nbytes, int L_rt, float resolution, PcDecState& s, float logit) {
    const unsigned long long MASK = (1ull << PC_AC_BITS) - 1, TOP = 1ull << (PC_AC_BITS - 1), SECOND = TOP >> 1;
    const unsigned long long MAX_TOTAL = (1ull << (PC_AC_BITS - 2)) + 2;
    const int L = LC ? LC : L_rt, lane = threadIdx.x & 63;
    auto bcast = [](float v, int src) -> float { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), src)); };
    float m = bcast(logit, 48);
#pragma unroll
    for (int j = 1; j < L; ++j) m = fmaxf(m, bcast(logit, 48 + j));
    const float e = (lane >= 48 && lane < 48 + L) ? expf(logit - m) : 0.f;
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < L; ++j) sum += bcast(e, 48 + j);
    const float pr = e / sum;
    long long fl = (long long)__fmul_rn(pr, resolution);
    fl = fl < 1 ? 1 : fl;
    const unsigned f32 = (unsigned)fl;                   // <= resolution < 2^31 (total is checked against 2^30 + 2 below)
    unsigned long long total = 0;
#pragma unroll
    for (int j = 0; j < L; ++j) total += (unsigned)__builtin_amdgcn_readlane((int)f32, 48 + j);
    if (total > MAX_TOTAL || (fl >> 31) != 0) s.error = 1;
    const unsigned long long r = s.high - s.low + 1;
    const unsigned long long value = pc_udiv((s.code - s.low + 1) * total - 1, r);
    int sym = 0;
    unsigned long long cum = 0;
    unsigned fs = (unsigned)__builtin_amdgcn_readlane((int)f32, 48);
    while (sym + 1 < L && cum + fs <= value) { cum += fs; ++sym; fs = (unsigned)__builtin_amdgcn_readlane((int)f32, 48 + sym); }
    const unsigned long long cum_lo = cum, cum_hi = cum + fs;
    s.high = s.low + pc_udiv(cum_hi * r, total) - 1;
    s.low = s.low + pc_udiv(cum_lo * r, total);
    while (((s.low ^ s.high) & TOP) == 0) {
        s.code = ((s.code << 1) & MASK) | (unsigned)pc_dec_bit(bits, nbytes, s);
        s.low = (s.low << 1) & MASK;
        s.high = ((s.high << 1) & MASK) | 1;
    }
    while ((s.low & ~s.high & SECOND) != 0) {
        s.code = (s.code & TOP) | ((s.code << 1) & (MASK >> 1)) | (unsigned)pc_dec_bit(bits, nbytes, s);
        s.low = (s.low << 1) & (MASK >> 1);
        s.high = ((s.high << 1) & (MASK >> 1)) | TOP | 1;
    }
    return sym;
}

__device__ __forceinline__ void pc_dec_store(const PcDecArgs& a, long long idx, int sym) {
    const int HW = a.h * a.w;
    const int c = (int)(idx / HW), rr = (int)(idx - (long long)c * HW);
    a.symbols[idx] = sym;
    a.vol[((size_t)(c + 4) * (a.h + 8) + rr / a.w + 4) * (a.w + 8) + rr % a.w + 4] = a.centers[sym];
}

__global__ __launch_bounds__(256) void pc_dec_step_kernel(const PcDecArgs a) {
    __shared__ long long sh_next;
    if (threadIdx.x == 0) {
        PcDecState s = *a.st;
        const int sym = pc_dec_symbol(a, s, a.logits);
        pc_dec_store(a, s.next, sym);
        s.next += 1;
        *a.st = s;
        sh_next = s.next;
        __threadfence_block();
    }
    __syncthreads();
    if (sh_next < (long long)a.C * a.h * a.w) pc_dec_gather(a, sh_next);
}

// ---- the same loop as ONE persistent work-group (k = 24): no launches between symbols -------------------------------------
// The five launches per symbol above cost ~5 us of launch latency each on top of ~5 us of work.  Here one work-group
// keeps the coder state in registers and the activations of the current 5x9x9 context in LDS and runs, per symbol:
// gather -> layer 0 (VALU, one lane per voxel) -> the three matrix-core layers -> table + range-decoder step.
// Bit-identical to the parallel pass by construction: every output is the same operation sequence -- layer 0 the fmaf
// chain of pc_conv3d_kernel<.., FIRST> in (kd,kh,kw) order, the other layers the MFMA chain of pc_mfma_kernel in
// (8-channel chunk, tap, k-step) order with the same packed A fragments, then + bias, ReLU, + residual.  Only the
// voxel -> lane assignment differs (the 75 / 18 / 1 output voxels of the context are packed densely into 32-voxel
// accumulator tiles: three waves, one wave, one wave), which no output value depends on.
struct PcFusedArgs {
    PcDecArgs d;
    const float* w0; const float* b0;          // layer 0: TF filter [2,3,3,1,k], bias
    const float* pk1; const float* b1;         // packed k -> k
    const float* pk2; const float* b2;
    const float* pk3; const float* b3;         // packed k -> L
    int* status;
};

// One of the PC_NP partial sums (steps [42 PART, 42 PART + 42) of the 168-step K sequence of pc_mfma_kernel<24, ...>) for
// NTL 32-voxel tiles at once: input volume [24][ID][IH][IW] in LDS, output voxel q = 32 i + (lane & 31) of the
// (ID-1, IH-2, IW-2) grid.  The tiles share the A fragments and give the wave independent accumulators to interleave.
template <int ID, int IH, int IW, int NTL, int PART>
__device__ __forceinline__ void pc_fused_part(const float* __restrict__ sin, const pc_f32x4* __restrict__ wp, int lane,
                                              pc_f32x16 (&acc)[NTL]) {
    constexpr int OH = IH - 2, OW = IW - 2, NV = (ID - 1) * OH * OW, IVOL = ID * IH * IW;
    constexpr int G0 = 42 * PART, G1 = G0 + 42, TS0 = G0 / 4, TS1 = (G1 - 1) / 4;       // tap-steps (c8 * 14 + t) touched
    static_assert(3 * PC_NT * 4 == 42 * PC_NP, "k = 24: 168 steps in 4 parts");
    const int kh = lane >> 5;
    int base[NTL];
#pragma unroll
    for (int i = 0; i < NTL; ++i) {
        const int q = 32 * i + (lane & 31);
        const int qq = q < NV ? q : 0;
        const int od = qq / (OH * OW), oy = (qq / OW) % OH, ox = qq % OW;
        base[i] = (od * IH + oy) * IW + ox + kh * IVOL;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    }
    pc_f32x4 av[TS1 - TS0 + 1];
#pragma unroll
    for (int ts = TS0; ts <= TS1; ++ts) av[ts - TS0] = wp[(size_t)ts * 64];               // all A fragments of the part up front
#pragma unroll
    for (int ts = TS0; ts <= TS1; ++ts) {
        const int c8 = ts / PC_NT, t = ts % PC_NT;
        const int tapoff = pc_tap_kd(t) * IH * IW + pc_tap_kh(t) * IW + pc_tap_kw(t);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int g = 4 * ts + ks;
            if (g < G0 || g >= G1) continue;
#pragma unroll
            for (int i = 0; i < NTL; ++i) {
                const float bv = sin[base[i] + (8 * c8 + 2 * ks) * IVOL + tapoff];
                acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[ts - TS0][ks], bv, acc[i], 0, 0, 0);
            }
        }
    }
}

template <int ID, int IH, int IW, int NTL>
__device__ __forceinline__ void pc_fused_layer(const float* __restrict__ sin, const float* __restrict__ pk, int wave, int lane,
                                               pc_f32x16 (&acc)[NTL]) {
    const pc_f32x4* wp = reinterpret_cast<const pc_f32x4*>(pk) + lane;
    if (wave == 0) pc_fused_part<ID, IH, IW, NTL, 0>(sin, wp, lane, acc);
    else if (wave == 1) pc_fused_part<ID, IH, IW, NTL, 1>(sin, wp, lane, acc);
    else if (wave == 2) pc_fused_part<ID, IH, IW, NTL, 2>(sin, wp, lane, acc);
    else pc_fused_part<ID, IH, IW, NTL, 3>(sin, wp, lane, acc);
}

__global__ __launch_bounds__(256) void pc_dec_fused_kernel(const PcFusedArgs f) {
    constexpr int K = 24;
    __shared__ float s_ctx[5 * 9 * 9];
    __shared__ float s_a0[K * 196];            // layer 0 output  [k][4][7][7]
    __shared__ float s_a1[K * 75];             // res1/conv1      [k][3][5][5]
    __shared__ float s_a2[K * 18];             // res1/conv2 + skip [k][2][3][3]
    __shared__ float s_logits[16];
    __shared__ float s_red[4 * 16 * 64];       // the four partial accumulators of one tile, [part][register][lane]
    __shared__ float s_w0[13 * K];             // layer-0 filter rows of the 13 live taps, live-tap order
    __shared__ float s_bias[3 * K + 16];       // b0 | b1 | b2 | b3
    __shared__ float s_centers[16];
    const PcDecArgs& a = f.d;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int e = tid; e < 13 * K; e += 256) {
        const int lt = e / K;                                   // live tap lt -> (kd,kh,kw): 0..8 = kd 0; 9..11 = (1,0,*); 12 = (1,1,0)
        const int tap = lt < 9 ? lt : (lt < 12 ? 9 + (lt - 9) : 12);
        s_w0[e] = f.w0[(size_t)tap * K + e % K];
    }
    if (tid < K) { s_bias[tid] = f.b0[tid]; s_bias[K + tid] = f.b1[tid]; s_bias[2 * K + tid] = f.b2[tid]; }
    if (tid < a.L) { s_bias[3 * K + tid] = f.b3[tid]; s_centers[tid] = a.centers[tid]; }
    const long long n = (long long)a.C * a.h * a.w;
    PcDecState s;                               // lives in thread 0's registers for the whole volume
    if (tid == 0) {
        pc_dec_state_init(s, a.bits, a.nbytes);
        for (int i = 0; i < PC_AC_BITS; ++i) s.code = (s.code << 1) | (unsigned)pc_dec_bit(a, s);
        pc_dec_store(a, 0, a.first_sym);        // the first symbol is not coded
    }
    __syncthreads();
    const int HW = a.h * a.w, PH = a.h + 8, PW = a.w + 8;
#ifdef PC_DEC_PROF
    unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tl = __builtin_amdgcn_s_memtime();
#define PC_PH(i) do { const unsigned long long tn_ = __builtin_amdgcn_s_memtime(); ph[i] += tn_ - tl; tl = tn_; } while (0)
#else
#define PC_PH(i) do { } while (0)
#endif
    for (long long idx = 1; idx < n; ++idx) {
        // ---- context of symbol idx: padded block [c, c+5) x [y, y+9) x [x, x+9) ----
        {
            const int c = (int)(idx / HW), r = (int)(idx - (long long)c * HW);
            const int y = r / a.w, x = r - y * a.w;
            for (int e = tid; e < 405; e += 256) {
                const int d = e / 81, r2 = e - d * 81;
                s_ctx[e] = a.vol[((size_t)(c + d) * PH + y + r2 / 9) * PW + x + r2 % 9];
            }
        }
        __syncthreads();
        PC_PH(0);
        // ---- layer 0: 1 -> k, first mask (13 live taps), + bias, ReLU; one lane = one of the 196 voxels ----
        if (tid < 196) {
            const int od = tid / 49, oy = (tid / 7) % 7, ox = tid % 7;
            float acc[K];
#pragma unroll
            for (int c = 0; c < K; ++c) acc[c] = 0.f;
#pragma unroll
            for (int kd = 0; kd < 2; ++kd)
#pragma unroll
                for (int kh2 = 0; kh2 < 3; ++kh2)
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) {
                        const bool dead = (kd == 1) && (kh2 == 2 || (kh2 == 1 && kw >= 1));
                        if (dead) continue;
                        const float xv = s_ctx[(od + kd) * 81 + (oy + kh2) * 9 + ox + kw];
                        const int tap = (kd * 3 + kh2) * 3 + kw;           // live taps are 0..12 in this order
                        const float* wp = s_w0 + tap * K;
#pragma unroll
                        for (int c = 0; c < K; ++c) acc[c] = fmaf(xv, wp[c], acc[c]);
                    }
#pragma unroll
            for (int c = 0; c < K; ++c) s_a0[c * 196 + tid] = fmaxf(acc[c] + s_bias[c], 0.f);
        }
        __syncthreads();
        PC_PH(1);
        // ---- res1/conv1: k -> k, ReLU; 75 voxels = 3 tiles; wave w computes partial sum w of all three ----
        {
            pc_f32x16 acc[3];
            pc_fused_layer<4, 7, 7, 3>(s_a0, f.pk1, wave, lane, acc);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
#pragma unroll
                for (int r = 0; r < 16; ++r) s_red[(wave * 16 + r) * 64 + lane] = acc[i][r];
                __syncthreads();
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int o = tid + 256 * e, r = o >> 6, ln = o & 63;
                    const int co = (r & 3) + 8 * (r >> 2) + 4 * (ln >> 5), q = 32 * i + (ln & 31);
                    const float v = (s_red[o] + s_red[1024 + o]) + (s_red[2048 + o] + s_red[3072 + o]);
                    if (co < K && q < 75) s_a1[co * 75 + q] = fmaxf(v + s_bias[K + co], 0.f);
                }
                __syncthreads();
            }
        }
        PC_PH(2);
        // ---- res1/conv2: k -> k, linear, + layer-0 output cropped [2:, 2:-2, 2:-2]; 18 voxels = 1 tile ----
        {
            pc_f32x16 acc[1];
            pc_fused_layer<3, 5, 5, 1>(s_a1, f.pk2, wave, lane, acc);
#pragma unroll
            for (int r = 0; r < 16; ++r) s_red[(wave * 16 + r) * 64 + lane] = acc[0][r];
            __syncthreads();
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int o = tid + 256 * e, r = o >> 6, ln = o & 63;
                const int co = (r & 3) + 8 * (r >> 2) + 4 * (ln >> 5), q = ln & 31;
                const float v = (s_red[o] + s_red[1024 + o]) + (s_red[2048 + o] + s_red[3072 + o]);
                if (co < K && q < 18) {
                    const int od = q / 9, oy = (q / 3) % 3, ox = q % 3;
                    float x = v + s_bias[2 * K + co];
                    x += s_a0[co * 196 + ((od + 2) * 7 + oy + 2) * 7 + ox + 2];
                    s_a2[co * 18 + q] = x;
                }
            }
            __syncthreads();
        }
        PC_PH(3);
        // ---- conv2 (final): k -> L, ReLU; one voxel ----
        {
            pc_f32x16 acc[1];
            pc_fused_layer<2, 3, 3, 1>(s_a2, f.pk3, wave, lane, acc);
            if ((lane & 31) == 0) {
#pragma unroll
                for (int r = 0; r < 8; ++r) s_red[(wave * 16 + r) * 64 + lane] = acc[0][r];
            }
            __syncthreads();
            if (tid < 16) {
                // channel co lives in register r = (co & 3) + 4 * (co >> 3) of lane 32 * ((co >> 2) & 1)
                const int co = tid, r = (co & 3) + 4 * (co >> 3), ln = 32 * ((co >> 2) & 1), o = r * 64 + ln;
                const float v = (s_red[o] + s_red[1024 + o]) + (s_red[2048 + o] + s_red[3072 + o]);
                if (co < a.L) s_logits[co] = fmaxf(v + s_bias[3 * K + co], 0.f);
            }
            __syncthreads();
        }
        PC_PH(4);
        if (tid == 0) {
            const int sym = pc_dec_symbol(a, s, s_logits);
            const int c = (int)(idx / HW), rr = (int)(idx - (long long)c * HW);
            a.symbols[idx] = sym;
            a.vol[((size_t)(c + 4) * PH + rr / a.w + 4) * PW + rr % a.w + 4] = s_centers[sym];
            __threadfence_block();
        }
        __syncthreads();
        PC_PH(5);
    }
    if (tid == 0) *f.status = s.error;
#ifdef PC_DEC_PROF
    if (tid == 0) for (int i = 0; i < 6; ++i) ((unsigned long long*)a.st)[i] = ph[i];
#endif
}

// ---- the persistent decoder with activation caches (k = 24): one NEW voxel per layer per symbol ----------------------------
// pc_dec_fused_kernel recomputes the whole 5x9x9 context of every symbol: 196 + 75 + 18 + 1 voxels.  But an activation depends
// only on symbols BEFORE its own position (the first layer's mask excludes the centre), so every voxel of every layer can
// be computed exactly once, the moment its last input is known, and kept (Fast-PixelCNN caching; here for a VALID-conv
// network over a padded volume, so the caches include the halo voxels that see pad values).  In absolute indices of the
// padded volume V[(C+4)][(h+8)][(w+8)]:
//     A0[d][i][j] = relu(conv0(V[d..d+1][i..i+2][j..j+2]))          d <= C+2, i <= h+5, j <= w+5
//     A1[d][i][j] = relu(conv1(A0[d..d+1][i..i+2][j..j+2]))         d <= C+1, i <= h+3, j <= w+3
//     A2[d][i][j] = conv2(A1[d..d+1][i..i+2][j..j+2]) + A0[d+2][i+2][j+2]
//     logits of symbol (c, y, x) = relu(conv3(A2[c..c+1][y..y+2][x..x+2]))
// and the last live tap of every window is its (1,1,1) corner ((1,1,0) for conv0).  The kernel sweeps P = (D, I, J) over the
// padded volume in raster order; at P it knows V[P] and computes  A0[D-1][I-1][J] -> A1[D-2][I-2][J-1] -> A2[D-3][I-3][J-2]
// -> the logits of the symbol at V[D][I][J+1], decodes it, and moves on.  Everything else those four need was computed at
// an earlier P: 13 of a window's 14 taps are prefetched from the caches (channels-last, in HBM/L2) while the range decoder
// works on the previous symbol, the (1,1,0) tap is the previous step's voxel and stays in LDS.
// Bit-identical to the parallel pass: fp32 MFMA is an fma chain in ascending k (tools/mfma_order.hip: v_mfma_f32_32x32x2_f32 and
// 16x16x4 against fmaf chains, 0 mismatches), so ONE output of pc_mfma_kernel is four fmaf chains over the K sequence
// (8-channel group, tap, channel pair) cut at 42-step boundaries, summed (p0 + p1) + (p2 + p3).  Wave w runs part w; lanes
// 0..23 hold the weights of conv1's outputs, lanes 24..47 conv2's, lanes 48.. conv3's -- the same 84 registers per lane serve
// all three layers, each layer is one pass of 84 dependent v_fma over broadcast LDS reads.
struct PcCachedArgs {
    PcDecArgs d;
    const float* w0; const float* b0; const float* w1; const float* b1; const float* w2; const float* b2; const float* w3; const float* b3;
    float* c0; float* c1; float* c2;          // activation caches, [d][i][j][24]
    int* status;
};

// chain position of (tap t, channel ci) in the K sequence of pc_mfma_kernel<24, ...>: 2 * (4 * ((ci / 8) * 14 + t) + (ci % 8) / 2) + ci % 2
__device__ __forceinline__ int pc_chain_idx(int t, int ci) { return 8 * ((ci >> 3) * PC_NT + t) + (ci & 7); }

// The decoder of ONE volume by ONE work-group: the body of pc_dec_cached_kernel (a whole volume) and of pc_dec_tiles_batch_kernel
// (one tile of a volume per work-group).  f holds what all volumes of a launch share (weights, centres, C, L, resolution); the volume
// being decoded -- stream, extents, first symbol, padded volume, caches, status -- comes as plain values, so that a kernel can
// take them from a table without a private copy of the struct (which would live in scratch).  Symbol (c, y, x) is stored at
// out[c * out_cs + y * out_rs + x]: out_cs = h * w, out_rs = w for a whole volume; the strides of the full volume, and out
// moved to the tile's corner, for a tile.
// SYMS = false (ic_pc_decode_tiles_batch_f32 with symbols == NULL): nothing is stored through out; the padded volume still
// receives every symbol's centre, which is what that caller copies out.
// LIM = true (the *_channels entries, preview): only channels 0 .. cdec - 1 are decoded, 1 <= cdec < C (cdec == C, a tile of the per-tile entry that is whole, is the full sweep).  The stream codes its symbols
// in (c, y, x) order and the masks are causal in c, so these are a prefix of the stream and the sweep simply ends after plane
// D = cdec + 3; nothing of the per-symbol path changes, and the strides of the caches and of V do not depend on C.  cdec is a plain,
// uniform value like the others (not a patched copy of f, see above); LIM = false does not read it and is the full decoder as before.
// SEG = true (ic_pc_decode_tiles_batch_layers_f32, container format 6): the stream is cut at channel planes into nlayers segments,
// each a coder run of its own.  bits / nbytes are segment 0; segment g >= 1 is segs[g] (offsets from seg_base) and begins with the
// first symbol of channel ends[g - 1].  The step that decodes that symbol -- D - 4 == ends[g - 1], I == 4, J == 3 -- is the cut: wave
// 0 folds s.error into a sticky word, re-initialises the coder state on segment g and reads the 32 code bits, exactly as at the
// start of a stream; the sweep, the caches and the context know nothing of it.  Past its end a segment reads as zeros (its own
// nbytes bounds pc_dec_bit).  segs and ends are the tile's rows of device tables in the workspace, the index is uniform: scalar
// loads, a handful per tile, and no per-lane copy of either table.  With LIM the sweep ends before the cuts of the layers that
// begin at or above cdec: their segments are never read.  SEG = false reads none of this and is the decoder as before.
// FROM = true (ic_pc_decode_tiles_batch_layers_resume_f32; only with LIM && SEG): gfrom is the layer the tile continues with, uniform
// like cdec.  gfrom == 0 is the sweep from the start.  gfrom > 0: an earlier launch has swept this tile up to plane D = cfrom + 3 with
// cfrom = ends[gfrom - 1] and has left V and the caches in the slot; this sweep begins at the step behind that one's last and runs up
// to plane cdec + 3 > cfrom + 3.  FROM = false reads none of this and is the decoder as before.
template <bool SYMS = true, bool LIM = false, bool SEG = false, bool FROM = false>
__device__ __forceinline__ void pc_dec_cached_body(const PcCachedArgs& f, const unsigned char* bits, long long nbytes, int h, int w, int first_sym,
                                                   float* vol, float* c0, float* c1, float* c2, int* status,
                                                   long long* __restrict__ out, long long out_cs, int out_rs, int cdec = 0,
                                                   const unsigned char* seg_base = nullptr, const ic_pc_seg_t* __restrict__ segs = nullptr,
                                                   const int* __restrict__ ends = nullptr, int nlayers = 0, int gfrom = 0) {
    static_assert(!FROM || (LIM && SEG), "a sweep continues at a layer cut of a limited sweep");
    constexpr int K = 24, KT = PC_NT * K;                 // 336 inputs per output
    __shared__ __attribute__((aligned(16))) float s_in[3][KT];          // inputs of conv1 / conv2 / conv3 in chain order
    __shared__ __attribute__((aligned(16))) float s_v[16];              // the 13 live taps of conv0
    __shared__ float s_part[2][4][64];
    __shared__ float s_centers[16];
    const PcDecArgs& a = f.d;                             // centres, C, L, resolution: what all volumes of a launch share
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int L = a.L;
    // ---- per-lane constants ----
    const int grp = lane < 24 ? 0 : (lane < 48 ? 1 : 2), co = lane - (grp == 2 ? 48 : 24 * grp), co0 = lane % 24;
    const int cout_g = grp == 2 ? L : K;
    const float* wl = grp == 0 ? f.w1 : (grp == 1 ? f.w2 : f.w3);
    float wreg[84];
#pragma unroll
    for (int n = 0; n < 84; ++n) {
        const int g = 42 * wave + (n >> 1), ts = g >> 2, c8 = ts / PC_NT, t = ts - c8 * PC_NT;
        const int ci = 8 * c8 + 2 * (g & 3) + (n & 1);
        const int tap = (pc_tap_kd(t) * 3 + pc_tap_kh(t)) * 3 + pc_tap_kw(t);
        wreg[n] = co < cout_g ? wl[((size_t)tap * K + ci) * cout_g + co] : 0.f;
    }
    float w0reg[13];
#pragma unroll
    for (int lt = 0; lt < 13; ++lt) w0reg[lt] = f.w0[lt * K + co0];     // live taps of the first mask are TF taps 0..12
    const float bias0 = f.b0[co0];
    const float bias_l = grp == 0 ? f.b1[co] : (grp == 1 ? f.b2[co] : (co < L ? f.b3[co] : 0.f));
    if (tid < L) s_centers[tid] = a.centers[tid];
    const float pad = a.centers[0];
    // ---- prefetch role: thread -> (layer pl, tap t < 12, channel quad q), and the conv0 taps on threads 0..11 ----
    const int pl = tid / 84, pe = tid - pl * 84, pt = pe / 6, pq = pe - pt * 6;
    const bool pf_on = tid < 252 && pt < 12;
    const int pkd = pt < 9 ? 0 : 1, pkh = pt < 9 ? pt / 3 : 0, pkw = pt < 9 ? pt % 3 : pt - 9;
    const int ni = h + 6 - 2 * pl, nj = w + 6 - 2 * pl;
    const float* cpl = pl == 0 ? c0 : (pl == 1 ? c1 : c2);
    const int pdst = 8 * ((pq >> 1) * PC_NT + pt) + 4 * (pq & 1);      // chain position of channels 4 pq .. 4 pq + 3 of tap pt
    const int vkd = tid < 9 ? 0 : 1, vkh = tid < 9 ? tid / 3 : 0, vkw = tid < 9 ? tid % 3 : tid - 9;
    const int PH = h + 8, PW = w + 8;
    const int D1 = (LIM ? cdec : a.C) + 3, I1 = h + 6, J1 = w + 5;       // last D, I, J of the sweep
    auto layer_valid = [&](int l, int D, int I, int J) -> bool {     // does step (D, I, J) produce a voxel of layer l + 1?
        return D >= 2 + l && I >= 2 + l && J >= 1 + l && I <= h + 5 - l && J <= w + 4 - l;
    };
    pc_f32x4 pf = {0.f, 0.f, 0.f, 0.f};
    float pv = pad;
    auto prefetch = [&](int D, int I, int J) {
        if (pf_on && layer_valid(pl, D, I, J)) {
            const int off = (((D - 2 - pl + pkd) * ni + (I - 2 - pl + pkh)) * nj + (J - 1 - pl + pkw)) * K + 4 * pq;
            pf = *reinterpret_cast<const pc_f32x4*>(cpl + off);
        }
        if (tid < 12) pv = vol[((size_t)(D - 1 + vkd) * PH + (I - 1 + vkh)) * PW + J + vkw];
    };
    typedef const __attribute__((address_space(4))) ic_pc_seg_t* seg_cptr;
    typedef const __attribute__((address_space(4))) int* int_cptr;
    // FROM, gfrom > 0: the sweep continues at (cfrom + 4, 1, 0), the step behind the last one, (cfrom + 3, h + 6, w + 5), of the sweep
    // that stopped at channel cfrom.  Nothing of that sweep's LDS or registers is needed: at J = 0 no layer is valid (layer_valid asks
    // J >= 1 + l), so the step produces no cache voxel and no logits, and what it reads of s_in -- the tap-12 slots it never wrote
    // included -- flows into nothing that is kept, exactly as at (1, 1, 0) of a fresh sweep and at the first step of every row; the
    // tap-12 carry into J = 1 is this step's own A0 voxel.  V[D][1][0] is pad as at a fresh start.  The coder needs no state either:
    // the first symbol of channel cfrom, at (cfrom + 4, 4, 3), is the cut that initialises it on segment gfrom, and no step before
    // that one decodes.  So segment 0 is neither initialised from nor read: s holds a coder at rest until the cut.
    bool resumed = false;
    int cfrom = 0;
    if constexpr (FROM) {
        resumed = gfrom > 0;
        if (resumed) cfrom = ((int_cptr)ends)[gfrom - 1];
    }
    PcDecState s;                                         // wave 0 keeps the coder state, identical in all its lanes
    if (!resumed) {
        pc_dec_state_init(s, bits, nbytes);
        if (wave == 0)
            for (int i = 0; i < PC_AC_BITS; ++i) s.code = (s.code << 1) | (unsigned)pc_dec_bit(bits, nbytes, s);
    } else {
        s.low = 0; s.high = (1ull << PC_AC_BITS) - 1; s.code = 0;
        s.byte_pos = -1; s.bit_left = 0; s.cur_byte = 0; s.nxt_byte = 0; s.error = 0; s.next = 1;
    }
    if (tid == 0) s_v[12] = pad;                          // V[1][1][0]; resumed: V[cfrom + 4][1][0]
    // SEG: the layer whose segment comes next, the channel it begins with (-1: none left), and the sticky error of the segments done
    // (the two tables were written by the copies that precede the launch and nothing in the kernel stores to them: they are read
    // through the constant address space, which is what lets a uniform index become a scalar load behind the kernel's own stores)
    int seg_next = 1, seg_cut = -1, sticky = 0;
    if constexpr (SEG) seg_cut = nlayers > 1 ? ((int_cptr)ends)[0] : -1;
    if constexpr (FROM) if (resumed) { seg_next = gfrom; seg_cut = cfrom; }      // the next cut is the first symbol this sweep decodes
    // LDS hand-over between the waves: wait for this wave's LDS operations only.  (__syncthreads() also waits for the global
    // stores of the cache voxels to be acknowledged; their readers are a row of steps away and every wave drains its
    // memory counter at the top of each step, where it consumes its prefetch.)
    auto lds_barrier = []() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); };
    int D = 1, I = 1, J = 0;
    if constexpr (FROM) if (resumed) D = cfrom + 4;
    prefetch(D, I, J);
    // one chain pass: this wave's part of the K sequence for the output this lane holds the weights of
    auto chain = [&](const float* in) -> float {
        const pc_f32x4* in4 = reinterpret_cast<const pc_f32x4*>(in + 84 * wave);
        float acc = 0.f;
#pragma unroll
        for (int n4 = 0; n4 < 21; ++n4) {
            const pc_f32x4 v = in4[n4];
            acc = fmaf(wreg[4 * n4], v[0], acc); acc = fmaf(wreg[4 * n4 + 1], v[1], acc);
            acc = fmaf(wreg[4 * n4 + 2], v[2], acc); acc = fmaf(wreg[4 * n4 + 3], v[3], acc);
        }
        return acc;
    };
#ifdef PC_DEC_PROF
    unsigned long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tl = __builtin_amdgcn_s_memtime();
#endif
    for (;;) {
        PC_PH(6);
        // ---- the prefetched taps of this step -> LDS ----
        if (pf_on) *reinterpret_cast<pc_f32x4*>(&s_in[pl][pdst]) = pf;
        if (tid < 12) s_v[tid] = pv;
        lds_barrier();                                    // also: s_v[12] from the previous step's decode
        PC_PH(0);
        const bool v1 = layer_valid(0, D, I, J), v2 = layer_valid(1, D, I, J), v3 = layer_valid(2, D, I, J);
        // ---- conv0: every lane computes channel lane % 24 (so lane 24 + c holds the skip operand of conv2's output c) ----
        float a0 = 0.f;
        {
            const pc_f32x4* v4 = reinterpret_cast<const pc_f32x4*>(s_v);
            const pc_f32x4 va = v4[0], vb = v4[1], vc = v4[2], vd = v4[3];
            const float vv[13] = {va[0], va[1], va[2], va[3], vb[0], vb[1], vb[2], vb[3], vc[0], vc[1], vc[2], vc[3], vd[0]};
#pragma unroll
            for (int lt = 0; lt < 13; ++lt) a0 = fmaf(vv[lt], w0reg[lt], a0);
        }
        a0 = fmaxf(a0 + bias0, 0.f);
        if (lane < K) {
            s_in[0][pc_chain_idx(13, lane)] = a0;         // every wave writes the same value: no barrier before its own reads
            if (wave == 0) c0[(((size_t)(D - 1) * (h + 6) + (I - 1)) * (w + 6) + J) * K + lane] = a0;
        }
        PC_PH(1);
        // ---- conv1 ----
        s_part[0][wave][lane] = chain(s_in[0]);
        lds_barrier();
        if (grp == 0) {
            const float v = (s_part[0][0][lane] + s_part[0][1][lane]) + (s_part[0][2][lane] + s_part[0][3][lane]);
            const float a1 = fmaxf(v + bias_l, 0.f);
            s_in[1][pc_chain_idx(13, co)] = a1;
            if (wave == 0 && v1) c1[(((size_t)(D - 2) * (h + 4) + (I - 2)) * (w + 4) + (J - 1)) * K + co] = a1;
        }
        PC_PH(2);
        // ---- conv2 + skip ----
        s_part[1][wave][lane] = chain(s_in[1]);
        lds_barrier();
        if (grp == 1) {
            const float v = (s_part[1][0][lane] + s_part[1][1][lane]) + (s_part[1][2][lane] + s_part[1][3][lane]);
            float a2 = v + bias_l;
            a2 += a0;
            s_in[2][pc_chain_idx(13, co)] = a2;
            if (wave == 0 && v2) c2[(((size_t)(D - 3) * (h + 2) + (I - 3)) * (w + 2) + (J - 2)) * K + co] = a2;
        }
        PC_PH(3);
        // ---- conv3 -> logits of the symbol at V[D][I][J + 1] ----
        float logit = 0.f;
        if (v3) {
            s_part[0][wave][lane] = chain(s_in[2]);
            lds_barrier();
            const float v = (s_part[0][0][lane] + s_part[0][1][lane]) + (s_part[0][2][lane] + s_part[0][3][lane]);
            logit = fmaxf(v + bias_l, 0.f);
        }
        PC_PH(4);
        // next step's coordinates
        int Dn = D, In = I, Jn = J + 1;
        if (Jn > J1) { Jn = 0; if (++In > I1) { In = 1; ++Dn; } }
        if (wave == 0) {
            float vnext = pad;
            if (v3) {
                const bool first = D == 4 && I == 4 && J == 3;                  // the first symbol is not coded
                if constexpr (SEG) {
                    if (I == 4 && J == 3 && D - 4 == seg_cut) {                 // the cut: this symbol is the first of segment seg_next
                        seg_next = __builtin_amdgcn_readfirstlane(seg_next);
                        const long long seg_off = ((seg_cptr)segs)[seg_next].off, seg_bytes = ((seg_cptr)segs)[seg_next].nbytes;
                        sticky |= s.error;
                        bits = seg_base + seg_off; nbytes = seg_bytes;
                        pc_dec_state_init(s, bits, nbytes);
                        for (int i = 0; i < PC_AC_BITS; ++i) s.code = (s.code << 1) | (unsigned)pc_dec_bit(bits, nbytes, s);
                        ++seg_next;
                        seg_cut = seg_next < nlayers ? ((int_cptr)ends)[seg_next - 1] : -1;
                    }
                }
                const int sym = first ? first_sym : (L == 6 ? pc_dec_symbol_wave<6>(bits, nbytes, L, a.resolution, s, logit) : pc_dec_symbol_wave<0>(bits, nbytes, L, a.resolution, s, logit));
                vnext = s_centers[sym];
                if (lane == 0) {
                    if (SYMS) out[(long long)(D - 4) * out_cs + (long long)(I - 4) * out_rs + (J - 3)] = sym;
                    vol[((size_t)D * PH + I) * PW + J + 1] = vnext;
                }
            }
            if (lane == 0) s_v[12] = vnext;               // V at the next step's position (pad outside the symbol volume)
        }
        PC_PH(5);
        if (Dn > D1) break;
        // (1,1,0) taps of the next step = this step's voxels: centre slot -> tap-12 slot
        if (tid >= 64 && tid < 64 + 3 * K) {
            const int e = tid - 64, l2 = e / K, c = e - l2 * K;
            s_in[l2][pc_chain_idx(12, c)] = s_in[l2][pc_chain_idx(13, c)];
        }
        D = Dn; I = In; J = Jn;
        prefetch(D, I, J);
    }
    if (tid == 0) *status = SEG ? (sticky | s.error) : s.error;
#ifdef PC_DEC_PROF
    if (tid == 0) printf("pc_dec_cached phases (clocks, thread 0): wait+stage %llu | conv0 %llu | conv1 %llu | conv2 %llu | conv3 %llu | decode %llu | tail+prefetch issue %llu\n",
                         ph[0], ph[1], ph[2], ph[3], ph[4], ph[5], ph[6]);
#endif
}

__global__ __launch_bounds__(256) void pc_dec_cached_kernel(const PcCachedArgs f) {
    pc_dec_cached_body(f, f.d.bits, f.d.nbytes, f.d.h, f.d.w, f.d.first_sym, f.d.vol, f.c0, f.c1, f.c2, f.status,
                       f.d.symbols, (long long)f.d.h * f.d.w, f.d.w);
}

// the first cdec < C channels of one volume (ic_pc_decode_channels_f32): the sweep stops after them, then the same work-group
// writes `fill` into the channels it did not decode -- every position of `symbols` is written
__global__ __launch_bounds__(256) void pc_dec_cached_channels_kernel(const PcCachedArgs f, const int cdec, const int fill) {
    pc_dec_cached_body<true, true>(f, f.d.bits, f.d.nbytes, f.d.h, f.d.w, f.d.first_sym, f.d.vol, f.c0, f.c1, f.c2, f.status,
                                   f.d.symbols, (long long)f.d.h * f.d.w, f.d.w, cdec);
    const long long plane = (long long)f.d.h * f.d.w, n = (long long)(f.d.C - cdec) * plane;
    long long* rest = f.d.symbols + (long long)cdec * plane;
    for (long long i = threadIdx.x; i < n; i += 256) rest[i] = fill;
}

// ---- wavefront-ordered tiles (container format 5, IC_PC_DECODE_WAVEFRONT) ----------------------------------------------------
// The four masked layers make symbol (c, y, x) depend only on symbols of strictly smaller T = x + 2 y + 4 c (codec.py derives
// this from the masks), so a stream that codes a tile front by front -- all symbols of one T, in (c, y, x) order -- lets the
// decoder evaluate the network for a whole front at once; only the range decoder's step per symbol stays serial.
// Same work mapping and workspace slot as pc_dec_cached_body (one work-group per tile: padded volume V and the caches A0, A1,
// A2, channels-last), but the sweep runs over hyperplanes of the padded volume, T = J + 2 I + 4 D.  The last live tap of a
// window has the largest T of its taps: offset 7 for the (1,1,1) corner of the "other" mask, 6 for the first mask (three taps
// share it, all of them V).  With every V of T' < T known, step T runs four phases behind barriers:
//     1. A0 voxels of front T - 7      (taps: V up to front T - 1)
//     2. A1 voxels of front T - 14     (taps: A0 up to front T - 7)
//     3. A2 voxels of front T - 21     (taps: A1 up to front T - 14; skip operand A0[d+2][i+2][j+2] on front T - 7)
//     4. logits of the symbols on front T of V (taps: A2 up to front T - 21), 64 candidates at a time into LDS,
// then wave 0 decodes that chunk's symbols one after the other with pc_dec_symbol_wave and stores their centres into V.
// Every cache voxel a later phase reads -- halo voxels included -- is written exactly once, at the step its front comes up,
// before its first read; voxels whose front lies beyond the last symbol's are never read and never written.
// Each phase is parallel over (voxel, group of output channels).  One output is the four fmaf chains of pc_mfma_kernel's K
// sequence (pc_chain_idx order, cut at 84 = 42 channel pairs), summed (p0 + p1) + (p2 + p3), then bias / ReLU / skip exactly as
// pc_dec_cached_body does: the logits are bit-identical to the parallel pass, which the tables are a function of.

// the voxels (d, i, j) of a box ND x NI x NJ with j + 2 i + 4 d == S as a dense range of candidates e in [0, nd * iw): d ascending,
// then i ascending (j follows), so the candidates that are voxels come in (d, i, j) order
struct PcFront { int S, NI, NJ, d_lo, nd, iw; };
__device__ __forceinline__ int pc_cdiv_pos(int n, int k) { return n <= 0 ? 0 : (n + k - 1) / k; }
__device__ __forceinline__ PcFront pc_front(int S, int ND, int NI, int NJ) {
    PcFront f;
    f.S = S; f.NI = NI; f.NJ = NJ;
    f.d_lo = pc_cdiv_pos(S - (NJ - 1) - 2 * (NI - 1), 4);
    const int d_hi = min(ND - 1, S >> 2);
    f.nd = S < 0 ? 0 : max(d_hi - f.d_lo + 1, 0);
    f.iw = min(NI, (NJ + 1) >> 1);                         // no d has more voxels on one front
    return f;
}
__device__ __forceinline__ bool pc_front_voxel(const PcFront& f, int e, int& d, int& i, int& j) {
    const int dd = e / f.iw, ii = e - dd * f.iw;
    d = f.d_lo + dd;
    const int R = f.S - 4 * d;                             // >= 0: d <= S / 4
    i = pc_cdiv_pos(R - (f.NJ - 1), 2) + ii;               // the smallest i with j <= NJ - 1, then upwards
    j = R - 2 * i;
    return i < f.NI && j >= 0;
}

// COB outputs (channels co0 .. co0 + COB - 1 of a layer with `cout` outputs, w already moved to co0) of the voxel whose window
// starts at `in` in a channels-last cache of row stride NJ and plane stride NI * NJ voxels
template <int COB>
__device__ __forceinline__ void pc_wave_chain(const float* __restrict__ in, int NI, int NJ, const float* __restrict__ w, int cout,
                                              float (&v)[COB]) {
    constexpr int K = 24;
    static_assert(COB == 1 || COB == 4, "one output, or four through 16-byte filter loads");
    float acc[PC_NP][COB];
#pragma unroll
    for (int p = 0; p < PC_NP; ++p)
#pragma unroll
        for (int r = 0; r < COB; ++r) acc[p][r] = 0.f;
    const int rs = NJ * K, ds = NI * rs;
    // a part is 21 steps of four chain positions, 8 * (c8 * 14 + t) + 4 * half + c; the parts are unrolled (their accumulators are
    // registers), the steps inside one are a loop of uniform address arithmetic: unrolled as a whole, the 420 loads of one output
    // group are hoisted together and spill
#pragma unroll
    for (int part = 0; part < PC_NP; ++part) {
#pragma unroll 3
        for (int uu = 0; uu < 21; ++uu) {
            const int u = 21 * part + uu, c8 = u / 28, t = (u - 28 * c8) >> 1, ci0 = 8 * c8 + 4 * (u & 1);
            // live tap t of the "other" mask is TF tap t: (kd, kh, kw) = (0, t / 3, t % 3), (1, 0, t - 9), (1, 1, t - 12)
            const int kd = t >= 9 ? 1 : 0, kh = t < 9 ? t / 3 : (t < 12 ? 0 : 1), kw = t < 9 ? t - 3 * kh : (t < 12 ? t - 9 : t - 12);
            const pc_f32x4 x = *reinterpret_cast<const pc_f32x4*>(in + kd * ds + kh * rs + kw * K + ci0);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float* wp = w + (t * K + ci0 + c) * cout;
                if constexpr (COB == 4) {
                    const pc_f32x4 wv = *reinterpret_cast<const pc_f32x4*>(wp);
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[part][r] = fmaf(wv[r], x[c], acc[part][r]);
                } else {
                    acc[part][0] = fmaf(wp[0], x[c], acc[part][0]);
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < COB; ++r) v[r] = (acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r]);
}

// LIM = true (preview of the first cdec < C channels): the loop ends at the front of the last symbol of channel cdec - 1,
// T_stop = (w + 3) + 2 (h + 3) + 4 (cdec + 3).  A front <= T_stop also holds symbols of channels >= cdec, and the stream has them
// in between the others: the range decoder steps through them like through any symbol, their centres go into V (later fronts of
// the wanted channels have them in their context) and every cache phase keeps its full depth range; they are only not stored
// through out.  The symbols stepped through are the first codec.wavefront_prefix_count(C, h, w, cdec) of the stream's order.
// SEG = true (the *_fronts entries, container format 8): the stream is cut into nlayers segments, each a coder run of its own -- not at
// channel planes, which are no prefix of this order, but at FRONTS: segment g ends with the last symbol of front
// t_g = (w - 1) + 2 (h - 1) + 4 (ends[g] - 1), the front of the last symbol of channel ends[g] - 1 (this tile's own h, w), so the segments
// 0 .. g are exactly what a LIM sweep with cdec = ends[g] steps through.  bits / nbytes are segment 0; segment g >= 1 is segs[g] (offsets
// from seg_base).  When phase 4 first comes to a front above t_g -- T - 28 > t_g, before that front's first symbol -- wave 0 folds
// s.error into a sticky word, re-initialises the coder state on segment g + 1 and reads the 32 code bits, exactly as at the start of
// a stream: a wave-uniform branch between the barrier behind phase 3 and the one behind the chunk's logits, where wave 0 has no other
// work that anyone waits for.  The cuts lie at least four fronts apart (the ends increase), a step advances one front: one cut per
// step at the most.  The fronts, the caches and the context know nothing of it; LDS does not grow.  Past its end a segment reads as
// zeros (its own nbytes bounds pc_dec_bit).  segs and ends are the tile's rows of device tables that no kernel writes, read through
// the constant address space with uniform indices: scalar loads.  With LIM the loop ends at T_stop(cdec) before it comes to a front
// above t_g of any layer that ends at or above cdec: only the segments of layers that begin below cdec are read.  Everything a later
// front needs -- V and the three caches -- is in the slot and the coder starts afresh at each cut, so a sweep that stopped at a layer
// end could be continued by a later launch, as the raster FROM sweep is.  SEG = false reads none of this and is the decoder as before.
// FROM = true (ic_pc_decode_tiles_batch_fronts_resume_f32; only with LIM && SEG): gfrom is the layer the tile continues with, uniform
// like cdec.  gfrom == 0 is the sweep from the start.  gfrom > 0: an earlier launch has run this tile's loop up to T = T_base + 4 cfrom,
// cfrom = ends[gfrom - 1] -- the T_cut of layer gfrom - 1 -- and has left V and the caches in the slot; this loop runs
// T = T_base + 4 cfrom + 1 .. T_last(cdec).  Nothing of that launch's LDS or registers is needed.  s_logits is written and read within a
// chunk and s_centers is loaded again.  A step reads V and the caches at fronts below its own only (T - 1, T - 7, T - 14, T - 21 and less):
// phases 1 - 3 of the first step read voxels of earlier steps, which are in the slot whichever launch ran them, and write the voxels of
// fronts T - 7, T - 14, T - 21, which no earlier step wrote.  The coder needs no state: the first step has T > T_cut, so the cut branch in
// front of phase 4 initialises it on segment gfrom before the first symbol is decoded, exactly as in the middle of a sweep.  Until then
// s holds a coder at rest, and no segment below gfrom -- segment 0 included -- is initialised from or read.
// What the raster FROM sweep does not have to carry: the sweep to cfrom has stepped through symbols of channels >= cfrom (those that
// share its fronts).  Their centres are in V, but they were not stored through out and this sweep does not come to them again.  So the
// FROM sweeps keep every symbol they decode in `plane`, a byte per symbol in the slot's part of the workspace, (c, y, x) order of
// the tile, and store nothing through out: the caller copies [cfrom, cdec) out of the plane behind the body.  A byte of the plane is
// only ever copied out, never used as an index.  FROM = false reads none of this and is the decoder as before.
// DEPTH = true (IC_PC_DECODE_DEPTH, container format 10; only with LIM, without SEG): the stream holds the LIVE positions only,
// c < depth[(y / dblock) * dnbx + x / dblock] (a byte above C counts as C); `depth` is the tile's plane, which the caller has taken off
// the front of the stream (bits / nbytes are the coder's part), dmax its largest entry after the clamp, >= 1, and cdec =
// min(channels, dmax).  No channel at or above dmax has a live position and none of them is in the context of a lower one (the masks
// are causal in c), so the whole sweep -- cache phases and candidates -- runs over dmax channels in place of C.  Liveness is decided in
// the parallel part of a chunk: the lanes of a dead slot compute no logits, the lane that owns the slot (co == 0) stores `fill`
// through out and its centre into V there and then, and leaves a byte in s_live for wave 0, whose serial loop only steps over the
// slot -- the plane is never read between two coder steps.  The first position is uncoded as ever; dead, it is `fill` like any other.
// RANS = true (IC_PC_DECODE_RANS(W), container format 12; only with LIM, without SEG, FROM and DEPTH): the stream is that of W
// interleaved rANS coders (imgcomp_hip.h), coder = candidate index mod W.  Phases 1 - 3 and the logits of a chunk of CH candidates
// are the decoder's as before; behind the chunk's barrier wave 0 does not step a coder through the chunk symbol by symbol
// (pc_dec_symbol_wave is not on this path) but
//   - lane k builds the table of slot k from s_logits[k] -- pc_table_row, then pc_rans_row -- and stores its prefix sums back in
//     place as integers (a chunk starts at a multiple of CH, so slot k belongs to coder k mod W);
//   - in CH / W sub-rounds lanes l < W each decode the symbol of slot s W + l from their own state, take one 16-bit word if the
//     state fell below 2^16 -- the lanes that need one take consecutive words in lane order, addressed with a ballot and a prefix
//     count from the wave-uniform number of words taken, every byte read only below nbytes -- and store their own symbol through
//     out and its centre into V.  A slot that is no position costs an idle lane and no word.
// Every trip count is fixed by the tile's geometry and W; nothing waits on anything; a symbol is < L whatever the bytes are, because
// the table's sums end at M.  At the end of a full decode (cdec == C) the states must all be 2^16 and the words taken must end the
// stream: else status 4, OR-ed with status 1 of a table whose total was too large.
// RDO = true (IC_PC_DECODE_RDO; only with LIM and cdec == C, without SEG, FROM, DEPTH and RANS): not a decoder but the encoder's
// rate-aware symbol CHOOSER, the same sweep with nothing to read symbols from.  bits / nbytes are the tile's record (imgcomp_hip.h):
// lam as an f64, then the tile's masked bottleneck values z, f32 in (c, y, x) order; the caller has checked its length and its
// alignment.  Phases 1 - 3 and the logits of a chunk are the decoder's as before; behind the chunk's barrier lane k < nc of wave 0
// decides slot k by pc_rdo_pick -- the slot's table row, the integer log2 of its entries, z, the first minimum of distortion +
// lam * rate -- and stores its symbol through out and its centre into V, where the later fronts' contexts find it.  The positions
// of a front do not see each other (a context holds smaller T only), so the lanes of a chunk and the chunks of a front are
// independent: no serial part, no coder state, no pc_dec_symbol_wave, no read outside the record.  Every trip count is fixed by the
// tile's geometry.  first_sym is not read.  status: 1 if a table's total was too large (that position is decided by distortion alone).
template <int LC>
__device__ __forceinline__ bool pc_dec_rans_build(float (*row)[16], int slot, float resolution) {
    float l[LC];
#pragma unroll
    for (int j = 0; j < LC; ++j) l[j] = row[slot][j];
    unsigned cum[LC];
    const bool ok = pc_rans_row<LC>(l, resolution, cum);
    unsigned* o = reinterpret_cast<unsigned*>(row[slot]);
#pragma unroll
    for (int j = 0; j < 16; ++j) o[j] = j < LC ? cum[j < LC ? j : 0] : PC_RANS_M;
    return ok;
}

template <bool SYMS, bool LIM = false, bool SEG = false, bool FROM = false, bool DEPTH = false, bool RANS = false, bool RDO = false>
__device__ __forceinline__ void pc_dec_wave_body(const PcCachedArgs& f, const unsigned char* bits, long long nbytes, int h, int w, int first_sym,
                                                 float* vol, float* c0, float* c1, float* c2, int* status,
                                                 long long* __restrict__ out, long long out_cs, int out_rs, int cdec = 0,
                                                 const unsigned char* seg_base = nullptr, const ic_pc_seg_t* __restrict__ segs = nullptr,
                                                 const int* __restrict__ ends = nullptr, int nlayers = 0, int gfrom = 0,
                                                 unsigned char* __restrict__ plane = nullptr,
                                                 const unsigned char* __restrict__ depth = nullptr, int dblock = 1, int dnbx = 0, int dmax = 0,
                                                 int fill = 0, int rlanes = 0) {
    static_assert(!FROM || (LIM && SEG), "a sweep continues at a layer cut of a limited sweep");
    static_assert(!DEPTH || (LIM && !SEG), "the depth plane belongs to the unsegmented limited sweep");
    static_assert(!RANS || (LIM && !SEG && !FROM && !DEPTH), "the interleaved coders belong to the unsegmented limited sweep");
    static_assert(!RDO || (LIM && !SEG && !FROM && !DEPTH && !RANS), "the symbol chooser is the unsegmented limited sweep without a coder");
    constexpr int K = 24, G = K / 4, CH = 64;             // CH: candidates of a front whose logits are in LDS at once
    __shared__ float s_logits[CH + (DEPTH ? 1 : 0)][16];  // DEPTH: one more row, CH bytes: s_live
    __shared__ float s_centers[16];
    static_assert(sizeof(float) * 16 == CH, "s_live is one row of s_logits");
    unsigned char* const s_live = reinterpret_cast<unsigned char*>(s_logits[DEPTH ? CH : 0]);       // (read and written with DEPTH only)
    const PcDecArgs& a = f.d;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int L = a.L, C = DEPTH ? dmax : a.C;            // DEPTH: the channels that hold anything
    if (tid < L) s_centers[tid] = a.centers[tid];
    bool resumed = false;
    int cfrom = 0;
    if constexpr (FROM) {
        resumed = gfrom > 0;
        if (resumed) cfrom = ((const __attribute__((address_space(4))) int*)ends)[gfrom - 1];
    }
    PcDecState s;                                         // wave 0 keeps the coder state, identical in all its lanes
    // RANS: wave 0, lane l < W keeps coder l's state; the words taken so far and the status are wave-uniform / per lane
    unsigned rx = 0;
    long long rtaken = 0;
    int rerr = 0;
    // RDO: the record's lam and z (uniform addresses; lam is a scalar load)
    double rlam = 0.0;
    const float* rz = nullptr;
    if constexpr (RDO) {
        s.error = 0;
        rlam = *reinterpret_cast<const double*>(bits);
        rz = reinterpret_cast<const float*>(bits + 8);
    } else
    if constexpr (RANS) {
        s.error = 0;
        if (wave == 0 && lane < rlanes) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const long long o = 4ll * lane + i;
                rx |= (o < nbytes ? (unsigned)bits[o] : 0u) << (8 * i);
            }
        }
    } else if (!resumed) {
        pc_dec_state_init(s, bits, nbytes);
        if (wave == 0)
            for (int i = 0; i < PC_AC_BITS; ++i) s.code = (s.code << 1) | (unsigned)pc_dec_bit(bits, nbytes, s);
    } else {                                              // a coder at rest: the first step's cut initialises it on segment gfrom
        s.low = 0; s.high = (1ull << PC_AC_BITS) - 1; s.code = 0;
        s.byte_pos = -1; s.bit_left = 0; s.cur_byte = 0; s.nxt_byte = 0; s.error = 0; s.next = 1;
    }
    const int PH = h + 8, PW = w + 8;
    const int N0i = h + 6, N0j = w + 6, N1i = h + 4, N1j = w + 4, N2i = h + 2, N2j = w + 2;
    const int T_last = (w + 3) + 2 * (h + 3) + 4 * ((LIM ? cdec : C) + 3);    // the last symbol's front (LIM: of channel cdec - 1)
    // SEG: the segment that comes next, the last front of the one being read (in the loop's terms, T = front + 28; none left: beyond the
    // sweep), and the sticky error of the segments done
    typedef const __attribute__((address_space(4))) ic_pc_seg_t* seg_cptr;
    typedef const __attribute__((address_space(4))) int* int_cptr;
    const int T_base = (w - 1) + 2 * (h - 1) - 4 + 28;                        // T of front t_g is T_base + 4 ends[g]
    int seg_next = 1, T_cut = 0x7fffffff, sticky = 0;
    if constexpr (SEG) T_cut = nlayers > 1 ? T_base + 4 * ((int_cptr)ends)[0] : 0x7fffffff;
    int T_first = 7;
    if constexpr (FROM) if (resumed) { seg_next = gfrom; T_cut = T_base + 4 * cfrom; T_first = T_cut + 1; }
    __syncthreads();
    for (int T = T_first; T <= T_last; ++T) {
        {   // ---- 1: A0, first mask (13 live taps = TF taps 0..12), + bias, ReLU ----
            const PcFront fr = pc_front(T - 7, C + 3, N0i, N0j);
            for (int n = tid; n < fr.nd * fr.iw * G; n += 256) {
                const int e = n / G, cg = n - e * G;
                int d, i, j;
                if (!pc_front_voxel(fr, e, d, i, j)) continue;
                const float* vp = vol + ((size_t)d * PH + i) * PW + j;
                float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int lt = 0; lt < 13; ++lt) {
                    const int kd = lt < 9 ? 0 : 1, kh = lt < 9 ? lt / 3 : (lt < 12 ? 0 : 1), kw = lt < 9 ? lt % 3 : (lt < 12 ? lt - 9 : 0);
                    const float xv = vp[(kd * PH + kh) * PW + kw];
                    const pc_f32x4 wv = *reinterpret_cast<const pc_f32x4*>(f.w0 + lt * K + 4 * cg);
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[r] = fmaf(xv, wv[r], acc[r]);
                }
                const pc_f32x4 b = *reinterpret_cast<const pc_f32x4*>(f.b0 + 4 * cg);
                pc_f32x4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = fmaxf(acc[r] + b[r], 0.f);
                *reinterpret_cast<pc_f32x4*>(c0 + (((size_t)d * N0i + i) * N0j + j) * K + 4 * cg) = o;
            }
        }
        __syncthreads();
        {   // ---- 2: A1 = relu(conv1(A0) + bias) ----
            const PcFront fr = pc_front(T - 14, C + 2, N1i, N1j);
            for (int n = tid; n < fr.nd * fr.iw * G; n += 256) {
                const int e = n / G, cg = n - e * G;
                int d, i, j;
                if (!pc_front_voxel(fr, e, d, i, j)) continue;
                float v[4];
                pc_wave_chain<4>(c0 + (((size_t)d * N0i + i) * N0j + j) * K, N0i, N0j, f.w1 + 4 * cg, K, v);
                const pc_f32x4 b = *reinterpret_cast<const pc_f32x4*>(f.b1 + 4 * cg);
                pc_f32x4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = fmaxf(v[r] + b[r], 0.f);
                *reinterpret_cast<pc_f32x4*>(c1 + (((size_t)d * N1i + i) * N1j + j) * K + 4 * cg) = o;
            }
        }
        __syncthreads();
        {   // ---- 3: A2 = conv2(A1) + bias + A0[d+2][i+2][j+2] ----
            const PcFront fr = pc_front(T - 21, C + 1, N2i, N2j);
            for (int n = tid; n < fr.nd * fr.iw * G; n += 256) {
                const int e = n / G, cg = n - e * G;
                int d, i, j;
                if (!pc_front_voxel(fr, e, d, i, j)) continue;
                float v[4];
                pc_wave_chain<4>(c1 + (((size_t)d * N1i + i) * N1j + j) * K, N1i, N1j, f.w2 + 4 * cg, K, v);
                const pc_f32x4 b = *reinterpret_cast<const pc_f32x4*>(f.b2 + 4 * cg);
                const pc_f32x4 sk = *reinterpret_cast<const pc_f32x4*>(c0 + (((size_t)(d + 2) * N0i + i + 2) * N0j + j + 2) * K + 4 * cg);
                pc_f32x4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) { float a2 = v[r] + b[r]; a2 += sk[r]; o[r] = a2; }
                *reinterpret_cast<pc_f32x4*>(c2 + (((size_t)d * N2i + i) * N2j + j) * K + 4 * cg) = o;
            }
        }
        __syncthreads();
        // ---- 4: the symbols (c, y, x) with x + 2 y + 4 c == T - 28: logits, then the range decoder in (c, y, x) order ----
        const PcFront fr = pc_front(T - 28, C, h, w);
        const int ncand = fr.nd * fr.iw;
        if constexpr (SEG) {
            if (wave == 0 && T > T_cut) {                 // the cut: this front's symbols are the first of segment seg_next
                seg_next = __builtin_amdgcn_readfirstlane(seg_next);
                const long long seg_off = ((seg_cptr)segs)[seg_next].off, seg_bytes = ((seg_cptr)segs)[seg_next].nbytes;
                sticky |= s.error;
                bits = seg_base + seg_off; nbytes = seg_bytes;
                pc_dec_state_init(s, bits, nbytes);
                for (int i = 0; i < PC_AC_BITS; ++i) s.code = (s.code << 1) | (unsigned)pc_dec_bit(bits, nbytes, s);
                ++seg_next;
                T_cut = seg_next < nlayers ? T_base + 4 * ((int_cptr)ends)[seg_next - 1] : 0x7fffffff;
            }
        }
        for (int cb = 0; cb < ncand; cb += CH) {
            const int nc = min(CH, ncand - cb);
            for (int n = tid; n < nc * L; n += 256) {
                const int slot = n / L, co = n - slot * L;
                int c, y, x;
                if (!pc_front_voxel(fr, cb + slot, c, y, x)) continue;
                if constexpr (DEPTH) {
                    // (a load of the plane, behind the check of the stream's length that the caller has made: off the serial path)
                    const bool live = c < min((int)depth[(y / dblock) * dnbx + x / dblock], C);
                    if (co == 0) {
                        s_live[slot] = live ? 1 : 0;
                        if (!live) {
                            if (SYMS && c < cdec) out[(long long)c * out_cs + (long long)y * out_rs + x] = fill;
                            vol[((size_t)(c + 4) * PH + y + 4) * PW + x + 4] = s_centers[fill];
                        }
                    }
                    if (!live) continue;
                }
                float v[1];
                pc_wave_chain<1>(c2 + (((size_t)c * N2i + y) * N2j + x) * K, N2i, N2j, f.w3 + co, L, v);
                s_logits[slot][co] = fmaxf(v[0] + f.b3[co], 0.f);
            }
            __syncthreads();
            if constexpr (RDO) {
                if (wave == 0) {                          // lane k decides slot k
                    int c, y, x;
                    if (lane < nc && pc_front_voxel(fr, cb + lane, c, y, x)) {
                        const float z = rz[(c * h + y) * w + x];
                        const bool rated = (c | y | x) != 0;                      // the first position is stored raw: no rate
                        bool ok = true;
                        int sym = 0;
                        switch (L) {
#define PC_RDO_CASE(l) case l: sym = pc_rdo_pick<l>(s_logits[lane], rated, a.resolution, z, s_centers, rlam, ok); break;
                            PC_RDO_CASE(1) PC_RDO_CASE(2) PC_RDO_CASE(3) PC_RDO_CASE(4) PC_RDO_CASE(5) PC_RDO_CASE(6)
                            PC_RDO_CASE(7) PC_RDO_CASE(8) PC_RDO_CASE(9) PC_RDO_CASE(10) PC_RDO_CASE(11) PC_RDO_CASE(12)
                            PC_RDO_CASE(13) PC_RDO_CASE(14) PC_RDO_CASE(15) PC_RDO_CASE(16)
#undef PC_RDO_CASE
                        }
                        if (!ok) rerr |= 1;
                        if (SYMS) out[(long long)c * out_cs + (long long)y * out_rs + x] = sym;
                        vol[((size_t)(c + 4) * PH + y + 4) * PW + x + 4] = s_centers[sym];
                    }
                }
            } else
            if constexpr (RANS) {
                if (wave == 0) {
                    {   // the tables of the chunk's slots, one per lane
                        int c, y, x;
                        if (lane < nc && pc_front_voxel(fr, cb + lane, c, y, x) && (c | y | x) != 0) {
                            bool ok = true;
                            switch (L) {
#define PC_RANS_CASE(l) case l: ok = pc_dec_rans_build<l>(s_logits, lane, a.resolution); break;
                                PC_RANS_CASE(1) PC_RANS_CASE(2) PC_RANS_CASE(3) PC_RANS_CASE(4) PC_RANS_CASE(5) PC_RANS_CASE(6)
                                PC_RANS_CASE(7) PC_RANS_CASE(8) PC_RANS_CASE(9) PC_RANS_CASE(10) PC_RANS_CASE(11) PC_RANS_CASE(12)
                                PC_RANS_CASE(13) PC_RANS_CASE(14) PC_RANS_CASE(15) PC_RANS_CASE(16)
#undef PC_RANS_CASE
                            }
                            if (!ok) rerr |= 1;
                        }
                    }
                    // the rows are read by other lanes of this wave: its LDS stores are done and visible before the first read
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                    for (int sb = 0; sb < nc; sb += rlanes) {                     // CH / W sub-rounds at the most; uniform
                        const int k = sb + lane;
                        int c = 0, y = 0, x = 0;
                        const bool valid = lane < rlanes && k < nc && pc_front_voxel(fr, cb + k, c, y, x);
                        int sym = first_sym;                                      // the first symbol is not coded
                        bool need = false;
                        if (valid && (c | y | x) != 0) {
                            const unsigned* row = reinterpret_cast<const unsigned*>(s_logits[k]);
                            unsigned cum[16];
#pragma unroll
                            for (int j = 0; j < 16; ++j) cum[j] = row[j];
                            const unsigned sv = rx & 0xffffu;
                            unsigned cg = 0, nx = PC_RANS_M;
                            sym = 0;
#pragma unroll
                            for (int j = 1; j < 16; ++j) {                        // entries from L on are M: never <= sv
                                if (cum[j] <= sv) { sym = j; cg = cum[j]; }
                                else nx = min(nx, cum[j]);
                            }
                            rx = (nx - cg) * (rx >> 16) + (sv - cg);              // < 2^32: (nx - cg) ((x >> 16) + 1) <= 2^16 2^16
                            need = rx < PC_RANS_M;
                        }
                        const unsigned long long needing = __ballot(need);
                        if (need) {
                            const long long o = 4ll * rlanes + 2 * (rtaken + __popcll(needing & ((1ull << lane) - 1)));
                            const unsigned lo = o < nbytes ? bits[o] : 0u, hi = o + 1 < nbytes ? bits[o + 1] : 0u;
                            rx = (rx << 16) | lo | (hi << 8);
                        }
                        rtaken += __popcll(needing);
                        if (valid) {
                            if (SYMS && c < cdec) out[(long long)c * out_cs + (long long)y * out_rs + x] = sym;
                            vol[((size_t)(c + 4) * PH + y + 4) * PW + x + 4] = s_centers[sym];
                        }
                    }
                }
            } else
            if (wave == 0) {
                unsigned long long livemask = ~0ull;                              // DEPTH: the chunk's live bytes as one scalar word
                if constexpr (DEPTH) livemask = __ballot(lane < nc && s_live[lane] != 0);
                for (int k = 0; k < nc; ++k) {
                    int c, y, x;
                    if (!pc_front_voxel(fr, cb + k, c, y, x)) continue;          // wave-uniform
                    if constexpr (DEPTH) if (!((livemask >> k) & 1)) continue;   // dead: stored by the slot's lane above
                    int sym = first_sym;                                          // the first symbol is not coded
                    if ((c | y | x) != 0) {
                        const float logit = (lane >= 48 && lane < 48 + L) ? s_logits[k][lane - 48] : 0.f;
                        sym = L == 6 ? pc_dec_symbol_wave<6>(bits, nbytes, L, a.resolution, s, logit)
                                     : pc_dec_symbol_wave<0>(bits, nbytes, L, a.resolution, s, logit);
                    }
                    if (lane == 0) {
                        if constexpr (FROM) plane[(c * h + y) * w + x] = (unsigned char)sym;
                        else if (SYMS && (!LIM || c < cdec)) out[(long long)c * out_cs + (long long)y * out_rs + x] = sym;
                        vol[((size_t)(c + 4) * PH + y + 4) * PW + x + 4] = s_centers[sym];
                    }
                }
            }
            __syncthreads();                              // V of this front before the next step's conv0; s_logits free again
        }
    }
    if constexpr (RDO) {
        if (wave == 0) {
            const int st = __ballot(rerr != 0) ? 1 : 0;
            if (lane == 0) *status = st;
        }
    } else
    if constexpr (RANS) {
        if (wave == 0) {                                  // the end check of a full decode; status 1 and 4 OR-ed over the lanes
            const bool bad4 = cdec == a.C && ((lane < rlanes && rx != PC_RANS_M) || 4ll * rlanes + 2 * rtaken != nbytes);
            const int st = (__ballot(rerr != 0) ? 1 : 0) | (__ballot(bad4) ? 4 : 0);
            if (lane == 0) *status = st;
        }
    } else
    if (tid == 0) *status = SEG ? (sticky | s.error) : s.error;
}

// ---- tiles: one work-group per tile, the tiles of all volumes in one launch ---------------------------------------------------
// A tile is a (C, th, tw) block of a symbol volume that was coded as a volume of its own (own padding, own stream, first
// symbol uncoded).  Work-group t decodes tiles[t] with pc_dec_cached_body -- pc_dec_wave_body for streams in wavefront order --
// in slot t of the workspace (padded volume + three caches, laid out for the largest tile; a smaller tile uses a prefix of each
// part with its own strides) and stores its symbols straight into its volume.  A work-group reads only what it wrote itself or
// what an earlier launch wrote (weights, centres, streams, the tables, the filled volumes): nothing passes between work-groups,
// nothing depends on co-residency.
// The volume of a tile -- own (h, w), own place in `symbols` and `q` -- comes from a second table (ic_pc_decode_tiles_batch_f32).
// Without that table there is one volume, `one`, which travels in the kernel arguments and holds every tile whatever its
// `volume` field says (ic_pc_decode_tiles_f32: its workspace has no room for a device copy of a volume table).
// q = centers[symbols] is what the decoder's padded volume holds at the end of the sweep (every decoded symbol's centre was
// stored there for the context gathers), so after the body the work-group copies its tile's interior out: all 256 threads,
// consecutive x on consecutive lanes, once per tile -- nothing is added to the per-symbol path of the bodies.
// LIM (ic_pc_decode_tiles_batch_channels_f32, cdec < C): the bodies stop after channel cdec - 1 and the same copy loop writes the
// rest -- q = centers[fill] and, with SYMS, symbols = fill for c >= cdec.  V is not read there: in the wavefront order it holds
// the centres of the symbols of later channels that the coder had to step through.
struct PcTilesBatchArgs {
    PcCachedArgs f;                   // weights, centres, C, L, resolution only: the rest comes from tiles[blockIdx.x]
    const unsigned char* bits;        // all streams
    const ic_pc_tile_t* tiles;        // device copies of the two tables
    const ic_pc_volume_t* volumes;    // null: every tile belongs to `one`
    ic_pc_volume_t one;
    char* slots; size_t slot_bytes, off_c0, off_c1, off_c2;
    long long* symbols; float* q; int* status;
    int cdec, fill;                   // LIM kernels only
    const ic_pc_seg_t* segs;          // SEG kernels only: device copy of the segment table (ntiles x nlayers, tile-major),
    const int* ends;                  //   of the layer ends (nlayers),
    int nlayers;                      //   and their number
    const int* tile_channels;         // PER kernels only: device copy of the channel limit per tile (ntiles)
    const int* tile_from;             // FROM kernels only: device copy of the layer every tile continues with (ntiles),
    int* done;                        //   and the channels the workspace holds of every tile (ntiles; written by the kernel alone)
    unsigned char* planes;            // WAVE FROM kernels only: a byte per symbol of every tile, plane_bytes per tile, (c, y, x) order
    size_t plane_bytes;               //   of the tile's own extent (written and read by the kernel alone)
    int depth_block;                  // DEPTH kernels only: the side b of a block of the depth plane, 1 .. 255
    int rans_lanes;                   // RANS kernels only: the number W of interleaved coders, 8 / 16 / 32 / 64
};

// SEG: the tile's stream is its nlayers segments, segs[blockIdx.x * nlayers + g]; the descriptor's stream_off / stream_bytes are not
// read.  Raster (ic_pc_decode_tiles_batch_layers_f32): cut at channel planes.  WAVE (ic_pc_decode_tiles_batch_fronts_f32): cut at fronts
// -- the two bodies each know one kind of cut; a channel plane is no prefix of a wavefront-ordered stream, so there is no WAVE decoder
// of plane cuts and none is selected by any flag.
// PER (ic_pc_decode_tiles_batch_layers_pertile_f32): the channel limit is the tile's own, tile_channels[blockIdx.x] in 1 .. C, in
// place of the launch's cdec.  A uniform index into a table that no kernel writes, read like the segment table through the constant
// address space: one scalar load per tile, a uniform value as cdec is, and nothing of it in the body's per-symbol path.  A tile whose
// limit is C is decoded whole; the copy loop then has no channel to fill.
// FROM (ic_pc_decode_tiles_batch_layers_resume_f32): the tile continues with layer gfrom = tile_from[blockIdx.x], read like the limit.
// gfrom == 0 is PER.  gfrom > 0: the slot holds the tile swept up to channel cfrom = ends[gfrom - 1] by an earlier launch on the same
// stream, and done[blockIdx.x] says so -- a word per tile that only this kernel writes: cdec behind a sweep that ended with status
// 0, -1 behind one that did not.  A work-group whose done word is not cfrom stores status 2 and returns: no symbol, no q, nothing
// of its slot or of done is touched.  Otherwise the body sweeps the channels [cfrom, cdec) (none if cfrom == cdec: a uniform branch
// around it) and the copy loop writes those and the fill above cdec; the channels below cfrom are the earlier call's and stay.
// Still nothing passes between work-groups: a work-group reads its own slot and its own done word.
// WAVE && FROM (ic_pc_decode_tiles_batch_fronts_resume_f32): the same for front-cut streams, pc_dec_wave_body<.., FROM>.  A slot swept
// in one order is of no use to the other -- the raster sweep fills the caches plane by plane, the front sweep front by front -- and the
// two entries may be given the same workspace, so the done word tells them apart: the raster kernels write cdec >= 1, these write
// -2 - cdec <= -3, both write -1 behind an error, and each takes only its own kind for a match.  The body stores no symbol through
// `symbols`; it keeps every symbol it steps through in the tile's byte plane (see the body), and the copy loop writes the symbols of
// [cfrom, cdec) from the plane next to q from V.  The plane of a tile holds every symbol of the channels below cdec after a sweep to
// cdec, whichever launches decoded them: each lies on a front <= T_last(cdec), and every front is swept once.
// DEPTH (ic_pc_decode_tiles_batch_channels_f32 with IC_PC_DECODE_DEPTH(b); WAVE && LIM only, channels == C included): the first
// nby * nbx bytes of the tile's stream, nby = ceil(th / b), nbx = ceil(tw / b), are its depth plane and the coder starts behind them.
// A stream shorter than that: status 2, nothing decoded, nothing written.  All 256 lanes reduce the plane's largest entry (clamped to
// C) to dmax; the sweep is the LIM sweep to cdec = min(channels, dmax) over dmax channels, and the copy loop's fill covers the
// channels from cdec up -- dead everywhere, or beyond the preview.  dmax == 0: no body at all, status 0, everything is fill.
// RANS (ic_pc_decode_tiles_batch_channels_f32 with IC_PC_DECODE_RANS(W); WAVE && LIM only, channels == C included): the tile's stream
// is that of W interleaved rANS coders; the sweep is the LIM sweep to cdec, its serial part replaced (pc_dec_wave_body, RANS).
template <bool WAVE, bool SYMS, bool LIM = false, bool SEG = false, bool PER = false, bool FROM = false, bool DEPTH = false, bool RANS = false>
__global__ __launch_bounds__(256) void pc_dec_tiles_batch_kernel(const PcTilesBatchArgs t) {
    static_assert(!RANS || (WAVE && LIM && !SEG && !DEPTH), "the interleaved coders belong to the unsegmented wavefront sweep with a limit");
    static_assert(!PER || (LIM && SEG), "the limit per tile belongs to the segmented decoders: a limited sweep over a tile's segments");
    static_assert(!FROM || PER, "a sweep continues where a sweep with a limit per tile stopped");
    static_assert(!DEPTH || (WAVE && LIM && !SEG), "the depth plane belongs to the unsegmented wavefront sweep with a limit");
    constexpr int DONE_SIGN = (WAVE && FROM) ? -1 : 1, DONE_BASE = (WAVE && FROM) ? -2 : 0;     // done word of a status-0 sweep to c: DONE_BASE + DONE_SIGN * c
    const ic_pc_tile_t tl = t.tiles[blockIdx.x];
    // v = volumes ? volumes[tl.volume] : one, as a uniform branch around a scalar load.  (Written as a select, it becomes a select
    // between the two ADDRESSES, kernel arguments or global memory, and a load through a flat pointer into vector registers:
    // 8 more VGPRs per lane, held across the body.)
    ic_pc_volume_t v = t.one;
    if (t.volumes) { v = t.volumes[tl.volume]; asm volatile("" ::: "memory"); }
    char* slot = t.slots + (size_t)blockIdx.x * t.slot_bytes;
    const long long corner = (long long)tl.y0 * v.w + tl.x0, plane = (long long)v.h * v.w;
    int cdec = LIM ? t.cdec : 0;
    if constexpr (PER) cdec = ((const __attribute__((address_space(4))) int*)t.tile_channels)[blockIdx.x];
    int cfrom = 0;                    // FROM: the channels below it are the earlier call's
    if constexpr (FROM) {
        typedef const __attribute__((address_space(4))) int* int_cptr;
        typedef const __attribute__((address_space(4))) ic_pc_seg_t* seg_cptr;
        const int gfrom = ((int_cptr)t.tile_from)[blockIdx.x];
        const ic_pc_seg_t* segs = t.segs + (size_t)blockIdx.x * t.nlayers;
        long long off0 = 0, nbytes0 = 0;                   // segment 0 of a tile that continues is not looked at
        if (gfrom > 0) {
            cfrom = ((int_cptr)t.ends)[gfrom - 1];
            if (t.done[blockIdx.x] != DONE_BASE + DONE_SIGN * cfrom) {      // the slot does not hold this tile up to cfrom (uniform)
                if (threadIdx.x == 0) t.status[blockIdx.x] = 2;
                return;
            }
        } else {
            off0 = ((seg_cptr)segs)[0].off; nbytes0 = ((seg_cptr)segs)[0].nbytes;
        }
        if constexpr (WAVE) {
            if (cfrom < cdec)
                pc_dec_wave_body<SYMS, true, true, true>(t.f, t.bits + off0, nbytes0, tl.th, tl.tw, tl.first_sym, (float*)slot,
                                                         (float*)(slot + t.off_c0), (float*)(slot + t.off_c1), (float*)(slot + t.off_c2), t.status + blockIdx.x,
                                                         nullptr, 0, 0, cdec, t.bits, segs, t.ends, t.nlayers, gfrom,
                                                         t.planes + (size_t)blockIdx.x * t.plane_bytes);
            else if (threadIdx.x == 0) t.status[blockIdx.x] = 0;
        } else if (cfrom < cdec)
            pc_dec_cached_body<SYMS, true, true, true>(t.f, t.bits + off0, nbytes0, tl.th, tl.tw, tl.first_sym, (float*)slot,
                                                       (float*)(slot + t.off_c0), (float*)(slot + t.off_c1), (float*)(slot + t.off_c2), t.status + blockIdx.x,
                                                       SYMS ? t.symbols + v.symbols_off + corner : nullptr, plane, v.w, cdec,
                                                       t.bits, segs, t.ends, t.nlayers, gfrom);
        else if (threadIdx.x == 0) t.status[blockIdx.x] = 0;
        if (threadIdx.x == 0) t.done[blockIdx.x] = t.status[blockIdx.x] == 0 ? DONE_BASE + DONE_SIGN * cdec : -1;       // (thread 0 stored the status)
    } else if constexpr (WAVE && SEG) {
        const ic_pc_seg_t* segs = t.segs + (size_t)blockIdx.x * t.nlayers;
        typedef const __attribute__((address_space(4))) ic_pc_seg_t* seg_cptr;      // (a table no kernel writes: see the body)
        const long long off0 = ((seg_cptr)segs)[0].off, nbytes0 = ((seg_cptr)segs)[0].nbytes;
        pc_dec_wave_body<SYMS, LIM, true>(t.f, t.bits + off0, nbytes0, tl.th, tl.tw, tl.first_sym, (float*)slot,
                                          (float*)(slot + t.off_c0), (float*)(slot + t.off_c1), (float*)(slot + t.off_c2), t.status + blockIdx.x,
                                          SYMS ? t.symbols + v.symbols_off + corner : nullptr, plane, v.w, cdec,
                                          t.bits, segs, t.ends, t.nlayers);
    } else if constexpr (DEPTH) {
        __shared__ int s_dmax;
        const int b = t.depth_block, nbx = (tl.tw + b - 1) / b, nd = ((tl.th + b - 1) / b) * nbx;        // nd <= th * tw
        if (tl.stream_bytes < nd) {                       // (uniform) no room for the plane: not a stream of this format
            if (threadIdx.x == 0) t.status[blockIdx.x] = 2;
            return;
        }
        const unsigned char* depth = t.bits + tl.stream_off;
        if (threadIdx.x == 0) s_dmax = 0;
        __syncthreads();
        int m = 0;
        for (int i = threadIdx.x; i < nd; i += 256) m = max(m, min((int)depth[i], t.f.d.C));
        if (m) atomicMax(&s_dmax, m);                     // LDS; once per tile
        __syncthreads();
        const int dmax = s_dmax;
        cdec = min(cdec, dmax);
        if (dmax > 0)
            pc_dec_wave_body<SYMS, true, false, false, true>(t.f, depth + nd, tl.stream_bytes - nd, tl.th, tl.tw, tl.first_sym, (float*)slot,
                                                             (float*)(slot + t.off_c0), (float*)(slot + t.off_c1), (float*)(slot + t.off_c2), t.status + blockIdx.x,
                                                             SYMS ? t.symbols + v.symbols_off + corner : nullptr, plane, v.w, cdec,
                                                             nullptr, nullptr, nullptr, 0, 0, nullptr, depth, b, nbx, dmax, t.fill);
        else if (threadIdx.x == 0) t.status[blockIdx.x] = 0;
    } else if constexpr (RANS) {
        pc_dec_wave_body<SYMS, true, false, false, false, true>(t.f, t.bits + tl.stream_off, tl.stream_bytes, tl.th, tl.tw, tl.first_sym, (float*)slot,
                                                                (float*)(slot + t.off_c0), (float*)(slot + t.off_c1), (float*)(slot + t.off_c2), t.status + blockIdx.x,
                                                                SYMS ? t.symbols + v.symbols_off + corner : nullptr, plane, v.w, cdec,
                                                                nullptr, nullptr, nullptr, 0, 0, nullptr, nullptr, 1, 0, 0, 0, t.rans_lanes);
    } else if constexpr (WAVE)
        pc_dec_wave_body<SYMS, LIM>(t.f, t.bits + tl.stream_off, tl.stream_bytes, tl.th, tl.tw, tl.first_sym, (float*)slot,
                                    (float*)(slot + t.off_c0), (float*)(slot + t.off_c1), (float*)(slot + t.off_c2), t.status + blockIdx.x,
                                    SYMS ? t.symbols + v.symbols_off + corner : nullptr, plane, v.w, cdec);
    else if constexpr (SEG) {
        const ic_pc_seg_t* segs = t.segs + (size_t)blockIdx.x * t.nlayers;
        typedef const __attribute__((address_space(4))) ic_pc_seg_t* seg_cptr;      // (a table no kernel writes: see the body)
        const long long off0 = ((seg_cptr)segs)[0].off, nbytes0 = ((seg_cptr)segs)[0].nbytes;
        pc_dec_cached_body<SYMS, LIM, true>(t.f, t.bits + off0, nbytes0, tl.th, tl.tw, tl.first_sym, (float*)slot,
                                            (float*)(slot + t.off_c0), (float*)(slot + t.off_c1), (float*)(slot + t.off_c2), t.status + blockIdx.x,
                                            SYMS ? t.symbols + v.symbols_off + corner : nullptr, plane, v.w, cdec,
                                            t.bits, segs, t.ends, t.nlayers);
    } else
        pc_dec_cached_body<SYMS, LIM>(t.f, t.bits + tl.stream_off, tl.stream_bytes, tl.th, tl.tw, tl.first_sym, (float*)slot,
                                      (float*)(slot + t.off_c0), (float*)(slot + t.off_c1), (float*)(slot + t.off_c2), t.status + blockIdx.x,
                                      SYMS ? t.symbols + v.symbols_off + corner : nullptr, plane, v.w, cdec);
    if (!(LIM && SYMS) && t.q == nullptr) return;
    __syncthreads();                  // the volume's last stores (lane 0 of wave 0) are visible to the whole work-group
    const float* vol = (const float*)slot;
    float* q;
    if constexpr (LIM) q = t.q ? t.q + v.q_off + corner : nullptr;
    else q = t.q + v.q_off + corner;
    const int PH = tl.th + 8, PW = tl.tw + 8, n = t.f.d.C * tl.th * tl.tw;
    if constexpr (!LIM) {
        for (int i = threadIdx.x; i < n; i += 256) {
            const int x = i % tl.tw, y = (i / tl.tw) % tl.th, c = i / (tl.tw * tl.th);
            q[(long long)c * plane + (long long)y * v.w + x] = vol[((size_t)(c + 4) * PH + y + 4) * PW + x + 4];
        }
    } else {
        const float qfill = t.f.d.centers[t.fill];
        long long* syms = SYMS ? t.symbols + v.symbols_off + corner : nullptr;
        for (int i = threadIdx.x + (FROM ? cfrom * tl.th * tl.tw : 0); i < n; i += 256) {       // FROM: channels >= cfrom only
            const int x = i % tl.tw, y = (i / tl.tw) % tl.th, c = i / (tl.tw * tl.th);
            const long long o = (long long)c * plane + (long long)y * v.w + x;
            if (c < cdec) {
                if (q) q[o] = vol[((size_t)(c + 4) * PH + y + 4) * PW + x + 4];
                if constexpr (WAVE && FROM && SYMS) syms[o] = t.planes[(size_t)blockIdx.x * t.plane_bytes + i];
            } else {
                if (q) q[o] = qfill;
                if (SYMS) syms[o] = t.fill;
            }
        }
    }
}

// The rate-aware symbol chooser over tiles (ic_pc_decode_tiles_batch_channels_f32 with IC_PC_DECODE_RDO; pc_dec_wave_body, RDO): the
// launch shape, the tables and the slot of the wavefront decoder -- one work-group per tile, nothing passing between work-groups --,
// the tile's "stream" being its record.  A kernel of its own beside pc_dec_tiles_batch_kernel, whose forms stay what they were.
template <bool SYMS>
__global__ __launch_bounds__(256) void pc_rdo_tiles_batch_kernel(const PcTilesBatchArgs t) {
    const ic_pc_tile_t tl = t.tiles[blockIdx.x];
    const ic_pc_volume_t v = t.volumes[tl.volume];        // (the batch entry: there is always a volume table)
    char* slot = t.slots + (size_t)blockIdx.x * t.slot_bytes;
    const long long corner = (long long)tl.y0 * v.w + tl.x0, plane = (long long)v.h * v.w;
    const int C = t.f.d.C;
    pc_dec_wave_body<SYMS, true, false, false, false, false, true>(t.f, t.bits + tl.stream_off, tl.stream_bytes, tl.th, tl.tw, 0, (float*)slot,
                                                                   (float*)(slot + t.off_c0), (float*)(slot + t.off_c1), (float*)(slot + t.off_c2), t.status + blockIdx.x,
                                                                   SYMS ? t.symbols + v.symbols_off + corner : nullptr, plane, v.w, C);
    if (t.q == nullptr) return;
    __syncthreads();                  // the volume's last stores (wave 0) are visible to the whole work-group
    const float* vol = (const float*)slot;
    float* q = t.q + v.q_off + corner;
    const int PH = tl.th + 8, PW = tl.tw + 8, n = C * tl.th * tl.tw;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int x = i % tl.tw, y = (i / tl.tw) % tl.th, c = i / (tl.tw * tl.th);
        q[(long long)c * plane + (long long)y * v.w + x] = vol[((size_t)(c + 4) * PH + y + 4) * PW + x + 4];
    }
}

// symbol 0 in every tile's padded volume: grid (ceil(n / 256), ntiles)
__global__ __launch_bounds__(256) void pc_dec_fill_slots_kernel(char* __restrict__ slots, size_t slot_bytes, long long n,
                                                                const float* __restrict__ centers) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) ((float*)(slots + (size_t)blockIdx.y * slot_bytes))[i] = centers[0];
}

// the same for the tiles that start afresh (from[tile] == 0); the slot of a tile that continues keeps what the earlier launch left
__global__ __launch_bounds__(256) void pc_dec_fill_fresh_slots_kernel(char* __restrict__ slots, size_t slot_bytes, long long n,
                                                                      const float* __restrict__ centers, const int* __restrict__ from) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (from[blockIdx.y] == 0 && i < n) ((float*)(slots + (size_t)blockIdx.y * slot_bytes))[i] = centers[0];
}

// slow path of the tile entries: a tile decoded into a buffer of its own -> its place in its volume, as symbols
// and / or centres
__global__ __launch_bounds__(256) void pc_tile_place_batch_kernel(const long long* __restrict__ src, long long* __restrict__ dst,
                                                                  float* __restrict__ q, const float* __restrict__ centers,
                                                                  int C, int th, int tw, int h, int w, int y0, int x0) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)C * th * tw) return;
    const int x = (int)(i % tw), y = (int)((i / tw) % th), c = (int)(i / ((long long)tw * th));
    const long long o = ((long long)c * h + y0 + y) * w + x0 + x, sym = src[i];
    if (dst) dst[o] = sym;
    if (q) q[o] = centers[sym];
}

static size_t pc_dec_align(size_t b) { return (b + 255) & ~(size_t)255; }

// activation caches of pc_dec_cached_kernel (k = 24): the three feature volumes of the padded symbol volume, channels-last
static size_t pc_dec_cache_floats(int C, int h, int w, int k, int layer) {
    return (size_t)k * (C + 3 - layer) * (h + 6 - 2 * layer) * (w + 6 - 2 * layer);
}
static size_t pc_dec_cache_bytes(int C, int h, int w, int k) {
    if (k != 24) return 0;
    size_t b = 0;
    for (int l = 0; l < 3; ++l) b += pc_dec_align(pc_dec_cache_floats(C, h, w, k, l) * sizeof(float));
    return b;
}

extern "C" size_t ic_pc_decode_workspace_bytes(int C, int h, int w, int k) {
    if (C <= 0 || h <= 0 || w <= 0 || k <= 0) return 0;
    return pc_dec_align((size_t)(C + 4) * (h + 8) * (w + 8) * sizeof(float)) + pc_dec_align(405 * sizeof(float)) +
           pc_dec_align(16 * sizeof(float)) + pc_dec_align(sizeof(PcDecState)) + ic_pc_workspace_bytes(1, 1, 1, 1, k) +
           pc_dec_cache_bytes(C, h, w, k);
}

// One volume, behind the entries' checks.  channels == C: the full decode, whatever fill_sym.  channels < C (k = 24, flags 0,
// which ic_pc_decode_channels_f32 has checked): the first channels only, the others filled with fill_sym.
static int pc_decode_impl(const uint8_t* bitstream, long long nbytes, int first_sym, const float* const* wtab_host,
                          const float* centers, int k, int L, float resolution, int64_t* symbols, int* status,
                          int C, int h, int w, void* workspace, int flags, int channels, int fill_sym, ic_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    char* p = (char*)workspace;
    PcDecArgs a{};
    a.bits = bitstream; a.nbytes = nbytes; a.centers = centers; a.symbols = (long long*)symbols;
    a.C = C; a.h = h; a.w = w; a.L = L; a.first_sym = first_sym; a.resolution = resolution;
    const long long nvol = (long long)(C + 4) * (h + 8) * (w + 8);
    a.vol = (float*)p; p += pc_dec_align((size_t)nvol * sizeof(float));
    a.ctx = (float*)p; p += pc_dec_align(405 * sizeof(float));
    float* logits = (float*)p; p += pc_dec_align(16 * sizeof(float));
    a.logits = logits;
    a.st = (PcDecState*)p; p += pc_dec_align(sizeof(PcDecState));
    void* pcws = p;
    const size_t pcws_bytes = ic_pc_workspace_bytes(1, 1, 1, 1, k);
    p += pcws_bytes;
    hipLaunchKernelGGL(pc_dec_fill_kernel, dim3((unsigned)((nvol + 255) / 256)), dim3(256), 0, st, a.vol, nvol, centers);
    if (k == 24 && !(flags & (IC_PC_DECODE_PER_LAYER | IC_PC_DECODE_RECOMPUTE))) {
        PcCachedArgs f{};
        f.d = a;
        f.w0 = wtab_host[0]; f.b0 = wtab_host[1]; f.w1 = wtab_host[2]; f.b1 = wtab_host[3];
        f.w2 = wtab_host[4]; f.b2 = wtab_host[5]; f.w3 = wtab_host[6]; f.b3 = wtab_host[7];
        f.c0 = (float*)p; p += pc_dec_align(pc_dec_cache_floats(C, h, w, k, 0) * sizeof(float));
        f.c1 = (float*)p; p += pc_dec_align(pc_dec_cache_floats(C, h, w, k, 1) * sizeof(float));
        f.c2 = (float*)p;
        f.status = status;
        if (channels < C) hipLaunchKernelGGL(pc_dec_cached_channels_kernel, dim3(1), dim3(256), 0, st, f, channels, fill_sym);
        else hipLaunchKernelGGL(pc_dec_cached_kernel, dim3(1), dim3(256), 0, st, f);
        IC_LAUNCH_CHECK();
        return IC_OK;
    }
    // filters packed once (pc_forward's own layout: after the three feature volumes of the 5x9x9 context)
    const bool use_mfma = pc_mfma_supported(k, L);
    if (use_mfma) {
        float* pk1 = (float*)pcws + (size_t)k * (4 * 7 * 7 + 3 * 5 * 5 + 2 * 3 * 3);
        const int rc = pc_pack_filters(wtab_host, k, L, pk1, st);
        if (rc) return rc;
    }
    if (use_mfma && k == 24 && !(flags & IC_PC_DECODE_PER_LAYER)) {
        PcFusedArgs f{};
        f.d = a;
        float* pk1 = (float*)pcws + (size_t)k * (4 * 7 * 7 + 3 * 5 * 5 + 2 * 3 * 3);
        f.w0 = wtab_host[0]; f.b0 = wtab_host[1];
        f.pk1 = pk1; f.b1 = wtab_host[3];
        f.pk2 = pk1 + pc_packed_floats(k, k); f.b2 = wtab_host[5];
        f.pk3 = pk1 + 2 * pc_packed_floats(k, k); f.b3 = wtab_host[7];
        f.status = status;
        hipLaunchKernelGGL(pc_dec_fused_kernel, dim3(1), dim3(256), 0, st, f);
        IC_LAUNCH_CHECK();
        return IC_OK;
    }
    hipLaunchKernelGGL(pc_dec_init_kernel, dim3(1), dim3(256), 0, st, a);
    IC_LAUNCH_CHECK();
    const long long n = (long long)C * h * w;
    auto one_symbol = [&]() -> int {
        int rc = pc_forward(a.ctx, 1, nullptr, wtab_host, k, L, 0.f, logits, nullptr, 1, 1, 1, 1, pcws, pcws_bytes, st, true);
        if (rc) return rc;
        hipLaunchKernelGGL(pc_dec_step_kernel, dim3(1), dim3(256), 0, st, a);
        return IC_OK;
    };
    // Every symbol runs the same five kernels with the SAME arguments (context, logits and coder state live at fixed
    // addresses), so a block of PC_DEC_GRAPH symbols is captured once into a hipGraph and replayed: the host cost of
    // ~1 M kernel launches per Kodak image (58 us per symbol, launch-bound) drops to one graph launch per block.
    long long i = 1;
    constexpr int PC_DEC_GRAPH = 128;
    if (n - 1 >= 2 * PC_DEC_GRAPH) {
        // capture is not allowed on the legacy default stream (torch's current stream by default): the loop runs on a
        // private stream ordered after / before the caller's by events
        // (created per call and destroyed before returning: the library keeps no per-process or per-device objects)
        hipStream_t own = nullptr;
        hipEvent_t ev_in = nullptr, ev_out = nullptr;
        bool ok = hipStreamCreateWithFlags(&own, hipStreamNonBlocking) == hipSuccess &&
                  hipEventCreateWithFlags(&ev_in, hipEventDisableTiming) == hipSuccess &&
                  hipEventCreateWithFlags(&ev_out, hipEventDisableTiming) == hipSuccess;
        auto release = [&]() {
            if (ev_in) (void)hipEventDestroy(ev_in);
            if (ev_out) (void)hipEventDestroy(ev_out);
            if (own) (void)hipStreamDestroy(own);
        };
        if (!ok) { release(); own = nullptr; (void)hipGetLastError(); }
        if (ok) {
            const hipStream_t caller = st;
            ok = hipEventRecord(ev_in, caller) == hipSuccess && hipStreamWaitEvent(own, ev_in, 0) == hipSuccess;
            if (ok) {
                st = own;
                int rc = IC_OK;
                hipGraph_t graph = nullptr;
                hipGraphExec_t exec = nullptr;
                if (hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed) == hipSuccess) {
                    for (int j = 0; j < PC_DEC_GRAPH && rc == IC_OK; ++j) rc = one_symbol();
                    const hipError_t e = hipStreamEndCapture(st, &graph);
                    if (rc == IC_OK && e == hipSuccess && graph &&
                        hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess) {
                        bool launched = true;
                        for (; launched && i + PC_DEC_GRAPH <= n; i += PC_DEC_GRAPH) launched = hipGraphLaunch(exec, st) == hipSuccess;
                        // the executable graph must outlive its last launch: wait before destroying it
                        (void)hipStreamSynchronize(st);
                        (void)hipGraphExecDestroy(exec);
                        if (!launched) rc = IC_ERR_ARG;
                    }
                    if (graph) (void)hipGraphDestroy(graph);
                }
                (void)hipGetLastError();
                for (; rc == IC_OK && i < n; ++i) rc = one_symbol();
                if (rc == IC_OK && hipMemcpyAsync(status, &a.st->error, sizeof(int), hipMemcpyDeviceToDevice, st) != hipSuccess) rc = IC_ERR_ARG;
                // the caller's stream continues after everything queued on the private one (also on the error paths)
                if (hipEventRecord(ev_out, own) != hipSuccess || hipStreamWaitEvent(caller, ev_out, 0) != hipSuccess) rc = rc ? rc : IC_ERR_ARG;
                if (rc == IC_OK) { const hipError_t e2 = hipGetLastError(); if (e2 != hipSuccess) rc = (int)e2; }
                release();           // destruction is deferred by the runtime until the queued work has drained
                return rc;
            }
            release();
        }
    }
    for (; i < n; ++i) {
        int rc = one_symbol();
        if (rc) return rc;
    }
    IC_LAUNCH_CHECK();
    if (hipMemcpyAsync(status, &a.st->error, sizeof(int), hipMemcpyDeviceToDevice, st) != hipSuccess) return IC_ERR_ARG;
    return IC_OK;
}

extern "C" int ic_pc_decode_f32(const uint8_t* bitstream, long long nbytes, int first_sym, const float* const* wtab_host,
                                const float* centers, int k, int L, float resolution, int64_t* symbols, int* status,
                                int C, int h, int w, void* workspace, size_t workspace_bytes, int flags, ic_stream_t stream) {
    IC_CHECK_ARG(bitstream && wtab_host && centers && symbols && status && workspace);
    IC_CHECK_ARG(nbytes >= 0 && C > 0 && h > 0 && w > 0 && k > 0 && L > 0 && first_sym >= 0 && first_sym < L);
    if (L > 16 || (flags & (IC_PC_DECODE_WAVEFRONT | IC_PC_DECODE_DEPTH(0xff) | IC_PC_DECODE_RANS(0xff) | IC_PC_DECODE_RDO))) return IC_ERR_UNSUPPORTED;      // (the wavefront order: the batch entry only; the depth plane, the rANS coders and the symbol chooser: its channels form only)
    if (workspace_bytes < ic_pc_decode_workspace_bytes(C, h, w, k)) return IC_ERR_WORKSPACE;
    return pc_decode_impl(bitstream, nbytes, first_sym, wtab_host, centers, k, L, resolution, symbols, status, C, h, w, workspace,
                          flags, C, 0, stream);
}

// preview: channels 0 .. channels - 1 decoded, the others fill_sym.  Only the k = 24 kernel has the limit: no slow path.
extern "C" int ic_pc_decode_channels_f32(const uint8_t* bitstream, long long nbytes, int first_sym, const float* const* wtab_host,
                                         const float* centers, int k, int L, float resolution, int64_t* symbols, int* status,
                                         int C, int h, int w, void* workspace, size_t workspace_bytes, int flags, ic_stream_t stream,
                                         int channels, int fill_sym) {
    IC_CHECK_ARG(bitstream && wtab_host && centers && symbols && status && workspace);
    IC_CHECK_ARG(nbytes >= 0 && C > 0 && h > 0 && w > 0 && k > 0 && L > 0 && first_sym >= 0 && first_sym < L);
    IC_CHECK_ARG(channels >= 1 && channels <= C && fill_sym >= 0 && fill_sym < L);
    if (L > 16 || k != 24 || flags != 0) return IC_ERR_UNSUPPORTED;
    if (workspace_bytes < ic_pc_decode_workspace_bytes(C, h, w, k)) return IC_ERR_WORKSPACE;
    return pc_decode_impl(bitstream, nbytes, first_sym, wtab_host, centers, k, L, resolution, symbols, status, C, h, w, workspace,
                          flags, channels, fill_sym, stream);
}

// ---- the tile entries: nine of them, behind them one request, one check, one workspace layout, one launch ------------------------

// a slot (k = 24): a tile's padded volume and its three caches
static size_t pc_dec_tile_slot_bytes(int C, int th, int tw, int k) {
    return pc_dec_align((size_t)(C + 4) * (th + 8) * (tw + 8) * sizeof(float)) + pc_dec_cache_bytes(C, th, tw, k);
}

// What an entry is given besides the tile table, which all have: it requires the host pointers of these, and its workspace holds
// their device copies.
enum : unsigned {
    PC_TILES_VOLUMES = 1,             // the volume table: every entry but ic_pc_decode_tiles_f32, which has one (h, w)
    PC_TILES_SEGS = 2,                // segment table and layer ends: the layers and fronts entries
    PC_TILES_LIMITS = 4,              // a channel limit per tile: their pertile and resume forms
    PC_TILES_RESUME = 8,              // the layer every tile continues with, and the done words that no copy touches: the resume forms
    PC_TILES_PLANES = 16,             // the symbol planes: ic_pc_decode_tiles_batch_fronts_resume_f32
    PC_TILES_LAYERS = PC_TILES_VOLUMES | PC_TILES_SEGS,
    PC_TILES_PERTILE = PC_TILES_LAYERS | PC_TILES_LIMITS,
    PC_TILES_LAYERS_RESUME = PC_TILES_PERTILE | PC_TILES_RESUME,
    PC_TILES_FRONTS_RESUME = PC_TILES_LAYERS_RESUME | PC_TILES_PLANES,
};

// Where everything lies in a tile entry's workspace, as offsets.  The size functions return `total`, the entries take their pointers
// from the rest, and nothing else in this file knows the order: tile table, volume table, segment table, layer ends, limits, from,
// done -- each aligned, those the entry does not have empty.  Then either one slot per tile (k = 24) or what the single-volume paths
// need for the largest tile plus that tile's symbols (the slow path), the larger of the two.  Last the symbol planes, a byte per
// symbol of the largest tile, per tile: behind everything the layers resume entry lays out, so that the two resume entries may be
// handed the same workspace and share everything up to the done words.
struct PcTilesLayout { size_t tiles, volumes, segs, ends, limits, from, done, slots, planes, total, slot_bytes, plane_bytes; };

static PcTilesLayout pc_tiles_layout(int C, int th_max, int tw_max, int ntiles, int nvolumes, int k, int nlayers, unsigned tables) {
    PcTilesLayout l{};
    size_t p = 0;
    const auto table = [&p](unsigned present, size_t bytes) { const size_t at = p; p += present ? pc_dec_align(bytes) : 0; return at; };
    l.tiles = table(1, (size_t)ntiles * sizeof(ic_pc_tile_t));
    l.volumes = table(tables & PC_TILES_VOLUMES, (size_t)nvolumes * sizeof(ic_pc_volume_t));
    l.segs = table(tables & PC_TILES_SEGS, (size_t)ntiles * nlayers * sizeof(ic_pc_seg_t));
    l.ends = table(tables & PC_TILES_SEGS, (size_t)nlayers * sizeof(int));
    l.limits = table(tables & PC_TILES_LIMITS, (size_t)ntiles * sizeof(int));
    l.from = table(tables & PC_TILES_RESUME, (size_t)ntiles * sizeof(int));
    l.done = table(tables & PC_TILES_RESUME, (size_t)ntiles * sizeof(int));
    l.slot_bytes = pc_dec_tile_slot_bytes(C, th_max, tw_max, k);
    const size_t slots = k == 24 ? (size_t)ntiles * l.slot_bytes : 0;
    const size_t loop = ic_pc_decode_workspace_bytes(C, th_max, tw_max, k) + pc_dec_align((size_t)C * th_max * tw_max * sizeof(int64_t));
    l.slots = p; p += slots > loop ? slots : loop;
    l.plane_bytes = pc_dec_align((size_t)C * th_max * tw_max);
    l.planes = p; p += (tables & PC_TILES_PLANES) ? (size_t)ntiles * l.plane_bytes : 0;
    l.total = p;
    return l;
}

// what the eight size functions return: the layout's total, 0 for counts that no entry takes
static size_t pc_tiles_workspace_bytes(int C, int th_max, int tw_max, int ntiles, int nvolumes, int k, int nlayers, unsigned tables) {
    if (C <= 0 || th_max <= 0 || tw_max <= 0 || ntiles <= 0 || k <= 0) return 0;
    if ((tables & PC_TILES_VOLUMES) && nvolumes <= 0) return 0;
    if ((tables & PC_TILES_SEGS) && (nlayers < 1 || nlayers > 16)) return 0;
    return pc_tiles_layout(C, th_max, tw_max, ntiles, nvolumes, k, nlayers, tables).total;
}

// Everything an entry is given (host only, not ABI).  `tables` says which entry it is: which of the pointers below it requires and
// what its workspace holds.  What an entry does not have keeps the value pc_tiles_request gives it.
struct PcTilesRequest {
    unsigned tables;
    const uint8_t* bitstreams; long long total_bytes; const ic_pc_tile_t* tiles; int ntiles;
    const ic_pc_volume_t* volumes; int nvolumes;      // PC_TILES_VOLUMES; else nvolumes is 0 and
    ic_pc_volume_t one;                               //   this is the volume: it travels in the kernel arguments, the tiles' `volume` is not read
    const float* const* wtab; const float* centers; int k, L; float resolution;
    int64_t* symbols; float* q;                       // symbols || q; the single-volume entry has no q, so symbols
    int* status; int C; void* workspace; size_t workspace_bytes;
    int flags;                                        // the caller's
    ic_stream_t stream;
    bool takes_channels;                              // the channels entry: like the segmented ones it has no slow path, whatever `channels`
    int channels, fill_sym;                           // channels == C: the full decode, whatever fill_sym; channels < C (k = 24 kernels only): the
                                                      //   first channels of every tile, the others fill_sym
    const int* ends; int nlayers; const ic_pc_seg_t* segs;        // PC_TILES_SEGS; else nlayers is 0
    const int* tile_channels;                         // PC_TILES_LIMITS: in place of `channels`, which is then C
    const int* tile_from;                             // PC_TILES_RESUME
    int order;                                        // what the decoder is told.  PC_TILES_SEGS: 0 (raster, plane cuts) or IC_PC_DECODE_WAVEFRONT
                                                      //   (front cuts), the caller's own flags must be 0 for both; else the caller's flags
    int th_max, tw_max;                               // the largest tile: pc_tiles_check fills them in
    int depth_block;                                  // IC_PC_DECODE_DEPTH(b) of the caller's flags, 0 without: pc_tiles_check fills it in
    int rans_lanes;                                   // IC_PC_DECODE_RANS(W) of the caller's flags, 0 without: pc_tiles_check fills it in
    bool rdo;                                         // IC_PC_DECODE_RDO, accepted: the streams are records, the sweep chooses symbols: pc_tiles_check fills it in
};

// the arguments that all entries but the single-volume one begin with, and the values of a full decode of unsegmented streams
static PcTilesRequest pc_tiles_request(unsigned tables, const uint8_t* bitstreams, long long total_bytes, const ic_pc_tile_t* tiles_host,
                                       int ntiles, const ic_pc_volume_t* volumes_host, int nvolumes, const float* const* wtab_host,
                                       const float* centers, int k, int L, float resolution, int64_t* symbols, float* q, int* status, int C,
                                       void* workspace, size_t workspace_bytes, int flags, ic_stream_t stream) {
    PcTilesRequest r{};
    r.tables = tables;
    r.bitstreams = bitstreams; r.total_bytes = total_bytes; r.tiles = tiles_host; r.ntiles = ntiles;
    r.volumes = volumes_host; r.nvolumes = nvolumes;
    r.wtab = wtab_host; r.centers = centers; r.k = k; r.L = L; r.resolution = resolution;
    r.symbols = symbols; r.q = q; r.status = status; r.C = C; r.workspace = workspace; r.workspace_bytes = workspace_bytes;
    r.flags = flags; r.stream = stream;
    r.channels = C; r.fill_sym = 0; r.order = flags;
    return r;
}

// what every entry asks of a descriptor, for a tile of an (h, w) volume
static bool pc_tile_ok(const ic_pc_tile_t& d, int h, int w, long long total_bytes, int L) {
    return d.th >= 1 && d.tw >= 1 && d.y0 >= 0 && d.x0 >= 0 && d.th <= h - d.y0 && d.tw <= w - d.x0 &&
           d.stream_off >= 0 && d.stream_bytes >= 0 && d.stream_off <= total_bytes && d.stream_bytes <= total_bytes - d.stream_off &&
           d.first_sym >= 0 && d.first_sym < L;
}

// Everything about the request and its tables is decided here, on the host, before the first HIP call and without a read through a
// device pointer: every fault of an argument first, then what is unsupported, then the workspace size.  -> th_max, tw_max, the layout.
static int pc_tiles_check(PcTilesRequest& r, PcTilesLayout& l) {
    const bool batch = r.tables & PC_TILES_VOLUMES, segmented = r.tables & PC_TILES_SEGS;
    const bool pertile = r.tables & PC_TILES_LIMITS, resume = r.tables & PC_TILES_RESUME;
    IC_CHECK_ARG(r.bitstreams && r.tiles && r.wtab && r.centers && (r.symbols || r.q) && r.status && r.workspace);
    IC_CHECK_ARG((!batch || r.volumes) && (!segmented || (r.ends && r.segs)) && (!pertile || r.tile_channels) && (!resume || r.tile_from));
    IC_CHECK_ARG(r.total_bytes >= 0 && r.ntiles > 0 && r.C > 0 && r.k > 0 && r.L > 0);
    IC_CHECK_ARG(batch ? r.nvolumes > 0 : r.one.h > 0 && r.one.w > 0);
    IC_CHECK_ARG(r.channels >= 1 && r.channels <= r.C && r.fill_sym >= 0 && r.fill_sym < r.L);
    if (segmented) {
        IC_CHECK_ARG(r.nlayers >= 1 && r.nlayers <= 16);
        IC_CHECK_ARG(r.ends[0] >= 1 && r.ends[r.nlayers - 1] == r.C);
        for (int g = 1; g < r.nlayers; ++g) IC_CHECK_ARG(r.ends[g] > r.ends[g - 1]);
    }
    for (int n = 0; n < r.nvolumes; ++n) {
        const ic_pc_volume_t& v = r.volumes[n];
        IC_CHECK_ARG(v.h >= 1 && v.w >= 1 && v.symbols_off >= 0 && v.q_off >= 0);
    }
    // the symbol chooser's flag where it can be accepted at all (the channels entry, alone in the flags): its tiles are records,
    // whose faults are faults of an argument like any other; everywhere else the flag is refused as unsupported further down
    const bool rdo_asked = (r.flags & IC_PC_DECODE_RDO) != 0;
    const bool records = r.takes_channels && batch && !segmented && r.flags == IC_PC_DECODE_RDO;
    IC_CHECK_ARG(!records || (uintptr_t)r.bitstreams % 8 == 0);
    r.th_max = r.tw_max = 0;
    for (int t = 0; t < r.ntiles; ++t) {
        ic_pc_tile_t d = r.tiles[t];
        if (rdo_asked) d.first_sym = 0;                   // ignored on input
        const int from = resume ? r.tile_from[t] : 0, limit = pertile ? r.tile_channels[t] : r.channels;
        IC_CHECK_ARG(from >= 0 && from <= r.nlayers);     // (from == nlayers: the tile is whole, its limit can only be C)
        IC_CHECK_ARG(limit >= 1 && limit <= r.C && (from ? r.ends[from - 1] : 0) <= limit);
        IC_CHECK_ARG(!batch || (d.volume >= 0 && d.volume < r.nvolumes));
        if (segmented) { d.stream_off = 0; d.stream_bytes = 0; }             // not read: the segments stand for them
        const ic_pc_volume_t& v = batch ? r.volumes[d.volume] : r.one;
        IC_CHECK_ARG(pc_tile_ok(d, v.h, v.w, r.total_bytes, r.L));
        IC_CHECK_ARG(!records || (d.stream_off % 8 == 0 && d.stream_bytes == 8 + 4ll * r.C * d.th * d.tw));
        // the segments THIS call reads: from `from` on (segment 0 only for a tile that starts afresh), of the layers that begin below
        // the limit, the launch's or the tile's own
        for (int g = from; g < r.nlayers && (g == 0 || r.ends[g - 1] < limit); ++g) {
            const ic_pc_seg_t& sg = r.segs[(size_t)t * r.nlayers + g];
            IC_CHECK_ARG(sg.off >= 0 && sg.nbytes >= 0 && sg.off <= r.total_bytes && sg.nbytes <= r.total_bytes - sg.off);
        }
        r.th_max = d.th > r.th_max ? d.th : r.th_max;
        r.tw_max = d.tw > r.tw_max ? d.tw : r.tw_max;
    }
    if (r.L > 16) return IC_ERR_UNSUPPORTED;
    // the depth plane (bits 8 - 15 of the flags) has one decoder too: the wavefront sweep with a limit of the k = 24 kernel, so the flag
    // is the channels entry's alone, there only beside IC_PC_DECODE_WAVEFRONT, and unsupported everywhere else.  Behind this the flags
    // are what they are without it.
    // the interleaved rANS coders (bits 16 - 23 of the flags) likewise: the channels entry's alone, k = 24, and there ALONE in the flags --
    // the order is implied; beside IC_PC_DECODE_WAVEFRONT, a depth block or a slow-path flag, with another W, in any other entry: unsupported
    // the symbol chooser (bit 24) likewise: the channels entry's alone, k = 24, alone in the flags, and over all channels
    r.rdo = false;
    if (rdo_asked) {
        if (!records || r.k != 24 || r.channels != r.C) return IC_ERR_UNSUPPORTED;
        r.rdo = true;
        r.flags = r.order = IC_PC_DECODE_WAVEFRONT;
    }
    r.rans_lanes = (r.flags >> 16) & 0xff;
    if (r.rans_lanes) {
        const int W = r.rans_lanes;
        if (!r.takes_channels || !batch || segmented || r.k != 24 || r.flags != IC_PC_DECODE_RANS(W) || !(W == 8 || W == 16 || W == 32 || W == 64))
            return IC_ERR_UNSUPPORTED;
        r.flags = r.order = IC_PC_DECODE_WAVEFRONT;
    }
    r.depth_block = (r.flags >> 8) & 0xff;
    if (r.depth_block) {
        if (!r.takes_channels || !batch || segmented || r.k != 24 || r.flags != (IC_PC_DECODE_WAVEFRONT | IC_PC_DECODE_DEPTH(r.depth_block)))
            return IC_ERR_UNSUPPORTED;
        r.flags = r.order = IC_PC_DECODE_WAVEFRONT;
    }
    // the wavefront order has one decoder, the k = 24 kernel: no slow path, no combination with the test flags -- and as a flag it
    // is the unsegmented batch entries' alone (the fronts entries are told by their name, their flags are 0 like the layers entries')
    if ((r.flags & IC_PC_DECODE_WAVEFRONT) && (!batch || segmented || r.k != 24 || r.flags != IC_PC_DECODE_WAVEFRONT)) return IC_ERR_UNSUPPORTED;
    // only the k = 24 kernels have the channel limit and the segments: no slow path for the entries that take either
    if ((r.takes_channels || segmented) && (r.k != 24 || (r.flags & ~IC_PC_DECODE_WAVEFRONT))) return IC_ERR_UNSUPPORTED;
    l = pc_tiles_layout(r.C, r.th_max, r.tw_max, r.ntiles, r.nvolumes, r.k, r.nlayers, r.tables);
    if (r.workspace_bytes < l.total) return IC_ERR_WORKSPACE;
    return IC_OK;
}

// the form of pc_dec_tiles_batch_kernel for a launch, by its template arguments (per implies lim and seg, from implies per; depth is
// the wavefront sweep with a limit and without segments): the 28 forms named here are the ones the file instantiates
typedef void (*PcTilesKernel)(const PcTilesBatchArgs);
template <bool WAVE, bool LIM, bool SEG, bool PER, bool FROM>
static PcTilesKernel pc_tiles_kernel_of(bool syms) {
    return syms ? pc_dec_tiles_batch_kernel<WAVE, true, LIM, SEG, PER, FROM> : pc_dec_tiles_batch_kernel<WAVE, false, LIM, SEG, PER, FROM>;
}
static PcTilesKernel pc_tiles_kernel(bool wave, bool syms, bool lim, bool seg, bool per, bool from, bool depth, bool rans) {
    if (rans) return syms ? pc_dec_tiles_batch_kernel<true, true, true, false, false, false, false, true>
                          : pc_dec_tiles_batch_kernel<true, false, true, false, false, false, false, true>;     // (pc_tiles_check: wave, not seg, no depth)
    if (depth) return syms ? pc_dec_tiles_batch_kernel<true, true, true, false, false, false, true>
                           : pc_dec_tiles_batch_kernel<true, false, true, false, false, false, true>;     // (pc_tiles_check: wave, not seg)
    if (!seg) return !lim ? (wave ? pc_tiles_kernel_of<true, false, false, false, false>(syms) : pc_tiles_kernel_of<false, false, false, false, false>(syms))
                          : (wave ? pc_tiles_kernel_of<true, true, false, false, false>(syms) : pc_tiles_kernel_of<false, true, false, false, false>(syms));
    if (!wave) return !lim ? pc_tiles_kernel_of<false, false, true, false, false>(syms) : !per ? pc_tiles_kernel_of<false, true, true, false, false>(syms)
                    : !from ? pc_tiles_kernel_of<false, true, true, true, false>(syms) : pc_tiles_kernel_of<false, true, true, true, true>(syms);
    return !lim ? pc_tiles_kernel_of<true, false, true, false, false>(syms) : !per ? pc_tiles_kernel_of<true, true, true, false, false>(syms)
         : !from ? pc_tiles_kernel_of<true, true, true, true, false>(syms) : pc_tiles_kernel_of<true, true, true, true, true>(syms);
}

// The tiles of one call, behind pc_tiles_check.
static int pc_decode_tiles_impl(const PcTilesRequest& r, const PcTilesLayout& l) {
    const bool wavefront = (r.order & IC_PC_DECODE_WAVEFRONT) != 0;
    hipStream_t st = (hipStream_t)r.stream;
    char* const ws = (char*)r.workspace;
    const int ntiles = r.ntiles, C = r.C;
    if (r.k == 24 && (r.order == 0 || wavefront)) {
        PcTilesBatchArgs a{};
        // the tables are pageable host memory: the runtime has taken its copy of them when these return
        const auto upload = [&](size_t at, const void* host, size_t bytes) {
            return hipMemcpyAsync(ws + at, host, bytes, hipMemcpyHostToDevice, st) == hipSuccess;
        };
        if (!upload(l.tiles, r.tiles, (size_t)ntiles * sizeof(ic_pc_tile_t))) return IC_ERR_ARG;
        a.tiles = (const ic_pc_tile_t*)(ws + l.tiles);
        if (r.nvolumes) {
            if (!upload(l.volumes, r.volumes, (size_t)r.nvolumes * sizeof(ic_pc_volume_t))) return IC_ERR_ARG;
            a.volumes = (const ic_pc_volume_t*)(ws + l.volumes);
        } else {
            a.one = r.one;
        }
        if (r.nlayers) {              // the layers and fronts entries
            if (!upload(l.segs, r.segs, (size_t)ntiles * r.nlayers * sizeof(ic_pc_seg_t))) return IC_ERR_ARG;
            if (!upload(l.ends, r.ends, (size_t)r.nlayers * sizeof(int))) return IC_ERR_ARG;
            a.segs = (const ic_pc_seg_t*)(ws + l.segs); a.ends = (const int*)(ws + l.ends); a.nlayers = r.nlayers;
        }
        if (r.tile_channels) {        // their pertile and resume forms
            if (!upload(l.limits, r.tile_channels, (size_t)ntiles * sizeof(int))) return IC_ERR_ARG;
            a.tile_channels = (const int*)(ws + l.limits);
        }
        if (r.tile_from) {            // the resume forms: `done` is the kernel's alone, no copy touches it
            if (!upload(l.from, r.tile_from, (size_t)ntiles * sizeof(int))) return IC_ERR_ARG;
            a.tile_from = (const int*)(ws + l.from);
            a.done = (int*)(ws + l.done);
            if (wavefront) { a.planes = (unsigned char*)ws + l.planes; a.plane_bytes = l.plane_bytes; }
        }
        a.f.d.centers = r.centers; a.f.d.C = C; a.f.d.L = r.L; a.f.d.resolution = r.resolution;
        a.f.w0 = r.wtab[0]; a.f.b0 = r.wtab[1]; a.f.w1 = r.wtab[2]; a.f.b1 = r.wtab[3];
        a.f.w2 = r.wtab[4]; a.f.b2 = r.wtab[5]; a.f.w3 = r.wtab[6]; a.f.b3 = r.wtab[7];
        a.bits = r.bitstreams; a.slots = ws + l.slots; a.slot_bytes = l.slot_bytes;
        a.off_c0 = pc_dec_align((size_t)(C + 4) * (r.th_max + 8) * (r.tw_max + 8) * sizeof(float));
        a.off_c1 = a.off_c0 + pc_dec_align(pc_dec_cache_floats(C, r.th_max, r.tw_max, r.k, 0) * sizeof(float));
        a.off_c2 = a.off_c1 + pc_dec_align(pc_dec_cache_floats(C, r.th_max, r.tw_max, r.k, 1) * sizeof(float));
        a.symbols = (long long*)r.symbols; a.q = r.q; a.status = r.status;
        const long long nvol = (long long)(C + 4) * (r.th_max + 8) * (r.tw_max + 8);
        if (r.tile_from)
            hipLaunchKernelGGL(pc_dec_fill_fresh_slots_kernel, dim3((unsigned)((nvol + 255) / 256), (unsigned)ntiles), dim3(256), 0, st,
                               a.slots, a.slot_bytes, nvol, r.centers, a.tile_from);
        else
            hipLaunchKernelGGL(pc_dec_fill_slots_kernel, dim3((unsigned)((nvol + 255) / 256), (unsigned)ntiles), dim3(256), 0, st,
                               a.slots, a.slot_bytes, nvol, r.centers);
        a.cdec = r.channels; a.fill = r.fill_sym; a.depth_block = r.depth_block; a.rans_lanes = r.rans_lanes;
        const PcTilesKernel kernel = pc_tiles_kernel(wavefront, r.symbols != nullptr, r.tile_channels || r.channels < C || r.rans_lanes, r.nlayers != 0,
                                                     r.tile_channels != nullptr, r.tile_from != nullptr, r.depth_block != 0, r.rans_lanes != 0);
        if (r.rdo) {
            if (r.symbols) hipLaunchKernelGGL(pc_rdo_tiles_batch_kernel<true>, dim3((unsigned)ntiles), dim3(256), 0, st, a);
            else hipLaunchKernelGGL(pc_rdo_tiles_batch_kernel<false>, dim3((unsigned)ntiles), dim3(256), 0, st, a);
        } else
        hipLaunchKernelGGL(kernel, dim3((unsigned)ntiles), dim3(256), 0, st, a);
        IC_LAUNCH_CHECK();
        return IC_OK;
    }
    // the slow path (other k, or one of the test flags): tile after tile through the single-volume decoder, then into place
    char* const p = ws + l.slots;
    const size_t loop_ws = ic_pc_decode_workspace_bytes(C, r.th_max, r.tw_max, r.k);
    int64_t* tile_syms = (int64_t*)(p + loop_ws);
    for (int t = 0; t < ntiles; ++t) {
        const ic_pc_tile_t& d = r.tiles[t];
        const ic_pc_volume_t& v = r.nvolumes ? r.volumes[d.volume] : r.one;
        const int rc = ic_pc_decode_f32(r.bitstreams + d.stream_off, d.stream_bytes, d.first_sym, r.wtab, r.centers, r.k, r.L, r.resolution,
                                        tile_syms, r.status + t, C, d.th, d.tw, p, loop_ws, r.flags, r.stream);
        if (rc) return rc;
        const long long n = (long long)C * d.th * d.tw;
        hipLaunchKernelGGL(pc_tile_place_batch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const long long*)tile_syms,
                           r.symbols ? (long long*)r.symbols + v.symbols_off : nullptr, r.q ? r.q + v.q_off : nullptr, r.centers,
                           C, d.th, d.tw, v.h, v.w, d.y0, d.x0);
    }
    IC_LAUNCH_CHECK();
    return IC_OK;
}

static int pc_decode_tiles(PcTilesRequest r) {
    PcTilesLayout l;
    const int rc = pc_tiles_check(r, l);
    return rc ? rc : pc_decode_tiles_impl(r, l);
}

extern "C" size_t ic_pc_decode_tiles_workspace_bytes(int C, int th_max, int tw_max, int ntiles, int k) {
    return pc_tiles_workspace_bytes(C, th_max, tw_max, ntiles, 0, k, 0, 0);
}

extern "C" int ic_pc_decode_tiles_f32(const uint8_t* bitstreams, long long total_bytes, const ic_pc_tile_t* tiles_host, int ntiles,
                                      const float* const* wtab_host, const float* centers, int k, int L, float resolution,
                                      int64_t* symbols, int* status, int C, int h, int w, void* workspace,
                                      size_t workspace_bytes, int flags, ic_stream_t stream) {
    PcTilesRequest r = pc_tiles_request(0, bitstreams, total_bytes, tiles_host, ntiles, nullptr, 0, wtab_host, centers, k, L, resolution,
                                        symbols, nullptr, status, C, workspace, workspace_bytes, flags, stream);
    r.one = {h, w, 0, 0};
    return pc_decode_tiles(r);
}

extern "C" size_t ic_pc_decode_tiles_batch_workspace_bytes(int C, int th_max, int tw_max, int ntiles, int nvolumes, int k) {
    return pc_tiles_workspace_bytes(C, th_max, tw_max, ntiles, nvolumes, k, 0, PC_TILES_VOLUMES);
}

extern "C" int ic_pc_decode_tiles_batch_f32(const uint8_t* bitstreams, long long total_bytes, const ic_pc_tile_t* tiles_host, int ntiles,
                                            const ic_pc_volume_t* volumes_host, int nvolumes, const float* const* wtab_host,
                                            const float* centers, int k, int L, float resolution, int64_t* symbols, float* q,
                                            int* status, int C, void* workspace, size_t workspace_bytes, int flags,
                                            ic_stream_t stream) {
    return pc_decode_tiles(pc_tiles_request(PC_TILES_VOLUMES, bitstreams, total_bytes, tiles_host, ntiles, volumes_host, nvolumes, wtab_host,
                                            centers, k, L, resolution, symbols, q, status, C, workspace, workspace_bytes, flags, stream));
}

// preview of the tiles of several volumes: as above with the channel limit; flags is 0 or IC_PC_DECODE_WAVEFRONT, k is 24
extern "C" int ic_pc_decode_tiles_batch_channels_f32(const uint8_t* bitstreams, long long total_bytes, const ic_pc_tile_t* tiles_host, int ntiles,
                                                     const ic_pc_volume_t* volumes_host, int nvolumes, const float* const* wtab_host,
                                                     const float* centers, int k, int L, float resolution, int64_t* symbols, float* q,
                                                     int* status, int C, void* workspace, size_t workspace_bytes, int flags,
                                                     ic_stream_t stream, int channels, int fill_sym) {
    PcTilesRequest r = pc_tiles_request(PC_TILES_VOLUMES, bitstreams, total_bytes, tiles_host, ntiles, volumes_host, nvolumes, wtab_host,
                                        centers, k, L, resolution, symbols, q, status, C, workspace, workspace_bytes, flags, stream);
    r.takes_channels = true; r.channels = channels; r.fill_sym = fill_sym;
    return pc_decode_tiles(r);
}

// the segmented entries' own arguments: the limit is the launch's (`channels`) or the tiles' own (tile_channels_host, channels = C);
// tile_from_layer_host: the resume entries; order: what the entry's name says
static int pc_decode_tiles_segments(PcTilesRequest r, int channels, const int* tile_channels_host, const int* tile_from_layer_host,
                                    int fill_sym, const int* layer_ends_host, int nlayers, const ic_pc_seg_t* segs_host, int order) {
    r.channels = channels; r.fill_sym = fill_sym;
    r.tile_channels = tile_channels_host; r.tile_from = tile_from_layer_host;
    r.ends = layer_ends_host; r.nlayers = nlayers; r.segs = segs_host; r.order = order;
    return pc_decode_tiles(r);
}

// ---- layered tiles (container format 6): every tile's raster stream as nlayers segments --------------------------------------
extern "C" size_t ic_pc_decode_tiles_batch_layers_workspace_bytes(int C, int th_max, int tw_max, int ntiles, int nvolumes, int k, int nlayers) {
    return pc_tiles_workspace_bytes(C, th_max, tw_max, ntiles, nvolumes, k, nlayers, PC_TILES_LAYERS);
}

extern "C" int ic_pc_decode_tiles_batch_layers_f32(const uint8_t* bitstreams, long long total_bytes, const ic_pc_tile_t* tiles_host, int ntiles,
                                                   const ic_pc_volume_t* volumes_host, int nvolumes, const float* const* wtab_host,
                                                   const float* centers, int k, int L, float resolution, int64_t* symbols, float* q,
                                                   int* status, int C, void* workspace, size_t workspace_bytes, int flags,
                                                   ic_stream_t stream, int channels, int fill_sym,
                                                   const int* layer_ends_host, int nlayers, const ic_pc_seg_t* segs_host) {
    return pc_decode_tiles_segments(pc_tiles_request(PC_TILES_LAYERS, bitstreams, total_bytes, tiles_host, ntiles, volumes_host, nvolumes, wtab_host,
                                                     centers, k, L, resolution, symbols, q, status, C, workspace, workspace_bytes, flags, stream),
                                    channels, nullptr, nullptr, fill_sym, layer_ends_host, nlayers, segs_host, 0);
}

// ---- layered tiles with a channel limit per tile: what a damaged or cut format-6 file still holds of every tile ---------------
extern "C" size_t ic_pc_decode_tiles_batch_layers_pertile_workspace_bytes(int C, int th_max, int tw_max, int ntiles, int nvolumes, int k, int nlayers) {
    return pc_tiles_workspace_bytes(C, th_max, tw_max, ntiles, nvolumes, k, nlayers, PC_TILES_PERTILE);
}

extern "C" int ic_pc_decode_tiles_batch_layers_pertile_f32(const uint8_t* bitstreams, long long total_bytes, const ic_pc_tile_t* tiles_host, int ntiles,
                                                           const ic_pc_volume_t* volumes_host, int nvolumes, const float* const* wtab_host,
                                                           const float* centers, int k, int L, float resolution, int64_t* symbols, float* q,
                                                           int* status, int C, void* workspace, size_t workspace_bytes, int flags,
                                                           ic_stream_t stream, const int* tile_channels_host, int fill_sym,
                                                           const int* layer_ends_host, int nlayers, const ic_pc_seg_t* segs_host) {
    return pc_decode_tiles_segments(pc_tiles_request(PC_TILES_PERTILE, bitstreams, total_bytes, tiles_host, ntiles, volumes_host, nvolumes, wtab_host,
                                                     centers, k, L, resolution, symbols, q, status, C, workspace, workspace_bytes, flags, stream),
                                    C, tile_channels_host, nullptr, fill_sym, layer_ends_host, nlayers, segs_host, 0);
}

// ---- front-layered tiles (container format 8): every tile's wavefront-ordered stream as nlayers segments cut at fronts ------------
// The arguments, the checks and the workspace of the two layered entries; only the meaning of a segment differs (pc_dec_wave_body, SEG).
extern "C" size_t ic_pc_decode_tiles_batch_fronts_workspace_bytes(int C, int th_max, int tw_max, int ntiles, int nvolumes, int k, int nlayers) {
    return pc_tiles_workspace_bytes(C, th_max, tw_max, ntiles, nvolumes, k, nlayers, PC_TILES_LAYERS);
}

extern "C" int ic_pc_decode_tiles_batch_fronts_f32(const uint8_t* bitstreams, long long total_bytes, const ic_pc_tile_t* tiles_host, int ntiles,
                                                   const ic_pc_volume_t* volumes_host, int nvolumes, const float* const* wtab_host,
                                                   const float* centers, int k, int L, float resolution, int64_t* symbols, float* q,
                                                   int* status, int C, void* workspace, size_t workspace_bytes, int flags,
                                                   ic_stream_t stream, int channels, int fill_sym,
                                                   const int* layer_ends_host, int nlayers, const ic_pc_seg_t* segs_host) {
    return pc_decode_tiles_segments(pc_tiles_request(PC_TILES_LAYERS, bitstreams, total_bytes, tiles_host, ntiles, volumes_host, nvolumes, wtab_host,
                                                     centers, k, L, resolution, symbols, q, status, C, workspace, workspace_bytes, flags, stream),
                                    channels, nullptr, nullptr, fill_sym, layer_ends_host, nlayers, segs_host, IC_PC_DECODE_WAVEFRONT);
}

extern "C" size_t ic_pc_decode_tiles_batch_fronts_pertile_workspace_bytes(int C, int th_max, int tw_max, int ntiles, int nvolumes, int k, int nlayers) {
    return pc_tiles_workspace_bytes(C, th_max, tw_max, ntiles, nvolumes, k, nlayers, PC_TILES_PERTILE);
}

extern "C" int ic_pc_decode_tiles_batch_fronts_pertile_f32(const uint8_t* bitstreams, long long total_bytes, const ic_pc_tile_t* tiles_host, int ntiles,
                                                           const ic_pc_volume_t* volumes_host, int nvolumes, const float* const* wtab_host,
                                                           const float* centers, int k, int L, float resolution, int64_t* symbols, float* q,
                                                           int* status, int C, void* workspace, size_t workspace_bytes, int flags,
                                                           ic_stream_t stream, const int* tile_channels_host, int fill_sym,
                                                           const int* layer_ends_host, int nlayers, const ic_pc_seg_t* segs_host) {
    return pc_decode_tiles_segments(pc_tiles_request(PC_TILES_PERTILE, bitstreams, total_bytes, tiles_host, ntiles, volumes_host, nvolumes, wtab_host,
                                                     centers, k, L, resolution, symbols, q, status, C, workspace, workspace_bytes, flags, stream),
                                    C, tile_channels_host, nullptr, fill_sym, layer_ends_host, nlayers, segs_host, IC_PC_DECODE_WAVEFRONT);
}

// ---- layered tiles, continued: every tile from the layer where an earlier call on the same workspace stopped --------------------
extern "C" size_t ic_pc_decode_tiles_batch_layers_resume_workspace_bytes(int C, int th_max, int tw_max, int ntiles, int nvolumes, int k, int nlayers) {
    return pc_tiles_workspace_bytes(C, th_max, tw_max, ntiles, nvolumes, k, nlayers, PC_TILES_LAYERS_RESUME);
}

extern "C" int ic_pc_decode_tiles_batch_layers_resume_f32(const uint8_t* bitstreams, long long total_bytes, const ic_pc_tile_t* tiles_host, int ntiles,
                                                          const ic_pc_volume_t* volumes_host, int nvolumes, const float* const* wtab_host,
                                                          const float* centers, int k, int L, float resolution, int64_t* symbols, float* q,
                                                          int* status, int C, void* workspace, size_t workspace_bytes, int flags,
                                                          ic_stream_t stream, const int* tile_from_layer_host, const int* tile_channels_host,
                                                          int fill_sym, const int* layer_ends_host, int nlayers, const ic_pc_seg_t* segs_host) {
    return pc_decode_tiles_segments(pc_tiles_request(PC_TILES_LAYERS_RESUME, bitstreams, total_bytes, tiles_host, ntiles, volumes_host, nvolumes, wtab_host,
                                                     centers, k, L, resolution, symbols, q, status, C, workspace, workspace_bytes, flags, stream),
                                    C, tile_channels_host, tile_from_layer_host, fill_sym, layer_ends_host, nlayers, segs_host, 0);
}

// ---- front-layered tiles, continued: every tile's front sweep from the layer end where an earlier call on the same workspace stopped ---
extern "C" size_t ic_pc_decode_tiles_batch_fronts_resume_workspace_bytes(int C, int th_max, int tw_max, int ntiles, int nvolumes, int k, int nlayers) {
    return pc_tiles_workspace_bytes(C, th_max, tw_max, ntiles, nvolumes, k, nlayers, PC_TILES_FRONTS_RESUME);
}

extern "C" int ic_pc_decode_tiles_batch_fronts_resume_f32(const uint8_t* bitstreams, long long total_bytes, const ic_pc_tile_t* tiles_host, int ntiles,
                                                          const ic_pc_volume_t* volumes_host, int nvolumes, const float* const* wtab_host,
                                                          const float* centers, int k, int L, float resolution, int64_t* symbols, float* q,
                                                          int* status, int C, void* workspace, size_t workspace_bytes, int flags,
                                                          ic_stream_t stream, const int* tile_from_layer_host, const int* tile_channels_host,
                                                          int fill_sym, const int* layer_ends_host, int nlayers, const ic_pc_seg_t* segs_host) {
    return pc_decode_tiles_segments(pc_tiles_request(PC_TILES_FRONTS_RESUME, bitstreams, total_bytes, tiles_host, ntiles, volumes_host, nvolumes, wtab_host,
                                                     centers, k, L, resolution, symbols, q, status, C, workspace, workspace_bytes, flags, stream),
                                    C, tile_channels_host, tile_from_layer_host, fill_sym, layer_ends_host, nlayers, segs_host, IC_PC_DECODE_WAVEFRONT);
}
