// Device range ENCODER of the real-bpp path: the mirror image of ic_pc_decode_f32 (pc_decode.hip).
//   host statement: arithmetic_coding.encode_sequence(symbols[1:], freqs[1:]) over the tables of PredictionNetwork.get_all;
//   the bytes written here are identical to that coder's (tests/test_gpu_codec.py), which tests/golden/arithcoding.npz pins to
//   the reference coder.
//
// What moved: the host path materialises the int64 table and the fp32 probabilities of EVERY position (count x L x 12 bytes,
// 14 MB for a Kodak volume), copies them to the host and steps a Python coder over them.  Here the table row of a symbol lives
// in the registers of one lane for as long as it takes to pick (cum_lo, cum_hi, total) of the symbol that occurred; nothing
// but the byte stream (~18 KB for that volume) is written.
//
// Work mapping: one work-group of two waves per volume (grid = N); ic_pc_encode_segments_f32: per segment of a volume (grid = N * nsegs).
//   wave 1, producer: chunk c + 1 = 64 consecutive symbols, one per lane: pc_table_row (softmax, L expf, truncation -- the
//       expression the decoder uses), prefix sums up to the symbol, 1.0 / total in double.  Result: three LDS words + one double
//       per symbol, double-buffered.
//   wave 0, coder: chunk c, strictly sequential (the range after a symbol depends on every earlier rounding).  Each lane loads
//       the triple of "its" symbol once; step k reads lane k's values with v_readlane, so the serial chain holds no LDS or
//       memory latency and never waits for an expf: the producer runs one chunk ahead, behind one barrier per 64 symbols.
// Serial step (word level; the host coder's loops per bit, restated):
//   narrow   r = high - low + 1 (<= 2^32);  high = low + cum_hi r / total - 1;  low += cum_lo r / total   (64-bit products)
//   shift    n = clz(low ^ high) equal leading bits leave at once: the first, then the pending run inverted, then the rest
//   underflow m = number of leading (low = 1, high = 0) positions below the top bit, dropped at once; pending += m
//   output   64-bit reservoir, flushed in whole bytes (lane j stores byte j of a flush: one vector store per flush);
//            a pending run longer than the reservoir is aligned to a byte and stored as whole 0x00 / 0xff bytes.
#include "common.h"
#include "pc_table.h"

#define PCE_CHUNK 64
#define PCE_MAX_TOTAL ((1u << 30) + 2u)       // arithmetic_coding.MAX_TOTAL for 32 state bits

struct PcEncArgs {
    const float* logits;          // (N, count, L)
    const long long* symbols;     // (N, count)
    unsigned char* out;           // (N, capacity)
    long long* nbytes;            // (N)
    int* status;                  // (N)
    long long count, capacity;
    float resolution;
};

// byte sink of one volume; identical in every lane of the coder wave
struct PceSink {
    unsigned char* p;
    long long pos, cap;
    unsigned long long res;       // the low `nres` bits are waiting, oldest bit highest
    int nres;                     // < 8 between calls
    int ovf;
};

// append the low k bits of `bits` (k <= 56, the other bits of `bits` zero); whole bytes leave at once
__device__ __forceinline__ void pce_put(PceSink& o, unsigned long long bits, int k, int lane) {
    if (o.ovf) return;
    o.res = (o.res << k) | bits;
    o.nres += k;
    if (o.nres >= 8) {
        const int nb = o.nres >> 3, rem = o.nres & 7;
        if (o.pos + nb > o.cap) { o.ovf = 1; return; }                   // never a store at or beyond capacity
        if (lane < nb) o.p[o.pos + lane] = (unsigned char)(o.res >> (rem + 8 * (nb - 1 - lane)));
        o.pos += nb;
        o.nres = rem;
        o.res &= (1ull << rem) - 1;
    }
}

// p copies of `bit`; p has no upper bound (every underflow step of the coder adds to the pending run)
__device__ __forceinline__ void pce_put_run(PceSink& o, int bit, long long p, int lane) {
    const unsigned long long ones = bit ? ~0ull : 0ull;
    if (p <= 48) { pce_put(o, ones & ((1ull << p) - 1), (int)p, lane); return; }
    const int k = 8 - o.nres;                                            // 1..8 bits complete the current byte
    pce_put(o, ones & ((1ull << k) - 1), k, lane);
    p -= k;
    if (o.ovf) return;
    const long long nb = p >> 3;                                         // whole bytes of the run, stored 64 per pass
    if (o.pos + nb > o.cap) { o.ovf = 1; return; }
    for (long long i = lane; i < nb; i += 64) o.p[o.pos + i] = (unsigned char)ones;
    o.pos += nb;
    const int t = (int)(p & 7);
    pce_put(o, ones & ((1ull << t) - 1), t, lane);
}

// floor(n / d) for n < 2^63, 1 <= d <= 2^30 + 2, n / d <= 2^32, with inv = 1.0 / (double)d computed off the serial path.
// Exact: (double)n, inv and their product each carry a relative rounding error <= 2^-53, so the product differs from n / d by
// less than 2^32 * 3.01 * 2^-53 < 2^-19; its integer part is therefore floor(n / d) - 1, floor(n / d) or floor(n / d) + 1, and
// the exact 64-bit remainder n - q d decides which (one correction step in either direction suffices).
__device__ __forceinline__ unsigned long long pce_div(unsigned long long n, unsigned d, double inv) {
    unsigned long long q = (unsigned long long)((double)n * inv);
    const long long rem = (long long)(n - q * d);
    if (rem < 0) --q; else if (rem >= (long long)d) ++q;
    return q;
}

__device__ __forceinline__ unsigned pce_lane_u32(unsigned v, int src) { return (unsigned)__builtin_amdgcn_readlane((int)v, src); }

// One coder run by one work-group of two waves: symbols [first, end) of the volume whose logits / symbols start at `logits` /
// `symbols` (first >= 1: symbol 0 of a volume is never coded), the coder started afresh and terminated at the end, its bytes at
// out[0 .. cap), their number and the status in *nbytes_out / *status_out.  first == end is the one byte 0x80.
template <int LC>
__device__ __forceinline__ void pce_code_range(const float* __restrict__ logits, const long long* __restrict__ symbols, long long first,
                                               long long end, float resolution, unsigned char* out, long long cap,
                                               long long* nbytes_out, int* status_out) {
    __shared__ unsigned s_lo[2][PCE_CHUNK], s_hi[2][PCE_CHUNK], s_tot[2][PCE_CHUNK];
    __shared__ double s_inv[2][PCE_CHUNK];
    __shared__ int s_stop[2];            // by chunk parity: a wave still reading chunk c's flag is not overtaken by chunk c + 1's
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long ncoded = end - first;
    const long long nchunks = (ncoded + PCE_CHUNK - 1) / PCE_CHUNK;

    PceSink o;
    o.p = out; o.pos = 0; o.cap = cap; o.res = 0; o.nres = 0; o.ovf = 0;
    unsigned low = 0, high = 0xffffffffu;
    long long pending = 0;
    int err = 0;
    if (threadIdx.x < 2) s_stop[threadIdx.x] = 0;
    __syncthreads();

    for (long long c = 0; c <= nchunks; ++c) {
        if (wave == 1 && c < nchunks) {
            // ---- producer: the table of symbol i, reduced to what the coder needs of it ----
            const long long i = first + c * PCE_CHUNK + lane;
            const int b = (int)(c & 1);
            const long long sym = i < end ? symbols[i] : 0;
            if (i < end && sym == IC_PC_ENCODE_SKIP) {
                // a position the stream does not code: the whole interval, (cum_lo, cum_hi, total) = (0, 1, 1).  With r = high - low + 1
                // the coder's step gives high = low + r - 1 and low += 0, both unchanged, and the state it starts from is renormalised
                // (top bits differ, no underflow position), so nothing is shifted out either: the serial loop steps over it as it is.
                // The logits of the position are not read.
                s_lo[b][lane] = 0u;
                s_hi[b][lane] = 1u;
                s_tot[b][lane] = 1u;
                s_inv[b][lane] = 1.0;
            } else if (i < end) {
                float l[LC];
#pragma unroll
                for (int j = 0; j < LC; ++j) l[j] = logits[i * LC + j];
                long long fr[LC];
                pc_table_row(l, LC, resolution, fr, nullptr);
                unsigned long long lo = 0, f = 0, total = 0;
                bool big = false;
#pragma unroll
                for (int j = 0; j < LC; ++j) {
                    const unsigned long long fj = (unsigned long long)fr[j];
                    big |= fj > PCE_MAX_TOTAL;                            // also keeps the sums below from wrapping
                    total += fj;
                    if (j < sym) lo += fj;
                    if (j == sym) f = fj;
                }
                big |= total > PCE_MAX_TOTAL;
                // total word: 0 = symbol outside [0, L) (status 3), 0xffffffff = table too large (status 1)
                const unsigned tw = (sym < 0 || sym >= LC) ? 0u : big ? 0xffffffffu : (unsigned)total;
                s_lo[b][lane] = (unsigned)lo;
                s_hi[b][lane] = (unsigned)(lo + f);
                s_tot[b][lane] = tw;
                s_inv[b][lane] = 1.0 / (double)(tw ? tw : 1u);
            }
        }
        if (wave == 0 && c > 0) {
            // ---- coder: chunk c - 1, one symbol after the other ----
            const int b = (int)((c - 1) & 1);
            const long long left = ncoded - (c - 1) * PCE_CHUNK;
            const int cnt = left < PCE_CHUNK ? (int)left : PCE_CHUNK;
            const unsigned my_lo = s_lo[b][lane], my_hi = s_hi[b][lane], my_tot = s_tot[b][lane];
            const unsigned long long my_inv = (unsigned long long)__double_as_longlong(s_inv[b][lane]);
            for (int k = 0; k < cnt; ++k) {
                const unsigned cum_lo = pce_lane_u32(my_lo, k), cum_hi = pce_lane_u32(my_hi, k), total = pce_lane_u32(my_tot, k);
                const double inv = __longlong_as_double((long long)(((unsigned long long)pce_lane_u32((unsigned)(my_inv >> 32), k) << 32) |
                                                                    pce_lane_u32((unsigned)my_inv, k)));
                if (total - 1u >= PCE_MAX_TOTAL) { err = total ? 1 : 3; break; }
                const unsigned long long r = (unsigned long long)high - low + 1;
                const unsigned long long qh = pce_div(cum_hi * r, total, inv), ql = pce_div(cum_lo * r, total, inv);
                high = low + (unsigned)qh - 1u;                           // mod 2^32: the true values lie in [0, 2^32)
                low = low + (unsigned)ql;
                const unsigned x = low ^ high;
                const int n = x ? __builtin_clz(x) : 32;
                if (n) {
                    const unsigned long long top = (unsigned long long)low >> (32 - n);
                    if (pending == 0) {
                        pce_put(o, top, n, lane);
                    } else {
                        const int bit = (int)(low >> 31);
                        pce_put(o, (unsigned long long)bit, 1, lane);
                        pce_put_run(o, bit ^ 1, pending, lane);
                        pending = 0;
                        pce_put(o, top & ((1ull << (n - 1)) - 1), n - 1, lane);
                    }
                    low = (unsigned)((unsigned long long)low << n);
                    high = (unsigned)(((unsigned long long)high << n) | ((1ull << n) - 1));
                    if (o.ovf) break;
                }
                // now low = 0..., high = 1...; every further position with low = 1, high = 0 is an underflow bit
                const unsigned y = (low & ~high) << 1;
                const int m = __builtin_clz(~y);                           // bit 0 of y is 0: m <= 31
                if (m) {
                    pending += m;
                    low = (low << m) & 0x7fffffffu;
                    high = ((high << m) & 0x7fffffffu) | 0x80000000u | ((1u << m) - 1u);
                }
            }
            if ((err || o.ovf) && lane == 0) s_stop[c & 1] = 1;
        }
        __syncthreads();
        if (s_stop[c & 1]) break;                                         // uniform: read after the barrier by both waves
    }

    if (wave == 0) {
        if (!err) {
            pce_put(o, 1ull, 1, lane);                                    // finish(): a single 1 bit, pending bits are not flushed
            if (o.nres) pce_put(o, 0ull, 8 - o.nres, lane);               // BitOutputStream.close(): zero padding
        }
        if (lane == 0) {
            *nbytes_out = o.pos;
            *status_out = err ? err : o.ovf ? 2 : 0;
        }
    }
}

template <int LC>
__global__ __launch_bounds__(128) void pc_encode_kernel(const PcEncArgs a) {
    const int vol = blockIdx.x;
    pce_code_range<LC>(a.logits + (size_t)vol * a.count * LC, a.symbols + (size_t)vol * a.count, 1, a.count, a.resolution,
                       a.out + (size_t)vol * a.capacity, a.capacity, a.nbytes + vol, a.status + vol);     // symbol 0 is not coded
}

// ---- segments (container format 6): sub-ranges of a volume as independent coder runs, one work-group each ----------------------
// Work-group vol * nsegs + s codes symbols [max(1, ends[s - 1]), ends[s]) of volume vol into out[vol][s][0 .. capacity).  The tables
// are those of the whole volume (the logits are given), only the coder state starts afresh.  The ends travel in the kernel
// arguments; they are picked by a chain of selects over constant indices (an index computed at run time into a by-value array
// makes the compiler keep a private copy of it).
#define PCE_MAX_SEGS 16
struct PcEncSegArgs {
    PcEncArgs e;                  // out: (N, nsegs, capacity), nbytes / status: (N, nsegs)
    int nsegs;
    long long ends[PCE_MAX_SEGS]; // cumulative symbol counts, strictly increasing, ends[0] >= 1, ends[nsegs - 1] == count
};

template <int LC>
__global__ __launch_bounds__(128) void pc_encode_segments_kernel(const PcEncSegArgs a) {
    const int vol = (int)(blockIdx.x / (unsigned)a.nsegs), seg = (int)(blockIdx.x - (unsigned)vol * (unsigned)a.nsegs);
    long long first = 1, end = a.ends[0];
#pragma unroll
    for (int j = 1; j < PCE_MAX_SEGS; ++j)
        if (j == seg) { first = a.ends[j - 1]; end = a.ends[j]; }
    const size_t slot = (size_t)vol * a.nsegs + seg;
    pce_code_range<LC>(a.e.logits + (size_t)vol * a.e.count * LC, a.e.symbols + (size_t)vol * a.e.count, first, end, a.e.resolution,
                       a.e.out + slot * a.e.capacity, a.e.capacity, a.e.nbytes + slot, a.e.status + slot);
}

// ---- lane-parallel rANS tiles (container format 12): W interleaved coders, one stream, one wave per volume ---------------------
// ic_pc_encode_segments_f32 with nsegs = IC_PC_ENCODE_RANS(W).  The inputs are in round order (element r W + l is coder l's of round
// r); the wave runs the rounds from the last to the first and writes the stream from the end of the volume's capacity towards its
// start, so the decoder, which runs them forwards, finds the words in the order it takes them.  Lane l < W is coder l: pc_table_row
// (the ONE expression), pc_rans_row, then the step
//     if x >= g << 16 (64-bit: g may be 2^16): emit x & 0xffff, x >>= 16 -- at most once;   x = ((x / g) << 16) + x % g + cg.
// The words of a round go in front of what is written, the emitting lanes in ascending order: lane l stores at
// end - 2 popcount(emitting lanes >= l), found with one ballot; then the W states in front of all words.  `end` is wave-uniform and a
// round is stored only if it fits behind byte 0 of the volume's capacity -- as the states are -- so nothing is ever stored outside
// [0, capacity).  Every trip count is fixed by (count, W); only which lanes store one word depends on the data.
// A round with a bad symbol (status 3), else with a table whose total is too large (status 1), ends the run, as a round that does not
// fit does (status 2): a uniform break.  nbytes is 0 then.
struct PcEncRansArgs {
    PcEncArgs e;                  // logits (N, count, L), symbols (N, count) in round order; out (N, capacity), nbytes / status (N)
    int lanes;                    // W
};

template <int LC>
__global__ __launch_bounds__(64) void pc_encode_rans_kernel(const PcEncRansArgs a) {
    const int vol = blockIdx.x, lane = threadIdx.x, W = a.lanes;
    const long long count = a.e.count, cap = a.e.capacity, R = count / W;
    const float* __restrict__ logits = a.e.logits + (size_t)vol * count * LC;
    const long long* __restrict__ symbols = a.e.symbols + (size_t)vol * count;
    unsigned char* out = a.e.out + (size_t)vol * cap;
    unsigned x = PC_RANS_M;
    long long end = cap;                                                  // the stream so far is out[end .. cap); uniform
    int status = 0;
    for (long long r = R - 1; r >= 0; --r) {
        int bad = 0;
        bool emit = false;
        unsigned word = 0;
        if (lane < W) {
            const long long i = r * W + lane;
            const long long sym = symbols[i];
            if (sym != IC_PC_ENCODE_SKIP) {
                if (sym < 0 || sym >= LC) {
                    bad = 3;
                } else {
                    float l[LC];
#pragma unroll
                    for (int j = 0; j < LC; ++j) l[j] = logits[i * LC + j];
                    unsigned cum[LC];
                    if (!pc_rans_row<LC>(l, a.e.resolution, cum)) bad = 1;
                    unsigned cg = 0, nx = PC_RANS_M;
#pragma unroll
                    for (int j = 0; j < LC; ++j)
                        if (j == (int)sym) { cg = cum[j]; nx = j + 1 < LC ? cum[j + 1] : PC_RANS_M; }
                    const unsigned g = nx - cg;                           // 1 .. 2^16
                    if (!bad) {
                        if ((unsigned long long)x >= ((unsigned long long)g << 16)) { emit = true; word = x & 0xffffu; x >>= 16; }
                        x = ((x / g) << 16) + x % g + cg;
                    }
                }
            }
        }
        const unsigned long long bad3 = __ballot(bad == 3), bad1 = __ballot(bad == 1), emitting = __ballot(emit);
        if (bad3 | bad1) { status = bad3 ? 3 : 1; break; }
        const long long nb = 2ll * __popcll(emitting);
        if (nb > end) { status = 2; break; }                              // never a store in front of the volume's capacity
        if (emit) {
            unsigned char* p = out + end - 2ll * __popcll(emitting >> lane);
            p[0] = (unsigned char)word;
            p[1] = (unsigned char)(word >> 8);
        }
        end -= nb;
    }
    if (!status) {
        if (4ll * W > end) status = 2;
        else {
            end -= 4ll * W;
            if (lane < W) {
                unsigned char* p = out + end + 4 * lane;
                p[0] = (unsigned char)x; p[1] = (unsigned char)(x >> 8); p[2] = (unsigned char)(x >> 16); p[3] = (unsigned char)(x >> 24);
            }
        }
    }
    if (lane == 0) {
        a.e.nbytes[vol] = status ? 0 : cap - end;
        a.e.status[vol] = status;
    }
}

extern "C" size_t ic_pc_encode_capacity_bytes(long long count) {
    return count > 0 ? (size_t)(4 * count + 16) : 0;
}

extern "C" int ic_pc_encode_f32(const float* logits, const int64_t* symbols, int N, long long count, int L, float resolution,
                                uint8_t* bitstream, long long capacity, long long* nbytes, int* status, ic_stream_t stream) {
    IC_CHECK_ARG(logits && symbols && bitstream && nbytes && status);
    IC_CHECK_ARG(N > 0 && count > 0 && L > 0 && capacity >= 0 && resolution > 0.f);
    if (L > 16) return IC_ERR_UNSUPPORTED;
    PcEncArgs a{};
    a.logits = logits; a.symbols = (const long long*)symbols; a.out = bitstream; a.nbytes = nbytes; a.status = status;
    a.count = count; a.capacity = capacity; a.resolution = resolution;
    hipStream_t st = (hipStream_t)stream;
#define PCE_CASE(l) case l: hipLaunchKernelGGL(pc_encode_kernel<l>, dim3((unsigned)N), dim3(128), 0, st, a); break;
    switch (L) {
        PCE_CASE(1) PCE_CASE(2) PCE_CASE(3) PCE_CASE(4) PCE_CASE(5) PCE_CASE(6) PCE_CASE(7) PCE_CASE(8)
        PCE_CASE(9) PCE_CASE(10) PCE_CASE(11) PCE_CASE(12) PCE_CASE(13) PCE_CASE(14) PCE_CASE(15) PCE_CASE(16)
    }
#undef PCE_CASE
    IC_LAUNCH_CHECK();
    return IC_OK;
}

extern "C" int ic_pc_encode_segments_f32(const float* logits, const int64_t* symbols, int N, long long count, int L, float resolution,
                                         const long long* seg_ends_host, int nsegs, uint8_t* bitstream, long long capacity,
                                         long long* nbytes, int* status, ic_stream_t stream) {
    // everything is decided here, on the host, before the launch: a refused call writes nothing
    IC_CHECK_ARG(logits && symbols && bitstream && nbytes && status && seg_ends_host);
    if (nsegs < 0) {                                                      // IC_PC_ENCODE_RANS(W): the interleaved coder, one wave per volume
        const int W = -nsegs;
        IC_CHECK_ARG(W == 8 || W == 16 || W == 32 || W == 64);
        IC_CHECK_ARG(N > 0 && count > 0 && L > 0 && capacity >= 0 && resolution > 0.f);
        IC_CHECK_ARG(seg_ends_host[0] == count && count % W == 0);
        if (L > 16) return IC_ERR_UNSUPPORTED;
        PcEncRansArgs ra{};
        ra.e.logits = logits; ra.e.symbols = (const long long*)symbols; ra.e.out = bitstream; ra.e.nbytes = nbytes; ra.e.status = status;
        ra.e.count = count; ra.e.capacity = capacity; ra.e.resolution = resolution;
        ra.lanes = W;
        hipStream_t rst = (hipStream_t)stream;
#define PCE_CASE(l) case l: hipLaunchKernelGGL(pc_encode_rans_kernel<l>, dim3((unsigned)N), dim3(64), 0, rst, ra); break;
        switch (L) {
            PCE_CASE(1) PCE_CASE(2) PCE_CASE(3) PCE_CASE(4) PCE_CASE(5) PCE_CASE(6) PCE_CASE(7) PCE_CASE(8)
            PCE_CASE(9) PCE_CASE(10) PCE_CASE(11) PCE_CASE(12) PCE_CASE(13) PCE_CASE(14) PCE_CASE(15) PCE_CASE(16)
        }
#undef PCE_CASE
        IC_LAUNCH_CHECK();
        return IC_OK;
    }
    IC_CHECK_ARG(N > 0 && count > 0 && L > 0 && capacity >= 0 && resolution > 0.f && nsegs >= 1);
    if (L > 16 || nsegs > PCE_MAX_SEGS) return IC_ERR_UNSUPPORTED;
    IC_CHECK_ARG(seg_ends_host[0] >= 1 && seg_ends_host[nsegs - 1] == count);
    for (int s = 1; s < nsegs; ++s) IC_CHECK_ARG(seg_ends_host[s] > seg_ends_host[s - 1]);
    IC_CHECK_ARG((long long)N * nsegs <= 0x7fffffffLL);
    PcEncSegArgs a{};
    a.e.logits = logits; a.e.symbols = (const long long*)symbols; a.e.out = bitstream; a.e.nbytes = nbytes; a.e.status = status;
    a.e.count = count; a.e.capacity = capacity; a.e.resolution = resolution;
    a.nsegs = nsegs;
    for (int s = 0; s < PCE_MAX_SEGS; ++s) a.ends[s] = seg_ends_host[s < nsegs ? s : nsegs - 1];
    hipStream_t st = (hipStream_t)stream;
#define PCE_CASE(l) case l: hipLaunchKernelGGL(pc_encode_segments_kernel<l>, dim3((unsigned)(N * nsegs)), dim3(128), 0, st, a); break;
    switch (L) {
        PCE_CASE(1) PCE_CASE(2) PCE_CASE(3) PCE_CASE(4) PCE_CASE(5) PCE_CASE(6) PCE_CASE(7) PCE_CASE(8)
        PCE_CASE(9) PCE_CASE(10) PCE_CASE(11) PCE_CASE(12) PCE_CASE(13) PCE_CASE(14) PCE_CASE(15) PCE_CASE(16)
    }
#undef PCE_CASE
    IC_LAUNCH_CHECK();
    return IC_OK;
}
