// What the sequential decoder (pc_decode.hip) takes from the context model (probclass.hip): not ABI.
#pragma once
#include "common.h"

typedef float pc_f32x16 __attribute__((ext_vector_type(16)));
typedef float pc_f32x4 __attribute__((ext_vector_type(4)));

#define PC_NT 14          // live taps of the "other" mask, order (kd,kh,kw)
#define PC_NP 4           // partial sums per output (see pc_mfma_kernel)
__device__ __forceinline__ constexpr int pc_tap_kd(int t) { return t < 9 ? 0 : 1; }
__device__ __forceinline__ constexpr int pc_tap_kh(int t) { return t < 9 ? t / 3 : (t < 12 ? 0 : 1); }
__device__ __forceinline__ constexpr int pc_tap_kw(int t) { return t < 9 ? t % 3 : (t < 12 ? t - 9 : t - 12); }

// matrix-core filter packings (k = 24 or 64, L <= 16): floats of one k -> cout layer; all three layers of a network in one launch
size_t pc_packed_floats(int k, int cout);
bool pc_mfma_supported(int k, int L);
int pc_pack_filters(const float* const* wt, int k, int L, float* packed, hipStream_t st);

// the four layers over (N, C, h, w); workspace as ic_pc_workspace_bytes.  prepacked: the packings already sit at its end
int pc_forward(const float* q, int prepadded, const int64_t* symbols, const float* const* wt, int k, int L,
               float pad_value, float* logits, float* bits, int N, int C, int h, int w,
               void* workspace, size_t workspace_bytes, hipStream_t st, bool prepacked = false);
