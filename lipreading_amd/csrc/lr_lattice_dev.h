// lr_lattice_dev.h — the device idioms shared by the kernels that walk the CTC Viterbi lattice: lr_align.hip, lr_spot.hip
// and lr_segment.hip.  Internal: every includer gets its own copy (anonymous namespace).
// The spotter's cell stays in lr_spot.hip: it carries a start frame with the score and weighs a fresh start, no code.
#pragma once
#include "lr_common.h"

namespace {

constexpr int LR_LATTICE_CHUNK = 16;   // steps per prefetch block and per back-pointer dword (2 bits a step)

// the lane below's value (lane 0: -inf / -1) — DPP wave_shr:1, a few cycles where a ds_bpermute costs an LDS round trip
__device__ __forceinline__ float lr_wave_up1(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(LR_NEG_INF), __float_as_int(v), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ int lr_wave_up1(int v) { return __builtin_amdgcn_update_dpp(-1, v, 0x138, 0xf, 0xf, false); }

// n rows of C floats, stride_t apart, into LDS (the caller places its __syncthreads()): coalesced, ten loads of a thread
// in flight.  The loads are unconditional (clamped), since a load under a branch is waited for inside it; their values are
// only used under the `i < tot` of the stores, so hipcc would SINK each load into its store's branch after all — ten
// serialised round trips.  Two empty asm statements with the registers as operands keep five loads in front of each wait.
__device__ __forceinline__ void lr_stage_rows(float* lds_dst, const float* lpb, int n, int C, int64_t stride_t, int tid,
                                              int nthr) {
  const int tot = n * C;
  const bool dense = stride_t == C;
  for (int i0 = 0; i0 < tot; i0 += nthr * 10) {
    float r[10];
#pragma unroll
    for (int u = 0; u < 10; ++u) {
      int i = i0 + u * nthr + tid;
      if (i >= tot) i = tot - 1;
      int64_t at = i;
      if (!dense) {
        const int t = i / C;
        at = (int64_t)t * stride_t + (i - t * C);
      }
      r[u] = lpb[at];
    }
    asm volatile("" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]));
    asm volatile("" : "+v"(r[5]), "+v"(r[6]), "+v"(r[7]), "+v"(r[8]), "+v"(r[9]));
#pragma unroll
    for (int u = 0; u < 10; ++u) {
      const int i = i0 + u * nthr + tid;
      if (i < tot) lds_dst[i] = r[u];
    }
  }
}

// an id that may stand in a transcript or a keyword
__device__ __forceinline__ bool lr_label_ok(int c, int C, int blank) { return (unsigned)c < (unsigned)C && c != blank; }

// the state of token i of the label row y: its class, and whether the blank below it may be skipped
__device__ __forceinline__ void lr_state_class(const int32_t* y, int i, int& cls, bool& skip) {
  cls = y[i];
  skip = i >= 1 && y[i - 1] != cls;
}

// One Viterbi cell: v becomes the first maximum of v (stay), a1 (one state up), a2 (two; the caller masks it to -inf where
// the skip is not allowed) IN THAT ORDER — part of the specification, the tests compare bit for bit.  Returns the
// back-pointer code 0 / 1 / 2; the caller adds lp.
__device__ __forceinline__ uint32_t lr_viterbi_cell(float& v, float a1, float a2) {
  uint32_t code = 0;
  if (a1 > v) { v = a1; code = 1; }
  if (a2 > v) { v = a2; code = 2; }
  return code;
}

// ---- the back-pointer table: bp[chunk * sst + s] holds the codes of LR_LATTICE_CHUNK steps of state s, step j at bit 2j
__device__ __forceinline__ uint32_t lr_bp_pack(uint32_t word, uint32_t code, int j) { return word | code << (2 * j); }
// one coalesced read of the 33 dwords of the chunk at bp[row] that a path standing at s_top can reach (it descends at most
// two states a step): lane i gets state s_top - i's.  Off: int in the aligner, int64_t in the segmenter's 538 MB table.
template <typename Off>
__device__ __forceinline__ uint32_t lr_bp_fetch(const uint32_t* bp, Off row, int s_top, int lane) {
  const int idx = s_top - lane;
  return lane <= 2 * LR_LATTICE_CHUNK && idx >= 0 ? bp[row + idx] : 0u;
}
// step j's code of the (uniform) state s out of lr_bp_fetch's w: v_readlane with a uniform lane, on the scalar unit
__device__ __forceinline__ int lr_bp_code(uint32_t w, int s_top, int s, int j) {
  const uint32_t word = (uint32_t)__builtin_amdgcn_readlane((int)w, __builtin_amdgcn_readfirstlane(s_top - s));
  return (int)((word >> (2 * j)) & 3u);
}

}  // namespace
