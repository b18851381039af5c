// lr_spot.hip — CTC keyword spotting on gfx950: for every (clip, keyword) pair, where the keyword is spoken and how
// well.  A dynamic programme with a free start and a free end over the 2L-1 states of the keyword
// (tokens with the blanks BETWEEN them), scored in frame ratios d[t][c] = lp[t][c] - max_c lp[t][c]; the start frame
// rides along with the score, so there is no back-pointer table and no walk back.
//
// ONE launch per call.  A workgroup (four waves) belongs to one sample and serves four keyword slots of it, one a wave:
//
//   rows        the sample's n rows go into LDS once per workgroup (lr_stage_rows) and become ratios in
//               place (a wave per row: maximum, one subtraction per element) while n*C*4 bytes fit; else only m[t] lies in
//               LDS and a lane forms lp[t][cls] - m[t] as it prefetches.  Either way one fp32 subtraction per (t, c).
//   slots       a slot is four consecutive keywords and belongs to one wave.  The wave runs it in passes: the widest
//               keyword left decides the segment (16 lanes up to 8 tokens, 32 up to 16, 64 up to 32) and 64 / segment
//               keywords go side by side.  Sorted by length (spot.py does that) a slot takes one pass at 4, two at 2
//               or four at 1; in any other order the answers are the same and only the packing is worse.
//   chain       lane = (keyword q, state j).  Per step the two lower neighbours' (score, start) pairs come over DPP
//               wave shifts and are MASKED by j (j >= 1, j >= 2 and a skip allowed), so nothing crosses a segment
//               whatever its width; state 0 also weighs the fresh start (0, t).  Two or three compares and one fp32
//               add per cell: bit-equal to the NumPy restatement.  d[t][cls(j)] for the next 16 steps is fetched
//               while the current 16 are stepped through, so no memory latency sits in the chain.
//   end trace   the lane of the last state keeps its 16 (score, start) pairs of a block in registers and stores them
//               after the block: into LDS while 16 traces fit beside the rows, else into the workspace, or straight
//               into the caller's end_score / end_start when those are given.
//   hits        the same wave, per keyword: max_hits passes over the n candidates, lanes striding over t, the spans
//               already taken held one per lane and read with a uniform v_readlane; wave arg-max with the smallest t
//               on ties.  Lane h then stores hit h.  No atomics anywhere.
//
// Lanes past a keyword's last state are not masked: a state only reads states below it in its own segment.
#include <type_traits>

#include "lr_lattice_dev.h"

namespace {

constexpr int kMaxKw = LR_SPOT_MAX_KW_LEN;
constexpr int kMaxT = LR_SPOT_MAX_T;
constexpr int kMaxHits = LR_SPOT_MAX_HITS;
constexpr int kThreads = 256, kWaves = 4;
constexpr int kSlot = 4;                     // keywords per wave slot (= keywords side by side at 16-lane segments)
constexpr int kLen16 = 8, kLen32 = 16;       // the longest keyword of a 16- / 32-lane segment (2L-1 <= 15 / 31)

enum { TRACE_LDS = 0, TRACE_WORKSPACE = 1, TRACE_CALLER = 2 };

struct SpotPlan {
  int rows_in_lds, trace_in_lds, wgs_per_sample;
  unsigned off_trace;   // byte offset into the dynamic LDS (the rows, or m[t], lie at 0)
  size_t lds_bytes, ws_bytes;
};

__host__ __device__ inline int seg_of(int len) { return len <= kLen16 ? 16 : (len <= kLen32 ? 32 : 64); }

// LR_OK, LR_ERR_INVALID_ARG or LR_ERR_UNSUPPORTED — from the sizes alone
int spot_plan(int B, int T, int C, int K, int max_kw_len, int H, SpotPlan* p) {
  if (B <= 0 || T <= 0 || C < 2 || K <= 0 || max_kw_len <= 0 || H <= 0) return LR_ERR_INVALID_ARG;
  if (max_kw_len > kMaxKw || T > kMaxT || H > kMaxHits) return LR_ERR_UNSUPPORTED;
  const size_t rows = lr_align_up((size_t)T * C * 4, 16);
  const size_t trace = (size_t)kWaves * kSlot * T * 8;   // score and start of 16 keywords in flight
  p->rows_in_lds = rows <= LR_LDS_BUDGET;
  size_t off = p->rows_in_lds ? rows : lr_align_up((size_t)T * 4, 16);
  p->off_trace = (unsigned)off;
  // (only beside staged rows: one threshold in T, not two)
  p->trace_in_lds = p->rows_in_lds && off + trace <= LR_LDS_BUDGET;
  if (p->trace_in_lds) off += trace;
  p->lds_bytes = off;
  p->ws_bytes = p->trace_in_lds ? 16 : (size_t)B * K * T * 8;
  const long slots = (K + kSlot - 1) / kSlot;
  p->wgs_per_sample = (int)((slots + kWaves - 1) / kWaves);
  if ((long)B * p->wgs_per_sample > 0x7fffffffL) return LR_ERR_UNSUPPORTED;
  return LR_OK;
}

struct SpotArgs {
  const float* lp;
  const int32_t* sizes;
  const int32_t* kw;
  const int32_t* kw_lens;
  const float* min_scores;
  float* hit_score;
  int32_t* hit_start;
  int32_t* hit_end;
  int32_t* n_hits;
  int32_t* status;
  float* tr_score;     // [B][K][T] in the workspace or the caller's; NULL with the trace in LDS
  int32_t* tr_start;
  int64_t stride_b, stride_t;
  int T, C, K, kw_stride, blank, H;
  int pad_trace;       // the trace is the caller's: every (b, k, t) is written
  SpotPlan plan;
};

__device__ __forceinline__ int uniform(int x) { return __builtin_amdgcn_readfirstlane(x); }

// every output of a pair that is not spotted: padding, n_hits = 0, its status (one wave)
__device__ void write_empty(const SpotArgs& a, int b, int k, int st, int lane) {
  const int64_t pair = (int64_t)b * a.K + k;
  if (lane < a.H) {
    a.hit_score[pair * a.H + lane] = LR_NEG_INF;
    a.hit_start[pair * a.H + lane] = -1;
    a.hit_end[pair * a.H + lane] = -1;
  }
  if (lane == 0) {
    a.n_hits[pair] = 0;
    a.status[pair] = st;
  }
  if (a.pad_trace)
    for (int t = lane; t < a.T; t += LR_WAVE) {
      a.tr_score[pair * a.T + t] = LR_NEG_INF;
      a.tr_start[pair * a.T + t] = -1;
    }
}

template <bool ROWS_LDS>
__global__ __launch_bounds__(kThreads) void spot_kernel(const SpotArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const SpotPlan& P = a.plan;
  const int T = a.T, C = a.C, K = a.K, H = a.H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / P.wgs_per_sample, wg = blockIdx.x - b * P.wgs_per_sample;
  float* rows = reinterpret_cast<float*>(lds);   // ROWS_LDS: d[t][c]; else m[t]
  const int n = a.sizes ? a.sizes[b] : T;
  const bool n_ok = n >= 1 && n <= T;            // (uniform over the workgroup)
  const float* lpb = a.lp + (int64_t)b * a.stride_b;
  const int64_t stt = a.stride_t;

  if (n_ok) {
    if (ROWS_LDS) {
      lr_stage_rows(rows, lpb, n, C, stt, tid, kThreads);   // ---- the sample's n rows into LDS
      __syncthreads();
      // ---- ratios in place: a wave per row
      for (int t = wave; t < n; t += kWaves) {
        float* row = rows + t * C;
        float mx = LR_NEG_INF;
        for (int c = lane; c < C; c += LR_WAVE) mx = fmaxf(mx, row[c]);
        mx = lr_wave_max(mx);
        for (int c = lane; c < C; c += LR_WAVE) row[c] = row[c] - mx;
      }
    } else {
      // ---- m[t] only: a wave per row, four rows' loads in flight
      for (int t0 = wave * 4; t0 < n; t0 += kWaves * 4) {
        float mx[4] = {LR_NEG_INF, LR_NEG_INF, LR_NEG_INF, LR_NEG_INF};
        for (int c = lane; c < C; c += LR_WAVE) {
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int t = min(t0 + u, n - 1);
            mx[u] = fmaxf(mx[u], lpb[(int64_t)t * stt + c]);
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float m = lr_wave_max(mx[u]);
          if (lane == 0 && t0 + u < n) rows[t0 + u] = m;
        }
      }
    }
    __syncthreads();
  }

  // ---- from here on the waves go their own ways: no workgroup barrier below
  float* lds_score = reinterpret_cast<float*>(lds + P.off_trace) + (size_t)wave * kSlot * 2 * T;
  const int k_slot = (wg * kWaves + wave) * kSlot;
  if (k_slot < K) {
    const int n_slot = min(kSlot, K - k_slot);
    // the slot's lengths and which of them are usable (lane i < 4 holds keyword i's)
    int my_len = 1, my_ok = 0;
    if (lane < n_slot) {
      const int l = a.kw_lens[k_slot + lane];
      my_ok = l >= 1 && l <= a.kw_stride;
      my_len = my_ok ? l : 1;
    }
    if (!n_ok) {
      for (int i = 0; i < n_slot; ++i) write_empty(a, b, k_slot + i, LR_SPOT_BAD_LENGTH, lane);
      return;
    }
    int i0 = 0;
    while (i0 < n_slot) {   // ---- one pass: keywords i0 .. i0 + nk of the slot, side by side
      int widest = 1;
      for (int i = i0; i < n_slot; ++i) widest = max(widest, uniform(__builtin_amdgcn_readlane(my_len, i)));
      const int seg = seg_of(widest);
      const int nk = min(LR_WAVE / seg, n_slot - i0);
      const int q = lane / seg, j = lane - q * seg;
      const bool mine = q < nk;
      const int qi = mine ? i0 + q : i0;          // (a lane past the pass's keywords shadows the first: never stored)
      const int k = k_slot + qi;
      const int L = __shfl(my_len, qi, LR_WAVE);
      const bool len_ok = __shfl(my_ok, qi, LR_WAVE) != 0;
      const int S = 2 * L - 1;
      // class of state j; bad ids, per keyword
      int cls = a.blank;
      bool skip = false, bad = false;
      if (len_ok && j < S && !(j & 1)) {
        const int32_t* y = a.kw + (int64_t)k * a.kw_stride;
        bad = !lr_label_ok(y[j >> 1], C, a.blank);
        if (!bad) lr_state_class(y, j >> 1, cls, skip);
      }
      const unsigned long long badmask = __ballot(bad && mine);
      const unsigned long long segmask = seg == 64 ? ~0ull : ((1ull << seg) - 1);
      const bool id_ok = ((badmask >> (q * seg)) & segmask) == 0;
      const bool live = mine && len_ok && id_ok;
      const bool tail = live && j == S - 1;       // the lane whose pair is the end trace
      if (!id_ok) {   // (its lanes step along harmlessly on the blank)
        cls = a.blank;
        skip = false;
      }
      float* trs;
      int32_t* trst;
      if (a.tr_score) {
        trs = a.tr_score + ((int64_t)b * K + k) * T;
        trst = a.tr_start + ((int64_t)b * K + k) * T;
      } else {
        trs = lds_score + (size_t)qi * 2 * T;
        trst = reinterpret_cast<int32_t*>(trs + T);
      }

      // ---- the chain
      auto load16 = [&](float* r, int blk) {
#pragma unroll
        for (int i = 0; i < LR_LATTICE_CHUNK; ++i) {
          int t = blk * LR_LATTICE_CHUNK + i;
          if (t >= n) t = n - 1;
          r[i] = ROWS_LDS ? rows[t * C + cls] : lpb[(int64_t)t * stt + cls] - rows[t];
        }
      };
      const int nblk = (n + LR_LATTICE_CHUNK - 1) / LR_LATTICE_CHUNK;
      float v = LR_NEG_INF;
      int st = -1;
      float cur[LR_LATTICE_CHUNK], nxt[LR_LATTICE_CHUNK];
      load16(cur, 0);
      // one block of 16 steps; FULL: all of them lie inside the clip (no per-step test, nothing to keep for the stores)
      auto block = [&](int blk, auto full) {
        constexpr bool FULL = decltype(full)::value;
        float ev[LR_LATTICE_CHUNK];
        int es[LR_LATTICE_CHUNK];
#pragma unroll
        for (int i = 0; i < LR_LATTICE_CHUNK; ++i) {
          const int t = blk * LR_LATTICE_CHUNK + i;
          if (FULL || t < n) {   // (uniform)
            const float a1r = lr_wave_up1(v), a2r = lr_wave_up1(a1r);
            const int s1r = lr_wave_up1(st), s2r = lr_wave_up1(s1r);
            const float a1 = j >= 1 ? a1r : LR_NEG_INF;
            const float a2 = skip ? a2r : LR_NEG_INF;
            float best = v;
            int bs = st;
            if (a1 > best) { best = a1; bs = s1r; }
            if (a2 > best) { best = a2; bs = s2r; }
            if (j == 0 && 0.f > best) { best = 0.f; bs = t; }
            v = best + cur[i];
            st = v == LR_NEG_INF ? -1 : bs;
          }
          ev[i] = v;
          es[i] = st;
        }
        if (tail) {
          const int left = FULL ? LR_LATTICE_CHUNK : n - blk * LR_LATTICE_CHUNK;
#pragma unroll
          for (int i = 0; i < LR_LATTICE_CHUNK; ++i) {
            if (FULL || i < left) {
              trs[blk * LR_LATTICE_CHUNK + i] = ev[i];
              trst[blk * LR_LATTICE_CHUNK + i] = es[i];
            }
          }
        }
      };
      for (int blk = 0; blk < nblk; ++blk) {
        load16(nxt, blk + 1 < nblk ? blk + 1 : blk);
        if ((blk + 1) * LR_LATTICE_CHUNK <= n)
          block(blk, std::true_type());
        else
          block(blk, std::false_type());
#pragma unroll
        for (int i = 0; i < LR_LATTICE_CHUNK; ++i) cur[i] = nxt[i];
      }
      // the tail lanes' stores before the other lanes' loads of them
      __threadfence_block();

      // ---- hits, keyword by keyword (everything below is uniform but the lane's own candidates)
      for (int g = 0; g < nk; ++g) {
        const int src = g * seg;                  // a lane of keyword g
        const int kg = k_slot + i0 + g;
        if (!uniform(__shfl((int)live, src, LR_WAVE))) {
          const bool lok = uniform(__shfl((int)len_ok, src, LR_WAVE)) != 0;
          write_empty(a, b, kg, lok ? LR_SPOT_BAD_ID : LR_SPOT_BAD_LENGTH, lane);
          continue;
        }
        const int64_t pair = (int64_t)b * K + kg;
        const float* gs;
        const int32_t* gst;
        if (a.tr_score) {
          gs = a.tr_score + pair * T;
          gst = a.tr_start + pair * T;
        } else {
          gs = lds_score + (size_t)(i0 + g) * 2 * T;
          gst = reinterpret_cast<const int32_t*>(gs + T);
        }
        const float thr = a.min_scores ? a.min_scores[kg] : LR_NEG_INF;
        float h_score = LR_NEG_INF;   // lane h: hit h
        int h_start = -1, h_end = -1;
        int nh = 0;
        for (; nh < H; ++nh) {
          float best = LR_NEG_INF;
          int bt = 0x7fffffff;
          for (int t = lane; t < n; t += LR_WAVE) {
            const float sc = gs[t];
            const int s0 = gst[t];
            bool ok = sc > LR_NEG_INF && sc >= thr;
            for (int u = 0; u < nh; ++u) {
              const int s1 = __builtin_amdgcn_readlane(h_start, u), e1 = __builtin_amdgcn_readlane(h_end, u);
              if (s0 < e1 && s1 < t + 1) ok = false;
            }
            if (ok && sc > best) {   // (t ascends: the first of equal scores stays)
              best = sc;
              bt = t;
            }
          }
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o, LR_WAVE);
            const int ot = __shfl_xor(bt, o, LR_WAVE);
            if (ob > best || (ob == best && ot < bt)) {
              best = ob;
              bt = ot;
            }
          }
          bt = uniform(bt);
          if (bt == 0x7fffffff) break;            // no candidate left
          const int s = gst[bt];
          if (lane == nh) {
            h_score = gs[bt];
            h_start = s;
            h_end = bt + 1;
          }
        }
        if (lane < H) {
          a.hit_score[pair * H + lane] = h_score;
          a.hit_start[pair * H + lane] = h_start;
          a.hit_end[pair * H + lane] = h_end;
        }
        if (lane == 0) {
          a.n_hits[pair] = nh;
          a.status[pair] = 0;
        }
        if (a.pad_trace)
          for (int t = n + lane; t < T; t += LR_WAVE) {
            a.tr_score[pair * T + t] = LR_NEG_INF;
            a.tr_start[pair * T + t] = -1;
          }
      }
      // the next pass overwrites the LDS traces this one read
      __threadfence_block();
      i0 += nk;
    }
  }
}

}  // namespace

extern "C" size_t lr_ctc_spot_workspace_bytes(int B, int T, int C, int K, int max_kw_len, int max_hits) {
  SpotPlan p;
  if (spot_plan(B, T, C, K, max_kw_len, max_hits, &p) != LR_OK) return 0;
  return p.ws_bytes;
}

extern "C" int lr_ctc_spot_plan(int B, int T, int C, int K, int max_kw_len, int max_hits, int32_t* plan) {
  LR_CHECK_ARG(plan);
  SpotPlan p;
  const int ok = spot_plan(B, T, C, K, max_kw_len, max_hits, &p);
  if (ok != LR_OK) return ok;
  const int seg = seg_of(max_kw_len);
  plan[0] = seg;
  plan[1] = kThreads;
  plan[2] = LR_WAVE / seg;
  plan[3] = kWaves;
  plan[4] = p.rows_in_lds;
  plan[5] = p.trace_in_lds ? TRACE_LDS : TRACE_WORKSPACE;
  plan[6] = (int32_t)p.lds_bytes;
  plan[7] = kWaves * kSlot;
  plan[8] = kLen16;
  plan[9] = kLen32;
  plan[10] = B * p.wgs_per_sample;
  return LR_OK;
}

extern "C" int lr_ctc_spot(const float* log_probs, int64_t stride_b, int64_t stride_t, const int32_t* sizes,
                           const int32_t* keywords, int kw_stride, const int32_t* kw_lens, const float* min_scores,
                           int blank, int max_hits, float* hit_score, int32_t* hit_start, int32_t* hit_end,
                           int32_t* n_hits, int32_t* status, float* end_score, int32_t* end_start, void* workspace,
                           size_t workspace_bytes, int B, int T, int C, int K, lr_stream_t stream) {
  LR_CHECK_ARG(log_probs && keywords && kw_lens && hit_score && hit_start && hit_end && n_hits && status);
  LR_CHECK_ARG(!end_score == !end_start);
  SpotPlan p;
  const int ok = spot_plan(B, T, C, K, kw_stride, max_hits, &p);
  if (ok != LR_OK) return ok;
  LR_CHECK_ARG(blank >= 0 && blank < C && stride_b >= 0 && stride_t >= 0);
  SpotArgs a;
  a.lp = log_probs; a.sizes = sizes; a.kw = keywords; a.kw_lens = kw_lens; a.min_scores = min_scores;
  a.hit_score = hit_score; a.hit_start = hit_start; a.hit_end = hit_end; a.n_hits = n_hits; a.status = status;
  a.stride_b = stride_b; a.stride_t = stride_t;
  a.T = T; a.C = C; a.K = K; a.kw_stride = kw_stride; a.blank = blank; a.H = max_hits;
  a.pad_trace = end_score != nullptr;
  if (end_score) {
    a.tr_score = end_score;
    a.tr_start = end_start;
    if (p.trace_in_lds) p.lds_bytes = p.off_trace;   // (no trace in LDS then)
  } else if (p.trace_in_lds) {
    a.tr_score = nullptr;
    a.tr_start = nullptr;
  } else {
    LR_CHECK_ARG(workspace);
    if (workspace_bytes < p.ws_bytes) return LR_ERR_WORKSPACE;
    a.tr_score = static_cast<float*>(workspace);
    a.tr_start = reinterpret_cast<int32_t*>(a.tr_score + (size_t)B * K * T);
  }
  a.plan = p;
  const dim3 grid((unsigned)(B * p.wgs_per_sample));
  if (p.rows_in_lds)
    LR_LAUNCH((spot_kernel<true>), grid, dim3(kThreads), (unsigned)p.lds_bytes, stream, a);
  else
    LR_LAUNCH((spot_kernel<false>), grid, dim3(kThreads), (unsigned)p.lds_bytes, stream, a);
  return lr_launch_status();
}
