// lr_align.hip — CTC forced alignment (Viterbi over the 2L+1-state lattice of lr_ctc.hip) on gfx950: per-frame
// token, per-token and per-word frame spans and log-probabilities for a KNOWN transcript.
//
// One launch per batch, one sample per workgroup, a lattice state per thread.
//
//   forward     v[t][s] = max(v[t-1][s], v[t-1][s-1], v[t-1][s-2] if allowed) + lp[t][cls(s)], first maximum wins
//               in that order (the back-pointer code 0 / 1 / 2): two or three compares and one fp32 add per cell, no
//               transcendental, so the result is bit-equal to a NumPy fp32 restatement.  Two shapes, as lr_ctc.hip:
//               ONE WAVE when 2L+1 <= 64 — the previous row's neighbours come from DPP wave shifts, no barrier
//               per step (with the rows in LDS the launch has four waves; the other three only help staging) — and
//               MULTI-WAVE up to 513 states with a double-buffered LDS row and one LDS-only barrier per step.
//               What costs time is the chain of n dependent steps; lp[t][cls(s)] does not depend on it, so a thread
//               reads its next 16 values (from the LDS image of the sample's rows when that fits, from global
//               memory otherwise) while it steps through the current 16.
//   table       2 bits per cell: a thread packs 16 consecutive steps of its own state into one dword and stores
//               bp[t / 16][s], coalesced across the wave; nothing is read-modify-written.  The table lies in LDS
//               while it fits beside the rest, else in the caller's workspace — one code path, a generic pointer.
//   walk back   wave 0, uniformly: per 16 steps ONE coalesced read of the 33 dwords the path can reach from where it
//               stands (it descends at most two states a step), then the steps themselves on the scalar unit
//               (v_readlane with a uniform lane, shifts); frame_token goes out 16 frames per store.
//   spans       token sums in ascending t, one token per thread; word grouping by one lane over the L role flags
//               staged in LDS, word sums one word per thread.  No atomics, no scratch beyond the workspace.
//
// Dead lanes (s > 2L) are not masked: a state only ever reads states below it, so what they compute is never used.
// The staging, the cell and the table's conventions are lr_lattice_dev.h's, shared with lr_spot.hip and lr_segment.hip.
#include "lr_lattice_dev.h"

namespace {

constexpr int kMaxL = 256;                   // as lr_ctc_nll
constexpr int kMaxT = LR_ALIGN_MAX_T;
constexpr int kStageThreads = 256;           // workgroup of the one-wave kernel

struct AlignPlan {
  int one_wave, sst, threads, lcap, nch;
  int lat_in_lds, bp_in_lds;
  unsigned off_rows, off_lat, off_bp;   // byte offsets into the dynamic LDS
  size_t lds_bytes, bp_bytes;           // bp_bytes: per sample
};

// LR_OK, LR_ERR_INVALID_ARG or LR_ERR_UNSUPPORTED — from the sizes alone
int align_plan(int B, int T, int C, int max_label_len, AlignPlan* p) {
  if (B <= 0 || T <= 0 || C < 2 || max_label_len < 0) return LR_ERR_INVALID_ARG;
  if (max_label_len > kMaxL || T > kMaxT) return LR_ERR_UNSUPPORTED;
  const int S = 2 * max_label_len + 1;
  p->one_wave = S <= LR_WAVE;
  p->sst = (S + LR_WAVE - 1) / LR_WAVE * LR_WAVE;
  p->lcap = max_label_len < 4 ? 4 : (max_label_len + 3) & ~3;
  p->nch = (T + LR_LATTICE_CHUNK - 1) / LR_LATTICE_CHUNK;
  // lab | role | tok_start | tok_end | tok_logp | word_first | word_count : lcap dwords each
  size_t off = (size_t)7 * p->lcap * 4;
  p->off_rows = (unsigned)off;
  if (!p->one_wave) off += (size_t)2 * p->sst * 4;
  p->off_lat = (unsigned)off;
  const size_t lat = lr_align_up((size_t)T * C * 4, 16);
  p->lat_in_lds = off + lat <= LR_LDS_BUDGET;
  if (p->lat_in_lds) off += lat;
  p->off_bp = (unsigned)off;
  p->bp_bytes = (size_t)p->nch * p->sst * 4;
  p->bp_in_lds = off + p->bp_bytes <= LR_LDS_BUDGET;
  if (p->bp_in_lds) off += p->bp_bytes;
  p->lds_bytes = off;
  // (the one-wave kernel's other three waves only stage the rows: without rows in LDS there is nothing for them to do)
  p->threads = p->one_wave ? (p->lat_in_lds ? kStageThreads : LR_WAVE) : p->sst;
  return LR_OK;
}

size_t align_ws_bytes(const AlignPlan& p, int B) {
  // (never 0: 0 is the query's answer for rejected arguments)
  return p.bp_in_lds ? 16 : (size_t)B * p.bp_bytes;
}

struct AlignArgs {
  const float* lp;
  const int32_t* sizes;
  const int32_t* targets;
  const int32_t* target_lens;
  const int32_t* roles;
  int32_t* frame_token;
  int32_t* tok_start;
  int32_t* tok_end;
  float* tok_logp;
  int32_t* word_first;
  int32_t* word_count;
  int32_t* word_start;
  int32_t* word_end;
  float* word_logp;
  int32_t* n_words;
  float* total;
  int32_t* status;
  uint32_t* bp_ws;
  int64_t stride_b, stride_t;
  int T, C, blank, target_stride;
  AlignPlan plan;
};

// the end state: 2L only on a strict win of v[2L] (vb) over v[2L-1] (vc); L == 0 has state 0 alone
__device__ __forceinline__ int end_state(int L, float vb, float vc) { return L == 0 ? 0 : (vb > vc ? 2 * L : 2 * L - 1); }

// every per-sample output of a sample that is not aligned: -1 / 0 / total = -inf
__device__ void write_empty(const AlignArgs& a, int b, int st, int nthr) {
  const int tid = threadIdx.x, W = a.target_stride;
  for (int t = tid; t < a.T; t += nthr) a.frame_token[(int64_t)b * a.T + t] = -1;
  for (int i = tid; i < W; i += nthr) {
    const int64_t o = (int64_t)b * W + i;
    a.tok_start[o] = -1;
    a.tok_end[o] = -1;
    a.tok_logp[o] = 0.f;
    if (a.roles) {
      a.word_first[o] = -1;
      a.word_count[o] = -1;
      a.word_start[o] = -1;
      a.word_end[o] = -1;
      a.word_logp[o] = 0.f;
    }
  }
  if (tid == 0) {
    a.status[b] = st;
    a.total[b] = LR_NEG_INF;
    if (a.n_words) a.n_words[b] = 0;
  }
}

template <bool ONE_WAVE, bool LAT_LDS>
__global__ __launch_bounds__(ONE_WAVE ? kStageThreads : 576) void align_kernel(const AlignArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  __shared__ int s_flag;
  __shared__ float s_total;
  const AlignPlan& P = a.plan;
  const int lcap = P.lcap, sst = P.sst, C = a.C, T = a.T, W = a.target_stride;
  int* lab = reinterpret_cast<int*>(lds);
  int* role = lab + lcap;
  int* tst = role + lcap;
  int* ten = tst + lcap;
  float* tlp = reinterpret_cast<float*>(ten + lcap);
  int* wfirst = reinterpret_cast<int*>(tlp + lcap);
  int* wcount = wfirst + lcap;
  float* rows = reinterpret_cast<float*>(lds + P.off_rows);
  float* lat = reinterpret_cast<float*>(lds + P.off_lat);
  const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6;
  uint32_t* bp = P.bp_in_lds ? reinterpret_cast<uint32_t*>(lds + P.off_bp) : a.bp_ws + (size_t)b * P.nch * sst;

  // ---- the sample's own status (uniform over the workgroup); ids past the length are not read
  const int n = a.sizes ? a.sizes[b] : T;
  const int L = a.target_lens[b];
  const int32_t* y = a.targets + (int64_t)b * W;
  int st = 0;
  if (n < 1 || n > T || L < 0 || L > W) {
    st = LR_ALIGN_BAD_LENGTH;
  } else {
    int bad = 0;
    for (int i = tid; i < L; i += nthr) {
      const int c = y[i];
      const bool ok = lr_label_ok(c, C, a.blank);
      bad |= !ok;
      lab[i] = ok ? c : 0;
      role[i] = ok && a.roles ? a.roles[c] : 0;
      tst[i] = 0;   // (every token of an aligned sample gets its span in the walk back; NaN input must still stay in bounds)
      ten[i] = 0;
    }
    if (__syncthreads_or(bad)) st = LR_ALIGN_BAD_ID;
  }
  if (st != 0) {
    write_empty(a, b, st, nthr);
    return;
  }
  const float* lpb = a.lp + (int64_t)b * a.stride_b;
  const int64_t stt = a.stride_t;

  if (LAT_LDS) {   // ---- the sample's n rows into LDS
    lr_stage_rows(lat, lpb, n, C, stt, tid, nthr);
    __syncthreads();
  }

  // ---- forward: thread s owns state s
  const int S = 2 * L + 1;
  const int nch = (n + LR_LATTICE_CHUNK - 1) / LR_LATTICE_CHUNK;
  if (!ONE_WAVE || wave == 0) {
    const int s = ONE_WAVE ? lane : tid;
    int cls = a.blank;
    bool skip = false;
    if ((s & 1) && s < S) lr_state_class(lab, s >> 1, cls, skip);
    auto load16 = [&](float* r, int k) {
#pragma unroll
      for (int j = 0; j < LR_LATTICE_CHUNK; ++j) {
        int t = k * LR_LATTICE_CHUNK + j;
        if (t >= n) t = n - 1;
        r[j] = LAT_LDS ? lat[t * C + cls] : lpb[(int64_t)t * stt + cls];
      }
    };
    // a virtual row before the first: 0 on state 0, so that step 0 gives v[0][0] = lp[0][blank], v[0][1] = lp[0][y[0]]
    // and -inf elsewhere (0 + x is exact); its codes are never followed
    float v = s == 0 ? 0.f : LR_NEG_INF;
    float cur[LR_LATTICE_CHUNK], nxt[LR_LATTICE_CHUNK];
    load16(cur, 0);
    for (int k = 0; k < nch; ++k) {
      load16(nxt, k + 1 < nch ? k + 1 : k);
      uint32_t word = 0;
#pragma unroll
      for (int j = 0; j < LR_LATTICE_CHUNK; ++j) {
        const int t = k * LR_LATTICE_CHUNK + j;
        if (t < n) {   // (uniform)
          float a1, a2;
          if (ONE_WAVE) {
            a1 = lr_wave_up1(v);
            a2 = lr_wave_up1(a1);
          } else {
            float* row = rows + (t & 1) * sst;
            row[s] = v;
            lr_lds_barrier();
            a1 = s >= 1 ? row[s - 1] : LR_NEG_INF;
            a2 = s >= 2 ? row[s - 2] : LR_NEG_INF;
          }
          if (!skip) a2 = LR_NEG_INF;
          float best = v;
          const uint32_t code = lr_viterbi_cell(best, a1, a2);
          v = best + cur[j];
          word = lr_bp_pack(word, code, j);
        }
      }
      bp[k * sst + s] = word;
#pragma unroll
      for (int j = 0; j < LR_LATTICE_CHUNK; ++j) cur[j] = nxt[j];
    }
    // ---- end state and total
    if (ONE_WAVE) {
      const float vb = __shfl(v, 2 * L, 64), vc = __shfl(v, L ? 2 * L - 1 : 0, 64);
      if (lane == 0) {
        const int end = end_state(L, vb, vc);
        s_flag = end;
        s_total = end == 2 * L ? vb : vc;
      }
    } else {
      rows[(n & 1) * sst + s] = v;   // (the buffer the last step did not read)
    }
  }
  __syncthreads();
  if (!ONE_WAVE && tid == 0) {
    const float* row = rows + (n & 1) * sst;
    const float vb = row[2 * L], vc = row[L ? 2 * L - 1 : 0];
    const int end = end_state(L, vb, vc);
    s_flag = end;
    s_total = end == 2 * L ? vb : vc;
  }
  if (!ONE_WAVE) __syncthreads();
  const float total = s_total;
  if (total == LR_NEG_INF) {
    write_empty(a, b, LR_ALIGN_INFEASIBLE, nthr);
    return;
  }

  // ---- walk back (wave 0; s is uniform)
  if (wave == 0) {
    int s = __builtin_amdgcn_readfirstlane(s_flag);
    int s_next = -1;
    for (int k = nch - 1; k >= 0; --k) {
      const int s_top = s;
      const uint32_t w = lr_bp_fetch(bp, k * sst, s_top, lane);
      const int jhi = min(LR_LATTICE_CHUNK - 1, n - 1 - k * LR_LATTICE_CHUNK);
      int ft = -1;
#pragma unroll
      for (int j = LR_LATTICE_CHUNK - 1; j >= 0; --j) {
        if (j > jhi) continue;   // (uniform)
        const int t = k * LR_LATTICE_CHUNK + j;
        const int i = s >> 1;
        if (lane == j) ft = (s & 1) ? i : -1;
        if ((s & 1) && lane == 0) {
          tst[i] = t;
          if (s != s_next) ten[i] = t + 1;
        }
        const int code = lr_bp_code(w, s_top, s, j);
        s_next = s;
        if (t > 0) s -= code;
      }
      if (lane <= jhi) a.frame_token[(int64_t)b * T + k * LR_LATTICE_CHUNK + lane] = ft;
    }
  }
  for (int t = n + tid; t < T; t += nthr) a.frame_token[(int64_t)b * T + t] = -1;
  __syncthreads();

  // ---- tokens: the span's log-probabilities summed in ascending t
  for (int i = tid; i < W; i += nthr) {
    const int64_t o = (int64_t)b * W + i;
    int t0 = -1, t1 = -1;
    float sum = 0.f;
    if (i < L) {
      t0 = tst[i];
      t1 = ten[i];
      const int c = lab[i];
      for (int t = t0; t < t1; ++t) sum += LAT_LDS ? lat[t * C + c] : lpb[(int64_t)t * stt + c];
      tlp[i] = sum;
    }
    a.tok_start[o] = t0;
    a.tok_end[o] = t1;
    a.tok_logp[o] = sum;
  }
  if (tid == 0) {
    a.status[b] = 0;
    a.total[b] = total;
  }
  if (!a.roles) {
    if (tid == 0 && a.n_words) a.n_words[b] = 0;
    return;
  }

  // ---- words: maximal runs of role-1 tokens
  if (tid == 0) {
    int nw = 0;
    for (int i = 0; i < L; ++i) {
      if (role[i] != 1) continue;
      if (i == 0 || role[i - 1] != 1) {
        wfirst[nw] = i;
        wcount[nw] = 0;
        ++nw;
      }
      ++wcount[nw - 1];
    }
    s_flag = nw;
    a.n_words[b] = nw;
  }
  __syncthreads();
  const int nw = s_flag;
  for (int w = tid; w < W; w += nthr) {
    const int64_t o = (int64_t)b * W + w;
    int f = -1, c = -1, t0 = -1, t1 = -1;
    float sum = 0.f;
    if (w < nw) {
      f = wfirst[w];
      c = wcount[w];
      t0 = tst[f];
      t1 = ten[f + c - 1];
      for (int i = f; i < f + c; ++i) sum += tlp[i];
    }
    a.word_first[o] = f;
    a.word_count[o] = c;
    a.word_start[o] = t0;
    a.word_end[o] = t1;
    a.word_logp[o] = sum;
  }
}

}  // namespace

extern "C" size_t lr_ctc_align_workspace_bytes(int B, int T, int C, int max_label_len) {
  AlignPlan p;
  if (align_plan(B, T, C, max_label_len, &p) != LR_OK) return 0;
  return align_ws_bytes(p, B);
}

extern "C" int lr_ctc_align_plan(int B, int T, int C, int max_label_len, int32_t* plan) {
  LR_CHECK_ARG(plan);
  AlignPlan p;
  const int ok = align_plan(B, T, C, max_label_len, &p);
  if (ok != LR_OK) return ok;
  plan[0] = p.one_wave;
  plan[1] = p.threads;
  plan[2] = p.lat_in_lds;
  plan[3] = p.bp_in_lds;
  plan[4] = (int32_t)p.lds_bytes;
  return LR_OK;
}

extern "C" int lr_ctc_align(const float* log_probs, int64_t stride_b, int64_t stride_t, const int32_t* sizes,
                            const int32_t* targets, int target_stride, const int32_t* target_lens,
                            const int32_t* class_roles, int blank, int32_t* frame_token, int32_t* tok_start,
                            int32_t* tok_end, float* tok_logp, int32_t* word_first, int32_t* word_count,
                            int32_t* word_start, int32_t* word_end, float* word_logp, int32_t* n_words, float* total,
                            int32_t* status, void* workspace, size_t workspace_bytes, int B, int T, int C,
                            int max_label_len, lr_stream_t stream) {
  LR_CHECK_ARG(log_probs && targets && target_lens && frame_token && tok_start && tok_end && tok_logp && total &&
               status && workspace);
  LR_CHECK_ARG(!class_roles || (word_first && word_count && word_start && word_end && word_logp && n_words));
  AlignPlan p;
  const int ok = align_plan(B, T, C, max_label_len, &p);
  if (ok != LR_OK) return ok;
  LR_CHECK_ARG(blank >= 0 && blank < C && target_stride >= 0 && target_stride <= max_label_len);
  LR_CHECK_ARG(stride_b >= 0 && stride_t >= 0);
  if (workspace_bytes < align_ws_bytes(p, B)) return LR_ERR_WORKSPACE;
  AlignArgs a;
  a.lp = log_probs; a.sizes = sizes; a.targets = targets; a.target_lens = target_lens; a.roles = class_roles;
  a.frame_token = frame_token; a.tok_start = tok_start; a.tok_end = tok_end; a.tok_logp = tok_logp;
  a.word_first = word_first; a.word_count = word_count; a.word_start = word_start; a.word_end = word_end;
  a.word_logp = word_logp; a.n_words = n_words; a.total = total; a.status = status;
  a.bp_ws = static_cast<uint32_t*>(workspace);
  a.stride_b = stride_b; a.stride_t = stride_t;
  a.T = T; a.C = C; a.blank = blank; a.target_stride = target_stride;
  a.plan = p;
  const unsigned lds = (unsigned)p.lds_bytes;
  if (p.one_wave) {
    if (p.lat_in_lds)
      LR_LAUNCH((align_kernel<true, true>), dim3(B), dim3(p.threads), lds, stream, a);
    else
      LR_LAUNCH((align_kernel<true, false>), dim3(B), dim3(p.threads), lds, stream, a);
  } else {
    if (p.lat_in_lds)
      LR_LAUNCH((align_kernel<false, true>), dim3(B), dim3(p.threads), lds, stream, a);
    else
      LR_LAUNCH((align_kernel<false, false>), dim3(B), dim3(p.threads), lds, stream, a);
  }
  return lr_launch_status();
}
