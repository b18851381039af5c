// lr_segment.hip — CTC segmentation on gfx950 (include/lipreading_hip.h A6g): the Viterbi lattice of
// lr_align.hip for a WHOLE video — tens of thousands of frames against thousands of caption tokens, the path free to
// start and end anywhere — and from its best path the frames of every token and of every utterance (caption).
//
// The lattice (up to 65536 x 32769 cells) fits no workgroup, so it spans many workgroups and many launches:
//
//   prepare     one workgroup per sample: the sample's status from its lengths, ids and utterance ranges, and its end
//               record {value, t, s} = {-inf, -1, -1}; both live in the workspace, where the later launches read them.
//   forward     ONE LAUNCH PER CHUNK of kF frames, grid = (state tiles, B), a lattice state per lane.  A state only
//               depends on states below it, at most two per frame, and that is used twice.  BETWEEN workgroups: a
//               workgroup that OWNS kOwn states recomputes a halo of kHalo = 2 kF + 2 states below them from the value
//               row saved at the chunk's start (two rows per sample ping-pong in the workspace); after k steps the
//               lowest 2k halo states are stale, and the owned ones, and the state just below them, never read a stale
//               one.  BETWEEN the waves of a workgroup: a wave owns kWaveOwn lanes and recomputes kWaveHalo = 2 kE + 2
//               below them, so it runs kE steps on its own — the previous row's neighbours come from DPP wave shifts,
//               no LDS and no barrier — and only every kE steps the waves exchange: owned lanes write their value to
//               LDS, one LDS-only barrier, halo lanes read what the wave below computed.  The recomputation is the same
//               fp32 add and compares on the same inputs as in the wave or tile below, so it is bit-identical to it,
//               and every workgroup of a launch is independent: the order between chunks is the launch order of the
//               one stream, nothing polls.  A lane packs 16 steps of its own state into one dword, bp[t / 16][s],
//               coalesced; only owned states are stored, so nothing is read-modify-written.  The lane that owns state
//               2L keeps the sample's end record: the wave shift of step t + 1 hands it v[t][2L-1] beside its own
//               v[t][2L] (the + 2 of both halos keeps that neighbour exact through the last step before an exchange).
//   walk back   one wave per sample: per 16 steps one coalesced read of the 33 dwords the path can reach, the steps
//               themselves with uniform values (v_readlane), frame_token 16 frames per store; stops after code 3.
//   spans       token bounds one FRAME per thread (a token's frames are contiguous: its first and last frame each see
//               a different neighbour), token sums one token per thread in ascending t, utterance sums one utterance
//               per thread in token order.
//
// Every offset into the table is 64-bit: at the limits it is 538 MB per sample.  Dead lanes (s > 2L) are not masked: a
// state only reads states below it.  Lanes below state 0 are held at -inf.  Cell and table: lr_lattice_dev.h.
#include "lr_lattice_dev.h"

namespace {

constexpr int kF = 64;                                // frames per forward launch
constexpr int kThreads = 512;                         // lanes of a forward workgroup
constexpr int kWaves = kThreads / LR_WAVE;
constexpr int kE = 8;                                 // steps a wave runs between two exchanges
constexpr int kWaveHalo = 2 * kE + 2;                 // +2: see kHalo
constexpr int kWaveOwn = LR_WAVE - kWaveHalo;         // 46 lanes a wave owns
constexpr int kSpan = kWaves * kWaveOwn;              // 368 states a workgroup computes (besides the lowest wave's halo)
constexpr int kHalo = 2 * kF + 2;                     // +2: state 2L-1 stays exact through the chunk's last step when 2L is a tile's first state
constexpr int kOwn = kSpan - kHalo;                   // 238 states a workgroup owns
constexpr int kRecWords = 16;                         // per-sample record in the workspace (64 bytes)
constexpr int kFwdLds = 2 * kSpan * 4;                // the double-buffered exchange row
static_assert(kF % kE == 0 && LR_LATTICE_CHUNK % kE == 0 && kOwn > 0, "exchanges fall on step boundaries of a dword");

enum { REC_VALUE = 0, REC_T = 1, REC_S = 2, REC_STATUS = 3 };

struct SegPlan {
  int tiles, sst, nch, launches;
  size_t bp_words, row_words;   // per sample
};

// LR_OK, LR_ERR_INVALID_ARG or LR_ERR_UNSUPPORTED — from the sizes alone
int seg_plan(int B, int T, int C, int max_tokens, SegPlan* p) {
  if (B <= 0 || T <= 0 || C < 2 || max_tokens < 0) return LR_ERR_INVALID_ARG;
  if (max_tokens > LR_SEG_MAX_TOKENS || T > LR_SEG_MAX_T || B > LR_SEG_MAX_B) return LR_ERR_UNSUPPORTED;   // (B is grid.y)
  const int S = 2 * max_tokens + 1;
  p->tiles = (S + kOwn - 1) / kOwn;
  p->sst = p->tiles * kOwn;
  p->nch = (T + LR_LATTICE_CHUNK - 1) / LR_LATTICE_CHUNK;
  p->launches = (T + kF - 1) / kF;
  p->bp_words = (size_t)p->nch * p->sst;
  p->row_words = (size_t)2 * p->sst;
  return LR_OK;
}

// [bp: B * nch * sst dwords][rows: 2 * B * sst floats][records: B * 16 dwords]
size_t seg_ws_bytes(const SegPlan& p, int B) { return (size_t)B * ((p.bp_words + p.row_words) * 4 + kRecWords * 4); }

struct SegArgs {
  const float* lp;
  const int32_t* sizes;
  const int32_t* targets;
  const int32_t* target_lens;
  const int32_t* utt_first;
  const int32_t* utt_count;
  const int32_t* n_utts;
  int32_t* frame_token;
  int32_t* tok_start;
  int32_t* tok_end;
  float* tok_logp;
  int32_t* utt_start;
  int32_t* utt_end;
  int32_t* utt_frames;
  float* utt_logp;
  int32_t* utt_worst;
  int32_t* span;
  float* total;
  int32_t* status;
  uint32_t* bp;
  float* rows;
  int32_t* recs;
  int64_t stride_b, stride_t;
  int B, T, C, blank, flags, target_stride, utt_stride;
  int sst, nch;
};

// ---- prepare: status and end record of every sample ---------------------------------------------------------------
__global__ __launch_bounds__(256) void seg_prepare_kernel(const SegArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
  const int W = a.target_stride;
  const int n = a.sizes ? a.sizes[b] : a.T;
  const int L = a.target_lens[b];
  const int U = a.n_utts ? a.n_utts[b] : 0;
  int st = 0;
  if (n < 1 || n > a.T || L < 0 || L > W || U < 0 || U > a.utt_stride) {
    st = LR_SEG_BAD_LENGTH;
  } else {
    const int32_t* y = a.targets + (int64_t)b * W;
    int bad = 0;
    for (int i = tid; i < L; i += nthr) {
      bad |= !lr_label_ok(y[i], a.C, a.blank);
    }
    if (__syncthreads_or(bad)) {
      st = LR_SEG_BAD_ID;
    } else {
      bad = 0;
      for (int u = tid; u < U; u += nthr) {
        const int64_t f = a.utt_first[(int64_t)b * a.utt_stride + u], c = a.utt_count[(int64_t)b * a.utt_stride + u];
        bad |= f < 0 || c < 0 || f + c > L;
      }
      if (__syncthreads_or(bad)) st = LR_SEG_BAD_UTTERANCE;
    }
  }
  // (a token the path does not visit — NaN input only — keeps an empty span inside the sample)
  for (int i = tid; i < W; i += nthr) {
    a.tok_start[(int64_t)b * W + i] = 0;
    a.tok_end[(int64_t)b * W + i] = 0;
  }
  if (tid == 0) {
    int32_t* rec = a.recs + (int64_t)b * kRecWords;
    rec[REC_VALUE] = __float_as_int(LR_NEG_INF);
    rec[REC_T] = -1;
    rec[REC_S] = -1;
    rec[REC_STATUS] = st;
  }
}

// ---- forward: frames [chunk * kF, chunk * kF + kF) of every sample that has them -------------------------------------
__global__ __launch_bounds__(kThreads) void seg_forward_kernel(const SegArgs a, const int chunk) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  float* rows = reinterpret_cast<float*>(lds);
  const int tile = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  int32_t* rec = a.recs + (int64_t)b * kRecWords;
  if (rec[REC_STATUS] != 0) return;
  const int n = a.sizes ? a.sizes[b] : a.T;
  const int L = a.target_lens[b];
  const int t0 = chunk * kF;
  const int base = tile * kOwn;
  // a launch past the sample's frames leaves its row and its end record alone; a tile above 2L computes nothing that is read
  if (t0 >= n || base > 2 * L) return;
  const int steps = min(kF, n - t0);
  const int wave = tid >> 6, lane = tid & 63;
  const int pos = wave * kWaveOwn + lane - kWaveHalo;   // place in the workgroup's span; < 0 on the lowest wave's halo lanes
  const int s = base - kHalo + pos;
  const bool wave_owned = lane >= kWaveHalo;            // (a state below that also lives in the wave below, which owns it)
  const bool owned = wave_owned && pos >= kHalo;        // s in [base, base + kOwn)
  const int32_t* y = a.targets + (int64_t)b * a.target_stride;
  int cls = a.blank;
  bool skip = false;
  if (s >= 0 && (s & 1) && s <= 2 * L) lr_state_class(y, s >> 1, cls, skip);
  const bool fresh_state = s == 0 || s == 1;
  const bool free_start = a.flags & LR_SEG_FREE_START, free_end = a.flags & LR_SEG_FREE_END;
  const bool end_thread = wave_owned && s == 2 * L;   // (owned: 2L >= base, and < base + kOwn or a higher tile would hold it)
  const float* lpb = a.lp + (int64_t)b * a.stride_b;
  const int64_t stt = a.stride_t;
  const float* row_in = a.rows + ((int64_t)(chunk & 1) * a.B + b) * a.sst;
  float* row_out = a.rows + ((int64_t)((chunk + 1) & 1) * a.B + b) * a.sst;
  uint32_t* bp = a.bp + (int64_t)b * a.nch * a.sst;

  float v = (chunk == 0 || s < 0) ? LR_NEG_INF : row_in[s];
  float ev = LR_NEG_INF;
  int et = -1, es = -1;
  if (end_thread) {
    ev = __int_as_float(rec[REC_VALUE]);
    et = rec[REC_T];
    es = rec[REC_S];
  }
  // the end candidates of frame tt, v[tt][2L-1] then v[tt][2L] (L == 0: v[tt][0] alone)
  auto end_candidates = [&](int tt, float below, float own) {
    if (free_end || tt == n - 1) {
      if (L > 0 && below > ev) { ev = below; et = tt; es = 2 * L - 1; }
      if (own > ev) { ev = own; et = tt; es = 2 * L; }
    }
  };
  auto load16 = [&](float* r, int g) {
#pragma unroll
    for (int j = 0; j < LR_LATTICE_CHUNK; ++j) {
      int t = t0 + g * LR_LATTICE_CHUNK + j;
      if (t >= n) t = n - 1;
      r[j] = lpb[(int64_t)t * stt + cls];
    }
  };
  const int groups = (steps + LR_LATTICE_CHUNK - 1) / LR_LATTICE_CHUNK;
  float cur[LR_LATTICE_CHUNK], nxt[LR_LATTICE_CHUNK];
  load16(cur, 0);
  for (int g = 0; g < groups; ++g) {
    load16(nxt, g + 1 < groups ? g + 1 : g);
    uint32_t word = 0;
#pragma unroll
    for (int j = 0; j < LR_LATTICE_CHUNK; ++j) {
      const int i = g * LR_LATTICE_CHUNK + j;   // step of this launch
      if (i < steps) {                // (uniform)
        const int t = t0 + i;
        if (i > 0 && i % kE == 0) {   // exchange: halo lanes take over what the wave below computed
          float* row = rows + ((i / kE) & 1) * kSpan;
          if (wave_owned) row[pos] = v;
          lr_lds_barrier();
          if (!wave_owned && pos >= 0) v = row[pos];
        }
        float a1 = lr_wave_up1(v), a2 = lr_wave_up1(a1);
        if (end_thread && i > 0) end_candidates(t - 1, a1, v);
        if (!skip) a2 = LR_NEG_INF;
        float best = v;
        uint32_t code = lr_viterbi_cell(best, a1, a2);
        if (fresh_state && (t == 0 || free_start) && 0.f > best) { best = 0.f; code = 3; }
        v = s < 0 ? LR_NEG_INF : best + cur[j];
        word = lr_bp_pack(word, code, j);
      }
    }
    if (owned) bp[(int64_t)(t0 / LR_LATTICE_CHUNK + g) * a.sst + s] = word;
#pragma unroll
    for (int j = 0; j < LR_LATTICE_CHUNK; ++j) cur[j] = nxt[j];
  }
  // ---- the last frame's end candidates need one more shift; the row goes out for the next chunk
  {
    const float below = lr_wave_up1(v);
    if (end_thread) {
      end_candidates(t0 + steps - 1, below, v);
      rec[REC_VALUE] = __float_as_int(ev);
      rec[REC_T] = et;
      rec[REC_S] = es;
    }
  }
  if (owned) row_out[s] = v;
}

// ---- walk back: one wave per sample -------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void seg_walk_kernel(const SegArgs a) {
  const int b = blockIdx.x, lane = threadIdx.x, T = a.T;
  const int32_t* rec = a.recs + (int64_t)b * kRecWords;
  int32_t* ftb = a.frame_token + (int64_t)b * T;
  int st = rec[REC_STATUS];
  const float total = __int_as_float(rec[REC_VALUE]);
  if (st == 0 && total == LR_NEG_INF) st = LR_SEG_INFEASIBLE;
  if (st != 0) {
    for (int t = lane; t < T; t += 64) ftb[t] = -1;
    if (lane == 0) {
      a.status[b] = st;
      a.total[b] = LR_NEG_INF;
      a.span[2 * b] = -1;
      a.span[2 * b + 1] = -1;
    }
    return;
  }
  const int t_end = __builtin_amdgcn_readfirstlane(rec[REC_T]);
  int s = __builtin_amdgcn_readfirstlane(rec[REC_S]);
  const uint32_t* bp = a.bp + (int64_t)b * a.nch * a.sst;
  for (int t = t_end + 1 + lane; t < T; t += 64) ftb[t] = -1;
  int t_first = 0;
  bool done = false;
  int k = t_end / LR_LATTICE_CHUNK;
  for (; k >= 0 && !done; --k) {
    const int s_top = s;
    const uint32_t w = lr_bp_fetch(bp, (int64_t)k * a.sst, s_top, lane);
    const int jhi = min(LR_LATTICE_CHUNK - 1, t_end - k * LR_LATTICE_CHUNK);
    int ft = -1;
#pragma unroll
    for (int j = LR_LATTICE_CHUNK - 1; j >= 0; --j) {
      if (j > jhi || done) continue;   // (uniform)
      const int t = k * LR_LATTICE_CHUNK + j;
      if (lane == j) ft = (s & 1) ? (s >> 1) : -1;
      const int code = lr_bp_code(w, s_top, s, j);
      if (code == 3 || t == 0) {
        done = true;
        t_first = t;
      } else {
        s -= code;
      }
    }
    if (lane <= jhi) ftb[k * LR_LATTICE_CHUNK + lane] = ft;
  }
  // (k + 1 is the chunk the walk stopped in; its frames before the path were stored as -1 above)
  for (int t = lane; t < (k + 1) * LR_LATTICE_CHUNK; t += 64) ftb[t] = -1;
  if (lane == 0) {
    a.status[b] = 0;
    a.total[b] = total;
    a.span[2 * b] = t_first;
    a.span[2 * b + 1] = t_end + 1;
  }
}

// ---- spans ---------------------------------------------------------------------------------------------------------------
// a frame per thread: the first and the last frame of a token's run
__global__ __launch_bounds__(256) void seg_bounds_kernel(const SegArgs a) {
  const int b = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x, T = a.T;
  if (t >= T || a.status[b] != 0) return;
  const int32_t* ftb = a.frame_token + (int64_t)b * T;
  const int i = ftb[t];
  if (i < 0) return;
  const int prev = t > 0 ? ftb[t - 1] : -1, next = t + 1 < T ? ftb[t + 1] : -1;
  if (prev != i) a.tok_start[(int64_t)b * a.target_stride + i] = t;
  if (next != i) a.tok_end[(int64_t)b * a.target_stride + i] = t + 1;
}

// a token per thread: its log-probabilities summed in ascending t
__global__ __launch_bounds__(256) void seg_tokens_kernel(const SegArgs a) {
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x, W = a.target_stride;
  if (i >= W) return;
  const int64_t o = (int64_t)b * W + i;
  int t0 = -1, t1 = -1;
  float sum = 0.f;
  if (a.status[b] == 0 && i < a.target_lens[b]) {
    t0 = a.tok_start[o];
    t1 = a.tok_end[o];
    const float* col = a.lp + (int64_t)b * a.stride_b + a.targets[o];
    for (int t = t0; t < t1; ++t) sum += col[(int64_t)t * a.stride_t];
  }
  a.tok_start[o] = t0;
  a.tok_end[o] = t1;
  a.tok_logp[o] = sum;
}

// an utterance per thread, sequential over its tokens: the order of the sums is part of the specification
__global__ __launch_bounds__(256) void seg_utts_kernel(const SegArgs a) {
  const int b = blockIdx.y, u = blockIdx.x * 256 + threadIdx.x, US = a.utt_stride, W = a.target_stride;
  if (u >= US) return;
  const int64_t o = (int64_t)b * US + u;
  int t0 = -1, t1 = -1, frames = 0, worst = -1;
  float sum = 0.f;
  if (a.status[b] == 0 && u < a.n_utts[b] && a.utt_count[o] > 0) {
    const int f = a.utt_first[o], c = a.utt_count[o];
    const int32_t* ts = a.tok_start + (int64_t)b * W;
    const int32_t* te = a.tok_end + (int64_t)b * W;
    const float* tl = a.tok_logp + (int64_t)b * W;
    t0 = ts[f];
    t1 = te[f + c - 1];
    worst = f;
    float low = tl[f];
    for (int i = f; i < f + c; ++i) {
      frames += te[i] - ts[i];
      const float p = tl[i];
      sum += p;
      if (p < low) { low = p; worst = i; }
    }
  }
  a.utt_start[o] = t0;
  a.utt_end[o] = t1;
  a.utt_frames[o] = frames;
  a.utt_logp[o] = sum;
  a.utt_worst[o] = worst;
}

}  // namespace

extern "C" size_t lr_ctc_segment_workspace_bytes(int B, int T, int C, int max_tokens) {
  SegPlan p;
  if (seg_plan(B, T, C, max_tokens, &p) != LR_OK) return 0;
  return seg_ws_bytes(p, B);
}

extern "C" int lr_ctc_segment_plan(int B, int T, int C, int max_tokens, int32_t* plan) {
  LR_CHECK_ARG(plan);
  SegPlan p;
  const int ok = seg_plan(B, T, C, max_tokens, &p);
  if (ok != LR_OK) return ok;
  plan[0] = kOwn;
  plan[1] = kF;
  plan[2] = p.launches;
  plan[3] = p.tiles * B;
  plan[4] = kThreads;
  plan[5] = kFwdLds;
  return LR_OK;
}

// ev: NULL, or four events recorded before the forward launches, after them, after the walk back and after the spans
static int segment_impl(const float* log_probs, int64_t stride_b, int64_t stride_t, const int32_t* sizes,
                        const int32_t* targets, int target_stride, const int32_t* target_lens, const int32_t* utt_first,
                        const int32_t* utt_count, int utt_stride, const int32_t* n_utts, int blank, int flags,
                        int32_t* frame_token, int32_t* tok_start, int32_t* tok_end, float* tok_logp, int32_t* utt_start,
                        int32_t* utt_end, int32_t* utt_frames, float* utt_logp, int32_t* utt_worst, int32_t* span,
                        float* total, int32_t* status, void* workspace, size_t workspace_bytes, int B, int T, int C,
                        int max_tokens, lr_stream_t stream, hipEvent_t* ev) {
  LR_CHECK_ARG(log_probs && targets && target_lens && frame_token && tok_start && tok_end && tok_logp && span && total &&
               status && workspace);
  LR_CHECK_ARG(!n_utts || (utt_first && utt_count && utt_start && utt_end && utt_frames && utt_logp && utt_worst));
  SegPlan p;
  const int ok = seg_plan(B, T, C, max_tokens, &p);
  if (ok != LR_OK) return ok;
  LR_CHECK_ARG(blank >= 0 && blank < C && target_stride >= 0 && target_stride <= max_tokens && utt_stride >= 0);
  LR_CHECK_ARG(stride_b >= 0 && stride_t >= 0 && (flags & ~(LR_SEG_FREE_START | LR_SEG_FREE_END)) == 0);
  if (workspace_bytes < seg_ws_bytes(p, B)) return LR_ERR_WORKSPACE;
  SegArgs a;
  a.lp = log_probs; a.sizes = sizes; a.targets = targets; a.target_lens = target_lens;
  a.utt_first = utt_first; a.utt_count = utt_count; a.n_utts = n_utts;
  a.frame_token = frame_token; a.tok_start = tok_start; a.tok_end = tok_end; a.tok_logp = tok_logp;
  a.utt_start = utt_start; a.utt_end = utt_end; a.utt_frames = utt_frames; a.utt_logp = utt_logp; a.utt_worst = utt_worst;
  a.span = span; a.total = total; a.status = status;
  a.bp = static_cast<uint32_t*>(workspace);
  a.rows = reinterpret_cast<float*>(a.bp + (size_t)B * p.bp_words);
  a.recs = reinterpret_cast<int32_t*>(a.rows + (size_t)B * p.row_words);
  a.stride_b = stride_b; a.stride_t = stride_t;
  a.B = B; a.T = T; a.C = C; a.blank = blank; a.flags = flags; a.target_stride = target_stride;
  a.utt_stride = n_utts ? utt_stride : 0;
  a.sst = p.sst; a.nch = p.nch;
  hipStream_t hs = (hipStream_t)stream;
  LR_LAUNCH(seg_prepare_kernel, dim3(B), dim3(256), 0, stream, a);
  int st = lr_launch_status();
  if (ev) (void)hipEventRecord(ev[0], hs);
  for (int chunk = 0; chunk < p.launches && st == LR_OK; ++chunk) {
    LR_LAUNCH(seg_forward_kernel, dim3(p.tiles, B), dim3(kThreads), kFwdLds, stream, a, chunk);
    st = lr_launch_status();
  }
  if (st != LR_OK) return st;
  if (ev) (void)hipEventRecord(ev[1], hs);
  LR_LAUNCH(seg_walk_kernel, dim3(B), dim3(64), 0, stream, a);
  if ((st = lr_launch_status()) != LR_OK) return st;
  if (ev) (void)hipEventRecord(ev[2], hs);
  LR_LAUNCH(seg_bounds_kernel, dim3((T + 255) / 256, B), dim3(256), 0, stream, a);
  if ((st = lr_launch_status()) != LR_OK) return st;
  if (target_stride > 0) {
    LR_LAUNCH(seg_tokens_kernel, dim3((target_stride + 255) / 256, B), dim3(256), 0, stream, a);
    if ((st = lr_launch_status()) != LR_OK) return st;
  }
  if (a.utt_stride > 0) {
    LR_LAUNCH(seg_utts_kernel, dim3((a.utt_stride + 255) / 256, B), dim3(256), 0, stream, a);
    st = lr_launch_status();
  }
  if (ev) (void)hipEventRecord(ev[3], hs);
  return st;
}

extern "C" int lr_ctc_segment(const float* log_probs, int64_t stride_b, int64_t stride_t, const int32_t* sizes,
                              const int32_t* targets, int target_stride, const int32_t* target_lens,
                              const int32_t* utt_first, const int32_t* utt_count, int utt_stride, const int32_t* n_utts,
                              int blank, int flags, int32_t* frame_token, int32_t* tok_start, int32_t* tok_end,
                              float* tok_logp, int32_t* utt_start, int32_t* utt_end, int32_t* utt_frames, float* utt_logp,
                              int32_t* utt_worst, int32_t* span, float* total, int32_t* status, void* workspace,
                              size_t workspace_bytes, int B, int T, int C, int max_tokens, lr_stream_t stream) {
  return segment_impl(log_probs, stride_b, stride_t, sizes, targets, target_stride, target_lens, utt_first, utt_count,
                      utt_stride, n_utts, blank, flags, frame_token, tok_start, tok_end, tok_logp, utt_start, utt_end,
                      utt_frames, utt_logp, utt_worst, span, total, status, workspace, workspace_bytes, B, T, C, max_tokens,
                      stream, nullptr);
}

extern "C" int lr_ctc_segment_phases(const float* log_probs, int64_t stride_b, int64_t stride_t, const int32_t* sizes,
                                     const int32_t* targets, int target_stride, const int32_t* target_lens,
                                     const int32_t* utt_first, const int32_t* utt_count, int utt_stride,
                                     const int32_t* n_utts, int blank, int flags, int32_t* frame_token, int32_t* tok_start,
                                     int32_t* tok_end, float* tok_logp, int32_t* utt_start, int32_t* utt_end,
                                     int32_t* utt_frames, float* utt_logp, int32_t* utt_worst, int32_t* span, float* total,
                                     int32_t* status, void* workspace, size_t workspace_bytes, int B, int T, int C,
                                     int max_tokens, float* phase_ms, lr_stream_t stream) {
  LR_CHECK_ARG(phase_ms);
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  int st = LR_OK;
  for (int i = 0; i < 4 && st == LR_OK; ++i)
    if (hipEventCreate(&ev[i]) != hipSuccess) st = LR_ERR_LAUNCH;
  if (st == LR_OK)
    st = segment_impl(log_probs, stride_b, stride_t, sizes, targets, target_stride, target_lens, utt_first, utt_count,
                      utt_stride, n_utts, blank, flags, frame_token, tok_start, tok_end, tok_logp, utt_start, utt_end,
                      utt_frames, utt_logp, utt_worst, span, total, status, workspace, workspace_bytes, B, T, C, max_tokens,
                      stream, ev);
  if (st == LR_OK && hipEventSynchronize(ev[3]) != hipSuccess) st = LR_ERR_LAUNCH;
  for (int i = 0; i < 3 && st == LR_OK; ++i)
    if (hipEventElapsedTime(&phase_ms[i], ev[i], ev[i + 1]) != hipSuccess) st = LR_ERR_LAUNCH;
  for (int i = 0; i < 4; ++i)
    if (ev[i]) (void)hipEventDestroy(ev[i]);
  return st;
}
