// lr_edit.hip — batched Levenshtein scoring of decoded class ids against label ids.
//
// What the host path does per utterance in Python (decoder.py Decoder.cer / Decoder.wer on joined label strings)
// as one launch per batch: one pair per workgroup.
//
//   expansion   every class id spells a (possibly empty) string of SYMBOLS (indices into the scorer's sorted alphabet);
//               a sequence expands to the concatenation of its spellings.  Each thread takes a contiguous chunk of the
//               ids, counts the symbols it will write, a block prefix sum gives its offset, and it writes them into
//               LDS — with the spaces left out in the character unit.  In the word unit the expansion keeps the spaces,
//               and a second pass of the same shape (count word starts, prefix sum, write) records every word's
//               start, length and FNV-1a hash.  Nothing goes through global scratch.
//   DP          D[i][j] along anti-diagonals d = i + j: the cells of one diagonal are independent, three diagonals of
//               uint16 live in LDS, indexed by i.  One barrier per diagonal; the launch uses a single wavefront per pair
//               while the shorter side's capacity is <= 512 (the usual case: 75 frames against a caption), where that
//               barrier costs nothing, and four wavefronts above.  Two words are equal iff their hashes, lengths AND
//               characters are: the hash only spares the character loop.
//   alignment   (character unit) every inner cell keeps the step the walk back will take there, 2 bits, in LDS while
//               the whole table fits and in the caller's workspace otherwise (same code: a generic pointer).  Rows are
//               padded to 4 cells so that the cells of one diagonal never share a byte; bytes are updated by plain
//               read-modify-write, cells of one byte lying on different diagonals, i.e. either side of a barrier.
//               The walk back is one lane, at most n + m steps; its confusion-matrix updates are global atomics without
//               a return value — a few dozen per pair over a (K+1)^2 table, contention is not a concern at these counts.
//
// The kernel is latency-bound and tiny (a 75 x 75 pair is 149 dependent diagonals of <= 75 cells): there is no
// share-of-peak figure for it.  What it buys is that scoring is one launch and nothing returns to the host.
#include "lr_common.h"

namespace {

constexpr int kMaxDist = LR_EDIT_MAX_CHARS;         // expanded characters per side, distance modes
constexpr int kMaxAlign = LR_EDIT_MAX_ALIGN_CHARS;  // per side, alignment mode
constexpr int kOneWaveCap = 512;
constexpr int kOut = LR_EDIT_OUT_STRIDE;

struct EditPlan {
  int capH, capR;      // expanded characters a side can reach: width * longest spelling
  int capWH, capWR;    // words a side can reach (word unit)
  int nd;              // entries of one diagonal
  int threads;
  unsigned off_rc, off_words, off_diag, off_dirs;   // byte offsets into the dynamic LDS
  size_t lds_bytes;
  size_t dirs_bytes;   // per pair (alignment mode)
  int dirs_in_lds;
};

// LR_OK, LR_ERR_INVALID_ARG or LR_ERR_UNSUPPORTED — from the sizes alone, no device read
int edit_plan(int B, int hyp_width, int ref_width, int max_spelling, int mode, EditPlan* p) {
  if (B <= 0 || hyp_width <= 0 || ref_width <= 0 || max_spelling <= 0) return LR_ERR_INVALID_ARG;
  if (mode != LR_EDIT_CHARS && mode != LR_EDIT_WORDS && mode != LR_EDIT_CHARS_ALIGN) return LR_ERR_INVALID_ARG;
  const int64_t capH = (int64_t)hyp_width * max_spelling, capR = (int64_t)ref_width * max_spelling;
  const int64_t lim = mode == LR_EDIT_CHARS_ALIGN ? kMaxAlign : kMaxDist;
  if (capH > lim || capR > lim) return LR_ERR_UNSUPPORTED;
  p->capH = (int)capH;
  p->capR = (int)capR;
  p->capWH = (p->capH + 1) / 2;
  p->capWR = (p->capR + 1) / 2;
  p->threads = (capH < capR ? capH : capR) <= kOneWaveCap ? LR_WAVE : 4 * LR_WAVE;
  size_t off = lr_align_up((size_t)p->capH * 2, 4);
  p->off_rc = (unsigned)off;
  off += lr_align_up((size_t)p->capR * 2, 4);
  p->off_words = (unsigned)off;
  if (mode == LR_EDIT_WORDS) off += (size_t)(p->capWH + p->capWR) * 8;   // start u16, length u16, hash u32
  p->nd = (mode == LR_EDIT_WORDS ? p->capWH : p->capH) + 1;
  p->off_diag = (unsigned)off;
  off += lr_align_up((size_t)3 * p->nd * 2, 4);
  p->off_dirs = (unsigned)off;
  p->dirs_bytes = 0;
  p->dirs_in_lds = 0;
  if (mode == LR_EDIT_CHARS_ALIGN) {
    p->dirs_bytes = lr_align_up((size_t)p->capH * ((p->capR + 3) / 4), 4);
    if (off + p->dirs_bytes <= LR_LDS_BUDGET) {
      p->dirs_in_lds = 1;
      off += p->dirs_bytes;
    }
  }
  p->lds_bytes = off;
  return LR_OK;
}

size_t edit_ws_bytes(const EditPlan& p, int B) {
  // (never 0: 0 is the query's answer for rejected arguments)
  return p.dirs_bytes && !p.dirs_in_lds ? (size_t)B * p.dirs_bytes : 16;
}

struct EditArgs {
  const int32_t* hyp;
  const int32_t* hyp_lens;
  const int32_t* ref;
  const int32_t* ref_lens;
  const int32_t* spell_off;
  const int32_t* spell_sym;
  const int32_t* gate;
  int32_t* out;
  unsigned long long* totals;
  unsigned long long* conf;
  unsigned char* dirs_ws;
  int64_t hyp_stride, hyp_lens_stride, ref_stride, ref_lens_stride;
  int n_classes, space_sym, K, hyp_width, ref_width;
  EditPlan plan;
};

// exclusive prefix sum of one int per thread over the workgroup; *total = the sum.  tmp: NT / 64 ints of LDS
template <int NT>
__device__ __forceinline__ int block_scan(int v, int* tmp, int* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) tmp[w] = x;
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < NT / 64; ++k) {
    const int t = tmp[k];
    if (k < w) off += t;
    tot += t;
  }
  __syncthreads();   // tmp is free again
  *total = tot;
  return off + x - v;
}

// ids[0..len) -> their spellings' symbols in dst[0..return); -1 if they would not fit `cap` (a longest-spelling
// argument smaller than the table's: nothing is written then)
template <int NT>
__device__ int expand(const int32_t* __restrict__ ids, int len, const int32_t* __restrict__ spell_off,
                      const int32_t* __restrict__ spell_sym, int drop_sym, uint16_t* dst, int cap, int* tmp) {
  const int per = (len + NT - 1) / NT;
  const int t0 = min(len, (int)threadIdx.x * per), t1 = min(len, t0 + per);
  int cnt = 0;
  for (int t = t0; t < t1; ++t) {
    const int id = ids[t];
    for (int k = spell_off[id], e = spell_off[id + 1]; k < e; ++k) cnt += spell_sym[k] != drop_sym;
  }
  int total;
  int at = block_scan<NT>(cnt, tmp, &total);
  if (total > cap) return -1;
  for (int t = t0; t < t1; ++t) {
    const int id = ids[t];
    for (int k = spell_off[id], e = spell_off[id + 1]; k < e; ++k) {
      const int s = spell_sym[k];
      if (s != drop_sym) dst[at++] = (uint16_t)s;
    }
  }
  __syncthreads();
  return total;
}

// the words of c[0..L) (maximal runs without `space`): start, length, FNV-1a hash; returns their number
template <int NT>
__device__ int find_words(const uint16_t* c, int L, int space, uint16_t* ws, uint16_t* wl, uint32_t* wh, int* tmp) {
  const int per = (L + NT - 1) / NT;
  const int p0 = min(L, (int)threadIdx.x * per), p1 = min(L, p0 + per);
  int cnt = 0;
  for (int p = p0; p < p1; ++p) cnt += c[p] != space && (p == 0 || c[p - 1] == space);
  int total;
  int at = block_scan<NT>(cnt, tmp, &total);
  for (int p = p0; p < p1; ++p) {
    if (c[p] != space && (p == 0 || c[p - 1] == space)) {
      uint32_t h = 2166136261u;
      int e = p;
      while (e < L && c[e] != space) h = (h ^ c[e++]) * 16777619u;
      ws[at] = (uint16_t)p;
      wl[at] = (uint16_t)(e - p);
      wh[at] = h;
      ++at;
    }
  }
  __syncthreads();
  return total;
}

template <int NT, int MODE>
__global__ __launch_bounds__(NT) void edit_kernel(const EditArgs a) {
  extern __shared__ uint32_t lds[];
  __shared__ int tmp[NT / 64];
  unsigned char* base = reinterpret_cast<unsigned char*>(lds);
  const EditPlan& P = a.plan;
  uint16_t* hc = reinterpret_cast<uint16_t*>(base);
  uint16_t* rc = reinterpret_cast<uint16_t*>(base + P.off_rc);
  uint16_t* diag = reinterpret_cast<uint16_t*>(base + P.off_diag);
  const int tid = threadIdx.x, pair = blockIdx.x;
  int32_t* out = a.out + (int64_t)pair * kOut;
  const int32_t* hyp = a.hyp + (int64_t)pair * a.hyp_stride;
  const int32_t* ref = a.ref + (int64_t)pair * a.ref_stride;
  const int hl = a.hyp_lens[(int64_t)pair * a.hyp_lens_stride], rl = a.ref_lens[(int64_t)pair * a.ref_lens_stride];

  // ---- the pair's own status: lengths inside the rows, ids inside the spelling table (ids past the length are not read)
  int status = 0;
  if (hl < 0 || hl > a.hyp_width || rl < 0 || rl > a.ref_width) {
    status = LR_EDIT_BAD_LENGTH;   // (uniform over the workgroup)
  } else {
    int bad = 0;
    for (int t = tid; t < hl; t += NT) bad |= (unsigned)hyp[t] >= (unsigned)a.n_classes;
    for (int t = tid; t < rl; t += NT) bad |= (unsigned)ref[t] >= (unsigned)a.n_classes;
    if (__syncthreads_or(bad)) status = LR_EDIT_BAD_ID;
  }
  int n = 0, m = 0;
  if (status == 0) {
    const int drop = MODE == LR_EDIT_WORDS ? -2 : a.space_sym;   // (-2 matches no symbol: the word unit keeps its spaces)
    n = expand<NT>(hyp, hl, a.spell_off, a.spell_sym, drop, hc, P.capH, tmp);
    m = expand<NT>(ref, rl, a.spell_off, a.spell_sym, drop, rc, P.capR, tmp);
    if (n < 0 || m < 0) status = LR_EDIT_BAD_SPELLING;
  }
  if (status != 0) {
    if (tid < kOut) out[tid] = tid == 0 ? status : 0;
    return;
  }

  uint16_t *hws = nullptr, *hwl = nullptr, *rws = nullptr, *rwl = nullptr;
  uint32_t *hwh = nullptr, *rwh = nullptr;
  if (MODE == LR_EDIT_WORDS) {
    unsigned char* w = base + P.off_words;
    hwh = reinterpret_cast<uint32_t*>(w);
    rwh = hwh + P.capWH;
    hws = reinterpret_cast<uint16_t*>(rwh + P.capWR);
    hwl = hws + P.capWH;
    rws = hwl + P.capWH;
    rwl = rws + P.capWR;
    n = find_words<NT>(hc, n, a.space_sym, hws, hwl, hwh, tmp);
    m = find_words<NT>(rc, m, a.space_sym, rws, rwl, rwh, tmp);
  }

  // ---- the walk-back table: zeroed, then every inner cell ORs its 2 bits in
  unsigned char* dirs = nullptr;
  const int rs = (m + 3) & ~3;   // cells per row
  if (MODE == LR_EDIT_CHARS_ALIGN) {
    dirs = P.dirs_in_lds ? base + P.off_dirs : a.dirs_ws + (size_t)pair * P.dirs_bytes;
    uint32_t* z = reinterpret_cast<uint32_t*>(dirs);
    const int words = (n * (rs >> 2) + 3) >> 2;
    for (int k = tid; k < words; k += NT) z[k] = 0u;
    __syncthreads();
  }

  // ---- D along anti-diagonals; diag[d % 3][i] = D[i][d - i]
  const int nd = P.nd;
  for (int d = 0; d <= n + m; ++d) {
    uint16_t* cur = diag + (d % 3) * nd;
    const uint16_t* p1 = diag + ((d + 2) % 3) * nd;
    const uint16_t* p2 = diag + ((d + 1) % 3) * nd;
    const int lo = max(0, d - m), hi = min(n, d);
    for (int i = lo + tid; i <= hi; i += NT) {
      const int j = d - i;
      int v;
      if (i == 0) {
        v = j;
      } else if (j == 0) {
        v = i;
      } else {
        bool eq;
        if (MODE == LR_EDIT_WORDS) {
          eq = hwh[i - 1] == rwh[j - 1] && hwl[i - 1] == rwl[j - 1];
          if (eq) {
            const uint16_t* x = hc + hws[i - 1];
            const uint16_t* y = rc + rws[j - 1];
            for (int k = 0, L = hwl[i - 1]; k < L; ++k)
              if (x[k] != y[k]) {
                eq = false;
                break;
              }
          }
        } else {
          eq = hc[i - 1] == rc[j - 1];
        }
        const int dg = p2[i - 1] + (eq ? 0 : 1);   // D[i-1][j-1]
        const int lf = p1[i] + 1;                  // D[i][j-1]: the reference character is absent (deletion)
        const int up = p1[i - 1] + 1;              // D[i-1][j]: the hypothesis character has no counterpart (insertion)
        v = min(dg, min(lf, up));
        if (MODE == LR_EDIT_CHARS_ALIGN) {
          const int code = v == dg ? 0 : (v == lf ? 1 : 2);   // the walk's order of preference
          if (code) {
            const int cell = (i - 1) * rs + (j - 1);
            dirs[cell >> 2] |= (unsigned char)(code << ((cell & 3) * 2));
          }
        }
      }
      cur[i] = (uint16_t)v;
    }
    __syncthreads();
  }

  if (tid != 0) return;
  const int dist = diag[((n + m) % 3) * nd + n];
  const bool open = a.gate == nullptr || *a.gate == 0;
  int hits = 0, sub = 0, ins = 0, del = 0;
  if (MODE == LR_EDIT_CHARS_ALIGN) {
    const int K = a.K;
    unsigned long long* conf = open ? a.conf : nullptr;
    const int64_t ld = K + 1;
    int i = n, j = m;
    while (i > 0 || j > 0) {
      int code;
      if (i > 0 && j > 0) {
        const int cell = (i - 1) * rs + (j - 1);
        code = (dirs[cell >> 2] >> ((cell & 3) * 2)) & 3;
      } else {
        code = j > 0 ? 1 : 2;
      }
      int r = K, h = K;
      if (code == 0) {
        r = rc[--j];
        h = hc[--i];
        if (r == h) ++hits; else ++sub;
      } else if (code == 1) {
        r = rc[--j];
        ++del;
      } else {
        h = hc[--i];
        ++ins;
      }
      if (conf && r <= K && h <= K) atomicAdd(conf + r * ld + h, 1ull);
    }
  }
  out[0] = 0;
  out[1] = dist;
  out[2] = m;
  out[3] = n;
  out[4] = hits;
  out[5] = sub;
  out[6] = ins;
  out[7] = del;
  if (a.totals && open) {
    unsigned long long* t = a.totals + (MODE == LR_EDIT_WORDS ? 8 : 0);
    atomicAdd(t + 0, (unsigned long long)dist);
    atomicAdd(t + 1, (unsigned long long)m);
    atomicAdd(t + 2, (unsigned long long)n);
    if (MODE == LR_EDIT_CHARS_ALIGN) {
      atomicAdd(t + 3, (unsigned long long)hits);
      atomicAdd(t + 4, (unsigned long long)sub);
      atomicAdd(t + 5, (unsigned long long)ins);
      atomicAdd(t + 6, (unsigned long long)del);
    }
    atomicAdd(t + 7, 1ull);
  }
}

template <int NT>
void launch(int mode, const EditArgs& a, int B, hipStream_t stream) {
  const unsigned lds = (unsigned)a.plan.lds_bytes;
  if (mode == LR_EDIT_WORDS)
    LR_LAUNCH((edit_kernel<NT, LR_EDIT_WORDS>), dim3(B), dim3(NT), lds, stream, a);
  else if (mode == LR_EDIT_CHARS_ALIGN)
    LR_LAUNCH((edit_kernel<NT, LR_EDIT_CHARS_ALIGN>), dim3(B), dim3(NT), lds, stream, a);
  else
    LR_LAUNCH((edit_kernel<NT, LR_EDIT_CHARS>), dim3(B), dim3(NT), lds, stream, a);
}

}  // namespace

extern "C" size_t lr_edit_workspace_bytes(int B, int hyp_width, int ref_width, int max_spelling, int mode) {
  EditPlan p;
  if (edit_plan(B, hyp_width, ref_width, max_spelling, mode, &p) != LR_OK) return 0;
  return edit_ws_bytes(p, B);
}

extern "C" int lr_edit_distance(const int32_t* hyp, int64_t hyp_stride, const int32_t* hyp_lens,
                                int64_t hyp_lens_stride, const int32_t* ref, int64_t ref_stride,
                                const int32_t* ref_lens, int64_t ref_lens_stride, const int32_t* spell_off,
                                const int32_t* spell_sym, int n_classes, int max_spelling, int space_sym, int mode,
                                int32_t* out, int64_t* totals, int64_t* conf, int K, const int32_t* gate,
                                void* workspace, size_t workspace_bytes, int B, int hyp_width, int ref_width,
                                lr_stream_t stream) {
  LR_CHECK_ARG(hyp && hyp_lens && ref && ref_lens && spell_off && spell_sym && out && workspace);
  LR_CHECK_ARG(n_classes > 0 && K > 0 && K < 65535 && space_sym >= -1 && space_sym < K);
  LR_CHECK_ARG(hyp_stride >= 0 && ref_stride >= 0 && hyp_lens_stride >= 0 && ref_lens_stride >= 0);
  EditPlan p;
  const int ok = edit_plan(B, hyp_width, ref_width, max_spelling, mode, &p);
  if (ok != LR_OK) return ok;
  if (workspace_bytes < edit_ws_bytes(p, B)) return LR_ERR_WORKSPACE;
  EditArgs a;
  a.hyp = hyp; a.hyp_lens = hyp_lens; a.ref = ref; a.ref_lens = ref_lens;
  a.spell_off = spell_off; a.spell_sym = spell_sym; a.gate = gate; a.out = out;
  a.totals = reinterpret_cast<unsigned long long*>(totals);
  a.conf = mode == LR_EDIT_CHARS_ALIGN ? reinterpret_cast<unsigned long long*>(conf) : nullptr;
  a.dirs_ws = static_cast<unsigned char*>(workspace);
  a.hyp_stride = hyp_stride; a.hyp_lens_stride = hyp_lens_stride;
  a.ref_stride = ref_stride; a.ref_lens_stride = ref_lens_stride;
  a.n_classes = n_classes; a.space_sym = space_sym; a.K = K; a.hyp_width = hyp_width; a.ref_width = ref_width;
  a.plan = p;
  if (p.threads == LR_WAVE)
    launch<LR_WAVE>(mode, a, B, (hipStream_t)stream);
  else
    launch<4 * LR_WAVE>(mode, a, B, (hipStream_t)stream);
  return lr_launch_status();
}
