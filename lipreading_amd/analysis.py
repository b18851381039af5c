"""Beam-search transcripts from the attention decoder — `src/models/lipreader/analysis.py:12-66` (inference).

The reference decodes one utterance at a time on the host, drawing each hypothesis's candidates with a multinomial.
Here the whole batch goes through one encoder pass and one `CharDecodingStep.beam_search` call on the device, with
the deterministic rule of lipreading_amd/csrc/lr_attn_beam.hip (top-K candidates; PAD and BOS never candidates).
The strings keep the reference's format.  The reference's confusion matrix (analysis.py:132-153) is computed here
from the decoded transcript's alignment on the device (confusion_matrix below); its plots are not ported.
"""
import torch

from .data import BOS, EOS, host_max_len

# analysis.py:133-139: the 26 letters grouped by viseme (vowels and w / b p m / f v / alveolars / j / velars and x / h)
VISEME_ORDER = list("aeiyouw" "bpm" "fv" "tdnszlr" "j" "kqcgx" "h")


def encode_for_beam(encoder, frames, frame_lens, device, with_ctc=False):
  """One encoder pass over the batch -> (hidden (B, T, Hd), frame_lens on the device, final_state, y): y is the CTC
  head's log-probs (B, T, V+1) of the same pass with with_ctc=True, else None."""
  if with_ctc:
    need_ctc_head(encoder)
  frame_lens_d = frame_lens.to(device)
  out = encoder(frames.to(device), frame_lens_d, max_len=host_max_len(frame_lens))
  hidden, state = (out[1], out[2]) if encoder.enable_ctc else (out[0], out[1])
  return hidden, frame_lens_d, state, (out[0] if with_ctc else None)


def need_ctc_head(encoder):
  """The joint search reads the encoder's CTC head: raise if it has none."""
  if not getattr(encoder, "enable_ctc", False):
    raise ValueError("joint CTC/attention decoding (ctc_weight > 0) needs an encoder built with enable_ctc=True")


def best_beam(decoding_step, hidden, frame_lens, state, beam_width, max_label_len, ctc_log_probs=None,
              ctc_weight=0.0, pre_beam=None, lm=None):
  """The best hypothesis of every utterance, left on the device: (ids (B, L) view, lens (B,) view) of beam slot 0.
  With ctc_log_probs the joint CTC/attention search; without, beam_search gets no joint keyword at all.  `lm` (a
  lm.WordLM) adds the word language model to either; without one beam_search gets no such keyword."""
  joint = {} if ctc_log_probs is None else dict(ctc_log_probs=ctc_log_probs, ctc_weight=ctc_weight,
                                                 pre_beam=pre_beam)
  if lm is not None:
    joint.update(lm=lm, pre_beam=pre_beam)
  ids, lens, _ = decoding_step.beam_search(hidden, frame_lens, state, beam_width=beam_width,
                                           max_label_len=max_label_len, **joint)
  return ids[:, 0], lens[:, 0]


def best_ids(decoding_step, hidden, frame_lens, state, beam_width, max_label_len, ctc_log_probs=None,
             ctc_weight=0.0, pre_beam=None, lm=None):
  """best_beam's hypotheses as host lists of token ids (the final EOS included when reached)."""
  ids, lens = best_beam(decoding_step, hidden, frame_lens, state, beam_width, max_label_len, ctc_log_probs,
                        ctc_weight, pre_beam, lm)
  ids, lens = ids.cpu(), lens.cpu()
  return [ids[b, :int(lens[b])].tolist() for b in range(ids.shape[0])]


def rescored_best(decoding_step, hidden, frame_lens, state, hyp_ids, hyp_lens, first_scores, ctc_weight=0.5,
                  length_bonus=0.0):
  """Two-pass decoding's answer, left on the device: the CTC N-best list (hyp_ids (B, N, W) classes,
  hyp_lens, first_scores: BeamCTCDecoder.decode_ids' ids, lens and scores, or their [:, :N] part) rescored by
  CharDecodingStep.rescore, and the hypothesis it ranks first returned in DECODER tokens (class - 1), cut at its first
  EOS: (ids (B, W) int32, lens (B,) int32), lens counting the tokens before that EOS.  Nothing is read back."""
  order = decoding_step.rescore(hidden, frame_lens, state, hyp_ids, hyp_lens, first_scores, ctc_weight=ctc_weight,
                                length_bonus=length_bonus)[0]
  B, _, W = hyp_ids.shape
  best = order[:, :1].long()
  ids = torch.gather(hyp_ids, 1, best[:, :, None].expand(B, 1, W))[:, 0] - 1
  lens = torch.gather(hyp_lens, 1, best)[:, 0].clamp(0, W).to(torch.int32)
  at = torch.arange(W, device=ids.device, dtype=torch.int32)[None, :]
  eos = decoding_step.char2idx[EOS]
  first_eos = torch.where((ids == eos) & (at < lens[:, None]), at, lens[:, None]).min(dim=1)[0]
  return ids, first_eos.to(torch.int32)


def inference(encoder, decoding_step, frames, frame_lens, chars, char_lens, device, char2idx, beam_width=5,
              max_label_len=100, ctc_weight=0.0, lm=None):
  """analysis.py:12-66.  Returns (outputs, gt): outputs[i] = '<BOS>' + the best hypothesis's characters (with
  '<EOS>' if it reached one), gt[i] = chars[i][:char_lens[i]] joined.  ctc_weight > 0 runs the joint CTC/attention
  search on the CTC head of the same encoder pass (the encoder needs enable_ctc); `lm` (a lm.WordLM over
  decoder.ctc_labels(char2idx)) adds the word language model to the search."""
  if ctc_weight > 0:
    need_ctc_head(encoder)
  idx2char = {val: key for key, val in char2idx.items()}
  encoder.eval()
  decoding_step.eval()
  with torch.no_grad():
    hidden, lens_d, state, y = encode_for_beam(encoder, frames, frame_lens, device, with_ctc=ctc_weight > 0)
    best = best_ids(decoding_step, hidden, lens_d, state, beam_width, max_label_len, ctc_log_probs=y,
                    ctc_weight=ctc_weight, lm=lm)
  outputs = [''.join(idx2char[int(i)] for i in [char2idx[BOS]] + h) for h in best]
  chars, char_lens = chars.cpu(), char_lens.cpu()
  gt = [''.join(idx2char[int(c)] for c in chars[i][:int(char_lens[i])]) for i in range(len(best))]
  return outputs, gt


def confusion_matrix(encoder, data_loader, device, char2idx, decoder=None, class_names=None):
  """Character confusion matrix of the CTC head's transcripts over `data_loader`: a numpy int64
  (len(class_names), len(class_names)) array, rows = the label's character, columns = the decoded one, in the
  reference's viseme order (VISEME_ORDER) by default.  decoder=None scores the greedy path, a BeamCTCDecoder its best
  hypothesis.

  This differs from the reference on purpose.  The reference (analysis.py:97-153) tabulates multinomial SAMPLES of
  the attention decoder under teacher forcing, position by position; this tabulates the DECODED transcript aligned
  to the label by the edit-distance walk back of lr_edit_distance (diagonal first, then a deletion,
  then an insertion), so a dropped or extra character shifts nothing.  Insertions and deletions have no cell in
  the returned cut; a class name outside the scorer's alphabet gets an all-zero row and column."""
  from . import train as T
  names = list(VISEME_ORDER if class_names is None else class_names)
  _, scorer = T._device_score_run(encoder, data_loader, device, char2idx, decoder=decoder, units=('char',), align=True)
  conf, symbols = scorer.confusion()
  conf = conf.cpu().numpy()
  at = {ch: i for i, ch in enumerate(symbols)}
  import numpy as np
  out = np.zeros((len(names), len(names)), dtype=np.int64)
  for i, r in enumerate(names):
    for j, h in enumerate(names):
      if r in at and h in at:
        out[i, j] = conf[at[r], at[h]]
  return out


def word_timings(encoder, data_loader, device, char2idx, fps=29.97):
  """Per utterance of `data_loader`, in its order: [(word, start_seconds, end_seconds, mean log-probability per
  frame)] from the forced alignment of the caption against the encoder's CTC head (train.align_loader, DESIGN.md
  §19); None for an utterance that could not be aligned (a clip too short to spell its caption)."""
  from . import train as T
  out = []
  for rec in T.align_loader(encoder, data_loader, device, char2idx, fps=fps):
    if rec["status"] != 0:
      out.append(None)
    else:
      out.append([(w, s / fps, e / fps, lp / max(e - s, 1)) for w, s, e, lp in rec["words"]])
  return out


def caption_contains(caption, keyword):
  """Does `keyword` (a word or a phrase) occur in `caption` at word boundaries: with the caption's edge or a ' ' on
  either side."""
  at = caption.find(keyword)
  while at >= 0:
    end = at + len(keyword)
    if (at == 0 or caption[at - 1] == ' ') and (end == len(caption) or caption[end] == ' '):
      return True
    at = caption.find(keyword, at + 1)
  return False


def keyword_counts(captions, hits, keywords):
  """Per keyword, at utterance level: dict(keyword, utterances (captions that contain it), hit (of those, how many have
  a hit of it), false_hits (hits of it on utterances whose caption does not contain it)).  `hits[i]` is utterance i's
  list of spot records (their `index` names the keyword).  Counts only: rates are the caller's."""
  out = [dict(keyword=kw, utterances=0, hit=0, false_hits=0) for kw in keywords]
  for caption, found in zip(captions, hits):
    per = [0] * len(out)
    for h in found:
      per[h["index"]] += 1
    for k, kw in enumerate(keywords):
      if caption_contains(caption, kw):
        out[k]["utterances"] += 1
        out[k]["hit"] += per[k] > 0
      else:
        out[k]["false_hits"] += per[k]
  return out


def keyword_report(encoder, data_loader, device, char2idx, keywords, **spotter_kw):
  """keyword_counts of train.spot_loader's hits against the loader's own captions (BOS and EOS
  stripped), both taken from ONE walk of the loader: a shuffling loader is counted right and pays its decode once."""
  from . import train as T
  inv = {v: k for k, v in char2idx.items()}
  keywords = list(keywords)
  captions, hits = [], []
  walk = T.spot_batches(encoder, data_loader, device, char2idx, keywords, **spotter_kw)
  for (_, _, chars, char_lens), spotted in walk:
    for b in range(len(char_lens)):
      captions.append(''.join(inv[int(c)] for c in chars[b, 1:int(char_lens[b]) - 1]))
    hits.extend(spotted)
  return keyword_counts(captions, hits, keywords)


def caption_shifts(records, min_confidence=0.5):
  """How far CTC segmentation moved each video's captions: per record of train.segment_videos (or of the
  driver's --segment file) dict(video, status, captions, median_shift_s, max_shift_s, low_confidence).  A caption's
  shift is the larger of |new_start_s - old_start_s| and |new_end_s - old_end_s|; low_confidence counts the captions
  whose confidence is below `min_confidence` or that hold no frame.  A video that was not segmented (status != 0) has
  None shifts and low_confidence = its number of captions."""
  out = []
  for rec in records:
    caps = rec["captions"]
    row = dict(video=rec["video"], status=rec["status"], captions=len(caps), median_shift_s=None, max_shift_s=None,
               low_confidence=len(caps))
    if rec["status"] == 0 and caps:
      shifts = sorted(max(abs(c["new_start_s"] - c["old_start_s"]), abs(c["new_end_s"] - c["old_end_s"])) for c in caps)
      mid = len(shifts) // 2
      row["median_shift_s"] = shifts[mid] if len(shifts) % 2 else 0.5 * (shifts[mid - 1] + shifts[mid])
      row["max_shift_s"] = shifts[-1]
      row["low_confidence"] = sum(1 for c in caps if c["confidence"] is None or c["confidence"] < min_confidence)
    out.append(row)
  return out


# ---- commit delay of a streamed beam search (decoder.BeamStream) ------------------------------------

def commit_delay(reads, offsets, total_frames):
  """How long after it was spoken each character of the final best hypothesis became final.

  reads: [(frames, stable)] of one utterance in feeding order — the frames consumed at a read and the stable-prefix
  length it reported; offsets: the final best hypothesis's frame offsets, one per character; total_frames: the
  utterance's length.  Character i is committed at the first read whose stable exceeds i; its delay is that read's
  frame count minus offsets[i].  A character no read before the end covered is committed when the utterance ends, at
  total_frames.  -> (delays [int] per character, how many were committed only at the end).  Pure: no tensors."""
  delays, at_end = [], 0
  k = 0
  reads = [(int(f), int(s)) for f, s in reads]
  for i, off in enumerate(offsets):
    while k < len(reads) and reads[k][1] <= i:
      k += 1   # stable never decreases, so the first covering read of character i is not before that of i - 1
    at = reads[k][0] if k < len(reads) else total_frames
    if at >= total_frames:
      at, at_end = total_frames, at_end + 1
    delays.append(at - int(off))
  return delays, at_end


def commit_delay_stats(per_utterance):
  """[(delays, at_end)] of commit_delay over a loader -> dict(chars, mean, p90, end_share): the mean and the 90th
  percentile (nearest rank) of the delays in frames, and the share of characters committed only at the end.  No
  characters: chars 0 and None for the rest."""
  delays = sorted(d for ds, _ in per_utterance for d in ds)
  n = len(delays)
  if n == 0:
    return dict(chars=0, mean=None, p90=None, end_share=None)
  rank = -(-9 * n // 10)   # ceil(0.9 n)
  return dict(chars=n, mean=sum(delays) / n, p90=delays[rank - 1],
              end_share=sum(e for _, e in per_utterance) / n)
