"""The caller on the other side of the hot path: what `src/scripts/train.py` does around
`train()` / `eval()`, so the reference's `config/` flag files drive the MI355X path unchanged.

  python -m lipreading_amd.driver config/train/attn/attention_type --data=<name> [--flag=value ...]

Mirrors (reference file:line, read for behaviour only):
  _init_models   train.py:57-79    VideoEncoder(...) + CharDecodingStep(...), same keyword arguments
  restore        train.py:82-132   name-and-shape tolerant checkpoint load
  train          train.py:134-320  flags and defaults :134-167; epoch loop: patience / annealing
                                   (lr /= 5, reload best weights) :256-268, linear teacher-forcing
                                   decay :270-272, Adam re-created every epoch :275-276, eval on
                                   val/train, best_{encoder,decoder}.pth :287-288
  flag files     utils/cmd_line.py: one `--name=value` per line; booleans as `--flag=True|False`
Out of scope here (the reference's control plane, not the path): tensorboard logging, sample
printing and confusion-matrix plots (train.py:296-318), sentence re-segmentation (needs spaCy).
"""
import os
import sys
import time

import numpy as np
import torch

DEFAULTS = dict(  # train.py:134-167
    data="StephenColbert/medium_no_vtx1", labels="labels.json", sentence_dataset=False,
    occlussion_threshold=0.8, train_split=0.8, num_workers=1, refresh=False,
    patience=10, batch_size=4, learning_rate=1e-4, annealings=2, enable_ctc=False, grad_norm=50,
    tr_epochs=50, max_tfr=0.9, min_tfr=0.0,
    num_layers=1, frame_dim=68 * 3, hidden_size=700, char_dim=300,
    rnn_type='LSTM', attention_type='1_layer_nn', attn_hidden_size=-1, bidirectional=False,
    rnn_dropout=0.0, seed=123456, cuda=False,
    # not reference flags: where data/ and weights/ live, a cap for smoke runs, and the encoder+CTC-only
    # loop (no attention decoder; error = greedy-decoded CER) that the archived trainer's flag files select
    root=".", max_epochs=None, ctc_only=False, step_graphs=True,
    # build-defined pixel regime (BASELINE configs[1] "3Dconv+BiGRU+CTC", configs[4] "transformer encoder over
    # per-frame conv features"): --frontend=conv3d reads a dataview written with frames (u8 frames + landmarks),
    # crops the mouth on the device (lr_lip_crop_u8) and puts the STCNN frontend in front of the sequence encoder;
    # --encoder=transformer swaps the recurrent encoder for the transformer (hidden_size = d_model, num_layers
    # layers, --nhead heads).  Either one selects the encoder+CTC loop with greedy CER (no attention decoder).
    frontend="none", encoder="rnn", nhead=4, crop_size=96,
    # the CTC decoder behind the ctc_only loop's CER: greedy (the default) or beam (decoder.BeamCTCDecoder, no
    # language model, ctcdecode's default cutoff_top_n=40) with --beam_width hypotheses; --lm_path (an ARPA
    # file, '' = none) adds a word language model weighted by --lm_alpha, plus --lm_beta per word
    ctc_decoder="greedy", beam_width=100, lm_path="", lm_alpha=0.0, lm_beta=0.0,
    # --hotwords=a,b,c ('' = none) tells the beam decoder which words to expect: each raises the score of the
    # hypotheses that spell it by --hotword_weight, at the start of a word (BeamCTCDecoder's hotwords)
    hotwords="", hotword_weight=10.0,
    # --stream_chunk=N (0 = off) with --ctc_decoder=beam: the evaluation decodes every batch through a resumable
    # session (decoder.BeamStream) fed N frames at a time with a read after every chunk, not in one
    # call.  A session equals the one-shot search bit for bit, so the CER / WER are by construction the same as
    # without the flag; what it adds is the validation pass's commit delay — how many frames after it was spoken a
    # character of the final transcript became final (mean, 90th percentile, share committed only at the end)
    stream_chunk=0,
    # --stream_encoder=True with --stream_chunk=N: the evaluation's encoder runs chunk by chunk as well, through a
    # resumable encoder session (encoder_stream.ChunkedEncoder) — the whole live transcriber, not only
    # its search.  Needs --ctc_decoder=beam, --bidirectional=False, --encoder=rnn and --frontend=none
    stream_encoder=False,
    # --stream_lookahead=N (-1 = off) with --stream_chunk=M: the evaluation's BIDIRECTIONAL encoder runs chunk by chunk
    # through a look-ahead session (encoder_lookahead.ChunkedLookaheadEncoder): the forward direction
    # carries its state, the backward one restarts N frames past every chunk.  CER / WER against N is the model's
    # accuracy / latency curve.  Needs --ctc_decoder=beam, --enable_ctc=True, --ctc_only=True, --bidirectional=True,
    # --encoder=rnn and --frontend=none; not together with --stream_encoder
    stream_lookahead=-1,
    # --stream_frontend=True with --frontend=conv3d: the evaluation's conv frontend runs chunk by chunk as well, through
    # a frontend session (frontend_stream.ChunkedPixelLipReader) in front of the encoder session: the
    # pixel regime streamed end to end.  Needs --encoder=rnn, --stream_chunk>0 and exactly one of --stream_encoder=True
    # (with --bidirectional=False) or --stream_lookahead>=0.  The frontend adds 3 frames of latency
    stream_frontend=False,
    # --tfm_chunk=N (0 = off) with --encoder=transformer: chunk-limited self-attention in training and
    # evaluation alike — a frame attends to its own chunk of N frames and --tfm_left_chunks=M whole chunks before it, so
    # the model looks at most N - 1 frames ahead whatever its depth, and can be run from a cache
    tfm_chunk=0, tfm_left_chunks=0,
    # --stream_tfm=True with --stream_chunk=N: the evaluation's transformer encoder runs chunk by chunk through a
    # session (transformer_stream.ChunkedTransformerEncoder); with --frontend=conv3d the conv frontend
    # runs through its own session in front of it.  Needs --encoder=transformer, --tfm_chunk>0 and --ctc_decoder=beam
    stream_tfm=False,
    # the error of a model WITH the attention decoder: teacher (the live loop's sampled-token mismatch rate under
    # teacher forcing, train.eval) or beam (the edit-distance CER of the decoder's own beam-search transcript,
    # train.attention_cer, --attn_beam_width hypotheses of up to --attn_max_label_len characters) or joint (the same
    # CER of the joint CTC/attention beam search, the CTC head's prefix probability weighted by --attn_ctc_weight;
    # needs --enable_ctc) or rescore (two-pass decoding, DESIGN.md §32: the CER of the CTC beam search's
    # --attn_rescore_nbest best hypotheses rescored by the attention decoder, train.rescored_cer, the first pass weighted
    # by --attn_ctc_weight and --attn_length_bonus added per scored token; needs --enable_ctc=True, --ctc_decoder=beam
    # and a decoder, and takes --lm_path / --hotwords for its first pass)
    attn_decode="teacher", attn_beam_width=10, attn_max_label_len=100, attn_ctc_weight=0.3,
    attn_rescore_nbest=10, attn_length_bonus=0.0,
    # --attn_lm_path (an ARPA file, '' = none) adds a word language model to the --attn_decode=beam|joint search
    # (lm.WordLM), weighted by --attn_lm_alpha, plus --attn_lm_beta per word
    attn_lm_path="", attn_lm_alpha=0.0, attn_lm_beta=0.0,
    # --prefetch=N > 0: the three loaders are loader.PrefetchLoader of depth N (batch k+1 is gathered into pinned
    # memory, uploaded and collated on a copy stream while step k runs); 0 = the plain BatchLoader
    prefetch=0,
    # --augment=flip=0.5,shift=0.08,zoom=0.1,tjitter=0.05,tmask=2x10: training-time clip augmentation of the TRAIN
    # loader only (augment.AugmentSpec; applied inside the prefetch loader's collate launch, so it needs --prefetch);
    # the per-epoch Train CER is scored on clean clips.  --augment_seed: the stream of draws (None = --seed)
    augment="", augment_seed=None,
    # --crop=box|stable: the mouth window of the pixel regime, for the train, validation and test loaders alike (a model
    # is evaluated on the crops it was trained on).  box: the bounding box of each frame's mouth points
    # (lr_lip_crop_u8).  stable: centre = the mouth points' mean, side = --crop_extent eye distances, axes along the
    # line between the eyes, all averaged over 2 * --crop_smooth + 1 frames (lr_lip_stable_collate_u8)
    crop="box", crop_extent=1.25, crop_smooth=2,
    # --lmk_pose=none|rigid|similarity: the landmark regime's counterpart, for the train, validation and test loaders
    # alike.  Every frame's landmarks are aligned to a canonical face inside the collate launch
    # (lr_lmk_pose_collate_f32, landmarks.PoseSpec): the head's translation and rotation (rigid) and also its scale
    # (similarity) are taken out, estimated from the nose bridge and the eye corners over 2 * --lmk_pose_smooth + 1
    # frames.  --lmk_pose_template=PATH.npy: the canonical face (68, 3); loaded when the file exists, otherwise fitted
    # from the training set (landmarks.fit_template) and written there ('' = fitted, not written)
    lmk_pose="none", lmk_pose_smooth=0, lmk_pose_template="",
    # --lmk_augment=mirror=0.5,rot=10/10/15,scale=0.1,stretch=0.05,shift=0.05,jitter=0.01: training-time augmentation
    # of the landmark regime's TRAIN batches (augment.LandmarkAugmentSpec: one 3x3 matrix, a shift and noise per clip;
    # lr_lmk_augment_f32 behind the prefetch loader's collate launch, so it needs --prefetch).  Its seed is
    # --augment_seed (None = --seed); the per-epoch Train CER is scored on clean clips
    lmk_augment="",
    # who scores the transcripts behind the edit-distance errors (greedy, --ctc_decoder=beam, --attn_decode=beam|joint):
    # host (the Python loops of train.greedy_cer / ctc_cer / attention_cer) or device (train.device_scores: the ids
    # never leave the GPU, lr_edit_distance scores them, one read per loader; the epoch summary then carries val_wer)
    score="host",
    # --align=PATH ('' = off): after the last epoch, the forced alignment of every validation caption against the CTC
    # head as it then stands (train.align_loader: lr_ctc_align) — one JSON object per line: utterance index, status,
    # total, words and characters with their frame and second spans.  Needs a CTC head.
    align="",
    # --spot=PATH ('' = off) with --keywords=a,b,c (or a file, one keyword per line): after the last epoch, where each
    # keyword is spoken in every validation utterance by the CTC head as it then stands (train.spot_loader:
    # lr_ctc_spot) — one JSON object per line: utterance index, frames, hits with their frame and second spans, score
    # and confidence.  --spot_confidence=p in (0, 1] (0 = no threshold) keeps spans whose per-character confidence is
    # at least p; --spot_max_hits spans per (utterance, keyword).  Needs a CTC head.
    spot="", keywords="", spot_confidence=0.0, spot_max_hits=4,
    # --segment=PATH ('' = off): after the last epoch, CTC segmentation of every validation VIDEO (train.segment_videos:
    # lr_ctc_segment) — the video's clips encoded and joined into one stream, its whole caption track aligned against it
    # with both ends free — one JSON object per line: the video, status, stream length, and per kept caption its text,
    # old and new times, confidence and worst character.  Needs a CTC head.
    segment="",
    # --mwer=N (0 = off): train the encoder+CTC loop on the expected edit distance over the beam search's N best
    # hypotheses (minimum word / character error rate, train.train_mwer) plus --mwer_ctc_weight times the
    # CTC loss as an anchor.  --mwer_unit=char|word: the edit distance that is the risk.  --mwer_reference=True adds the
    # reference transcript as one more hypothesis where no beam is exact.  Needs --ctc_decoder=beam and a CTC-only
    # regime; the search is the evaluation's own (beam width, language model, hotwords).
    mwer=0, mwer_ctc_weight=0.01, mwer_unit="char", mwer_reference=False,
    # --transducer=True: a transducer head (transducer.TransducerHead) beside the CTC head of the
    # encoder+CTC loop, for every --frontend / --encoder combination: trained on the RNN-T loss plus
    # --transducer_ctc_weight times the CTC loss (train.train_transducer); the validation and test errors are the CER of
    # its greedy transcripts (at most --transducer_max_symbols characters per frame), and best_transducer.pth is kept
    # beside best_encoder.pth.  --transducer_joint: the joint width, --transducer_embed: the label embedding's,
    # --transducer_context=1|2: how many previous characters the prediction network sees.  Needs --enable_ctc=True
    # --ctc_only=True; not together with --mwer, the --stream_* flags or another --attn_decode than the default.
    # --transducer_beam=W (0: greedy): the reported CER is that of the top hypothesis of the transducer beam search of
    # width W <= 32 (transducer.rnnt_beam; at most --transducer_max_symbols <= 8 label rounds per frame)
    transducer=False, transducer_joint=256, transducer_embed=64, transducer_context=2, transducer_ctc_weight=0.3,
    transducer_max_symbols=5, transducer_beam=0,
)


def _coerce(name, text, like):
  if isinstance(like, bool):
    if text.lower() in ("true", "1", "yes", ""):
      return True
    if text.lower() in ("false", "0", "no"):
      return False
    raise ValueError("--%s expects True/False, got %r" % (name, text))
  if like is None:
    return None if text.lower() == "none" else int(text)
  if isinstance(like, int):
    return int(float(text)) if text.lower() != "none" else None
  if isinstance(like, float):
    return float(text)
  return text


# Flags of the reference's config/ files that are not parameters of the live train() (train.py:134-167):
#  - `--teacher_forcing_ratio` (config/train/attn/*, config/archive/experiments/ecd/*) predates the
#    max_tfr/min_tfr schedule; it maps to max_tfr.
#  - the archived trainer's set (archive/train_model.py:186-205; config/train/micro and
#    config/train/test_train_nano — BASELINE configs[0]/[1] — are written in it): the ones with a live
#    counterpart are renamed, the rest (SGD momentum, checkpointing, tensorboard) have no meaning on
#    this path and are accepted with a warning.  That trainer is CTC-only, so its files switch enable_ctc on.
RENAMED = {"teacher_forcing_ratio": "max_tfr", "dataset": "data", "batch": "batch_size", "epochs": "max_epochs",
           "hidden_layers": "num_layers", "max_norm": "grad_norm"}
IGNORED = {"momentum", "anneal", "annealing", "checkpoint", "tensorboard", "continue_from", "silent"}
ARCHIVED_ONLY = {"dataset", "batch", "epochs", "hidden_layers", "max_norm"} | IGNORED


def parse_flags(argv, defaults=DEFAULTS):
  """Positional arguments are flag files (one or several `--name=value` tokens per line, as under
  the reference's config/); later `--name=value` arguments override them.  Unknown flags are an
  error, as in the reference's argument parser; deprecated / archived ones (RENAMED, IGNORED) are
  accepted with a warning."""
  tokens = []
  for a in argv:
    if a.startswith("--"):
      tokens.append(a)
    else:
      with open(a) as f:
        tokens += [t for t in f.read().replace("\n", " ").split(" ") if t.startswith("--")]
  out = dict(defaults)
  archived = False
  explicit = set()
  for t in tokens:
    name, _, text = t[2:].partition("=")
    archived = archived or name in ARCHIVED_ONLY
    if name in IGNORED:
      print("warning: --%s has no meaning on this path; ignored" % name, file=sys.stderr)
      continue
    if name in RENAMED:
      print("warning: --%s is read as --%s" % (name, RENAMED[name]), file=sys.stderr)
      name = RENAMED[name]
    if name not in out:
      raise SystemExit("unknown flag --%s" % name)
    out[name] = _coerce(name, text, defaults[name])
    explicit.add(name)
  if isinstance(out.get("rnn_type"), str):
    out["rnn_type"] = out["rnn_type"].upper()          # the archived files write `gru`
  if archived:
    # archive/train_model.py trains a CTC-only model (no attention decoder) and reports greedy CER/WER; its
    # LipReader is bidirectional throughout.  These are that trainer's DEFAULTS: a flag the command line or the
    # file sets itself (e.g. --bidirectional=False) wins.
    for name, value in (("enable_ctc", True), ("ctc_only", True), ("bidirectional", True)):
      if name not in explicit:
        out[name] = value
  if out.get("frontend") not in ("none", "conv3d"):
    raise SystemExit("--frontend must be none or conv3d")
  if out.get("encoder") not in ("rnn", "transformer"):
    raise SystemExit("--encoder must be rnn or transformer")
  if out.get("ctc_decoder") not in ("greedy", "beam"):
    raise SystemExit("--ctc_decoder must be greedy or beam")
  if out.get("lm_path") and out.get("ctc_decoder") != "beam":
    raise SystemExit("--lm_path needs --ctc_decoder=beam")
  if (out.get("hotwords") or "hotword_weight" in explicit) and out.get("ctc_decoder") != "beam":
    raise SystemExit("--hotwords and --hotword_weight need --ctc_decoder=beam")
  if int(out.get("stream_chunk") or 0) < 0:
    raise SystemExit("--stream_chunk must be >= 0")
  if out.get("stream_chunk") and out.get("ctc_decoder") != "beam":
    raise SystemExit("--stream_chunk needs --ctc_decoder=beam")
  stream_frontend_check(out)
  stream_encoder_check(out)
  stream_lookahead_check(out)
  tfm_chunk_check(out)
  if out.get("attn_decode") not in ("teacher", "beam", "joint", "rescore"):
    raise SystemExit("--attn_decode must be teacher, beam, joint or rescore")
  attn_rescore_check(out)
  if out.get("attn_decode") == "joint" and not out.get("enable_ctc"):
    raise SystemExit("--attn_decode=joint needs --enable_ctc (the CTC head's log-probs)")
  if out.get("attn_lm_path") and out.get("attn_decode") not in ("beam", "joint"):
    raise SystemExit("--attn_lm_path needs --attn_decode=beam or joint")
  if not 0.0 <= float(out.get("attn_ctc_weight", 0.3)) <= 1.0:
    raise SystemExit("--attn_ctc_weight must be in [0, 1]")
  if not 1 <= int(out.get("attn_beam_width", 10)) <= 32:
    raise SystemExit("--attn_beam_width must be in [1, 32]")
  if int(out.get("attn_max_label_len", 100)) < 1:
    raise SystemExit("--attn_max_label_len must be positive")
  if out.get("score") not in ("host", "device"):
    raise SystemExit("--score must be host or device")
  if out["frontend"] != "none" or out["encoder"] != "rnn":
    # the build-defined regimes are encoder + CTC (BASELINE configs[1], [4]); no attention decoder behind them
    for name in ("enable_ctc", "ctc_only"):
      if name not in explicit:
        out[name] = True
  augment_spec(out)
  lmk_augment_spec(out)
  crop_check(out)
  lmk_pose_check(out)
  align_check(out)
  spot_check(out)
  segment_check(out)
  mwer_check(out)
  transducer_check(out)
  return out


def augment_spec(f):
  """The AugmentSpec of the flags `f` (None without --augment).  ValueError for a policy that does not parse and for
  --augment without --prefetch: the augmentation runs inside the prefetch loader's collate launch."""
  from .augment import AugmentSpec
  seed = f.get("augment_seed")
  spec = AugmentSpec.parse(f.get("augment") or "", seed=f.get("seed", 0) if seed is None else seed)
  if spec is not None and not f.get("prefetch"):
    raise ValueError("--augment=%s needs --prefetch=N > 0 (got --prefetch=%r)" % (f["augment"], f.get("prefetch")))
  return spec


def lmk_augment_spec(f):
  """The LandmarkAugmentSpec of the flags `f` (None without --lmk_augment).  ValueError for a policy that does not
  parse, for --lmk_augment without --prefetch (lr_lmk_augment_f32 runs behind the prefetch loader's collate launch) and
  for --lmk_augment in the pixel regime, which feeds no landmarks to the encoder."""
  from .augment import LandmarkAugmentSpec
  seed = f.get("augment_seed")
  spec = LandmarkAugmentSpec.parse(f.get("lmk_augment") or "", seed=f.get("seed", 0) if seed is None else seed)
  if spec is not None and not f.get("prefetch"):
    raise ValueError("--lmk_augment=%s needs --prefetch=N > 0 (got --prefetch=%r)"
                     % (f["lmk_augment"], f.get("prefetch")))
  if spec is not None and f.get("frontend", "none") == "conv3d":
    raise ValueError("--lmk_augment=%s augments the landmarks the encoder reads; --frontend=conv3d reads mouth crops "
                     "(its counterpart is --augment)" % f["lmk_augment"])
  return spec


def crop_check(f):
  """ValueError for a --crop that is neither box nor stable, and for a window --crop=stable cannot cut."""
  crop = f.get("crop", "box")
  if crop not in ("box", "stable"):
    raise ValueError("--crop must be box or stable (got --crop=%r)" % (crop,))
  if crop == "stable":
    extent, smooth = f.get("crop_extent"), f.get("crop_smooth")
    if not (isinstance(extent, float) and 0.0 < extent < float("inf")):
      raise ValueError("--crop_extent must be a positive number (got %r)" % (extent,))
    if not (isinstance(smooth, int) and 0 <= smooth <= 32):
      raise ValueError("--crop_smooth must be in [0, 32] frames (got %r)" % (smooth,))
  return crop


def lmk_pose_check(f):
  """ValueError for a --lmk_pose that is none of none, rigid and similarity, for a --lmk_pose_smooth outside [0, 32] and
  for --lmk_pose in the pixel regime, which feeds no landmarks to the encoder."""
  mode = f.get("lmk_pose", "none")
  if mode not in ("none", "rigid", "similarity"):
    raise ValueError("--lmk_pose must be none, rigid or similarity (got --lmk_pose=%r)" % (mode,))
  if mode == "none":
    return mode
  smooth = f.get("lmk_pose_smooth", 0)
  if isinstance(smooth, bool) or not (isinstance(smooth, int) and 0 <= smooth <= 32):
    raise ValueError("--lmk_pose_smooth must be in [0, 32] frames (got %r)" % (smooth,))
  if f.get("frontend", "none") == "conv3d":
    raise ValueError("--lmk_pose=%s normalises the landmarks the encoder reads; --frontend=conv3d reads mouth crops "
                     "(its counterpart is --crop=stable)" % mode)
  return mode


def lmk_pose_spec(f, train_set, device):
  """The PoseSpec of the flags `f` (None for --lmk_pose=none).  The template is loaded from --lmk_pose_template when
  that file exists; otherwise it is fitted from `train_set`'s clips and written there (under torch.distributed by rank
  0 only).  One printed line says which."""
  if lmk_pose_check(f) == "none":
    return None
  from .landmarks import PoseSpec, fit_template
  path = f.get("lmk_pose_template") or ""
  if path and os.path.isfile(path):
    template = np.load(path, allow_pickle=False)
    if template.shape != (68, 3):
      raise ValueError("--lmk_pose_template=%s holds shape %r, not (68, 3)" % (path, tuple(template.shape)))
    print("Landmark pose: %s, template loaded from %s" % (f["lmk_pose"], path))
  else:
    template = fit_template(train_set.frames, device=device)
    writer = not (torch.distributed.is_available() and torch.distributed.is_initialized()
                  and torch.distributed.get_rank() != 0)
    if path and writer:
      if os.path.dirname(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
      with open(path, "wb") as fh:           # (np.save(path) would append .npy to another extension)
        np.save(fh, template)
    print("Landmark pose: %s, template fitted from %d training clips%s"
          % (f["lmk_pose"], len(train_set.frames), " and written to %s" % path if path and writer else ""))
  return PoseSpec(template, radius=int(f.get("lmk_pose_smooth", 0)), scale=f["lmk_pose"] == "similarity")


def align_check(f):
  """ValueError for --align without a CTC head (neither --enable_ctc nor a regime that is encoder + CTC)."""
  if f.get("align") and not f.get("enable_ctc"):
    raise ValueError("--align=%s needs a CTC head: --enable_ctc=True (or a CTC-only regime)" % f["align"])


def segment_check(f):
  """ValueError for --segment without a CTC head (neither --enable_ctc nor a regime that is encoder + CTC)."""
  if f.get("segment") and not f.get("enable_ctc"):
    raise ValueError("--segment=%s needs a CTC head: --enable_ctc=True (or a CTC-only regime)" % f["segment"])


def mwer_check(f):
  """ValueError for --mwer outside the encoder+CTC loop or without the beam decoder, for an N the kernels or the
  search cannot serve, and for a unit that is neither char nor word."""
  if f.get("mwer_unit", "char") not in ("char", "word"):
    raise ValueError("--mwer_unit must be char or word (got --mwer_unit=%r)" % (f["mwer_unit"],))
  n = f.get("mwer") or 0
  if not n:
    return
  if not (f.get("ctc_only") and f.get("enable_ctc")):
    raise ValueError("--mwer=%d trains the encoder+CTC loop: it needs --ctc_only=True --enable_ctc=True (or a "
                     "CTC-only regime)" % n)
  if f.get("ctc_decoder") != "beam":
    raise ValueError("--mwer=%d needs --ctc_decoder=beam: its hypotheses are the beam search's" % n)
  slots = n + bool(f.get("mwer_reference"))
  if n < 1 or slots > 16 or n > int(f.get("beam_width", 100)):
    raise ValueError("--mwer=%d: between 1 and %d hypotheses%s, and no more than --beam_width=%s"
                     % (n, 16 - bool(f.get("mwer_reference")), " beside the reference" * bool(f.get("mwer_reference")),
                        f.get("beam_width")))
  if not float(f.get("mwer_ctc_weight", 0.01)) >= 0.0:
    raise ValueError("--mwer_ctc_weight must be >= 0 (got %r)" % (f["mwer_ctc_weight"],))


def transducer_check(f):
  """ValueError for --transducer outside the encoder+CTC loop, together with a flag whose evaluation or training it
  would replace, or with sizes the kernels do not take."""
  beam = int(f.get("transducer_beam", 0))
  if beam and not f.get("transducer"):
    raise ValueError("--transducer_beam=%d searches the transducer head: it needs --transducer=True" % beam)
  if not f.get("transducer"):
    return
  if not 0 <= beam <= 32:
    raise ValueError("--transducer_beam must be in [0, 32] (0: greedy; got %d)" % beam)
  if beam > 0 and int(f.get("transducer_max_symbols", 5)) > 8:
    raise ValueError("--transducer_beam=%d runs at most 8 label rounds per frame: --transducer_max_symbols=%d is too "
                     "many" % (beam, int(f["transducer_max_symbols"])))
  if not (f.get("ctc_only") and f.get("enable_ctc")):
    raise ValueError("--transducer=True trains beside the encoder+CTC loop: it needs --ctc_only=True --enable_ctc=True")
  if f.get("mwer"):
    raise ValueError("--transducer=True and --mwer=%d both replace the training objective: choose one" % f["mwer"])
  streaming = [n for n in ("stream_chunk", "stream_encoder", "stream_frontend", "stream_tfm") if f.get(n)]
  if int(f.get("stream_lookahead", -1)) >= 0:
    streaming.append("stream_lookahead")
  if streaming:
    raise ValueError("--transducer=True is evaluated one-shot by its greedy decoder: not together with --%s (a live "
                     "session over the decoder's state is not built)" % streaming[0])
  if f.get("attn_decode", "teacher") != "teacher":
    raise ValueError("--transducer=True has no attention decoder behind it: --attn_decode=%s does not apply"
                     % f["attn_decode"])
  if f.get("score", "host") != "host":
    raise ValueError("--transducer=True is scored by the host CER loop: --score=%s does not apply" % f["score"])
  if int(f.get("transducer_context", 2)) not in (1, 2):
    raise ValueError("--transducer_context must be 1 or 2 (got %r)" % (f["transducer_context"],))
  if not 1 <= int(f.get("transducer_joint", 256)) <= 512 or int(f.get("transducer_embed", 64)) < 1:
    raise ValueError("--transducer_joint must be in [1, 512] and --transducer_embed positive (got %r, %r)"
                     % (f.get("transducer_joint"), f.get("transducer_embed")))
  if int(f.get("transducer_max_symbols", 5)) < 1:
    raise ValueError("--transducer_max_symbols must be at least 1 (got %r)" % (f["transducer_max_symbols"],))
  if not float(f.get("transducer_ctc_weight", 0.3)) >= 0.0:
    raise ValueError("--transducer_ctc_weight must be >= 0 (got %r)" % (f["transducer_ctc_weight"],))


def spot_check(f):
  """ValueError for --spot without a CTC head or without --keywords, and for thresholds outside their ranges."""
  if not f.get("spot"):
    return
  if not f.get("enable_ctc"):
    raise ValueError("--spot=%s needs a CTC head: --enable_ctc=True (or a CTC-only regime)" % f["spot"])
  if not f.get("keywords"):
    raise ValueError("--spot=%s needs --keywords=a,b,c or --keywords=FILE" % f["spot"])
  if not 0.0 <= float(f.get("spot_confidence") or 0.0) <= 1.0:
    raise ValueError("--spot_confidence must be 0 (no threshold) or a confidence up to 1, got %r"
                     % (f["spot_confidence"],))
  if not 1 <= int(f.get("spot_max_hits", 4)) <= 16:
    raise ValueError("--spot_max_hits must be in [1, 16], got %r" % (f["spot_max_hits"],))


def read_keywords(text):
  """--keywords: a comma-separated list, or a file with one keyword per line.  Text with a comma in it is always a
  list; without one it is a file if it names one, else a single keyword.  Blanks around a keyword are dropped (blanks
  inside a phrase stay); empty entries and lines are skipped."""
  if "," not in text and os.path.isfile(text):
    with open(text) as f:
      words = f.read().splitlines()
  else:
    words = text.split(",")
  words = [w.strip() for w in words if w.strip()]
  if not words:
    raise ValueError("--keywords=%s names no keyword" % text)
  return words


def write_spots(path, encoder, loader, device, char2idx, keywords, min_confidence=None, max_hits=4, fps=29.97):
  """train.spot_loader over `loader` as JSON lines in `path`: index, frames, hits (keyword, start / end in frames,
  start_s / end_s in seconds, score, confidence).  Returns dict(path, utterances, keywords, hits)."""
  import json
  from . import train as T
  n = total = 0
  with open(path, "w") as out:
    for rec in T.spot_loader(encoder, loader, device, char2idx, keywords, fps=fps, max_hits=max_hits,
                             min_confidence=min_confidence):
      found = [dict(keyword=h["keyword"], start=h["start"], end=h["end"], start_s=h["start"] / fps,
                    end_s=h["end"] / fps, score=h["score"], confidence=h["confidence"]) for h in rec["hits"]]
      out.write(json.dumps(dict(index=rec["index"], frames=rec["frames"], hits=found)) + "\n")
      n += 1
      total += len(found)
  return dict(path=path, utterances=n, keywords=len(keywords), hits=total)


def write_segments(path, encoder, vid_dirs, device, char2idx, batch_size, fps=29.97, **how):
  """train.segment_videos over `vid_dirs` as JSON lines in `path`, one per video (its record as it is).  Returns
  dict(path, videos, captions, segmented): videos written, captions kept in them, videos with status 0.  `how` goes to
  segment_videos (the collate function and `pixels` of the regime, the occlusion threshold)."""
  import json
  from . import train as T
  n = caps = ok = 0
  with open(path, "w") as out:
    for rec in T.segment_videos(encoder, vid_dirs, device, char2idx, batch_size, fps=fps, **how):
      out.write(json.dumps(rec) + "\n")
      n += 1
      caps += len(rec["captions"])
      ok += rec["status"] == 0
  return dict(path=path, videos=n, captions=caps, segmented=int(ok))


def write_alignments(path, encoder, loader, device, char2idx, fps=29.97):
  """train.align_loader over `loader` as JSON lines in `path`: index, status, total, frames, and for words and chars
  text, start / end (frames), start_s / end_s (seconds) and logp.  Returns dict(path, utterances, infeasible)."""
  import json
  from . import train as T

  def spans(items):
    return [dict(text=t, start=s, end=e, start_s=s / fps, end_s=e / fps, logp=lp) for t, s, e, lp in items]

  n = infeasible = 0
  with open(path, "w") as out:
    for rec in T.align_loader(encoder, loader, device, char2idx, fps=fps):
      out.write(json.dumps(dict(index=rec["index"], status=rec["status"], total=rec["total"], frames=rec["frames"],
                                words=spans(rec["words"]), chars=spans(rec["chars"]))) + "\n")
      n += 1
      infeasible += rec["status"] == 1
  return dict(path=path, utterances=n, infeasible=int(infeasible))


def init_models(char2idx, num_layers, frame_dim, hidden_size, char_dim, enable_ctc, rnn_type,
                attention_type, attn_hidden_size, bidirectional, rnn_dropout, device):
  """train.py:57-79 with the HIP-backed modules."""
  from .attention_decoder import CharDecodingStep
  from .encoder import VideoEncoder
  encoder = VideoEncoder(frame_dim, hidden_size, rnn_type=rnn_type, num_layers=num_layers,
                         bidirectional=bidirectional, rnn_dropout=rnn_dropout, enable_ctc=enable_ctc,
                         vocab_size=len(char2idx), char2idx=char2idx, device=device).to(device)
  decoding_step = CharDecodingStep(encoder, char_dim=char_dim, vocab_size=len(char2idx), char2idx=char2idx,
                                   rnn_dropout=rnn_dropout, attention_type=attention_type,
                                   attn_hidden_size=attn_hidden_size, device=device).to(device)
  return encoder, decoding_step


def init_pixel_model(char2idx, f, device):
  """BUILD-DEFINED (no reference symbol): [conv3d frontend ->] recurrent or transformer encoder -> CTC head.
  The sequence encoder keeps the reference's constructor arguments where it has them."""
  from .encoder import VideoEncoder
  pixels = f["frontend"] == "conv3d"
  frame_dim = f["frame_dim"]
  if pixels:
    from .frontend import ConvFrontend3D, PixelLipReader, feature_dim
    frame_dim = feature_dim(f["crop_size"], f["crop_size"])
  if f["encoder"] == "transformer":
    from .transformer import TransformerVideoEncoder
    enc = TransformerVideoEncoder(frame_dim, d_model=f["hidden_size"], nhead=f["nhead"], num_layers=f["num_layers"],
                                  dim_feedforward=4 * f["hidden_size"], enable_ctc=True, vocab_size=len(char2idx),
                                  char2idx=char2idx, attn_chunk=int(f.get("tfm_chunk") or 0),
                                  attn_left_chunks=int(f.get("tfm_left_chunks") or 0))
  else:
    enc = VideoEncoder(frame_dim, f["hidden_size"], rnn_type=f["rnn_type"], num_layers=f["num_layers"],
                       bidirectional=f["bidirectional"], rnn_dropout=f["rnn_dropout"], enable_ctc=True,
                       vocab_size=len(char2idx), char2idx=char2idx, device=device)
  model = PixelLipReader(enc, ConvFrontend3D()) if pixels else enc
  return model.to(device)


def restore(net, save_file, verbose=True):
  """Load every tensor of the checkpoint whose name exists in `net` with the same shape; report
  (not raise on) the rest — train.py:82-132.  Accepts the reference's `best_encoder.pth` /
  `best_decoder.pth` state_dicts: the HIP-backed modules keep the reference's key names
  (SURVEY.md 8b).  Returns (restored, ignored, untouched) name lists."""
  own = net.state_dict()
  ckpt = torch.load(save_file, map_location="cpu")
  restored, mismatched = [], []
  with torch.no_grad():
    for name, value in ckpt.items():
      if name not in own:
        continue
      if tuple(own[name].shape) != tuple(value.shape):
        mismatched.append(name)
        if verbose:
          print('\t\tShape mismatch for var', name, 'expected', tuple(own[name].shape), 'got', tuple(value.shape))
        continue
      own[name].copy_(value.data if isinstance(value, torch.nn.Parameter) else value)
      restored.append(name)
  ignored = sorted(set(ckpt.keys()) - set(restored))
  untouched = sorted(set(own.keys()) - set(restored))
  if verbose:
    print('\t\tRestored all variables' if not ignored else '\t\tDid not restore:\n\t' + '\n\t'.join(ignored))
    print('\t\tNo new variables' if not untouched
          else '\t\tInitialized but did not modify:\n\t' + '\n\t'.join(untouched))
    print('\tRestored %s' % save_file)
  return restored, ignored, untouched


def weights_path(root, data):
  """weights/<data>/<n>: a fresh numbered directory per run (utility.py getRelWeightsPath)."""
  base = os.path.join(root, "weights", data)
  os.makedirs(base, exist_ok=True)
  taken = [int(d) for d in os.listdir(base) if d.isdigit()]
  path = os.path.join(base, str(max(taken) + 1 if taken else 0))
  os.makedirs(path)
  return path


def attn_rescore_check(f):
  """--attn_decode=rescore needs both heads and the CTC beam search, and streams only through the causal RNN session:
  SystemExit naming the flag otherwise."""
  import math
  if f.get("attn_decode") != "rescore":
    return
  nbest, bonus = f.get("attn_rescore_nbest", 10), f.get("attn_length_bonus", 0.0)
  if isinstance(nbest, bool) or not isinstance(nbest, int) or not 1 <= nbest <= min(int(f.get("beam_width", 100)), 128):
    raise SystemExit("--attn_rescore_nbest must be in [1, min(--beam_width, 128)]")
  if isinstance(bonus, bool) or not isinstance(bonus, (int, float)) or not math.isfinite(bonus):
    raise SystemExit("--attn_length_bonus must be a finite number")
  if not f.get("enable_ctc"):
    raise SystemExit("--attn_decode=rescore needs --enable_ctc=True (the first pass reads the CTC head)")
  if f.get("ctc_decoder") != "beam":
    raise SystemExit("--attn_decode=rescore needs --ctc_decoder=beam (the first pass is the CTC beam search)")
  if f.get("ctc_only"):
    raise SystemExit("--attn_decode=rescore needs the attention decoder: not with --ctc_only=True")
  for name, on in (("stream_lookahead", int(-1 if f.get("stream_lookahead") is None else f["stream_lookahead"]) >= 0),
                   ("stream_tfm", bool(f.get("stream_tfm"))), ("stream_frontend", bool(f.get("stream_frontend")))):
    if on:
      raise SystemExit("--attn_decode=rescore does not go with --%s: only the causal RNN session (--stream_encoder=True) "
                       "hands the decoder a final state" % name)


def stream_encoder_check(f):
  """--stream_encoder needs what an encoder session can run: SystemExit otherwise."""
  if not f.get("stream_encoder"):
    return
  if not int(f.get("stream_chunk") or 0) > 0:
    raise SystemExit("--stream_encoder needs --stream_chunk>0 (the chunk the encoder is fed in)")
  if f.get("ctc_decoder") != "beam":
    raise SystemExit("--stream_encoder needs --ctc_decoder=beam")
  if f.get("bidirectional"):
    raise SystemExit("--stream_encoder needs --bidirectional=False: a session runs causally")
  if f.get("encoder") != "rnn" or (f.get("frontend") != "none" and not f.get("stream_frontend")):
    raise SystemExit("--stream_encoder needs --encoder=rnn and --frontend=none")


def stream_lookahead_check(f):
  """--stream_lookahead needs what a look-ahead session can run: SystemExit otherwise."""
  n = int(-1 if f.get("stream_lookahead") is None else f.get("stream_lookahead"))
  if n < -1:
    raise SystemExit("--stream_lookahead must be >= 0 (or -1: off)")
  if n < 0:
    return
  if f.get("stream_encoder"):
    raise SystemExit("--stream_lookahead does not go with --stream_encoder=True (the causal session): drop one of them")
  if not int(f.get("stream_chunk") or 0) > 0:
    raise SystemExit("--stream_lookahead needs --stream_chunk>0 (the chunk the encoder is fed in)")
  if f.get("ctc_decoder") != "beam":
    raise SystemExit("--stream_lookahead needs --ctc_decoder=beam")
  if not f.get("enable_ctc") or not f.get("ctc_only"):
    raise SystemExit("--stream_lookahead needs the encoder + CTC loop (--enable_ctc=True --ctc_only=True)")
  if not f.get("bidirectional"):
    raise SystemExit("--stream_lookahead needs --bidirectional=True (a uni-directional encoder streams with "
                     "--stream_encoder=True)")
  if f.get("encoder") != "rnn" or (f.get("frontend") != "none" and not f.get("stream_frontend")):
    raise SystemExit("--stream_lookahead needs --encoder=rnn and --frontend=none")


def stream_frontend_check(f):
  """--stream_frontend needs what a frontend session and the encoder session behind it can run: SystemExit otherwise.
  (With it, --stream_encoder and --stream_lookahead take --frontend=conv3d.)"""
  if not f.get("stream_frontend"):
    return
  if f.get("frontend") != "conv3d":
    raise SystemExit("--stream_frontend needs --frontend=conv3d (the frontend it streams)")
  if f.get("encoder") != "rnn":
    raise SystemExit("--stream_frontend needs --encoder=rnn (there is no session for the transformer encoder)")
  if not int(f.get("stream_chunk") or 0) > 0:
    raise SystemExit("--stream_frontend needs --stream_chunk>0 (the chunk the frontend is fed in)")
  causal = bool(f.get("stream_encoder"))
  ahead = int(-1 if f.get("stream_lookahead") is None else f.get("stream_lookahead")) >= 0
  if causal == ahead:
    raise SystemExit("--stream_frontend needs exactly one of --stream_encoder=True (with --bidirectional=False) or "
                     "--stream_lookahead>=0: the encoder session its features feed")
  if causal and f.get("bidirectional"):
    raise SystemExit("--stream_frontend with --stream_encoder=True needs --bidirectional=False: a session runs causally")


def tfm_chunk_check(f):
  """--tfm_chunk / --tfm_left_chunks / --stream_tfm need the transformer encoder (and the last one what its session and
  the search behind it can run): SystemExit otherwise."""
  chunk, left = int(f.get("tfm_chunk") or 0), int(f.get("tfm_left_chunks") or 0)
  if chunk < 0:
    raise SystemExit("--tfm_chunk must be >= 0 (0: every frame attends to the whole clip)")
  if left < 0:
    raise SystemExit("--tfm_left_chunks must be >= 0")
  if chunk and f.get("encoder") != "transformer":
    raise SystemExit("--tfm_chunk needs --encoder=transformer (the attention it limits)")
  if left and f.get("encoder") != "transformer":
    raise SystemExit("--tfm_left_chunks needs --encoder=transformer (the attention it limits)")
  if left and not chunk:
    raise SystemExit("--tfm_left_chunks needs --tfm_chunk>0 (the chunks it counts)")
  if not f.get("stream_tfm"):
    return
  if f.get("encoder") != "transformer":
    raise SystemExit("--stream_tfm needs --encoder=transformer (the encoder it streams)")
  if not chunk:
    raise SystemExit("--stream_tfm needs --tfm_chunk>0: a full-attention model cannot be cached")
  if not int(f.get("stream_chunk") or 0) > 0:
    raise SystemExit("--stream_tfm needs --stream_chunk>0 (the pieces the encoder is fed in)")
  if f.get("ctc_decoder") != "beam":
    raise SystemExit("--stream_tfm needs --ctc_decoder=beam")


def _cer(correct, count):
  return float(count - correct) / count if count else 1.0


def make_error_of(f, encoder, decoding_step, ctc_decoder, device, char2idx):
  """The driver's error measure for a loader, by the flags `f`.  With --score=device the edit-distance errors are
  scored on the GPU (train.device_scores: the same floats) and `error_of.last_scores` holds the latest call's dict
  (cer, wer, ...); the teacher-forced mismatch rate is not an edit distance and is untouched."""
  from . import train as T
  on_device = f.get("score", "host") == "device"
  with_lm = {}   # the keyword reaches the searches only with a model
  if f.get("attn_lm_path") and decoding_step is not None and f["attn_decode"] in ("beam", "joint"):
    from .decoder import ctc_labels
    from .lm import WordLM
    with_lm = dict(lm=WordLM(f["attn_lm_path"], ctc_labels(char2idx), alpha=f["attn_lm_alpha"], beta=f["attn_lm_beta"]))

  def scored(loader, **how):
    error_of.last_scores = T.device_scores(encoder, loader, device, char2idx, **how)
    return error_of.last_scores["cer"]

  def error_of(loader):
    """The live loop's "CER" is the sampled-token mismatch rate of the attention decoder (train.py:287-288
    via eval's correct/count), or with --attn_decode=beam the edit-distance CER of its beam-search transcripts
    (--attn_decode=joint: of the joint CTC/attention beam search's; --attn_decode=rescore: of the CTC beam search's
    N-best rescored by the decoder);
    without a decoder it is the greedy-decoded CER of the CTC head (decoder.py:64-73 on :182-197, as
    archive/train_model.py:351-357 composes them), or the beam-decoded one with --ctc_decoder=beam."""
    if on_device and decoding_step is None:
      return scored(loader, decoder=ctc_decoder)
    if decoding_step is not None and f["attn_decode"] == "rescore":
      how = dict(ctc_weight=f["attn_ctc_weight"], length_bonus=f["attn_length_bonus"])
      if on_device:
        return scored(loader, decoder=ctc_decoder, decoding_step=decoding_step,
                      rescore_nbest=f["attn_rescore_nbest"], **how)
      return T.rescored_cer(encoder, decoding_step, loader, device, char2idx, ctc_decoder,
                            nbest=f["attn_rescore_nbest"], **how)
    if on_device and f["attn_decode"] in ("beam", "joint"):
      return scored(loader, decoding_step=decoding_step, beam_width=f["attn_beam_width"],
                    max_label_len=f["attn_max_label_len"],
                    ctc_weight=f["attn_ctc_weight"] if f["attn_decode"] == "joint" else 0.0, **with_lm)
    if decoding_step is None:
      if ctc_decoder is not None:
        return T.ctc_cer(encoder, loader, device, char2idx, ctc_decoder)
      return T.greedy_cer(encoder, loader, device, char2idx)
    if f["attn_decode"] == "beam":
      return T.attention_cer(encoder, decoding_step, loader, device, char2idx, beam_width=f["attn_beam_width"],
                             max_label_len=f["attn_max_label_len"], **with_lm)
    if f["attn_decode"] == "joint":
      return T.attention_cer(encoder, decoding_step, loader, device, char2idx, beam_width=f["attn_beam_width"],
                             max_label_len=f["attn_max_label_len"], ctc_weight=f["attn_ctc_weight"], **with_lm)
    _, correct, count, _ = T.eval(encoder, decoding_step, loader, device, char2idx)
    return _cer(correct, count)
  error_of.last_scores = None
  return error_of


def run(**flags):
  """The training loop of train.py:134-320 on one MI355X.  Returns a summary dict."""
  from . import train as T
  from .data import make_collate_fn
  from .dataset import FrameCaptionDataset, make_loader, split_dataset
  from .optim import FlatParameters, FusedAdam
  f = dict(DEFAULTS)
  f.update(flags)
  augment = augment_spec(f)
  lmk_augment = lmk_augment_spec(f)
  crop_check(f)
  lmk_pose_check(f)
  if f["frontend"] != "none" or f["encoder"] != "rnn":
    # the build-defined regimes are encoder + CTC with greedy CER (parse_flags sets the same for flag files)
    f["enable_ctc"], f["ctc_only"] = flags.get("enable_ctc", True), flags.get("ctc_only", True)
  align_check(f)
  spot_check(f)
  segment_check(f)
  mwer_check(f)
  transducer_check(f)
  stream_frontend_check(f)
  stream_encoder_check(f)
  stream_lookahead_check(f)
  tfm_chunk_check(f)
  attn_rescore_check(f)
  torch.manual_seed(f["seed"])
  rand = np.random.RandomState(seed=f["seed"])
  assert torch.cuda.is_available(), "the driver runs the HIP path: an MI355X is required (no CPU fallback)"
  device = torch.device("cuda")
  if not f["cuda"]:
    print("note: --cuda=False is ignored: this build has no CPU execution path")
  print("Initializing dataset '{}'".format(f["data"]))
  splits = split_dataset(f["root"], f["data"], f["train_split"], rand=rand)
  pixels = f["frontend"] == "conv3d"
  sets = [FrameCaptionDataset(f["root"], f["data"], name, ids, labels=f["labels"],
                              threshold=f["occlussion_threshold"], sentence_dataset=f["sentence_dataset"],
                              refresh=f["refresh"], pixels=pixels)
          for name, ids in zip(("train", "val", "test"), splits)]
  char2idx = sets[0].char2idx
  pose = None
  if pixels:
    # u8 frames + landmarks -> mouth crops (B, Tmax, 3, S, S) on the GPU (lr_lip_crop_u8)
    from .data import make_pixel_collate_fn
    collate = make_pixel_collate_fn(device, size=f["crop_size"], crop=f["crop"], extent=f["crop_extent"],
                                    radius=f["crop_smooth"])
    if f["crop"] != "box":
      print("Mouth crops: %s (extent %g eye distances, smoothed over %d frames)" %
            (f["crop"], f["crop_extent"], 2 * f["crop_smooth"] + 1))
  else:
    pose = lmk_pose_spec(f, sets[0], device)
    # padded on the GPU (lr_collate_pad_f32, or lr_lmk_pose_collate_f32 with --lmk_pose); lengths stay on the host
    collate = make_collate_fn(device, pose=pose) if pose is not None else make_collate_fn(device)
  # only the train loader is augmented; validation and test clips are served as they are.  The crop and the landmark
  # pose are one for all three
  train_loader, val_loader, test_loader = (make_loader(d, f["batch_size"], collate, prefetch=f["prefetch"], device=device,
                                                       pixels=pixels, size=f["crop_size"], crop=f["crop"],
                                                       extent=f["crop_extent"], radius=f["crop_smooth"], pose=pose,
                                                       augment=augment if d is sets[0] else None,
                                                       lmk_augment=lmk_augment if d is sets[0] else None) for d in sets)
  if augment is not None:
    print("Augmenting the training clips: %s (seed %d)" % (augment, augment.seed))
  if lmk_augment is not None:
    print("Augmenting the training landmarks: %s (seed %d)" % (lmk_augment, lmk_augment.seed))
  print("Initializing model")
  ctc_only = bool(f["ctc_only"])
  if pixels or f["encoder"] == "transformer":
    assert ctc_only and f["enable_ctc"], "--frontend=conv3d / --encoder=transformer run the encoder+CTC loop"
    encoder, decoding_step = init_pixel_model(char2idx, f, device), None
  else:
    encoder, decoding_step = init_models(char2idx, f["num_layers"], f["frame_dim"], f["hidden_size"], f["char_dim"],
                                         f["enable_ctc"], f["rnn_type"], f["attention_type"], f["attn_hidden_size"],
                                         f["bidirectional"], f["rnn_dropout"], device)
  if ctc_only:
    assert f["enable_ctc"], "--ctc_only needs --enable_ctc"
    decoding_step = None
    flats = (FlatParameters(encoder),)
  else:
    flats = (FlatParameters(encoder), FlatParameters(decoding_step))
  weights_dir = weights_path(f["root"], f["data"])
  encoder_path = os.path.join(weights_dir, "best_encoder.pth")
  decoder_path = os.path.join(weights_dir, "best_decoder.pth")

  ctc_decoder = None
  two_pass = decoding_step is not None and f["attn_decode"] == "rescore"   # the first pass is the CTC beam search
  if (ctc_only or two_pass) and f["ctc_decoder"] == "beam":
    from .decoder import BeamCTCDecoder, ctc_labels
    labels = ctc_labels(char2idx)
    ctc_decoder = BeamCTCDecoder(labels, lm_path=f["lm_path"] or None, alpha=f["lm_alpha"],
                                 beta=f["lm_beta"], beam_width=f["beam_width"], blank_index=0,
                                 log_probs_input=True,
                                 hotwords=[w for w in f["hotwords"].split(",") if w] or None,
                                 hotword_weight=f["hotword_weight"], hotword_anchor=" " in labels)

  chunked = None
  if ctc_decoder is not None and f["stream_chunk"]:
    from .decoder import ChunkedBeamDecoder
    chunked = ChunkedBeamDecoder(ctc_decoder, f["stream_chunk"])
  eval_encoder = encoder
  if f["stream_encoder"]:
    if chunked is None or (decoding_step is not None and not two_pass):
      raise SystemExit("--stream_encoder needs the encoder + CTC loop (--enable_ctc=True --ctc_only=True) or "
                       "--attn_decode=rescore")
    if not f["stream_frontend"]:
      from .encoder_stream import ChunkedEncoder
      eval_encoder = ChunkedEncoder(encoder, f["stream_chunk"])
  if f["stream_lookahead"] >= 0:
    if chunked is None or decoding_step is not None:
      raise SystemExit("--stream_lookahead needs the encoder + CTC loop (--enable_ctc=True --ctc_only=True)")
    if not f["stream_frontend"]:
      from .encoder_lookahead import ChunkedLookaheadEncoder
      eval_encoder = ChunkedLookaheadEncoder(encoder, f["stream_chunk"], f["stream_lookahead"])
  if f["stream_frontend"]:
    from .frontend_stream import ChunkedPixelLipReader
    eval_encoder = ChunkedPixelLipReader(encoder, f["stream_chunk"],
                                         lookahead=f["stream_lookahead"] if f["stream_lookahead"] >= 0 else None)
  if f["stream_tfm"]:
    if chunked is None or decoding_step is not None:
      raise SystemExit("--stream_tfm needs the encoder + CTC loop (--enable_ctc=True --ctc_only=True)")
    from .transformer_stream import ChunkedTransformerEncoder, ChunkedTransformerPixelLipReader
    eval_encoder = (ChunkedTransformerPixelLipReader(encoder, f["stream_chunk"]) if pixels
                    else ChunkedTransformerEncoder(encoder, f["stream_chunk"]))
  error_of = make_error_of(f, eval_encoder, decoding_step, chunked or ctc_decoder, device, char2idx)
  head, head_path = None, os.path.join(weights_dir, "best_transducer.pth")
  if f["transducer"]:
    from .transducer import TransducerHead
    inner = getattr(encoder, "encoder", encoder)   # (PixelLipReader wraps the sequence encoder)
    enc_dim = inner.d_model if hasattr(inner, "d_model") else inner.num_dirs * inner.hidden_size
    head = TransducerHead(enc_dim, len(char2idx), char2idx, joint_dim=f["transducer_joint"],
                          embed_dim=f["transducer_embed"], context=f["transducer_context"]).to(device)
    flats = flats + (FlatParameters(head),)
    # an edit-distance CER of free-running transcripts can exceed 1 (insertions): the first epoch's pair is kept whatever
    # it scores, and replaced only by a better one
    encoder.best_error = head.best_error = float("inf")
    print("Transducer head: joint width %d, label embedding %d, %d characters of context, CTC weight %g"
          % (f["transducer_joint"], f["transducer_embed"], f["transducer_context"], f["transducer_ctc_weight"]))

    def error_of(loader):
      """The CER of the transducer's greedy transcripts, or of its beam search's top hypotheses."""
      return T.transducer_cer(encoder, head, loader, device, char2idx, max_symbols=f["transducer_max_symbols"],
                              beam_width=f["transducer_beam"])
    error_of.last_scores = None

  def validation_error():
    """error_of(val_loader); with --stream_chunk also the pass's commit delay, printed and returned."""
    if chunked is None:
      return error_of(val_loader), None
    chunked.commit_delay()   # what the passes since the last validation left
    cer = error_of(val_loader)
    delay = chunked.commit_delay()
    streamed = " (encoder streamed)" if f["stream_encoder"] else ""
    if f["stream_lookahead"] >= 0:
      streamed = " (encoder streamed: adds %d frames of look-ahead latency)" % f["stream_lookahead"]
    if f["stream_frontend"]:
      streamed = streamed[:-1] + "; frontend streamed: adds 3 frames of latency)"
    if f["stream_tfm"]:
      streamed = " (encoder streamed: adds up to %d frames of look-ahead latency%s)" % (
          f["tfm_chunk"] - 1, "; frontend streamed: adds 3 frames of latency" if pixels else "")
    if delay["chars"]:
      print("\tCommit delay (chunks of %d frames): mean %.2f frames, p90 %d, %.1f%% of %d characters only at the end%s"
            % (f["stream_chunk"], delay["mean"], delay["p90"], 100.0 * delay["end_share"], delay["chars"], streamed))
    else:
      print("\tCommit delay (chunks of %d frames): no characters decoded%s" % (f["stream_chunk"], streamed))
    return cer, delay
  mwer = None
  if f["mwer"]:
    from .mwer import MWERLoss
    mwer = MWERLoss(ctc_decoder, nbest=f["mwer"], unit=f["mwer_unit"], with_reference=f["mwer_reference"])
    print("Training on the expected %s edit distance over %d beam hypotheses%s (CTC weight %g)"
          % (f["mwer_unit"], f["mwer"], " and the reference" if f["mwer_reference"] else "", f["mwer_ctc_weight"]))

  opt =tuple(FusedAdam(fl, lr=f["learning_rate"]) for fl in flats)
  if pixels and hasattr(encoder, "encoder"):
    # (single process, one backward per step: the sequence encoder's share of the clip's sum of squares is taken beside
    # the conv backward, optim.FusedAdam.sum_squares_early)
    opt[0].sum_squares_early(encoder.encoder)
  # the step of every batch shape (B, Tmax, Lmax) is captured once as a hipGraph and replayed — in the landmark
  # regimes, whose steps are launch-bound (0.4-2 ms of 14-100 short launches).  The pixel regimes' steps are GPU-bound
  # (~45 launches, 2.3 ms) and replay no faster than eager launches (2.55 against 2.47 ms at the bench shape, bench.py's
  # launch_probe; with six hardware queues the replay is 3.4 ms, lipreading_amd/__init__.py): eager there.
  graphs = T.StepGraphs(enabled=bool(f["step_graphs"]) and not pixels)

  print("Initial evaluation...")
  val_cer, commit = validation_error()
  print("\tCER: ", val_cer)
  best_val_cer, best_idx = 1.0, -1
  lr = f["learning_rate"]
  epochs, annealings = 0, 0
  history = []
  t0 = time.time()
  print("Beginning training loop")
  while val_cer < best_val_cer or annealings < f["annealings"]:
    if f["max_epochs"] is not None and epochs >= f["max_epochs"]:
      break
    print("Epoch {}:".format(epochs + 1))
    if epochs - best_idx > f["patience"]:
      annealings += 1
      lr /= 5
      print(f'\tAnnealing to {lr}')
      if os.path.isfile(encoder_path):
        restore(encoder, encoder_path)
        if not ctc_only:
          restore(decoding_step, decoder_path)
        if head is not None and os.path.isfile(head_path):
          restore(head, head_path)
      best_idx = epochs
    tfr = max(f["min_tfr"], f["max_tfr"] - epochs / f["tr_epochs"])
    assert 0.0 <= tfr <= 1.0
    print(f'\tCurrent Teacher Forcing Ratio: {tfr}')
    for o in opt:
      o.reset(lr)     # what re-creating Adam every epoch does (:275-276): moments and step count start over
    expected_risk = None
    if mwer is not None:
      expected_risk, ctc_loss = T.train_mwer(encoder, train_loader, opt[0], device, char2idx, mwer,
                                             grad_norm=f["grad_norm"], ctc_weight=f["mwer_ctc_weight"])
      dec_loss = 0.0
      print(f'\tAVG Expected Risk: {expected_risk}')
    elif head is not None:
      transducer_loss, ctc_loss = T.train_transducer(encoder, head, train_loader, opt, device, char2idx,
                                                     grad_norm=f["grad_norm"], ctc_weight=f["transducer_ctc_weight"])
      dec_loss = 0.0
      print(f'\tAVG Transducer Loss: {transducer_loss}')
    else:
      dec_loss, ctc_loss = T.train(encoder, decoding_step, train_loader, opt[0] if ctc_only else opt, device, char2idx,
                                   teacher_forcing_ratio=tfr, grad_norm=f["grad_norm"], graphs=graphs)
    print(f'\tAVG Decoder Loss: {dec_loss}')
    print(f'\tAVG CTC Loss: {ctc_loss}')
    val_cer, commit = validation_error()
    val_scores = error_of.last_scores   # (--score=device: the validation pass's dict, before the next pass replaces it)
    clean = augment is None and lmk_augment is None
    train_cer = error_of(train_loader if clean else train_loader.plain())   # on clean clips
    encoder.save_best_model(val_cer, encoder_path)
    if head is not None:
      head.save_best_model(val_cer, head_path)
    if not ctc_only:
      decoding_step.save_best_model(val_cer, decoder_path)
    test_cer = error_of(test_loader)
    print(f'\tTrain CER: {train_cer}')
    print(f'\tVal CER: {val_cer}')
    print(f'\tTest CER: {test_cer}')
    stats = T.last_epoch_stats or {}
    history.append(dict(epoch=epochs, decoder_loss=dec_loss, ctc_loss=ctc_loss, train_cer=train_cer,
                        val_cer=val_cer, test_cer=test_cer, lr=lr, tfr=tfr,
                        # batches that updated nothing (the reference's `continue`, train_better_model.py:49-50) and how
                        # many of them because a one-launch recurrence timed out
                        skipped_batches=stats.get("skipped", 0), recurrence_faults=stats.get("recurrence_faults", 0)))
    if expected_risk is not None:
      history[-1]["expected_risk"] = expected_risk
    if head is not None:
      history[-1]["transducer_loss"] = transducer_loss
      print(f'\tTransducer CER (val): {val_cer}')
    if val_scores is not None:
      history[-1]["val_wer"] = val_scores["wer"]
      print(f'\tVal WER: {val_scores["wer"]}')
    if commit is not None:
      history[-1]["commit_delay"] = commit
    if val_cer < best_val_cer:   # :339-341
      best_val_cer, best_idx = val_cer, epochs
    epochs += 1
  out = dict(history=history, weights_dir=weights_dir, seconds=time.time() - t0, epochs=epochs,
             graph_captures=graphs.captures, graph_replays=graphs.replays, encoder=encoder,
             decoding_step=decoding_step, char2idx=char2idx, loaders=(train_loader, val_loader, test_loader))
  if head is not None:
    out["transducer"] = head
    if os.path.isfile(head_path) and os.path.isfile(encoder_path):
      restore(encoder, encoder_path)   # the pair that scored best, as the annealing restores it
      restore(head, head_path)
    out["transducer_path"] = head_path
  if commit is not None:
    out["commit_delay"] = commit
  if f["align"]:
    out["align"] = write_alignments(f["align"], encoder, val_loader, device, char2idx)
    print("Aligned %(utterances)d validation utterances (%(infeasible)d too short for their caption): %(path)s"
          % out["align"])
  if f["spot"]:
    out["spot"] = write_spots(f["spot"], encoder, val_loader, device, char2idx, read_keywords(f["keywords"]),
                              min_confidence=f["spot_confidence"] or None, max_hits=f["spot_max_hits"])
    print("Spotted %(keywords)d keywords in %(utterances)d validation utterances (%(hits)d hits): %(path)s"
          % out["spot"])
  if f["segment"]:
    out["segment"] = write_segments(f["segment"], encoder, sorted(splits[1]), device, char2idx, f["batch_size"],
                                    collate_fn=collate, pixels=pixels, threshold=f["occlussion_threshold"])
    print("Segmented %(segmented)d of %(videos)d validation videos (%(captions)d captions): %(path)s" % out["segment"])
  return out


def main(argv=None):
  flags = parse_flags(sys.argv[1:] if argv is None else argv)
  out = run(**flags)
  print("done: %d epochs in %.1f s, weights in %s" % (out["epochs"], out["seconds"], out["weights_dir"]))


if __name__ == "__main__":
  main()
