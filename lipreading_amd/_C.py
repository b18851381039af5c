"""ctypes binding of include/lipreading_hip.h, read from the header itself at import (_header.py).

A new entry point, constant or struct field is written in the header (and the .hip file) and nowhere else.

The product path has no CPU fallback: if the shared object is missing or a kernel reports an
error, the call raises.  Nothing in this module imports from oracle/.
"""
import ctypes
import os
from ctypes import c_float, c_int  # noqa: F401  (what callers compare the entries of SIGNATURES with)

from . import _build
from ._header import P, read  # noqa: F401  (P: every device pointer crosses the boundary as void*)

_lib = None

with open(_build.HEADER) as _f:
  # SIGNATURES: name -> (restype, argtypes);  CONSTANTS: every enumerator and #define LR_*, also module attributes
  # (LR_OK, LR_ERR_*, LR_SPOT_MAX_T, ...);  _STRUCTS: typedef name -> _fields_
  SIGNATURES, CONSTANTS, _STRUCTS = read(_f.read())
globals().update(CONSTANTS)


def _struct(name, typedef):
  return type(name, (ctypes.Structure,), {"_fields_": _STRUCTS[typedef],
                                          "__doc__": "%s (include/lipreading_hip.h)." % typedef})


DecoderParams = _struct("DecoderParams", "lr_decoder_params")
DecoderGrads = _struct("DecoderGrads", "lr_decoder_grads")
FgemmJob = _struct("FgemmJob", "lr_fgemm_job")
DecoderUpper = _struct("DecoderUpper", "lr_decoder_upper")              # layers 1.. of the decoder's RNN stack
DecoderUpperGrads = _struct("DecoderUpperGrads", "lr_decoder_upper_grads")


class LipReadingHipError(RuntimeError):
  pass


def lib_path():
  # LIPREADING_HIP_LIB: another build of the same C ABI (A/B timing of kernel variants: tools/build_variant.sh)
  return os.environ.get("LIPREADING_HIP_LIB") or _build.LIB_PATH


def lib():
  """Load (once) and return the C-ABI library.  Raises if it has not been built."""
  global _lib
  if _lib is None:
    path = lib_path()
    if not os.path.exists(path):
      raise LipReadingHipError(
          "%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
          "(there is no CPU fallback for the MI355X hot path)" % path)
    # torch bundles its own libamdhip64.so.7; load it FIRST so that this library binds to the
    # same HIP runtime instance that owns torch's streams and allocations.  (Loaded the other
    # way round, /opt/rocm's runtime and torch's coexist and every launch on a torch stream
    # fails with an invalid-handle error.)
    import torch  # noqa: F401
    handle = ctypes.CDLL(path)
    for name, (restype, argtypes) in SIGNATURES.items():
      fn = getattr(handle, name)  # AttributeError if the header and the .so disagree
      fn.restype = restype
      fn.argtypes = argtypes
    _lib = handle
    if torch.cuda.is_available():
      handle.lr_fault_words_ptr()   # allocate the device-side fault words now, outside any stream capture
  return _lib


def check(status, what=""):
  if status != 0:
    msg = lib().lr_status_string(int(status)).decode()
    raise LipReadingHipError("%s failed: %s (%d)" % (what or "lipreading_hip call", msg, status))


def stream_handle():
  """hipStream_t of torch's current stream as an integer (void*)."""
  import torch
  return torch.cuda.current_stream().cuda_stream


def ptr(t):
  """Device pointer of a tensor (None -> NULL)."""
  return None if t is None else t.data_ptr()


def require_cuda(*tensors):
  for t in tensors:
    if t is not None and not t.is_cuda:
      raise LipReadingHipError(
          "lipreading_amd ops run on the MI355X only; got a %s tensor (no CPU fallback)" % t.device)
