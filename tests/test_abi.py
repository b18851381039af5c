"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol that
include/lipreading_hip.h declares (no compute calls without a GPU); and the binding that _C reads out of
that header agrees with the compiler's own reading of it."""
import ctypes
import json
import os
import re
import subprocess

import pytest

from lipreading_amd import _build, _C, _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
  text = open(os.path.join(ROOT, "include", "lipreading_hip.h")).read()
  text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
  return sorted(set(re.findall(r"\b(lr_[a-z0-9_]+)\s*\(", text)))


def test_library_builds_and_exports_every_declared_symbol():
  path = _build.build_library()
  assert os.path.exists(path)
  lib = _C.lib()
  names = declared_symbols()
  assert len(names) >= 15
  for n in names:
    assert hasattr(lib, n), "header declares %s but the .so does not export it" % n


def test_version_and_status_strings():
  lib = _C.lib()
  assert lib.lr_version() >= 100
  assert lib.lr_status_string(0) == b"ok"
  assert b"workspace" in lib.lr_status_string(-2)
  assert lib.lr_ctc_workspace_bytes(32, 75, 65, 31) == (2 * 32 * 75 * 64 + 32 * 31 + 32 * 65) * 4
  # label length clamped to <= 256 (ctc_loss.py:46): 513 states -> stride 576
  assert lib.lr_ctc_workspace_bytes(1, 10, 65, 300) == (2 * 10 * 576 + 256 + 65) * 4


def test_null_arguments_are_rejected_without_a_device():
  lib = _C.lib()
  assert lib.lr_ctc_reduce(None, None, None, 1, None, None, None, 4, None) == -1
  assert lib.lr_lmk_translate(None, None, None, 1, 68, None) == -1


def test_product_path_has_no_cpu_fallback():
  import torch
  from lipreading_amd.ctc import ctc_loss_with_status
  lp = torch.zeros(2, 5, 65)
  with pytest.raises(_C.LipReadingHipError):
    ctc_loss_with_status(lp, torch.zeros(2, 3, dtype=torch.long), torch.tensor([5, 5]),
                         torch.tensor([3, 3]), "mean")


def test_product_package_never_imports_the_oracle():
  pkg = os.path.join(ROOT, "lipreading_amd")
  for dirpath, _, files in os.walk(pkg):
    for f in files:
      if f.endswith((".py", ".hip", ".h", ".cpp")):
        src = open(os.path.join(dirpath, f)).read()
        assert not re.search(r"^\s*(from|import)\s+oracle\b|import_module\(.oracle|oracle/_ref|lr_oracle",
                             src, flags=re.M), "%s reaches into oracle/" % f


def test_per_unit_compile_flags_name_existing_units_and_reach_the_tools():
  """_build.UNIT_FLAGS (flags of single translation units) must name sources that exist — a typo would silently build
  the unit without them — and the two shell tools that compile a unit on their own (variant libraries for A/B timing,
  the register-usage report) must repeat them, or they would time / report another kernel than the library holds."""
  units = {os.path.splitext(os.path.basename(p))[0] for p in _build.sources()}
  root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
  for unit, flags in _build.UNIT_FLAGS.items():
    assert unit in units, unit
    assert flags and all(isinstance(f, str) for f in flags)
    for tool in ("tools/build_variant.sh", "tools/hip_resources.sh"):
      with open(os.path.join(root, tool)) as f:
        text = f.read()
      assert unit in text and " ".join(flags) in text, (tool, unit)


# ---- the binding against the compiler's reading of the header ------------------------------------------------------

# desugared C types of the x86-64 Linux ABI -> ctypes; written here, not taken from the reader: a second reading
_C_TYPES = {"int": ctypes.c_int, "long": ctypes.c_int64, "unsigned long": ctypes.c_size_t,
            "long long": ctypes.c_longlong, "float": ctypes.c_float, "double": ctypes.c_double, "void": None}
_STRUCT_CLASSES = {"lr_decoder_params": _C.DecoderParams, "lr_decoder_grads": _C.DecoderGrads,
                   "lr_fgemm_job": _C.FgemmJob, "lr_decoder_upper": _C.DecoderUpper,
                   "lr_decoder_upper_grads": _C.DecoderUpperGrads}


def _clang(*args):
  """Output of the clang that belongs to hipcc, run over the header as C.  No clang is a failure: the build needs it."""
  rocm = os.path.dirname(os.path.dirname(os.path.realpath(_build._hipcc())))
  found = [p for p in (os.path.join(rocm, "llvm", "bin", "clang"), os.path.join(rocm, "lib", "llvm", "bin", "clang"))
           if os.path.exists(p)]
  assert found, "no clang beside hipcc under %s" % rocm
  return subprocess.run([found[0], "-x", "c"] + list(args) + [_build.HEADER], check=True, capture_output=True,
                        text=True).stdout


@pytest.fixture(scope="module")
def ast():
  return json.loads(_clang("-fsyntax-only", "-Xclang", "-ast-dump=json"))["inner"]


def _expected(qual, typedefs, ret=False):
  """ctypes class of a C type as the AST spells it, typedefs followed down to the builtin type."""
  qual = qual.strip()
  array = re.fullmatch(r"(.*)\[(\d+)\]", qual)
  if array:
    return _expected(array[1], typedefs) * int(array[2])
  while qual in typedefs:
    qual = typedefs[qual]
  if qual.endswith("*"):
    return ctypes.c_char_p if ret and qual == "const char *" else ctypes.c_void_p
  return _C_TYPES[qual]


def test_prototypes_agree_with_the_compiler(ast):
  typedefs = {n["name"]: n["type"]["qualType"] for n in ast if n["kind"] == "TypedefDecl"}
  functions = [n for n in ast if n["kind"] == "FunctionDecl"]
  assert sorted(f["name"] for f in functions) == sorted(_C.SIGNATURES) and len(functions) >= 124
  for f in functions:
    restype, argtypes = _C.SIGNATURES[f["name"]]
    qual = f["type"]["qualType"]
    assert restype is _expected(qual[:qual.index("(")], typedefs, ret=True), f["name"]
    params = [p for p in f.get("inner", []) if p["kind"] == "ParmVarDecl"]
    assert len(argtypes) == len(params), f["name"]
    for i, (got, p) in enumerate(zip(argtypes, params)):
      assert got is _expected(p["type"]["qualType"], typedefs), (f["name"], i, p["name"], p["type"])


def test_constants_agree_with_the_compiler(ast):
  want = {c["name"]: int(c["inner"][0]["value"]) for e in ast if e["kind"] == "EnumDecl"
          for c in e["inner"] if c["kind"] == "EnumConstantDecl"}
  assert sum(e["kind"] == "EnumDecl" for e in ast) == 4 and "LR_RNN_RECUR_SPLIT" in want
  for line in _clang("-dM", "-E").splitlines():
    m = re.fullmatch(r"#define (LR_\w+) (.*)", line)
    if m:
      value = re.fullmatch(r"\(?(-?\d+)\)?", m[2].strip())
      assert value, "%s is not an integer" % line
      want[m[1]] = int(value[1])
  assert "LR_DEC_MAX_LAYERS" in want and "LR_SPOT_BAD_LENGTH" in want
  assert _C.CONSTANTS == want
  for name, value in want.items():
    assert getattr(_C, name) == value, name


def test_struct_layouts_agree_with_the_compiler(ast):
  """Equal field names and types in equal order: ctypes and the compiler then lay the struct out by the same C rules."""
  typedefs = {n["name"]: n["type"]["qualType"] for n in ast if n["kind"] == "TypedefDecl"}
  records = {n["id"]: n for n in ast if n["kind"] == "RecordDecl"}
  seen = set()
  for n in ast:
    if n["kind"] != "TypedefDecl" or not n["type"]["qualType"].startswith("struct lr_"):
      continue
    owner = n["inner"][0]
    while "decl" not in owner:   # older clangs wrap the RecordType in an ElaboratedType
      owner = owner["inner"][0]
    fields = [f for f in records[owner["decl"]["id"]]["inner"] if f["kind"] == "FieldDecl"]
    assert not any(f.get("isBitfield") for f in fields), n["name"]
    want = [(f["name"], _expected(f["type"]["qualType"], typedefs)) for f in fields]
    assert list(_STRUCT_CLASSES[n["name"]]._fields_) == want, n["name"]
    seen.add(n["name"])
  assert seen == set(_STRUCT_CLASSES)
  assert ctypes.sizeof(_C.DecoderUpper) == 8 + 4 * 7 * 8 + 8 and ctypes.sizeof(_C.FgemmJob) == 8 * 8 + 15 * 4 + 4


# ---- the reader refuses what it does not understand (text only) ------------------------------------------------------

def _header_text():
  with open(_build.HEADER) as f:
    return f.read()


@pytest.mark.parametrize("old, new, named", [
    ("int lr_version(void);", "int lr_version(unsigned short n);", "lr_version"),             # a type outside the list
    ("int lr_version(void);", "int lr_version(void (*done)(int code));", "lr_version"),       # a function pointer
    ("int lr_device_count(void);", "int lr_device_count(int);", "lr_device_count"),           # a parameter with no name
    ("LR_CTC_SUM = 0,", "LR_CTC_SUM,", "lr_ctc_reduction"),                                   # an enumerator with no value
    ("#define LR_DEC_MAX_LAYERS 8\n", "#define LR_DEC_MAX_LAYERS 8\n#define LR_X 1.5\n", "LR_X 1.5"),
    ("  int num_layers;\n", "  int num_layers : 3;\n", "lr_decoder_upper"),                   # a bit-field
    ("int lr_version(void);", "int stray_symbol(int a);\nint lr_version(void);", "stray_symbol"),
])
def test_reader_refuses_what_is_outside_the_dialect(old, new, named):
  text = _header_text()
  assert text.count(old) == 1
  _header.read(text)   # the header itself reads
  with pytest.raises(_header.HeaderError, match=re.escape(named)):
    _header.read(text.replace(old, new))


def test_reader_takes_a_prototype_over_several_lines():
  one = "typedef void* lr_stream_t;\nsize_t lr_f(const float* const* w_host, int64_t n, float eps, lr_stream_t stream);\n"
  three = ("typedef void* lr_stream_t;\nsize_t lr_f(const float* const* w_host, /* HOST array */\n"
           "            int64_t n,   // elements\n            float eps, lr_stream_t stream);\n")
  want = {"lr_f": (ctypes.c_size_t, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p])}
  assert _header.read(one) == (want, {}, {}) and _header.read(three) == _header.read(one)
