"""Reader of include/lipreading_hip.h: the header's text -> what _C binds (prototypes, constants, structs).

The header is this project's own and keeps to a narrow dialect.  The reader understands that dialect
only: whatever else it meets raises HeaderError with the declaration in the message.  Nothing is guessed or skipped.
"""
import ctypes
import re

P = ctypes.c_void_p  # every pointer crosses the boundary as void*
SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
           "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double,
           "long long": ctypes.c_longlong, "lr_stream_t": P}

_INT = r"-?(?:0[xX][0-9a-fA-F]+|\d+)"
_DEFINE = re.compile(r"#define (LR_\w+) (?:(%s)|\((-\d+)\))" % _INT)
_IGNORED = re.compile(r'#include <\w+\.h>|#ifdef __cplusplus|#ifndef \w+_H|#define \w+_H|#endif')
_DECL = re.compile(r"\s*((?:[^;{}]|\{[^{}]*\})*);")               # up to a ';' outside braces
_POINTER = re.compile(r"(?:const )?[A-Za-z_]\w*(?:\*(?:const)?)+")  # T*, const T*, T* const*, struct pointers
_NAMED = re.compile(r"([^,:()\[\]]*[\s*])(\w+)")                   # `type name`
_FIELD = re.compile(r"([^,:()\[\]]*[\s*])(\w+(?: ?, ?\w+)*)(?:\[([\w\s+*()-]+)\])?")


class HeaderError(ValueError):
  pass


def _ctype(t, decl, ret=False):
  t = re.sub(r"\s*\*\s*", "*", t.strip())
  if ret and t in ("void", "const char*"):
    return None if t == "void" else ctypes.c_char_p
  if t in SCALARS:
    return SCALARS[t]
  if _POINTER.fullmatch(t):
    return P
  raise HeaderError("type %r is outside the header's dialect in: %s" % (t, decl))


def _fields(body, consts, decl):
  *fields, rest = body.split(";")
  out = []
  for f in fields + ([rest] if rest.strip() else []):
    m = _FIELD.fullmatch(f.strip())
    if not m or (m[3] and "," in m[2]):
      raise HeaderError("field %r is neither `type a, b;` nor `type a[N];` in: %s" % (f.strip(), decl))
    t = _ctype(m[1], decl)
    if m[3]:
      try:
        t = t * int(eval(m[3], {"__builtins__": {}}, dict(consts)))   # names, integers, + - * ( ) only
      except Exception as e:
        raise HeaderError("array length %r (%s) in: %s" % (m[3], e, decl))
    out += [(n.strip(), t) for n in m[2].split(",")]
  return out


def read(text):
  """Header text -> (prototypes {name: (restype, [argtypes])}, constants {name: int}, structs {name: [(field, ctype)]})."""
  protos, consts, structs, code = {}, {}, {}, []
  for line in re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S).split("\n"):
    d = " ".join(line.split())
    m = _DEFINE.fullmatch(d)
    if not d.startswith("#"):
      code.append(line)
    elif m:
      consts[m[1]] = int(m[2] or m[3], 0)
    elif not _IGNORED.fullmatch(d):
      raise HeaderError("directive outside the header's dialect: %s" % d)
  body = "\n".join(code)
  m = re.fullmatch(r'\s*extern "C" \{(.*)\}\s*', body, flags=re.S)
  body = m[1] if m else body
  for decl in _DECL.findall(body):
    d = " ".join(decl.split())
    enum = re.fullmatch(r"typedef enum (\w+) \{ ?(.*?) ?\} \1", d)
    struct = re.fullmatch(r"typedef struct (?:(\w+) )?\{ ?(.*?) ?\} (\w+)", d)
    proto = re.fullmatch(r"(.*[\s*])(lr_\w+) ?\((.*)\)", d)
    if d == "typedef void* lr_stream_t":
      continue
    if enum:
      for e in enum[2].split(","):
        m = re.fullmatch(r"(\w+) ?= ?(%s)" % _INT, e.strip())
        if not m:
          raise HeaderError("enumerator %r has no explicit integer value in: %s" % (e.strip(), d))
        consts[m[1]] = int(m[2], 0)
    elif struct and struct[1] in (None, struct[3]):
      structs[struct[3]] = _fields(struct[2], consts, d)
    elif proto and not d.startswith("typedef"):
      args = []
      for p in ([] if proto[3].strip() == "void" else proto[3].split(",")):
        m = _NAMED.fullmatch(p.strip())
        if not m:
          raise HeaderError("parameter %r is not `type name` in: %s" % (p.strip(), d))
        args.append(_ctype(m[1], d))
      protos[proto[2]] = (_ctype(proto[1], d, ret=True), args)
    else:
      raise HeaderError("declaration outside the header's dialect: %s" % d)
  left = _DECL.sub("", body).strip()
  if left:
    raise HeaderError("text outside the header's dialect: %s" % left[:200])
  return protos, consts, structs
