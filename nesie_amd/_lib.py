"""ctypes binding of ``include/*.h`` (libnesie_hip.so).

This is the binding a maintainer of the reference would write in place of its
pybind11 shims: plain pointers, ints and a stream handle.
The prototypes are READ from the headers at import, so the headers are the only
place an argument list is written down.  The library is looked up in-tree only
(``nesie_amd/libnesie_hip.so``) and a missing or unloadable library -- or a
missing header -- is an ImportError, never a silent fallback.
"""
import ctypes
import glob
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NESIE_LIB") or os.path.join(_HERE, "libnesie_hip.so")
INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), "include")

_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double,
            "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t}
_RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "long long": ctypes.c_longlong,
            "const char *": ctypes.c_char_p}
_PROTOTYPE = re.compile(r"([\w\s\*]+?)\b(nesie_\w+)\s*\(([^()]*)\)")


def _ctype(spelling, name):
    """One parameter (``const float *x``, ``long long p``, ``void *stream``) -> its ctype."""
    if "*" in spelling:
        return ctypes.c_void_p
    words = spelling.split()          # type words, then the parameter's name
    try:
        return _SCALARS[" ".join(words[:-1])]
    except KeyError:
        raise TypeError(f"{name}: no ctypes mapping for the parameter '{spelling}'") from None


def parse_prototypes(text):
    """Every ``RET nesie_name(ARGS);`` of a header's text -> {name: (restype, [argtypes])}.
    A type outside the few the C ABI uses is a TypeError naming the function, never a guess."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*|^\s*#[^\n]*", " ", text, flags=re.M)
    out = {}
    for statement in re.split(r"[;{}]", text):
        m = _PROTOTYPE.fullmatch(" ".join(statement.split()))
        if m is None:
            continue
        ret, name, params = (s.strip() for s in m.groups())
        if ret not in _RETURNS:
            raise TypeError(f"{name}: no ctypes mapping for the return type '{ret}'")
        params = [] if params in ("", "void") else params.split(",")
        out[name] = (_RETURNS[ret], [_ctype(p.strip(), name) for p in params])
    return out


def _read_headers():
    headers = sorted(glob.glob(os.path.join(INCLUDE_DIR, "*.h")))
    if not headers:
        raise ImportError(f"no headers under {INCLUDE_DIR}: the binding is derived from them")
    out = {}
    for h in headers:
        with open(h) as f:
            out.update(parse_prototypes(f.read()))
    return out


# name -> (restype, argtypes) of every function the headers declare (stream last)
SIGNATURES = _read_headers()

_lib = None


def load():
    """Load libnesie_hip.so once and attach argtypes.  Raises ImportError."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (or `make -C nesie_amd/csrc`). nesie_amd has no CPU fallback.")
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the host
        raise ImportError(f"cannot load {LIB_PATH}: {e}") from e
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = restype
    _lib = lib
    return lib


def call(name, *args):
    """Call an entry point that returns a status; non-zero becomes a RuntimeError.  The
    functions that return a size, a count or a flag are reached through ``load()``."""
    if SIGNATURES[name][0] is not ctypes.c_int:
        raise TypeError(f"{name} does not return a status: call it through load()")
    lib = load()
    status = getattr(lib, name)(*args)
    if status != 0:
        msg = lib.nesie_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{name} failed (status {status}): {msg}")


def library_sha256():
    """sha256 of the library file ``load()`` maps (bench.py ties the PMC traffic figures under
    profiles/ to the build that produced them with it)."""
    import hashlib
    h = hashlib.sha256()
    with open(LIB_PATH, 'rb') as f:
        for chunk in iter(lambda: f.read(1 << 20), b''):
            h.update(chunk)
    return h.hexdigest()
