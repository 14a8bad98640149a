"""ctypes loader of the gfx950 C-ABI library (include/avt.h).

The ABI is written down once, in the header: every csrc/*.hip includes it, so the compiler holds the definitions to it, and the
ctypes table (SIGNATURES) and the version (ABI_VERSION) here are parsed from it (parse_header, abi_version) — a declaration the
parser cannot read, a name declared twice or a missing version is an error, never a default conversion.

There is no CPU fallback: if libavt_hip.so is missing or a call fails, the
product path raises.  Build it with `python -c "import __graft_entry__ as g; g.build()"`
or `make -C audio-video-textures_amd/csrc`.
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
# AVT_HIP_LIB selects another build of the same ABI (the diagnostic libavt_hip_stamp.so of `make stamp`); default = the product
LIB_PATH = os.environ.get("AVT_HIP_LIB") or os.path.join(_HERE, "libavt_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "avt.h")


class AvtError(RuntimeError):
    pass


_SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}
_DECL = re.compile(r"\b(int|int64_t|const\s+char\s*\*)\s*\b(avt_[a-z0-9_]+)\s*\(([^()]*)\)\s*;")


def _ctype(decl, name):
    """One declared type, with or without the parameter's name, as ctypes passes it: a pointer or array is an address (char*: a
    string), a scalar must be one of _SCALARS."""
    words = [w for w in decl.replace("*", " * ").replace("[", " [").split() if w != "const"]
    if any(w[0] in "*[" for w in words):
        return C.c_char_p if words[0] == "char" else C.c_void_p
    if not 1 <= len(words) <= 2 or words[0] not in _SCALARS:
        raise AvtError("include/avt.h: %s has a parameter `%s` whose type this binding does not know" % (name, decl.strip()))
    return _SCALARS[words[0]]


def parse_header(text):
    """The text of include/avt.h -> {name: (restype, [argtypes])} for every avt_* function it declares.  Raises AvtError for a
    parameter type outside the ABI's vocabulary, for a name declared twice, and for any avt_* name followed by `(` that is not a
    declaration it has read."""
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    code = re.sub(r"^[ \t]*#.*$", "", code, flags=re.M)
    table = {}
    for ret, name, params in _DECL.findall(code):
        if name in table:
            raise AvtError("include/avt.h: %s is declared twice" % name)
        params = [] if params.strip() in ("", "void") else params.split(",")
        table[name] = (_ctype(ret, name), [_ctype(p, name) for p in params])
    unread = set(re.findall(r"\b(avt_[a-z0-9_]+)\s*\(", code)) - set(table)
    if unread:
        raise AvtError("include/avt.h: cannot read the declaration of %s" % ", ".join(sorted(unread)))
    return table


def abi_version(text):
    """The header's `#define AVT_ABI_VERSION n` -> n; a header without it is an AvtError."""
    m = re.search(r"^[ \t]*#[ \t]*define[ \t]+AVT_ABI_VERSION[ \t]+(\d+)\b", text, flags=re.M)
    if not m:
        raise AvtError("include/avt.h: no #define AVT_ABI_VERSION")
    return int(m.group(1))


with open(HEADER_PATH) as _f:
    _TEXT = _f.read()
_ABI = parse_header(_TEXT)
SIGNATURES = {name: argtypes for name, (_, argtypes) in _ABI.items() if name != "avt_last_error"}  # name -> argtypes
ABI_VERSION = abi_version(_TEXT)

_lib = None


def _bind(fn):
    fn.restype, fn.argtypes = _ABI[fn.__name__]
    return fn


def lib():
    """The loaded library; raises (never falls back) if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AvtError(
                "HIP extension not built: %s is missing. Run `make -C %s` (needs hipcc); "
                "there is no CPU fallback for the hot path." % (LIB_PATH, os.path.join(_HERE, "csrc")))
        handle = C.CDLL(LIB_PATH)
        for name in _ABI:
            if not hasattr(handle, name):
                raise AvtError("libavt_hip.so does not export %s: rebuild with `make -C %s`" % (name, os.path.join(_HERE, "csrc")))
            _bind(getattr(handle, name))
        if handle.avt_abi_version() != ABI_VERSION:
            raise AvtError("libavt_hip.so ABI version %d, expected %d: rebuild with `make -C %s`"
                           % (handle.avt_abi_version(), ABI_VERSION, os.path.join(_HERE, "csrc")))
        if os.environ.get("AVT_SMALL_TILE", "") == "0":  # (A/Bs: the training convolutions' 64-row tile at small batches off)
            handle.avt_conv_x3_set_small_tile(0)
        if os.environ.get("AVT_WGRAD_ROUNDS", "") == "0":  # (A/Bs: the weight gradient's round-aware split over positions off)
            handle.avt_wgrad_x3_set_xl(7)
        _lib = handle
    return _lib


def _failure(what, status):
    msg = lib().avt_last_error()
    return AvtError("%s failed (%d): %s" % (what, status, msg.decode() if msg else "?"))


def check(status, what):
    if status != 0:
        raise _failure(what, status)


def _errcheck(status, fn, args):
    if status != 0:
        raise _failure(fn.__name__, status)
    return status


class _Checked:
    """The same library, for the entries that return an AVT_* status: checked.avt_X(...) is avt_X with the header's signature that
    raises AvtError (check()'s message, labelled with the entry's own name) on a non-zero status and returns the status otherwise.
    Queries whose return value is an answer (*_supported, *_rows, *_bytes, *_ksize, *_picked, avt_abi_version, the *_set_* switches)
    go through lib().  Each function is a ctypes object of its own, so lib()'s raw entries keep returning the status."""

    def __getattr__(self, name):  # (first use only: the function then sits in the instance's dict)
        if name not in _ABI:
            raise AttributeError(name)
        fn = _bind(lib()[name])
        fn.errcheck = _errcheck
        setattr(self, name, fn)
        return fn


checked = _Checked()
