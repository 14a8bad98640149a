"""One-off check for the change that derives the ctypes table from include/avt.h: the hand-written SIGNATURES / _RETURNS_I64 of an
earlier revision of _lib.py against _lib.parse_header of the current header, entry by entry.  Pointers compare as "pointer" (the
hand table typed some host arrays POINTER(c_float) / POINTER(c_int32)); scalars and return types compare exactly.  No GPU, no library.

    python tools/compare_abi_tables.py [REV]      (REV: the revision that still has the hand table; default HEAD~)
"""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIB_PY = "audio-video-textures_amd/_lib.py"


def kind(t):
    return "pointer" if t in (C.c_void_p, C.c_char_p) or hasattr(t, "contents") else t


def main():
    rev = sys.argv[1] if len(sys.argv) > 1 else "HEAD~"
    old = {"__file__": os.path.join(ROOT, LIB_PY), "__name__": "old_lib"}
    exec(subprocess.check_output(["git", "-C", ROOT, "show", "%s:%s" % (rev, LIB_PY)], text=True), old)
    import avtex

    with open(avtex._lib.HEADER_PATH) as f:
        new = avtex._lib.parse_header(f.read())
    diffs = []
    for name, argtypes in old["SIGNATURES"].items():
        ret = C.c_int64 if name in old["_RETURNS_I64"] else C.c_int
        if name not in new:
            diffs.append("%s: not parsed" % name)
        elif (ret, [kind(t) for t in argtypes]) != (new[name][0], [kind(t) for t in new[name][1]]):
            diffs.append("%s: hand %s %s, parsed %s %s" % (name, ret.__name__, [getattr(kind(t), "__name__", kind(t)) for t in argtypes],
                                                          new[name][0].__name__, [getattr(kind(t), "__name__", kind(t)) for t in new[name][1]]))
    extra = sorted(set(new) - set(old["SIGNATURES"]))
    print("\n".join(diffs + ["%s: %d hand-written entries (%d returning int64_t) against %d parsed, %d differences; parsed only: %s"
                             % (rev, len(old["SIGNATURES"]), len(old["_RETURNS_I64"]), len(new), len(diffs), ", ".join(extra) or "none")]))
    return 1 if diffs else 0


if __name__ == "__main__":
    sys.exit(main())
