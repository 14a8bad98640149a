"""The C-ABI library loads on a box without a GPU and exports every symbol include/avt.h declares, and no avt_* function besides; the
ctypes binding table and the ABI version are parsed from the header and cover it one to one; every entry recorded in
tests/golden/abi_entries.txt keeps its signature; host-only entry points behave.  No device calls here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch


def _header_functions(path):
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(avt_[a-z0-9_]+)\s*\(", src)))


def _exported_functions(path):
    """Names of the functions an ELF64 little-endian shared library defines in its dynamic symbol table (.dynsym / .dynstr)."""
    import struct

    with open(path, "rb") as f:
        elf = f.read()
    assert elf[:6] == b"\x7fELF\x02\x01", "not a little-endian ELF64 file"
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    # a section header: name u32, type u32, flags u64, addr u64, offset u64, size u64, link u32, info u32, addralign u64, entsize u64
    sections = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + n * shentsize) for n in range(shnum)]
    SHT_DYNSYM, STT_FUNC, SHN_UNDEF = 11, 2, 0
    names = set()
    for _, kind, _, _, offset, size, link, _, _, entsize in sections:
        if kind != SHT_DYNSYM:
            continue
        strtab = sections[link][4]  # .dynstr's file offset
        for at in range(offset, offset + size, entsize):
            st_name, st_info, _, st_shndx = struct.unpack_from("<IBBH", elf, at)  # (then value u64, size u64)
            if st_info & 15 == STT_FUNC and st_shndx != SHN_UNDEF:
                names.add(elf[strtab + st_name:elf.index(b"\0", strtab + st_name)].decode())
    return names


def test_library_exports_every_declared_symbol(avt):
    names = _header_functions(avt._lib.HEADER_PATH)
    assert len(names) >= 14
    handle = ctypes.CDLL(avt._lib.LIB_PATH)
    for n in names:
        assert hasattr(handle, n), "libavt_hip.so does not export %s" % n
    assert sorted(list(avt._lib.SIGNATURES) + ["avt_last_error"]) == names
    # ... and the converse: every avt_* function the library defines is declared (no entry point outside the header)
    exported = sorted(n for n in _exported_functions(avt._lib.LIB_PATH) if n.startswith("avt_"))
    assert exported == names, sorted(set(exported) ^ set(names))


def test_header_binding_and_library_carry_one_version(avt):
    """The header's #define is the only place the number is written: the binding parses it, the library compiles it in.  A stale library
    (built from another header) is what disagrees in practice."""
    with open(avt._lib.HEADER_PATH) as f:
        text = f.read()
    defined = [int(v) for v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+AVT_ABI_VERSION[ \t]+(\d+)", text, flags=re.M)]
    assert len(defined) == 1
    assert defined[0] == avt._lib.abi_version(text) == avt._lib.ABI_VERSION == avt._lib.lib().avt_abi_version()
    assert defined[0] >= 9
    with pytest.raises(avt._lib.AvtError, match="AVT_ABI_VERSION"):
        avt._lib.abi_version("/* #define AVT_ABI_VERSION in words only */\nint avt_abi_version(void);\n")


def _type_names(restype, argtypes):
    """A signature in the names the binding's vocabulary is written in (c_int64.__name__ itself is the platform's c_long)."""
    C = ctypes
    names = {getattr(C, n): n for n in ("c_int", "c_int64", "c_float", "c_double", "c_size_t", "c_void_p", "c_char_p")}
    return [names[t] for t in [restype] + list(argtypes)]


def test_every_recorded_entry_keeps_its_signature(avt):
    """tests/golden/abi_entries.txt holds one line per entry of include/avt.h — `name restype argtypes...` in ctypes type names, sorted by
    name — written once as `" ".join([name] + _type_names(*sig))` for every (name, sig) of parse_header(include/avt.h); an entry added
    later adds its line.  Every recorded entry must still be declared with exactly that signature: a removed or changed one fails by name."""
    with open(avt._lib.HEADER_PATH) as f:
        table = avt._lib.parse_header(f.read())
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "abi_entries.txt")) as f:
        recorded = [line.split() for line in f.read().splitlines()]
    assert len(recorded) >= 130 and len({r[0] for r in recorded}) == len(recorded)
    for name, *types in recorded:
        assert name in table, "include/avt.h no longer declares %s" % name
        assert _type_names(*table[name]) == types, "%s changed its signature" % name


def test_parsed_signatures_of_each_declaration_shape(avt):
    """The ctypes table is parse_header(include/avt.h): one entry pinned for every shape of declaration the parser has to read."""
    C = ctypes
    i, i64, vp = C.c_int, C.c_int64, C.c_void_p
    with open(avt._lib.HEADER_PATH) as f:
        table = avt._lib.parse_header(f.read())
    assert table["avt_device_check"] == (i, [C.c_char_p, C.c_size_t])
    assert table["avt_logmel_f64"] == (i, [vp, i, i64, vp, i, i, i, vp, i, C.c_double, vp, vp])
    assert table["avt_pw_x3_f32"] == (i, [vp, i, i, vp, vp, vp, vp, i, vp, i, i, i64, i, vp])  # int64_t m: the 12th argument
    assert table["avt_weight_planes_t_f32"] == (i, [vp, i, i, i, vp, i, vp, vp, vp])  # const int32_t* sel: a host array
    assert table["avt_frames_resize_aa_norm_u8"] == (i, [vp, i, i, i, i, vp, vp, vp, vp])  # const float* mean / std: host arrays
    assert table["avt_abi_version"] == (i, [])
    assert table["avt_bn_train_ws_bytes_pre"] == (i64, [i, i, i])
    assert table["avt_last_error"] == (C.c_char_p, [])
    assert table["avt_conv3d_wgrad_x3_det_ws_bytes"] == (i64, [i] * 21)
    assert table["avt_conv3d_wgrad_x3_det_sub_f32"] == (i, [vp, vp, vp] + [i] * 21 + [vp, i64, vp])
    assert table["avt_stem_wgrad_x3_det_ws_bytes"] == (i64, [i] * 7)
    assert table["avt_stem_wgrad_x3_det"] == (i, [vp, vp, vp, vp] + [i] * 7 + [vp, i64, vp])
    assert table["avt_state_job_bytes"] == (i, []) and table["avt_state_copy_multi"] == (i, [vp, vp, i, vp])
    # the atomic entries the deterministic ones mirror: the same arguments, less zero_dw, plus (ws, ws_bytes)
    sub, det = table["avt_conv3d_wgrad_x3_sub_f32"][1], table["avt_conv3d_wgrad_x3_det_sub_f32"][1]
    assert det == sub[:-2] + [vp, i64] + sub[-1:]
    stem, sdet = table["avt_stem_wgrad_x3"][1], table["avt_stem_wgrad_x3_det"][1]
    assert sdet == stem[:-1] + [vp, i64] + stem[-1:]
    assert {n: a for n, (_, a) in table.items() if n != "avt_last_error"} == avt._lib.SIGNATURES
    lib, checked = avt._lib.lib(), avt._lib.checked
    for name in ("avt_pw_x3_f32", "avt_conv3d_wgrad_x3_det_ws_bytes", "avt_state_copy_multi"):  # lib() binds the header's types
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == table[name]
    assert list(checked.avt_stem_wgrad_x3_det.argtypes) == table["avt_stem_wgrad_x3_det"][1]  # ... and so does `checked`
    assert list(checked.avt_state_copy_multi.argtypes) == table["avt_state_copy_multi"][1]
    assert lib.avt_bn_train_ws_bytes_pre.restype is i64 and lib.avt_last_error.restype is C.c_char_p


@pytest.mark.parametrize("text", [
    "int avt_x(unsigned long n);",                            # a scalar outside the ABI's vocabulary
    "int avt_x(int n, long m);",
    "int avt_x(const float* x, int (*done)(int), void* stream);",  # a function pointer
    "int avt_a(int n), avt_b(int m);",                        # two declarators: the strict pattern reads neither
    "int avt_a(int n);\nvoid avt_b(int n);",                  # a return type outside the ABI's: avt_b is seen, not read
    "int avt_a(int n);\nint avt_b(int n)\n/* ; */ { return n; }",  # no terminating semicolon
], ids=["unsigned-long", "long", "function-pointer", "two-declarators", "void-return", "no-semicolon"])
def test_parser_refuses_what_it_cannot_read(avt, text):
    with pytest.raises(avt._lib.AvtError):
        avt._lib.parse_header(text)


def test_a_name_declared_twice_is_an_error(avt):
    """What the dict of declarations would keep silently — the last one — is refused, whether or not the two agree."""
    for text in ("int avt_a(int n);\nint avt_b(void);\nint avt_a(int n);", "int avt_a(int n);\nint64_t avt_a(const float* x, int n);"):
        with pytest.raises(avt._lib.AvtError, match="avt_a is declared twice"):
            avt._lib.parse_header(text)


def test_parser_reads_arrays_and_unnamed_parameters(avt):
    C = ctypes
    table = avt._lib.parse_header("#define AVT_X (1)\n/* avt_gone(int) */\nint64_t avt_y(const float mean[3], int, double* out,\n"
                                  "              const char *name /* avt_z( */);")
    assert table == {"avt_y": (C.c_int64, [C.c_void_p, C.c_int, C.c_void_p, C.c_char_p])}


def test_checked_entries_raise_and_raw_entries_return_the_status(avt):
    """_lib.checked.avt_X and _lib.lib().avt_X are two ctypes functions of one symbol: the first raises check()'s error under the
    entry's own name, the second keeps returning the status.  Host-only entries: no device is touched."""
    lib, checked = avt._lib.lib(), avt._lib.checked
    k, b = np.zeros((32, 11), np.int32), np.zeros((32, 2), np.int32)
    with pytest.raises(avt._lib.AvtError) as e:
        checked.avt_resize_u8_tables(45, 32, 1, 9, k.ctypes.data, b.ctypes.data)  # Lanczos 45 -> 32 has 11 taps, not 9
    assert lib.avt_resize_u8_tables(45, 32, 1, 9, k.ctypes.data, b.ctypes.data) == -1
    message = lib.avt_last_error().decode()
    assert "11 taps" in message and str(e.value) == "avt_resize_u8_tables failed (-1): " + message
    with pytest.raises(avt._lib.AvtError) as e2:
        avt._lib.check(-1, "avt_resize_u8_tables")
    assert str(e2.value) == str(e.value)
    assert lib.avt_resize_u8_tables.errcheck is not checked.avt_resize_u8_tables.errcheck
    assert checked.avt_resize_u8_tables is checked.avt_resize_u8_tables and "avt_resize_u8_tables" in vars(checked)
    assert list(checked.avt_resize_u8_tables.argtypes) == list(lib.avt_resize_u8_tables.argtypes)
    with pytest.raises(AttributeError):
        checked.avt_no_such_entry
    fast, slow = np.full(32, -1, np.int32), np.full(8, -1, np.int32)
    assert checked.avt_clip_sample_table(20, fast.ctypes.data, slow.ctypes.data) == 0
    want_fast, want_slow = avt.ops.clip_sample_table(20)
    assert np.array_equal(fast, want_fast) and np.array_equal(slow, want_slow)


def test_plane_job_table_layout_matches_the_header(avt):
    """AvtPlaneJob (include/avt.h) as the three parties see it: the header's fields mirrored in ctypes, the library's own sizeof, and the
    struct format train_ops.pack_plane_jobs packs the device table with — and the table's bytes for one job of each kind (rows, transposed
    with three selected taps, gathered rows; made-up addresses) against the ctypes mirror filled field by field."""
    import struct

    from avtex import train_ops

    class AvtPlaneJob(ctypes.Structure):
        _fields_ = ([(n, ctypes.c_void_p) for n in ("w", "hi", "lo", "wscale", "map")] +
                    [(n, ctypes.c_int32) for n in ("kind", "f16", "rows", "k", "cout", "taps", "cin", "nsel", "gx", "gy", "blk0", "pad_")] +
                    [("sel", ctypes.c_int32 * 32)])

    src = open(avt._lib.HEADER_PATH).read()
    body = src[src.index("typedef struct AvtPlaneJob {"):src.index("} AvtPlaneJob;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = re.findall(r"\b([a-z_0-9]+)(?:\[32\])?\s*[;,]", body)
    assert declared == [f[0] for f in AvtPlaneJob._fields_], declared
    assert ctypes.sizeof(AvtPlaneJob) == avt._lib.lib().avt_weight_planes_job_bytes() == struct.calcsize("<5Q12i32i") == 216
    assert AvtPlaneJob.sel.offset == 88 and AvtPlaneJob.blk0.offset == 80

    def fields(ptrs, ints, sel=()):
        return {"fields": tuple(ptrs) + tuple(ints), "sel": tuple(sel)}

    # (owner's address, job): kind 0 = 24 rows of 72 into fp16 planes with a row scale, one block per row; kind 1 = [cout 40, 9 taps,
    # cin 48] transposed for taps 8, 4, 0: 2 x 2 tiles of 32 per tap; kind 2 = 16 rows of 40 gathered through an index map
    jobs = [(0x7F0000001000, dict(fields((0xA000, 0xB000, 0xC000, 0), (0, 1, 24, 72, 0, 0, 0, 0, 0, 0)), off=0, blocks=24)),
            (0x7F0000001000, dict(fields((0xD000, 0xE000, 0, 0), (1, 0, 0, 0, 40, 9, 48, 3, 2, 2), (8, 4, 0)), off=64, blocks=12)),
            (0x7F0000200000, dict(fields((0x1A000, 0x1B000, 0, 0x1C000), (2, 0, 16, 40, 0, 0, 0, 0, 0, 0)), off=4096, blocks=16))]
    raw, blk2job, blocks = train_ops.pack_plane_jobs(jobs)
    want, blk0 = b"", 0
    for base, j in jobs:
        s = AvtPlaneJob()
        s.w = base + j["off"]
        s.hi, s.lo, s.wscale, s.map = (v or None for v in j["fields"][:4])
        (s.kind, s.f16, s.rows, s.k, s.cout, s.taps, s.cin, s.nsel, s.gx, s.gy) = j["fields"][4:]
        s.blk0, s.pad_ = blk0, 0
        for i, v in enumerate(j["sel"]):
            s.sel[i] = v  # (the other taps stay zero)
        want += bytes(s)
        blk0 += j["blocks"]
    assert raw == want and len(raw) == 3 * 216
    assert [AvtPlaneJob.from_buffer_copy(raw, 216 * n).blk0 for n in range(3)] == [0, 24, 36]
    assert list(AvtPlaneJob.from_buffer_copy(raw, 216).sel) == [8, 4, 0] + [0] * 29
    assert blocks == 52 and blk2job.dtype == np.int32 and blk2job.tolist() == [0] * 24 + [1] * 12 + [2] * 16
    raw0, blk0_, blocks0 = train_ops.pack_plane_jobs([])
    assert raw0 == b"" and blocks0 == 0 and blk2job.dtype == blk0_.dtype and blk0_.shape == (0,)


def test_no_torch_types_in_header(avt):
    src = open(avt._lib.HEADER_PATH).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)  # comments cite the torch calls each entry replaces
    assert "torch" not in code.lower() and "at::" not in code and "Tensor" not in code and 'extern "C"' in code


def test_product_never_imports_the_oracle(avt):
    root = os.path.dirname(avt._lib.LIB_PATH)
    for dp, _, files in os.walk(root):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                txt = open(os.path.join(dp, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt and "avt_oracle" not in txt.replace(
                    "oracle/avt_oracle.c", ""), f


def test_cpu_tensors_are_rejected_not_emulated(avt):
    with pytest.raises(avt._lib.AvtError):
        avt.ops.l2norm_rows(torch.zeros(4, 8))
    with pytest.raises(avt._lib.AvtError):
        avt.ops.sim_gemm_nt(torch.zeros(4, 8), torch.zeros(4, 8), 0.1)
    with pytest.raises(avt._lib.AvtError):
        avt.texture.TextureEngine(torch.nn.Linear(2, 2), torch.nn.Linear(2, 2), window=4, stride=2, device="cpu")


@pytest.mark.parametrize("W", [2, 5, 10, 13, 15, 20, 32, 33, 64, 100])
def test_sample_table_equals_torch_linspace(avt, W):
    fast, slow = avt.ops.clip_sample_table(W)
    ref_fast = torch.linspace(0, W - 1, 32).long()
    ref_slow = ref_fast[torch.linspace(0, 31, 8).long()]
    assert np.array_equal(fast, ref_fast.numpy()) and np.array_equal(slow, ref_slow.numpy())


def test_clip_pack_plan_is_the_inverse_of_the_sample_table(avt):
    W, S, n = 20, 4, 9
    starts = np.arange(n) * S
    F_ = starts[-1] + W + 2
    off, slot = avt.ops.clip_pack_plan(starts, W, F_)
    fast, slow = avt.ops.clip_sample_table(W)
    assert off[0] == 0 and off[-1] == n * 40 and len(slot) == n * 40
    seen = set()
    for f in range(F_):
        for v in slot[off[f] : off[f + 1]]:
            win, s = divmod(int(v), 40)
            src = starts[win] + (slow[s] if s < 8 else fast[s - 8])
            assert src == f
            seen.add(int(v))
    assert seen == set(range(n * 40))
    with pytest.raises(avt._lib.AvtError):
        avt.ops.clip_pack_plan(np.array([F_ - 3]), W, F_)  # window leaves the video: loud error


def test_conv_ktab(avt):
    tab = avt.ops.conv3d_ktab(16, (1, 3, 3), 10, 12, 16)
    assert tab.shape == (8 * 3 + 2, 2)  # K = 144 -> 3 K-steps of 64, + 16 zero bytes
    kc = 5  # chunk 5: tap 2 (dh=0, dw=2), channels 8..15
    assert tab[kc, 1] == (1 | 1 << 8 | 1 << 18) and tab[kc, 0] == 2 * 16 + 8
    assert (tab[18:24, 1] == -1).all() and (tab[24:] == 0).all()


# ---- argument rejection of the convolution / pointwise entries: every AVT_REQUIRE runs before the first HIP call, so the raw entries
# can be called on a box without a GPU with made-up (16-byte-aligned, never dereferenced) addresses and ONE bad argument each
_P = [0x10000 * (i + 1) for i in range(10)]  # fake device addresses
_GEOM = dict(batch=2, t=5, h=8, w=6, cin=24, cout=40, kt=2, kh=1, kw=3, st=1, sh=2, sw=1, pt=1, ph=0, pw=2, to=0, ho=0, wo=0,
             ldi=24, ldo=40, ldr=0, relu=1, out_row_stride=1, out_h=0, out_w=0, plane_dtype=0)
_GEOM_S1 = dict(_GEOM, sh=1)  # the entries without strides
_PW = dict(ldx=64, k=64, ldr=0, ldy=64, n=64, m=100, relu=1, plane_dtype=0)


def _ints(g, names):
    return [g[n] for n in names.split()]


_ENTRIES = {
    "avt_conv3d_igemm_bf16": (_GEOM, lambda g: [_P[0], _P[1], _P[2], 0, _P[3], _P[4]] + _ints(
        g, "batch t h w cin cout kt kh kw st sh sw pt ph pw to ho wo ldi ldo ldr relu") + [0]),
    "avt_conv3d_igemm_x3": (_GEOM, lambda g: [_P[0], _P[1], _P[2], _P[3], _P[4], 0, 0, _P[5], _P[6], _P[7]] + _ints(
        g, "batch t h w cin cout kt kh kw st sh sw pt ph pw to ho wo ldi ldo ldr relu out_row_stride out_h out_w plane_dtype") + [0, 0]),
    "avt_conv3d_igemm_x3_f32": (_GEOM, lambda g: [_P[0], _P[1], _P[2], 0, 0, _P[3], _P[4]] + _ints(
        g, "batch t h w cin cout kt kh kw st sh sw pt ph pw ldi ldo ldr plane_dtype") + [0]),
    "avt_conv3d_igemm_x3_f32_ex": (_GEOM_S1, lambda g: [_P[0], _P[1], _P[2], 0, _P[3], _P[4]] + _ints(
        g, "batch t h w cin cout kt kh kw pt ph pw to ho wo ldi ldo out_row_stride out_h out_w plane_dtype") + [0]),
    "avt_pw_x3": (_PW, lambda g: [_P[0], _P[1], g["ldx"], g["k"], _P[2], _P[3], _P[4], 0, 0, 0, g["ldr"], _P[5], _P[6], g["ldy"], g["n"],
                                  g["m"], g["relu"], g["plane_dtype"], 0]),
    "avt_pw_x3_f32": (_PW, lambda g: [_P[0], g["ldx"], g["k"], _P[1], _P[2], 0, 0, 0, _P[3], g["ldy"], g["n"], g["m"], g["plane_dtype"], 0]),
}
_BIG = dict(batch=1 << 12, t=8, h=256, w=256, kt=3)  # 2^31 input rows of 24 channels, temporal taps: no frame ranges
# ... and with few rows, so that the input plane's term of the shared check trips alone: 4096 x 240 rows of 2192 columns are 2^31 + 7.3e6
# elements, the output is 786 432 rows of 40
_BIG_IN = dict(batch=1 << 12, ldi=2192, kt=3)
_REJECTED = [
    ("avt_conv3d_igemm_bf16", dict(cin=12), "avt_conv3d_igemm_bf16: Cin/Cout must be multiples of 8"),
    ("avt_conv3d_igemm_bf16", dict(kw=9), "avt_conv3d_igemm_bf16: kernel extents must be 1..8"),
    ("avt_conv3d_igemm_bf16", dict(ldo=32), "avt_conv3d_igemm_bf16: leading dimensions must be multiples of 8 and cover the channels"),
    ("avt_conv3d_igemm_bf16", _BIG_IN, "avt_conv3d_igemm_bf16: tensor too large for 32-bit offsets"),
    ("avt_conv3d_igemm_x3", dict(cin=12), "avt_conv3d_igemm_x3: Cin/Cout must be multiples of 8"),
    ("avt_conv3d_igemm_x3", dict(kw=9), "avt_conv3d_igemm_x3: kernel extents must be 1..8"),
    ("avt_conv3d_igemm_x3", dict(ldo=32), "avt_conv3d_igemm_x3: leading dimensions must be multiples of 8 and cover the channels"),
    # the layer's output is 6 x 4 x 8: stride-2 rows need a grid of 7 x 15
    ("avt_conv3d_igemm_x3", dict(out_row_stride=2, out_h=7, out_w=14),
     "avt_conv3d_igemm_x3: the remapped rows need an out_h x out_w grid that holds 2 x (4 x 8), no residual"),
    ("avt_conv3d_igemm_x3", dict(out_row_stride=2, out_h=6, out_w=15),
     "avt_conv3d_igemm_x3: the remapped rows need an out_h x out_w grid that holds 2 x (4 x 8), no residual"),
    ("avt_conv3d_igemm_x3", _BIG_IN, "avt_conv3d_igemm_x3: tensor too large for 32-bit offsets"),
    ("avt_conv3d_igemm_x3", dict(plane_dtype=2), "avt_conv3d_igemm_x3: plane_dtype must be 0 (bf16) or 1 (fp16)"),
    ("avt_conv3d_igemm_x3_f32", dict(cin=12), "avt_conv3d_igemm_x3_f32: Cin/Cout must be multiples of 8"),
    ("avt_conv3d_igemm_x3_f32", dict(kw=9), "avt_conv3d_igemm_x3_f32: kernel extents must be 1..8"),
    ("avt_conv3d_igemm_x3_f32", dict(ldo=32), "avt_conv3d_igemm_x3_f32: leading dimensions must be multiples of 8 and cover the channels"),
    ("avt_conv3d_igemm_x3_f32", _BIG, "avt_conv3d_igemm_x3_f32: input too large for 32-bit byte offsets"),
    ("avt_conv3d_igemm_x3_f32", dict(plane_dtype=2), "avt_conv3d_igemm_x3_f32: plane_dtype must be 0 (bf16) or 1 (fp16)"),
    ("avt_conv3d_igemm_x3_f32_ex", dict(cin=12), "avt_conv3d_igemm_x3_f32: Cin/Cout must be multiples of 8"),
    ("avt_conv3d_igemm_x3_f32_ex", dict(kw=9), "avt_conv3d_igemm_x3_f32: kernel extents must be 1..8"),
    ("avt_conv3d_igemm_x3_f32_ex", dict(ldo=32), "avt_conv3d_igemm_x3_f32: leading dimensions must be multiples of 8 and cover the channels"),
    # stride 1: the output is 6 x 8 x 8; one class of a stride-2 transposed convolution needs a grid of 15 x 15
    ("avt_conv3d_igemm_x3_f32_ex", dict(out_row_stride=2, out_h=15, out_w=14),
     "avt_conv3d_igemm_x3_f32: the remapped rows need an out_h x out_w grid that holds 2 x (8 x 8), no residual"),
    ("avt_conv3d_igemm_x3_f32_ex", dict(out_row_stride=2, out_h=14, out_w=15),
     "avt_conv3d_igemm_x3_f32: the remapped rows need an out_h x out_w grid that holds 2 x (8 x 8), no residual"),
    ("avt_conv3d_igemm_x3_f32_ex", dict(to=8), "avt_conv3d_igemm_x3_f32: bad output extent 8x8x8 (max 7x8x10)"),  # max = the formula's 6x8x8 + (k - 1) / s
    ("avt_conv3d_igemm_x3_f32_ex", _BIG, "avt_conv3d_igemm_x3_f32: input too large for 32-bit byte offsets"),
    ("avt_conv3d_igemm_x3_f32_ex", dict(plane_dtype=2), "avt_conv3d_igemm_x3_f32: plane_dtype must be 0 (bf16) or 1 (fp16)"),
    ("avt_pw_x3", dict(k=192, ldx=192), "avt_pw_x3: unsupported layer K=192 N=64"),
    ("avt_pw_x3", dict(ldy=56), "avt_pw_x3: bad sizes / leading dimensions"),
    ("avt_pw_x3", dict(plane_dtype=2), "avt_pw_x3: bad plane_dtype"),
    ("avt_pw_x3_f32", dict(k=96, ldx=96), "avt_pw_x3_f32: unsupported layer K=96 N=64"),
    ("avt_pw_x3_f32", dict(ldy=60), "avt_pw_x3_f32: bad sizes / leading dimensions"),
    ("avt_pw_x3_f32", dict(plane_dtype=2), "avt_pw_x3_f32: bad plane_dtype"),
]


# (with made-up addresses a check that went missing would be a real launch: never where a device is visible)
@pytest.mark.skipif(torch.cuda.is_available(), reason="made-up device addresses: only on a box without a GPU")
@pytest.mark.parametrize("entry,bad,message", _REJECTED, ids=["%s-%s" % (e, "-".join(b)) for e, b, _ in _REJECTED])
def test_bad_arguments_are_rejected_before_any_launch(avt, entry, bad, message):
    lib = avt._lib.lib()
    base, args = _ENTRIES[entry]
    assert set(bad) <= set(base)
    AVT_ERR_ARG = -1  # include/avt.h
    assert getattr(lib, entry)(*args(dict(base, **bad))) == AVT_ERR_ARG
    assert lib.avt_last_error().decode() == message
