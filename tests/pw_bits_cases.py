"""The cases of tests/test_gpu_pw_bits.py (and of tools/record_wgrad_bits.py with this module named): every entry of csrc/pw_x3.hip
on inputs built on the host, every output buffer pre-filled with a byte pattern and hashed WHOLE, byte for byte, so that a store
outside the slice shows too.

These kernels have no atomics and a launch geometry fixed by (k, n, m, groups): every output is reproducible as it stands.  Inputs
are wgrad_bits_cases.hashed values, split into planes by fused_slowfast.split_planes and packed by pack_pw_planes (both elementwise
and exact).  The statistics entries are called with a workspace filled here (ops.pw_x3_f32_stats allocates its own with torch.empty)
and only the partial rows — the head of the workspace, sized by the `*_rows` query — are hashed.

What each list has to reach (the instance, the ragged edge, the path) is asserted below on the host, with the library's own tile
arithmetic restated: a case list that stops reaching one fails at import."""
import hashlib
import zlib

from wgrad_bits_cases import DEV, hashed

FILL = 0xA5
NW = 8  # waves per workgroup
DTYPES = ("f16", "bf16")
PAD = (8, 16, 24)  # ldx - k, ldy - n, ldr - n of the padded cases

# pw_x3_kernel.  name: k, n, m, residual, relu, padded leading dimensions
M_RAGGED = 16 * 8 * 3 + 5  # three rounds of one row group's 8 waves and a ragged last tile
PW = {
    "nt2": (64, 32, M_RAGGED, 1, 1, 0),
    "nt4": (64, 64, M_RAGGED, 0, 1, 0),
    "nt8": (64, 128, M_RAGGED, 1, 0, 0),
    "nt16": (64, 256, M_RAGGED, 1, 1, 0),
    "ragged-k72": (72, 64, M_RAGGED, 1, 1, 1),
    "ragged-k136-less-than-a-tile": (136, 64, 5, 0, 0, 0),
    "k-step-1": (32, 32, 5, 1, 1, 0),
    "k-step-8": (256, 128, M_RAGGED, 0, 1, 0),
    "k-step-10": (320, 64, M_RAGGED, 1, 1, 0),
    "k-step-16": (512, 64, M_RAGGED, 1, 0, 1),
    "chunks-2": (128, 512, M_RAGGED, 1, 1, 1),
    "chunks-8": (128, 2048, M_RAGGED, 0, 1, 0),
}
PW_TWICE = {"twice-round-the-loop": (128, 2048, 4099, 1, 1, 0)}  # fp16 planes only: the one large case
# avt_lateral_x3 at kt 7, stride 4, pad 3, t = 9 (frames below 0 and past the end, a last partial window), hw = 35.  name: cin, cout
LATERAL = {"k-step-2": (8, 32), "k-step-7": (32, 64), "k-step-14": (64, 128), "padded-tile-pair": (8, 16)}
LAT_B, LAT_T, LAT_HW, LAT_KT, LAT_ST, LAT_PT = 2, 9, 35, 7, 4, 3
# avt_pw_chain_x3 (64 -> 256 -> 64).  name: m, residual
CHAIN = {"ragged-residual": (261, 1), "past-the-grid": (32768 + 133, 0)}  # 256 workgroups x 8 waves = 2048 tiles = 32768 rows
# pw_x3_f32_kernel, plain.  name: k, n, m
F32 = {
    "k8-nt2": (8, 32, M_RAGGED),
    "k40-nt4": (40, 64, M_RAGGED),
    "k104-nt8": (104, 128, 5),
    "k256-nt8": (256, 128, M_RAGGED),
    "k64-nt16": (64, 256, M_RAGGED),
    "k128-chunks-2": (128, 512, M_RAGGED),
}
# ... with the forward statistics (STATS == 1) at the three scratch widths.  name: k, n;  rows per group: 389 / 197
STATS = {"pw32-narrow": (40, 32), "pw64": (64, 128), "pw32-lds": (128, 256)}
ROWS_G = {1: M_RAGGED, 2: 197}
# ... and the backward form (STATS == 2; bf16 planes).  name: k, n, groups
BWD = {"n64": (128, 64, 2), "n256": (64, 256, 1), "n256-k128": (128, 256, 2)}
BWD_MASK = ("bits", "beta", "norelu")


def k_steps(k):
    return (k + 31) // 32


def pick_nt1(k1s, n):  # csrc/pw_x3.hip
    if n % 32:
        return 0
    return next((t for t in (16, 8, 4, 2) if (n // 16) % t == 0 and 2 * t * k1s <= 128), 0)


def row_groups(lds_bytes, n_chunks, ntiles, groups=1):  # csrc/pw_x3.hip: pf_row_groups
    per_cu = 1 if lds_bytes > 80 * 1024 else (2 if lds_bytes > 52 * 1024 else 3)
    n_rg = max(8, (256 * per_cu) // (n_chunks * groups) // 8 * 8)
    return min(n_rg, -(-(-(-ntiles // NW)) // 8) * 8)


def stat_width(k1s, nt1):  # csrc/pw_x3.hip: PfStat::PW
    nc = nt1 * 16
    return nc if nc < 64 else (32 if 2 * nt1 * k1s * 1024 >= 96 * 1024 else 64)


def _reached(cases):
    return {(k_steps(c[0]), pick_nt1(k_steps(c[0]), c[1])) for c in cases}


_px = _reached(PW.values())
assert {t for _, t in _px} == {2, 4, 8, 16} and {s for s, _ in _px} == {1, 2, 3, 4, 5, 8, 10, 16}, _px
assert {c[1] // (16 * pick_nt1(k_steps(c[0]), c[1])) for c in PW.values()} >= {1, 2, 8}
assert any(c[0] % 32 and c[5] for c in PW.values()) and any(c[2] < 16 for c in PW.values())
assert {(c[3], c[4]) for c in PW.values()} == {(0, 0), (0, 1), (1, 0), (1, 1)}
_k, _n, _m = PW_TWICE["twice-round-the-loop"][:3]
_lds = 2 * 16 * k_steps(_k) * 1024 + 2 * 16 * 16 * 4
assert pick_nt1(k_steps(_k), _n) == 16 and row_groups(_lds, _n // 256, -(-_m // 16)) * NW < -(-_m // 16)  # a wave takes a second tile
assert [k_steps(LAT_KT * c[0]) for c in LATERAL.values()] == [2, 7, 14, 2]
assert (LAT_T + 2 * LAT_PT - LAT_KT) // LAT_ST + 1 == 3 and 2 * LAT_ST - LAT_PT + LAT_KT - 1 >= LAT_T and LAT_PT > 0
assert any(m > 256 * NW * 16 for m, _ in CHAIN.values())
_f = _reached(F32.values())
assert {t for _, t in _f} == {2, 4, 8, 16} and {s for s, _ in _f} == {1, 2, 4, 8} and sum(c[0] % 32 != 0 for c in F32.values()) == 3, _f
assert [stat_width(k_steps(k), pick_nt1(k_steps(k), n)) for k, n in STATS.values()] == [32, 64, 32]
assert [pick_nt1(k_steps(k), n) for k, n in STATS.values()] == [2, 8, 16]
assert [pick_nt1(k_steps(k), n) for k, n, _ in BWD.values()] == [4, 16, 16]  # (16 runs as 8 tiles, two chunks)
assert all(r % 16 for r in ROWS_G.values())

KEYS = (["pw/%s/%s" % (n, d) for n in PW for d in DTYPES] + ["pw/%s/f16" % n for n in PW_TWICE] +
        ["lateral/%s/%s" % (n, d) for n in LATERAL for d in DTYPES] + ["chain/%s/%s" % (n, d) for n in CHAIN for d in DTYPES] +
        ["f32/%s/%s/add%d" % (n, d, a) for n in F32 for d in DTYPES for a in (0, 1)] +
        ["stats/%s/%s/g%d" % (n, d, g) for n in STATS for d in DTYPES for g in (1, 2)] +
        ["bwd/%s/%s/add%d" % (n, mk, a) for n in BWD for mk in BWD_MASK for a in (0, 1)])

_HOST = {}


def _h(tag, *shape):
    """fp32 host tensor of a case (hashed values in (-0.5, 0.5)): built once, shared by the case's settings, never written to."""
    import torch
    if (tag, shape) not in _HOST:
        _HOST[(tag, shape)] = torch.from_numpy(hashed(shape, zlib.crc32(tag.encode())))
    return _HOST[(tag, shape)]


def _dtype(d):
    from avtex import ops
    return ops.X3_F16 if d == "f16" else ops.X3_BF16


def _planes(w, d, ld=0):
    """[m, c] fp32 -> device (hi, lo) planes [m, max(ld, c)], the padding columns zero"""
    import torch
    from avtex.fused_slowfast import split_planes
    hi, lo = split_planes(w, _dtype(d))
    if ld > w.shape[1]:
        hi, lo = (torch.nn.functional.pad(p, (0, ld - w.shape[1])) for p in (hi, lo))
    return hi.contiguous().to(DEV), lo.contiguous().to(DEV)


def _packed(w, d):
    from avtex.fused_slowfast import pack_pw_planes, split_planes
    return tuple(pack_pw_planes(p).to(DEV) for p in split_planes(w, _dtype(d)))


def _filled(dtype, *shape):
    """an output buffer: every byte FILL"""
    import torch
    n = 1
    for s in shape:
        n *= s
    return torch.full((n * torch.empty((), dtype=dtype).element_size(),), FILL, dtype=torch.uint8, device=DEV).view(dtype).view(*shape)


def _ptrs(pair):
    return (pair[0].data_ptr(), pair[1].data_ptr())


def _scale(tag, n, d):
    """per-channel scales in (0.5, 1.5) for fp16 planes (whose weights carry row scales), none for bf16"""
    return (_h(tag + "/scale", n) + 1.0).to(DEV) if d == "f16" else None


def _pw(name, d):
    from avtex import ops
    k, n, m, has_res, relu, padded = {**PW, **PW_TWICE}[name]
    dx, dy, dr = PAD if padded else (0, 0, 0)
    x = _planes(_h(name + "/x", m, k), d, k + dx)
    w = _packed(_h(name + "/w", n, k), d)
    res = _planes(_h(name + "/r", m, n), d, n + dr) if has_res else None
    y = (_filled(x[0].dtype, m, n + dy), _filled(x[0].dtype, m, n + dy))
    ops.pw_x3(_ptrs(x), k + dx, k, w[0], w[1], _h(name + "/b", n).to(DEV), _scale(name, n, d), _ptrs(res) if res else None, n + dr, _ptrs(y),
              n + dy, n, m, relu, _dtype(d))
    return y


def _lateral(name, d):
    import torch
    from avtex import ops
    cin, cout = LATERAL[name]
    n = -(-cout // 32) * 32  # the weight rows, bias and scales are padded to whole tile pairs
    to = (LAT_T + 2 * LAT_PT - LAT_KT) // LAT_ST + 1
    x = _planes(_h(name + "/x", LAT_B * LAT_T * LAT_HW, cin), d)
    w = _h(name + "/w", n, LAT_KT * cin).clone()
    w[cout:] = 0.0
    bias = _h(name + "/b", n).clone()
    bias[cout:] = 0.0
    y = (_filled(torch.bfloat16, LAT_B * to * LAT_HW, cout), _filled(torch.bfloat16, LAT_B * to * LAT_HW, cout))
    pk = _packed(w, d)
    ops.lateral_x3(_ptrs(x), cin, cin, pk[0], pk[1], bias.to(DEV), _scale(name, n, d), _ptrs(y), cout, cout, LAT_B, LAT_T, LAT_HW, LAT_KT,
                   LAT_ST, LAT_PT, True, _dtype(d))
    return y


def _chain(name, d):
    import torch
    from avtex import ops
    m, has_res = CHAIN[name]
    x = _planes(_h(name + "/x", m, 64), d)
    res = _planes(_h(name + "/r", m, 256), d) if has_res else None
    y = (_filled(torch.bfloat16, m, 256), _filled(torch.bfloat16, m, 256))
    z = (_filled(torch.bfloat16, m, 64), _filled(torch.bfloat16, m, 64))
    ops.pw_chain_x3(_ptrs(x), 64, 64, _packed(_h("chain/w1", 256, 64), d), _h("chain/b1", 256).to(DEV), _scale("chain/1", 256, d),
                    _ptrs(res) if res else None, 256, _ptrs(y), 256, 256, True, _packed(_h("chain/w2", 64, 256), d),
                    _h("chain/b2", 64).to(DEV), _scale("chain/2", 64, d), _ptrs(z), 64, 64, m, _dtype(d))
    return y + z


def _f32_weights(tag, n, k, d):
    """plain [n, k] planes; fp16 planes hold weights scaled up (the training path's row scaling), undone by the scales"""
    w = _h(tag + "/w", n, k)
    return _planes(w * 1024.0 if d == "f16" else w, d)


def _f32(name, d, add):
    import torch
    from avtex import ops
    k, n, m = F32[name]
    wh, wl = _f32_weights(name, n, k, d)
    y = _filled(torch.float32, m, n)
    ops.pw_x3_f32(_h(name + "/x", m, k).to(DEV), k, wh, wl, _scale(name, n, d), y, n, _dtype(d), add=_h(name + "/a", m, n).to(DEV) if add else None)
    return (y,)


def _workspace(rows, n, groups):
    """-> (the BatchNorm workspace with every byte FILL, the bytes of its head that hold the partial rows)"""
    from avtex import ops
    ws, _ = ops._stat_ws(rows, n, groups, DEV)
    head = groups * rows * 2 * n * 8  # per row: two statistics of n channels in fp64
    assert 0 < head <= ws.numel()
    return ws.fill_(FILL), head


def _stats(name, d, groups):
    import torch
    from avtex import _lib, ops
    k, n = STATS[name]
    m = ROWS_G[groups] * groups
    rows = _lib.lib().avt_pw_x3_f32_stat_rows(k, n, m, groups)
    assert rows > 0
    ws, head = _workspace(rows, n, groups)
    wh, wl = _f32_weights(name, n, k, d)
    x, y, scale = _h(name + "/x", m, k).to(DEV), _filled(torch.float32, m, n), _scale(name, n, d)
    ops.K.avt_pw_x3_f32_stats(ops._p(x), k, k, ops._p(wh), ops._p(wl), ops._p(scale), ops._p(y), n, n, m, _dtype(d), ops._p(ws), groups,
                              ops._stream())
    return y, ws[:head]


def _bwd(name, mask_kind, add):
    import torch
    from avtex import _lib, ops
    k, n, groups = BWD[name]
    m = ROWS_G[groups] * groups
    rows = _lib.lib().avt_pw_x3_f32_bwdstats_rows(k, n, m, groups)
    assert rows > 0
    ws, head = _workspace(rows, n, groups)
    wh, wl = _f32_weights(name, n, k, "bf16")
    dy, y = _h(name + "/dy", m, k).to(DEV), _filled(torch.float32, m, n)
    addt = _h(name + "/a", m, n).to(DEV) if add else None
    bx, mean = _h(name + "/bx", m, n).to(DEV), (_h(name + "/mean", groups * n) * 0.25).to(DEV)
    invstd, gamma, beta = (_h(name + "/invstd", groups * n) + 1.0).to(DEV), (_h(name + "/gamma", n) + 1.0).to(DEV), _h(name + "/beta", n).to(DEV)
    # saved mask bits: one byte per four elements, in its low nibble (any fixed bytes do)
    mask = ((_h(name + "/mask", m * n // 4) + 0.5) * 256.0).to(torch.uint8).to(DEV) if mask_kind == "bits" else None
    ops.K.avt_pw_x3_f32_bwdstats(ops._p(dy), k, k, ops._p(wh), ops._p(wl), ops._p(addt), n, ops._p(y), n, n, m, ops.X3_BF16, ops._p(bx),
                                 ops._p(mean), ops._p(invstd), ops._p(gamma), ops._p(beta) if mask_kind == "beta" else None, ops._p(mask),
                                 0 if mask_kind == "norelu" else 1, ops._p(ws), groups, ops._stream())
    return y, ws[:head]


def digest(key):
    """SHA-256 over the bytes of every output buffer of one key of KEYS, in the order the case returns them."""
    import torch
    family, name, *rest = key.split("/")
    if family == "pw":
        out = _pw(name, rest[0])
    elif family == "lateral":
        out = _lateral(name, rest[0])
    elif family == "chain":
        out = _chain(name, rest[0])
    elif family == "f32":
        out = _f32(name, rest[0], rest[1] == "add1")
    elif family == "stats":
        out = _stats(name, rest[0], int(rest[1][1:]))
    else:
        out = _bwd(name, rest[0], rest[1] == "add1")
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in out:
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()
