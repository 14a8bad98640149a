"""The makers of the training step's 16-bit planes, one by one at their edges, against tests/weight_planes_refs.py (numpy, pinned to
float64 and by hand in tests/test_weight_planes_refs_host.py): weight_planes_kernel, weight_planes_t_kernel, weight_planes_gather_kernel,
weight_planes_multi_kernel and clip_planes_kernel of csrc/stem_train.hip.  Planes are compared as raw 16-bit words and wscale as raw
32-bit words; a NaN by kind, not payload.  Then the convolutions: a weight row times 2^s has the same planes and another wscale, so the
output channel is the same bits times 2^s — in every form train_ops._conv_x3_rows runs in, and in the stems.

Every test prints the figures it asserts on (pytest -s shows them)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import weight_planes_refs as R

pytestmark = pytest.mark.gpu

PLANES = [("bf16x3", R.BF16), ("f16x3", R.F16)]
SENT = 0xFFFF            # guard / "not yet written" word of a plane: a NaN with every payload bit set, which no conversion makes
SENT32 = 0xFFFFFFFF      # the same for wscale
GUARD = 64               # guard words on each side of an output
_p = pytest.mark.parametrize


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same(got, want, plane, what):
    got, want = R.words(got) if torch.is_tensor(got) else got, np.asarray(want, np.uint16)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = R.same_words(got, want, plane)
    assert ok.all(), "%s: %d of %d words differ, first at %s: %#06x, reference %#06x" % (
        what, (~ok).sum(), ok.size, np.argwhere(~ok)[0].tolist(), got[~ok][0], want[~ok][0])


def _same32(got, want, what):
    g, w = R.bits32(got.cpu().numpy() if torch.is_tensor(got) else got), R.bits32(want)
    assert g.shape == w.shape and (g == w).all(), "%s: wscale words %s, reference %s at %s" % (
        what, [hex(v) for v in g[g != w][:4]], [hex(v) for v in w[g != w][:4]], np.flatnonzero(g != w)[:4].tolist())


class Guarded:
    """A device buffer of n 16-bit (or 32-bit) words between two runs of GUARD sentinel words, every word a sentinel at first."""

    def __init__(self, n, dev, wide=False):
        self.n, self.wide = int(n), wide
        self.buf = torch.full((self.n + 2 * GUARD,), -1, dtype=torch.int32 if wide else torch.int16, device=dev)
        self.view = self.buf[GUARD:GUARD + self.n].view(torch.float32 if wide else torch.bfloat16)  # what the package's builders take
        self.ptr = C.c_void_p(self.view.data_ptr())

    def words(self, what):
        """-> the n words between the guards; the guards must be intact."""
        raw = self.buf.cpu().numpy().view(np.uint32 if self.wide else np.uint16)
        sent = SENT32 if self.wide else SENT
        assert (raw[:GUARD] == sent).all() and (raw[GUARD + self.n:] == sent).all(), "%s: written outside the output" % what
        return raw[GUARD:GUARD + self.n].copy()


# ---------------------------------------------------------------- rows: ops.weight_planes_f32
@functools.lru_cache(maxsize=None)
def _rows_case(K, plane):
    names, w = R.edge_rows(K)
    return (names, w) + R.rows_ref(w, plane)


@_p("rows", [1, 3])
@_p("K", R.ROW_KS)
@_p("name,plane", PLANES)
def test_rows_at_every_edge(avt, dev, name, plane, K, rows):
    """Every edge row, launched alone (rows = 1) and in threes (neighbours of another scale): the reference's words."""
    names, w, e_hi, e_lo, e_ws = _rows_case(K, plane)
    wd = _up(w, dev)
    starts = [min(i, len(w) - rows) for i in range(0, len(w), rows)]
    outs = [avt.ops.weight_planes_f32(wd[i:i + rows], plane) for i in starts]
    torch.cuda.synchronize()
    for i, (hi, lo, ws) in zip(starts, outs):
        what = "K=%d %s rows %s" % (K, name, names[i:i + rows])
        _same(hi, e_hi[i:i + rows], plane, what + " hi")
        _same(lo, e_lo[i:i + rows], plane, what + " lo")
        if plane == R.F16:
            _same32(ws, e_ws[i:i + rows], what)
        else:
            assert ws is None


@_p("K", [2, 514])
def test_a_row_with_an_infinity(avt, dev, K):
    """The kernel takes frexpf of an infinite maximum.  Pinned: the infinity comes out as that infinity after (hi + lo) * wscale, wscale
    is a finite positive power of two, every other row is the reference's.  (What the row's finite entries become: include/avt.h.)"""
    w = R.inf_rows(K)
    hi, lo, ws = avt.ops.weight_planes_f32(_up(w, dev), R.F16)
    torch.cuda.synchronize()
    hi, lo, ws = R.words(hi), R.words(lo), ws.cpu().numpy()
    back = R.scaled_back(hi, lo, ws, R.F16)
    assert back[1, 1 % K] == np.inf and back[2, 0] == -np.inf
    m, e = np.frexp(ws)
    assert np.isfinite(ws).all() and (ws > 0).all() and (m == 0.5).all()
    e_hi, e_lo, e_ws = R.rows_ref(w, R.F16)
    for r in (0, 3):
        _same(hi[r], e_hi[r], R.F16, "row %d hi" % r)
        _same(lo[r], e_lo[r], R.F16, "row %d lo" % r)
        assert R.bits32(ws)[r] == R.bits32(e_ws)[r]
    fin = np.isfinite(w[1:3])
    err = np.abs(back[1:3][fin] - w[1:3][fin].astype(np.float64))
    print("infinity rows K=%d: wscale 2^%s; finite entries: largest |w| %.4g came back as %.6g, worst |error| %.3g, non-finite results %d"
          % (K, (e[1:3] - 1).tolist(), np.abs(w[1:3][fin]).max(), np.abs(back[1:3][fin]).max(), err.max(), (~np.isfinite(back[1:3][fin])).sum()))


def test_scale_invariance_is_exact(avt, dev):
    """planes(w * 2^s) has the words of planes(w) and wscale is multiplied by exactly 2^s, s in -6 .. 6 drawn per row."""
    _, w = R.edge_rows(514)
    mx = R.finite_max(w)
    w = w[(mx >= 2.0 ** -60) & (mx <= 2.0 ** 100)]  # (the shifted row stays clear of the 1e-30 clamp and of FLT_MAX)
    s = R.scale_shifts(len(w))
    assert set(s.tolist()) == set(range(-6, 7))
    two_s = np.ldexp(np.float32(1), s)
    a = avt.ops.weight_planes_f32(_up(w, dev), R.F16)
    b = avt.ops.weight_planes_f32(_up((w * two_s[:, None]).astype(np.float32), dev), R.F16)
    torch.cuda.synchronize()
    _same(b[0], R.words(a[0]), R.F16, "hi")
    _same(b[1], R.words(a[1]), R.F16, "lo")
    _same32(b[2], a[2].cpu().numpy() * two_s, "w * 2^s")


@_p("K", [2, 514])
def test_the_torch_route_on_the_device_gives_the_kernels_bits(avt, dev, K):
    """weight_planes._row_scaled_planes on DEVICE tensors (how the stems' LDS image is made): torch's frexp and the assembled scale
    there give the reference's words on every edge row, and on a row with an infinity what the kernel gives (exponent 0)."""
    from avtex import weight_planes

    _, w = R.edge_rows(K)
    e_hi, e_lo, e_ws = R.rows_ref(w, R.F16)
    hi, lo, sc = weight_planes._row_scaled_planes(_up(w, dev))
    _same(hi, e_hi, R.F16, "torch route on the device, K=%d hi" % K)
    _same(lo, e_lo, R.F16, "torch route on the device, K=%d lo" % K)
    _same32((1.0 / sc).float(), e_ws, "torch route on the device, K=%d" % K)
    wi = _up(R.inf_rows(K), dev)
    k_hi, k_lo, k_ws = avt.ops.weight_planes_f32(wi, R.F16)
    hi, lo, sc = weight_planes._row_scaled_planes(wi)
    torch.cuda.synchronize()
    _same(hi, R.words(k_hi), R.F16, "infinity rows hi")
    _same(lo, R.words(k_lo), R.F16, "infinity rows lo")
    _same32((1.0 / sc).float(), k_ws.cpu().numpy(), "infinity rows")


# ---------------------------------------------------------------- transposed: ops.weight_planes_t_f32
def _transposed(avt, dev, w, sel, cout=None, taps=None, cin=None):
    """avt_weight_planes_t_f32 into guarded, sentinel-filled outputs -> (hi, lo) words [cin, nsel, cout]."""
    co, tp, ci = w.shape
    cout, taps, cin = cout or co, taps or tp, cin or ci
    wd = _up(w, dev)
    hi, lo = Guarded(cin * len(sel) * cout, dev), Guarded(cin * len(sel) * cout, dev)
    arr = (C.c_int32 * len(sel))(*[int(v) for v in sel])
    try:
        avt.ops.K.avt_weight_planes_t_f32(avt.ops._p(wd), cout, taps, cin, arr, len(sel), hi.ptr, lo.ptr, avt.ops._stream())
    finally:
        torch.cuda.synchronize()
        out = [g.words("transposed") for g in (hi, lo)]
    return out


@_p("cout,taps,cin", R.T_SHAPES)
def test_transposed_planes_at_tile_edges(avt, dev, cout, taps, cin):
    """Every selection of the issue at every shape: all of [cin, nsel * cout] written (no sentinel left), nothing beside it, the
    reference's words."""
    w = R.transposed_weight(cout, taps, cin)
    for name, sel in R.transposed_sels(taps).items():
        e_hi, e_lo = R.transposed_ref(w, sel)
        hi, lo = _transposed(avt, dev, w, sel)
        assert (hi != SENT).all() and (lo != SENT).all(), "%s: words left unwritten" % name
        assert np.array_equal(hi, e_hi.reshape(-1)), "%s %s: hi" % (name, sel)
        assert np.array_equal(lo, e_lo.reshape(-1)), "%s %s: lo" % (name, sel)
        # and through the package's wrapper (its own allocation)
        p_hi, p_lo = avt.ops.weight_planes_t_f32(_up(w, dev), sel)
        assert p_hi.shape == (cin, len(sel) * cout)
        assert np.array_equal(R.words(p_hi).reshape(-1), hi) and np.array_equal(R.words(p_lo).reshape(-1), lo)


@_p("what,shape,sel", [("nsel_33", (4, 40, 8), list(range(33))), ("tap_equal_to_taps", (4, 9, 8), [0, 9]), ("odd_cout", (3, 2, 8), [0, 1])])
def test_transposed_refusals_come_before_any_launch(avt, dev, what, shape, sel):
    from avtex._lib import AvtError

    wd = _up(R.transposed_weight(*shape), dev)
    hi, lo = Guarded(shape[2] * len(sel) * shape[0], dev), Guarded(shape[2] * len(sel) * shape[0], dev)
    arr = (C.c_int32 * len(sel))(*sel)
    with pytest.raises(AvtError):
        avt.ops.K.avt_weight_planes_t_f32(avt.ops._p(wd), shape[0], shape[1], shape[2], arr, len(sel), hi.ptr, lo.ptr, avt.ops._stream())
    torch.cuda.synchronize()
    assert (hi.words(what) == SENT).all() and (lo.words(what) == SENT).all(), "a refused call wrote"
    with pytest.raises(AvtError):
        avt.ops.weight_planes_t_f32(wd, sel)


# ---------------------------------------------------------------- gathered rows: ops.weight_planes_gather_f32
def _storage(n, key):
    """fp32 [n]: magnitudes over 2^-8 .. 2^8 with -0.0, an fp32 denormal and, as the LAST element, the largest magnitude of all — one
    ulp below 2^9, where the scale's exponent steps."""
    g = R._rng(n, key)
    s = (g.uniform(0.5, 1.0, n) * 2.0 ** g.integers(-8, 9, n) * g.choice([-1.0, 1.0], n)).astype(np.float32)
    s[1], s[2] = np.float32(-0.0), np.array([0x00000123], np.uint32).view(np.float32)[0]
    s[n - 1] = -R._ulps(np.float32(512.0), -1)
    return s


def _gather_map(n, rows, K, key):
    g = R._rng(n, rows, K, key)
    m = g.integers(0, n, (rows, K)).astype(np.int32)
    m[g.uniform(size=(rows, K)) < 0.2] = -1     # zero taps
    m[0, 0] = n - 1                             # the last storage element
    m[1, :] = -1                                # a row that is all -1
    m[2, :] = m[2, 0] = 5                       # one offset, repeated
    m[3, : K // 2] = n - 1                      # the last element repeated, then others
    m[4, K - 1] = -1
    m[5, 0] = 0                                 # the FIRST storage element: offset 0 is an element, not a zero tap
    if rows > 6:
        m[6, K - 1] = 0
    return m


def _layouts(s, dev):
    """The same memory as a contiguous and as a channels-last [4, 8, 1, 3, 3] weight (n = 288)."""
    t = torch.from_numpy(s.copy())
    yield "contiguous", t.view(4, 8, 1, 3, 3).to(dev)
    yield "channels_last", t.view(4, 1, 3, 3, 8).permute(0, 4, 1, 2, 3).to(dev)


@_p("K", [2, 514])
@_p("name,plane", PLANES)
def test_gathered_rows(avt, dev, name, plane, K):
    n, rows = 288, 7
    s, m = _storage(n, K), _gather_map(n, rows, K, plane)
    e_hi, e_lo, e_ws = R.gather_ref(s, m, plane)
    md = _up(m, dev)
    for layout, w in _layouts(s, dev):
        assert (layout == "contiguous") == w.is_contiguous() and w.is_contiguous(memory_format=torch.channels_last_3d) == (layout != "contiguous")
        hi, lo, ws = avt.ops.weight_planes_gather_f32(w, md, plane)
        torch.cuda.synchronize()
        _same(hi, e_hi, plane, "%s K=%d %s hi" % (name, K, layout))
        _same(lo, e_lo, plane, "%s K=%d %s lo" % (name, K, layout))
        if plane == R.F16:
            _same32(ws, e_ws, "%s K=%d %s" % (name, K, layout))
        else:
            assert ws is None


# ---------------------------------------------------------------- one launch: ops.weight_planes_multi
def test_every_kind_in_one_launch(avt, dev):
    """One table from the package's own builders with rows, transposed and gathered jobs of both plane types, a one-block job between
    many-block jobs, in two orders: every output against the REFERENCE, guards intact."""
    from avtex import job_tables, ops, weight_planes as wp

    _, w_rows = R.edge_rows(514)
    w_one = R.edge_rows(4)[1][3:4]                        # one row = one block (a maximum one ulp below a power of two)
    w_t1, w_t2 = R.transposed_weight(2, 1, 1), R.transposed_weight(34, 2, 33)   # one block; 2 x 2 tiles x 2 taps
    s, m = _storage(288, 99), _gather_map(288, 7, 514, 99)
    m2 = _gather_map(288, 6, 2, 98)
    specs = [("rows_f16", "rows", w_rows, R.F16), ("t_one_block", "t", w_t1, [0]), ("gather_bf16", "gather", m, R.BF16),
             ("rows_bf16_one_block", "rows", w_one, R.BF16), ("t_tiles", "t", w_t2, [1, 0]), ("gather_f16", "gather", m2, R.F16),
             ("rows_f16_one_block", "rows", w_one, R.F16), ("rows_bf16", "rows", w_rows, R.BF16)]
    sd = list(_layouts(s, dev))[1][1]
    for order in (list(range(len(specs))), [7, 6, 0, 3, 2, 1, 5, 4]):
        jobs, outs = [], []
        for i in order:
            name, kind, data, arg = specs[i]
            if kind == "t":
                cout, taps, cin = data.shape
                src = _up(data, dev)
                hi, lo = Guarded(cin * len(arg) * cout, dev), Guarded(cin * len(arg) * cout, dev)
                jobs.append((src.data_ptr(), wp._job_transposed(src, src, hi.view, lo.view, cout, taps, cin, arg)))
                want = tuple(e.reshape(-1) for e in R.transposed_ref(data, arg)) + (None,)
                outs.append((name, R.BF16, src, hi, lo, None, want))
                continue
            if kind == "rows":
                src, idx, (rows, k) = _up(data, dev), None, data.shape
                want = R.rows_ref(data, arg)
            else:
                src, idx, (rows, k) = sd, _up(data, dev), data.shape
                want = R.gather_ref(s, data, arg)
            hi, lo = Guarded(rows * k, dev), Guarded(rows * k, dev)
            ws = Guarded(rows, dev, wide=True) if arg == R.F16 else None
            jobs.append((src.data_ptr(), wp._job_rows(src, src, hi.view, lo.view, None if ws is None else ws.view, arg == R.F16, rows, k, idx_map=idx)))
            outs.append((name, arg, (src, idx), hi, lo, ws, tuple(None if e is None else e.reshape(-1) for e in want)))
        blocks = [j["blocks"] for _, j in jobs]
        assert 1 in blocks[1:-1] and max(blocks) > 30, blocks  # a one-block job between many-block jobs
        tabs = job_tables._JobTable("the test's plane table", job_tables._PLANE_JOB, ops.weight_planes_job_bytes)
        tab = tabs.get(tuple((base + j["off"],) + j["fields"] + j["sel"] for base, j in jobs), dev, lambda: wp.pack_plane_jobs(jobs))
        assert tab.blocks == sum(blocks)
        ops.weight_planes_multi(tab.jobs, tab.blk2job, tab.blocks)
        torch.cuda.synchronize()
        for name, plane, _, hi, lo, ws, want in outs:
            got_hi, got_lo = hi.words(name), lo.words(name)
            assert (got_hi != SENT).all() and (got_lo != SENT).all(), "%s: words left unwritten" % name
            _same(got_hi, want[0], plane, name + " hi")
            _same(got_lo, want[1], plane, name + " lo")
            if ws is not None:
                assert (R.bits32(ws.words(name).view(np.float32)) == R.bits32(want[2])).all(), name + " wscale"


# ---------------------------------------------------------------- clip planes: ops.clip_planes_f32
CLIP_SHAPES = [(1, 3, 1, 1, n) for n in (1, 255, 256, 257, 513)] + [(2, 3, 3, 5, 7)]
LAYOUTS = ["ncdhw", "ndhwc", "window", "expanded"]


def _clip_view(x, layout, dev):
    """The values of x (numpy [B, 3, T, H, W]) behind a device view of the named layout -> (view, the values it shows)."""
    t = torch.from_numpy(x)
    if layout == "ncdhw":
        return t.to(dev), x
    if layout == "ndhwc":
        v = t.to(dev).contiguous(memory_format=torch.channels_last_3d)
        assert v.stride()[1] == 1
        return v, x
    if layout == "window":  # inside a larger tensor of another value, every second column
        b, c, tt, h, w = x.shape
        big = torch.full((b + 1, c, tt + 2, h + 3, 2 * w + 5), 777.0, device=dev)
        v = big[1:, :, 1:1 + tt, 2:2 + h, 3:3 + 2 * w:2]
        v.copy_(t)
        return v, x
    if layout == "expanded":  # stride 0: every clip of the batch (3 of them) is the first one's memory
        v = t[:1].to(dev).expand(3, -1, -1, -1, -1)
        assert v.stride()[0] == 0
        return v, np.broadcast_to(x[:1], (3,) + x.shape[1:])
    raise KeyError(layout)


def _check_clip(avt, v, shown, plane, what):
    hi, lo = avt.ops.clip_planes_f32(v, plane)
    torch.cuda.synchronize()
    e_hi, e_lo = R.clip_ref(shown, plane)
    zero = R.split(np.zeros(1, np.float32), plane)
    ghi, glo = R.words(hi), R.words(lo)
    assert (ghi[..., 3] == zero[0][0]).all() and (glo[..., 3] == zero[1][0]).all(), what + ": channel 3 is not the split of zero"
    _same(ghi, e_hi, plane, what + " hi")
    _same(glo, e_lo, plane, what + " lo")


@_p("layout", LAYOUTS)
@_p("shape", CLIP_SHAPES, ids=lambda s: "x".join(map(str, s)))
@_p("name,plane", PLANES)
def test_clip_planes_at_block_edges_in_every_layout(avt, dev, name, plane, shape, layout):
    x = R.clip_values(shape, key=shape[-1])
    v, shown = _clip_view(x, layout, dev)
    _check_clip(avt, v, shown, plane, "%s %s %s" % (name, shape, layout))


@_p("name,plane", PLANES)
def test_clip_planes_with_a_batch_stride_beyond_2_to_31(avt, dev, name, plane):
    """Two clips 2^31 + 24 elements apart in an uninitialised allocation of 8.6 GB, of which only the two clips are written."""
    shape = (2, 3, 3, 5, 7)
    x = R.clip_values(shape, key=7)
    per = int(np.prod(shape[1:]))
    sb = (1 << 31) + 24
    big = torch.empty(sb + per, dtype=torch.float32, device=dev)
    v = big.as_strided(shape, (sb, 105, 35, 7, 1))
    v.copy_(torch.from_numpy(x))
    assert v.stride()[0] > (1 << 31)
    _check_clip(avt, v, x, plane, "%s batch stride 2^31 + 24" % name)
    del v, big
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- the scale reaches the right channel
S3, P3, ONE = (1, 3, 3), (0, 1, 1), (1, 1, 1)
# id -> (cin, cout, kernel, stride, pad, input dims (B, T, H, W), settings, what must have happened)
FORMS = {
    # "tile": the M tile's rows, read back from the library (64 output channels always run the 128-row tile, whatever the switch says:
    # the 64-row tile is for wider layers, so the pair at 128 channels is the one that runs two different kernels); "rides": whether
    # the BatchNorm statistics are left by the convolution's own epilogue when stats= is given (_conv_x3_rows)
    "general_64_64_k133_switch_off": (64, 64, S3, ONE, P3, (2, 2, 8, 8), {"small_tile": 0}, {"form": 1, "tile": 128, "rides": True}),
    "general_64_64_k133_switch_on": (64, 64, S3, ONE, P3, (2, 2, 8, 8), {"small_tile": 1}, {"form": 1, "tile": 128, "rides": True}),
    "general_64_128_k133_tile128": (64, 128, S3, ONE, P3, (2, 2, 8, 8), {"small_tile": 0}, {"form": 1, "tile": 128, "rides": True}),
    "general_64_128_k133_tile64": (64, 128, S3, ONE, P3, (2, 2, 8, 8), {"small_tile": 1}, {"form": 1, "tile": 64, "rides": True}),
    "temporal_64_64_k311": (64, 64, (3, 1, 1), ONE, (1, 0, 0), (2, 2, 8, 8), {}, {"form": 1, "rides": True}),
    "grouped_8_8_k133": (8, 8, S3, ONE, P3, (2, 2, 8, 8), {}, {"form": 4, "rides": True}),
    "grouped_wide_16_64_k133": (16, 64, S3, ONE, P3, (2, 2, 8, 8), {}, {"form": 4, "rides": False}),  # (4 x 64 columns > _STAT_GROUP_COLS)
    "grouped_temporal_8_32_k511": (8, 32, (5, 1, 1), ONE, (2, 0, 0), (2, 2, 8, 8), {}, {"form": 1, "rides": True}),  # (32 outputs: _conv_form stops at g = 1)
    "grouped_temporal_8_8_k511": (8, 8, (5, 1, 1), ONE, (2, 0, 0), (2, 2, 8, 8), {}, {"form": 4, "rides": True}),
    "pointwise_64_256": (64, 256, ONE, ONE, (0, 0, 0), (2, 2, 8, 8), {}, {"form": 0, "calls": "pw_f32", "rides": True}),
    "pointwise_256_64": (256, 64, ONE, ONE, (0, 0, 0), (2, 2, 8, 8), {}, {"form": 0, "calls": "pw_f32", "rides": True}),
    "stem_patch_3_8_kt5": (3, 8, (5, 7, 7), (1, 2, 2), (2, 3, 3), (1, 4, 64, 64), {}, {"calls": "stem_fwd_patch", "rides": False}),
    "stem_patch_3_64_kt1": (3, 64, (1, 7, 7), (1, 2, 2), (0, 3, 3), (1, 4, 64, 64), {}, {"calls": "stem_fwd_patch", "rides": False}),
    "stem_generic_3_64_kt5": (3, 64, (5, 7, 7), (1, 2, 2), (2, 3, 3), (2, 4, 16, 16), {"stem_patch": 0}, {"no_calls": "stem_fwd_patch", "rides": True}),
}


def _shift(co):
    return (5 * co) % 13 - 6


def _run_form(dev, case, weight, with_stats):
    """conv3d forward (then bn_act when with_stats) under the case's settings, from an empty plane cache -> (y, running_mean | None)."""
    from avtex import ops, train_ops

    cin, cout, kernel, stride, pad, dims, sets, must = FORMS[case]
    conv = nn.Conv3d(cin, cout, kernel, stride=stride, padding=pad, bias=False).to(dev).to(memory_format=torch.channels_last_3d).train()
    with torch.no_grad():
        conv.weight.copy_(weight)
    bn = nn.BatchNorm3d(cout).to(dev).train() if with_stats else None
    g = torch.Generator().manual_seed(cin * 1000 + cout)
    x = torch.randn(dims[0], cin, *dims[1:], generator=g).to(dev)
    if cin != 3:
        x = x.contiguous(memory_format=torch.channels_last_3d)
        assert train_ops._conv_form(cin, cout, kernel, stride, pad, dims[3]) == must["form"]
    keep_tile = ops.conv_x3_set_small_tile(sets.get("small_tile", 1))
    keep_patch, train_ops._STEM_PATCH = train_ops._STEM_PATCH, sets.get("stem_patch", 1)
    train_ops.invalidate_weight_cache(drop=True)
    before = dict(train_ops.CALLS)
    try:
        if "tile" in must:  # rows of statistics partials = M tiles: which tile this layer runs on under the switch
            from avtex import _lib
            m = dims[0] * dims[1] * dims[2] * dims[3]
            assert _lib.lib().avt_conv3d_igemm_x3_f32_stat_rows(cout, cin * kernel[0] * kernel[1] * kernel[2], m, 1) == -(-m // must["tile"])
        with torch.no_grad(), train_ops.bn_replicas(1):
            assert train_ops.conv_fusable(x, conv)
            y = train_ops.conv3d(x, conv, stats=bn)
            rides = hasattr(y, "_avt_stats")
            if bn is not None:
                train_ops.bn_act(y, bn)
        torch.cuda.synchronize()
    finally:
        ops.conv_x3_set_small_tile(keep_tile)
        train_ops._STEM_PATCH = keep_patch
        train_ops.invalidate_weight_cache(drop=True)
    assert train_ops.CALLS["conv_fwd_x3"] == before["conv_fwd_x3"] + 1
    if "calls" in must:
        assert train_ops.CALLS[must["calls"]] == before[must["calls"]] + 1
    if "no_calls" in must:
        assert train_ops.CALLS[must["no_calls"]] == before[must["no_calls"]]
    return y, (None if bn is None else bn.running_mean.clone()), rides


@_p("with_stats", [False, True], ids=["plain", "stats"])
@_p("case", sorted(FORMS))
def test_a_rows_scale_reaches_its_own_output_channel(avt, dev, case, with_stats):
    """Row co of the weight times 2^s(co), s(co) = (5 co) % 13 - 6: identical planes, wscale[co] times 2^s — so output channel co is the
    first run's times 2^s(co) BIT FOR BIT.  A scale applied one channel off, or one scale to a whole tile, cannot pass: neighbouring
    channels differ by 2^5 or 2^-8.  With stats= the running mean of the BatchNorm behind it scales too, within the tolerance
    tests/test_gpu_bn_train.py holds the fused pass to (2e-5 of the largest entry; partial sums regroup, so not exactly)."""
    cin, cout, kernel = FORMS[case][:3]
    torch.manual_seed(cout * 31 + cin)
    w = nn.Conv3d(cin, cout, kernel, bias=False).weight.detach().to(dev)
    two_s = torch.tensor([2.0 ** _shift(co) for co in range(cout)], device=dev)
    y1, rm1, rides1 = _run_form(dev, case, w, with_stats)
    y2, rm2, rides2 = _run_form(dev, case, w * two_s.view(-1, 1, 1, 1, 1), with_stats)
    assert y1.shape == y2.shape and y1.shape[1] == cout and bool(torch.isfinite(y2).all())
    assert bool((y1.abs().flatten(2).amax(2).amax(0) > 0).all()), "a channel of zeros shows nothing"
    want = y1 * two_s.view(1, -1, 1, 1, 1)
    bad = (want != y2).flatten(2).any(2).any(0).nonzero().flatten().tolist()
    assert not bad, "%s: channels %s are not the first run's times 2^s" % (case, bad[:8])
    if with_stats:
        err = float((rm2 / two_s - rm1).abs().max()) / float(rm1.abs().max())
        print("%s: statistics on the epilogue %s; running_mean / 2^s against the first run: %.3g of the largest entry" % (case, rides1, err))
        assert rides1 == rides2 == FORMS[case][7]["rides"], "the statistics did not come from where this case expects them"
        assert err <= 2e-5 and float(rm1.abs().max()) > 0


def test_rows_spanning_2_to_the_80_against_float64(avt, dev):
    """The general tile with weight rows scaled by 2^-40 .. 2^40 (wscale from 2^-55 to 2^26) against a float64 convolution.  Bound per
    output, from the formats: each product carries the two splits and the dropped lo * lo term, 3 * 2^-22 of |x| |w|, and an fp32
    accumulation of K = 576 terms in whatever order at most K * 2^-24 of sum |x| |w|."""
    case = "general_64_64_k133_switch_on"
    cin, cout, kernel, stride, pad, dims = FORMS[case][:6]
    torch.manual_seed(5)
    exps = torch.tensor([(7 * co) % 81 - 40 for co in range(cout)])
    assert int(exps.min()) == -40 and int(exps.max()) == 40
    w = nn.Conv3d(cin, cout, kernel, bias=False).weight.detach() * (2.0 ** exps.double()).float().view(-1, 1, 1, 1, 1)
    y, _, _ = _run_form(dev, case, w.to(dev), False)
    g = torch.Generator().manual_seed(cin * 1000 + cout)
    x = torch.randn(dims[0], cin, *dims[1:], generator=g)  # _run_form's input
    y64 = F.conv3d(x.double(), w.double(), padding=pad)
    mag = F.conv3d(x.double().abs(), w.double().abs(), padding=pad)
    K = cin * 9
    ratio = ((y.cpu().double() - y64).abs() / ((3 * 2.0 ** -22 + K * 2.0 ** -24) * mag)).flatten(2).amax(2).amax(0)
    print("rows spanning 2^-40 .. 2^40: worst error / bound %.4f (channel %d, row scale 2^%d)" % (float(ratio.max()), int(ratio.argmax()), int(exps[ratio.argmax()])))
    assert float(ratio.max()) <= 1.0
