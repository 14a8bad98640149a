"""The memory-bound helpers in front of and behind every inference encoder, one by one at their edges: the stem and VGGish
max-pools and the head's average pool (csrc/pool.hip), and clip packing (csrc/clip_pack.hip).  The pools are compared with
F.max_pool2d on the joined values (a max of representable values is representable: exact), the head mean and the packing
bit for bit with the restatements of tests/pack_pool_refs.py, which tests/test_pack_pool_refs_host.py pins to the oracle."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pack_pool_refs as R

pytestmark = pytest.mark.gpu

MODES = ["bf16", "bf16x3", "f16x3"]  # one bf16 plane; (hi, lo) bf16 planes; (hi, lo) fp16 planes
SENT = 0xC0E0  # the sentinel word around every output slice: bf16 -7.0 (fp16 -2.4375), never a result
FILL = 1.0e4   # what lies beyond the input's channel slice and in dropped rows / columns: it must never win a max
INF, NAN = {"bf16x3": 0x7F80, "f16x3": 0x7C00}, {"bf16x3": 0x7FC0, "f16x3": 0x7E00}


def _gen(*key):
    return torch.Generator().manual_seed(int(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key))) + 37)


def _randn(*shape, key=()):
    return torch.randn(*shape, generator=_gen(*shape, *key)).numpy()


def _encode(x, mode):
    """fp32 array -> the words of the plane(s) that carry it: [hi] for bf16, [hi, lo] for the plane pairs."""
    if mode == "bf16":
        return [R._rne_bf16(np.ascontiguousarray(x, dtype=np.float32))]
    return list(R.split(x, R.PLANE[mode]))


def _decode(planes, mode):
    if mode == "bf16":
        return R.plane_f32(planes[0], R.BF16)
    return R.join(planes[0], planes[1], R.PLANE[mode])


def _up(wd, dev):
    return R.plane_tensor(wd).to(dev)


def _pool_ref(v, ks):
    """fp32 [n, h, w, c] -> F.max_pool2d (3, 2, 1) or (2, 2) on the CPU, NHWC again."""
    t = torch.from_numpy(np.ascontiguousarray(v)).permute(0, 3, 1, 2)
    return (F.max_pool2d(t, 3, 2, 1) if ks == 3 else F.max_pool2d(t, 2, 2)).permute(0, 2, 3, 1).contiguous()


def _run_pool(ops, dev, mode, planes, geom, ks=3, wide_in=False, wide_out=False, tgroup=1, frame_idx=None, bt=None):
    """planes: words [frames, h, w, c] of the input; -> (output plane words [bt * tgroup, ho, wo, c / tgroup] ...).  wide_in:
    the input rows are c + 8 wide, the last 8 columns hold FILL.  wide_out: the output is columns 8 .. 8 + c / tgroup of rows
    c / tgroup + 16 wide; the sentinel columns on both sides must come back untouched, in every plane."""
    frames, h, w, c = geom
    bt = frames if bt is None else bt
    cg = c // tgroup
    ho, wo = ((h - 1) // 2 + 1, (w - 1) // 2 + 1) if ks == 3 else (h // 2, w // 2)
    ldi, ldo, col = c + (8 if wide_in else 0), cg + (16 if wide_out else 0), 8 if wide_out else 0
    fill = _encode(np.full(1, FILL, np.float32), mode)
    ins, outs = [], []
    for wd, fw in zip(planes, fill):
        buf = np.full((frames * h * w, ldi), fw[0], np.uint16)
        buf[:, :c] = wd.reshape(-1, c)
        ins.append(_up(buf, dev))
        outs.append(_up(np.full((bt * tgroup * ho * wo, ldo), SENT, np.uint16), dev))
    ip, op = [t.data_ptr() for t in ins], [t.data_ptr() + 2 * col for t in outs]
    if mode == "bf16":
        assert frame_idx is None
        if ks == 3:
            ops.maxpool_hw3s2(ip[0], op[0], bt, h, w, c, ldi, ldo, tgroup=tgroup)
        else:
            ops.maxpool_hw2s2(ip[0], op[0], bt, h, w, c, ldi, ldo)
    elif ks == 3:
        fi = None if frame_idx is None else torch.tensor(frame_idx, dtype=torch.int32, device=dev)
        ops.maxpool_hw3s2_x3(ip, op, bt, h, w, c, ldi, ldo, R.PLANE[mode], tgroup=tgroup, frame_idx=fi)
    else:
        ops.maxpool_hw2s2_x3(ip, op, bt, h, w, c, ldi, ldo, R.PLANE[mode])
    torch.cuda.synchronize()
    res = []
    for t in outs:
        wd = R.words(t)
        assert (wd[:, :col] == SENT).all() and (wd[:, col + cg:] == SENT).all(), "the pool wrote outside its column slice"
        res.append(np.ascontiguousarray(wd[:, col : col + cg]).reshape(bt * tgroup, ho, wo, cg))
    return res


def _check_pool(ops, dev, mode, x, ks=3, tgroup=1, frame_idx=None, planes=None, **kw):
    """x fp32 [frames, h, w, c] (or ready plane words): run, compare with torch.equal; finite results must also be the
    restated split of the maximum, word for word."""
    planes = _encode(x, mode) if planes is None else planes
    geom = planes[0].shape
    v = _decode(planes, mode)
    frames, h, w, c = geom
    if tgroup > 1:  # [bt, h, w, tgroup, c/tgroup] -> [bt * tgroup, h, w, c/tgroup]
        v = np.ascontiguousarray(v.reshape(frames, h, w, tgroup, c // tgroup).transpose(0, 3, 1, 2, 4)).reshape(frames * tgroup, h, w, -1)
    bt = None
    if frame_idx is not None:
        v, bt = v[np.asarray(frame_idx)], len(frame_idx)
    ref = _pool_ref(v, ks)
    got_planes = _run_pool(ops, dev, mode, planes, geom, ks=ks, tgroup=tgroup, frame_idx=frame_idx, bt=bt, **kw)
    got = torch.from_numpy(_decode(got_planes, mode))
    assert got.shape == ref.shape
    return got, ref, got_planes


def _assert_exact(got, ref, got_planes, mode):
    assert torch.equal(got, ref)
    for g, e in zip(got_planes, _encode(ref.numpy(), mode)):
        assert np.array_equal(g, e), "the output planes are not the split of the maximum"


# ---------------------------------------------------------------- 3x3 stride-2 pools
SHAPES3 = [(1, 1, 1), (2, 1, 2), (2, 2, 1), (3, 5, 4), (2, 9, 10), (1, 8, 7)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bt,h,w", SHAPES3)
def test_maxpool3_shapes_and_slices(avt, dev, mode, bt, h, w):
    """Every extent from 1 (all taps clamped) to more than one window, 1 to 9 channel chunks, input and output as column
    slices of wider rows, on unit-normal and on all-negative data (a pool that pads with zeros fails the latter)."""
    from avtex import ops

    for c in (8, 16, 72):
        for neg in (False, True):
            x = _randn(bt, h, w, c, key=(neg,))
            x = -np.abs(x) - 1 if neg else x
            for wide_in in (False, True):
                for wide_out in (False, True):
                    got, ref, gp = _check_pool(ops, dev, mode, x, wide_in=wide_in, wide_out=wide_out)
                    _assert_exact(got, ref, gp, mode)
                    assert not neg or (got <= -1).all()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c,tgroup", [(16, 2), (32, 2), (32, 4), (64, 4)])
def test_maxpool3_ungroups_time_grouped_rows(avt, dev, mode, c, tgroup):
    """tgroup > 1 (the fast stem is c = 32, tgroup = 4): input row = tgroup frames of c / tgroup channels, output = plain
    frames b * tgroup + j.  Every (frame, group) carries its own offset, so a swapped frame and group is off by whole units."""
    from avtex import ops

    for bt, h, w in [(1, 1, 1), (3, 5, 4), (2, 9, 10)]:
        x = _randn(bt, h, w, tgroup, c // tgroup, key=(tgroup,))
        x = x + 8.0 * (np.arange(bt)[:, None] * tgroup + np.arange(tgroup)[None, :])[:, None, None, :, None].astype(np.float32)
        for wide_in, wide_out in [(False, False), (True, True), (False, True)]:
            got, ref, gp = _check_pool(ops, dev, mode, x.reshape(bt, h, w, c), tgroup=tgroup, wide_in=wide_in, wide_out=wide_out)
            _assert_exact(got, ref, gp, mode)


@pytest.mark.parametrize("mode", MODES[1:])
@pytest.mark.parametrize("table,idx", [(3, [2, 0, 0, 1, 2, 1, 0]), (5, [3, 1, 1, 3, 1, 3, 1])])
def test_maxpool3_x3_frame_index(avt, dev, mode, table, idx):
    """frame_idx: output frame b pools table frame idx[b]; repeated, out of order, and over a table with frames that no entry
    names (they hold FILL and must not show)."""
    from avtex import ops

    for h, w, c in [(5, 4, 8), (9, 10, 16), (1, 2, 72)]:
        x = _randn(table, h, w, c) + 8.0 * np.arange(table, dtype=np.float32)[:, None, None, None]
        x[[f for f in range(table) if f not in idx]] = FILL
        for wide in (False, True):
            got, ref, gp = _check_pool(ops, dev, mode, x, frame_idx=idx, wide_in=wide, wide_out=wide)
            _assert_exact(got, ref, gp, mode)
            assert (got < FILL).all()


# (position, sign bit) in a [2, 9, 10, 16] input: a corner tap (one window) and an interior tap (even row, odd column: two
# windows; odd row, odd column: four) for each sign, in frames and channels of their own
SPECIAL_AT = [((0, 0, 0, 1), 0), ((0, 4, 5, 3), 0x8000), ((1, 8, 9, 2), 0x8000), ((1, 3, 5, 5), 0)]


@pytest.mark.parametrize("mode", MODES[1:])
def test_maxpool3_x3_nan_reaches_the_output(avt, dev, mode):
    """The plane-pair pools promise that a poisoned activation reaches the embedding.  One NaN in a wave also sends the whole
    wave down split_pairs' careful branch: every other value must come out as before."""
    from avtex import ops

    hi, lo = _encode(_randn(2, 9, 10, 16), mode)
    for pos, sign in SPECIAL_AT:
        hi[pos], lo[pos] = NAN[mode] | sign, 0
    got, ref, gp = _check_pool(ops, dev, mode, None, planes=[hi, lo], wide_in=True, wide_out=True)
    gn, rn = torch.isnan(got), torch.isnan(ref)
    assert torch.equal(gn, rn) and int(rn.sum()) == 1 + 2 + 1 + 4
    assert torch.equal(got[~gn], ref[~rn])
    for g, e in zip(gp, _encode(ref.numpy(), mode)):
        assert np.array_equal(g[~rn.numpy()], e[~rn.numpy()])


@pytest.mark.parametrize("mode", MODES)
def test_maxpool3_infinities(avt, dev, mode):
    """+-inf at the same taps.  fp16 planes and the bf16 plane keep +inf an infinity; bf16 PLANE PAIRS have no special case
    (csrc/split_planes.h: the low plane of an infinity is inf - inf), so there +inf arrives as hi = +inf with a NaN beside it —
    still not a finite number.  -inf never wins a window that holds anything else.  Everything else is exact."""
    from avtex import ops

    planes = _encode(_randn(2, 9, 10, 16), mode)
    inf = INF.get(mode, 0x7F80)
    for pos, sign in SPECIAL_AT:
        planes[0][pos] = inf | sign
        if len(planes) == 2:
            planes[1][pos] = 0
    got, ref, gp = _check_pool(ops, dev, mode, None, planes=planes, wide_in=True, wide_out=True)
    pinf = torch.isinf(ref)
    assert int(pinf.sum()) == 1 + 4 and (ref[pinf] > 0).all()
    assert torch.equal(got[~pinf], ref[~pinf])
    if mode == "bf16x3":
        assert (gp[0][pinf.numpy()] == inf).all() and not torch.isfinite(got[pinf]).any()
    else:
        assert torch.equal(got, ref)
    for g, e in zip(gp, _encode(ref.numpy(), mode)):
        assert np.array_equal(g[~pinf.numpy()], e[~pinf.numpy()])


def test_maxpool3_f16x3_range_edges(avt, dev):
    """The ends of the fp16 range, and windows whose low planes (rows 7, 8: values near 2^-5) or both planes (rows 3 to 5: values
    near 2^-16) are fp16 subnormals: the pool must neither clamp early nor flush them."""
    from avtex import ops

    x = _randn(2, 9, 10, 16)
    x[:, 3:6] *= np.float32(2.0 ** -16)  # the windows of output row 2 hold nothing else
    x[:, 7:9] *= np.float32(2.0 ** -5)   # nor do those of output row 4
    x[0, 0, 0, 0], x[0, 1, 9, 1], x[1, 1, 2, 2] = 65504.0, -65504.0, 65504.0
    x[1, 0:2, 5:8, 3] = -65504.0         # one whole window (output row 0, column 3)
    hi, lo = _encode(x, "f16x3")
    sub = lambda wd: ((wd & 0x7C00) == 0) & ((wd & 0x03FF) != 0)
    assert sub(hi[:, 3:6]).mean() > 0.9 and sub(lo[:, 7:9]).mean() > 0.9
    got, ref, gp = _check_pool(ops, dev, "f16x3", x, wide_in=True, wide_out=True)
    _assert_exact(got, ref, gp, "f16x3")
    assert (got == 65504.0).sum() >= 2 and got[1, 0, 3, 3] == -65504.0
    assert sub(gp[0][:, 2]).mean() > 0.9 and sub(gp[1][:, 4]).mean() > 0.9


# ---------------------------------------------------------------- 2x2 pools
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("h,w", [(2, 2), (3, 2), (2, 3), (7, 5), (25, 16)])
def test_maxpool2_shapes_slices_and_dropped_edges(avt, dev, mode, h, w):
    """MaxPool2d(2, 2), floor mode: an odd last row / column is dropped.  It holds FILL (and, for the plane pairs, NaN): neither
    may reach the output."""
    from avtex import ops

    for c in (8, 24, 72):
        for drop in ("fill", "nan") if mode != "bf16" and (h % 2 or w % 2) else ("fill",):
            planes = _encode(_randn(2, h, w, c), mode)
            edge = _encode(np.full(1, FILL, np.float32), mode) if drop == "fill" else [[NAN[mode]], [0]]
            for wd, e in zip(planes, edge):
                if h % 2:
                    wd[:, h - 1] = e[0]
                if w % 2:
                    wd[:, :, w - 1] = e[0]
            for wide_in in (False, True):
                for wide_out in (False, True):
                    got, ref, gp = _check_pool(ops, dev, mode, None, ks=2, planes=[p.copy() for p in planes], wide_in=wide_in,
                                               wide_out=wide_out)
                    _assert_exact(got, ref, gp, mode)
                    assert (got < 100).all()


# ---------------------------------------------------------------- above 65536 * 256 output chunks: the grid-stride loop
GS = (33, 225, 225, 320)  # 33 * 113 * 113 * 40 = 16,855,080 chunks, the smallest such total above 2^24 = 16,777,216


def test_maxpool3_bf16_grid_stride(avt, dev):
    """Above 65536 workgroups the kernel walks its outputs in a grid-stride loop (production: 166 windows x 8 frames x 56 x 56 x
    8 chunks = 33 M).  Reference: torch's own max_pool2d on the device, on the bf16 -> fp32 values, three frames at a time."""
    from avtex import ops

    bt, h, w, c = GS
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    assert bt * ho * wo * (c // 8) > 65536 * 256 >= (bt - 1) * ho * wo * (c // 8)
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.empty((bt, h, w, c), dtype=torch.bfloat16, device=dev)
    for i in range(0, bt, 3):
        x[i : i + 3] = torch.randn(x[i : i + 3].shape, generator=g, device=dev).to(torch.bfloat16) + float(i)
    out = torch.full((bt, ho, wo, c), -7.0, dtype=torch.bfloat16, device=dev)
    ops.maxpool_hw3s2(x.data_ptr(), out.data_ptr(), bt, h, w, c, c, c)
    torch.cuda.synchronize()
    for i in range(0, bt, 3):
        ref = F.max_pool2d(x[i : i + 3].float().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
        assert torch.equal(out[i : i + 3].float(), ref), "frames %d.." % i


def test_maxpool3_x3_grid_stride(avt, dev):
    """The same total through the plane-pair kernel (fp16 planes), driven by frame_idx over a two-frame table so that the input is
    small: both output planes equal index_select of the table's pooled and split frames, compared on the device."""
    from avtex import ops

    bt, h, w, c = GS
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    g = torch.Generator(device=dev).manual_seed(6)
    x = torch.randn((2, h, w, c), generator=g, device=dev)
    hi = x.to(torch.float16)
    lo = (x - hi.float()).to(torch.float16)
    pooled = F.max_pool2d((hi.float() + lo.float()).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()
    eh = pooled.to(torch.float16)  # |x| < 65504: split2's clamps and selects are identities
    el = (pooled - eh.float()).to(torch.float16)
    idx = torch.tensor([(i * i + i // 3) % 2 for i in range(bt)], dtype=torch.int32, device=dev)
    assert 0 < int(idx.sum()) < bt
    oh = torch.full((bt, ho, wo, c), float("nan"), dtype=torch.float16, device=dev)
    ol = torch.full_like(oh, float("nan"))
    ops.maxpool_hw3s2_x3((hi.data_ptr(), lo.data_ptr()), (oh.data_ptr(), ol.data_ptr()), bt, h, w, c, c, c, R.F16, frame_idx=idx)
    torch.cuda.synchronize()
    assert torch.equal(oh.view(torch.int16), eh.index_select(0, idx.long()).view(torch.int16))
    assert torch.equal(ol.view(torch.int16), el.index_select(0, idx.long()).view(torch.int16))


# ---------------------------------------------------------------- head mean
def _run_mean(ops, dev, mode, planes, b, P, C, wide_in):
    """planes: words [b, P, C] -> (the kernel's [b, C] fp32, the restatement's), the kernel writing columns 8 .. 8 + C of a
    [b, C + 24] table whose other columns must stay as they were."""
    ldi = C + (8 if wide_in else 0)
    fill = _encode(np.full(1, FILL, np.float32), mode)
    ins = []
    for wd, fw in zip(planes, fill):
        buf = np.full((b * P, ldi), fw[0], np.uint16)
        buf[:, :C] = wd.reshape(-1, C)
        ins.append(_up(buf, dev))
    out = torch.full((b, C + 24), -7.0, dtype=torch.float32, device=dev)
    if mode == "bf16":
        ops.mean_positions(ins[0].data_ptr(), b, P, C, ldi, out, 8)
    else:
        ops.mean_positions_x3([t.data_ptr() for t in ins], b, P, C, ldi, out, 8, R.PLANE[mode])
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert (o[:, :8] == -7.0).all() and (o[:, 8 + C:] == -7.0).all(), "the mean wrote outside its column slice"
    v = _decode(planes, mode)
    return np.ascontiguousarray(o[:, 8 : 8 + C]), np.stack([R.mean_positions(v[i]) for i in range(b)])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("P", [1, 7, 31, 32, 33, 392])
def test_mean_positions_bit_for_bit(avt, dev, mode, P):
    """include/avt.h promises a deterministic summation order; this is the order: 32 row groups (empty ones below P = 32), then a
    fixed 32-term reduce, then one division.  Channel counts cover a partial last block of 64 behind full ones."""
    from avtex import ops

    for C in (8, 24, 64, 72, 136):
        for b in (1, 3):
            planes = _encode(_randn(b, P, C, key=(1,)) + np.float32(0.25), mode)
            for wide_in in (False, True):
                got, exp = _run_mean(ops, dev, mode, planes, b, P, C, wide_in)
                bad = R.bits(got) != R.bits(exp)
                assert not bad.any(), "P %d C %d b %d: %d means differ, first %r != %r" % (P, C, b, bad.sum(), got[bad][0], exp[bad][0])


@pytest.mark.parametrize("mode", MODES)
def test_mean_positions_nan_and_inf_stay_in_their_channel(avt, dev, mode):
    from avtex import ops

    b, P, C = 3, 33, 72
    planes = _encode(_randn(b, P, C, key=(2,)), mode)
    for pos, word in [((0, 5, 3), 0x7FC0 if mode != "f16x3" else 0x7E00), ((1, 32, 70), INF.get(mode, 0x7F80)),
                      ((2, 0, 64), INF.get(mode, 0x7F80) | 0x8000)]:
        planes[0][pos] = word
        if len(planes) == 2:
            planes[1][pos] = 0
    got, exp = _run_mean(ops, dev, mode, planes, b, P, C, True)
    assert np.isnan(got[0, 3]) and got[1, 70] == np.inf and got[2, 64] == -np.inf
    assert np.isfinite(got).sum() == got.size - 3
    fin = np.isfinite(exp)
    assert np.array_equal(np.isfinite(got), fin) and np.array_equal(R.bits(got)[fin], R.bits(exp)[fin])


# ---------------------------------------------------------------- clip packing
def _to_ndhwc(ref):  # [n, 3, T, hw, hw] -> [n, T, hw, hw, 3]
    return np.ascontiguousarray(ref.transpose(0, 2, 3, 4, 1))


def _check_pack(ops, dev, frames, starts, win_len, hw, mean=0.45, std=0.225, bgr=True):
    n_frames = frames.shape[0]
    table = R.pack_frames(frames, hw, mean, std, bgr)
    refs = [R.pack_clip(frames, int(s), win_len, hw, mean, std, bgr, table=table) for s in starts]
    ref = [np.stack([r[0] for r in refs]), np.stack([r[1] for r in refs])]
    assert ref[0].shape == (len(starts), 3, 8, hw, hw) and ref[1].shape == (len(starts), 3, 32, hw, hw)
    fd = torch.from_numpy(frames).to(dev)
    kw = dict(out_hw=hw, mean=mean, std=std, bgr=bgr)
    d_starts = torch.tensor(starts, dtype=torch.int32, device=dev)
    f32 = ops.clip_pack(fd, starts, win_len, dtype=torch.float32, **kw)
    b16 = ops.clip_pack(fd, starts, win_len, dtype=torch.bfloat16, **kw)
    g32 = ops.clip_pack_gather(fd, d_starts, win_len, dtype=torch.float32, **kw)
    g16 = ops.clip_pack_gather(fd, d_starts, win_len, dtype=torch.bfloat16, **kw)
    c16 = ops.clip_pack(fd, starts, win_len, layout="ndhwc4", **kw)
    px = {m: ops.clip_pack(fd, starts, win_len, layout="ndhwc4", planes=m, **kw) for m in ("bf16x3", "f16x3")}
    torch.cuda.synchronize()
    for k, r in enumerate(ref):
        what = "%s pathway, %d frames %r -> %d, windows %r of %d" % (("slow", "fast")[k], n_frames, frames.shape[1:3], hw, list(starts), win_len)
        rt = torch.from_numpy(r)
        for got in (f32[k], g32[k]):  # fp32: bit for bit, plan form and gather form
            assert got.shape == rt.shape and got.dtype == torch.float32
            assert np.array_equal(R.bits(got.cpu().numpy()), R.bits(r)), what
        for got in (b16[k], g16[k]):  # bf16: the correctly rounded fp32 result, every element
            assert got.shape == rt.shape and torch.equal(got.cpu().view(torch.int16), rt.bfloat16().view(torch.int16)), what
        rl = _to_ndhwc(r)
        got = c16[k].cpu()
        assert got.shape == rl.shape[:4] + (4,) and (got[..., 3].view(torch.int16) == 0).all(), what
        assert torch.equal(got[..., :3].contiguous().view(torch.int16), torch.from_numpy(rl).bfloat16().view(torch.int16)), what
        for m, sp in px.items():
            eh, el = R.split(rl, R.PLANE[m])
            gh, gl = R.words(sp[k].hi), R.words(sp[k].lo)
            assert gh.shape == rl.shape[:4] + (4,) and not gh[..., 3].any() and not gl[..., 3].any(), what
            assert np.array_equal(gh[..., :3], eh) and np.array_equal(gl[..., :3], el), what + " " + m


def _windows(win_len):
    """Three windows, out of order and overlapping; the last frame of the third is the last one any window holds."""
    starts = [2, 0, 2 + max(1, win_len // 3)]
    return starts, max(starts) + win_len


PACK_SIZES = [(75, 133, 98),  # downscale; the scalar-store ncthw kernel; ndhwc4: 25 four-pixel chunks, the last one half outside, ragged last row tile
              (37, 53, 24),   # the 16-byte-store ncthw kernel; height up, width down
              (1, 1, 8),      # every index clamped; more rows per workgroup than the image has
              (3, 200, 6),    # out_hw no multiple of 8 or 4
              (64, 48, 2)]    # the smallest out_hw


@pytest.mark.parametrize("H,W,hw", PACK_SIZES)
@pytest.mark.parametrize("win_len", [1, 7, 20, 32, 33, 50])
def test_clip_pack_edges(avt, dev, H, W, hw, win_len):
    """Every output form of the packing, bit for bit.  win_len 1 and 7 repeat frames in the fast pathway, 32 samples each once,
    33 and 50 skip frames (at 50, and between the windows at 1, some frames are sampled by nobody).  Once a window ends on the
    last frame; once two more frames follow that no window holds."""
    from avtex import ops

    starts, used = _windows(win_len)
    frames = torch.randint(0, 256, (used + 2, H, W, 3), generator=_gen(H, W, hw, win_len), dtype=torch.uint8).numpy()
    hit = set(int(s + o) for s in starts for o in R.sample_indices(win_len)[0])
    assert used - 1 in hit and (win_len not in (1, 50) or hit != set(range(used)))  # frames inside the span that nobody samples
    _check_pack(ops, dev, np.ascontiguousarray(frames[:used]), starts, win_len, hw)
    _check_pack(ops, dev, frames, starts, win_len, hw)


def test_clip_pack_rgb_order_and_other_normalisation(avt, dev):
    from avtex import ops

    starts, used = _windows(20)
    frames = torch.randint(0, 256, (used, 37, 53, 3), generator=_gen(20), dtype=torch.uint8).numpy()
    _check_pack(ops, dev, frames, starts, 20, 24, mean=0.3, std=0.5, bgr=False)
    _check_pack(ops, dev, frames, starts, 20, 98, mean=0.3, std=0.5, bgr=False)
