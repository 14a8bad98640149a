"""The five passes of csrc/interp.hip one by one, on both plane types, against the fp32 restatements of
tests/interp_kernel_refs.py (pinned to the oracle on the CPU by test_interp_kernel_refs_host.py).  The file promises the
reference's fp32 operation order, so every comparison is for equal BITS: fp32 outputs as int32 words, output planes as the
16-bit words of split(reference).  The one exception is stated where it is used: `final` with free visibility logits,
where the device's expf may differ from the host's exp in the last bits.

Inputs that arrive as planes are split on the host and the reference consumes join(hi, lo), so kernel and reference see the
same values.  Every output buffer has spare rows (and spare channels where a slice is written) filled with a fixed bit
pattern that must survive.  Every test prints the figures it asserts on (pytest -s shows them)."""
import numpy as np
import pytest
import torch

import interp_kernel_refs as R
from interp_weights import frame_pair, unet_state
from oracle import interp_ref

pytestmark = pytest.mark.gpu

PLANES = [pytest.param(R.BF16, id="bf16"), pytest.param(R.F16, id="f16")]
MEAN2 = (0.1, 0.5, 0.9)
S16, S32, S8 = 0x5A5A, 0x5A5A5A5A, 0x5A  # the sentinel, as a 16-bit plane word / an fp32 word / a byte


def _gen(*key):
    return torch.Generator().manual_seed(int(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key))) + 41)


def _rng(*key):
    return np.random.default_rng([int(k) for k in key] + [41])


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


class Planes:
    """A plane pair [rows + spare, ld] on the device, pre-filled with the sentinel, and the Act of its slice [rows, c0 : c0 + c]."""

    def __init__(self, dev, rows, c, ld=None, c0=0, spare=1):
        from avtex.fused_slowfast import Act
        self.rows, self.c, self.c0 = rows, c, c0
        ld = c if ld is None else ld
        self.hi = torch.full((rows + spare, ld), S16, dtype=torch.int16, device=dev).view(torch.bfloat16)
        self.lo = torch.full((rows + spare, ld), S16, dtype=torch.int16, device=dev).view(torch.bfloat16)
        self.act = Act(self.hi, None, c0=c0, C=c, lo=self.lo)

    @property
    def ptrs(self):
        return self.act.ptrs

    @property
    def ld(self):
        return self.act.ld

    def put(self, x, pd):
        """Write split(x [rows, c]) into the slice; -> the fp32 values the planes then stand for (join)."""
        hi, lo = R.split(np.asarray(x, np.float32).reshape(self.rows, self.c), pd)
        sl = slice(self.c0, self.c0 + self.c)
        self.hi[: self.rows, sl] = hi.to(self.hi.device)
        self.lo[: self.rows, sl] = lo.to(self.lo.device)
        return R.join(hi, lo, pd)

    def check(self, what, exp, pd, nan_at=None):
        """The slice holds split(exp) word for word and everything around it still holds the sentinel."""
        torch.cuda.synchronize()
        eh, el = R.split(np.asarray(exp, np.float32).reshape(self.rows, self.c), pd)
        sl = slice(self.c0, self.c0 + self.c)
        for name, got, want in (("hi", self.hi, eh), ("lo", self.lo, el)):
            g, w = R.words(got), R.words(want)
            same = g[: self.rows, sl] == w
            if nan_at is not None:  # (a NaN's payload is not pinned: checked by the caller on the joined value)
                same |= nan_at.reshape(self.rows, self.c)
            assert same.all(), "%s: %s plane differs in %d of %d words" % (what, name, int((~same).sum()), same.size)
            rest = np.ones(g.shape, bool)
            rest[: self.rows, sl] = False
            assert (g[rest] == S16).all(), "%s: %s plane written outside its slice" % (what, name)

    def untouched(self):
        torch.cuda.synchronize()
        return bool((R.words(self.hi) == S16).all() and (R.words(self.lo) == S16).all())

    def values(self, pd):
        torch.cuda.synchronize()
        sl = slice(self.c0, self.c0 + self.c)
        return R.join(self.hi[: self.rows, sl].contiguous(), self.lo[: self.rows, sl].contiguous(), pd)


def _f32_buf(dev, rows, c, spare=1):
    return torch.full((rows + spare, c), S32, dtype=torch.int32, device=dev).view(torch.float32)


def _check_f32(what, buf, exp, rows, nan_at=None):
    torch.cuda.synchronize()
    g = buf.cpu().view(torch.int32).numpy().view(np.uint32)
    same = g[:rows] == _bits(exp).reshape(rows, -1)
    if nan_at is not None:
        same |= nan_at.reshape(rows, -1)
    assert same.all(), "%s: differs in %d of %d words" % (what, int((~same).sum()), same.size)
    assert (g[rows:] == S32).all(), "%s: written past its last row" % what


# ---------------------------------------------------------------- pack_pair
def _pack_frames(h, w):
    """Two different frames: ramps that take all 256 values in every channel within any 256 consecutive pixels (the steps 1 and 77
    are odd), plus noise bytes past the first 256 pixels."""
    p = np.arange(h * w, dtype=np.int64)[:, None]
    ch = np.arange(3, dtype=np.int64)[None, :]
    f0, f1 = (p + 37 * ch) % 256, (77 * p + 91 * ch + 13) % 256
    noise = _rng(h, w).integers(0, 256, size=(2, h * w, 3))
    f0[256:], f1[256:] = noise[0, 256:], noise[1, 256:]
    if h * w >= 256:
        assert all(len(set(f[:, c].tolist())) == 256 for f in (f0, f1) for c in range(3))
    assert h * w == 1 or not np.array_equal(f0, f1)
    return [torch.from_numpy(f.astype(np.uint8).reshape(h, w, 3)) for f in (f0, f1)]


@pytest.mark.parametrize("mean", [interp_ref.MEAN, MEAN2], ids=["mean", "mean2"])
@pytest.mark.parametrize("h,w", [(1, 1), (3, 5), (16, 16), (17, 31)])
@pytest.mark.parametrize("pd", PLANES)
def test_pack_pair(avt, dev, pd, h, w, mean):
    f0, f1 = _pack_frames(h, w)
    img = _f32_buf(dev, 2 * h * w, 4, spare=w)
    x = Planes(dev, h * w, 8)
    avt.ops.interp_pack_pair(f0.to(dev), f1.to(dev), mean, img[: 2 * h * w].view(2, h, w, 4), x.ptrs, pd)
    eimg, erow = R.pack_pair_ref(f0, f1, mean)
    assert not eimg[:, :, :, 3].any() and not erow[:, :, 6:].any()
    _check_f32("img", img, eimg, 2 * h * w)  # (bits: the fourth lane is +0.0)
    x.check("flowComp input", erow, pd)


# ---------------------------------------------------------------- avgpool2 / upsample2
def _slab(dev, pd, shape, sliced, key):
    """Input planes of an NHWC extent, contiguous or as the channel slice [8 : 8 + c] of rows c + 16 wide (junk around it)."""
    b, h, w, c = shape
    x = torch.randn(b * h * w, c, generator=_gen(key, *shape)).numpy() * np.float32(3.0)
    src = Planes(dev, b * h * w, c, ld=c + 16, c0=8) if sliced else Planes(dev, b * h * w, c)
    return src, src.put(x, pd).reshape(shape)


@pytest.mark.parametrize("sliced", [False, True], ids=["contiguous", "sliced"])
@pytest.mark.parametrize("shape", [(1, 2, 2, 8), (2, 4, 6, 8), (3, 6, 10, 24), (1, 32, 48, 32)])
@pytest.mark.parametrize("pd", PLANES)
def test_avgpool2(avt, dev, pd, shape, sliced):
    b, h, w, c = shape
    src, xin = _slab(dev, pd, shape, sliced, 1)
    rows = b * (h // 2) * (w // 2)
    dst = Planes(dev, rows, c, ld=c + 24, c0=8) if sliced else Planes(dev, rows, c)  # (sliced: ldi = c + 16, ldo = c + 24)
    avt.ops.avgpool2_x3(src.ptrs, (b, h, w), c, src.ld, dst.ptrs, dst.ld, pd)
    dst.check("avgpool2 %s" % (shape,), R.avgpool2_ref(xin), pd)


@pytest.mark.parametrize("sliced", [False, True], ids=["contiguous", "sliced"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 8), (2, 1, 5, 8), (2, 3, 1, 16), (3, 5, 7, 24), (1, 16, 24, 32)])
@pytest.mark.parametrize("pd", PLANES)
def test_upsample2(avt, dev, pd, shape, sliced):
    b, h, w, c = shape
    src, xin = _slab(dev, pd, shape, sliced, 2)
    rows = b * 4 * h * w
    dst = Planes(dev, rows, c, ld=c + 24, c0=8) if sliced else Planes(dev, rows, c)
    avt.ops.upsample2_bilinear_x3(src.ptrs, (b, h, w), c, src.ld, dst.ptrs, dst.ld, pd)
    dst.check("upsample2 %s" % (shape,), R.upsample2_ref(xin), pd)  # (and the rest of the concat row keeps the sentinel)


# ---------------------------------------------------------------- refusals
def test_pool_and_upsample_refusals(avt, dev):
    """Each bad geometry raises AvtError before anything is launched: the output keeps its bit pattern.  (The buffers are large
    enough for the nearest legal geometry.)"""
    ops, Err = avt.ops, avt._lib.AvtError
    src = Planes(dev, 256, 32)
    src.put(np.ones((256, 32), np.float32), R.F16)
    dst = Planes(dev, 1024, 32)
    sp, dp = src.ptrs, dst.ptrs
    off4 = lambda p: (p[0] + 8, p[1] + 8)  # a slice that starts at channel 4: 8-byte aligned only
    pool = [("odd h", sp, (1, 3, 4), 8, 8, dp, 8, 1), ("odd w", sp, (1, 4, 5), 8, 8, dp, 8, 1), ("c % 8", sp, (1, 4, 4), 12, 16, dp, 16, 1),
            ("ldi < c", sp, (1, 4, 4), 16, 8, dp, 16, 1), ("ldo < c", sp, (1, 4, 4), 16, 16, dp, 8, 1),
            ("ldi % 8", sp, (1, 4, 4), 16, 20, dp, 16, 1), ("ldo % 8", sp, (1, 4, 4), 16, 16, dp, 20, 1),
            ("input slice at channel 4", off4(sp), (1, 4, 4), 8, 32, dp, 32, 1), ("output slice at channel 4", sp, (1, 4, 4), 8, 32, off4(dp), 32, 1),
            ("plane_dtype 2", sp, (1, 4, 4), 8, 8, dp, 8, 2)]
    for fn, cases in ((ops.avgpool2_x3, pool), (ops.upsample2_bilinear_x3, [c for c in pool if not c[0].startswith("odd")])):
        for what, xp, dims, c, ldi, yp, ldo, pd in cases:
            with pytest.raises(Err):
                fn(xp, dims, c, ldi, yp, ldo, pd)
            assert dst.untouched(), "%s: %s wrote its output" % (fn.__name__, what)


def test_interp_refusals(avt, dev):
    """plane_dtype 2 for the three interpolation passes, slomo factors 1 and 18, and a frame of 4097 x 4096 (2^24 + 4096 pixels:
    the size check comes before any access, so the buffers are dummies)."""
    ops, Err = avt.ops, avt._lib.AvtError
    h, w = 4, 4
    f = torch.zeros((h, w, 3), dtype=torch.uint8, device=dev)
    img = _f32_buf(dev, 2 * h * w, 4)
    imgv = img[: 2 * h * w].view(2, h, w, 4)
    x8, x24, flow = Planes(dev, h * w, 8), Planes(dev, 16 * h * w, 24), Planes(dev, 16 * h * w, 8)
    ft = _f32_buf(dev, 16 * h * w, 4)
    out = torch.full((16 * h * w + 1, 3), S8, dtype=torch.uint8, device=dev)

    def clean(what):
        torch.cuda.synchronize()
        ok = x8.untouched() and x24.untouched() and bool((out == S8).all())
        ok = ok and all(bool((b.view(torch.int32) == S32).all()) for b in (img, ft))
        assert ok, "%s wrote an output" % what

    with pytest.raises(Err):
        ops.interp_pack_pair(f, f, interp_ref.MEAN, imgv, x8.ptrs, 2)
    clean("pack_pair, plane_dtype 2")
    with pytest.raises(Err):  # (straight through the checked ABI: ops takes the extents from the frame tensor)
        avt._lib.checked.avt_interp_pack_pair_u8(ops._p(f), ops._p(f), 4097, 4096, ops._mean3(interp_ref.MEAN), ops._p(img), x8.ptrs[0],
                                                 x8.ptrs[1], 1, ops._stream())
    clean("pack_pair, 4097 x 4096")
    img_in = torch.zeros((2, h, w, 4), dtype=torch.float32, device=dev)  # (inputs of the next two passes)
    ftin = torch.zeros((16 * h * w, 4), dtype=torch.float32, device=dev)
    flow.put(np.zeros((16 * h * w, 8), np.float32), R.F16)
    for sf, pd in ((1, 1), (18, 1), (1, 0), (18, 0), (3, 2)):
        with pytest.raises(Err):
            ops.interp_mid_input(img_in, flow.ptrs, h, w, sf, x24.ptrs, ft, pd)
        clean("mid_input, sf %d plane_dtype %d" % (sf, pd))
        with pytest.raises(Err):
            ops.interp_final(img_in, ftin, flow.ptrs, h, w, sf, interp_ref.MEAN, out, pd)
        clean("final, sf %d plane_dtype %d" % (sf, pd))


# ---------------------------------------------------------------- the flows of mid_input / final
FRAMES = [(1, 1), (5, 7), (16, 16), (33, 17)]
SFS = [2, 3, 17]


def _huge(pd):
    return 6.0e4 if pd == R.F16 else 1e30  # fp16 planes: the format's range


def _noise_img(h, w):
    """pack_pair_ref of two noise frames: neighbouring pixels are uncorrelated, so a wrong tap is O(0.3)."""
    f = _rng(h, w, 7).integers(0, 256, size=(2, h, w, 3)).astype(np.uint8)
    return R.pack_pair_ref(f[0], f[1], interp_ref.MEAN)[0]


def _mixture(h, w, n, pd, key, kinds):
    """[n, h*w, 4] flows (x, y, x, y): the pixel's index modulo 11 picks the kind, every channel draws its own value."""
    rng = _rng(h, w, n, key)
    hw = h * w
    kind = np.asarray(kinds)[(np.arange(hw) + 1) % 11]  # (pixel 0, all of a 1x1 frame: the second kind)
    ext = np.asarray([w + 3, h + 3, w + 3, h + 3], np.float32)
    sign = rng.choice(np.asarray([-1.0, 1.0], np.float32), size=(n, hw, 4))
    val = {
        "zero": np.zeros((n, hw, 4), np.float32),
        "sub": rng.uniform(-0.95, 0.95, size=(n, hw, 4)).astype(np.float32),
        "few": (rng.standard_normal((n, hw, 4)) * 2.5).astype(np.float32),
        "int": rng.integers(-3, 4, size=(n, hw, 4)).astype(np.float32),
        "half": rng.integers(-3, 3, size=(n, hw, 4)).astype(np.float32) + np.float32(0.5),
        "out": sign * ext,
        "huge": sign * np.float32(_huge(pd)),
    }
    out = np.zeros((n, hw, 4), np.float32)
    for name, v in val.items():
        out[:, kind == name] = v[:, kind == name]
    return out


MIX = ["zero", "sub", "int", "huge", "out", "half", "sub", "huge", "out", "few", "int"]
MIX_NON_INTEGER = ["sub", "few", "sub", "few", "out", "sub", "few", "sub", "few", "sub", "few"]


def _targeted(h, w):
    """d [h*w, 2] such that the sample at pixel + d - 1/2 lands, on each of the four sides, on the edge pixel's centre, half a pixel
    outside, one pixel outside and a whole extent outside (16 targets, dealt over the pixels)."""
    py, px = np.divmod(np.arange(h * w), w)
    j = (px + 5 * py) % 16
    side, off = j // 4, j % 4
    outward = np.where(off == 3, np.where(side < 2, w, h), np.asarray([0.0, 0.5, 1.0, 0.0])[off]).astype(np.float64)
    sx = np.where(side == 0, -outward, np.where(side == 1, w - 1 + outward, px))
    sy = np.where(side == 2, -outward, np.where(side == 3, h - 1 + outward, py))
    d = np.stack((sx - px + 0.5, sy - py + 0.5), 1).astype(np.float32)
    assert np.array_equal(d * 4, np.round(d * 4)) and np.abs(d * 4).max() <= 512  # 4 d is exact in either plane pair
    return d


def _run_mid(avt, dev, pd, h, w, sf, img, flow8):
    nt, hw = sf - 1, h * w
    fl = Planes(dev, hw, 8)
    fin = fl.put(flow8, pd)
    x = Planes(dev, nt * hw, 24)
    ft = _f32_buf(dev, nt * hw, 4)
    avt.ops.interp_mid_input(torch.from_numpy(img).to(dev), fl.ptrs, h, w, sf, x.ptrs, ft[: nt * hw].view(nt, h, w, 4), pd)
    return fin, x, ft


def _flow8(flow4, key):
    """[hw, 4] -> [hw, 8]: channels 4-7 hold non-zero junk that nothing may read."""
    junk = _rng(len(flow4), key).uniform(1.0, 100.0, size=(len(flow4), 4)).astype(np.float32)
    return np.concatenate((flow4, junk), 1)


@pytest.mark.parametrize("sf", SFS)
@pytest.mark.parametrize("h,w", FRAMES)
@pytest.mark.parametrize("pd", PLANES)
def test_mid_input(avt, dev, pd, h, w, sf):
    nt, hw = sf - 1, h * w
    img = _noise_img(h, w)
    fin, x, ft = _run_mid(avt, dev, pd, h, w, sf, img, _flow8(_mixture(h, w, 1, pd, 1, MIX)[0], 1))
    eft, erow, inside, outside = R.mid_input_ref(img, fin[:, :4].reshape(h, w, 4), sf, masks=True)
    print("mid_input %dx%d sf %d: all four taps inside %.2f, a tap outside %.2f of the warped pixels" % (h, w, sf, inside.mean(), outside.mean()))
    if h > 1 and w > 1:  # (a frame of one row or column always has a tap outside: the sample sits at pixel + flow - 1/2)
        assert inside.mean() >= 0.25 and outside.mean() >= 0.25
    assert np.isfinite(erow).all() and not erow[..., 20:].any()
    if sf == 17:  # 16 different coefficient sets: equal bits prove that frame k used slot k
        assert len({eft[k].tobytes() for k in range(nt)}) == nt
    _check_f32("ft", ft, eft, nt * hw)
    x.check("ArbTimeFlowIntrp input", erow, pd)


@pytest.mark.parametrize("h,w", [(8, 16), (33, 17)])
@pytest.mark.parametrize("pd", PLANES)
def test_mid_input_at_the_frame_borders(avt, dev, pd, h, w):
    """sf = 2: the coefficients are exactly -+1/4, so F_0_1 = 0, F_1_0 = 4 d gives F_t_0 = d and F_t_1 = -d exactly."""
    img, d = _noise_img(h, w), _targeted(h, w)
    flow4 = np.concatenate((np.zeros_like(d), 4 * d), 1)
    fin, x, ft = _run_mid(avt, dev, pd, h, w, 2, img, _flow8(flow4, 2))
    assert np.array_equal(fin[:, :4], flow4)
    eft, erow, inside, outside = R.mid_input_ref(img, fin[:, :4].reshape(h, w, 4), 2, masks=True)
    assert np.array_equal(eft[0].reshape(-1, 4), np.concatenate((d, -d), 1))
    assert outside[0].mean() >= 0.5 and inside[1].any()
    _check_f32("ft", ft, eft, h * w)
    x.check("ArbTimeFlowIntrp input", erow, pd)


@pytest.mark.parametrize("pd", PLANES)
def test_mid_input_nan_flow_poisons_its_pixel_only(avt, dev, pd):
    """A NaN flow gives NaN (a NaN weight times a zero tap), as torch's grid_sample does; every other pixel keeps its bits."""
    h, w, sf = 5, 7, 3
    nt, hw, bad = sf - 1, h * w, 17
    img = _noise_img(h, w)
    flow8 = _flow8(_mixture(h, w, 1, pd, 3, ["sub"] * 11)[0], 3)
    fin, x, ft = _run_mid(avt, dev, pd, h, w, sf, img, flow8)
    eft, erow = R.mid_input_ref(img, fin[:, :4].reshape(h, w, 4), sf)
    _check_f32("ft", ft, eft, nt * hw)
    x.check("clean", erow, pd)
    flow8[bad, 0] = np.nan  # F_0_1's x: every weight of both warps at this pixel
    fin, xp, ftp = _run_mid(avt, dev, pd, h, w, sf, img, flow8)
    assert np.isnan(fin[bad, 0]) and np.isnan(fin).sum() == 1
    pft, prow = R.mid_input_ref(img, fin[:, :4].reshape(h, w, 4), sf)
    nan_ft, nan_row = np.isnan(pft).reshape(nt * hw, 4), np.isnan(prow).reshape(nt * hw, 24)
    want = np.zeros((nt, hw, 24), bool)
    want[:, bad, [6, 10, 12]] = True   # the flow itself, F_t_1 x, F_t_0 x
    want[:, bad, 14:20] = True         # both warps, every colour
    assert np.array_equal(nan_row, want.reshape(nt * hw, 24)) and nan_ft.sum() == 2 * nt
    _check_f32("ft", ftp, pft, nt * hw, nan_at=nan_ft)
    xp.check("poisoned", prow, pd, nan_at=nan_row)
    got_ft = ftp[: nt * hw].cpu().numpy()
    assert np.array_equal(np.isnan(got_ft), nan_ft) and np.array_equal(np.isnan(xp.values(pd)), nan_row)
    keep = ~nan_row
    assert np.array_equal(R.words(xp.hi)[: nt * hw][keep], R.words(x.hi)[: nt * hw][keep])  # bit-equal to the run without the poison
    assert np.array_equal(R.words(xp.lo)[: nt * hw][keep], R.words(x.lo)[: nt * hw][keep])


# ---------------------------------------------------------------- final
def _run_final(avt, dev, pd, h, w, sf, img, ft, o8, mean=interp_ref.MEAN):
    nt, hw = sf - 1, h * w
    op = Planes(dev, nt * hw, 8)
    oin = op.put(o8, pd)
    out = torch.full((nt * hw + w, 3), S8, dtype=torch.uint8, device=dev)
    avt.ops.interp_final(torch.from_numpy(img).to(dev), torch.from_numpy(ft).to(dev), op.ptrs, h, w, sf, mean,
                         out[: nt * hw].view(nt, h, w, 3), pd)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[nt * hw :] == S8).all(), "final wrote past its last frame"
    eu8, pre = R.final_ref(img, ft.reshape(nt, h, w, 4), oin.reshape(nt, h, w, 8), sf, mean)
    return got[: nt * hw].reshape(nt, h, w, 3), eu8, pre


def _o8(res4, logit, key):
    """[n, 4] residual flows + [n] logits -> [n, 8]: channels 5-7 hold junk."""
    junk = _rng(len(res4), key).uniform(1.0, 100.0, size=(len(res4), 3)).astype(np.float32)
    return np.concatenate((res4, logit[:, None].astype(np.float32), junk), 1)


@pytest.mark.parametrize("sf", SFS)
@pytest.mark.parametrize("h,w", FRAMES)
@pytest.mark.parametrize("pd", PLANES)
def test_final_exact_sigmoid(avt, dev, pd, h, w, sf):
    """Logits from {0, +40, -100}: expf gives exactly 1, an underflow to 1 + eps = 1 and +inf, so V0 is 0.5, 1 or 0 whatever
    expf's last bit, and the uint8 frames must be equal at every pixel.  Even pixels carry F_t = 1/2, so an integer residual puts
    the sample on a pixel centre: (k / 255 - m + m) * 255 sits next to an integer there.  The same residuals, flows and logits
    serve every intermediate frame, so consecutive frames differ through the blend weights of their slot alone."""
    nt, hw = sf - 1, h * w
    rng = _rng(h, w, sf, 5)
    img = _noise_img(h, w)
    ft1 = rng.uniform(-0.95, 0.95, size=(hw, 4)).astype(np.float32)
    ft1[0::2] = 0.5
    res = _mixture(h, w, 1, pd, 5, MIX)[0]
    logit = rng.choice(np.asarray([0.0, 0.0, 40.0, -100.0], np.float32), size=hw)
    logit[0] = 0.0
    ft, o8 = np.tile(ft1, (nt, 1)), np.tile(_o8(res, logit, 5), (nt, 1))
    got, eu8, pre = _run_final(avt, dev, pd, h, w, sf, img, ft, o8)
    near = np.abs(pre - np.round(pre)) < 1e-3
    print("final %dx%d sf %d, exact sigmoid: %.3f of the values within 1e-3 of an integer" % (h, w, sf, near.mean()))
    if hw >= 35:
        assert near.sum() >= 3  # the centre samples are there
        for k in range(nt - 1):  # sf = 17: 16 distinct blends
            assert not np.array_equal(eu8[k], eu8[k + 1])
    assert np.array_equal(got, eu8), "%d of %d bytes differ" % (int((got != eu8).sum()), got.size)


@pytest.mark.parametrize("h,w", [(8, 16), (33, 17)])
@pytest.mark.parametrize("pd", PLANES)
def test_final_at_the_frame_borders(avt, dev, pd, h, w):
    """F_t = 0, so the residual is the flow: the targeted border samples of I0 (and their mirror images of I1), exact logits,
    a second mean."""
    hw = h * w
    img, d = _noise_img(h, w), _targeted(h, w)
    logit = _rng(h, w, 6).choice(np.asarray([0.0, 40.0, -100.0], np.float32), size=hw)
    o8 = _o8(np.concatenate((d, -d), 1), logit, 6)
    for mean in (interp_ref.MEAN, MEAN2):
        got, eu8, _ = _run_final(avt, dev, pd, h, w, 2, img, np.zeros((hw, 4), np.float32), o8, mean)
        assert np.array_equal(got, eu8), "%d of %d bytes differ" % (int((got != eu8).sum()), got.size)


@pytest.mark.parametrize("sf", SFS)
@pytest.mark.parametrize("h,w", FRAMES)
@pytest.mark.parametrize("pd", PLANES)
def test_final_free_logits(avt, dev, pd, h, w, sf):
    """Logits N(0, 2) and non-integer flows, different for every intermediate frame.  The device's expf and the host's exp may
    differ in the last bits: V0 moves by about 2^-22 relative and the value before truncation by at most about
    255 |g0 - g1| 2^-21 = 1.2e-4.  Values whose REFERENCE lies within 1e-3 of an integer (8x that bound, the figure of the G10
    test) may differ by one level; every other byte must be equal.  Near values: at most 1 % (0.2 % expected)."""
    nt, hw = sf - 1, h * w
    rng = _rng(h, w, sf, 8)
    img = _noise_img(h, w)
    ft = rng.uniform(-0.95, 0.95, size=(nt * hw, 4)).astype(np.float32)
    res = _mixture(h, w, nt, pd, 8, MIX_NON_INTEGER).reshape(nt * hw, 4)
    logit = (rng.standard_normal(nt * hw) * 2.0).astype(np.float32)
    got, eu8, pre = _run_final(avt, dev, pd, h, w, sf, img, ft, _o8(res, logit, 8))
    near = np.abs(pre - np.round(pre)) < 1e-3
    d = np.abs(got.astype(np.int32) - eu8.astype(np.int32))
    print("final %dx%d sf %d, free logits: near an integer %d of %d, bytes differing %d" % (h, w, sf, int(near.sum()), near.size, int((d > 0).sum())))
    assert near.mean() <= 0.01 or near.sum() <= 1
    assert not d[~near].any() and int(d.max()) <= 1


# ---------------------------------------------------------------- end to end at the slomo factors G10 does not hold
@pytest.mark.parametrize("sf", [2, 17])
def test_interpolator_matches_oracle_at_other_factors(avt, dev, sf):
    """Interpolator on a 32x64 pair against interp_ref.interpolate_pair, by G10's criterion: at most one grey level, on fewer
    than 1e-3 of the values (the convolutions carry a 2^-22 split; see test_gpu_interp.py).  Weights and frames are those of
    test_interpolator_is_deterministic_and_handles_other_sizes.  Measured: 1.6e-4 of the values at sf 2 (1 of 6144), 4e-5 at
    sf 17 (4 of 98304); five other seed choices gave 0 to 8.1e-4 at sf 2 and 3e-5 to 4.7e-4 at sf 17."""
    from avtex import slowmo
    h, w = 32, 64
    fc, at = unet_state(6, 4, 31, head_gain=20.0), unet_state(20, 5, 32, head_gain=5.0)
    f0, f1 = frame_pair(9, h, w)
    it = slowmo.Interpolator(h, w, sf, dev)
    it.flow_comp.load_state_dict(fc)
    it.arb_time.load_state_dict(at)
    out = it(f0.to(dev), f1.to(dev))
    torch.cuda.synchronize()
    exp = interp_ref.interpolate_pair(fc, at, f0, f1, sf).numpy()
    assert tuple(out.shape) == exp.shape == (sf - 1, h, w, 3) and out.dtype == torch.uint8
    d = np.abs(out.cpu().numpy().astype(np.int32) - exp.astype(np.int32))
    frac = float((d > 0).mean())
    print("interpolator sf %d: values differing %.5f, max |diff| %d" % (sf, frac, int(d.max())))
    for k in range(sf - 2):
        assert not np.array_equal(exp[k], exp[k + 1])
    assert int(d.max()) <= 1
    assert frac < 1e-3, frac
