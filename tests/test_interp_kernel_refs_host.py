"""The restatements of tests/interp_kernel_refs.py (what tests/test_gpu_interp_kernels.py holds csrc/interp.hip to, bit for
bit) pinned to the oracle on the CPU: oracle/interp_ref.py and the torch operations it is made of.  torch's fused CPU
kernels do not follow the kernel's documented operation order, so the upsample and the back-warp agree to a measured
tolerance only; a restatement that picked a wrong tap or weight would be off by O(1) on these unit-normal inputs.

Every test prints the figures it asserts on (pytest -s shows them)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import interp_kernel_refs as R
from oracle import interp_ref

# measured maxima of |restatement - torch| on the input families below (see each test), and the bounds asserted: 4x, the
# slack for a torch build whose vectorised kernels re-associate differently
UPSAMPLE_MEASURED, UPSAMPLE_TOL = 3.6e-7, 4 * 3.6e-7
BACKWARP_MEASURED, BACKWARP_TOL = 1.6e-6, 4 * 1.6e-6


def _gen(*key):
    return torch.Generator().manual_seed(int(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key))) + 29)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _nchw(x):  # numpy [b,h,w,c] -> torch [b,c,h,w]
    return torch.from_numpy(np.ascontiguousarray(x)).permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


# ---------------------------------------------------------------- split / join
@pytest.mark.parametrize("pd", [R.BF16, R.F16])
def test_split_is_the_products_split_planes(avt, pd):
    from avtex import ops
    from avtex.fused_slowfast import split_planes
    assert (R.BF16, R.F16) == (ops.X3_BF16, ops.X3_F16)
    x = torch.randn(4096, generator=_gen(pd, 1)) * torch.logspace(-6, 4, 4096)
    hi, lo = R.split(x, pd)
    ph, pl = split_planes(x, pd)
    assert np.array_equal(R.words(hi), R.words(ph)) and np.array_equal(R.words(lo), R.words(pl))
    v = R.join(hi, lo, pd)
    assert float(x.abs().max()) < 65504.0
    err, mag = np.abs(v.astype(np.float64) - x.numpy()), np.abs(x.numpy()).astype(np.float64)
    # split_planes.h: bf16 planes 2^-16 |x| at every magnitude; fp16 planes 2^-22 |x|, or 2^-24 absolute below 2^-3
    bound = mag * 2.0 ** -16 if pd == R.BF16 else np.maximum(mag * 2.0 ** -22, 2.0 ** -24)
    print("plane_dtype %d: worst split/join error / bound %.3f" % (pd, float((err / bound).max())))
    assert (err <= bound).all()


def test_split_special_values_follow_split_planes_h():
    """fp16 planes: finite values clamp to +-65504, an infinity stays that infinity with lo = 0, a NaN stays a NaN with lo = 0."""
    x = np.array([1e30, -7e4, 65504.0, np.inf, -np.inf, np.nan, 6.0e4], np.float32)
    v = R.join(*R.split(x, R.F16), R.F16)
    assert np.array_equal(v[:5], np.array([65504.0, -65504.0, 65504.0, np.inf, -np.inf], np.float32))
    assert np.isnan(v[5]) and v[6] == np.float32(6.0e4)
    assert np.array_equal(R.words(R.split(x, R.F16)[1])[3:6], np.zeros(3, np.uint16))
    b = R.join(*R.split(x, R.BF16), R.BF16)
    assert abs(float(b[0]) / 1e30 - 1) < 2.0 ** -16 and np.isnan(b[5])


# ---------------------------------------------------------------- avgpool2 / upsample2
@pytest.mark.parametrize("shape", [(1, 2, 2, 8), (2, 4, 6, 8), (3, 6, 10, 24), (1, 32, 48, 32), (3, 8, 12, 16)])
def test_avgpool2_ref_is_bit_equal_to_torch(shape):
    x = torch.randn(shape, generator=_gen(*shape)).numpy()
    exp = _nhwc(F.avg_pool2d(_nchw(x), 2))
    assert np.array_equal(_bits(R.avgpool2_ref(x)), _bits(exp))


UP_SHAPES = [(1, 1, 1, 8), (2, 1, 5, 8), (2, 3, 1, 16), (3, 5, 7, 24), (1, 16, 24, 32), (3, 8, 12, 16)]


def test_upsample2_ref_matches_torch():
    """Measured here: max |restatement - F.interpolate| = 3.6e-7 over these shapes on unit-normal inputs (52-100 % of the values
    bit-equal); asserted: 4x that, 1.44e-6."""
    worst = 0.0
    for shape in UP_SHAPES:
        x = torch.randn(shape, generator=_gen(*shape)).numpy()
        got = R.upsample2_ref(x)
        exp = _nhwc(F.interpolate(_nchw(x), scale_factor=2, mode="bilinear", align_corners=False))
        assert got.shape == exp.shape and got.dtype == np.float32
        err = float(np.abs(got - exp).max())
        print("upsample %s: max |diff| %.3e, bit-equal %.1f %%" % (shape, err, 100.0 * float((_bits(got) == _bits(exp)).mean())))
        worst = max(worst, err)
    print("upsample: worst %.3e (measured %.1e, bound %.2e)" % (worst, UPSAMPLE_MEASURED, UPSAMPLE_TOL))
    assert worst <= UPSAMPLE_TOL


def test_up_src_extents_of_one_and_odd():
    """h = 1: both taps are row 0 whatever the weights; odd n: the last two outputs clamp their second tap to n - 1."""
    i0, i1, l0, l1 = R.up_src(1)
    assert i0.tolist() == [0, 0] and i1.tolist() == [0, 0]
    assert l0.tolist() == [1.0, 0.75] and l1.tolist() == [0.0, 0.25]
    i0, i1, l0, l1 = R.up_src(5)
    assert i0.tolist() == [0, 0, 0, 1, 1, 2, 2, 3, 3, 4] and i1.tolist() == [1, 1, 1, 2, 2, 3, 3, 4, 4, 4]
    assert l1.tolist() == [0.0, 0.25, 0.75, 0.25, 0.75, 0.25, 0.75, 0.25, 0.75, 0.25]


# ---------------------------------------------------------------- backwarp
BW_SHAPES = [(1, 1), (1, 9), (9, 1), (5, 7), (16, 24), (33, 17)]
BW_SCALES = [0.3, 3.0, 40.0]


def _bw_inputs(h, w, scale):
    g = _gen(h, w, int(scale * 10))
    img = torch.randn(h, w, 3, generator=g).numpy()
    flow = (torch.randn(h * w * 2, generator=g) * scale).numpy()
    flow[0::5] = np.round(flow[0::5])  # every fifth flow an integer: samples on pixel centres, weights exactly 0 and 1
    flow[0::7] += np.float32(0.5)      # every seventh shifted by half a pixel
    return img, flow.reshape(h, w, 2)


def _oracle_backwarp(img, flow):
    out = interp_ref.backwarp(_nchw(img[None]), _nchw(flow[None]))
    return _nhwc(out)[0]


def test_backwarp_ref_matches_oracle():
    """Measured here: max |restatement - interp_ref.backwarp| = 1.6e-6 (1.52e-6, at 33x17 with 0.3-pixel flows) over these shapes
    and flow scales on unit-normal images (62-100 % of the values bit-equal); asserted: 4x that, 6.4e-6.  A wrong tap is off by
    O(1)."""
    worst = 0.0
    for h, w in BW_SHAPES:
        for scale in BW_SCALES:
            img, flow = _bw_inputs(h, w, scale)
            got, inside, outside = R.backwarp_ref(img, flow, masks=True)
            exp = _oracle_backwarp(img, flow)
            assert got.shape == exp.shape and got.dtype == np.float32
            err = float(np.abs(got - exp).max())
            print("backwarp %dx%d flows x%.1f: max |diff| %.3e, bit-equal %.1f %%, all taps inside %.2f, some outside %.2f"
                  % (h, w, scale, err, 100.0 * float((_bits(got) == _bits(exp)).mean()), inside.mean(), outside.mean()))
            worst = max(worst, err)
    print("backwarp: worst %.3e (measured %.1e, bound %.2e)" % (worst, BACKWARP_MEASURED, BACKWARP_TOL))
    assert worst <= BACKWARP_TOL


def test_backwarp_ref_half_pixel_convention():
    """The reference normalises the grid as for align_corners=True and torch samples it with align_corners=False, so the sample
    sits at pixel + flow - 1/2: a flow of 0 averages the 2x2 block up and to the left (zeros outside), a flow of 1/2 returns the
    image, and 1/2 + an integer the shifted image with zeros where the source is outside.  Extents that are powers of two keep
    the normalisation exact."""
    img = torch.randn(8, 16, 3, generator=_gen(8, 16)).numpy()
    f = np.zeros((8, 16, 2), np.float32)
    pad = np.zeros((9, 17, 3), np.float32)
    pad[1:, 1:] = img
    quarter = np.float32(0.25)
    exp = ((pad[:-1, :-1] * quarter + pad[:-1, 1:] * quarter) + pad[1:, :-1] * quarter) + pad[1:, 1:] * quarter
    got = R.backwarp_ref(img, f)
    assert np.array_equal(_bits(got), _bits(exp))
    assert float(np.abs(got - _oracle_backwarp(img, f)).max()) <= BACKWARP_TOL
    f[:] = 0.5
    got, inside, outside = R.backwarp_ref(img, f, masks=True)
    assert np.array_equal(_bits(got), _bits(img))
    assert inside[:-1, :-1].all() and outside[-1].all() and outside[:, -1].all()  # the (weight 0) taps past the last row / column
    f[:, :, 0], f[:, :, 1] = 3.5, -1.5
    exp = np.zeros_like(img)
    exp[2:, :13] = img[:6, 3:]
    got = R.backwarp_ref(img, f)
    assert np.array_equal(got, exp)
    assert np.array_equal(got, _oracle_backwarp(img, f))


def test_backwarp_ref_special_values():
    """Flows of +-1e30 give exact zeros, a NaN flow gives NaN; interp_ref.backwarp does the same.  (Every other pixel has a
    flow of 1/2: the image itself.)"""
    img = torch.randn(8, 8, 3, generator=_gen(8, 8)).numpy()
    flow = np.full((8, 8, 2), 0.5, np.float32)
    flow[1, 2, 0], flow[2, 3, 1], flow[3, 4] = 1e30, -1e30, (-1e30, 1e30)
    flow[4, 5, 0], flow[0, 6, 1] = np.nan, np.nan
    got, exp = R.backwarp_ref(img, flow), _oracle_backwarp(img, flow)
    for a in (got, exp):
        for y, x in ((1, 2), (2, 3), (3, 4)):
            assert np.array_equal(_bits(a[y, x]), np.zeros(3, np.uint32))  # +0.0, not -0.0
        assert np.isnan(a[4, 5]).all() and np.isnan(a[0, 6]).all()
    rest = np.ones((8, 8), bool)
    for y, x in ((1, 2), (2, 3), (3, 4), (4, 5), (0, 6)):
        rest[y, x] = False
    assert np.array_equal(_bits(got[rest]), _bits(img[rest]))


# ---------------------------------------------------------------- pack_pair -> mid_input -> final against the oracle's formulas
def test_composition_matches_the_oracle_formulas():
    """pack_pair_ref -> mid_input_ref -> final_ref at 16x24, sf = 5 with random flows, residuals and logits, against
    interp_ref.to_tensor / backwarp / to_u8 and the formulas of interp_ref.interpolate_pair (the loop over k).  Images,
    F_t_0 / F_t_1: bit-equal (elementwise in both).  Warped channels: BACKWARP_TOL.  Values before truncation: BACKWARP_TOL * 255
    (measured 3.1e-5; the images are within [-0.43, 0.61], so the warps differ by less than on unit-normal inputs, and torch's
    sigmoid differs from 1 / (1 + exp(-x)) by an ulp).  uint8: at most one level, only where the value is within 1e-3 of an
    integer."""
    h, w, sf = 16, 24, 5
    nt = sf - 1
    g = _gen(h, w, sf)
    f0 = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)
    f1 = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)
    flow = torch.randn(1, 4, h, w, generator=g) * 3.0
    o = torch.cat((torch.randn(nt, 4, h, w, generator=g) * 0.7, torch.randn(nt, 1, h, w, generator=g) * 2.0), 1)
    # the restatements
    img, row8 = R.pack_pair_ref(f0, f1, interp_ref.MEAN)
    ft, row = R.mid_input_ref(img, _nhwc(flow)[0], sf)
    u8, pre = R.final_ref(img, ft, _nhwc(o), sf, interp_ref.MEAN)
    # the oracle
    i0, i1 = interp_ref.to_tensor(f0).unsqueeze(0), interp_ref.to_tensor(f1).unsqueeze(0)
    assert np.array_equal(_bits(img[0, :, :, :3]), _bits(_nhwc(i0)[0])) and np.array_equal(_bits(img[1, :, :, :3]), _bits(_nhwc(i1)[0]))
    assert not img[:, :, :, 3].any() and not row8[:, :, 6:].any()
    assert np.array_equal(row8[:, :, :3], img[0, :, :, :3]) and np.array_equal(row8[:, :, 3:6], img[1, :, :, :3])
    f01, f10 = flow[:, :2], flow[:, 2:]
    mean = torch.tensor(interp_ref.MEAN).view(3, 1, 1)
    worst_g = worst_p = 0.0
    for k in range(1, sf):
        t = float(k) / sf
        temp = -t * (1 - t)
        ft0 = temp * f01 + (t * t) * f10
        ft1 = ((1 - t) * (1 - t)) * f01 + temp * f10
        g0, g1 = interp_ref.backwarp(i0, ft0), interp_ref.backwarp(i1, ft1)
        x = _nhwc(torch.cat((i0, i1, f01, f10, ft1, ft0, g1, g0), 1))[0]
        assert np.array_equal(_bits(ft[k - 1]), _bits(_nhwc(torch.cat((ft0, ft1), 1))[0]))
        assert np.array_equal(_bits(row[k - 1, :, :, :14]), _bits(x[:, :, :14]))
        worst_g = max(worst_g, float(np.abs(row[k - 1, :, :, 14:20] - x[:, :, 14:]).max()))
        assert not row[k - 1, :, :, 20:].any()
        ok = o[k - 1 : k]
        ft0f, ft1f = ok[:, :2] + ft0, ok[:, 2:4] + ft1
        v0 = torch.sigmoid(ok[:, 4:5])
        v1 = 1 - v0
        g0f, g1f = interp_ref.backwarp(i0, ft0f), interp_ref.backwarp(i1, ft1f)
        w0, w1 = 1 - t, t
        p = (w0 * v0 * g0f + w1 * v1 * g1f) / (w0 * v0 + w1 * v1)
        pf = ((p[0] - (-mean)) / torch.ones(3).view(3, 1, 1)).mul(255).permute(1, 2, 0).numpy()  # to_u8 before .byte()
        exp_u8 = interp_ref.to_u8(p[0]).numpy()
        worst_p = max(worst_p, float(np.abs(pre[k - 1] - pf).max()))
        d = np.abs(u8[k - 1].astype(np.int32) - exp_u8.astype(np.int32))
        near = np.abs(pre[k - 1] - np.round(pre[k - 1])) < 1e-3
        print("composition k=%d: uint8 pixels differing %d of %d, near an integer %d" % (k, int((d > 0).sum()), d.size, int(near.sum())))
        assert int(d.max()) <= 1 and not (d > 0)[~near].any()
    print("composition: warped channels %.3e (bound %.2e), before truncation %.3e (bound %.2e)"
          % (worst_g, BACKWARP_TOL, worst_p, BACKWARP_TOL * 255))
    assert worst_g <= BACKWARP_TOL and worst_p <= BACKWARP_TOL * 255


def test_mid_and_fin_coefficients():
    """sf = 2: exactly -1/4, 1/4, 1/4, -1/4 and 1/2, 1/2; sf = 17 fills all 16 slots with distinct values."""
    assert R.mid_coef(2).tolist() == [[-0.25, 0.25, 0.25, -0.25]]
    assert [c.tolist() for c in R.fin_coef(2)] == [[0.5], [0.5]]
    c = R.mid_coef(17)
    assert c.shape == (16, 4) and len({tuple(r) for r in c.tolist()}) == 16
    assert np.array_equal(c[:, 0], c[:, 3]) and (c[:, 0] < 0).all() and (c[:, 1:3] > 0).all()
