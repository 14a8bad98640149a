"""The restatements of tests/pack_pool_refs.py (what tests/test_gpu_pack_pool_edges.py holds csrc/clip_pack.hip and
csrc/pool.hip to, bit for bit) pinned on the CPU: the clip packing to oracle/ref_py.pack_clip (torch fp32), the source
index to its invariants, the plane split to the package's host split_planes and to the bounds csrc/split_planes.h
states, and the head mean to an fp64 mean — and shown to differ from a plain sequential sum, so that the order is pinned.

Every test prints the figures it asserts on (pytest -s shows them)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pack_pool_refs as R
from oracle import ref_py


def _gen(*key):
    return torch.Generator().manual_seed(int(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key))) + 31)


# ---------------------------------------------------------------- clip packing
@pytest.mark.parametrize("H,W,hw", [(128, 128, 224), (90, 120, 224), (360, 640, 224), (480, 854, 224), (37, 53, 98),
                                    (1, 1, 8), (3, 1000, 6)])
def test_pack_clip_matches_the_oracle(H, W, hw):
    """Six roundings at most on values <= max|LUT| lie between the two fp32 evaluations (torch blends rows first and has
    its own operation order): 8 units of 2^-24 max|LUT| leave two of slack."""
    win_len, start = 20, 2
    frames = torch.randint(0, 256, (start + win_len + 1, H, W, 3), generator=_gen(H, W, hw), dtype=torch.uint8)
    slow, fast = R.pack_clip(frames.numpy(), start, win_len, hw)
    eslow, efast = ref_py.pack_clip(frames, start, win_len, out_hw=hw)
    assert slow.shape == (3, 8, hw, hw) and fast.shape == (3, 32, hw, hw) and slow.dtype == np.float32
    tol = 8 * 2.0 ** -24 * float(np.abs(R.norm_lut(0.45, 0.225)).max())
    d = max(float(np.abs(slow - eslow.numpy()).max()), float(np.abs(fast - efast.numpy()).max()))
    # for information: the fp64 bilinear of the same frames (the source index is fp32 in torch and in the kernel, so this
    # differs by far more at wide sources)
    x = frames[start : start + win_len].double() / 255
    x = ((x[..., [2, 1, 0]] - 0.45) / 0.225).permute(3, 0, 1, 2)
    f64 = F.interpolate(x[:, torch.from_numpy(R.sample_indices(win_len)[0])], size=(hw, hw), mode="bilinear")
    d64 = float((torch.from_numpy(fast).double() - f64).abs().max())
    print("pack_clip %dx%d -> %d: |restatement - oracle| %.3g (tolerance %.3g), |restatement - fp64 bilinear| %.3g"
          % (H, W, hw, d, tol, d64))
    assert d <= tol


def test_pack_clip_bgr_mean_std_and_sampling():
    """bgr = False, another mean / std, and window lengths on both sides of 32 against the oracle."""
    frames = torch.randint(0, 256, (60, 21, 17, 3), generator=_gen(5), dtype=torch.uint8)
    for win_len, start, bgr, mean, std in [(1, 59, True, 0.45, 0.225), (7, 3, False, 0.3, 0.5), (33, 0, True, 0.45, 0.225),
                                           (50, 10, False, 0.3, 0.5)]:
        slow, fast = R.pack_clip(frames.numpy(), start, win_len, 12, mean, std, bgr)
        eslow, efast = ref_py.pack_clip(frames, start, win_len, out_hw=12, mean=mean, std=std, bgr=bgr)
        tol = 8 * 2.0 ** -24 * float(np.abs(R.norm_lut(mean, std)).max())
        assert np.abs(slow - eslow.numpy()).max() <= tol and np.abs(fast - efast.numpy()).max() <= tol
        fi, si = R.sample_indices(win_len)
        ofi, osi = ref_py.sample_indices(win_len)
        assert np.array_equal(fi, ofi) and np.array_equal(si, osi)


@pytest.mark.parametrize("n_out", [1, 2, 7, 98, 224])
def test_src_index_invariants(n_out):
    for n_in in list(range(1, 65)) + [224, 360, 854]:
        i0, i1, l1 = R.src_index(R.src_scale(n_in, n_out), n_out, n_in)
        assert l1.dtype == np.float32 and len(i0) == len(i1) == len(l1) == n_out
        assert (0 <= i0).all() and (i0 <= i1).all() and (i1 <= n_in - 1).all() and (i1 - i0 <= 1).all()
        assert (l1 >= 0).all()
        assert ((l1 < 1) | (i0 == i1)).all()  # clamped onto the last pixel, the weight multiplies two equal taps
        # against the index in exact arithmetic: the tap may move only where s is within fp32 rounding of an integer
        s = np.maximum((n_in / n_out) * (np.arange(n_out) + 0.5) - 0.5, 0.0)
        e0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
        pos = i0 + np.where(i0 == i1, 0.0, l1.astype(np.float64))  # the sampled position
        assert np.abs(pos - np.minimum(s, n_in - 1)).max() <= 2.0 ** -22 * n_in and (np.abs(i0 - e0) <= 1).all()


# ---------------------------------------------------------------- split / join
_EDGES = [0.0, -0.0, 65504.0, -65504.0, 65520.0, 1e5, -1e5, 2.0 ** -3, 2.0 ** -14, 2.0 ** -24, 6e-8, -6e-8]


@pytest.mark.parametrize("plane", ["bf16x3", "f16x3"])
def test_split_is_the_packages_split_planes_bit_for_bit(avt, plane):
    from avtex import ops
    from avtex.fused_slowfast import split_planes

    pd = R.PLANE[plane]
    assert (R.BF16, R.F16) == (ops.X3_BF16, ops.X3_F16)
    rnd = torch.randn(8192, generator=_gen(pd, 1)) * torch.logspace(-9, 4.5, 8192)
    x = torch.cat([rnd, torch.tensor(_EDGES, dtype=torch.float32)])
    hi, lo = R.split(x, pd)
    ph, pl = split_planes(x, pd)
    assert np.array_equal(hi, R.words(ph)) and np.array_equal(lo, R.words(pl))
    # infinities and NaNs: the same words where the value is not a NaN, a NaN where it is one (its payload is nobody's promise)
    sp = torch.tensor([float("inf"), float("-inf"), float("nan"), -float("nan")], dtype=torch.float32)
    for (a, b) in zip(R.split(sp, pd), split_planes(sp, pd)):
        fa, fb = R.plane_f32(a, pd), R.plane_f32(R.words(b), pd)
        assert np.array_equal(np.isnan(fa), np.isnan(fb)) and np.array_equal(a[~np.isnan(fa)], R.words(b)[~np.isnan(fb)])
    v = R.join(*R.split(sp, pd), pd)
    assert np.isnan(v[2]) and np.isnan(v[3])
    if pd == R.F16:  # an infinity stays that infinity (hi = +-inf, lo = 0); a NaN's lo is 0 too
        assert v[0] == np.inf and v[1] == -np.inf and np.array_equal(R.split(sp, pd)[1], np.zeros(4, np.uint16))


@pytest.mark.parametrize("plane", ["bf16x3", "f16x3"])
def test_join_of_split_is_within_the_stated_bounds(plane):
    """csrc/split_planes.h: bf16 planes |x - hi - lo| <= 2^-16 |x| at every magnitude; fp16 planes <= 2^-22 |x| while lo is a
    normal fp16, 2^-24 absolute below; finite values beyond the fp16 range clamp to +-65504."""
    pd = R.PLANE[plane]
    rnd = (torch.randn(8192, generator=_gen(pd, 2)) * torch.logspace(-9, 4.5, 8192)).numpy()
    x = np.concatenate([rnd[np.abs(rnd) <= 65504.0], np.array(_EDGES[:4] + _EDGES[7:], np.float32)])
    v = R.join(*R.split(x, pd), pd)
    err, mag = np.abs(v.astype(np.float64) - x), np.abs(x).astype(np.float64)
    bound = mag * 2.0 ** -16 if pd == R.BF16 else np.maximum(mag * 2.0 ** -22, 2.0 ** -24)
    print("%s: worst split/join error / bound %.3f" % (plane, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all()
    big = np.array([65520.0, 1e5, -1e5, 3e38], np.float32)
    if pd == R.F16:
        assert np.array_equal(R.join(*R.split(big, pd), pd), np.array([65504.0, 65504.0, -65504.0, 65504.0], np.float32))
        assert np.array_equal(R.split(np.array([0.0, -0.0], np.float32), pd)[0], np.array([0, 0x8000], np.uint16))
    else:
        assert (np.abs(R.join(*R.split(big, pd), pd).astype(np.float64) - big) <= np.abs(big) * 2.0 ** -16).all()


# ---------------------------------------------------------------- head mean
@pytest.mark.parametrize("P", [1, 7, 31, 32, 33, 392])
def test_mean_positions_against_fp64(P):
    x = (torch.randn(P, 72, generator=_gen(P)) + 0.25).numpy()
    got = R.mean_positions(x)
    assert got.dtype == np.float32 and got.shape == (72,)
    err = float(np.abs(got.astype(np.float64) - x.astype(np.float64).mean(0)).max())
    bound = P * 2.0 ** -24 * float(np.abs(x).max())
    print("mean_positions P=%d: |restatement - fp64 mean| %.3g (bound %.3g)" % (P, err, bound))
    assert err <= bound


def test_mean_positions_pins_the_order():
    """At P = 392 (the slow head: 8 x 7 x 7) the 32-group order gives other bits than a plain sequential fp32 sum, and than
    the same groups reduced from the last to the first: a kernel that summed in either of those orders would not pass."""
    x = (torch.randn(392, 64, generator=_gen(392, 1)) + 0.25).numpy()
    got = R.mean_positions(x)
    seq = np.zeros(64, np.float32)
    for r in range(392):
        seq = seq + x[r]
    seq = seq / np.float32(392)
    acc = np.zeros((32, 64), np.float32)
    for r in range(392):
        acc[r % 32] = acc[r % 32] + x[r]
    rev = np.zeros(64, np.float32)
    for g in range(31, -1, -1):
        rev = rev + acc[g]
    rev = rev / np.float32(392)
    n_seq, n_rev = int((R.bits(got) != R.bits(seq)).sum()), int((R.bits(got) != R.bits(rev)).sum())
    print("mean_positions P=392: %d of 64 channels differ from a sequential sum, %d from the reversed reduce" % (n_seq, n_rev))
    assert n_seq >= 1 and n_rev >= 1
