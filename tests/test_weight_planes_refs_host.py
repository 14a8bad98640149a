"""The references of tests/weight_planes_refs.py (what tests/test_gpu_weight_planes_edges.py holds csrc/stem_train.hip's plane makers
to, word for word) pinned on the CPU: by hand on a few rows, against float64 on every edge input, and the package's torch route
(weight_planes._row_scaled_planes + fused_slowfast.split_planes: the stems, the 49- and 343-tap filters, weights that are not
channels-last) against the same contract and, bit for bit, against the references.

Every test prints the figures it asserts on (pytest -s shows them)."""
import numpy as np
import pytest
import torch

import weight_planes_refs as R

PLANES = [("bf16x3", R.BF16), ("f16x3", R.F16)]
_p = pytest.mark.parametrize


def _hex(a):
    return [hex(int(v)) for v in np.asarray(a).reshape(-1)]


# ---------------------------------------------------------------- by hand
def test_rows_by_hand_fp16():
    one_below = np.array([0x3F7FFFFF], np.uint32).view(np.float32)[0]  # 1 - 2^-24
    w = np.array([[1.0, 0.5],                 # frexp(1) = (0.5, 1): sc = 2^9, wscale = 2^-9; 512 = 0x6000, 256 = 0x5C00
                  [3.0, -0.0],                # e = 2: sc = 2^8; 768 = 0x6200, -0 keeps its sign in hi, lo = (-0) - (-0) = +0
                  [1.0, 1.0 + 2.0 ** -12],    # e = 1: 512 + 2^-3 -> hi 512 (step 0.5), lo 2^-3 = 0x3000
                  [one_below, 0.0],           # e = 0: sc = 2^10 -> 1024 - 2^-14: hi 1024 = 0x6400, lo -2^-14 = 0x8400
                  [0.0, 0.0]], np.float32)    # mx = 1e-30 = 0.63 * 2^-99: wscale = 2^-109
    hi, lo, ws = R.rows_ref(w, R.F16)
    assert _hex(hi) == _hex([0x6000, 0x5C00, 0x6200, 0x8000, 0x6000, 0x6000, 0x6400, 0x0000, 0, 0])
    assert _hex(lo) == _hex([0, 0, 0, 0, 0, 0x3000, 0x8400, 0, 0, 0])
    assert _hex(R.bits32(ws)) == _hex([0x3B000000, 0x3B800000, 0x3B000000, 0x3A800000, 0x09000000])


def test_rows_by_hand_bf16():
    w = np.array([[1.0, 1.0 + 2.0 ** -8], [-2.5, 2.0 ** -140]], np.float32)  # a tie rounds to even: hi 1, lo 2^-8; a bf16 denormal
    hi, lo, ws = R.rows_ref(w, R.BF16)
    assert ws is None
    assert _hex(hi) == _hex([0x3F80, 0x3F80, 0xC020, 0x0000])  # 2^-140 is below half the bf16 denormal step 2^-133: gone
    assert _hex(lo) == _hex([0, 0x3B80, 0, 0])


def test_transposed_gather_and_clip_by_hand():
    w = np.array([[[1.0], [2.0]], [[3.0], [4.0]]], np.float32)  # [cout 2][taps 2][cin 1]
    hi, lo = R.transposed_ref(w, [1, 0])
    assert hi.shape == (1, 2, 2) and _hex(hi) == _hex([0x4000, 0x4080, 0x3F80, 0x4040]) and not lo.any()  # [tap 1: 2, 4][tap 0: 1, 3]
    hi, lo, ws = R.gather_ref(np.array([1.0, 2.0], np.float32), np.array([[1, -1], [-1, -1]], np.int32), R.F16)
    assert _hex(hi) == _hex([0x6000, 0, 0, 0]) and not lo.any() and _hex(R.bits32(ws)) == _hex([0x3B800000, 0x09000000])
    hi, lo = R.clip_ref(np.array([1.0, 2.0, 3.0], np.float32).reshape(1, 3, 1, 1, 1), R.BF16)
    assert hi.shape == (1, 1, 1, 1, 4) and _hex(hi) == _hex([0x3F80, 0x4000, 0x4040, 0]) and not lo.any()
    x = R.clip_values((2, 3, 1, 3, 5))
    hi, lo = R.clip_ref(x, R.F16)
    assert not hi[..., 3].any() and not lo[..., 3].any()
    e_hi, e_lo = R.split(x, R.F16)
    assert np.array_equal(hi[..., :3], np.moveaxis(e_hi, 1, -1)) and np.array_equal(lo[..., :3], np.moveaxis(e_lo, 1, -1))


def test_the_edge_inputs_hold_what_they_are_named_for():
    for K in R.ROW_KS:
        names, w = R.edge_rows(K)
        assert w.shape == (len(names), K) and w.dtype == np.float32 and len(set(names)) == len(names)
        mx = R.finite_max(w)
        for i, m in enumerate(R.scale_edge_maxima()):
            assert mx[i] == m
        row = dict(zip(names, w))
        assert (np.abs(row["below_1e-30_with_denormals"]) < 1e-30).all() and (np.abs(row["below_1e-30_with_denormals"]) < 2.0 ** -126).any()
        assert np.signbit(row["all_negative_zero"]).all() and np.isnan(row["nan_beside_finite_entries"]).sum() == min(2, K - 1)
        assert np.abs(row["max_at_column_0"]).argmax() == 0 and np.abs(row["max_at_last_column"]).argmax() == K - 1
        c = np.abs(row["max_in_second_trip"]).argmax()
        assert c == R.second_trip_column(K) and (K <= 256 or 256 <= c < 512)
        assert np.isfinite(w[~np.isnan(w)]).all() and np.isinf(R.inf_rows(K)).sum() == 2
    x = R.clip_values((1, 3, 1, 1, 257))
    for v in np.concatenate([R.CLIP_VALUES, R.CLIP_DENORMALS]):
        assert (np.isnan(x).any() if np.isnan(v) else ((x == v) & (np.signbit(x) == np.signbit(v))).any()), v


# ---------------------------------------------------------------- the contract against float64
def _check_contract(w, hi, lo, ws, plane, what):
    ratio, scaled = R.contract_ratio(w, hi, lo, ws, plane)
    nan = np.isnan(w)
    back = R.scaled_back(hi, lo, ws, plane)
    assert np.array_equal(np.isnan(back), nan) or plane == R.BF16, "a NaN moved"
    if plane == R.BF16:  # beyond BF16_TOP the high plane is an infinity and the low one the opposite infinity: the pair joins to a NaN
        top = np.abs(w) > R.BF16_TOP
        assert np.array_equal(np.isnan(back), nan | top)
    msg = "%s: worst error / bound %.3f" % (what, ratio)
    if scaled is not None:
        big = R.finite_max(w) >= np.float32(1e-30)
        msg += ", scaled maxima in [%.6f, %.6f] * 2^9" % (scaled[big].min() / 512, scaled[big].max() / 512)
        assert (scaled[big] >= 512).all() and (scaled[big] < 1024).all(), msg
    print(msg)
    assert ratio <= 1.0, msg
    return ratio


@_p("K", R.ROW_KS)
@_p("name,plane", PLANES)
def test_rows_ref_keeps_the_contract_on_every_edge_row(K, name, plane):
    _, w = R.edge_rows(K)
    hi, lo, ws = R.rows_ref(w, plane)
    _check_contract(w, hi, lo, ws, plane, "rows_ref %s K=%d" % (name, K))
    if plane == R.F16:  # the scale is a power of two and undoes itself exactly
        m, _ = np.frexp(ws)
        assert (m == 0.5).all() and (ws > 0).all() and np.isfinite(ws).all()
        # a NaN stays a NaN at its place only
        back = R.scaled_back(hi, lo, ws, plane)
        assert np.array_equal(np.isnan(back), np.isnan(w))


@_p("name,plane", PLANES)
def test_rows_ref_is_scale_invariant(name, plane):
    """planes(w * 2^s) are the words of planes(w) and wscale is multiplied by exactly 2^s (fp16 planes; bf16 planes have no scale)."""
    _, w = R.edge_rows(514)
    keep = (R.finite_max(w) >= 2.0 ** -60) & (R.finite_max(w) <= 2.0 ** 100)  # (the shifted row must stay clear of the clamp and of FLT_MAX)
    w = w[keep]
    s = R.scale_shifts(len(w))
    w2 = (w * np.ldexp(np.float32(1), s)[:, None]).astype(np.float32)
    a, b = R.rows_ref(w, plane), R.rows_ref(w2, plane)
    if plane == R.F16:
        assert R.same_words(a[0], b[0], plane).all() and R.same_words(a[1], b[1], plane).all()
        assert np.array_equal(R.bits32(b[2]), R.bits32(a[2] * np.ldexp(np.float32(1), s)))
    else:
        assert np.array_equal(R.plane_f32(b[0], plane), R.plane_f32(a[0], plane) * np.ldexp(np.float32(1), s)[:, None], equal_nan=True)


@_p("name,plane", PLANES)
def test_clip_ref_and_transposed_ref_keep_the_split(name, plane):
    x = R.clip_values((2, 3, 3, 5, 7), key=1)
    hi, lo = R.clip_ref(x, plane)
    fin = np.isfinite(x) & (np.abs(x) <= (65504.0 if plane == R.F16 else R.BF16_TOP))
    back = np.moveaxis(R.join(hi, lo, plane)[..., :3], -1, 1).astype(np.float64)
    tol = np.maximum(2.0 ** -22 * np.abs(x), 2.0 ** -24) if plane == R.F16 else np.maximum(2.0 ** -16 * np.abs(x), 2.0 ** -134)
    assert (np.abs(back[fin] - x[fin]) <= tol[fin]).all()
    if plane == R.F16:  # finite values beyond the range clamp, an infinity stays that infinity, a NaN a NaN
        assert (np.abs(back[np.isfinite(x) & (np.abs(x) > 65504)]) == 65504).all()
        assert np.array_equal(back[np.isinf(x)], x[np.isinf(x)]) and np.isnan(back[np.isnan(x)]).all()
    for cout, taps, cin in R.T_SHAPES:
        w = R.transposed_weight(cout, taps, cin)
        for sel in R.transposed_sels(taps).values():
            th, tl = R.transposed_ref(w, sel)
            assert th.shape == (cin, len(sel), cout)
            for a, tap in enumerate(sel):
                eh, el = R.split(np.ascontiguousarray(w[:, tap, :].T), R.BF16)
                assert np.array_equal(th[:, a, :], eh) and np.array_equal(tl[:, a, :], el)


# ---------------------------------------------------------------- the package's torch route
def _torch_rows(w, plane):
    from avtex import ops, weight_planes
    from avtex.fused_slowfast import split_planes

    t = torch.from_numpy(np.ascontiguousarray(w))
    if plane == R.BF16:
        hi, lo = split_planes(t, ops.X3_BF16)
        return R.words(hi), R.words(lo), None
    hi, lo, sc = weight_planes._row_scaled_planes(t)
    return R.words(hi), R.words(lo), (1.0 / sc).float().numpy()


@_p("K", R.ROW_KS)
@_p("name,plane", PLANES)
def test_the_torch_route_keeps_the_contract_and_equals_rows_ref(avt, K, name, plane):
    """The same rows through weight_planes._row_scaled_planes / fused_slowfast.split_planes: the contract, then the reference's bits.
    (Until the exponent came from torch.frexp, 2^(9 - floor(log2(mx))) in fp32 gave HALF the scale for a maximum one ulp below a power
    of two — log2 rounds up to the integer — and the scaled maximum lay just under 2^9: profiles/r29/README.md lists the rows.)"""
    names, w = R.edge_rows(K)
    hi, lo, ws = _torch_rows(w, plane)
    e_hi, e_lo, e_ws = R.rows_ref(w, plane)
    if plane == R.F16:
        bad = np.flatnonzero(R.bits32(ws) != R.bits32(e_ws))
        for r in bad:
            print("row %d %s: max %r, wscale %r, reference %r" % (r, names[r], float(R.finite_max(w)[r]), float(ws[r]), float(e_ws[r])))
        assert len(bad) == 0, "%d rows with another scale than the kernel's" % len(bad)
    _check_contract(w, hi, lo, ws, plane, "torch route %s K=%d" % (name, K))
    assert R.same_words(hi, e_hi, plane).all() and R.same_words(lo, e_lo, plane).all()


def test_the_torch_route_on_a_row_with_an_infinity(avt):
    """What the kernel's test pins, on the torch route: the infinity comes back as that infinity, wscale is a finite positive power of
    two, every other row is the reference's."""
    w = R.inf_rows(514)
    hi, lo, ws = _torch_rows(w, R.F16)
    back = R.scaled_back(hi, lo, ws, R.F16)
    assert back[1, 1] == np.inf and back[2, 0] == -np.inf and np.isinf(back).sum() == 2
    m, _ = np.frexp(ws)
    assert np.isfinite(ws).all() and (ws > 0).all() and (m == 0.5).all()
    e_hi, e_lo, e_ws = R.rows_ref(w, R.F16)
    for r in (0, 3):
        assert np.array_equal(hi[r], e_hi[r]) and np.array_equal(lo[r], e_lo[r]) and R.bits32(ws)[r] == R.bits32(e_ws)[r]
