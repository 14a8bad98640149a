"""CPU proof of tests/nxn_refs.py, the references of tests/test_gpu_nxn_edges.py: the references against hand-computed
rows and against each other, the exactness condition of every exact_gemm shape, and the C oracle (oracle/cref) against
the references on every edge input the GPU suite feeds the kernels, so that the GPU suite's bit-exact comparisons with
the oracle are not circular.  Every test prints the figures it asserts on (pytest -s shows them)."""
import numpy as np
import pytest

import nxn_refs as R
from oracle import cref

U = R.U


# ---------------------------------------------------------------- the references themselves
def test_l2norm_refs_by_hand():
    x = np.array([[3.0, 4.0], [0.0, 0.0], [1e-20, 0.0]], np.float32)
    y = R.l2norm64(x)
    assert np.allclose(y[0], [0.6, 0.8], rtol=1e-15) and (y[1] == 0).all()
    assert y[2, 0] == float(np.float32(1e-20)) / 1e-12  # a norm below eps: x / eps
    t = R.l2norm_torch(x)
    assert np.abs(t - y).max() <= 2 * U * np.abs(y).max()
    # fp32 semantics: NaN poisons its row, inf gives zeros and one NaN, a sum of squares past the fp32 range gives zeros
    s = np.ones((4, 8), np.float32)
    s[0, 2] = np.nan
    s[1, 2] = np.inf
    s[2] = 1e19
    t = R.l2norm_torch(s)
    assert np.isnan(t[0]).all()
    assert np.isnan(t[1, 2]) and (np.delete(t[1], 2) == 0).all()
    assert (t[2] == 0).all() and float((s[2].astype(np.float64) ** 2).sum()) > R.F32_SUM_OVERFLOW
    assert np.allclose(t[3], 8 ** -0.5)
    assert R.same_with_nan(t, t.copy()) and not R.same_with_nan(t, np.zeros_like(t))


def test_row_select_refs_by_hand_and_against_each_other():
    for L in (8, 256):
        x = R.exact_rows(L)
        for ref in (R.row_select_ref, R.row_select64):
            o = ref(x[0], threshold=0.0)
            assert o["cnt"] == L and (np.asarray(o["p"]) == 1.0 / L).all() and o["row_sum"] == 3 * L and o["row_max"] == 1.0 / L
            for th, (idx, p) in R.EXACT_ROW1.items():
                o = ref(x[1], threshold=th)
                assert o["idx"].tolist() == idx and o["row_sum"] == 8 and o["row_max"] == 0.5, (L, th)
                assert np.abs(np.asarray(o["p"], np.float64) - np.asarray(p, np.float64)).max() <= U, (L, th)
    # the [pos] + others order (validate.py:369-378)
    assert R.target_order(0, 5).tolist() == [1, 2, 3, 4]
    assert R.target_order(2, 5).tolist() == [3, 0, 1, 4]
    assert R.target_order(3, 5).tolist() == [4, 0, 1, 2]
    assert R.target_order(4, 5).tolist() == [4, 0, 1, 2, 3]
    # torch fp32 and fp64 agree on the gap rows: same survivors, p within fp32 noise of a 4100-term sum
    for W in (300, 4100):
        x = R.gap_rows(4, W, 1)
        xa = R.gap_rows(4, W, 2, [np.nonzero(row > 3.0)[0] for row in x], m=0.7)  # (the audio row's survivors in the same places)
        worst = 0.0
        for r in range(4):
            for kw in (dict(threshold=0.3), dict(threshold=0.3, xa=xa[r], alpha=0.5)):
                a, b = R.row_select_ref(x[r], **kw), R.row_select64(x[r], **kw)
                assert np.array_equal(a["idx"], b["idx"]) and a["cnt"] == r + 1  # (gap_rows: row r has r + 1 survivors)
                worst = max(worst, float((np.abs(a["p"] - b["p"]) / b["p"]).max()))
        print("row_select_ref vs row_select64, W=%d: p %.2f u" % (W, worst / U))
        assert worst <= 1e-5
    # special values, by the reference's own lines
    o = R.row_select_ref(np.array([1, np.nan, 3, 2], np.float32), threshold=0.3)
    assert o["cnt"] == 4 and np.isnan(o["p"]).all() and np.isnan(o["row_max"])
    o = R.row_select_ref(np.array([1, np.inf, 3, 2], np.float32), threshold=0.3)
    assert o["idx"].tolist() == [1] and np.isnan(o["p"]).all() and np.isnan(o["row_max"])
    o = R.row_select_ref(np.array([1, -1, 0, 0], np.float32), threshold=0.3)
    assert o["cnt"] == 4 and np.isnan(o["p"]).all() and np.isnan(o["row_max"])


def test_topk_ref_by_hand():
    x = np.array([[1, np.nan, 3, 2, -np.inf]], np.float32)
    idx, val = R.topk_ref(x, 5, np.array([0]))
    assert idx.tolist() == [[2, 3, 4, -1, -1]]
    assert val.tolist() == [[3.0, 2.0, -np.inf, -np.inf, -np.inf]]
    idx, _ = R.topk_ref(np.array([[2, 7, 7, 1, 7]], np.float32), 4)
    assert idx.tolist() == [[1, 2, 4, 0]]  # ties: the lower column first


@pytest.mark.parametrize("mode,d", R.exact_shapes())
def test_exact_gemm_condition_holds(mode, d):
    """The worst case of sum |terms|, in integer units (2^-8 in the bf16 modes), stays below 2^24 at every depth the GPU
    suite uses; exact_gemm asserts the same on the data it draws."""
    worst = {"f32": 64, "bf16": 4 * 256, "bf16x3": 4 * 256 + 8}[mode] * d
    c = R.exact_gemm(mode, 3, 2, d)
    print("%s d=%d: sum |terms| <= %d (drawn: %d) of %d" % (mode, d, worst, c["bound"], R.EXACT_LIMIT))
    assert c["bound"] <= worst < R.EXACT_LIMIT


def test_exact_gemm_by_hand():
    c = R.exact_gemm("bf16x3", 2, 3, 5, temp=0.1)
    v = lambda k: R.bf16_value(c[k]).astype(np.float64)
    full = (v("qh") + v("ql")) @ (v("th") + v("tl")).T
    lolo = v("ql") @ v("tl").T
    assert np.array_equal(c["acc"], full - lolo) and np.abs(lolo).max() > 0  # hi hi + hi lo + lo hi, and lo lo would show
    assert np.array_equal(c["expect"], (c["acc"].astype(np.float32) / np.float32(0.1)))
    assert np.abs(v("ql")).max() == 2.0 / 256 and np.abs(v("qh")).max() == 2.0
    assert not np.array_equal(c["ql"][:2, :5], c["tl"][:2, :5])  # drawn independently


# ---------------------------------------------------------------- the C oracle against the references
@pytest.mark.parametrize("d0,d1", R.L2_WIDTHS)
def test_oracle_l2norm_widths(d0, d1):
    for n in R.L2_ROWS:
        x0, x1 = R.l2norm_input(n, d0, d1)
        y, hi, lo = cref.l2norm_rows(x0, x1)
        R.check_l2norm("oracle n=%d d=%d+%d" % (n, d0, d1), y, hi, lo, x0, x1)


@pytest.mark.parametrize("d0,d1", R.L2_SCALE_WIDTHS)
@pytest.mark.parametrize("scale", R.L2_SCALES)
def test_oracle_l2norm_scales(scale, d0, d1):
    x0, x1 = R.l2norm_input(5, d0, d1, scale=scale)
    y, hi, lo = cref.l2norm_rows(x0, x1)
    R.check_l2norm("oracle scale=%g d=%d" % (scale, d0 + d1), y, hi, lo, x0, x1)
    if scale == 1e18 and d0 + d1 >= 3072:
        assert (y == 0).all()  # the sum of squares is past the fp32 range: F.normalize's zeros


@pytest.mark.parametrize("d0,d1", R.L2_SPECIAL_WIDTHS)
@pytest.mark.parametrize("special", R.L2_SPECIAL)
def test_oracle_l2norm_special_rows(special, d0, d1):
    """Fix 1 in the oracle: a NaN entry gives an all-NaN row (it gave 1e12-sized finite values)."""
    x0, x1 = R.l2norm_input(5, d0, d1, special=special)
    y, hi, lo = cref.l2norm_rows(x0, x1)
    R.check_l2norm("oracle %s d=%d+%d" % (special, d0, d1), y, hi, lo, x0, x1)
    row, col = 2, (d0 + d1) // 3
    if special == "nan":
        assert np.isnan(y[row]).all()
    elif special == "inf":
        assert np.isnan(y[row, col]) and (np.delete(y[row], col) == 0).all()
    else:
        assert (y[row] == 0).all()
    assert np.isfinite(np.delete(y, row, axis=0)).all()


def _f32_shapes():
    return R.SIM_F32_V2 + [R.SIM_F32_R2_SHAPE + (d,) for d in R.SIM_F32_R2_D] + [R.SIM_F32_R2_SHAPE + (64,)]


@pytest.mark.parametrize("nq,nt,d", _f32_shapes())
def test_oracle_sim_f32_equals_exact_gemm(nq, nt, d):
    c = R.exact_gemm("f32", nq, nt, d)
    out = cref.sim_f32(c["q"], c["t"], c["temp"])
    assert np.array_equal(out.view(np.uint32), c["expect"].view(np.uint32))
    if nq * nt * d < 1e6:
        assert np.array_equal(cref.sim_f32(c["q"], c["t"], c["temp"], naive=True).view(np.uint32), c["expect"].view(np.uint32))


def _bf16_shapes():
    s = [(nq, nt, d) for d in R.SIM_BF16_D for nq, nt in R.SIM_BF16_SHAPES] + [R.SIM_BF16_LONG]
    return [(m,) + x for m in ("bf16", "bf16x3") for x in s] + [("bf16x3",) + x for x in R.SIM_XL_SHAPES]


@pytest.mark.parametrize("mode,nq,nt,d", _bf16_shapes())
def test_oracle_sim_bf16_equals_exact_gemm(mode, nq, nt, d):
    c = R.exact_gemm(mode, nq, nt, d)
    out = cref.sim_bf16(c["qh"], c["ql"], c["th"], c["tl"], c["temp"], mode == "bf16x3")
    assert np.array_equal(out.view(np.uint32), c["expect"].view(np.uint32))


@pytest.mark.parametrize("group", R.TR_GROUPS)
def test_oracle_row_transition(group):
    for case in R.transition_cases(group):
        o = cref.row_transition(case["sim"], q_ids=case["q_ids"], sim_a=case["sim_a"], alpha=case["alpha"],
                                threshold=case["threshold"], cap=case["cap"])
        R.check_select(o, case, "oracle")


def test_oracle_exact_rows_bit_for_bit():
    R.check_exact_rows(lambda x, th, cap: cref.row_transition(x, threshold=th, cap=cap))


def test_oracle_row_max_propagates_nan():
    """Fix 2 in the oracle: a NaN p anywhere makes row_max NaN, as output.max() does; it used to need the NaN at p[0]."""
    x = np.array([[1, 2, np.inf, 4], [np.inf, 2, 3, 4], [0, 0, 0, 0], [1, -1, 0, 0], [1, 2, np.nan, 4]], np.float32)
    o = cref.row_transition(x, threshold=0.3, cap=4)
    assert np.isnan(o["stats"][:, 1]).all()
    assert o["cnt"].tolist() == [1, 1, 4, 4, 4]
    assert o["idx"][0, 0] == 2 and o["idx"][1, 0] == 0
    # finite rows are untouched: the maximum of finite values is the same by either rule
    y = R.gap_rows(7, 300, 3)
    o = cref.row_transition(y, threshold=0.3, cap=8)
    p = y.astype(np.float64) / y.astype(np.float64).sum(axis=1, keepdims=True)
    assert np.abs(o["stats"][:, 1] - p.max(axis=1)).max() <= 2.01 * U * p.max()


@pytest.mark.parametrize("nt", R.TOPK_WIDTHS)
def test_oracle_topk_equals_topk_ref(nt):
    """Fix 3 in the oracle: a NaN score is never picked, whatever its column."""
    x, self_col = R.topk_input(nt)
    for k in sorted({1, min(nt, 40), nt, nt + 3}):
        for sc in (self_col, None):
            oi, ov = cref.row_topk(x, k, sc)
            ri, rv = R.topk_ref(x, k, sc)
            assert np.array_equal(oi, ri), (nt, k)
            assert np.array_equal(ov, rv), (nt, k)
            assert not np.isnan(ov).any()
    oi, ov = cref.row_topk(np.array([[1, np.nan, 3, 2, -np.inf]], np.float32), 5, np.array([0], np.int64))
    assert oi.tolist() == [[2, 3, 4, -1, -1]]  # (it picked the NaN first: [1, 2, 3, 4, -1])
