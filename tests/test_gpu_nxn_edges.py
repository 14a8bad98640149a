"""The N x N build of validate() at its edges: csrc/l2norm.hip, csrc/sim_gemm.hip (both f32 tiles, the bf16 / bf16x3 tile,
the 256 x 256 tile behind avt_gemm_nt_x3_f32out) and csrc/transition.hip (row_transition, row_topk), each against the
references of tests/nxn_refs.py (proved on the CPU by test_nxn_refs_host.py, which also holds the C oracle to them on
these very inputs) and bit for bit against the C oracle where the build defines a canonical order.

Dispatch boundaries from both sides, ragged tiles, pitched rows and outputs behind sentinels, NULL optional outputs,
operands past 4 GiB, and special values (NaN, +-inf, zero rows), which are ordinary data for these kernels.
Every bound is derived where it is used (here or in nxn_refs.py); every test prints the figures it asserts on."""
import numpy as np
import pytest
import torch

import nxn_refs as R
from oracle import cref

pytestmark = pytest.mark.gpu

SENT = 7.0  # what every output buffer holds before a call (a bf16 number too); -7 in the integer outputs
SENT_I = -7


def _t(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bf(bits, dev):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16).to(dev)


def _u16(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _same_bits(a, b):
    """Bit for bit, except that any NaN equals any NaN (the CPU and the GPU differ in the sign and payload they generate)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == np.uint16:
        a, b = R.bf16_value(a), R.bf16_value(b)
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def _off_by_one_float(a, dev):
    """The array on the device, contiguous, its first element 4 bytes past a 16-byte boundary."""
    flat = torch.empty(a.size + 4, dtype=torch.float32, device=dev)
    v = flat[1 : 1 + a.size].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# ---------------------------------------------------------------- l2norm
def _l2(avt, dev, x0, x1, want=("y", "hi", "lo"), x0_dev=None):
    """One raw avt_l2norm_rows call into buffers of n + 1 rows: the guard row keeps its sentinel.  -> (y, hi bits, lo bits)"""
    P, n, d0 = avt.ops._p, x0.shape[0], x0.shape[1]
    d1 = 0 if x1 is None else x1.shape[1]
    tx0, tx1 = (_t(x0, dev) if x0_dev is None else x0_dev), _t(x1, dev)
    y = torch.full((n + 1, d0 + d1), SENT, device=dev) if "y" in want else None
    hi = torch.full((n + 1, d0 + d1), SENT, device=dev, dtype=torch.bfloat16) if "hi" in want else None
    lo = torch.full((n + 1, d0 + d1), SENT, device=dev, dtype=torch.bfloat16) if "lo" in want else None
    avt.ops.K.avt_l2norm_rows(P(tx0), d0, P(tx1), d1, n, 1e-12, P(y), P(hi), P(lo), avt.ops._stream())
    for o in (y, hi, lo):
        assert o is None or bool((o[n].float() == SENT).all()), "the row after the last was written"
    return (None if y is None else y[:n].cpu().numpy(), None if hi is None else _u16(hi[:n]), None if lo is None else _u16(lo[:n]))


def _l2_check(avt, dev, who, x0, x1, **kw):
    y, hi, lo = _l2(avt, dev, x0, x1, **kw)
    oy, ohi, olo = cref.l2norm_rows(x0, x1)
    assert _same_bits(y, oy) and _same_bits(hi, ohi) and _same_bits(lo, olo), who + ": not the oracle's bits"
    R.check_l2norm(who, y, hi, lo, x0, x1)
    return y, hi, lo


@pytest.mark.parametrize("d0,d1", R.L2_WIDTHS)
def test_l2norm_widths_and_rows(avt, dev, d0, d1):
    """Across the register cache (3072 elements), the production split 2304 + 768, the scalar kernel's widths (d1 % 4 != 0;
    d = 1, 2, 3, 63, 65), with 1, 4 and 5 rows (four rows per workgroup)."""
    for n in R.L2_ROWS:
        x0, x1 = R.l2norm_input(n, d0, d1)
        _l2_check(avt, dev, "n=%d d=%d+%d" % (n, d0, d1), x0, x1)


@pytest.mark.parametrize("d", [256, 3076])
def test_l2norm_misaligned_input_takes_the_scalar_kernel(avt, dev, d):
    x0, _ = R.l2norm_input(5, d, 0)
    _l2_check(avt, dev, "x0 4 bytes off, d=%d" % d, x0, None, x0_dev=_off_by_one_float(x0, dev))


@pytest.mark.parametrize("d0,d1", [(256, 0), (3076, 0), (65, 0)])
def test_l2norm_each_output_subset_alone(avt, dev, d0, d1):
    x0, x1 = R.l2norm_input(5, d0, d1)
    y, hi, lo = _l2(avt, dev, x0, x1)
    for want in (("y",), ("hi", "lo"), ("lo",), ("hi",)):
        sy, shi, slo = _l2(avt, dev, x0, x1, want=want)
        for name, full, sub in (("y", y, sy), ("hi", hi, shi), ("lo", lo, slo)):
            assert (sub is None) == (name not in want)
            assert sub is None or np.array_equal(sub, full), (want, name)
    print("d=%d+%d: y | hi+lo | lo | hi alone equal the full call; guard rows intact" % (d0, d1))


@pytest.mark.parametrize("d0,d1", R.L2_SCALE_WIDTHS)
@pytest.mark.parametrize("scale", R.L2_SCALES)
def test_l2norm_scales(avt, dev, scale, d0, d1):
    """1e-30 and 1e-20: the norm is below eps, y = x / eps.  1e18 at d >= 3072: the sum of squares is past the fp32 range,
    the norm is inf and the row is F.normalize's zeros (check_l2norm takes torch as the reference there)."""
    x0, x1 = R.l2norm_input(5, d0, d1, scale=scale)
    y, _, _ = _l2_check(avt, dev, "scale=%g d=%d" % (scale, d0 + d1), x0, x1)
    if scale == 1e18 and d0 + d1 >= 3072:
        assert (y == 0).all()
    else:
        assert (y != 0).any() and np.isfinite(y).all()


@pytest.mark.parametrize("d0,d1", R.L2_SPECIAL_WIDTHS)
@pytest.mark.parametrize("special", R.L2_SPECIAL)
def test_l2norm_special_rows(avt, dev, special, d0, d1):
    """A NaN entry gives an all-NaN row, as F.normalize's clamp_min does (`nrm > eps ? nrm : eps` took the eps branch and
    scaled the finite entries by 1e12); an inf entry gives zeros and one NaN; a zero row stays zero; the other rows of the
    same workgroup are untouched."""
    x0, x1 = R.l2norm_input(5, d0, d1, special=special)
    y, hi, lo = _l2_check(avt, dev, "%s d=%d+%d" % (special, d0, d1), x0, x1)
    row, col = 2, (d0 + d1) // 3
    if special == "nan":
        assert np.isnan(y[row]).all() and np.isnan(R.bf16_value(hi[row])).all() and np.isnan(R.bf16_value(lo[row])).all()
    elif special == "inf":
        assert np.isnan(y[row, col]) and (np.delete(y[row], col) == 0).all()
    else:
        assert (y[row] == 0).all() and (hi[row] & 0x7FFF == 0).all() and (lo[row] & 0x7FFF == 0).all()
    assert np.isfinite(np.delete(y, row, axis=0)).all()


# ---------------------------------------------------------------- similarity, exact
def _sim_raw(avt, dev, mode, q, ql, t, tl, nq, nt, d, temp, pad=0):
    """One raw avt_sim_gemm_nt call into a sentinel-filled [nq + 1, nt + pad] buffer (ldo = nt + pad)."""
    P = avt.ops._p
    out = torch.full((nq + 1, nt + pad), SENT, device=dev)
    avt.ops.K.avt_sim_gemm_nt(P(q), P(ql), P(t), P(tl), nq, nt, d, float(temp), avt.ops._PREC[mode], P(out), nt + pad, avt.ops._stream())
    assert bool((out[nq] == SENT).all()) and bool((out[:, nt:] == SENT).all()), "written outside [nq, nt]"
    return out[:nq, :nt].cpu().numpy()


def _sim_xl(avt, dev, qh, ql, th, tl, nq, nt, d, temp, pad=0):
    """The 256 x 256 tile, called as ops.sim_gemm_nt calls it (so that which tile runs is not in question)."""
    P = avt.ops._p
    out = torch.full((nq + 1, nt + pad), SENT, device=dev)
    avt.ops.K.avt_gemm_nt_x3_f32out(P(qh), P(ql), d, P(th), P(tl), P(out), nt + pad, nq, nt, d, float(temp),
                                    P(avt.ops._gemm_ktab(d, d, dev)), avt.ops.X3_BF16, avt.ops._stream())
    assert bool((out[nq] == SENT).all()) and bool((out[:, nt:] == SENT).all()), "written outside [nq, nt]"
    return out[:nq, :nt].cpu().numpy()


def _expect_exact(who, out, c):
    bad = out.view(np.uint32) != c["expect"].view(np.uint32)
    print("%s: %d of %d entries differ from the exact integer / fp32(temp); sum |terms| <= %d < 2^24" % (who, int(bad.sum()), bad.size, c["bound"]))
    if bad.any():
        i, j = np.argwhere(bad)[0]
        raise AssertionError("%s: out[%d, %d] = %r, exact %r (accumulator %r)" % (who, i, j, out[i, j], c["expect"][i, j], c["acc"][i, j]))


def _run_bf16(avt, dev, c, nq, nt, d, pad=0, xl=False):
    a = [_bf(c[k], dev) for k in ("qh", "ql", "th", "tl")]
    if xl:
        return _sim_xl(avt, dev, a[0], a[1], a[2], a[3], nq, nt, d, c["temp"], pad)
    if c["mode"] == "bf16":
        a[1] = a[3] = None
    return _sim_raw(avt, dev, c["mode"], a[0], a[1], a[2], a[3], nq, nt, d, c["temp"], pad)


@pytest.mark.parametrize("nq,nt,d", R.SIM_F32_V2)
def test_sim_f32_v2_exact(avt, dev, nq, nt, d):
    """Aligned fp32 below 4 GiB: sim_f32_v2_kernel (buffer loads, 64-byte K-steps).  d = 4, 20, 2312 end inside a K-step."""
    c = R.exact_gemm("f32", nq, nt, d)
    for pad in (0, 3):  # ldo = nt and nt + 3
        _expect_exact("f32 v2 %s ldo=nt+%d" % ((nq, nt, d), pad), _sim_raw(avt, dev, "f32", _t(c["q"], dev), None, _t(c["t"], dev), None, nq, nt, d, c["temp"], pad), c)


@pytest.mark.parametrize("d", R.SIM_F32_R2_D + [64])
def test_sim_f32_round2_tile_exact(avt, dev, d):
    """d % 4 != 0, or (d = 64) a q that starts 4 bytes off a 16-byte boundary: sim_gemm_kernel<F32, unaligned>."""
    nq, nt = R.SIM_F32_R2_SHAPE
    c = R.exact_gemm("f32", nq, nt, d)
    q = _off_by_one_float(c["q"], dev) if d == 64 else _t(c["q"], dev)
    for pad in (0, 3):
        _expect_exact("f32 round-2 tile %s ldo=nt+%d" % ((nq, nt, d), pad), _sim_raw(avt, dev, "f32", q, None, _t(c["t"], dev), None, nq, nt, d, c["temp"], pad), c)


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
@pytest.mark.parametrize("d", R.SIM_BF16_D)
def test_sim_bf16_plain_tile_exact(avt, dev, mode, d):
    """d % 8 != 0 takes the element-wise loads; 63 / 64 / 65 / 72 end a 64-element K-step one short, exactly, one and eight over."""
    for nq, nt in R.SIM_BF16_SHAPES:
        c = R.exact_gemm(mode, nq, nt, d)
        _expect_exact("%s %s" % (mode, (nq, nt, d)), _run_bf16(avt, dev, c, nq, nt, d, pad=1), c)


def test_sim_bf16_plain_tile_exact_at_the_widest_embedding(avt, dev):
    nq, nt, d = R.SIM_BF16_LONG
    for mode in ("bf16", "bf16x3"):
        c = R.exact_gemm(mode, nq, nt, d)
        _expect_exact("%s %s" % (mode, (nq, nt, d)), _run_bf16(avt, dev, c, nq, nt, d), c)


@pytest.mark.parametrize("nq,nt,d", R.SIM_XL_SHAPES)
def test_sim_bf16x3_on_the_256_tile_exact(avt, dev, nq, nt, d):
    """The tile ops.sim_gemm_nt takes with SIM_XL = "always": one row, a ragged second row tile, the deepest K it accepts;
    contiguous and through a pitched `out` (ldo = nt + 4: the tile wants ldo % 4 == 0)."""
    c = R.exact_gemm("bf16x3", nq, nt, d)
    for pad in (0, 4):
        _expect_exact("bf16x3 256-tile %s ldo=nt+%d" % ((nq, nt, d), pad), _run_bf16(avt, dev, c, nq, nt, d, pad=pad, xl=True), c)
    keep, avt.ops.SIM_XL = avt.ops.SIM_XL, "always"
    try:  # ... and through the wrapper, which must choose that tile for these shapes
        a = [_bf(c[k], dev) for k in ("qh", "ql", "th", "tl")]
        out = avt.ops.sim_gemm_nt(a[0], a[2], c["temp"], "bf16x3", q_lo=a[1], t_lo=a[3]).cpu().numpy()
    finally:
        avt.ops.SIM_XL = keep
    _expect_exact("bf16x3 by ops.sim_gemm_nt %s" % ((nq, nt, d),), out, c)


NONFINITE = [("f32", (130, 129, 20), False), ("f32", (37, 130, 33), False), ("bf16", (129, 127, 65), False),
             ("bf16x3", (129, 127, 65), False), ("bf16x3", (257, 256, 256), True)]


@pytest.mark.parametrize("mode,shape,xl", NONFINITE)
def test_sim_nonfinite_poisons_its_row_or_column_only(avt, dev, mode, shape, xl):
    """One NaN in q (last row, last k) and one inf in t (last row but one, k = 0): row nq - 1 and column nt - 2 are
    non-finite (x * inf is inf or NaN for every x, zero included), every other entry is the exact value."""
    nq, nt, d = shape
    c = R.exact_gemm(mode, nq, nt, d)
    if mode == "f32":
        c["q"][nq - 1, d - 1] = np.nan
        c["t"][nt - 2, 0] = np.inf
        out = _sim_raw(avt, dev, "f32", _t(c["q"], dev), None, _t(c["t"], dev), None, nq, nt, d, c["temp"])
    else:
        c["qh"][nq - 1, d - 1] = 0x7FC0
        c["th"][nt - 2, 0] = 0x7F80
        out = _run_bf16(avt, dev, c, nq, nt, d, xl=xl)
    poisoned = np.zeros((nq, nt), bool)
    poisoned[nq - 1, :] = True
    poisoned[:, nt - 2] = True
    print("%s %s%s: %d non-finite entries, %d expected" % (mode, shape, " 256-tile" if xl else "", int((~np.isfinite(out)).sum()), int(poisoned.sum())))
    assert np.array_equal(~np.isfinite(out), poisoned)
    assert np.isnan(out[nq - 1]).all()
    assert np.array_equal(out[~poisoned].view(np.uint32), c["expect"][~poisoned].view(np.uint32))


def test_sim_f32_operand_of_4_gib_and_the_largest_below(avt, dev):
    """q of 65536 x 16384 fp32 is exactly 2^32 bytes: past the 32-bit offsets of sim_f32_v2_kernel, so the round-2 tile with
    64-bit addresses takes it (the only way to sim_gemm_kernel<F32, aligned>); 65535 rows is the largest operand v2 accepts
    (2^32 - 65536 bytes, below the 2^32 - 64 guard and its 0xFFFFFFF0 sentinel).  Integer data made on the device; the
    first, middle and last 128 rows equal the exact expectation and the same kernel run on a copy of those rows alone."""
    free = torch.cuda.mem_get_info(dev)[0]
    if free < 24 * 2 ** 30:
        pytest.skip("needs 24 GiB of free device memory, the device reports %.1f GiB" % (free / 2 ** 30))
    n, d, nt, temp = 65536, R.SIM_BIG_D, R.SIM_BIG_NT, 0.1
    assert 64 * d < R.EXACT_LIMIT  # entries in [-8, 8]: sum |terms| <= 64 d
    q = torch.empty((n, d), dtype=torch.float32, device=dev)
    q.random_(0, 17, generator=torch.Generator(device=dev).manual_seed(5)).sub_(8.0)
    t = torch.empty((nt, d), dtype=torch.float32, device=dev)
    t.random_(0, 17, generator=torch.Generator(device=dev).manual_seed(6)).sub_(8.0)
    assert q.numel() * 4 == 2 ** 32 and float(q.min()) == -8 and float(q.max()) == 8
    t64 = t.cpu().numpy().astype(np.float64)

    def expect(rows):
        acc = rows.cpu().numpy().astype(np.float64) @ t64.T
        return (acc.astype(np.float32) / np.float32(temp)).view(np.uint32)

    try:
        for rows, swapped in ((n, False), (n - 1, False), (n, True)):
            qq = q[:rows]
            assert (rows * d * 4 < 2 ** 32 - 64) == (rows < n)
            if swapped:  # the 4 GiB operand as t: out [nt, rows]
                out = _sim_raw(avt, dev, "f32", t, None, qq, None, nt, rows, d, temp).T
            else:
                out = _sim_raw(avt, dev, "f32", qq, None, t, None, rows, nt, d, temp)
            for lo in (0, (rows // 2) - 64 + 1, rows - 128):
                part = qq[lo : lo + 128].clone()
                e = expect(part)
                bad = int((out[lo : lo + 128].view(np.uint32) != e).sum())
                if swapped:
                    alone = _sim_raw(avt, dev, "f32", t, None, part, None, nt, 128, d, temp).T
                else:
                    alone = _sim_raw(avt, dev, "f32", part, None, t, None, 128, nt, d, temp)
                bad2 = int((out[lo : lo + 128].view(np.uint32) != alone.view(np.uint32)).sum())
                print("rows=%d%s slice %d: %d entries off the exact value, %d off the slice alone" % (rows, " (as t)" if swapped else "", lo, bad, bad2))
                assert bad == 0 and bad2 == 0, (rows, swapped, lo)
            del out
    finally:
        del q
        torch.cuda.empty_cache()


# ---------------------------------------------------------------- row_transition
_OUTS = ("idx", "seg", "p", "cnt", "stats")


def _rt(avt, dev, case, want=_OUTS, ld_pad=0, lda_pad=0):
    """One raw avt_row_transition call.  Outputs are sentinel-filled with a guard row; pitched inputs carry NaN between the
    rows (a kernel that read the pitch would poison its sums).  -> dict of numpy arrays (None where not asked for)."""
    P = avt.ops._p
    sim, sim_a, q_ids, cap = case["sim"], case["sim_a"], case["q_ids"], case["cap"]
    nq, nt = sim.shape

    def pitched(a, pad):
        if a is None:
            return None
        b = torch.full((nq, nt + pad), float("nan"), device=dev)
        b[:, :nt] = torch.from_numpy(a)
        return b

    s, sa, qi = pitched(sim, ld_pad), pitched(sim_a, lda_pad), _t(q_ids, dev)
    o = dict(idx=torch.full((nq + 1, cap), SENT_I, dtype=torch.int32, device=dev) if "idx" in want and cap else None,
             seg=torch.full((nq + 1, cap), SENT_I, dtype=torch.int32, device=dev) if "seg" in want and cap else None,
             p=torch.full((nq + 1, cap), SENT, device=dev) if "p" in want and cap else None,
             cnt=torch.full((nq + 1,), SENT_I, dtype=torch.int32, device=dev) if "cnt" in want else None,
             stats=torch.full((nq + 1, 4), SENT, device=dev) if "stats" in want else None)
    avt.ops.K.avt_row_transition(P(s), nq, nt, nt + ld_pad, P(qi), nt if q_ids is not None else 0, P(sa), nt + lda_pad if sim_a is not None else 0,
                                 float(case["alpha"]), float(case["threshold"]), int(cap), P(o["idx"]), P(o["seg"]), P(o["p"]), P(o["cnt"]),
                                 P(o["stats"]), avt.ops._stream())
    res = {}
    for k, v in o.items():
        if v is not None:
            v = v.cpu().numpy()
            assert (v[nq] == (SENT if v.dtype.kind == "f" else SENT_I)).all(), "the row after the last was written: " + k
            v = v[:nq]
        res[k] = v
    return res


def _oracle(case):
    return cref.row_transition(case["sim"], q_ids=case["q_ids"], sim_a=case["sim_a"], alpha=case["alpha"], threshold=case["threshold"],
                               cap=case["cap"])


def _check_vs_oracle(g, o, case):
    """idx / seg / p / cnt / row_sum / row_max bit for bit; ce and entropy within the tolerance test_gpu_kernels.py has always
    used for these reporting values (fast exp / log); every slot past min(cnt, cap) still holds its sentinel."""
    cap, who = case["cap"], case["name"]
    if g["cnt"] is not None:
        assert np.array_equal(g["cnt"], o["cnt"]), who
    for r in range(len(o["cnt"])):
        k = min(int(o["cnt"][r]), cap)
        for name in ("idx", "seg", "p"):
            if g[name] is not None:
                assert _same_bits(g[name][r, :k], o[name][r, :k]), (who, name, r)
                assert (g[name][r, k:] == (SENT if name == "p" else SENT_I)).all(), (who, name, r, "a slot past cnt was written")
    if g["stats"] is not None:
        assert _same_bits(g["stats"][:, :2], o["stats"][:, :2]), (who, g["stats"][:, :2], o["stats"][:, :2])
        np.testing.assert_allclose(g["stats"][:, 2:], o["stats"][:, 2:], rtol=5e-6, atol=2e-6, err_msg=who)


@pytest.mark.parametrize("group", ["plain", "perm", "placement", "blend", "special"])
def test_row_transition_edges(avt, dev, group):
    """plain / perm: row lengths on both sides of every width at which the launcher changes kernel (2048 / 4096 / 8192 /
    16384), as nt and, under q_ids, as L = nt - 1 (nt for the last query), for queries 0, 1, middle, nt - 2, nt - 1; the small
    rows.  placement: survivors only in the last ragged round, all inside one wave, every entry (threshold 1 and 1.5),
    exactly one, exact ties in the first and last rounds.  blend: the audio row with alpha 0, 1, 0.5.  special: one NaN,
    +inf, -inf, an all-zero row, [1, -1, 0, ...], a negative sum, in each of the five kernels: row_select_ref (the
    reference's lines in torch) decides the survivors, and row_max is NaN wherever torch's is."""
    for case in R.transition_cases(group):
        g = _rt(avt, dev, case)
        _check_vs_oracle(g, _oracle(case), case)
        R.check_select(g, case, "kernel")


def test_row_transition_exact_rows(avt, dev):
    def run(x, th, cap):
        return _rt(avt, dev, dict(sim=x, sim_a=None, q_ids=None, cap=cap, alpha=0.5, threshold=th))

    R.check_exact_rows(run)


def test_row_transition_capacity_and_optional_outputs(avt, dev):
    """cap = 1, cap = 0 with all three survivor outputs NULL (cnt and stats only), cap > L, and each survivor output alone:
    cnt is the true count whatever the cap, and nothing past min(cnt, cap) is written."""
    for case in R.transition_cases("capacity"):
        o = _oracle(case)
        full = _rt(avt, dev, case)
        if case["cap"] == 0:
            assert full["idx"] is None and full["seg"] is None and full["p"] is None
        _check_vs_oracle(full, o, case)
        R.check_select(full, case, "kernel")
        assert full["cnt"].tolist() == [1, 2, 3, 4, 5, 6, 7]  # gap_rows: row r has r + 1 survivors
        if case["cap"]:
            for alone in ("idx", "seg", "p"):
                g = _rt(avt, dev, case, want=(alone, "cnt", "stats"))
                assert [k for k in ("idx", "seg", "p") if g[k] is not None] == [alone]
                assert np.array_equal(g[alone], full[alone]) and np.array_equal(g["cnt"], full["cnt"])
                assert np.array_equal(g["stats"], full["stats"])
            g = _rt(avt, dev, case, want=("idx",))  # no cnt, no stats
            assert np.array_equal(g["idx"], full["idx"])
    print("cap 1 / 0 / 400 / 3: cnt 1..7 throughout, each of idx / seg / p alone equals the full call")


def test_row_transition_pitched_rows(avt, dev):
    """ld = nt + 5, ld_a = nt + 9 (NaN between the rows): bit for bit the contiguous call, in a 256-thread, a 1024-thread
    and the wide-row kernel, with and without q_ids."""
    cases = [c for c in R.transition_cases("blend") if "alpha=0.5" in c["name"] or "perm" in c["name"]]
    cases += [c for c in R.transition_cases("plain") if c["name"] in ("plain L=257", "plain L=8193", "plain L=16385")]
    for case in cases:
        a, b = _rt(avt, dev, case), _rt(avt, dev, case, ld_pad=5, lda_pad=9)
        for k in _OUTS:
            assert np.array_equal(a[k], b[k]), (case["name"], k)
        assert np.isfinite(b["stats"]).all()
    print("pitched == contiguous for", [c["name"] for c in cases])


# ---------------------------------------------------------------- row_topk
def _topk(avt, dev, x, k, self_col, ld_pad=0):
    """One raw avt_row_topk call; a pitched input carries 1e30 between the rows (it would be picked if it were read)."""
    P = avt.ops._p
    nq, nt = x.shape
    s = torch.full((nq, nt + ld_pad), 1e30, device=dev)
    s[:, :nt] = torch.from_numpy(x)
    idx = torch.full((nq + 1, k), SENT_I, dtype=torch.int32, device=dev)
    val = torch.full((nq + 1, k), SENT, device=dev)
    avt.ops.K.avt_row_topk(P(s), nq, nt, nt + ld_pad, P(_t(self_col, dev)), int(k), P(idx), P(val), avt.ops._stream())
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    assert (idx[nq] == SENT_I).all() and (val[nq] == SENT).all()
    return idx[:nq], val[:nq]


@pytest.mark.parametrize("nt", R.TOPK_WIDTHS)
def test_row_topk_edges(avt, dev, nt):
    """Both register forms on both sides of 4096, the widest row; k = 1, k = nt, k = nt + 3 (with a self column the tail is
    -1 / -inf); ties across lanes, waves and rounds, and a row that is one tie; self_col at 0 and nt - 1; a row of -inf (k
    distinct picks); NaNs at column 0, the middle and the last, and a row of NaN: never picked.  Pitched rows too."""
    x, self_col = R.topk_input(nt)
    for k in sorted({1, min(nt, 40), nt, nt + 3}):
        for sc, pad in ((self_col, 0), (None, 0), (self_col, 5)):
            if sc is None and k > 40:
                continue
            gi, gv = _topk(avt, dev, x, k, sc, pad)
            ri, rv = R.topk_ref(x, k, sc)
            assert np.array_equal(gi, ri), (nt, k, pad)
            assert np.array_equal(gv, rv), (nt, k, pad)
            if pad == 0:
                oi, ov = cref.row_topk(x, k, sc)
                assert np.array_equal(gi, oi) and np.array_equal(gv, ov), (nt, k)
        print("nt=%d k=%d: equal to topk_ref and the oracle; row of NaN -> %s" % (nt, k, gi[4, : min(k, 3)].tolist()))
    assert (gi[4] == -1).all() and np.isinf(gv[4]).all()


def test_row_topk_refuses_rows_wider_than_16384(avt, dev):
    x = torch.zeros((1, 16385), device=dev)
    with pytest.raises(avt._lib.AvtError, match=r"\(-2\)"):  # AVT_ERR_UNSUPPORTED
        avt.ops.row_topk(x, 4)
    i, v = avt.ops.row_topk(x[:, :16384].contiguous(), 4)  # the widest row it takes
    assert i.tolist() == [[0, 1, 2, 3]] and v.tolist() == [[0.0] * 4]
