"""tests/bn_train_refs.py on the CPU: the fp64 references against torch's float64 BatchNorm3d through autograd; the bounds of
its report() against a numpy model of csrc/bn_train.hip's own arithmetic — inside every bound as the kernel is written, outside
at least one with any single listed mistake switched in — and the producer-row builder against its own unpacking.  What the
device test (tests/test_gpu_bn_train_edges.py) then fails on is the kernel, not its yardstick."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_train_refs as R


def _torch64(x, res, gamma, beta, eps, relu, groups, dy):
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    rt = None if res is None else torch.from_numpy(res.astype(np.float64)).requires_grad_(True)
    w = torch.from_numpy(gamma.astype(np.float64)).requires_grad_(True)
    b = torch.from_numpy(beta.astype(np.float64)).requires_grad_(True)
    M, C = x.shape[0] // groups, x.shape[1]
    ys, means, vars_ = [], [], []
    for g in range(groups):
        rm, rv = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
        xg = xt[g * M:(g + 1) * M].t().reshape(1, C, M, 1, 1)
        # (momentum 1: the running statistics leave as the batch's own — mean and UNBIASED variance — with nothing to subtract)
        y = F.batch_norm(xg, rm, rv, w, b, True, 1.0, float(np.float64(np.float32(eps)))).reshape(C, M).t()
        means.append(rm)
        vars_.append(rv)
        ys.append(y)
    y = torch.cat(ys, 0)
    if rt is not None:
        y = y + rt
    if relu:
        y = F.relu(y)
    y.backward(torch.from_numpy(dy.astype(np.float64)))
    return (y.detach().numpy(), torch.stack(means).numpy(), torch.stack(vars_).numpy(), xt.grad.numpy(), None if rt is None else rt.grad.numpy(),
            w.grad.numpy(), b.grad.numpy())


@pytest.mark.parametrize("fam,m,c,groups,res,relu", [
    ("plain", 5, 8, 1, False, True), ("plain", 129, 8, 3, True, True), ("offset", 33, 64, 2, True, False),
    ("degenerate", 40, 16, 9, False, True), ("integer", 12, 32, 17, True, True), ("plain", 7, 2048, 2, False, False),
])
def test_references_equal_torch_float64(fam, m, c, groups, res, relu):
    x, gamma, beta = R.family(fam, m, c, groups)
    r, dy, _, _ = R.aux(fam, m, c, groups)
    r = r if res else None
    eps = R.EPS[fam]
    y, mean, unb, dx, dres, dgamma, dbeta = _torch64(x, r, gamma, beta, eps, relu, groups, dy)
    f = R.fwd_ref(x, r, gamma, beta, eps, relu, groups)
    # (the mask is an INPUT of bwd_ref: torch's own here — where a pre-activation is 0 in exact arithmetic, two fp64 evaluations
    #  need not agree on the sign of what is left)
    b = R.bwd_ref(dy, x, (y > 0) if relu else None, gamma, f["mean"], f["invstd"], groups)

    def close(a, e, what):
        scale = np.abs(e).max() + 1e-300
        assert np.abs(a - e).max() <= 1e-12 * scale, (what, np.abs(a - e).max() / scale)

    close(f["y"], y, "y")
    close(f["mean"], mean, "mean")
    close(f["var"] * m / (m - 1), unb, "var")
    close(b["dx"], dx, "dx")
    close(b["dgamma"], dgamma, "dgamma")
    close(b["dbeta"], dbeta, "dbeta")
    if res:
        close(b["dres"], dres, "dres")


def _report(fam, m, c, groups, res, relu, fault=None):
    x, gamma, beta = R.family(fam, m, c, groups)
    r, dy, rm, rv = R.aux(fam, m, c, groups)
    r = r if res else None
    out = R.kernel_model(x, r, gamma, beta, R.EPS[fam], relu, groups, R.MOMENTUM, rm, rv, dy, fault)
    out["save_mean"], out["save_invstd"] = out["save_mean"].reshape(-1), out["save_invstd"].reshape(-1)  # [groups * C], as the entry writes them
    k = R.chain_depth(m * groups, c, groups, R.layout_blocks(m * groups, c, groups))
    return R.report(out, x, r, gamma, beta, R.EPS[fam], relu, groups, R.MOMENTUM, rm, rv, dy, k)


_GROUPED = [(fam, R.GROUP_ROWS, c, g, True, True) for fam in ("integer",) for c in (32, 2048) for g in R.GROUP_COUNTS] + \
           [("offset", m, c, g, True, True) for (m, c, g) in R.GROUP_OFFSET_CASES]


@pytest.mark.parametrize("fam", ["plain", "offset", "integer", "degenerate"])
def test_the_kernels_arithmetic_stays_inside_every_bound(fam):
    """kernel_model(fault=None) — bn_train.hip's operations in float32, its fp64 sums in another order — on EVERY case of the
    device test of this family: the references and the bounds alone fail nothing."""
    cases = [c for c in R.fp64_cases() + _GROUPED if c[0] == fam]
    cases += [(fam, m, c, g, True, True) for (m, c, g) in ((1, 8, 4), (5, 8, 1), (129, 8, 2), (3, 1024, 1), (12, 2048, 9))]
    assert len(cases) >= 5
    worst = {}
    for case in cases:
        for n, v in _report(*case).items():
            worst[n] = max(worst.get(n, 0.0), v)
            assert v <= 1.0, (case, n, v)
    print(fam, {n: round(v, 3) for n, v in worst.items()})


@pytest.mark.parametrize("fault,case,outputs", [
    # x * sc + (beta - mean * sc): 1500 u of y on the OFFSET family, seen by y_apply alone (the bound against pure fp64 has to
    # allow save_mean's own rounding, which is of the same size: see bn_train_refs)
    ("folded", ("offset", 129, 8, 1, True, True), {"y_apply"}),
    ("fp32_sums", ("offset", 129, 8, 1, True, True), {"save_mean", "save_invstd", "y"}),
    ("biased_running_var", ("plain", 129, 8, 1, True, True), {"running_var"}),
    ("wrong_group_running", ("plain", R.GROUP_ROWS, 32, 9, True, True), {"running_mean", "running_var"}),
    # pre-activations of exactly 0 exist on the DEGENERATE family without a shortcut only
    ("mask_ge", ("degenerate", 129, 8, 1, False, True), {"dres", "dx", "dbeta"}),
    # var = 0 exactly in the constant channels of the DEGENERATE family: invstd = 1 / sqrt(eps), and its eps is chosen to show
    ("eps_double", ("degenerate", 129, 8, 1, True, True), {"save_invstd"}),
])
def test_each_single_mistake_breaks_a_bound(fault, case, outputs):
    rep = _report(*case, fault=fault)
    broken = {n for n, v in rep.items() if v > 1.0}
    assert outputs <= broken, (fault, case, rep)
    clean = _report(*case)
    assert all(v <= 1.0 for v in clean.values()), clean


def test_every_fault_is_listed():
    (mark,) = [m for m in test_each_single_mistake_breaks_a_bound.pytestmark if m.name == "parametrize"]
    assert {row[0] for row in mark.args[1]} == set(R.FAULTS)


def test_offset_family_keeps_the_cancellation_term_below_a_tenth_of_u():
    """The single-pass variance's term 1/2 k 2^-53 E[x^2] / (var + eps) on every offset-family case of the device test: the
    family is there for the apply pass's |mean| / std, not to sit on the variance's limit."""
    seen = 0
    for (fam, m, c, g, res, relu) in R.fp64_cases() + _GROUPED:
        if fam != "offset" or (res, relu) != (True, True) or m == 1:
            continue  # (one row: E[x^2] - mean^2 is x^2 - x^2, exactly 0 in fp64 — the term bounds an error that is not there)
        x, gamma, beta = R.family(fam, m, c, g)
        ref = R.fwd_ref(x, None, gamma, beta, R.EPS[fam], False, g)
        k = R.chain_depth(m * g, c, g, R.layout_blocks(m * g, c, g))
        assert R.invstd_slack(ref, R.EPS[fam], k).max() < R.U / 10, (m, c, g, k)
        if m > 1:
            assert (np.abs(ref["mean"]) * ref["invstd"]).min() >= 1000  # |mean| / std: what the folded form loses, in u
        seen += 1
    assert seen >= 10


def test_degenerate_eps_shows_its_rounding():
    eps = R.EPS["degenerate"]
    right = 1.0 / np.sqrt(np.float64(np.float32(eps)))
    wrong = np.float64(np.float32(1.0 / np.sqrt(np.float64(eps))))
    assert abs(wrong - right) > R.U * right and abs(np.float64(np.float32(right)) - right) <= R.U * right


def test_degenerate_family_has_what_it_is_for():
    x, gamma, beta = R.family("degenerate", 129, 16, 2)
    f = R.fwd_ref(x, None, gamma, beta, R.EPS["degenerate"], False, 2)
    assert np.all(f["var"][:, [0, 1, 8, 9]] == 0.0)                                  # constant channels, at g and 3 + g
    assert np.all(f["mean"][:, [2, 3]] == np.arange(2)[:, None])                    # symmetric channels: the mean is exact
    assert np.all(f["y"][:129, 0] == 0.0) and (f["y"][:, [2, 3]] == 0.0).sum() > 50  # pre-activations of exactly 0
    assert 0 < np.abs(f["y"][:, [2, 3]])[f["y"][:, [2, 3]] != 0].min() < 1e-4        # ... and tiny ones
    assert np.all((x[:129, 4] != 0).sum() == 1)                                     # one non-zero row


@pytest.mark.parametrize("c,unit", [(8, 1), (128, 1), (1024, 1), (2048, 2), (4096, 4)])
@pytest.mark.parametrize("per", [1, 2, 65, 129])
def test_partial_rows_round_trip(c, unit, per):
    rng = np.random.default_rng(c + per)
    groups = 3
    s0 = rng.integers(-5000, 5000, size=(groups, c)).astype(np.float64)
    s1 = rng.integers(0, 90000, size=(groups, c)).astype(np.float64)
    rows = R.partial_rows(s0, s1, c, per * unit, rng)
    nq, un = R.nq_unit(c)
    assert un == unit and rows.shape == (groups, per * unit, nq * 8) and np.all(rows == np.rint(rows))
    b0, b1 = R.unpack_partial_rows(rows, c)
    assert np.array_equal(b0, s0) and np.array_equal(b1, s1)
    # the layout, slot by slot, as channel_sums reads it: channel ch -> quad ch / 4, rows first = quad / 256, first + unit, ...
    for ch in (0, 5, c // 2 + 3, c - 1):
        quad, e = ch // 4, ch % 4
        slot, first = (quad % nq) * 8 + e, (quad // 256 if unit > 1 else 0)
        assert rows[1, first::unit, slot].sum() == s0[1, ch] and rows[1, first::unit, slot + 4].sum() == s1[1, ch]
    if per > 1:
        assert len(np.unique(rows[0, ::unit, 0])) > 1  # really split


def test_pack_mask_is_the_apply_pass_layout():
    rng = np.random.default_rng(0)
    y = rng.standard_normal((5, 16)).astype(np.float32)
    got = R.pack_mask(y, 16)
    for i in range(5 * 4):
        row, quad = divmod(i, 4)
        assert got[i] == sum(1 << e for e in range(4) if y[row, 4 * quad + e] > 0)


def test_layout_mirror_equals_the_library():
    """layout_blocks (used here for the chain depth) is bn_train.hip's layout(): equal to what avt_bn_train_ws_bytes implies on
    every shape of the device test, and each shape still has the workgroup and sweep count it was chosen for."""
    for (m, c, g, why, blocks, sw) in R.SHAPES + R.SWEEPS:
        assert R.layout_blocks(m * g, c, g) == R.blocks_of(m * g, c, g) == blocks, (m, c, g, why)
        assert R.sweeps(m * g, c, g, blocks) == sw, (m, c, g, why)
    for c in (32, 2048):
        for g in R.GROUP_COUNTS:
            assert R.layout_blocks(R.GROUP_ROWS * g, c, g) == R.blocks_of(R.GROUP_ROWS * g, c, g)
