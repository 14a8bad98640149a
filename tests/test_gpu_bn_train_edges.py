"""The seven kernels of csrc/bn_train.hip behind their six entries (avt_bn_train_ws_bytes / _ws_bytes_pre / _fwd / _fwd_pre /
_bwd / _bwd_pre) against fp64 and at their edges — the fused train-mode BatchNorm + shortcut + ReLU of the SlowFast blocks the
reference trains (contrastive_video_textures/train.py:114-141, models/models.py:385-417).  References, magnitudes, bounds and input
families: tests/bn_train_refs.py, proved on the CPU by tests/test_bn_train_refs_host.py (the kernel's arithmetic as written stays
inside every bound; each of six single mistakes leaves one).  The entries are called directly (ops.K / ops._p): train_ops never
passes y, never more than its own workspace, and reaches the *_pre entries only behind a convolution."""
import math

import numpy as np
import pytest
import torch

import bn_train_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x7FC5A5A5  # the bits of a quiet NaN with a payload nobody computes


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _n(t):
    return None if t is None else t.cpu().numpy()


def _ws(m, c, groups):
    from avtex import _lib
    n = int(_lib.lib().avt_bn_train_ws_bytes(m, c, groups))
    assert n > 0
    return torch.empty(n, dtype=torch.uint8, device=DEV)


def _fwd(x, res, gamma, beta, eps, relu, groups, rm=None, rv=None, tracked=None, want_mask=False, y=None, ldy=0, momentum=R.MOMENTUM,
         pre=None):
    """avt_bn_train_fwd (pre = (workspace, pre_rows): avt_bn_train_fwd_pre) on device tensors -> dict of device tensors.  rm / rv /
    tracked are updated in place.  y: where to write (a channel slice of wider rows with ldy), else a new [m, c]."""
    from avtex import ops
    m, c = x.shape
    out = {"save_mean": torch.empty(groups * c, device=DEV), "save_invstd": torch.empty(groups * c, device=DEV),
           "y": torch.empty(m, c, device=DEV) if y is None else y,
           "mask": torch.zeros(m * c // 4, dtype=torch.uint8, device=DEV) if want_mask else None}
    p = ops._p
    head = (p(x), p(res), p(out["y"]), m, c, p(gamma), p(beta), float(eps), float(momentum), 1 if relu else 0, groups)
    tail = (p(out["save_mean"]), p(out["save_invstd"]), p(rm), p(rv), p(tracked), p(out["mask"]), ldy)
    if pre is None:
        ws = _ws(m, c, groups)
        ops.K.avt_bn_train_fwd(*head, p(ws), ws.numel(), *tail, ops._stream())
    else:
        ops.K.avt_bn_train_fwd_pre(*head, p(pre[0]), pre[0].numel(), *tail, int(pre[1]), ops._stream())
    return out


def _bwd(dy, y, x, gamma, beta, f, relu, groups, mask=None, want_dres=False, ld_dy=0):
    """avt_bn_train_bwd with the forward's saved statistics f -> dict of device tensors (dres None unless asked for)."""
    from avtex import ops
    m, c = x.shape
    out = {"dx": torch.empty(m, c, device=DEV), "dres": torch.empty(m, c, device=DEV) if want_dres else None,
           "dgamma": torch.empty(c, device=DEV), "dbeta": torch.empty(c, device=DEV)}
    ws = _ws(m, c, groups)
    p = ops._p
    ops.K.avt_bn_train_bwd(p(dy), p(y), p(x), m, c, p(gamma), p(beta), p(f["save_mean"]), p(f["save_invstd"]), 1 if relu else 0, groups,
                           p(mask), p(ws), ws.numel(), p(out["dx"]), p(out["dres"]), p(out["dgamma"]), p(out["dbeta"]), ld_dy, ops._stream())
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _inputs(fam, m, c, groups):
    x, gamma, beta = R.family(fam, m, c, groups)
    res, dy, rm, rv = R.aux(fam, m, c, groups)
    return {"x": x, "gamma": gamma, "beta": beta, "res": res, "dy": dy, "rm": rm, "rv": rv}


def _run(h, eps, res, relu, groups):
    """Forward (running statistics and all) and backward of host inputs h on the device -> fp32 numpy outputs, report()'s names."""
    d = {k: _t(v) for k, v in h.items()}
    tracked = torch.zeros(1, dtype=torch.int64, device=DEV)
    r = d["res"] if res else None
    keep_mask = relu and res
    f = _fwd(d["x"], r, d["gamma"], d["beta"], eps, relu, groups, d["rm"], d["rv"], tracked, want_mask=keep_mask)
    b = _bwd(d["dy"], None, d["x"], d["gamma"], d["beta"], f, relu, groups, mask=f["mask"], want_dres=res)  # (train_ops' two forms)
    torch.cuda.synchronize()
    out = {n: _n(f[n]) for n in ("save_mean", "save_invstd", "y")}
    out.update(running_mean=_n(d["rm"]), running_var=_n(d["rv"]), tracked=int(tracked.item()))
    out.update({n: _n(b[n]) for n in ("dx", "dres", "dgamma", "dbeta") if b[n] is not None})
    return out


def _hold(what, rep):
    """Print the achieved error / bound of every output, then hold each to 1."""
    print("RATIO %s %s" % (what, " ".join("%s=%.3g" % kv for kv in rep.items())))
    for n, v in rep.items():
        assert v <= 1.0, (what, n, v)


def _edge(m, c, groups):
    for (mm, cc, gg, why, blocks, sw) in R.SHAPES + R.SWEEPS:
        if (mm, cc, gg) == (m, c, groups):
            return why, blocks, sw
    raise KeyError((m, c, groups))


@pytest.mark.parametrize("fam,m,c,groups,res,relu", R.fp64_cases())
def test_forward_and_backward_against_fp64(fam, m, c, groups, res, relu):
    """avt_bn_train_fwd + avt_bn_train_bwd: save_mean, save_invstd, y, both running statistics, num_batches_tracked, dx, dres,
    dgamma, dbeta against fp64 within the derived bounds of bn_train_refs.report() — plain, offset (|mean| / std >= 1200) and
    degenerate inputs (constant channels, pre-activations of exactly 0, a single non-zero row), with and without shortcut and
    ReLU, at layout()'s edges: C = 8 with 1 / 5 / 127 / 128 / 129 rows (fewer chunks than threads; one workgroup; the halving tree
    down to nq = 2), C = 1024 (nq = 256: no tree), C = 2048 / 4096 past 64 workgroups (unit 2 and 4, a second trip of the
    finalize lanes, first = quad / 256); and at ONE, TWO and THREE sweeps of the statistics walk (16 groups of 128 workgroups:
    16384 rows exactly one sweep, 32768 two — the paired loop alone —, 32769 two and two chunks, 49152 three — pair and tail in
    every thread; one group of 262145 rows on 1024 workgroups).  Each shape still has the workgroup and sweep count it is here for."""
    why, blocks, sw = _edge(m, c, groups)
    assert R.blocks_of(m * groups, c, groups) == blocks and R.sweeps(m * groups, c, groups, blocks) == sw, why
    h = _inputs(fam, m, c, groups)
    eps = R.EPS[fam]
    out = _run(h, eps, res, relu, groups)
    assert out.pop("tracked") == 1
    assert all(np.all(np.isfinite(v)) for v in out.values())
    k = R.chain_depth(m * groups, c, groups, blocks)
    rep = R.report(out, h["x"], h["res"] if res else None, h["gamma"], h["beta"], eps, relu, groups, R.MOMENTUM, h["rm"], h["rv"], h["dy"], k)
    assert ("dres" in rep) == res and len(rep) == (10 if res else 9)
    _hold("fp64 %s m%d c%d g%d res%d relu%d" % (fam, m, c, groups, res, relu), rep)


def _exact_dgamma(g, x, mean32, invstd32, groups):
    """float32 of the EXACT sum of the products the statistics pass forms, (double)g * float((x - mu) * is): with integer g they
    span far less than 53 bits, so no order of fp64 additions rounds."""
    G, M, C = groups, x.shape[0] // groups, x.shape[1]
    t = ((x.reshape(G, M, C) - mean32.reshape(G, 1, C)) * invstd32.reshape(G, 1, C)).astype(np.float64) * g.reshape(G, M, C)
    t = t.transpose(2, 0, 1).reshape(C, G * M)
    return np.array([math.fsum(row) for row in t], np.float64).astype(np.float32)


@pytest.mark.parametrize("c", [32, 2048])
@pytest.mark.parametrize("groups", R.GROUP_COUNTS)
def test_group_batches_equal_a_loop_of_single_group_calls(groups, c):
    """More groups than one trip of channel_sums (kGroupBatch = 8): 1, 7, 8 groups in one trip, 9 = a second trip of one group,
    16 = two full trips, 17 = a ragged third; C = 32 and C = 2048 (unit 2).  Integer inputs: every fp64 sum is exact, so ONE launch
    equals a loop of single-group launches bit for bit (save_mean, save_invstd, y, dx, dres), dbeta is float32 of the integer
    total over all groups and dgamma of the exact sum of the kernel's own products; the running statistics are running_ref of
    GROUP 0 (g0 > 0 trips must not touch them) bit for bit, and num_batches_tracked is 3 after three calls whatever the count."""
    m = R.GROUP_ROWS
    h = _inputs("integer", m, c, groups)
    d = {k: _t(v) for k, v in h.items()}
    eps = R.EPS["integer"]
    tracked = torch.zeros(1, dtype=torch.int64, device=DEV)
    f = _fwd(d["x"], d["res"], d["gamma"], d["beta"], eps, True, groups, d["rm"], d["rv"], tracked, want_mask=True)
    b = _bwd(d["dy"], None, d["x"], d["gamma"], d["beta"], f, True, groups, mask=f["mask"], want_dres=True)
    rm1, rv1 = d["rm"].clone(), d["rv"].clone()
    for _ in range(2):
        _fwd(d["x"], d["res"], d["gamma"], d["beta"], eps, True, groups, d["rm"], d["rv"], tracked)
    assert int(tracked.item()) == 3
    for g in range(groups):
        s = slice(g * m, (g + 1) * m)
        f1 = _fwd(d["x"][s], d["res"][s], d["gamma"], d["beta"], eps, True, 1, want_mask=True)
        b1 = _bwd(d["dy"][s], None, d["x"][s], d["gamma"], d["beta"], f1, True, 1, mask=f1["mask"], want_dres=True)
        cs = slice(g * c, (g + 1) * c)
        assert _same(f["save_mean"][cs], f1["save_mean"]) and _same(f["save_invstd"][cs], f1["save_invstd"]), g
        assert _same(f["y"][s], f1["y"]) and _same(b["dx"][s], b1["dx"]) and _same(b["dres"][s], b1["dres"]), g
        assert torch.equal(f["mask"][g * m * c // 4:(g + 1) * m * c // 4], f1["mask"]), g
    ref = R.fwd_ref(h["x"], h["res"], h["gamma"], h["beta"], eps, True, groups)
    mean32 = _n(f["save_mean"]).reshape(groups, c)
    assert np.array_equal(mean32, ref["mean"].astype(np.float32))  # exact sums: the correctly rounded mean
    em, ev = R.running_ref(h["rm"], h["rv"], mean32, ref["var"], m, R.MOMENTUM)
    assert np.array_equal(_n(rm1), em) and np.array_equal(_n(rv1), ev)
    gm = np.where(_n(f["y"]) > 0, h["dy"], np.float32(0))
    assert np.array_equal(_n(b["dres"]), gm)
    assert np.array_equal(_n(b["dbeta"]), gm.astype(np.float64).sum(axis=0).astype(np.float32))
    assert np.array_equal(_n(b["dgamma"]), _exact_dgamma(gm, h["x"], mean32, _n(f["save_invstd"]), groups))


@pytest.mark.parametrize("m,c,groups", R.GROUP_OFFSET_CASES)
def test_second_group_batch_against_fp64(m, c, groups):
    """9 groups of the offset family: the group of the SECOND trip of channel_sums (g0 = 8) has the right numbers against fp64,
    not merely the numbers of our own loop; C = 32 and C = 2048 (unit 2)."""
    h = _inputs("offset", m, c, groups)
    eps = R.EPS["offset"]
    out = _run(h, eps, True, True, groups)
    assert out.pop("tracked") == 1
    blocks = R.blocks_of(m * groups, c, groups)
    k = R.chain_depth(m * groups, c, groups, blocks)
    rep = R.report(out, h["x"], h["res"], h["gamma"], h["beta"], eps, True, groups, R.MOMENTUM, h["rm"], h["rv"], h["dy"], k)
    _hold("fp64 offset m%d c%d g%d groups" % (m, c, groups), rep)
    last = {n: (out[n].reshape(groups, -1)[-1:] if n in ("save_mean", "save_invstd") else out[n][-m:]) for n in ("save_mean", "save_invstd", "y")}
    s = slice(-m, None)
    rep9 = R.report(last, h["x"][s], h["res"][s], h["gamma"], h["beta"], eps, True, 1, R.MOMENTUM, None, None, None, k)
    _hold("fp64 offset m%d c%d last group alone" % (m, c), rep9)


def test_train_ops_counts_one_batch_per_call_whatever_the_groups():
    """train_ops.bn_act inside bn_replicas(9): num_batches_tracked is 3 after three calls and the running statistics are three
    momentum steps of GROUP 0's statistics (the DataParallel rule: replica 0's buffers are the ones kept) — what include/avt.h
    says of avt_bn_train_fwd's num_batches_tracked."""
    from avtex import train_ops
    groups, c, m = 9, 32, R.GROUP_ROWS
    h = _inputs("integer", m, c, groups)
    bn = torch.nn.BatchNorm3d(c, eps=R.EPS["integer"], momentum=R.MOMENTUM).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(_t(h["gamma"])); bn.bias.copy_(_t(h["beta"]))
        bn.running_mean.copy_(_t(h["rm"])); bn.running_var.copy_(_t(h["rv"]))
    x = _t(h["x"]).view(groups, 1, 3, 4, c).permute(0, 4, 1, 2, 3)
    assert train_ops.fusable(x, bn)
    before = train_ops.CALLS["bn_fwd"]
    with train_ops.bn_replicas(groups), torch.no_grad():
        for _ in range(3):
            train_ops.bn_act(x, bn, relu=True)
    assert train_ops.CALLS["bn_fwd"] == before + 3 and int(bn.num_batches_tracked) == 3
    ref = R.fwd_ref(h["x"], None, h["gamma"], h["beta"], R.EPS["integer"], True, groups)
    em, ev = h["rm"], h["rv"]
    for _ in range(3):
        em, ev = R.running_ref(em, ev, ref["mean"].astype(np.float32), ref["var"], m, R.MOMENTUM)
    assert np.array_equal(_n(bn.running_mean), em) and np.array_equal(_n(bn.running_var), ev)


@pytest.mark.parametrize("fam,m,c,groups", [("degenerate", 129, 8, 1), ("offset", 129, 8, 1), ("degenerate", 40, 2048, 3), ("offset", 33, 64, 9)])
def test_three_mask_forms_agree(fam, m, c, groups):
    """The ReLU mask from the saved bits, from the forward output y (a branch train_ops never takes) and recomputed from x and
    beta: bit-identical dx, dgamma, dbeta where they must agree — pre-activations of exactly 0 and of +-tiny (degenerate family)
    and |mean| / std = 1500 (offset), without a shortcut.  The mask bytes themselves are the packed bits of y > 0 (bit e of byte i:
    channel 4 (i % (C/4)) + e of chunk i).  With a shortcut the mask and the y form are bit-identical, dres included; with a
    shortcut and neither, the entry refuses before it launches anything."""
    from avtex import _lib, ops
    h = _inputs(fam, m, c, groups)
    d = {k: _t(v) for k, v in h.items()}
    eps = R.EPS[fam]
    f = _fwd(d["x"], None, d["gamma"], d["beta"], eps, True, groups, want_mask=True)
    y = _n(f["y"])
    assert np.array_equal(_n(f["mask"]), R.pack_mask(y, c))
    if fam == "degenerate":
        assert (y == 0).any() and np.all(y[:m, 0] == 0)  # a channel of pre-activations of exactly 0: nothing passes
        assert not np.any(_n(f["mask"]).reshape(-1, c // 4)[:m, 0] & 1)
    forms = [_bwd(d["dy"], None, d["x"], d["gamma"], d["beta"], f, True, groups, mask=f["mask"]),
             _bwd(d["dy"], f["y"], d["x"], d["gamma"], d["beta"], f, True, groups),
             _bwd(d["dy"], None, d["x"], d["gamma"], d["beta"], f, True, groups)]
    for other, name in zip(forms[1:], ("y", "recomputed")):
        for n in ("dx", "dgamma", "dbeta"):
            assert _same(forms[0][n], other[n]), (name, n)
    fr = _fwd(d["x"], d["res"], d["gamma"], d["beta"], eps, True, groups, want_mask=True)
    assert np.array_equal(_n(fr["mask"]), R.pack_mask(_n(fr["y"]), c))
    a = _bwd(d["dy"], None, d["x"], d["gamma"], d["beta"], fr, True, groups, mask=fr["mask"], want_dres=True)
    b = _bwd(d["dy"], fr["y"], d["x"], d["gamma"], d["beta"], fr, True, groups, want_dres=True)
    for n in ("dx", "dres", "dgamma", "dbeta"):
        assert _same(a[n], b[n]), n
    assert np.array_equal(_n(a["dres"]), np.where(_n(fr["y"]) > 0, h["dy"], np.float32(0)))
    # a shortcut, no mask, no y: refused (the unchecked binding: the status itself, and the reason on record)
    ws = _ws(m * groups, c, groups)
    p = ops._p
    rc = _lib.lib().avt_bn_train_bwd(p(d["dy"]), None, p(d["x"]), m * groups, c, p(d["gamma"]), p(d["beta"]), p(fr["save_mean"]),
                                     p(fr["save_invstd"]), 1, groups, None, p(ws), ws.numel(), p(a["dx"]), p(a["dres"]), p(a["dgamma"]),
                                     p(a["dbeta"]), 0, ops._stream())
    assert rc != 0 and b"ReLU needs the forward's mask" in _lib.lib().avt_last_error()


@pytest.mark.parametrize("c,e", [(8, 4), (2048, 64)])
@pytest.mark.parametrize("c_off", [0, 1])
def test_strided_slices(c, e, c_off):
    """ldy / ld_dy: the forward writes a channel slice of rows of C + e floats (at the head, and at channel offset e) that were
    pre-filled with a sentinel — the slice is bit-identical to the contiguous call's y and every float outside it keeps its bits;
    the backward reads such a slice of a wider gradient whose other columns are NaN — dx, dgamma, dbeta bit-identical to the
    contiguous call.  C = 8 and C = 2048 (unit 2: the strided walk of a row wider than a workgroup)."""
    m, groups = 37, 3
    off = c_off * e
    h = _inputs("plain", m, c, groups)
    d = {k: _t(v) for k, v in h.items()}
    eps = R.EPS["plain"]
    f0 = _fwd(d["x"], d["res"], d["gamma"], d["beta"], eps, True, groups, want_mask=True)
    b0 = _bwd(d["dy"], None, d["x"], d["gamma"], d["beta"], f0, True, groups, mask=f0["mask"], want_dres=True)
    ld = c + e
    wide = torch.full((m * groups, ld), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    f1 = _fwd(d["x"], d["res"], d["gamma"], d["beta"], eps, True, groups, want_mask=True, y=wide[:, off:], ldy=ld)
    got = _bits(wide)
    assert torch.equal(got[:, off:off + c], _bits(f0["y"]))
    outside = torch.cat([got[:, :off], got[:, off + c:]], 1)
    assert outside.numel() == m * groups * e and bool((outside == SENTINEL).all())
    assert torch.equal(f1["mask"], f0["mask"]) and _same(f1["save_mean"], f0["save_mean"]) and _same(f1["save_invstd"], f0["save_invstd"])
    gwide = torch.full((m * groups, ld), float("nan"), device=DEV)
    gwide[:, off:off + c] = d["dy"]
    b1 = _bwd(gwide[:, off:], None, d["x"], d["gamma"], d["beta"], f0, True, groups, mask=f0["mask"], want_dres=True, ld_dy=ld)
    for n in ("dx", "dres", "dgamma", "dbeta"):
        assert _same(b0[n], b1[n]), n
    assert bool(torch.isfinite(b1["dx"]).all())


PRE_PER = (1, 2, 63, 64, 65, 128, 129, 191, 192, 193, 300)  # pre_rows / unit


@pytest.mark.parametrize("groups", [1, 3, 9])
@pytest.mark.parametrize("c", [8, 32, 128, 2048, 4096])
def test_pre_entries_on_synthetic_partials(c, groups):
    """avt_bn_train_fwd_pre / avt_bn_train_bwd_pre / avt_bn_train_ws_bytes_pre, bn_pre_reduce_kernel and the finalize kernels'
    walk over a PRODUCER's rows, on integer totals split at random over pre_rows / unit = 1, 2, 63, 64, 65, 128 (the last count
    without pre-reduction), 129 (the first with it: chunks of 64, 64 and 1), 191, 192, 193 and 300 rows.  C = 8: rows of 16
    doubles, 16 row slices per workgroup, the tail walk only; C = 32: 4 slices, one 16-deep unrolled trip per full chunk; C = 128:
    one slice, four unrolled trips, unrolled + tail on a ragged chunk; C = 2048: unit 2, grid.z = 8; C = 4096: unit 4.  Groups 1,
    3 and 9 (a second trip of channel_sums over producer rows).  Every split gives the SAME bits — forward: those of plain
    avt_bn_train_fwd on the same x, with save_mean = float32(S0 / M); backward: dbeta / dgamma = float32 of the integer totals, dx
    within bwd_ref's bound for k0 = S0 / M, k1 = S1 / M.  The size query refuses pre_rows that are no multiple of unit, and the
    entries a workspace one byte short."""
    from avtex import _lib, ops
    lib, p = _lib.lib(), ops._p
    m = 24 if c <= 128 else 6
    nq, unit = R.nq_unit(c)
    h = _inputs("integer", m, c, groups)
    d = {k: _t(v) for k, v in h.items()}
    eps = R.EPS["integer"]
    x3 = h["x"].astype(np.float64).reshape(groups, m, c)
    S0, S1 = x3.sum(axis=1), (x3 * x3).sum(axis=1)
    rng = np.random.default_rng(c + groups)
    B0 = rng.integers(-40, 41, size=(groups, c)).astype(np.float64)   # stand-ins for sum g and sum g xhat
    B1 = rng.integers(-40, 41, size=(groups, c)).astype(np.float64)
    rm0, rv0, tr0 = d["rm"].clone(), d["rv"].clone(), torch.zeros(1, dtype=torch.int64, device=DEV)
    plain = _fwd(d["x"], d["res"], d["gamma"], d["beta"], eps, True, groups, rm0, rv0, tr0, want_mask=True)
    assert np.array_equal(_n(plain["save_mean"]).reshape(groups, c), (S0 / m).astype(np.float32))
    if unit > 1:
        assert lib.avt_bn_train_ws_bytes_pre(c, groups, unit + 1) == -1 and lib.avt_bn_train_ws_bytes_pre(c, groups, 129 * unit - 1) == -1
    first = None
    for per in PRE_PER:
        pre_rows = per * unit
        need = int(lib.avt_bn_train_ws_bytes_pre(c, groups, pre_rows))
        fin = -(-per // R.KPRE_ROWS) * unit if per > 2 * R.KPRE_ROWS else 0
        assert need == groups * ((pre_rows + fin) * nq * 64 + 8 * c), (per, need)  # 128: no second array; 129: three more rows x unit

        def workspace(s0, s1):
            ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
            rows = _t(R.partial_rows(s0, s1, c, pre_rows, rng).reshape(-1))
            ws[:rows.numel() * 8].view(torch.float64).copy_(rows)
            return ws

        rm, rv, tr = d["rm"].clone(), d["rv"].clone(), torch.zeros(1, dtype=torch.int64, device=DEV)
        f = _fwd(d["x"], d["res"], d["gamma"], d["beta"], eps, True, groups, rm, rv, tr, want_mask=True, pre=(workspace(S0, S1), pre_rows))
        for n in ("save_mean", "save_invstd", "y"):
            assert _same(f[n], plain[n]), (per, n)
        assert torch.equal(f["mask"], plain["mask"]) and _same(rm, rm0) and _same(rv, rv0) and int(tr.item()) == 1, per
        dx, dgamma, dbeta = torch.empty(groups * m, c, device=DEV), torch.empty(c, device=DEV), torch.empty(c, device=DEV)
        ws = workspace(B0, B1)
        args = (p(d["dy"]), p(d["x"]), groups * m, c, p(d["gamma"]), p(plain["save_mean"]), p(plain["save_invstd"]), groups, p(ws))
        outs = (pre_rows, p(dx), p(dgamma), p(dbeta), ops._stream())
        ops.K.avt_bn_train_bwd_pre(*args, need, *outs)
        assert np.array_equal(_n(dbeta), B0.sum(axis=0).astype(np.float32)) and np.array_equal(_n(dgamma), B1.sum(axis=0).astype(np.float32)), per
        if first is None:
            first = dx
            ref = R.fwd_ref(h["x"], None, h["gamma"], h["beta"], eps, False, groups)
            b = R.bwd_ref(h["dy"], h["x"], None, h["gamma"], ref["mean"], ref["invstd"], groups, k0=B0 / m, k1=B1 / m)
            rep = {"dx": R._ratio(np.abs(_n(dx).astype(np.float64) - b["dx"]), R.dx_bound(b))}
            _hold("pre c%d g%d bwd_pre" % (c, groups), rep)
        assert _same(dx, first), per
        # one byte short: refused, nothing launched (the return code alone)
        assert lib.avt_bn_train_bwd_pre(*args, need - 1, *outs) != 0
        assert lib.avt_bn_train_fwd_pre(p(d["x"]), None, p(f["y"]), groups * m, c, p(d["gamma"]), p(d["beta"]), float(eps), R.MOMENTUM, 1, groups,
                                        p(ws), need - 1, p(f["save_mean"]), p(f["save_invstd"]), None, None, None, None, 0, pre_rows,
                                        ops._stream()) != 0
    torch.cuda.synchronize()


def test_one_row_per_group():
    """Four groups of ONE row (torch refuses the shape; the kernel's documented behaviour is the reference): the variance is
    exactly 0, so invstd = float32(1 / sqrt(float32(eps))) — eps taken as the float it is —, y = beta (+ res), dx exactly 0,
    running_var moves toward 0 by momentum (the M > 1 guard of the unbiased variance: no division by M - 1 = 0), all finite."""
    groups, c = 4, 8
    eps = R.EPS["degenerate"]
    h = _inputs("plain", 1, c, groups)
    out = _run(h, eps, True, False, groups)
    assert out.pop("tracked") == 1 and all(np.all(np.isfinite(v)) for v in out.values())
    assert np.array_equal(out["save_mean"].reshape(groups, c), h["x"])
    want = np.float32(1.0 / np.sqrt(np.float64(np.float32(eps))))
    assert want != np.float32(1.0 / np.sqrt(np.float64(eps)))  # (this eps shows the difference)
    assert np.all(out["save_invstd"] == want)
    assert np.array_equal(out["y"], h["beta"][None, :] + h["res"])  # (x - mean) * sc = 0 exactly; beta + res, one rounding each way
    assert np.all(out["dx"] == 0) and np.array_equal(out["dres"], h["dy"])
    assert np.array_equal(out["dbeta"], h["dy"].astype(np.float64).sum(axis=0).astype(np.float32)) and np.all(out["dgamma"] == 0)
    m32 = np.float32(R.MOMENTUM)
    assert np.array_equal(out["running_var"], (np.float32(1) - m32) * h["rv"] + m32 * np.float32(0))
    assert np.array_equal(out["running_mean"], (np.float32(1) - m32) * h["rm"] + m32 * h["x"][0])
