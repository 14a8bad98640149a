"""The loss head (csrc/softmax_ce.hip, infonce.hip) and the classic baseline's kernels (csrc/pairwise.hip, classic.hip) at
their edges, each against the fp64 references of tests/loss_classic_refs.py (proved on the CPU by
test_loss_classic_refs_host.py): strided loops that take a second trip, guards that fire, dispatch and padding
boundaries, labels other than 0, logits where an fp32 exp would flush, cancelling gradients, zero rows, the LDS limit.

Every bound is derived where it is used; every test prints the figures it asserts on (pytest -s shows them)."""
import numpy as np
import pytest
import torch

import loss_classic_refs as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # fp32 unit roundoff


def _gen(*key):
    return torch.Generator().manual_seed(int(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key))) + 17)


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32)


def _np(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------- softmax cross-entropy
CE_SHAPES = [(1, 1), (3, 2), (4, 63), (5, 64), (9, 65), (2, 130), (7, 1000)]
CE_KINDS = ["randn10", "randn80", "shift1e4", "ties", "neg_inf"]
CE_CASES = [(b, c, k) for b, c in CE_SHAPES for k in CE_KINDS if c > 1 or k not in ("ties", "neg_inf")]


def _ce_labels(b, c):
    """Random int64 labels that include 0, c - 1 and (c > 64: c - 1 already is) a column past the first 64-lane trip."""
    lab = torch.randint(0, c, (b,), generator=_gen(b, c, 1)).numpy().astype(np.int64)
    lab[0] = 0
    lab[-1] = c - 1
    if b >= 3 and c > 64:
        lab[1] = 64 + (c - 64) // 2
    return lab


def _ce_logits(b, c, kind, lab):
    x = torch.randn(b, c, generator=_gen(b, c, 2)).numpy().astype(np.float32)
    if kind == "randn80":  # an fp32 exp(x - max) would flush most entries; 80 * (spread of c normals) stays below fp64's 745
        return x * np.float32(80)
    x = x * np.float32(10)
    if kind == "shift1e4":  # softmax is shift-invariant; max + log(sum) - x[y] at 1e4 would carry 1e-12 of absolute error
        return x + np.float32(1e4)
    rng = np.random.default_rng(1000 * b + c)
    if kind == "ties":  # two or three entries share the maximum; on odd rows the label is one of them
        for r in range(b):
            cols = set(rng.choice(c, size=min(c, 3), replace=False).tolist())
            if r % 2:
                cols.add(int(lab[r]))
            x[r, sorted(cols)] = x[r].max() + np.float32(1.5)
    if kind == "neg_inf":  # never column 0 (the label of the label-less run), never the label's column, never a whole row
        for r in range(b):
            free = [j for j in range(c) if j != 0 and j != lab[r]]
            if free:
                x[r, rng.choice(free, size=max(1, len(free) // 3), replace=False)] = -np.inf
        assert np.isinf(x).any() and not np.isinf(x).all(axis=1).any()
    return x


def _check_ce_fwd(what, loss, prob, x, lab):
    """loss, prob within one fp32 ulp of the fp64 value: the kernel works in fp64 (exp, log1p: a few fp64 ulp) and rounds to
    fp32 once, so it can differ from the correctly rounded fp32 value only next to a rounding tie, by one ulp."""
    rl, rp = R.softmax_ce_ref(x, lab)
    loss, prob = _np(loss).astype(np.float64), _np(prob).astype(np.float64)
    el, ep = np.abs(loss - rl) / R.ulp32(rl), np.abs(prob - rp) / R.ulp32(rp)
    rows = np.abs(prob.sum(axis=1) - 1.0)
    print("%s: loss %.3f ulp, prob %.3f ulp, |row sum - 1| %.2e (bound %.2e), %d prob entries at 0"
          % (what, el.max(), ep.max(), rows.max(), x.shape[1] * U, int((prob == 0).sum())))
    assert np.isfinite(loss).all() and (el <= 1.0).all()
    assert (ep <= 1.0).all()
    # below HALF the smallest fp32 subnormal the correctly rounded value is 0 (from there to 2^-149 it is 2^-149: the ulp
    # bound above covers that band)
    assert (prob[rp < 2.0 ** -150] == 0).all()
    assert (rows <= x.shape[1] * U).all()  # c roundings of at most 2^-24 each (entries <= 1), an exact sum otherwise


@pytest.mark.parametrize("b,c,kind", CE_CASES)
def test_softmax_ce_forward(avt, dev, b, c, kind):
    lab = _ce_labels(b, c)
    x = _ce_logits(b, c, kind, lab)
    xd = torch.from_numpy(x).to(dev)
    l0, p0 = avt.ops.softmax_ce_fwd(xd)  # label = NULL
    lz, pz = avt.ops.softmax_ce_fwd(xd, torch.zeros(b, dtype=torch.int64, device=dev))
    assert np.array_equal(_bits(l0), _bits(lz)) and np.array_equal(_bits(p0), _bits(pz))
    _check_ce_fwd("(%d,%d) %s label=None" % (b, c, kind), l0, p0, x, None)
    ll, pl = avt.ops.softmax_ce_fwd(xd, torch.from_numpy(lab).to(dev))
    assert np.array_equal(_bits(pl), _bits(p0))  # prob does not depend on the label
    _check_ce_fwd("(%d,%d) %s labels %s" % (b, c, kind, lab.tolist()), ll, pl, x, lab)


def test_softmax_ce_forward_keeps_a_loss_below_one_ulp_of_one(avt, dev):
    """The label on a maximum far above the rest: loss = log1p(rest) with rest from 1e-7 down to 1e-40, past the second
    trip of the strided loop, with and without a shift of 1e4."""
    c, gaps = 130, [16.0, 20.0, 30.0, 50.0, 80.0, 95.0]
    x = np.zeros((2 * len(gaps), c), np.float32)
    lab = np.array([(37 * r + 70) % c for r in range(len(x))], np.int64)
    for r in range(len(x)):
        x[r, lab[r]] = gaps[r % len(gaps)]
    x[len(gaps):] += np.float32(1e4)
    loss, prob = avt.ops.softmax_ce_fwd(torch.from_numpy(x).to(dev), torch.from_numpy(lab).to(dev))
    _check_ce_fwd("label on a lone maximum", loss, prob, x, lab)
    assert (_np(loss) > 0).all()


def test_softmax_ce_loss_only_and_prob_only_forms(avt, dev):
    """Straight through the C ABI: prob = NULL gives the same loss bits, loss = NULL the same prob bits."""
    b, c = 9, 65
    lab = _ce_labels(b, c)
    xd = torch.from_numpy(_ce_logits(b, c, "randn10", lab)).to(dev)
    ld = torch.from_numpy(lab).to(dev)
    loss, prob = avt.ops.softmax_ce_fwd(xd, ld)
    lib, p, st = avt._lib.lib(), avt.ops._p, avt.ops._stream
    loss_only = torch.full((b,), 7.0, device=dev)
    prob_only = torch.full((b, c), 7.0, device=dev)
    assert lib.avt_softmax_ce_fwd(p(xd), b, c, p(ld), p(loss_only), None, st()) == 0
    assert lib.avt_softmax_ce_fwd(p(xd), b, c, p(ld), None, p(prob_only), st()) == 0
    assert np.array_equal(_bits(loss_only), _bits(loss)) and np.array_equal(_bits(prob_only), _bits(prob))
    assert lib.avt_softmax_ce_fwd(p(xd), b, c, p(ld), None, None, st()) != 0  # nothing to write is an error, not a no-op


@pytest.mark.parametrize("b,c", CE_SHAPES)  # (9,65) and (7,1000): b * c = 585 and 7000, several 256-thread blocks and a tail
def test_softmax_ce_backward_is_the_fp32_expression(avt, dev, b, c):
    lab = _ce_labels(b, c)
    _, prob = avt.ops.softmax_ce_fwd(torch.from_numpy(_ce_logits(b, c, "randn10", lab)).to(dev))
    for scale in (1.0, 1.0 / b):
        for labels in (None, lab):
            d = avt.ops.softmax_ce_bwd(prob, None if labels is None else torch.from_numpy(labels).to(dev), scale=scale)
            want = R.softmax_ce_bwd_ref(_np(prob), labels, scale)
            assert np.array_equal(_np(d), want), (scale, labels)


def test_criterion_matches_fp64_cross_entropy(avt, dev):
    """InfoNCECriterion with non-zero labels vs torch.nn.functional.cross_entropy in fp64 autograd."""
    b, c = 5, 65
    lab = _ce_labels(b, c)
    assert (lab != 0).any()
    x = torch.from_numpy(_ce_logits(b, c, "randn10", lab))
    xd = x.to(dev).requires_grad_()
    loss = avt.models.InfoNCECriterion()(xd, torch.from_numpy(lab).to(dev))
    loss.backward()
    x64 = x.double().requires_grad_()
    ref = torch.nn.functional.cross_entropy(x64, torch.from_numpy(lab))
    ref.backward()
    rel = abs(float(loss) - float(ref)) / abs(float(ref))
    g, g64 = _np(xd.grad).astype(np.float64), x64.grad.numpy()
    bound = float(np.spacing(np.float32(np.abs(g64).max())))
    print("criterion: loss rel err %.3e (bound %.3e), grad max err %.3e (bound %.3e)" % (rel, 2.0 ** -23, np.abs(g - g64).max(), bound))
    # each row's loss is within 2^-24 relative of fp64 (one rounding); the fp32 mean of 5 positive terms adds at most 4 more
    # roundings to every term, so 5 * 2^-24 bounds the worst case and 2^-23 what rounding errors of either sign leave of it
    assert rel <= 2.0 ** -23
    assert (np.abs(g - g64) <= bound).all()


def test_out_of_range_labels_mark_their_rows_and_read_nothing(avt, dev):
    """A label < 0 or >= c: NaN in that row's loss and dlogits, prob and every other row as with valid labels.  The logits are
    the middle rows of a larger allocation, so that an unchecked x[label] stays inside allocated memory."""
    b, c, pad = 9, 65, 4
    big = torch.randn(b + 2 * pad, c, generator=_gen(b, c, 3)).mul(10).to(dev)
    xd = big[pad : pad + b]
    assert xd.is_contiguous() and xd.data_ptr() == big.data_ptr() + pad * c * 4
    lab = _ce_labels(b, c)
    bad = lab.copy()
    bad_rows = {2: -1, 3: 2 * c + 3, 5: c, 6: -c}  # all within two rows of their own
    for r, v in bad_rows.items():
        bad[r] = v
    l_ok, p_ok = avt.ops.softmax_ce_fwd(xd, torch.from_numpy(lab).to(dev))
    d_ok = avt.ops.softmax_ce_bwd(p_ok, torch.from_numpy(lab).to(dev), scale=1.0 / b)
    l_bad, p_bad = avt.ops.softmax_ce_fwd(xd, torch.from_numpy(bad).to(dev))
    d_bad = avt.ops.softmax_ce_bwd(p_bad, torch.from_numpy(bad).to(dev), scale=1.0 / b)
    torch.cuda.synchronize()
    marked = np.zeros(b, bool)
    marked[list(bad_rows)] = True
    print("loss with bad labels:", _np(l_bad).tolist())
    assert np.array_equal(np.isnan(_np(l_bad)), marked)
    assert np.array_equal(_bits(l_bad)[~marked], _bits(l_ok)[~marked])
    assert np.array_equal(_bits(p_bad), _bits(p_ok)) and np.isfinite(_np(p_bad)).all()
    assert np.array_equal(np.isnan(_np(d_bad)), np.repeat(marked[:, None], c, axis=1))
    assert np.array_equal(_bits(d_bad)[~marked], _bits(d_ok)[~marked])


# ---------------------------------------------------------------- InfoNCE logits
NCE_TEMP, NCE_EPS = 0.1, 1e-12
NCE_SHAPES = [(2, 3, d) for d in (1, 255, 256, 257, 1024, 1025, 4096, 4097, 16384)] + [(1, 1, 257), (3, 2, 257), (3, 15, 257)]
NCE_KINDS = ["randn", "pooled_relu", "scaled_1e-3", "scaled_1e3", "zero_q_row", "zero_t_row"]


def _nce_inputs(b, n, d, kind):
    """-> (q, t, g, base): base = the (q, t) whose logits this case must reproduce (the unscaled inputs of a scaled case)."""
    gen = _gen(b, n, d, 4)
    q, t, g = torch.randn(b, d, generator=gen), torch.randn(b, n, d, generator=gen), torch.randn(b, n, generator=gen)
    if kind == "pooled_relu":  # what the encoders hand over: average-pooled ReLU outputs, all >= 0, cosines near 1
        q, t = torch.relu(q + 2), torch.relu(t + 2)
    base = (q.clone(), t.clone())
    if kind.startswith("scaled"):
        s = float(kind.split("_")[1])
        q = q * s
        t[:, ::2] = t[:, ::2] * s
    if kind == "zero_q_row":
        q[0] = 0
        base = (q.clone(), t.clone())
    if kind == "zero_t_row":
        t[b - 1, n - 1] = 0
        base = (q.clone(), t.clone())
    return q, t, g, base


def _nce_stock_fp32(q, t, g, dev):
    """What the fused kernels replace: F.normalize / bmm / temp with autograd, fp32, on the device."""
    qs, ts = q.to(dev).requires_grad_(), t.to(dev).requires_grad_()
    out = R.infonce_expr(qs, ts, NCE_TEMP, NCE_EPS)
    out.backward(g.to(dev))
    return out.detach(), qs.grad, ts.grad


def _nce_check(what, got, stock, ref, base_logits, q, t):
    """Kernel no further from fp64 than twice the stock fp32 ops are (another summation order, nothing more), or within the
    project's tolerance for this op (test_infonce_fused_fwd_bwd_matches_autograd: 2e-5 on logits, 1e-5 * max(1, max|grad|)
    on gradients), whichever is larger.  The gradients are judged vector by vector (dq per b, dt per (b, j)), each with its
    own stock error and its own max|grad|: a zero row's gradient is 1/eps = 1e12 times a unit vector, and one floor for the
    whole tensor would then say nothing about the ordinary rows next to it."""
    for name, k, s, r in zip(("logits", "dq", "dt"), got[:3], stock, (ref["logits"], ref["dq"], ref["dt"])):
        dims = () if name == "logits" else (-1,)
        ek, es = (k.cpu().double() - r).abs().amax(dims).reshape(-1), (s.cpu().double() - r).abs().amax(dims).reshape(-1)
        floor = torch.full_like(ek, 2e-5) if name == "logits" else 1e-5 * r.abs().amax(dims).reshape(-1).clamp_min(1.0)
        allowed = torch.maximum(2.0 * es, floor)
        w = int((ek / allowed).argmax())  # the vector closest to (or furthest past) what it is allowed
        print("infonce %s | %s | kernel %.2e | stock %.2e | allowed %.2e | used %.3f"
              % (what, name, float(ek[w]), float(es[w]), float(allowed[w]), float(ek[w] / allowed[w])))
        assert bool(torch.isfinite(ek).all()) and bool((ek <= allowed).all()), (what, name, ek.tolist(), es.tolist(), floor.tolist())
    logits, inv_q, inv_t = got[0], got[3], got[4]
    # scaling a row by 1e-3 or 1e3 leaves its unit vector alone: the logits stay at those of the unscaled inputs
    e_base = float((logits.cpu().double() - base_logits).abs().max())
    es_base = float((stock[0].cpu().double() - base_logits).abs().max())
    assert e_base <= max(2.0 * es_base, 2e-5), (what, e_base, es_base)
    # inv norms: an sqrtf and a divide of half an ulp each, plus half the relative error of the fp32 sum of squares.  That sum is
    # up to 64 sequential adds per thread and a tree over 256 threads: its worst case is far past 4 ulp, its typical error
    # (roundings of either sign) well inside.  So this bound holds for these pinned inputs, statistically, not by construction:
    # a miss after a change of seed or of summation order is not by itself a kernel bug (measured: 1.83 ulp at the most).
    for name, k, r in (("inv_q", inv_q, ref["inv_q"]), ("inv_t", inv_t, ref["inv_t"])):
        e = np.abs(_np(k).astype(np.float64) - r.numpy()) / R.ulp32(r.numpy())
        print("infonce %s %-6s %.2f ulp" % (what, name, e.max()))
        assert (e <= 4.0).all(), (what, name, e.max())
    one_over_eps = np.float32(1.0) / np.float32(NCE_EPS)
    zq = _np((q == 0).all(dim=1))
    zt = _np((t == 0).all(dim=2))
    assert (_np(inv_q)[zq] == one_over_eps).all() and (_np(inv_t)[zt] == one_over_eps).all()
    assert (_np(logits)[zq] == 0).all() and (_np(logits)[zt] == 0).all()


@pytest.mark.parametrize("kind", NCE_KINDS)
@pytest.mark.parametrize("b,n,d", NCE_SHAPES)
def test_infonce_fwd_bwd(avt, dev, b, n, d, kind):
    """Measured on an MI355X, max-abs error against fp64 as kernel/stock of the vector that uses most of what it is allowed
    (the largest share used by any case: logits 0.07, dq 0.05, dt 0.25 of max(2 * stock, floor)):

    b,n,d      kind         logits             dq                 dt
    2,3,1      randn        9.54e-07/0.00e+00  3.55e-15/3.55e-15  2.48e-06/1.91e-06
    2,3,1      pooled_relu  9.54e-07/0.00e+00  5.17e-07/0.00e+00  1.48e-07/0.00e+00
    2,3,1      scaled_1e-3  9.54e-07/0.00e+00  0.00e+00/0.00e+00  1.76e-06/9.54e-07
    2,3,1      scaled_1e3   9.54e-07/0.00e+00  0.00e+00/3.73e-09  8.81e-07/9.54e-07
    2,3,1      zero_q_row   9.54e-07/0.00e+00  5.84e+05/6.00e+04  2.48e-06/1.91e-06
    2,3,1      zero_t_row   9.54e-07/0.00e+00  0.00e+00/3.81e-06  2.48e-06/1.91e-06
    2,3,255    randn        5.46e-08/2.64e-07  6.74e-08/3.90e-08  4.42e-08/3.45e-08
    2,3,255    pooled_relu  1.31e-06/1.31e-06  1.98e-08/1.98e-08  8.31e-09/8.68e-09
    2,3,255    scaled_1e-3  7.38e-08/1.86e-07  1.48e-05/9.79e-06  1.66e-05/1.05e-05
    2,3,255    scaled_1e3   6.89e-08/2.39e-07  3.03e-11/3.91e-11  3.30e-08/3.47e-08
    2,3,255    zero_q_row   5.46e-08/2.43e-07  1.62e+05/1.30e+05  4.42e-08/3.45e-08
    2,3,255    zero_t_row   5.46e-08/2.64e-07  5.61e-08/5.61e-08  5.46e+04/6.86e+04
    2,3,256    randn        1.02e-07/1.73e-07  2.35e-08/1.67e-08  1.68e-08/1.88e-08
    2,3,256    pooled_relu  1.33e-06/1.76e-06  7.55e-09/4.81e-09  5.49e-09/4.92e-09
    2,3,256    scaled_1e-3  4.87e-08/1.38e-07  2.57e-05/1.39e-05  1.61e-05/8.55e-06
    2,3,256    scaled_1e3   4.01e-08/1.33e-07  2.34e-11/1.31e-11  9.24e-09/4.47e-09
    2,3,256    zero_q_row   4.46e-08/1.73e-07  2.20e+05/2.08e+05  1.68e-08/1.88e-08
    2,3,256    zero_t_row   1.02e-07/1.73e-07  2.35e-08/1.67e-08  1.44e+05/2.39e+05
    2,3,257    randn        1.41e-07/1.41e-07  4.00e-08/4.00e-08  2.04e-08/3.38e-08
    2,3,257    pooled_relu  6.40e-07/1.00e-06  8.05e-09/8.97e-09  5.53e-09/5.73e-09
    2,3,257    scaled_1e-3  2.15e-07/2.62e-07  2.48e-05/1.99e-05  2.62e-05/1.09e-05
    2,3,257    scaled_1e3   1.33e-07/1.50e-07  2.63e-11/2.78e-11  1.33e-08/1.30e-08
    2,3,257    zero_q_row   1.41e-07/1.41e-07  5.90e+05/5.90e+05  1.98e-08/1.55e-08
    2,3,257    zero_t_row   1.41e-07/1.41e-07  4.00e-08/4.00e-08  1.07e+05/1.02e+05
    2,3,1024   randn        6.53e-08/2.42e-07  1.08e-08/1.83e-08  1.15e-08/1.39e-08
    2,3,1024   pooled_relu  9.96e-07/1.11e-06  3.96e-09/5.35e-09  3.55e-09/2.98e-09
    2,3,1024   scaled_1e-3  5.93e-08/2.18e-07  6.40e-06/7.17e-06  3.83e-06/5.60e-06
    2,3,1024   scaled_1e3   5.18e-08/2.16e-07  1.18e-11/1.24e-11  9.49e-09/1.05e-08
    2,3,1024   zero_q_row   6.53e-08/2.42e-07  1.44e+05/1.99e+05  1.15e-08/1.39e-08
    2,3,1024   zero_t_row   3.92e-08/2.42e-07  7.87e-09/1.40e-08  6.61e+04/4.79e+04
    2,3,1025   randn        3.81e-08/1.24e-07  1.03e-08/1.32e-08  8.54e-09/7.86e-09
    2,3,1025   pooled_relu  1.12e-06/1.30e-06  6.99e-09/8.17e-09  2.44e-09/3.07e-09
    2,3,1025   scaled_1e-3  5.45e-08/1.25e-07  9.88e-06/6.54e-06  6.44e-06/2.98e-06
    2,3,1025   scaled_1e3   9.81e-08/1.33e-07  1.52e-11/1.14e-11  4.96e-09/3.59e-09
    2,3,1025   zero_q_row   3.78e-08/8.14e-08  3.53e+05/4.61e+05  3.83e-09/2.35e-09
    2,3,1025   zero_t_row   3.81e-08/1.24e-07  1.03e-08/1.32e-08  1.22e+05/7.58e+04
    2,3,4096   randn        3.55e-08/1.55e-07  2.07e-09/1.64e-09  1.36e-09/1.06e-09
    2,3,4096   pooled_relu  1.19e-06/3.94e-06  6.77e-10/8.51e-10  5.32e-10/4.89e-10
    2,3,4096   scaled_1e-3  3.94e-08/1.80e-07  1.84e-06/2.12e-06  1.07e-06/7.55e-07
    2,3,4096   scaled_1e3   3.71e-08/1.86e-07  1.81e-12/1.81e-12  2.02e-09/9.64e-10
    2,3,4096   zero_q_row   1.36e-08/1.28e-07  9.42e+04/9.61e+04  1.36e-09/1.06e-09
    2,3,4096   zero_t_row   3.55e-08/1.55e-07  2.01e-09/1.80e-09  5.66e+04/5.38e+04
    2,3,4097   randn        3.71e-08/1.37e-07  9.91e-10/8.35e-10  6.94e-10/5.23e-10
    2,3,4097   pooled_relu  1.24e-06/3.99e-06  2.48e-10/1.78e-10  3.27e-10/1.69e-10
    2,3,4097   scaled_1e-3  2.91e-08/1.64e-07  9.23e-07/7.86e-07  2.49e-07/2.45e-07
    2,3,4097   scaled_1e3   4.27e-08/1.77e-07  7.03e-13/8.00e-13  4.49e-10/6.72e-10
    2,3,4097   zero_q_row   1.97e-08/9.46e-08  4.55e+04/4.55e+04  6.94e-10/5.23e-10
    2,3,4097   zero_t_row   3.71e-08/1.37e-07  9.91e-10/8.35e-10  2.43e+04/4.46e+04
    2,3,16384  randn        1.85e-08/1.27e-07  5.08e-10/4.53e-10  5.30e-10/2.24e-10
    2,3,16384  pooled_relu  1.18e-06/5.64e-06  3.60e-10/1.95e-10  2.55e-10/1.30e-10
    2,3,16384  scaled_1e-3  2.30e-08/1.48e-07  5.20e-07/4.13e-07  3.79e-07/2.41e-07
    2,3,16384  scaled_1e3   2.70e-08/1.46e-07  8.25e-13/4.28e-13  1.36e-10/1.83e-10
    2,3,16384  zero_q_row   1.85e-08/1.27e-07  6.06e+04/5.11e+04  4.28e-10/3.87e-10
    2,3,16384  zero_t_row   1.85e-08/1.27e-07  5.08e-10/4.53e-10  3.78e+04/3.88e+04
    1,1,257    randn        4.81e-08/1.08e-07  3.01e-08/3.01e-08  2.98e-08/2.81e-08
    1,1,257    pooled_relu  1.35e-06/3.98e-07  9.61e-09/7.60e-09  1.33e-08/7.52e-09
    1,1,257    scaled_1e-3  9.21e-08/2.71e-08  2.62e-05/1.73e-05  2.26e-05/1.89e-05
    1,1,257    scaled_1e3   3.66e-08/6.82e-09  3.00e-11/1.76e-11  2.10e-11/1.91e-11
    1,1,257    zero_q_row   0.00e+00/0.00e+00  3.72e+05/3.72e+05  0.00e+00/0.00e+00
    1,1,257    zero_t_row   0.00e+00/0.00e+00  0.00e+00/0.00e+00  2.91e+05/3.31e+05
    3,2,257    randn        9.37e-08/2.64e-07  3.16e-08/3.15e-08  4.96e-08/2.96e-08
    3,2,257    pooled_relu  9.19e-07/1.17e-06  1.16e-08/1.16e-08  1.50e-08/7.90e-09
    3,2,257    scaled_1e-3  1.08e-07/1.80e-07  2.79e-05/2.56e-05  1.60e-05/1.67e-05
    3,2,257    scaled_1e3   9.11e-08/1.45e-07  4.77e-11/3.12e-11  2.29e-08/1.74e-08
    3,2,257    zero_q_row   9.37e-08/2.64e-07  2.80e+05/4.43e+05  4.96e-08/2.96e-08
    3,2,257    zero_t_row   9.37e-08/2.64e-07  2.76e-08/2.93e-08  5.36e+05/5.12e+05
    3,15,257   randn        1.75e-07/2.38e-07  5.50e-08/4.32e-08  2.83e-08/1.71e-08
    3,15,257   pooled_relu  1.22e-06/1.61e-06  2.59e-08/1.87e-08  9.55e-09/8.83e-09
    3,15,257   scaled_1e-3  1.42e-07/2.15e-07  5.90e-05/3.50e-05  1.57e-05/7.95e-06
    3,15,257   scaled_1e3   1.45e-07/2.55e-07  6.26e-11/4.20e-11  4.09e-08/1.76e-08
    3,15,257   zero_q_row   1.17e-07/2.38e-07  6.28e+05/7.08e+05  2.21e-08/1.70e-08
    3,15,257   zero_t_row   1.75e-07/2.38e-07  5.40e-08/4.25e-08  2.20e+05/1.38e+05
    """
    q, t, g, base = _nce_inputs(b, n, d, kind)
    ref = R.infonce_ref(q, t, NCE_TEMP, NCE_EPS, g)
    base_logits = R.infonce_ref(base[0], base[1], NCE_TEMP, NCE_EPS)["logits"]
    qd, td, gd = q.to(dev), t.to(dev), g.to(dev)
    logits, inv_q, inv_t = avt.ops.infonce_fwd(qd, td, NCE_TEMP, NCE_EPS)
    dq, dt = avt.ops.infonce_bwd(qd, td, logits, gd, inv_q, inv_t, NCE_TEMP)
    assert logits.shape == (b, n) and inv_q.shape == (b,) and inv_t.shape == (b, n) and dq.shape == q.shape and dt.shape == t.shape
    _nce_check("(%d,%d,%d) %s" % (b, n, d, kind), (logits, dq, dt, inv_q, inv_t), _nce_stock_fp32(q, t, g, dev), ref, base_logits, q, t)
    if kind in ("zero_q_row", "zero_t_row"):
        assert int((q == 0).all(dim=1).sum()) + int((t == 0).all(dim=2).sum()) == 1


def test_infonce_through_the_autograd_function(avt, dev):
    b, n, d = 3, 15, 257
    q, t, g, base = _nce_inputs(b, n, d, "pooled_relu")
    ref = R.infonce_ref(q, t, NCE_TEMP, NCE_EPS, g)
    qd, td = q.to(dev).requires_grad_(), t.to(dev).requires_grad_()
    out, qh, th = avt.models._InfoNCELogits.apply_ops(qd, td, NCE_TEMP)
    assert qh is None and th is None
    out.backward(g.to(dev))
    inv = avt.ops.infonce_fwd(qd.detach(), td.detach(), NCE_TEMP, NCE_EPS)
    assert np.array_equal(_bits(out), _bits(inv[0]))
    _nce_check("(3,15,257) pooled_relu apply_ops", (out.detach(), qd.grad, td.grad, inv[1], inv[2]), _nce_stock_fp32(q, t, g, dev), ref,
               ref["logits"], q, t)


def test_infonce_refuses_a_row_past_the_register_limit(avt, dev):
    """d = 16385 is one past the last legal row length: an error, and nothing is written."""
    b, n, d = 2, 3, 16385
    q, t = torch.randn(b, d, device=dev), torch.randn(b, n, d, device=dev)
    with pytest.raises(avt._lib.AvtError):
        avt.ops.infonce_fwd(q, t, NCE_TEMP)
    lib, p, st = avt._lib.lib(), avt.ops._p, avt.ops._stream
    outs = [torch.full(s, 7.0, device=dev) for s in ((b, n), (b,), (b, n), (b, d), (b, n, d))]
    logits, inv_q, inv_t, dq, dt = outs
    assert lib.avt_infonce_fwd(p(q), p(t), b, n, d, NCE_TEMP, NCE_EPS, p(logits), p(inv_q), p(inv_t), st()) != 0
    assert lib.avt_infonce_bwd(p(q), p(t), p(logits), p(logits), p(inv_q), p(inv_t), b, n, d, NCE_TEMP, p(dq), p(dt), st()) != 0
    with pytest.raises(avt._lib.AvtError):
        avt.ops.infonce_bwd(q, t, logits, logits, inv_q, inv_t, NCE_TEMP)
    torch.cuda.synchronize()
    assert all(bool((o == 7.0).all()) for o in outs)


# ---------------------------------------------------------------- pairwise L2
@pytest.mark.parametrize("dup", [False, True])
@pytest.mark.parametrize("n,d", [(1, 1), (7, 5), (8, 255), (9, 256), (17, 257), (12, 1000)])
def test_pairwise_l2_is_within_one_ulp(avt, dev, n, d, dup):
    """fp64 accumulation of fp64 squares and ONE rounding to fp32: within one fp32 ulp of the exactly summed value."""
    x = (torch.randn(n, d, generator=_gen(n, d, 5)) * 100).numpy().astype(np.float32)
    if dup:
        x[n - 1] = x[n // 3]  # two identical rows (n = 1: the row itself)
    out = _np(avt.ops.pairwise_l2(torch.from_numpy(x).to(dev)))
    ref = R.pairwise_ref(x)
    e = np.abs(out.astype(np.float64) - ref) / R.ulp32(ref)
    print("pairwise (%d,%d) dup=%s: %.3f ulp" % (n, d, dup, e.max()))
    assert out.shape == (n, n) and (e <= 1.0).all()
    assert (np.diag(out) == 0).all()
    assert np.array_equal(out.view(np.uint32), out.T.view(np.uint32))
    if dup:
        assert out[n - 1, n // 3] == 0 and out[n // 3, n - 1] == 0
    if n > 1:
        assert (out[~np.eye(n, dtype=bool) & (ref > 0)] > 0).all()


# ---------------------------------------------------------------- diagonal filter
@pytest.mark.parametrize("weights", ["binomial", "random_sign"])
@pytest.mark.parametrize("n,fs", [(1, 1), (5, 1), (5, 5), (17, 4), (33, 2), (40, 16)])
def test_diag_filter_within_the_fma_chain_bound(avt, dev, n, fs, weights):
    gen = _gen(n, fs, 6)
    if weights == "binomial":
        w = (np.poly1d([0.5, 0.5]) ** (fs - 1)).coeffs.astype(np.float32)
        d1 = (torch.randn(n, n, generator=gen).abs() * 50).numpy().astype(np.float32)
    else:  # terms of either sign: the sum cancels and only the bound on sum |w d| holds
        w = torch.randn(fs, generator=gen).numpy().astype(np.float32)
        d1 = (torch.randn(n, n, generator=gen) * 50).numpy().astype(np.float32)
    assert w.shape == (fs,)
    out = _np(avt.ops.diag_filter(torch.from_numpy(d1).to(dev), torch.from_numpy(w).to(dev))).astype(np.float64)
    ref, mag = R.diag_filter_ref(d1, w)
    m = n - fs + 1
    err = np.abs(out - ref)
    print("diag_filter (%d,%d) %s: max err / (fs 2^-24 sum|w d|) = %.3f" % (n, fs, weights, (err / (fs * U * mag + 1e-300)).max()))
    assert out.shape == (m, m)
    assert (err <= fs * U * mag).all()  # fs fused multiply-adds, each rounding a partial sum that sum |w d| bounds
    if fs == 1:
        assert np.array_equal(out, (w[0] * d1).astype(np.float64))  # one rounded fp32 multiply


# ---------------------------------------------------------------- q-learning
def _q_run(avt, dev, d3, alpha, tol, max_iter):
    out, iters = avt.ops.q_learning(torch.from_numpy(d3).to(dev), alpha, tol, max_iter)
    return _np(out), int(iters.item())


@pytest.mark.parametrize("alpha", R.Q_ALPHAS)
@pytest.mark.parametrize("n", R.Q_SIZES)  # 2: the smallest; 64 / 65: one lane trip and two; 200: the LDS limit
def test_q_learning_is_bit_equal_to_the_sweep(avt, dev, n, alpha):
    d3 = R.q_input(n)
    want, sweeps, res = R.q_case(n, alpha)
    got, iters = _q_run(avt, dev, d3, alpha, R.Q_TOL, 1000)
    print("q_learning n=%d alpha=%g: %d sweeps (reference %d), residuals %s" % (n, alpha, iters, sweeps, [float(r) for r in res]))
    assert iters == sweeps
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[0].view(np.uint32), d3[0].view(np.uint32))
    assert not np.array_equal(got[1:], d3[1:])


def test_q_learning_stops_at_max_iter_and_at_a_loose_tol(avt, dev):
    n, alpha = 65, 0.997
    d3 = R.q_input(n)
    want5, it5, _ = R.q_case(n, alpha, R.Q_TOL, 5)
    assert it5 == 5 and R.q_case(n, alpha)[1] > 5  # the tolerance alone would go on
    got5, iters5 = _q_run(avt, dev, d3, alpha, R.Q_TOL, 5)
    assert iters5 == 5 and np.array_equal(got5.view(np.uint32), want5.view(np.uint32))
    want1, it1, _ = R.q_case(n, alpha, 1e30, 1000)
    got1, iters1 = _q_run(avt, dev, d3, alpha, 1e30, 1000)
    assert it1 == 1 and iters1 == 1 and np.array_equal(got1.view(np.uint32), want1.view(np.uint32))


def test_q_learning_refuses_what_does_not_fit(avt, dev):
    lib, p, st = avt._lib.lib(), avt.ops._p, avt.ops._stream
    assert lib.avt_q_learning_supported(1) == 0 and lib.avt_q_learning_supported(201) == 0
    assert lib.avt_q_learning_supported(2) == 1 and lib.avt_q_learning_supported(200) == 1
    assert not avt.ops.q_learning_supported(201)
    d3 = torch.rand(201, 201, device=dev) + 0.1
    with pytest.raises(avt._lib.AvtError):
        avt.ops.q_learning(d3, 0.997)
    out = torch.full((201, 201), 7.0, device=dev)
    iters = torch.full((1,), -3, dtype=torch.int32, device=dev)
    assert lib.avt_q_learning_f32(p(d3), 201, 0.997, 1e-3, 1000, p(out), p(iters), st()) != 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and int(iters.item()) == -3  # refused before any launch
