"""References and edge inputs of the N x N build of validate(): csrc/l2norm.hip, csrc/sim_gemm.hip (and the 256 x 256 tile
behind avt_gemm_nt_x3_f32out) and csrc/transition.hip, for tests/test_gpu_nxn_edges.py, proved on the CPU by
tests/test_nxn_refs_host.py.  Plain numpy / torch, no HIP, and nothing of oracle/: each reference restates the operation
(or the reference's own lines), none the kernel's order of work.  The input builders live here so that the host test
checks the C oracle on exactly the inputs the GPU test feeds the kernels."""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24  # fp32 unit roundoff


def _rng(*key):
    return np.random.default_rng([17] + [int(k) for k in key])


def same_with_nan(a, b):
    """Equal as values, NaN equal to NaN (whatever its sign or payload), -0 equal to +0."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(np.isnan(a), np.isnan(b))) and bool(np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]))


def bf16_bits(x):
    """fp32 values that ARE bf16 numbers -> their 16 bits (asserted: nothing is rounded here)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    assert not (u & 0xFFFF).any(), "not a bf16 value"
    return (u >> 16).astype(np.uint16)


def bf16_value(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


# ---------------------------------------------------------------- l2norm
def l2norm64(x0, x1=None, eps=1e-12):
    """x / max(sqrt(sum x^2), eps) per row in fp64 (numpy's pairwise fp64 sum: 1e-16 relative, nothing next to fp32)."""
    x = np.asarray(x0, np.float32).astype(np.float64)
    if x1 is not None:
        x = np.concatenate([x, np.asarray(x1, np.float32).astype(np.float64)], axis=1)
    with np.errstate(all="ignore"):
        nrm = np.sqrt((x * x).sum(axis=1, keepdims=True))
        return x / np.maximum(nrm, eps)


def l2norm_torch(x0, x1=None, eps=1e-12):
    """The reference's own line (models.py:347-351): torch.cat + F.normalize in fp32 on the CPU.  It decides where fp32
    semantics are the point: NaN, inf, a sum of squares past the fp32 range, a norm below eps."""
    x = torch.from_numpy(np.ascontiguousarray(x0, np.float32))
    if x1 is not None:
        x = torch.cat([x, torch.from_numpy(np.ascontiguousarray(x1, np.float32))], dim=1)
    return F.normalize(x, dim=1, eps=eps).numpy()



# (d0, d1): across the 3072-element register cache of the float4 kernel, the production split, the scalar kernel's widths
L2_WIDTHS = [(4, 0), (256, 0), (3068, 0), (3072, 0), (3076, 0), (2304, 768), (8, 3), (1, 0), (2, 0), (3, 0), (63, 0), (65, 0)]
L2_ROWS = [1, 4, 5]  # four rows per workgroup: one short, exactly one, one over
L2_SCALES = [1e-30, 1e-20, 1.0, 1e18]
L2_SCALE_WIDTHS = [(256, 0), (3076, 0), (65, 0), (3072, 0)]
L2_SPECIAL = ["nan", "inf", "zero"]
L2_SPECIAL_WIDTHS = [(256, 0), (3076, 0), (65, 0), (2304, 768)]


def l2norm_input(n, d0, d1, scale=1.0, special=None):
    """-> (x0, x1 | None).  special rows: row n // 2 gets one NaN / one +inf at column (d // 3) / is all zero."""
    r = _rng(n, d0, d1, 1)
    x = (r.standard_normal((n, d0 + d1)) * scale).astype(np.float32)
    if special is not None:
        row, col = n // 2, (d0 + d1) // 3
        if special == "nan":
            x[row, col] = np.nan
        elif special == "inf":
            x[row, col] = np.inf
        else:
            x[row] = 0.0
    x0 = np.ascontiguousarray(x[:, :d0])
    return x0, (np.ascontiguousarray(x[:, d0:]) if d1 else None)


F32_SUM_OVERFLOW = (2.0 - 2.0 ** -24) * 2.0 ** 127  # an fp64 sum of squares from here on rounds to fp32 inf


def check_l2norm(who, y, hi, lo, x0, x1):
    """y (fp32 | None), hi / lo (bf16 bit patterns | None) of one l2norm call against fp64 and torch; prints its figures.
    hi / lo are checked against y, so they need it."""
    x = x0 if x1 is None else np.concatenate([x0, x1], axis=1)
    special = ~np.isfinite(x).all(axis=1)
    with np.errstate(all="ignore"):
        ss = (x.astype(np.float64) ** 2).sum(axis=1)
    over = ss >= F32_SUM_OVERFLOW
    # (the kernel's fp64 sum is 1e-13 relative at worst from this one: no case may sit that close to the limit)
    assert (special | (np.abs(ss / F32_SUM_OVERFLOW - 1.0) > 1e-6)).all(), "sum of squares too near the fp32 limit"
    fp32_rows = special | over
    if y is not None:
        t, r64 = l2norm_torch(x0, x1), l2norm64(x0, x1)
        # where fp32 semantics are the point the reference's own F.normalize decides: a NaN row; zeros and one NaN; zeros
        assert same_with_nan(y[fp32_rows], t[fp32_rows]), who
        # elsewhere: ss is an fp64 sum (1e-13), rounded to fp32 (u); sqrtf halves that and adds its own rounding (1.5u); one
        # division (u): 2.5u, taken as 3u.  A norm below eps divides by eps itself: u.  No output here is subnormal.
        # (observed over the suite, kernel and oracle alike: 1.92 u)
        e = np.abs(y[~fp32_rows].astype(np.float64) - r64[~fp32_rows])
        a = np.abs(r64[~fp32_rows])
        print("%s: y %.2f u of |y| (bound 3 u)" % (who, (e[a > 0] / a[a > 0]).max() / U if (a > 0).any() else 0.0))
        assert (e <= 3 * U * a).all(), who
    if hi is not None or lo is not None:
        ok = np.isfinite(y)
        ay = np.abs(y[ok]).astype(np.float64)
        h = bf16_value(hi).astype(np.float64) if hi is not None else None
        l = bf16_value(lo).astype(np.float64) if lo is not None else None
        if h is not None:
            # hi = bf16_rne(y): 8 significant bits, so half a spacing is 2^-8 |y| at most (2^-134 among bf16 subnormals)
            assert (np.abs(y.astype(np.float64) - h)[ok] <= 2.0 ** -8 * ay + 2.0 ** -134).all(), who
            assert np.array_equal(np.isnan(h), np.isnan(y)), who
        if h is not None and l is not None:
            # lo = bf16_rne(y - hi) with y - hi exact in fp32: |y - hi - lo| <= 2^-8 |y - hi| <= 2^-16 |y|
            # = 1.53e-5 |y| (observed over the suite: 7.6e-6 |y|)
            e = np.abs(y.astype(np.float64) - h - l)[ok]
            print("%s: |y - hi - lo| %.3g of |y| (bound 2^-16 = %.3g)" % (who, (e[ay > 0] / ay[ay > 0]).max() if (ay > 0).any() else 0.0, 2.0 ** -16))
            assert (e <= 2.0 ** -16 * ay + 2.0 ** -134).all(), who


# ---------------------------------------------------------------- exact similarity
# Small-integer operands: every product and every partial sum, in any order and any grouping, is an integer (times 2^-8 in
# the bf16 modes) below 2^24 in magnitude, hence exact in fp32.  The kernel's accumulator must then hold exactly the
# integer, and the result is that integer divided once by fp32(temp), correctly rounded.
EXACT_LIMIT = 2 ** 24


def exact_gemm(mode, nq, nt, d, seed=0, temp=0.1):
    """-> dict: q, t (f32 mode: fp32 [.,d]) or qh, ql, th, tl (bf16 bit patterns, uint16; ql / tl all zero in mode "bf16");
    acc (the exact accumulator as fp64), expect (fp32), bound (sum |terms| in the scaled integer domain).
    f32: entries in [-8, 8].  bf16 / bf16x3: hi planes in [-2, 2], lo planes in [-2, 2] * 2^-8 drawn independently for q and t;
    bf16x3 expects exactly hi*hi + hi*lo + lo*hi (no lo*lo: 2^-16 of an integer would move the result)."""
    r = _rng(nq, nt, d, seed, {"f32": 0, "bf16": 1, "bf16x3": 2}[mode])
    c = dict(mode=mode, temp=temp)
    if mode == "f32":
        q = r.integers(-8, 9, (nq, d)).astype(np.float64)
        t = r.integers(-8, 9, (nt, d)).astype(np.float64)
        acc, scale = q @ t.T, 1.0
        c["bound"] = int((np.abs(q).sum(axis=1).max()) * 8)  # <= 64 d
        c.update(q=q.astype(np.float32), t=t.astype(np.float32))
    else:
        qh, th = r.integers(-2, 3, (nq, d)).astype(np.float64), r.integers(-2, 3, (nt, d)).astype(np.float64)
        ql, tl = r.integers(-2, 3, (nq, d)).astype(np.float64), r.integers(-2, 3, (nt, d)).astype(np.float64)  # units of 2^-8
        if mode == "bf16":
            ql[:], tl[:] = 0.0, 0.0
        acc256 = 256.0 * (qh @ th.T) + qh @ tl.T + ql @ th.T  # the integer, in units of 2^-8
        scale = 2.0 ** -8
        acc = acc256 * scale
        c["bound"] = int(256 * 4 * d + 4 * d + 4 * d) if mode == "bf16x3" else int(256 * 4 * d)
        f = lambda a, s: bf16_bits((a * s).astype(np.float32))
        c.update(qh=f(qh, 1.0), ql=f(ql, scale), th=f(th, 1.0), tl=f(tl, scale))
    # the exactness condition: the sum of |terms| (so every partial sum, in every order) stays below 2^24 integer units
    assert c["bound"] < EXACT_LIMIT, (mode, d, c["bound"])
    a32 = acc.astype(np.float32)
    assert np.array_equal(a32.astype(np.float64), acc)
    c["acc"] = acc
    c["expect"] = a32 / np.float32(temp)  # one IEEE fp32 division
    return c


SIM_F32_V2 = [(1, 1, 4), (128, 128, 16), (129, 127, 20), (130, 257, 2312), (5, 300, 14592)]
SIM_F32_R2_D = [1, 2, 3, 5, 7, 33, 101]
SIM_F32_R2_SHAPE = (37, 130)
SIM_BF16_D = [1, 7, 8, 9, 63, 64, 65, 72]
SIM_BF16_SHAPES = [(129, 127), (127, 130)]
SIM_BF16_LONG = (5, 130, 14592)
SIM_XL_SHAPES = [(1, 256, 256), (300, 256, 288), (257, 512, 8192)]
SIM_BIG_D, SIM_BIG_NT = 16384, 130  # the 4 GiB case: 65536 x 16384 fp32 against 130 rows


def exact_shapes():
    """(mode, d) of every exact_gemm case of the GPU suite, for the host test's check of the exactness condition."""
    out = [("f32", d) for _, _, d in SIM_F32_V2] + [("f32", d) for d in SIM_F32_R2_D] + [("f32", 64), ("f32", SIM_BIG_D)]
    for m in ("bf16", "bf16x3"):
        out += [(m, d) for d in SIM_BF16_D] + [(m, SIM_BF16_LONG[2])]
    return out + [("bf16x3", d) for _, _, d in SIM_XL_SHAPES]


# ---------------------------------------------------------------- row select
def target_order(q, n_seg):
    """validate.py:369-378: the positive pos = min(q + 1, n_seg - 1) first, then every other segment but q, ascending."""
    pos = min(q + 1, n_seg - 1)
    return np.array([pos] + [i for i in range(n_seg) if i != q and i != pos], np.int64)


def row_select_ref(x, xa=None, alpha=0.5, threshold=0.0):
    """validate.py:524-568 for one row, line by line, in torch fp32 on the CPU; x (and xa) already in target order.
    -> dict(idx, p, cnt, row_sum, row_max).  It decides what survives in rows with special values."""
    output = torch.from_numpy(np.array(x, np.float32))
    row_sum = output.sum().item()
    output /= output.sum()  # :524
    if xa is not None:
        output_a = torch.from_numpy(np.array(xa, np.float32))
        output_a /= output_a.sum()  # :526
        output = alpha * output + (1 - alpha) * output_a  # :527
    row_max = output.max().item()
    output[output < (output.max() - threshold * output.max())] = 0.0  # :554
    output[torch.nonzero(output).view(-1)] /= output.sum()  # :558
    choices = output.nonzero().view(-1)  # :568
    return dict(idx=choices.numpy().astype(np.int64), p=output[choices].numpy(), cnt=len(choices), row_sum=row_sum, row_max=row_max)


def row_select64(x, xa=None, alpha=0.5, threshold=0.0):
    """The same in fp64, for ordinary (finite) rows whose survivor set is unambiguous by construction."""
    p = np.asarray(x, np.float32).astype(np.float64)
    row_sum = p.sum()
    p = p / row_sum
    if xa is not None:
        pa = np.asarray(xa, np.float32).astype(np.float64)
        p = float(np.float32(alpha)) * p + (1.0 - float(np.float32(alpha))) * (pa / pa.sum())
    mx = p.max()
    cut = mx - float(np.float32(threshold)) * mx
    p = np.where(p < cut, 0.0, p)
    p = np.where(p != 0.0, p / p.sum(), 0.0)
    idx = np.nonzero(p)[0]
    return dict(idx=idx.astype(np.int64), p=p[idx], cnt=len(idx), row_sum=row_sum, row_max=mx, cut=cut)


def gap_rows(nq, L, seed, survivors=None, m=4.0):
    """Rows for threshold 0.3: survivors in [0.9, 1] m (at `survivors`, a list of positions per row, or 1 + r % 7 random
    ones), the rest in [0.05, 0.5] m.  max p lies in [0.9, 1] m / s, the cut 0.7 max p in [0.63, 0.7] m / s: every
    survivor is 0.2 m / s above it and every other entry 0.13 m / s below, 1e5 times what fp32 rounding can move."""
    r = _rng(nq, L, seed, 2)
    x = (r.random((nq, L)) * 0.45 + 0.05) * m
    for i in range(nq):
        pos = r.choice(L, size=min(L, 1 + i % 7), replace=False) if survivors is None else np.asarray(survivors[i])
        x[i, pos] = (0.9 + 0.1 * r.random(len(pos))) * m
    return x.astype(np.float32)


TR_EDGES = [2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385]
TR_SMALL = [1, 2, 63, 64, 65, 255, 256, 257]
TR_KERNEL_WIDTHS = [65, 2049, 4097, 8193, 16385]  # one width in each of the five kernels row_transition dispatches to
SPECIAL_ROWS = ["nan", "pinf", "ninf", "zero", "cancel", "negsum"]


def special_rows(L):
    """One row per SPECIAL_ROWS kind, [6, L]: special values are ordinary data for the select."""
    x = gap_rows(len(SPECIAL_ROWS), L, 99)
    mid = L // 2
    x[0, mid] = np.nan
    x[1, mid] = np.inf
    x[2, mid] = -np.inf
    x[3] = 0.0
    x[4] = 0.0
    if L >= 2:
        x[4, 0], x[4, 1] = 1.0, -1.0  # [1, -1, 0, ...]: the sum is exactly zero -> p = [inf, -inf, nan, ...]
    x[5] = -x[5]  # a negative sum: p = x / s is positive again (validate.py:524 divides whatever the sign)
    if L >= 8:
        x[5, 3] = 0.25  # ... and one positive score, whose p is negative
    return x


def exact_rows(L):
    """Two rows whose p, cut and renormalised p are known without a reference (L = 2^k >= 8) -> x [2, L].
    Row 0: L entries of 3: s = 3 L and p = 3 / (3 L) = 1 / L exactly; at threshold 0 all survive, s2 = 1, p stays 1 / L.
    Row 1: 4, 2, 1, 1 and L - 4 zeros: s = 8, p = .5, .25, .125, .125, 0, ...  (EXACT_ROW1 lists what survives.)"""
    assert L >= 8 and L & (L - 1) == 0
    x = np.zeros((2, L), np.float32)
    x[0] = 3.0
    x[1, :4] = [4.0, 2.0, 1.0, 1.0]
    return x


_F = np.float32
# threshold -> (survivor positions, their p) of exact_rows' row 1.  cut = .5 - fl(th) * .5 = .35, .2, .1 (each to 1e-8) and
# exactly 0: nowhere near a p.  The zeros are never survivors (nonzero()); at threshold 1 they are not cut either and add
# nothing to s2.  s2 = .5, .75, 1, 1 exactly, so the renormalised p is at most one correctly rounded fp32 division.
EXACT_ROW1 = {
    0.3: ([0], [_F(1.0)]),
    0.6: ([0, 1], [_F(0.5) / _F(0.75), _F(0.25) / _F(0.75)]),
    0.8: ([0, 1, 2, 3], [_F(0.5), _F(0.25), _F(0.125), _F(0.125)]),
    1.0: ([0, 1, 2, 3], [_F(0.5), _F(0.25), _F(0.125), _F(0.125)]),
}


def scatter_rows(rows, q_ids, nt, junk=1e6):
    """Rows given in target order -> the [nq, nt] score matrix avt_row_transition reads with q_ids: row r's entry for
    segment target_order(q)[i] is rows[r][i]; the query's own column (never read, unless q is last) holds `junk`."""
    sim = np.full((len(rows), nt), junk, np.float32)
    for r, q in enumerate(q_ids):
        order = target_order(int(q), nt)
        assert len(rows[r]) == len(order)
        sim[r, order] = rows[r]
    return sim


def perm_q_ids(nt):
    return np.array(sorted({0, 1, nt // 2, nt - 2, nt - 1} & set(range(nt))), np.int64)


def _case(name, sim, kind="gap", q_ids=None, sim_a=None, alpha=0.5, threshold=0.3, cap=16):
    return dict(name=name, sim=np.ascontiguousarray(sim, np.float32), kind=kind, q_ids=q_ids,
                sim_a=None if sim_a is None else np.ascontiguousarray(sim_a, np.float32), alpha=alpha, threshold=threshold, cap=cap)


def _perm_case(nt, seed, **kw):
    q_ids = perm_q_ids(nt)
    lens = [nt if q == nt - 1 else nt - 1 for q in q_ids]
    sim = scatter_rows([gap_rows(1, L, seed + i)[0] for i, L in enumerate(lens)], q_ids, nt)
    return _case("perm nt=%d" % nt, sim, q_ids=q_ids, **kw)


def transition_cases(group):
    """The inputs of one group of row_transition tests: a list of dicts (name, sim, kind, q_ids, sim_a, alpha, threshold,
    cap).  kind "gap": the fp64 survivor set is unambiguous (row_select64 decides); "special": row_select_ref decides."""
    c = []
    if group == "plain":  # both sides of every width at which the launcher changes kernel, and the small rows
        for L in TR_SMALL + TR_EDGES:
            c.append(_case("plain L=%d" % L, gap_rows(3, L, 1)))
    elif group == "perm":  # the same widths as ROW LENGTHS under q_ids: L = nt - 1, or nt for the last query
        for L in TR_EDGES:
            c += [_perm_case(L, 2), _perm_case(L + 1, 3)]
        c += [_perm_case(nt, 4) for nt in (2, 3, 65, 257)]
    elif group == "placement":
        for W in (300, 4100, 16383):  # 256 threads x 8; 1024 x 8; 1024 x 16: the last round of each is ragged
            nthr = 256 if W <= 4096 else 1024
            last = (W - 1) // nthr * nthr  # first position of the last round
            c.append(_case("last round W=%d" % W, gap_rows(2, W, 5, [[W - 1], [last, (last + W) // 2, W - 1]])))
            c.append(_case("one wave W=%d" % W, gap_rows(1, W, 6, [list(range(64, 128))]), cap=80))
            for th in (1.0, 1.5):  # cut = max - th max <= 0 < every p: all survive
                c.append(_case("every entry th=%g W=%d" % (th, W), gap_rows(2, W, 7), threshold=th, cap=W))
            c.append(_case("exactly one W=%d" % W, gap_rows(2, W, 8, [[W // 3], [last + 1]]), threshold=0.0))
            x = gap_rows(2, W, 9, [[5, W - 1], [0, 63, 64, last, W - 1]])
            x[0, [5, W - 1]] = 8.0  # exact ties for the maximum, first and last round; threshold 0 keeps exactly the ties
            x[1, [0, 63, 64, last, W - 1]] = 8.0
            c.append(_case("ties W=%d" % W, x, threshold=0.0))
    elif group == "capacity":
        x = gap_rows(7, 300, 10)  # 1 .. 7 survivors
        c += [_case("cap=1", x, cap=1), _case("cap=0", x, cap=0), _case("cap>L", x, cap=400), _case("cap=3", x, cap=3)]
    elif group == "blend":
        for W in (300, 4100, 16385):
            pos = [[1, W // 2], [W - 1], [0, 64, W - 2]]
            for alpha in (0.0, 1.0, 0.5):
                c.append(_case("blend alpha=%g W=%d" % (alpha, W), gap_rows(3, W, 11, pos), sim_a=gap_rows(3, W, 12, pos, m=0.7), alpha=alpha))
        q_ids = perm_q_ids(301)
        lens = [301 if q == 300 else 300 for q in q_ids]
        rows = lambda seed, m: [gap_rows(1, L, seed, [[0, L // 2]], m=m)[0] for L in lens]
        c.append(_case("blend perm", scatter_rows(rows(13, 4.0), q_ids, 301), q_ids=q_ids, sim_a=scatter_rows(rows(14, 0.3), q_ids, 301)))
    elif group == "special":
        for L in TR_KERNEL_WIDTHS:
            c.append(_case("special L=%d" % L, special_rows(L), kind="special", cap=L))
        c.append(_case("special L=2", special_rows(2), kind="special", cap=2))
    elif group == "exact":
        for L in (8, 256, 4096, 16384):
            x = exact_rows(L)
            c.append(_case("exact th=0 L=%d" % L, x[:1], kind="exact", threshold=0.0, cap=L))
            for th in EXACT_ROW1:
                c.append(_case("exact th=%g L=%d" % (th, L), x[1:], kind="exact", threshold=th, cap=8))
    else:
        raise KeyError(group)
    return c


TR_GROUPS = ["plain", "perm", "placement", "capacity", "blend", "special", "exact"]

# Error of the survivors' p against fp64, in units of |p| (all survivors of the "gap" rows are positive):
#   sf = fl(s): u.  p = fl(x / sf): 2u.  s2 = fl(sum of survivors' p), an fp64 sum of positive terms each 2u off,
#   rounded once: 3u.  pn = fl(p / s2f): 2u + 3u + u = 6u (+ O(u^2): the .01).
#   With the audio blend p = fl(fl(af p) + fl(bf pa)), af, bf >= 0 exact for alpha in {0, .5, 1}: 2u + u + u = 4u; s2: 5u;
#   pn: 4u + 5u + u = 10u.
# These are worst cases; the errors mostly cancel.  Observed over every case of the suite, kernel and oracle alike (the
# tests print them): p 2.12 u (1.82 u blended), row_sum 0.92 u of its 1 u bound, row_max 1.59 u of its 2 u (4 u blended) bound.
P_BOUND, P_BOUND_BLEND = 6.01 * U, 10.01 * U


def check_select(out, case, who):
    """out (dict of numpy arrays idx / seg / p [nq, cap], cnt [nq], stats [nq, 4], any of them None) against the
    references; prints the figures it asserts on."""
    sim, q_ids, cap = case["sim"], case["q_ids"], case["cap"]
    nq, nt = sim.shape
    worst_p = worst_s = worst_m = 0.0
    blend = case["sim_a"] is not None
    pb = P_BOUND_BLEND if blend else P_BOUND
    for r in range(nq):
        order = np.arange(nt) if q_ids is None else target_order(int(q_ids[r]), nt)
        x = sim[r, order]
        xa = case["sim_a"][r, order] if blend else None
        with np.errstate(all="ignore"):
            ref = (row_select_ref if case["kind"] == "special" else row_select64)(x, xa, case["alpha"], case["threshold"])
        what = "%s: %s row %d" % (who, case["name"], r)
        if out["cnt"] is not None:
            assert out["cnt"][r] == ref["cnt"], (what, int(out["cnt"][r]), ref["cnt"])
        k = min(ref["cnt"], cap)
        if out["idx"] is not None:
            assert np.array_equal(out["idx"][r, :k], ref["idx"][:k]), what
        if out["seg"] is not None:
            assert np.array_equal(out["seg"][r, :k], order[ref["idx"][:k]]), what
        st = None if out["stats"] is None else out["stats"][r].astype(np.float64)
        if case["kind"] == "special":
            if out["p"] is not None:
                assert np.array_equal(np.isnan(out["p"][r, :k]), np.isnan(ref["p"][:k])), what
            if st is not None:
                assert np.isnan(st[1]) == np.isnan(ref["row_max"]), (what, st[1], ref["row_max"])
                assert np.isnan(st[0]) == np.isnan(ref["row_sum"]), (what, st[0], ref["row_sum"])
            if not np.isfinite(x).all() or not np.isfinite(ref["p"]).all():
                continue
            ref = row_select64(x, xa, case["alpha"], case["threshold"])  # a finite special row (the negative sum): fp64 too
            assert ref["cnt"] == (out["cnt"][r] if out["cnt"] is not None else ref["cnt"]), what
        if out["p"] is not None and k:
            e = np.abs(out["p"][r, :k].astype(np.float64) - ref["p"][:k]) / np.abs(ref["p"][:k])
            worst_p = max(worst_p, e.max())
            assert (e <= pb).all(), (what, e.max() / U)
        if st is not None:
            es = abs(st[0] - ref["row_sum"]) / abs(ref["row_sum"])  # an fp64 sum rounded once: u
            em = abs(st[1] - ref["row_max"]) / abs(ref["row_max"])  # p before the renormalisation: 2u (4u blended)
            worst_s, worst_m = max(worst_s, es), max(worst_m, em)
            assert es <= 1.01 * U and em <= (4.01 if blend else 2.01) * U, (what, es / U, em / U)
    print("%s: %s  p %.2f u (bound %.2f u)  row_sum %.2f u (1 u)  row_max %.2f u (%d u)"
          % (who, case["name"], worst_p / U, pb / U, worst_s / U, worst_m / U, 4 if blend else 2))


def check_exact_rows(run):
    """run(x, threshold, cap) -> dict(idx, p, cnt, stats) as numpy: the rows of exact_rows, whose every output is known
    without a reference, bit for bit."""
    for L in (8, 256, 4096, 16384):
        x = exact_rows(L)
        o = run(x[:1], 0.0, L)
        assert o["cnt"][0] == L and (o["p"][0] == np.float32(1.0 / L)).all() and o["idx"][0].tolist() == list(range(L)), L
        assert o["stats"][0, 0] == 3 * L and o["stats"][0, 1] == np.float32(1.0 / L), L
        for th, (idx, p) in EXACT_ROW1.items():
            o = run(x[1:], th, 8)
            k = len(idx)
            assert o["cnt"][0] == k and o["idx"][0, :k].tolist() == idx, (L, th)
            assert np.array_equal(o["p"][0, :k], np.array(p, np.float32)), (L, th, o["p"][0, :k])
            assert o["stats"][0, 0] == 8 and o["stats"][0, 1] == 0.5, (L, th)
        print("exact rows L=%d: p = 1/L, and 4 2 1 1 at thresholds %s, bit for bit" % (L, sorted(EXACT_ROW1)))


# ---------------------------------------------------------------- top-k
def topk_ref(x, k, self_col=None):
    """Per row: the k largest non-NaN, non-excluded entries by (value descending, column ascending), padded with index -1 /
    value -inf.  -> (idx int32 [nq, k], val fp32 [nq, k])."""
    x = np.asarray(x, np.float32)
    nq, nt = x.shape
    idx = np.full((nq, k), -1, np.int32)
    val = np.full((nq, k), -np.inf, np.float32)
    for r in range(nq):
        cols = np.arange(nt)
        ok = ~np.isnan(x[r])
        if self_col is not None and 0 <= self_col[r] < nt:
            ok[self_col[r]] = False
        cols = cols[ok]
        v = x[r, cols]
        order = np.lexsort((cols, -v.astype(np.float64)))[:k]  # last key first: -value ascending, then column ascending
        idx[r, : len(order)] = cols[order]
        val[r, : len(order)] = v[order]
    return idx, val


TOPK_WIDTHS = [1, 2, 255, 256, 257, 4095, 4096, 4097, 16383, 16384]


def topk_input(nt):
    """-> (x [7, nt], self_col [7]).  Rows: random; ties across lanes, waves and the 1024-thread form's rounds (self column 0);
    all -inf (self column nt - 1); NaNs at column 0, the middle and the last; all NaN; random with self column nt - 1; a tie
    of EVERY entry."""
    r = _rng(nt, 3)
    x = r.standard_normal((7, nt)).astype(np.float32)
    self_col = np.full(7, -1, np.int64)
    for c in (0, 1, 63, 64, 65, 255, 256, 1023, 1024, 1025, 4095, 4096, nt - 2, nt - 1):
        if 0 <= c < nt:
            x[1, c] = 5.0
    self_col[1] = 0
    x[2] = -np.inf
    self_col[2] = nt - 1
    x[3, [0, nt // 2, nt - 1]] = np.nan
    x[4] = np.nan
    self_col[5] = nt - 1
    x[6] = 1.5
    return x, self_col
