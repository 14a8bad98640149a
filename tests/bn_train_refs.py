"""fp64 references, error magnitudes, a numpy model of the kernels' own arithmetic and the input families for the training
BatchNorm (csrc/bn_train.hip) — shared by tests/test_gpu_bn_train_edges.py (the kernels on the device) and
tests/test_bn_train_refs_host.py (the references and the bounds themselves, on the CPU).  Plain numpy, no torch, no HIP.

Rows are [M, C] fp32, `groups` equal consecutive slabs with statistics of their own.  u = 2^-24 (half an fp32 ulp, relative).

BOUNDS (report()).  Every one is a count of roundings times u times a magnitude; nothing here was fitted to a result.
  save_mean     1 fp32 ulp of float32(mean64): the kernel's mean is a correctly rounded fp64 quotient of an fp64 sum whose own
                error (k 2^-53 |x|) is far below the cast's.
  save_invstd   relative u + 1/2 k 2^-53 E[x^2] / (var + eps): the cast, and the single-pass variance E[x^2] - mean^2 whose two
                terms each carry k 2^-53 of their size from a chain of k fp64 additions (chain_depth()).
  y             8 u ((|x - mean| + |mean|) |invstd gamma| + |beta| + |res|): mean, subtract, invstd, scale product, multiply,
                add beta, add res, and the reference's own cast.  ReLU is 1-Lipschitz: no element is left out.
  y_apply       6 u (|x - mean| |invstd gamma| + |beta| + |res|) against fp64 evaluated FROM THE KERNEL'S OWN save_mean /
                save_invstd: subtract, scale product, multiply, add beta, add res, the cast.  The bound above has to charge
                u |mean| |invstd gamma| for the rounding of save_mean itself, and the folded form x * sc + (beta - mean * sc)
                loses the same order (three roundings of size |mean| |sc|): it cannot be told from the right form there.
                Given the saved statistics — which the two checks above hold to fp64 — the right form has no term in |mean|.
  dres          exact: the masked dy.
  dbeta         u |dbeta| + 64 2^-53 sum|g|: one cast of an fp64 sum of floats.
  dgamma        (5 u + d) sum|g| (|x - mean| + |mean|) invstd: xhat = (x - mu) * is carries mean, subtract, invstd, product;
                g * xhat is exact in fp64; the cast.  d = save_invstd's second term.
  dx            13 u |gamma invstd| (|g| + |k0| + (|x - mean| + |mean|) invstd |k1|) + 4 u |gamma invstd| |xhat| A1,
                A1 = sum|g| (|x - mean| + |mean|) invstd / M (dgamma's magnitude over the group's rows).  First term: xhat 4,
                k1's cast 1, xhat * k1 1, k0's cast 1, the two subtractions 2, gamma * invstd 2, the last product 1, the
                reference's cast 1.  Second term: k1 = float(s1 / M) inherits xhat's four roundings THROUGH THE SUM, where they
                are of the size of sum|g xhat|, not of |sum g xhat|: where s1 cancels (on the integer family often to exactly
                0) a bound in |k1| alone is missed by the kernel's model itself.  With k0 / k1 given (avt_bn_train_bwd_pre:
                the producer's sums, exact on the integer family) the second term is not there.
  running_*     2 fp32 ulp of running_ref() on the kernel's own save_mean and the fp64 variance: float(unbiased var) may fall
                on either side of a rounding boundary, and one more operation follows it.
"""
import numpy as np

U = 2.0 ** -24
KT = 256          # threads per workgroup
KMAX_BLOCKS = 1024
KPRE_ROWS = 64    # rows one pre-reduce workgroup sums
F32, F64 = np.float32, np.float64
FAULTS = ("folded", "fp32_sums", "biased_running_var", "wrong_group_running", "mask_ge", "eps_double")
# eps per family: torch's default, and on the degenerate family (whose constant channels have invstd = 1 / sqrt(eps) exactly) a
# value whose fp32 rounding SHOWS: float32(1 / sqrt(0.0085)) is more than u away from 1 / sqrt(float32(0.0085)).  Of the values
# k * 10^-e with k < 100 this is the only one: eps and float32(eps) differ by at most u, invstd by half of that.
EPS = {"plain": 1e-5, "offset": 1e-5, "integer": 1e-5, "degenerate": 0.0085}
MOMENTUM = 0.1


# ---------------------------------------------------------------- geometry (bn_train.hip: layout(), ws_bytes())
def nq_unit(c):
    q = c // 4
    return min(q, KT), max(q // KT, 1)


def layout_blocks(m, c, groups):
    """Workgroups per group for m rows IN ALL: layout() restated (the host test holds it to blocks_of where the library loads)."""
    nq, unit = nq_unit(c)
    mg = m // groups
    nchunk = mg * (c // 4)
    blocks = (nchunk + KT - 1) // KT
    most = max(2 * KMAX_BLOCKS // groups, 128) if groups > 1 else KMAX_BLOCKS
    blocks = min(blocks, most)
    cap = max(mg // 64 + 1, 128 if groups > 1 else 512)
    blocks = min(blocks, cap)
    return -(-blocks // unit) * unit


def blocks_of(m, c, groups):
    """Workgroups per group for m rows in all, from the library: avt_bn_train_ws_bytes = groups (blocks nq 64 + 8 C)."""
    from avtex import _lib
    ws = int(_lib.lib().avt_bn_train_ws_bytes(m, c, groups))
    nq, _ = nq_unit(c)
    assert ws > 0 and ws % groups == 0, (m, c, groups, ws)
    blocks, rem = divmod(ws // groups - 8 * c, nq * 64)
    assert rem == 0 and blocks > 0, (m, c, groups, ws)
    return blocks


def sweeps(m, c, groups, blocks):
    """Most chunks one thread of the statistics pass adds up (ceil: a ragged last sweep counts)."""
    nchunk = (m // groups) * (c // 4)
    return -(-nchunk // (blocks * KT))


def chain_depth(m, c, groups, blocks):
    """k: the longest chain of fp64 additions behind one channel's sum — the sweeps of one thread, 8 tree levels at the most,
    a finalize lane's walk over the rows of partials, 6 shuffles, and the 3 operations that make the variance."""
    return sweeps(m, c, groups, blocks) + 8 + -(-blocks // 64) + 6 + 3


# ---------------------------------------------------------------- input families
def family(name, m, c, groups, seed=0):
    """-> x [groups * m, c] fp32, gamma [c], beta [c].  Every channel has statistics of its own; group g carries an offset of g."""
    rng = np.random.default_rng([seed, m, c, groups, sum(map(ord, name))])
    ch = np.arange(c)
    gamma = (0.5 + (ch % 7) / 6.0) * np.where(ch % 5 == 4, -1.0, 1.0)
    beta = np.linspace(-0.3, 0.3, c)
    goff = np.repeat(np.arange(groups, dtype=F64), m)[:, None]
    rows = groups * m
    if name == "plain":
        x = rng.standard_normal((rows, c)) * (2.0 + 0.25 * (ch % 4)) + 0.7 + 0.1 * (ch % 7) + goff
    elif name == "offset":  # |mean| / std = 1500 at the least
        # (deviations of 0.015 .. 0.025 with alternating signs, not normal ones: three normal rows can fall within 0.001 of each
        #  other, and the variance's cancellation term — kept below u / 10 on this family — would be that channel's, not the family's)
        sign = np.where((np.arange(rows)[:, None] + rng.integers(0, 2, size=c)) % 2 == 0, 1.0, -1.0)
        x = sign * 0.02 * (0.75 + 0.5 * rng.random((rows, c))) + np.where(ch % 2 == 0, 1.0, -1.0) * (30.0 + goff)  # (the group's offset away from 0)
    elif name == "integer":
        x = rng.integers(-8 + ch % 4, 9 - ch % 3, size=(rows, c)).astype(F64) + goff
        gamma, beta = np.round(gamma * 4) / 4, np.round(beta * 8) / 8
    elif name == "degenerate":
        x = rng.standard_normal((rows, c)) * 1.5 + 0.3
        half = m // 2
        for g in range(groups):
            s = slice(g * m, (g + 1) * m)
            for k in ch:
                kind = k % 8
                if kind == 0:
                    x[s, k] = 0.0
                elif kind == 1:
                    x[s, k] = 3.0
                elif kind in (2, 3):  # v and -v in pairs (a 0 in the middle of an odd count): the mean is exactly 0
                    v = rng.choice(np.array([0.0, 0.0, 2.0 ** -20, 0.5, 1.0]), size=half)
                    col = np.concatenate([v, -v, np.zeros(m - 2 * half)])
                    x[s, k] = rng.permutation(col)
                elif kind == 4:  # a single non-zero row
                    x[s, k] = 0.0
                    x[g * m + int(rng.integers(0, m)), k] = 5.0
        x = x + goff
        flat = np.isin(ch % 8, (0, 2, 3))
        gamma, beta = np.where(flat, 1.0, gamma), np.where(flat, 0.0, beta)
    else:
        raise KeyError(name)
    return x.astype(F32), gamma.astype(F32), beta.astype(F32)


def aux(name, m, c, groups, seed=0):
    """-> res, dy [groups * m, c] fp32 and the running statistics the call starts from (integers on the integer family)."""
    rng = np.random.default_rng([seed + 1, m, c, groups, sum(map(ord, name))])
    rows = groups * m
    if name == "integer":
        res, dy = rng.integers(-4, 5, size=(rows, c)), rng.integers(-6, 7, size=(rows, c))
    else:
        res, dy = rng.standard_normal((rows, c)), rng.standard_normal((rows, c))
    ch = np.arange(c)
    return res.astype(F32), dy.astype(F32), (0.25 + 0.125 * (ch % 3)).astype(F32), (2.0 - 0.25 * (ch % 5)).astype(F32)


# ---------------------------------------------------------------- fp64 references
def _g3(a, groups):
    a = np.asarray(a)
    return a.reshape(groups, a.shape[0] // groups, a.shape[1])


def fwd_ref(x, res, gamma, beta, eps, relu, groups):
    """fp64 forward -> dict: mean, var (biased), invstd [groups, C]; y [M, C]; ex2 = E[x^2] [groups, C]; mag_y [M, C]."""
    x3 = _g3(x, groups).astype(F64)
    mean = x3.mean(axis=1)
    mean = mean + (x3 - mean[:, None]).mean(axis=1)  # (second pass of the mean: what fp64 left of the first)
    d = x3 - mean[:, None]
    var = (d * d).mean(axis=1)
    invstd = 1.0 / np.sqrt(var + F64(F32(eps)))
    sc = invstd * np.asarray(gamma, F64)
    y = d * sc[:, None] + np.asarray(beta, F64)
    mag = (np.abs(d) + np.abs(mean)[:, None]) * np.abs(sc)[:, None] + np.abs(np.asarray(beta, F64))
    if res is not None:
        r3 = _g3(res, groups).astype(F64)
        y, mag = y + r3, mag + np.abs(r3)
    if relu:
        y = np.maximum(y, 0.0)
    shape = np.asarray(x).shape
    return {"mean": mean, "var": var, "invstd": invstd, "y": y.reshape(shape), "mag_y": mag.reshape(shape), "ex2": (x3 * x3).mean(axis=1)}


def apply_ref(x, res, gamma, beta, mean32, invstd32, relu, groups):
    """fp64 y from GIVEN fp32 statistics [groups, C] (the kernel's saved ones) -> y, magnitude (no |mean| term: see y_apply)."""
    d = _g3(x, groups).astype(F64) - np.asarray(mean32, F32).astype(F64).reshape(groups, 1, -1)
    sc = np.asarray(invstd32, F32).astype(F64).reshape(groups, 1, -1) * np.asarray(gamma, F64)
    y = d * sc + np.asarray(beta, F64)
    mag = np.abs(d * sc) + np.abs(np.asarray(beta, F64))
    if res is not None:
        r3 = _g3(res, groups).astype(F64)
        y, mag = y + r3, mag + np.abs(r3)
    if relu:
        y = np.maximum(y, 0.0)
    shape = np.asarray(x).shape
    return y.reshape(shape), mag.reshape(shape)


def running_ref(rm, rv, mean, var, M, momentum):
    """bn_fwd_finalize_kernel's fp32 expression in numpy float32: GROUP 0's statistics only ([groups, C] or [C] inputs), the
    unbiased variance when there is more than one row.  mean: what the kernel saved (cast to fp32 here); var: fp64, biased."""
    mean, var = np.asarray(mean), np.asarray(var, F64)
    mean, var = (mean[0], var[0]) if mean.ndim == 2 else (mean, var)
    m = F32(momentum)
    unb = var * F64(M) / F64(M - 1) if M > 1 else var
    one = F32(1.0) - m
    return one * np.asarray(rm, F32) + m * mean.astype(F32), one * np.asarray(rv, F32) + m * unb.astype(F32)


def bwd_ref(dy, x, mask, gamma, mean, invstd, groups, k0=None, k1=None):
    """fp64 backward for a GIVEN mask ([M, C] bool, or None: no ReLU); mean / invstd [groups, C] fp64.  k0 / k1 [groups, C]
    given: dx from those means of g and g xhat (avt_bn_train_bwd_pre's contract) instead of the ones summed here.
    -> dict: dx, dres [M, C]; dgamma, dbeta [C]; mag_dx, mag_k1 [M, C] (the two terms of dx's bound); mag_dgamma, mag_dbeta [C]."""
    g = _g3(dy, groups).astype(F64)
    if mask is not None:
        g = np.where(_g3(mask, groups), g, 0.0)
    M = g.shape[1]
    d = _g3(x, groups).astype(F64) - np.asarray(mean, F64)[:, None]
    is_ = np.asarray(invstd, F64)[:, None]
    xhat = d * is_
    s0, s1 = g.sum(axis=1), (g * xhat).sum(axis=1)
    given = k1
    k0 = s0 / M if k0 is None else np.asarray(k0, F64)
    k1 = s1 / M if k1 is None else np.asarray(k1, F64)
    gi = np.asarray(gamma, F64) * is_
    size = (np.abs(d) + np.abs(np.asarray(mean, F64))[:, None]) * is_
    dx = gi * (g - k0[:, None] - xhat * k1[:, None])
    mag_dx = np.abs(gi) * (np.abs(g) + np.abs(k0)[:, None] + size * np.abs(k1)[:, None])
    mag_k1 = np.abs(gi * xhat) * ((np.abs(g) * size).sum(axis=1) / M)[:, None] if given is None else np.zeros_like(mag_dx)
    shape = np.asarray(x).shape
    return {"dx": dx.reshape(shape), "dres": g.reshape(shape), "dgamma": s1.sum(axis=0), "dbeta": s0.sum(axis=0),
            "mag_dx": mag_dx.reshape(shape), "mag_k1": mag_k1.reshape(shape), "mag_dgamma": (np.abs(g) * size).sum(axis=(0, 1)), "mag_dbeta": np.abs(g).sum(axis=(0, 1))}


# ---------------------------------------------------------------- the kernels' own arithmetic, in numpy
def _sum_rows(a):
    """[G, M, C] fp64 -> [G, C]: the rows summed last to first, PAIRWISE (numpy's sum along a contiguous axis): a chain about as
    deep as the kernel's thread / tree / lane walk, in another order.  (A plain running sum over 262145 rows is a chain ten
    thousand times deeper than the kernel's: on the offset family it misses the variance's bound, which the kernel does not.)"""
    return np.ascontiguousarray(a.transpose(0, 2, 1)[..., ::-1]).sum(axis=-1)


def kernel_model(x, res, gamma, beta, eps, relu, groups, momentum, rm, rv, dy, fault=None):
    """What bn_train.hip computes, operation by operation in float32 — except the sums, which are single-pass fp64 sums of x and
    (double)x * x as in the kernel but taken pairwise from the last row to the first (the kernel's order is its own business; its
    sums are held to bounds that no fp64 chain of its depth can miss).  fault: one of FAULTS, switched in alone.  -> dict of fp32 outputs."""
    assert fault is None or fault in FAULTS
    x3 = _g3(np.asarray(x, F32), groups)
    G, M, C = x3.shape
    gamma, beta = np.asarray(gamma, F32), np.asarray(beta, F32)
    if fault == "fp32_sums":
        s0 = np.add.reduce(x3, axis=1, dtype=F32).astype(F64)
        s1 = np.add.reduce(x3 * x3, axis=1, dtype=F32).astype(F64)
    else:
        r = x3.astype(F64)
        s0, s1 = _sum_rows(r), _sum_rows(r * r)
    mean = s0 / F64(M)
    var = np.maximum(s1 / F64(M) - mean * mean, 0.0)
    epsk = F64(eps) if fault == "eps_double" else F64(F32(eps))
    invstd = (1.0 / np.sqrt(var + epsk)).astype(F32)
    mu = mean.astype(F32)
    sc = invstd * gamma
    if fault == "folded":
        o = x3 * sc[:, None] + (beta - mu * sc)[:, None]
    else:
        o = (x3 - mu[:, None]) * sc[:, None] + beta
    if res is not None:
        o = o + _g3(np.asarray(res, F32), groups)
    mask = (o >= 0) if fault == "mask_ge" else (o > 0)
    y = np.maximum(o, F32(0)) if relu else o
    gr = G - 1 if fault == "wrong_group_running" else 0
    unb = var[gr] * F64(M) / F64(M - 1) if (M > 1 and fault != "biased_running_var") else var[gr]
    m32 = F32(momentum)
    out = {"save_mean": mu, "save_invstd": invstd, "y": y.reshape(G * M, C), "mask": mask.reshape(G * M, C),
           "running_mean": (F32(1) - m32) * np.asarray(rm, F32) + m32 * mu[gr],
           "running_var": (F32(1) - m32) * np.asarray(rv, F32) + m32 * unb.astype(F32)}
    if dy is not None:
        g = _g3(np.asarray(dy, F32), groups)
        if relu:
            g = np.where(mask, g, F32(0))
        t = (x3 - mu[:, None]) * invstd[:, None]
        p0 = _sum_rows(g.astype(F64))
        p1 = _sum_rows(g.astype(F64) * t.astype(F64))
        k0, k1 = (p0 / F64(M)).astype(F32), (p1 / F64(M)).astype(F32)
        dx = (gamma * invstd)[:, None] * (g - k0[:, None] - t * k1[:, None])
        out.update(dx=dx.reshape(G * M, C), dres=g.reshape(G * M, C), dbeta=np.cumsum(p0, axis=0)[-1].astype(F32),
                   dgamma=np.cumsum(p1, axis=0)[-1].astype(F32))
    assert all(v.dtype in (F32, np.bool_) for v in out.values()), {k: v.dtype for k, v in out.items()}
    return out


# ---------------------------------------------------------------- the bounds
def _ratio(err, bound):
    """Worst err / bound; 0 / 0 counts as 0 (an exact result held to an exact bound), anything over 0 as inf."""
    err, bound = np.asarray(err, F64), np.broadcast_to(np.asarray(bound, F64), np.shape(err))
    if not np.all(np.isfinite(err)):
        return float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


def ulp32(ref):
    return np.spacing(np.abs(np.asarray(ref, F64).astype(F32))).astype(F64)


def invstd_slack(ref, eps, k):
    """[groups, C]: save_invstd's second term, 1/2 k 2^-53 E[x^2] / (var + eps)."""
    return 0.5 * k * 2.0 ** -53 * ref["ex2"] / (ref["var"] + F64(F32(eps)))


def dx_bound(b):
    return 13 * U * b["mag_dx"] + 4 * U * b["mag_k1"]


def report(out, x, res, gamma, beta, eps, relu, groups, momentum, rm, rv, dy, k):
    """Every output in `out` (kernel_model's dict, or the same names from the device; fp32 numpy) against fp64 -> {name: worst
    error / bound}.  A value <= 1 passes.  The backward's mask is out["y"] > 0, the forward's own output."""
    M = np.asarray(x).shape[0] // groups
    ref = fwd_ref(x, res, gamma, beta, eps, relu, groups)
    slack = invstd_slack(ref, eps, k)
    r = {}
    got = {n: np.asarray(v).astype(F64) for n, v in out.items() if n != "mask"}
    C = np.asarray(x).shape[1]
    r["save_mean"] = _ratio(np.abs(got["save_mean"].reshape(groups, C) - ref["mean"].astype(F32).astype(F64)), ulp32(ref["mean"]))
    r["save_invstd"] = _ratio(np.abs(got["save_invstd"].reshape(groups, C) - ref["invstd"]) / ref["invstd"], U + slack)
    r["y"] = _ratio(np.abs(got["y"] - ref["y"]), 8 * U * ref["mag_y"])
    ya, maga = apply_ref(x, res, gamma, beta, out["save_mean"], out["save_invstd"], relu, groups)
    r["y_apply"] = _ratio(np.abs(got["y"] - ya), 6 * U * maga)
    if "running_mean" in out:
        em, ev = running_ref(rm, rv, np.asarray(out["save_mean"]).reshape(groups, C), ref["var"], M, momentum)
        r["running_mean"] = _ratio(np.abs(got["running_mean"] - em.astype(F64)), 2 * ulp32(em))
        r["running_var"] = _ratio(np.abs(got["running_var"] - ev.astype(F64)), 2 * ulp32(ev))
    if dy is not None and "dx" in out:
        mask = (np.asarray(out["y"]) > 0) if relu else None
        b = bwd_ref(dy, x, mask, gamma, ref["mean"], ref["invstd"], groups)
        if "dres" in out and out["dres"] is not None:
            r["dres"] = 0.0 if np.array_equal(np.asarray(out["dres"], F32), b["dres"].astype(F32)) else float("inf")
        r["dx"] = _ratio(np.abs(got["dx"] - b["dx"]), dx_bound(b))
        r["dgamma"] = _ratio(np.abs(got["dgamma"] - b["dgamma"]), (5 * U + slack.max(axis=0)) * b["mag_dgamma"])
        r["dbeta"] = _ratio(np.abs(got["dbeta"] - b["dbeta"]), U * np.abs(b["dbeta"]) + 64 * 2.0 ** -53 * b["mag_dbeta"])
    return r


# ---------------------------------------------------------------- producer partial rows for the *_pre entries
def partial_rows(sum0, sum1, C, pre_rows, rng):
    """Per-group, per-channel INTEGER totals [groups, C] -> [groups, pre_rows, nq * 8] doubles in channel_sums' layout: a row
    holds nq = min(C / 4, 256) quads, slot (quad % nq) * 8 + e the first sum of channel 4 quad + e and slot + 4 the second;
    with unit = C / 1024 > 1 row b holds quads (b % unit) * 256 ... only.  Every total is split at random into integers over
    the pre_rows / unit rows that hold its channel (all far below 2^53: any order of additions gives the total back)."""
    sum0, sum1 = np.asarray(sum0, F64), np.asarray(sum1, F64)
    groups = sum0.shape[0]
    nq, unit = nq_unit(C)
    assert pre_rows % unit == 0 and np.all(sum0 == np.rint(sum0)) and np.all(sum1 == np.rint(sum1))
    per = pre_rows // unit
    out = np.zeros((groups, pre_rows, nq * 8), F64)
    for which, tot in ((0, sum0), (4, sum1)):
        parts = rng.integers(-4096, 4097, size=(groups, per, C)).astype(F64)
        parts[:, -1, :] = tot - parts[:, :-1, :].sum(axis=1)
        for u in range(unit):  # rows u, u + unit, ...: quads u * 256 .. u * 256 + nq - 1
            ch = parts[:, :, u * nq * 4:(u + 1) * nq * 4].reshape(groups, per, nq, 4)
            view = out[:, u::unit, :].reshape(groups, per, nq, 8)
            view[..., which:which + 4] = ch
            out[:, u::unit, :] = view.reshape(groups, per, nq * 8)
    return out


def unpack_partial_rows(rows, C):
    """Sum of partial_rows' rows per slot -> (sum0, sum1) [groups, C] (the walk of channel_sums, in numpy)."""
    nq, unit = nq_unit(C)
    groups = rows.shape[0]
    s = [np.zeros((groups, C), F64), np.zeros((groups, C), F64)]
    for u in range(unit):
        t = rows[:, u::unit, :].sum(axis=1).reshape(groups, nq, 8)
        for w in (0, 1):
            s[w][:, u * nq * 4:(u + 1) * nq * 4] = t[..., 4 * w:4 * w + 4].reshape(groups, nq * 4)
    return s[0], s[1]


def pack_mask(y, C):
    """[M, C] -> the ReLU mask bytes of bn_fwd_apply_kernel: byte i is chunk i (row i / (C/4), quad i % (C/4)), bit e channel 4 quad + e."""
    b = (np.asarray(y) > 0).reshape(-1, 4).astype(np.uint8)
    return (b[:, 0] | (b[:, 1] << 1) | (b[:, 2] << 2) | (b[:, 3] << 3)).astype(np.uint8)


# ---------------------------------------------------------------- the cases of the fp64 comparison (GPU test; the host test reads them too)
# (rows per group, C, groups, what the shape is there for, workgroups per group, sweeps)
SHAPES = [
    (1, 8, 1, "fewer chunks than threads: one row", 1, 1),
    (5, 8, 1, "fewer chunks than threads", 1, 1),
    (127, 8, 1, "one workgroup, two idle threads", 1, 1),
    (128, 8, 1, "one workgroup exactly; the halving tree down to nq = 2", 1, 1),
    (129, 8, 1, "a second workgroup of two chunks", 2, 1),
    (3, 1024, 1, "nq = 256: the tree loop does not run", 3, 1),
    (33, 2048, 1, "unit 2, 66 workgroups: a second trip of the finalize lanes, first = quad / 256", 66, 1),
    (17, 4096, 1, "unit 4, 68 workgroups", 68, 1),
]
SWEEPS = [
    (16384, 8, 16, "one sweep exactly", 128, 1),
    (32768, 8, 16, "two sweeps: the paired loop runs, the tail does not", 128, 2),
    (32769, 8, 16, "two sweeps and two chunks", 128, 3),
    (49152, 8, 16, "three sweeps: pair and tail for every thread", 128, 3),
    (262145, 8, 1, "one group, 1024 workgroups, two sweeps and two chunks", 1024, 3),
]
GROUP_COUNTS = (1, 7, 8, 9, 16, 17)  # one ragged trip, one full trip of kGroupBatch, a second trip of 1 / 8 / 9 groups
GROUP_ROWS = 12
GROUP_OFFSET_CASES = [(GROUP_ROWS, 32, 9), (GROUP_ROWS, 2048, 9)]  # the offset family through the second trip, against fp64


def fp64_cases():
    """(family, rows per group, C, groups, res, relu) of the comparison with fp64: every family x shortcut x ReLU at layout()'s
    edges, one setting at the sweep counts (16 groups of the offset family would put |mean| at 45: its variance's
    cancellation term would pass u / 10, which is not what that family is for)."""
    out = [(fam, m, c, g, res, relu) for (m, c, g, _, _, _) in SHAPES for fam in ("plain", "offset", "degenerate")
           for res in (False, True) for relu in (False, True)]
    out += [("plain" if g > 1 else "offset", m, c, g, True, True) for (m, c, g, _, _, _) in SWEEPS]
    out += [("degenerate", SWEEPS[2][0], 8, 16, False, True)]
    return out
