"""Inputs and references of the wide classic-baseline kernels (csrc/classic_wide.hip) for tests/test_gpu_classic_wide.py,
proved on the CPU by tests/test_classic_wide_refs_host.py.  Plain numpy / torch, no HIP.  The sweep reference is
loss_classic_refs.q_learning_ref; everything computed here is computed once and shared (treat results as read-only)."""
import numpy as np
import torch

import loss_classic_refs as R

# ---------------------------------------------------------------- future-cost sweeps
Q_FAST_SEEDS = {201: 9202, 256: 9256, 257: 9257, 1025: 10025, 4097: 13098}
Q_SLOW_SEEDS = {201: 9703, 257: 9757}
Q_SLOW_TOL = 10e-3  # the baseline's own tolerance
# (input, n, alpha, tol, max_iter) -> sweeps of q_learning_ref, run on the CPU
Q_WIDE_SWEEPS = {("fast", n, a, R.Q_TOL, 1000): s for n in (201, 256, 257, 1025) for a, s in ((0.5, 2), (0.997, 5))}
Q_WIDE_SWEEPS[("fast", 4097, 0.5, R.Q_TOL, 1000)] = 2  # (one alpha: 17 M elements a sweep on the CPU)
Q_WIDE_SWEEPS.update({("slow", 201, 0.997, Q_SLOW_TOL, 1000): 765, ("slow", 257, 0.997, Q_SLOW_TOL, 1000): 766,
                      ("slow", 257, 0.997, Q_SLOW_TOL, 100): 100})


def q_fast(n):
    """d3 = |randn| + 0.1: ends within a few sweeps."""
    g = torch.Generator().manual_seed(Q_FAST_SEEDS[n])
    return (torch.randn(n, n, generator=g).abs() + 0.1).numpy().astype(np.float32)


def q_slow(n):
    """d3 = 1 + 0.05 |randn| with column 0 at 1000: the cost of reaching row 0 keeps the cheap cycles alive, as neighbouring
    frames do in a real video, and alpha = 0.997 then takes hundreds of sweeps."""
    g = torch.Generator().manual_seed(Q_SLOW_SEEDS[n])
    d = (1 + 0.05 * torch.randn(n, n, generator=g).abs()).float()
    d[:, 0] = 1000.0
    return d.numpy().astype(np.float32)


_INPUTS = {"fast": q_fast, "slow": q_slow, "edge": R.q_input}
_CACHE = {}


def q_wide_input(kind, n):
    key = ("input", kind, n)
    if key not in _CACHE:
        _CACHE[key] = _INPUTS[kind](n)
    return _CACHE[key]


def q_wide_case(kind, n, alpha, tol, max_iter=1000):
    """q_learning_ref of the named input -> (matrix, sweeps, residuals)."""
    key = (kind, n, alpha, tol, max_iter)
    if key not in _CACHE:
        _CACHE[key] = R.q_learning_ref(q_wide_input(kind, n), alpha, tol, max_iter)
    return _CACHE[key]


def diagonal_is_a_row_minimum(d):
    """Some row's diagonal entry is below all its others: a minimum without the k != j mask gives another matrix."""
    off = np.where(~np.eye(len(d), dtype=bool), d, np.float32(np.inf)).min(axis=1)
    return bool((np.diag(d) < off).any())


def q_vector_form(d3, alpha, tol=10e-3, max_iter=1000):
    """The sweep with the iteration kept in a vector: every row i >= 1 receives the same addend a_t[j] = fl32(alpha * mins_t[j]),
    so old_t[i, j] = fl32(d3[i, j] + a_{t-1}[j]) (old_0 = d3, row 0 always d3's) and nothing of size n^2 is kept between
    sweeps -> (matrix, sweeps, residuals) like q_learning_ref."""
    d3 = np.ascontiguousarray(d3, np.float32)
    n = d3.shape[0]
    alpha, tol = np.float32(alpha), np.float32(tol)
    off = ~np.eye(n, dtype=bool)

    def matrix(a):
        if a is None:
            return d3
        m = d3 + a[None, :]
        m[0] = d3[0]
        return m

    a_prev, it, residuals = None, 0, []
    while True:
        old = matrix(a_prev)
        a = alpha * np.where(off, old, np.float32(np.inf)).min(axis=1)
        assert a.dtype == np.float32
        d = (matrix(a) - old)[1:]
        res = np.float32((d * d).astype(np.float64).sum() / float(n * n))
        a_prev, it = a, it + 1
        residuals.append(res)
        if not (res > tol) or it >= max_iter:
            return matrix(a_prev).copy(), it, residuals


# ---------------------------------------------------------------- the P tail
P_SIZES = (2, 3, 65, 257, 1000)
P_SIGMA_FACTOR, P_THRESHOLD = 0.1, 0.75


def p_input(n):
    """d = 20 + 10 |randn| with a zero diagonal and, as two identical frames give, one duplicated pair of rows / columns
    (n // 3 and n - 1) whose mutual distance is 0.  n = 2 has no such pair: it would leave no element != 0 and sigma = 0 / 0."""
    key = ("p_input", n)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(31000 + n)
        d = (20 + 10 * torch.randn(n, n, generator=g).abs()).numpy().astype(np.float32)
        if n >= 3:
            a, b = n // 3, n - 1
            d[b, :] = d[a, :]
            d[:, b] = d[:, a]
            d[a, b] = d[b, a] = 0
        np.fill_diagonal(d, 0)
        _CACHE[key] = d
    return _CACHE[key]


def sigma_ref(d, sigma_factor):
    """fl32(fl32(sigma_factor) * fl32(fl32(S) / fl32(Z))) with S = numpy's fp64 sum and Z = the number of elements != 0."""
    d = np.asarray(d, np.float32)
    s, z = np.float32(d.astype(np.float64).sum()), np.float32(np.count_nonzero(d))
    return np.float32(np.float32(sigma_factor) * np.float32(s / z))


def p_ref64(d, sigma):
    """fp64 P from fp32 d and a given sigma -> (p64 [n, n], xmax [n] = max |d / sigma| of each row's SOURCE row); row i comes from
    row min(i + 1, n - 1) of d."""
    d = np.asarray(d, np.float32).astype(np.float64)
    n = len(d)
    src = np.minimum(np.arange(n) + 1, n - 1)
    x = -d[src] / float(sigma)
    e = np.exp(x)
    return e / e.sum(axis=1, keepdims=True), np.abs(x).max(axis=1)


def threshold_ref32(p, th):
    """q_learning.py:59-64 in fp32 on a given fp32 P."""
    p = np.asarray(p, np.float32)
    cut = p.max(axis=1, keepdims=True)
    lim = cut - np.float32(th) * cut
    assert lim.dtype == np.float32
    return np.where(p < lim, np.float32(0), p)


# ---------------------------------------------------------------- the chain
CHAIN_FRAMES, CHAIN_FILTER, CHAIN_SIGMA_FACTOR = 260, 16, 0.1


def chain_frames():
    return torch.randint(0, 256, (CHAIN_FRAMES, 16, 16, 3), generator=torch.Generator().manual_seed(7), dtype=torch.uint8)


def chain_host(classic):
    """classic.compute_D1 / compute_D2 / q_learning on the host for chain_frames() (m = 245 rows after the filter), and
    q_learning_ref's sweep count and residuals on the same d2 ** 0.7."""
    key = "chain_host"
    if key not in _CACHE:
        d1, p1, s1 = classic.compute_D1(chain_frames(), CHAIN_SIGMA_FACTOR)
        d2, p2, s2, _ = classic.compute_D2(d1, CHAIN_SIGMA_FACTOR, filter_size=CHAIN_FILTER)
        d3, p3, p3_new, s3 = classic.q_learning(d2, CHAIN_SIGMA_FACTOR)
        ref, sweeps, residuals = R.q_learning_ref((d2 ** 0.7).numpy(), 0.997, 10e-3, 1000)
        _CACHE[key] = dict(d1=d1, p1=p1, sigma1=s1, d2=d2, p2=p2, sigma2=s2, d3=d3, p3=p3, p3_new=p3_new, sigma3=s3,
                           ref_d3=ref, sweeps=sweeps, residuals=residuals)
    return _CACHE[key]


def reference_walk(p, n_steps, start, rng):
    """video_textures.py:48-51, 73-81, 103, 120 restated literally for a torch matrix."""
    this_frame = start
    new_frames_list = [start]
    jump_count = 0
    while len(new_frames_list) < n_steps:
        next_frame = rng.choice(p[this_frame].nonzero().view(-1).detach().cpu().numpy())
        if next_frame != this_frame + 1:
            jump_count += 1
        new_frames_list.append(next_frame)
        this_frame = next_frame
    return [int(f) for f in new_frames_list], jump_count
