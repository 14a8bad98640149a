"""The yardsticks of tests/test_gpu_classic_wide.py, checked on the CPU: the sweep counts the GPU tests expect, their
clearance from the tolerance, the vector form of the sweep, the fp64 P tail against classic._p_from_d, and texture_walk."""
import os

import numpy as np
import pytest
import torch

import classic_wide_refs as W
import loss_classic_refs as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("case", sorted(W.Q_WIDE_SWEEPS), ids=lambda c: "%s%d-a%g-tol%g-max%d" % c)
def test_sweep_counts_clearance_and_diagonal(case):
    kind, n, alpha, tol, max_iter = case
    d3 = W.q_wide_input(kind, n)
    out, sweeps, res = W.q_wide_case(kind, n, alpha, tol, max_iter)
    print("%s(%d) alpha=%g: %d sweeps, last residuals %s" % (kind, n, alpha, sweeps, [float(r) for r in res[-2:]]))
    assert sweeps == W.Q_WIDE_SWEEPS[case]
    assert R.residuals_clear_of_tol(res, tol, rel=1e-6)
    assert W.diagonal_is_a_row_minimum(d3)
    if max_iter == 100:
        assert abs(float(res[-1]) - 0.544) < 1e-3 and float(res[-1]) > tol  # the tolerance alone would go on
    assert np.array_equal(out[0].view(np.uint32), d3[0].view(np.uint32)) and not np.array_equal(out[1:], d3[1:])


def test_old_kernel_sizes_have_their_cases():
    for n in (2, 3, 65, 200):
        for alpha in R.Q_ALPHAS:
            assert R.q_case(n, alpha)[1] >= 1 and n in R.Q_SEEDS


@pytest.mark.parametrize("kind,n,alpha,tol", [("slow", 201, 0.997, W.Q_SLOW_TOL), ("fast", 257, 0.997, R.Q_TOL), ("fast", 257, 0.5, R.Q_TOL),
                                              ("edge", 2, 0.997, R.Q_TOL), ("edge", 65, 0.5, R.Q_TOL)])
def test_vector_form_is_bit_equal_to_the_sweep(kind, n, alpha, tol):
    want, sweeps, res = W.q_wide_case(kind, n, alpha, tol)
    got, it, res_v = W.q_vector_form(W.q_wide_input(kind, n), alpha, tol)
    assert it == sweeps
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(np.array(res_v).view(np.uint32), np.array(res).view(np.uint32))


def test_vector_form_stops_like_the_sweep():
    d3 = W.q_wide_input("fast", 257)
    for tol, max_iter in ((1e-30, 5), (1e30, 1000)):
        want, sweeps, _ = R.q_learning_ref(d3, 0.997, tol, max_iter)
        got, it, _ = W.q_vector_form(d3, 0.997, tol, max_iter)
        assert it == sweeps == (5 if max_iter == 5 else 1) and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_p_reference_agrees_with_the_host_tail(avt):
    """p_ref64 / sigma_ref / threshold_ref32 against classic._p_from_d on the reference's own matrices (fixture G8), at the
    tolerances tests/test_host_logic.py holds the host P1 / P2 to."""
    g = np.load(os.path.join(GOLD, "g8_classic.npz"))
    for name in ("d1", "d2", "d3"):
        d = g[name]
        p_host, s_host = avt.classic._p_from_d(torch.from_numpy(d), 0.1)
        sigma = W.sigma_ref(d, 0.1)
        # the host sums in fp32 (<= 400 entries, blocked: some log2(400) = 9 roundings of 2^-24 deep), the reference in fp64
        assert abs(float(sigma) - float(s_host)) <= 1e-6 * float(s_host)
        p64, xmax = W.p_ref64(d, sigma)
        np.testing.assert_allclose(p_host.numpy(), p64, rtol=1e-4, atol=1e-7)
        assert xmax.shape == (len(d),)
    # the threshold on the reference's P3 gives the reference's thresholded P3
    assert np.array_equal(W.threshold_ref32(g["p3"], 0.75), g["p3_thresholded"])


@pytest.mark.parametrize("n", W.P_SIZES)
def test_p_inputs_stay_in_the_normal_range(n):
    d = W.p_input(n)
    sigma = W.sigma_ref(d, W.P_SIGMA_FACTOR)
    p64, xmax = W.p_ref64(d, sigma)
    print("p_input(%d): sigma %.6f, max |d / sigma| %.2f, smallest p %.3e" % (n, float(sigma), xmax.max(), p64.min()))
    assert np.isfinite(sigma) and sigma > 0
    assert np.abs(d.astype(np.float64) / float(sigma)).max() <= 60  # exp(-60) = 8.8e-27 and p >= e / n: normal fp32 numbers
    assert p64.min() > 2.0 ** -126
    assert (np.diag(d) == 0).all()
    if n >= 3:
        a, b = n // 3, n - 1
        assert d[a, b] == 0 and d[b, a] == 0 and np.count_nonzero(d) == n * n - n - 2
        keep = [k for k in range(n) if k not in (a, b)]
        assert np.array_equal(d[a, keep], d[b, keep]) and np.array_equal(d[keep, a], d[keep, b])
    assert np.array_equal(p64[n - 2], p64[n - 1])


def test_chain_host_run_is_clear_of_the_tolerance(avt):
    """The host run the GPU chain test compares with: past the old kernel's 200 rows, q_learning_ref reproduces
    classic.q_learning bit for bit, and no residual lies within 1e-3 (relative) of the tolerance, so that a last-ulp difference of
    the device pow cannot move the sweep count."""
    h = W.chain_host(avt.classic)
    print("chain: %d rows, %d sweeps, last residuals %s" % (h["d3"].shape[0], h["sweeps"], [float(r) for r in h["residuals"][-2:]]))
    assert h["d3"].shape == (245, 245)
    assert np.array_equal(h["ref_d3"].view(np.uint32), h["d3"].numpy().view(np.uint32))
    assert R.residuals_clear_of_tol(h["residuals"], 10e-3, rel=1e-3)
    assert h["sweeps"] < 1000
    assert bool((h["p3_new"] > 0).any(dim=1).all())


# ---------------------------------------------------------------- texture_walk
def test_texture_walk_is_the_reference_loop(avt):
    p = torch.from_numpy(np.load(os.path.join(GOLD, "g8_classic.npz"))["p3_thresholded"])
    n, steps = p.shape[0], 60
    start = n // 2
    want, want_jumps = W.reference_walk(p, steps, start, np.random.RandomState(7))
    got, jumps = avt.classic.texture_walk(p, steps, start=start, rng=np.random.RandomState(7))
    print("walk on %d frames from %d: %d jumps in %d steps: %s" % (n, start, jumps, steps, got))
    assert got == want and jumps == want_jumps and len(got) == steps and got[0] == start
    assert all(isinstance(f, int) for f in got) and 0 < jumps
    assert jumps == sum(1 for a, b in zip(got, got[1:]) if b != a + 1)
    np.random.seed(7)
    assert avt.classic.texture_walk(p, steps, start=start) == (want, want_jumps)  # rng=None: the global stream, as the reference
    assert avt.classic.texture_walk(p.numpy(), steps, start=start, rng=np.random.RandomState(7)) == (want, want_jumps)
    # uniform over the survivors, not weighted by P: a row of two survivors with weights 0.999 / 0.001 splits evenly
    two = torch.zeros(3, 3)
    two[:, 0], two[:, 2] = 0.999, 0.001
    seq, _ = avt.classic.texture_walk(two, 2000, start=0, rng=np.random.RandomState(3))
    assert 800 < seq.count(2) < 1200 and seq.count(1) == 0


def test_texture_walk_with_one_survivor_never_leaves_it(avt):
    n = 9
    p = torch.zeros(n, n)
    p[torch.arange(n), (torch.arange(n) + 1) % n] = 1.0  # frame i -> i + 1, the last one back to 0
    seq, jumps = avt.classic.texture_walk(p, 3 * n + 1, start=4, rng=np.random.RandomState(1))
    assert seq == [(4 + k) % n for k in range(3 * n + 1)]
    assert jumps == 3  # only the wrap n - 1 -> 0 is a jump
    assert avt.classic.texture_walk(p, 1, start=4) == ([4], 0)
