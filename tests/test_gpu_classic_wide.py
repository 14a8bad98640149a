"""The classic baseline past 200 frames on the device (csrc/classic_wide.hip): the future-cost sweeps of any size bit-equal to
loss_classic_refs.q_learning_ref, the two-pass P tail against its fp64 evaluation, and the whole chain against the host
functions of classic.py.  The yardsticks are proved on the CPU by tests/test_classic_wide_refs_host.py.

Every bound is derived where it is used; every test prints the figures it asserts on (pytest -s shows them)."""
import numpy as np
import pytest
import torch

import classic_wide_refs as W
import loss_classic_refs as R

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


def _bits(a):
    a = _np(a) if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.uint32)


def _run(avt, dev, d3, alpha, tol, max_iter=1000):
    out, iters = avt.ops.q_learning_wide(torch.from_numpy(d3).to(dev), alpha, tol, max_iter)
    return _np(out), int(iters.item())


# ---------------------------------------------------------------- sweeps
# 201: the first size past the LDS kernel; 256 / 257: a full and an overfull 256-lane trip (a wave's 16-byte lanes: exactly one
# trip with every row aligned, and one trip plus a scalar tail on rows that start on any float; 2 and 3 are all tail);
# 1025: a last workgroup with one row for its four waves; 4097: one row more than the waves of one launch cover in one trip.  The
# slow inputs run through hundreds of launches, every polling interval and the lagged residual.
SWEEP_CASES = [("fast", n, a, R.Q_TOL) for n in (201, 256, 257, 1025) for a in (0.5, 0.997)] + [("fast", 4097, 0.5, R.Q_TOL)] + \
              [("slow", 201, 0.997, W.Q_SLOW_TOL), ("slow", 257, 0.997, W.Q_SLOW_TOL)] + \
              [("edge", n, a, R.Q_TOL) for n in (2, 3, 65, 200) for a in R.Q_ALPHAS]  # sizes the old kernel takes as well


@pytest.mark.parametrize("kind,n,alpha,tol", SWEEP_CASES, ids=["%s%d-a%g" % c[:3] for c in SWEEP_CASES])
def test_wide_sweeps_are_bit_equal_to_the_reference(avt, dev, kind, n, alpha, tol):
    d3 = W.q_wide_input(kind, n)
    want, sweeps, res = W.q_wide_case(kind, n, alpha, tol) if kind != "edge" else R.q_case(n, alpha)
    got, iters = _run(avt, dev, d3, alpha, tol)
    print("q_learning_wide %s(%d) alpha=%g: %d sweeps (reference %d), last residuals %s"
          % (kind, n, alpha, iters, sweeps, [float(r) for r in res[-2:]]))
    if kind != "edge":
        assert sweeps == W.Q_WIDE_SWEEPS[(kind, n, alpha, tol, 1000)]
    assert iters == sweeps
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[0].view(np.uint32), d3[0].view(np.uint32))
    assert not np.array_equal(got[1:], d3[1:])


def test_wide_sweeps_stop_at_max_iter_and_at_a_loose_tol(avt, dev):
    d3 = W.q_wide_input("slow", 257)
    want, sweeps, res = W.q_wide_case("slow", 257, 0.997, W.Q_SLOW_TOL, 100)
    got, iters = _run(avt, dev, d3, 0.997, W.Q_SLOW_TOL, 100)
    assert sweeps == 100 and float(res[-1]) > W.Q_SLOW_TOL  # the tolerance alone would go on
    assert iters == 100 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    d3 = W.q_wide_input("fast", 257)
    want5, it5, _ = R.q_learning_ref(d3, 0.997, 1e-30, 5)
    got5, iters5 = _run(avt, dev, d3, 0.997, 1e-30, 5)
    assert it5 == 5 and iters5 == 5 and np.array_equal(got5.view(np.uint32), want5.view(np.uint32))
    want1, it1, _ = R.q_learning_ref(d3, 0.997, 1e30, 1000)
    got1, iters1 = _run(avt, dev, d3, 0.997, 1e30, 1000)
    assert it1 == 1 and iters1 == 1 and np.array_equal(got1.view(np.uint32), want1.view(np.uint32))


def test_wide_sweeps_are_deterministic(avt, dev):
    d3 = W.q_wide_input("slow", 201)
    a, ia = _run(avt, dev, d3, 0.997, W.Q_SLOW_TOL)
    b, ib = _run(avt, dev, d3, 0.997, W.Q_SLOW_TOL)
    assert ia == ib == W.Q_WIDE_SWEEPS[("slow", 201, 0.997, W.Q_SLOW_TOL, 1000)]
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_wide_sweeps_refuse_bad_arguments_before_any_launch(avt, dev):
    lib, p, st = avt._lib.lib(), avt.ops._p, avt.ops._stream
    n = 201
    d3 = torch.rand(n, n, device=dev) + 0.1
    out = torch.full((n, n), 7.0, device=dev)
    iters = torch.full((1,), -3, dtype=torch.int32, device=dev)
    need = int(lib.avt_q_learning_wide_workspace_bytes(n))
    assert need > 0 and lib.avt_q_learning_wide_workspace_bytes(1) == 0 and lib.avt_q_learning_wide_workspace_bytes(65536) == 0
    assert lib.avt_q_learning_wide_supported(2) == 1 and lib.avt_q_learning_wide_supported(65535) == 1
    assert lib.avt_q_learning_wide_supported(1) == 0 and lib.avt_q_learning_wide_supported(65536) == 0
    big = int(lib.avt_q_learning_wide_workspace_bytes(65535))
    ws = torch.zeros(big + 64, dtype=torch.uint8, device=dev)  # enough for every n tried here
    ok = dict(d3=p(d3), n=n, max_iter=1000, out=p(out), ws=p(ws), ws_bytes=need)
    bad = [dict(n=1), dict(n=65536, ws_bytes=big + 64), dict(max_iter=0), dict(d3=None), dict(out=None), dict(ws=None),
           dict(ws_bytes=need - 1)]
    for change in bad:
        a = dict(ok, **change)
        rc = lib.avt_q_learning_wide_f32(a["d3"], a["n"], 0.997, 1e-3, a["max_iter"], a["out"], p(iters), a["ws"], a["ws_bytes"], st())
        print("refused %s: %d, %s" % (change, rc, lib.avt_last_error().decode()))
        assert rc != 0, change
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and int(iters.item()) == -3  # refused before any launch
    with pytest.raises(avt._lib.AvtError):
        avt.ops.q_learning_wide(torch.rand(1, 1, device=dev), 0.997)
    with pytest.raises(avt._lib.AvtError):
        avt.ops.q_learning_wide(d3, 0.997, max_iter=0)


# ---------------------------------------------------------------- the P tail
@pytest.mark.parametrize("n", W.P_SIZES)  # 2, 3: the smallest; 65: a ragged 64-lane wave; 257: a second trip; 1000: several statistics blocks
def test_classic_p_against_fp64(avt, dev, n):
    d = W.p_input(n)
    dd = torch.from_numpy(d).to(dev)
    p, sigma, p_thr = avt.ops.classic_p(dd, W.P_SIGMA_FACTOR, threshold=W.P_THRESHOLD)
    p2, sigma2 = avt.ops.classic_p(dd, W.P_SIGMA_FACTOR)
    assert np.array_equal(_bits(p2), _bits(p)) and float(sigma2) == float(sigma)  # the thresholded copy changes nothing else
    p, p_thr, sigma = _np(p), _np(p_thr), np.float32(sigma.item())
    # sigma: S is an fp64 sum in another order than numpy's (relative 1e-13 apart), then four fp32 roundings of the same
    # formula: off by one ulp only where fl32(S) falls next to a rounding boundary.  Z is implied: one element more or fewer
    # moves sigma by 1 / n^2 >= 1e-6 relative, 8 ulp and more
    want = W.sigma_ref(d, W.P_SIGMA_FACTOR)
    ulps = abs(float(sigma) - float(want)) / float(np.spacing(want))
    # p: the division rounds the argument x = -d / sigma by a relative 2^-24, which exp turns into a relative |x| 2^-24; expf adds
    # 1 ulp (2^-23 at the most); both pass to the row sum as well (together 2 |x| 2^-24 + 2^-22 = |x| 2^-23 + 2^-22); the sum and the
    # quotient add one rounding each (2^-23 in all).  xmax 2^-23 + 2^-21 covers the lot
    p64, xmax = W.p_ref64(d, sigma)
    bound = p64 * (xmax[:, None] * 2.0 ** -23 + 2.0 ** -21)
    err = np.abs(p.astype(np.float64) - p64)
    rows = np.abs(p.astype(np.float64).sum(axis=1) - 1.0)
    print("classic_p n=%d: sigma %.7g (%.2f ulp from the formula), max err / bound %.3f, xmax %.2f, |row sum - 1| %.2e (bound %.2e)"
          % (n, float(sigma), ulps, (err / bound).max(), xmax.max(), rows.max(), n * 2.0 ** -24))
    assert ulps <= 1.0
    assert np.isfinite(p).all() and (err <= bound).all()
    # the rounded row sum is within 2^-24 (relative) of the exact one, and the n quotients are each rounded by at most 2^-24 of
    # themselves, 2^-24 of their sum in all: 2^-23, which n 2^-24 covers from n = 2 on
    assert (rows <= n * 2.0 ** -24).all()
    assert np.array_equal(p[n - 2].view(np.uint32), p[n - 1].view(np.uint32))  # both from row n - 1 of d
    # the threshold, in fp32 on the kernel's own p
    want_thr = W.threshold_ref32(p, W.P_THRESHOLD)
    assert np.array_equal(p_thr.view(np.uint32), want_thr.view(np.uint32))
    assert np.array_equal(p_thr.max(axis=1), p.max(axis=1)) and ((p_thr == 0) | (p_thr == p)).all()
    if n >= 65:
        assert (p_thr == 0).any()


@pytest.mark.parametrize("n", W.P_SIZES)
def test_classic_p_row_0_of_d_reaches_sigma_only(avt, dev, n):
    d = W.p_input(n)
    dd = torch.from_numpy(d).to(dev)
    p, sigma, p_thr = avt.ops.classic_p(dd, W.P_SIGMA_FACTOR, threshold=W.P_THRESHOLD)
    other = d.copy()
    other[0] = 3.0 * d[0, ::-1] + 1.0  # permuted, and another sum and another count of zeros
    assert not np.array_equal(other[0], d[0])
    q, sigma_q, q_thr = avt.ops.classic_p(torch.from_numpy(other).to(dev), W.P_SIGMA_FACTOR, threshold=W.P_THRESHOLD,
                                          sigma=sigma.clone().reshape(1))
    assert float(sigma_q) == float(sigma)  # supplied, not recomputed
    assert np.array_equal(_bits(q), _bits(p)) and np.array_equal(_bits(q_thr), _bits(p_thr))
    _, sigma_own = avt.ops.classic_p(torch.from_numpy(other).to(dev), W.P_SIGMA_FACTOR)
    assert float(sigma_own) != float(sigma)  # ... and without the supplied one the changed row does move sigma
    assert abs(float(sigma_own) - float(W.sigma_ref(other, W.P_SIGMA_FACTOR))) <= float(np.spacing(W.sigma_ref(other, W.P_SIGMA_FACTOR)))


def test_classic_p_refuses_bad_arguments(avt, dev):
    lib, p, st = avt._lib.lib(), avt.ops._p, avt.ops._stream
    n = 65
    d = torch.from_numpy(W.p_input(n)).to(dev)
    out = torch.full((n, n), 7.0, device=dev)
    sigma = torch.full((1,), 7.0, device=dev)
    need = int(lib.avt_classic_p_workspace_bytes())
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    assert lib.avt_classic_p_f32(p(d), 1, 0.1, 0, p(sigma), 0.0, p(out), None, p(ws), need, st()) != 0
    assert lib.avt_classic_p_f32(p(d), 65536, 0.1, 0, p(sigma), 0.0, p(out), None, p(ws), need, st()) != 0
    assert lib.avt_classic_p_f32(None, n, 0.1, 0, p(sigma), 0.0, p(out), None, p(ws), need, st()) != 0
    assert lib.avt_classic_p_f32(p(d), n, 0.1, 0, p(sigma), 0.0, p(out), None, p(ws), need - 1, st()) != 0
    assert lib.avt_classic_p_f32(p(d), n, 0.1, 0, p(sigma), 0.0, p(out), None, None, need, st()) != 0
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and float(sigma) == 7.0


# ---------------------------------------------------------------- the chain
@pytest.fixture(scope="module")
def chain(avt, dev):
    return avt.classic.texture_device(W.chain_frames(), W.CHAIN_SIGMA_FACTOR, filter_size=W.CHAIN_FILTER, device=dev)


def test_texture_device_matches_the_host_chain(avt, dev, chain):
    """260 frames -> m = 245 rows after the 16-tap filter, past the old kernel's 200; the tolerances are those
    test_gpu_kernels.test_classic_d2_and_q_learning_on_device holds the same comparison to at 185 rows."""
    h = W.chain_host(avt.classic)
    assert chain["d1"].shape == (260, 260) and chain["d3"].shape == (245, 245)
    for k in ("d1", "d2", "d3"):
        np.testing.assert_allclose(_np(chain[k]), h[k].numpy(), rtol=1e-5, atol=1e-3, err_msg=k)
    for k in ("p1", "p2", "p3"):
        np.testing.assert_allclose(_np(chain[k]), h[k].numpy(), rtol=2e-3, atol=1e-7, err_msg=k)
    for k in ("sigma1", "sigma2", "sigma3"):
        np.testing.assert_allclose(float(chain[k]), float(h[k]), rtol=1e-5, err_msg=k)
    print("chain: %d sweeps on the device, %d on the host" % (chain["iters"], h["sweeps"]))
    assert chain["iters"] == h["sweeps"]
    assert np.array_equal(_np(chain["p3_new"]) > 0, h["p3_new"].numpy() > 0)


def test_q_learning_device_past_200_rows_is_the_chains_last_stage(avt, dev, chain):
    d3, p3, p3_new, sigma = avt.classic.q_learning_device(chain["d2"], W.CHAIN_SIGMA_FACTOR)
    assert np.array_equal(_bits(d3), _bits(chain["d3"])) and np.array_equal(_bits(p3), _bits(chain["p3"]))
    assert np.array_equal(_bits(p3_new), _bits(chain["p3_new"])) and float(sigma) == float(chain["sigma3"])


def test_texture_walk_on_the_device_matrix(avt, dev, chain):
    p = chain["p3_new"]
    assert p.is_cuda
    got = avt.classic.texture_walk(p, 90, rng=np.random.RandomState(11))  # from frame 100, the reference's start
    want = avt.classic.texture_walk(p.cpu(), 90, rng=np.random.RandomState(11))
    print("device walk: %d jumps in 90 steps" % got[1])
    assert got == want and got[0][0] == 100 and len(got[0]) == 90
