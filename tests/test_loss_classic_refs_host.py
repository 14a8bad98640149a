"""The references of tests/loss_classic_refs.py against what the project already trusts (the C oracle, oracle/ref_py, the
G8 fixture of the reference's own run, classic.q_learning), on the CPU, before anything is judged by them on a GPU."""
import os

import numpy as np
import pytest
import torch

import loss_classic_refs as R
from oracle import cref, ref_py

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _logits(b, c, seed, scale=10.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(b, c, generator=g) * scale).numpy().astype(np.float32)


@pytest.mark.parametrize("b,c", [(8, 15), (9, 65), (7, 1000), (1, 1)])
@pytest.mark.parametrize("labelled", [False, True])
def test_softmax_ce_ref_agrees_with_the_c_oracle(b, c, labelled):
    """Both work in fp64 and round once: one fp32 ulp apart at the most, forward; the backward is the same fp32 arithmetic."""
    x = _logits(b, c, 10 * b + c)
    label = np.random.default_rng(c).integers(0, c, b) if labelled else None
    loss, prob = R.softmax_ce_ref(x, label)
    ol, op = cref.softmax_ce_fwd(x, label)
    assert (np.abs(ol - loss) <= R.ulp32(loss)).all()
    assert (np.abs(op - prob) <= R.ulp32(prob)).all()
    assert (np.abs(prob.sum(1) - 1.0) < 1e-14).all()
    for scale in (1.0, 1.0 / b):
        assert np.array_equal(R.softmax_ce_bwd_ref(op, label, scale), cref.softmax_ce_bwd(op, label, scale))


def test_softmax_ce_ref_is_torch_log_softmax():
    x = _logits(6, 130, 5, 30.0)
    label = np.array([0, 129, 64, 7, 100, 1])
    loss, prob = R.softmax_ce_ref(x, label)
    lp = torch.log_softmax(torch.from_numpy(x).double(), dim=1)
    np.testing.assert_allclose(loss, -lp[torch.arange(6), torch.from_numpy(label)].numpy(), rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(prob, lp.exp().numpy(), rtol=1e-12, atol=0)


def test_softmax_ce_ref_keeps_a_loss_far_below_one_ulp_of_one():
    """The label on a maximum 30 and 50 above the rest: log(1 + s) in fp64 loses the loss (s = 9e-14: 1e-3 off; s = 2e-22:
    gone), log1p keeps it."""
    x = np.array([[0.0, 30.0, 0.0], [50.0, 0.0, 0.0]], np.float32)
    loss, _ = R.softmax_ce_ref(x, np.array([1, 0]))
    np.testing.assert_allclose(loss, [2 * np.exp(-30.0), 2 * np.exp(-50.0)], rtol=1e-12)
    ol, _ = cref.softmax_ce_fwd(x, np.array([1, 0]))  # the C oracle takes the same form
    assert (np.abs(ol - loss) <= R.ulp32(loss)).all()
    for shift in (0.0, 1e4):  # ... and shifted by 1e4, where max + log(sum) - x[label] would carry 2e-12 of absolute error
        xs = (np.array([[0.0, 14.0, 3.0]], np.float32) + np.float32(shift)).astype(np.float32)
        ls, _ = R.softmax_ce_ref(xs, np.array([1]))
        os_, _ = cref.softmax_ce_fwd(xs, np.array([1]))
        assert abs(ls[0] - (np.exp(-14.0) + np.exp(-11.0))) < 1e-9 and (np.abs(os_ - ls) <= R.ulp32(ls)).all()


def test_c_oracle_marks_out_of_range_labels_like_the_kernel():
    x = _logits(4, 5, 3)
    good, bad = np.array([1, 0, 4, 2]), np.array([1, -1, 5, 2])
    (lg, pg), (lb, pb) = cref.softmax_ce_fwd(x, good), cref.softmax_ce_fwd(x, bad)
    marked = np.array([False, True, True, False])
    assert np.array_equal(np.isnan(lb), marked) and np.array_equal(lb[~marked], lg[~marked]) and np.array_equal(pb, pg)
    db = cref.softmax_ce_bwd(pb, bad, 0.25)
    assert np.array_equal(np.isnan(db), np.repeat(marked[:, None], 5, axis=1))
    assert np.array_equal(db[~marked], cref.softmax_ce_bwd(pg, good, 0.25)[~marked])


def test_classic_refs_reproduce_the_oracle_and_the_reference_fixture():
    """pairwise_ref / diag_filter_ref vs ref_py.classic_d1_p1 / classic_d2 and the G8 arrays, at test_oracle_golden's tolerances."""
    g = np.load(os.path.join(GOLD, "g8_classic.npz"))
    frames = g["frames"]
    d1 = R.pairwise_ref(frames.reshape(len(frames), -1))
    o1, _, _ = ref_py.classic_d1_p1(frames, 0.1)
    np.testing.assert_allclose(d1, o1, rtol=2e-6, atol=1e-3)
    np.testing.assert_allclose(d1, g["d1"], rtol=2e-6, atol=1e-3)
    assert (np.diag(d1) == 0).all() and np.array_equal(d1, d1.T)
    w = (np.poly1d([0.5, 0.5]) ** 3).coeffs.astype(np.float32)
    d2, mag = R.diag_filter_ref(g["d1"], w)
    o2, _, _ = ref_py.classic_d2(g["d1"], 0.1, filter_size=4)
    np.testing.assert_allclose(d2, o2, rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(d2, g["d2"], rtol=1e-5, atol=1e-3)
    assert d2.shape == g["d2"].shape and (mag >= np.abs(d2) * (1 - 1e-15)).all()


def test_q_learning_ref_is_bit_equal_to_classic_q_learning(avt):
    g = np.load(os.path.join(GOLD, "g8_classic.npz"))
    mats = [torch.from_numpy(g["d2"])]
    for seed, n in ((1, 5), (2, 23)):
        mats.append(torch.randn(n, n, generator=torch.Generator().manual_seed(seed)).abs() + 0.1)
    for d2 in mats:
        want, _, _, _ = avt.classic.q_learning(d2, 0.1)
        got, sweeps, res = R.q_learning_ref((d2 ** 0.7).numpy(), 0.997, 10e-3, 1000)
        assert R.residuals_clear_of_tol(res, 10e-3) and len(res) == sweeps and 1 < sweeps < 1000
        assert np.array_equal(got.view(np.uint32), want.numpy().view(np.uint32))
        assert np.array_equal(got[0], (d2 ** 0.7).numpy()[0])


def test_q_learning_ref_stops_at_max_iter_and_at_a_loose_tol():
    d3 = R.q_input(65)
    full, sweeps, res = R.q_case(65, 0.997)
    assert sweeps > 5
    five, it5, res5 = R.q_learning_ref(d3, 0.997, R.Q_TOL, 5)
    assert it5 == 5 and res5 == res[:5] and not np.array_equal(five, full)
    one, it1, _ = R.q_learning_ref(d3, 0.997, 1e30, 1000)
    assert it1 == 1 and np.array_equal(one[0], d3[0]) and not np.array_equal(one[1:], d3[1:])


@pytest.mark.parametrize("n", R.Q_SIZES)
@pytest.mark.parametrize("alpha", R.Q_ALPHAS)
def test_q_learning_gpu_inputs_keep_every_residual_clear_of_tol(n, alpha):
    """Every input of the GPU test: no sweep's residual (the stopping one and the one before it included) within 1e-6
    relative of tol, so the kernel's own fp64 summation order cannot legitimately change the sweep count."""
    _, sweeps, res = R.q_case(n, alpha)
    assert len(res) == sweeps and sweeps < 1000 and not (res[-1] > np.float32(R.Q_TOL))
    assert R.residuals_clear_of_tol(res, R.Q_TOL)
    d3 = R.q_input(n)
    assert (np.diag(d3) < np.where(np.eye(n, dtype=bool), np.inf, d3).min(axis=1)).any()  # the k != j mask decides a minimum
    if n == 65 and alpha == 0.997:
        _, it5, res5 = R.q_case(65, 0.997, R.Q_TOL, 5)
        assert it5 == 5 and R.residuals_clear_of_tol(res5, R.Q_TOL) and res5[-1] > np.float32(R.Q_TOL)
