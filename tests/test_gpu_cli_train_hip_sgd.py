"""`train()` and `main.py` with train_ops.ArenaSGD (`--train_optimizer hip`) on the MI355X: an epoch replayed as a HIP graph
(`--train_graph 1`) follows the StepLR schedule and takes ONE step per batch from the first batch on, so it can be held to the eager
loop.  The fixture of test_train_one_epoch_as_a_replayed_graph (TinySlowFast, batch 4, drop_last, 32^2), three batches per epoch.

Graph against eager: the bound is max(the tolerance of test_graphed_step_equals_the_eager_step, 4 x floor), the floor being the largest
relative difference between two EAGER runs from the same seeds (the order of fp32 atomic sums is not fixed).  Measured on an MI355X:
profiles/r11/README.md."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tiny_encoders import TinySlowFast, seeded  # noqa: E402

pytestmark = pytest.mark.gpu


def _video(n=33, hw=32, seed=5):
    g = torch.Generator().manual_seed(seed)
    base = torch.rand((n // 6 + 2, hw, hw, 3), generator=g)
    t = torch.linspace(0, n / 6, n)
    i0 = t.floor().long()
    fr = (t - i0.float()).view(-1, 1, 1, 1)
    return (((1 - fr) * base[i0] + fr * base[i0 + 1]).clamp(0, 1) * 255).to(torch.uint8)


def _train(avt, dev, train_graph, gamma, epochs=2, after_epoch=None):
    """`epochs` epochs of train() with ArenaSGD(lr 0.05, momentum 0.9) + StepLR(step_size 1, gamma) from fixed seeds
    -> (losses per epoch, parameters, buffers)."""
    from avtex import train_ops

    args = SimpleNamespace(vdata="/tmp", adata=None, n_negs=10, img_size=32, enc_arch="slowfast", window=0, stride=0,
                           print_freq=100, log_freq=100, train_graph=train_graph)
    torch.manual_seed(1)
    ds = avt.AudioVideoSegments(args, "x", split="train", video=(_video(), 10.0))
    loader = torch.utils.data.DataLoader(ds, batch_size=4, shuffle=True, num_workers=0, drop_last=True)
    assert len(loader) == 3
    model = avt.ContrastivePredictionTemporal(seeded(TinySlowFast, 1), seeded(TinySlowFast, 2), None, 1, 128, temp=0.1,
                                              window=5, stride=2, enc_arch="slowfast", img_size=32).to(dev)
    opt = train_ops.ArenaSGD(model.parameters(), lr=0.05, momentum=0.9)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=gamma)
    np.random.seed(0)
    torch.manual_seed(2)
    train_ops.invalidate_weight_cache()
    before = train_ops.CALLS["sgd_multi"]
    losses = []
    for epoch in range(epochs):
        losses.append(avt.train(loader, model, opt, args, epoch))
        sched.step()
        if after_epoch is not None:
            torch.cuda.synchronize()
            after_epoch(epoch, model)
    torch.cuda.synchronize()
    # eager: one launch per batch; graph: two warm-up steps and the capture pass through the host, the replays do not
    assert train_ops.CALLS["sgd_multi"] - before == (3 if train_graph else 3 * epochs)
    return losses, [p.detach().clone() for p in model.parameters()], [b.detach().clone() for b in model.buffers()]


def _rel(a, b):
    return float((a.double() - b.double()).abs().max()) / max(float(a.double().abs().max()), 1e-30)


_EAGER = {}


def _eager(avt, dev):
    if "run" not in _EAGER:  # computed once, shared, left unchanged
        _EAGER["run"] = _train(avt, dev, 0, 0.1)
    return _EAGER["run"]


def test_graph_equals_eager_across_a_rate_boundary(avt, dev):
    le, pe, be = _eager(avt, dev)
    le2, pe2, be2 = _train(avt, dev, 0, 0.1)
    floor = max([_rel(a, b) for a, b in zip(pe + be, pe2 + be2)] + [abs(le[0] - le2[0]) / abs(le[0])])
    lg, pg, bg = _train(avt, dev, 1, 0.1)
    worst = max([_rel(a, b) for a, b in zip(pe + be, pg + bg)] + [abs(le[0] - lg[0]) / abs(le[0])])
    print("eager-vs-eager floor %.3e, graph-vs-eager %.3e, bound max(1e-5 |a| + 1e-7 [parameters] / 1e-6 [buffers], %.3e |a|); losses "
          "eager %s graph %s" % (floor, worst, 4 * floor, le, lg))
    assert abs(le[0] - lg[0]) <= max(1e-5 * max(1.0, abs(le[0])), 4 * floor * abs(le[0])), (le, lg)
    for a, b in zip(pe, pg):
        m = float(a.abs().max())
        assert float((a - b).abs().max()) <= max(1e-5 * m + 1e-7, 4 * floor * m), (floor, worst)
    for a, b in zip(be, bg):
        m = float(a.float().abs().max())
        assert float((a.float() - b.float()).abs().max()) <= max(1e-5 * m + 1e-6, 4 * floor * m), (floor, worst)
    assert all(np.isfinite(le + lg)) and len(pe) == len(pg) > 0


def test_rate_zero_before_the_second_epoch_freezes_the_parameters(avt, dev):
    """StepLR(gamma = 0), no weight decay: the replayed second epoch must not move a single bit of any parameter — with an optimizer whose
    rate is a kernel argument the replays would go on at 0.05."""
    seen = {}

    def after_epoch(epoch, model):
        seen[epoch] = [p.detach().clone() for p in model.parameters()]

    losses, params, _ = _train(avt, dev, 1, 0.0, after_epoch=after_epoch)
    assert all(np.isfinite(losses))
    assert all(torch.equal(a, b) for a, b in zip(seen[0], seen[1])) and all(torch.equal(a, b) for a, b in zip(seen[1], params))
    _, p_eager, _ = _eager(avt, dev)
    assert any(not torch.equal(a, b) for a, b in zip(params, p_eager))  # (the run with gamma 0.1 did go on training)


def test_cli_trains_with_the_hip_optimizer_as_a_replayed_graph(avt, dev, tmp_path, capsys, monkeypatch):
    """python main.py ... --train_optimizer hip --train_graph 1 --lr_steps 1 --epochs 2 on a .npz video: runs to the end, prints a
    second-epoch loss, and the optimizer's launch is the hand-written one."""
    from avtex import train_ops
    from avtex.main import cli
    from avtex.models import ModelBuilder3D

    vdir = tmp_path / "videos"
    vdir.mkdir()
    np.savez(vdir / "clip.npz", video=_video().numpy(), fps=10.0)
    monkeypatch.chdir(tmp_path)
    # the CLI's own flow with a toy encoder in the SlowFast slot (the real one at 224^2 is not a few-second test)
    monkeypatch.setitem(ModelBuilder3D._plugins, "slowfast", lambda img_size, window, pretrained: seeded(TinySlowFast, 1))
    np.random.seed(0)
    torch.manual_seed(0)
    before = train_ops.CALLS["sgd_multi"]
    cli(["-vdata", str(vdir), "-vl", "clip", "-ea", "slowfast", "-m", "1", "-negs", "10", "-bs", "4", "-size", "32", "-j", "0",
         "--lr", "0.05", "--lr_steps", "1", "--epochs", "2", "--train_optimizer", "hip", "--train_graph", "1", "-p", "1",
         "--logdir", str(tmp_path / "logs"), "--ckpt", str(tmp_path / "ckpt")])
    out = capsys.readouterr().out
    assert "train_optimizer='hip'" in out and "Training for 2 epochs." in out
    lines = [ln for ln in out.splitlines() if ln.startswith("Epoch: [1][")]
    assert len(lines) == 3, out[-2000:]
    loss = float(lines[-1].split("Loss ")[1].split()[0])
    assert np.isfinite(loss)
    assert train_ops.CALLS["sgd_multi"] - before == 3  # two warm-up steps + the capture; six replays
    assert any(f.endswith("_latest.pth.tar") for f in os.listdir(tmp_path / "ckpt"))  # checkpoints as with the default optimizer
