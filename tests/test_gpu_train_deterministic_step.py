"""--train_deterministic at the level of the training step: from one seed, two optimiser steps run twice in fresh models leave every
parameter, every BatchNorm buffer and both losses bit-equal — eagerly with torch's SGD, and as a replayed HIP graph with the HIP
optimizer — for the tiny SlowFast operator of test_gpu_cli_train.py (32^2, window 5, stride 2), a resnet10 at 32^2 fed by the device
batcher, and the real SlowFast at 64^2 (whose convolutions, stems and pools are the hand-written training kernels); and through
main.main: the flag's printed line, two runs' checkpoints tensor for tensor, and the refusal of --train_conv fp32.

Nothing here expects the DEFAULT mode to differ between runs: it may not, at these sizes."""
import itertools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tiny_encoders import TinySlowFast, seeded  # noqa: E402

pytestmark = pytest.mark.gpu


def _video(n, hw, seed=5):
    g = torch.Generator().manual_seed(seed)
    base = torch.rand((n // 6 + 2, hw, hw, 3), generator=g)
    t = torch.linspace(0, n / 6, n)
    i0 = t.floor().long()
    fr = (t - i0.float()).view(-1, 1, 1, 1)
    return (((1 - fr) * base[i0] + fr * base[i0 + 1]).clamp(0, 1) * 255).to(torch.uint8)


def _tiny_slowfast(avt, dev):
    """The operator and loader of test_gpu_cli_train.test_train_one_epoch; the first two batches of its shuffled epoch."""
    args = SimpleNamespace(vdata="/tmp", adata=None, n_negs=10, img_size=32, enc_arch="slowfast", window=0, stride=0)
    ds = avt.AudioVideoSegments(args, "x", split="train", video=(_video(90, 32), 10.0))
    assert (args.window, args.stride) == (5, 2)
    loader = torch.utils.data.DataLoader(ds, batch_size=4, shuffle=True, num_workers=0, drop_last=True)
    model = avt.ContrastivePredictionTemporal(seeded(TinySlowFast, 1), seeded(TinySlowFast, 2), None, 1, 128, temp=0.1, window=5, stride=2,
                                              enc_arch="slowfast", img_size=32).to(dev)
    return model, list(itertools.islice(loader, 2))


def _resnet10(avt, dev):
    """resnet10 at 32^2, W = 20, in the training layout; two batches of two items assembled on the device."""
    from avtex import resnet3d, synth, train_ops
    from avtex.dataset import DeviceSegmentBatcher

    hw, W = 32, 20
    args = SimpleNamespace(vdata="/tmp", adata=None, n_negs=8, img_size=hw, enc_arch="resnet10", window=0, stride=0)
    ds = avt.AudioVideoSegments(args, "x", split="train", video=(synth.structured_video(3, 204, 32, 32), 40.0))
    model = avt.ContrastivePredictionTemporal(resnet3d.build("resnet10", hw, W), resnet3d.build("resnet10", hw, W), None, 1, 512, temp=0.1,
                                              window=W, stride=8, enc_arch="resnet10", img_size=hw)
    model = train_ops.training_layout(synth.randomise_bn(model, 4, 0.0).to(dev))
    return model, list(itertools.islice(DeviceSegmentBatcher(ds, dev).loader(2), 2))


def _slowfast(avt, dev):
    """The real SlowFast at 64^2 in the training layout: one item with three target clips per step, seeded noise for frames."""
    from avtex import synth, train_ops
    from avtex.slowfast import SlowFast

    model = avt.ContrastivePredictionTemporal(SlowFast(), SlowFast(), None, 1, 128, temp=0.1, window=5, stride=2, enc_arch="slowfast",
                                              img_size=64)
    model = train_ops.training_layout(synth.randomise_bn(model, 4, 0.0).to(dev))
    g = torch.Generator().manual_seed(11)
    batches = []
    for _ in range(2):
        q = [torch.rand(1, 3, 8, 64, 64, generator=g), torch.rand(1, 3, 32, 64, 64, generator=g)]
        t = [torch.rand(1, 3, 3, 8, 64, 64, generator=g), torch.rand(1, 3, 3, 32, 64, 64, generator=g)]
        batches.append((q, None, torch.zeros(1, 10), t, None, torch.zeros(1, 3, 10)))
    return model, batches


FAMILIES = {"tiny-slowfast": (_tiny_slowfast, False), "resnet10": (_resnet10, True), "slowfast": (_slowfast, True)}


def _two_steps(avt, dev, family, graph):
    """Fresh data, model and optimizer from one seed; two steps of train(), one batch each -> (losses, parameters, buffers, launches)."""
    from avtex import train_ops
    build, _ = FAMILIES[family]
    torch.manual_seed(1)
    np.random.seed(0)
    train_ops.invalidate_weight_cache(drop=True)
    model, batches = build(avt, dev)
    if graph:
        opt = train_ops.ArenaSGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    else:
        opt = torch.optim.SGD(model.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    args = SimpleNamespace(print_freq=100, log_freq=100, train_graph=1 if graph else 0)
    before = dict(train_ops.CALLS)
    losses = [avt.train([b], model, opt, args, 0) for b in batches]
    torch.cuda.synchronize()
    ran = {k: train_ops.CALLS[k] - before[k] for k in before}
    return (losses, [p.detach().clone() for p in model.parameters()], {k: v.detach().clone() for k, v in model.named_buffers()}, ran)


@pytest.mark.parametrize("graph", [False, True], ids=["eager-torch-sgd", "graph-hip-sgd"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_two_steps_from_one_seed_repeat_bit_for_bit(avt, dev, capsys, family, graph):
    from avtex import train_ops
    assert train_ops.set_deterministic(True) is False
    try:
        a, b = _two_steps(avt, dev, family, graph), _two_steps(avt, dev, family, graph)
    finally:
        train_ops.set_deterministic(False)
    capsys.readouterr()
    la, pa, ba, ran = a
    lb, pb, bb, _ = b
    assert all(np.isfinite(la)) and la == lb, (la, lb)  # (Python floats of the loss tensors' bits: equal means bit-equal)
    assert len(pa) == len(pb) > 0 and all(torch.equal(x, y) for x, y in zip(pa, pb))
    assert set(ba) == set(bb) and all(torch.equal(ba[k], bb[k]) for k in ba)
    if FAMILIES[family][1]:  # the families with convolutions: every weight gradient went through the deterministic entries
        assert ran["wgrad_det"] > 0 and ran["miopen_wgrad"] == 0, ran
        assert any(k.endswith("running_mean") for k in ba)
    if graph:
        assert ran["sgd_multi"] > 0, ran


def _cli_args(tmp, vdir, extra):
    return ["-vdata", str(vdir), "-vl", "clip", "-ea", "resnet10", "-m", "1", "-negs", "8", "-bs", "4", "-size", "32", "--size", "32", "-j", "0",
            "--lr", "0.01", "--epochs", "1", "--train_input", "device", "-p", "1", "--logdir", str(tmp / "logs"), "--ckpt", str(tmp / "ckpt")] + extra


@pytest.mark.parametrize("how", [[], ["--train_graph", "1", "--train_optimizer", "hip"]], ids=["eager", "graph-hip-sgd"])
def test_main_with_the_flag_prints_its_line_and_repeats_a_checkpoint(avt, dev, tmp_path, capsys, monkeypatch, how):
    from avtex import train_ops
    from avtex.main import cli

    vdir = tmp_path / "videos"
    vdir.mkdir()
    np.savez(vdir / "clip.npz", video=_video(124, 32).numpy(), fps=40.0)
    states = []
    try:
        for run in range(2):
            out_dir = tmp_path / ("run%d" % run)
            out_dir.mkdir()
            monkeypatch.chdir(out_dir)
            np.random.seed(0)
            torch.manual_seed(0)
            train_ops.invalidate_weight_cache(drop=True)
            before = train_ops.CALLS["wgrad_det"]
            cli(_cli_args(out_dir, vdir, ["--train_deterministic"] + how))
            out = capsys.readouterr().out
            said = [ln for ln in out.splitlines() if "deterministic weight gradients" in ln]
            assert len(said) == 1 and "bit-reproducible within one process" in said[0], out[-2000:]
            assert train_ops.deterministic() and train_ops.CALLS["wgrad_det"] > before
            assert len([ln for ln in out.splitlines() if ln.startswith("Epoch: [0][")]) == 3, out[-2000:]  # 12 items, batches of 4
            ck = [f for f in os.listdir(out_dir / "ckpt") if f.endswith("_latest.pth.tar")]
            assert len(ck) == 1
            states.append(torch.load(out_dir / "ckpt" / ck[0], map_location="cpu", weights_only=False))
    finally:
        train_ops.set_deterministic(False)
    sa, sb = states[0]["state_dict"], states[1]["state_dict"]
    assert list(sa) == list(sb) and len(sa) > 0
    assert all(torch.equal(sa[k], sb[k]) for k in sa), [k for k in sa if not torch.equal(sa[k], sb[k])][:5]
    assert states[0]["best_loss"] == states[1]["best_loss"]


def test_main_refuses_the_flag_with_miopen_convolutions(avt, dev, tmp_path, capsys, monkeypatch):
    from avtex import train_ops
    from avtex.main import cli

    vdir = tmp_path / "videos"
    vdir.mkdir()
    np.savez(vdir / "clip.npz", video=_video(124, 32).numpy(), fps=40.0)
    monkeypatch.chdir(tmp_path)
    try:
        with pytest.raises(avt._lib.AvtError, match="train_conv x3"):
            cli(_cli_args(tmp_path, vdir, ["--train_conv", "fp32", "--train_deterministic"]))
        assert not train_ops.deterministic()
    finally:
        train_ops.set_conv_mode("x3")
        train_ops.set_deterministic(False)
    capsys.readouterr()
