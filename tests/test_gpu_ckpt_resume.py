"""--ckpt_train_state: a run interrupted after an epoch and resumed equals the uninterrupted run bit for bit.  The CLI recipe of
test_gpu_train_deterministic_step.py (resnet10 at 32^2, the 124-frame clip, 12 items in batches of 4, --train_input device
--train_deterministic) with --epochs 2 --lr_steps 1, so that the resume crosses a learning-rate decay: run A trains both epochs; run B
trains one, and — from OTHER seeds and a dropped weight-plane cache — resumes for the second.  Parameters, buffers, best_loss, momentum
buffers and the printed losses of epoch 1 must be equal; the same resume WITHOUT the flag must not be (momentum restarts, the rate
does not decay, the loader's stream restarts: what the flag is for); and the flag refuses a checkpoint that has no train_state."""
import contextlib
import io
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VARIANTS = {"eager-torch-sgd": [], "eager-hip-sgd": ["--train_optimizer", "hip"],
            "graph-hip-sgd": ["--train_graph", "1", "--train_optimizer", "hip"]}


def _video(n, hw, seed=5):
    g = torch.Generator().manual_seed(seed)
    base = torch.rand((n // 6 + 2, hw, hw, 3), generator=g)
    t = torch.linspace(0, n / 6, n)
    i0 = t.floor().long()
    fr = (t - i0.float()).view(-1, 1, 1, 1)
    return (((1 - fr) * base[i0] + fr * base[i0 + 1]).clamp(0, 1) * 255).to(torch.uint8)


def _run(root, name, extra, seed):
    """One cli() run in its own folder, from `seed` -> (stdout, the loaded *_latest checkpoint, its path)."""
    from avtex import train_ops
    from avtex.main import cli

    out_dir = root / name
    out_dir.mkdir()
    argv = ["-vdata", str(root / "videos"), "-vl", "clip", "-ea", "resnet10", "-m", "1", "-negs", "8", "-bs", "4", "-size", "32", "--size", "32",
            "-j", "0", "--lr", "0.01", "--lr_steps", "1", "--train_input", "device", "--train_deterministic", "-p", "1",
            "--logdir", str(out_dir / "logs"), "--ckpt", str(out_dir / "ckpt")] + extra
    cwd = os.getcwd()
    os.chdir(out_dir)
    np.random.seed(seed)
    torch.manual_seed(seed)
    torch.cuda.manual_seed(seed)
    train_ops.invalidate_weight_cache(drop=True)
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            cli(argv)
    finally:
        os.chdir(cwd)
        train_ops.set_deterministic(False)
    ck = [f for f in os.listdir(out_dir / "ckpt") if f.endswith("_latest.pth.tar")]
    assert len(ck) == 1
    path = out_dir / "ckpt" / ck[0]
    return buf.getvalue(), torch.load(path, map_location="cpu", weights_only=False), str(path)


def _losses(out, epoch):
    """The (val, avg) loss fields of the lines train() printed for `epoch`, as printed."""
    lines = [ln for ln in out.splitlines() if ln.startswith("Epoch: [%d][" % epoch)]
    return [re.search(r"Loss (\S+) \((\S+)\)", ln).groups() for ln in lines]


class _Runs:
    def __init__(self, root):
        self.root, self.first, self.whole = root, {}, {}
        (root / "videos").mkdir()
        np.savez(root / "videos" / "clip.npz", video=_video(124, 32).numpy(), fps=40.0)

    def first_epoch(self, variant):
        """Run B's first half: one epoch with --ckpt_train_state, from seed 0 (once per variant)."""
        if variant not in self.first:
            self.first[variant] = _run(self.root, "b1-" + variant, ["--epochs", "1", "--ckpt_train_state"] + VARIANTS[variant], 0)
        return self.first[variant]

    def uninterrupted(self, variant):
        """Run A: both epochs in one go, from seed 0 (once per variant)."""
        if variant not in self.whole:
            self.whole[variant] = _run(self.root, "a-" + variant, ["--epochs", "2", "--ckpt_train_state"] + VARIANTS[variant], 0)
        return self.whole[variant]


@pytest.fixture(scope="module")
def runs(tmp_path_factory, avt, dev):
    return _Runs(tmp_path_factory.mktemp("ckpt_resume"))


def _momentum(ck):
    st = ck["train_state"]["optimizer"]["state"]
    return {i: s["momentum_buffer"] for i, s in st.items() if s.get("momentum_buffer") is not None}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_a_resumed_run_equals_the_uninterrupted_one_bit_for_bit(avt, dev, runs, variant):
    how = VARIANTS[variant]
    out_a, a, _ = runs.uninterrupted(variant)
    out_b1, b1, path = runs.first_epoch(variant)
    assert b1["epoch"] == 1 and "train_state" in b1
    assert _losses(out_b1, 0) == _losses(out_a, 0) and len(_losses(out_a, 0)) == 3  # the two runs start alike
    out_b2, b, _ = _run(runs.root, "b2-" + variant, ["--epochs", "2", "--ckpt_train_state", "--resume", path] + how, 77)
    said = [ln for ln in out_b2.splitlines() if "restored the training state" in ln]
    assert len(said) == 1 and "learning rate 0.001" in said[0], out_b2[-2000:]  # epoch 1 trains at the decayed rate
    assert not _losses(out_b2, 0) and len(_losses(out_b2, 1)) == 3
    print("epoch-1 losses, uninterrupted: %s; resumed: %s" % (_losses(out_a, 1), _losses(out_b2, 1)))
    assert _losses(out_b2, 1) == _losses(out_a, 1)
    assert a["epoch"] == b["epoch"] == 2 and a["best_loss"] == b["best_loss"]
    sa, sb = a["state_dict"], b["state_dict"]
    assert list(sa) == list(sb) and len(sa) > 0
    assert any(k.endswith("running_mean") for k in sa) and any(k.endswith("num_batches_tracked") for k in sa)
    diff = [k for k in sa if not torch.equal(sa[k], sb[k])]
    assert not diff, diff[:5]
    ma, mb = _momentum(a), _momentum(b)
    assert set(ma) == set(mb) and len(ma) > 0
    assert all(torch.equal(ma[i], mb[i]) for i in ma), [i for i in ma if not torch.equal(ma[i], mb[i])][:5]
    ta, tb = a["train_state"], b["train_state"]
    assert ta["optimizer"]["param_groups"][0]["lr"] == tb["optimizer"]["param_groups"][0]["lr"]
    assert ta["scheduler"]["last_epoch"] == tb["scheduler"]["last_epoch"] == 1
    assert torch.equal(ta["loader"]["batcher"]["state"], tb["loader"]["batcher"]["state"])
    assert torch.equal(ta["torch_rng"], tb["torch_rng"])
    # the resumed epoch did change the model: equality above is not two copies of the checkpoint
    assert any(not torch.equal(b1["state_dict"][k], sb[k]) for k in sb if k.endswith("weight"))


def test_the_same_resume_without_the_flag_gives_other_parameters(avt, dev, runs):
    """The control: what --resume restores today (weights, epoch, best_loss) is not enough — this test can see what the flag fixes."""
    variant = "eager-torch-sgd"
    _, a, _ = runs.uninterrupted(variant)
    _, b1, path = runs.first_epoch(variant)
    out, c, _ = _run(runs.root, "control", ["--epochs", "2", "--resume", path], 0)
    assert len([ln for ln in out.splitlines() if "holds a train_state" in ln and "not used" in ln]) == 1
    assert "restored the training state" not in out and "train_state" not in c
    assert c["epoch"] == 2 and list(c["state_dict"]) == list(a["state_dict"])
    differ = [k for k in a["state_dict"] if not torch.equal(a["state_dict"][k], c["state_dict"][k])]
    assert len(differ) > 0


def test_the_flag_refuses_a_checkpoint_without_a_train_state(avt, dev, runs):
    _, b1, path = runs.first_epoch("eager-torch-sgd")
    bare = {k: v for k, v in b1.items() if k != "train_state"}
    stripped = str(runs.root / "stripped_latest.pth.tar")
    torch.save(bare, stripped)
    with pytest.raises(avt._lib.AvtError, match="holds no train_state"):
        _run(runs.root, "refused", ["--epochs", "2", "--ckpt_train_state", "--resume", stripped], 0)


def test_arena_sgd_momentum_keeps_its_layout_through_a_checkpoint(avt, dev, tmp_path):
    """ArenaSGD.load_state_dict after the state went through the host and a file: the momentum buffer of a channels-last weight still
    has its parameter's strides (step() checks that), and torch's SGD state loads into it."""
    from avtex import train_ops

    torch.manual_seed(3)
    w = torch.nn.Parameter(torch.randn(8, 4, 3, 3, 3, device=dev).contiguous(memory_format=torch.channels_last_3d))
    b = torch.nn.Parameter(torch.randn(8, device=dev))
    opt = train_ops.ArenaSGD([w, b], lr=0.1, momentum=0.9)
    for p in (w, b):
        p.grad = torch.randn_like(p)
    opt.step()
    torch.save({k: v for k, v in opt.state_dict().items()}, tmp_path / "opt.pth")
    want = [opt.state[p]["momentum_buffer"].clone() for p in (w, b)]
    sd = torch.load(tmp_path / "opt.pth", map_location="cpu", weights_only=False)
    sd["state"][0]["momentum_buffer"] = sd["state"][0]["momentum_buffer"].contiguous()  # the worst case: the layout was lost
    opt2 = train_ops.ArenaSGD([w, b], lr=0.1, momentum=0.9)
    opt2.load_state_dict(sd)
    for p, m in zip((w, b), want):
        buf = opt2.state[p]["momentum_buffer"]
        assert buf.is_cuda and train_ops._same_layout(buf, p) and torch.equal(buf, m)
    opt2.step()  # (its layout check passes)
    ref = torch.optim.SGD([w, b], lr=0.1, momentum=0.9)
    ref.load_state_dict(torch.load(tmp_path / "opt.pth", map_location="cpu", weights_only=False))
    assert all(torch.equal(ref.state[p]["momentum_buffer"], m) for p, m in zip((w, b), want))
