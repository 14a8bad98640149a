"""--ckpt_async through main.main: the CLI recipe of test_gpu_train_deterministic_step.py, three epochs from one seed, once with the flag
and once without — *_latest.pth.tar and *_best.pth.tar load to equal tensors (keys, order, dtypes, shapes, strides) and equal best_loss,
every loaded tensor owns exactly its bytes, and nothing is in flight once cli() has returned; and the stream-ordering hazard: a snapshot
taken while a training side stream still has work queued holds what that work wrote."""
import contextlib
import io
import os
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _video(n, hw, seed=5):
    g = torch.Generator().manual_seed(seed)
    base = torch.rand((n // 6 + 2, hw, hw, 3), generator=g)
    t = torch.linspace(0, n / 6, n)
    i0 = t.floor().long()
    fr = (t - i0.float()).view(-1, 1, 1, 1)
    return (((1 - fr) * base[i0] + fr * base[i0 + 1]).clamp(0, 1) * 255).to(torch.uint8)


def _run(root, name, extra):
    from avtex import train_ops
    from avtex.main import cli

    out_dir = root / name
    out_dir.mkdir()
    argv = ["-vdata", str(root / "videos"), "-vl", "clip", "-ea", "resnet10", "-m", "1", "-negs", "8", "-bs", "4", "-size", "32", "--size", "32",
            "-j", "0", "--lr", "0.01", "--epochs", "3", "--train_input", "device", "--train_deterministic", "-p", "1",
            "--logdir", str(out_dir / "logs"), "--ckpt", str(out_dir / "ckpt")] + extra
    cwd = os.getcwd()
    os.chdir(out_dir)
    np.random.seed(0)
    torch.manual_seed(0)
    train_ops.invalidate_weight_cache(drop=True)
    before = train_ops.CALLS["state_copy_multi"]
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            cli(argv)
    finally:
        os.chdir(cwd)
        train_ops.set_deterministic(False)
    # nothing in flight: the writer's thread has ended, no temporary file is left, both files are there
    assert not [t for t in threading.enumerate() if t.name == "avt-checkpoint-writer"]
    files = sorted(os.listdir(out_dir / "ckpt"))
    assert len(files) == 2 and files[0].endswith("_best.pth.tar") and files[1].endswith("_latest.pth.tar"), files
    return [torch.load(out_dir / "ckpt" / f, map_location="cpu", weights_only=False) for f in files], train_ops.CALLS["state_copy_multi"] - before


@pytest.mark.parametrize("extra", [[], ["--ckpt_train_state", "--train_optimizer", "hip"]], ids=["weights", "with-train-state"])
def test_async_checkpoints_equal_the_synchronous_ones(avt, dev, tmp_path, extra):
    (tmp_path / "videos").mkdir()
    np.savez(tmp_path / "videos" / "clip.npz", video=_video(124, 32).numpy(), fps=40.0)
    sync, launches = _run(tmp_path, "sync", extra)
    assert launches == 0
    asyn, launches = _run(tmp_path, "async", extra + ["--ckpt_async"])
    assert launches == 3  # one launch per epoch-end save
    for a, s in zip(asyn, sync):  # best, latest
        assert list(a) == list(s) == ["epoch", "arch", "state_dict", "best_loss"] + (["train_state"] if extra else [])
        assert (a["epoch"], a["arch"], a["best_loss"]) == (s["epoch"], s["arch"], s["best_loss"])
        sa, ss = a["state_dict"], s["state_dict"]
        assert type(sa) is type(ss) and list(sa) == list(ss) and len(sa) > 0 and sa._metadata == ss._metadata
        for k in sa:
            assert sa[k].dtype == ss[k].dtype and sa[k].shape == ss[k].shape and sa[k].stride() == ss[k].stride(), k
            assert torch.equal(sa[k], ss[k]), k
            assert sa[k].untyped_storage().nbytes() == sa[k].numel() * sa[k].element_size(), k  # not the whole pinned buffer
        if extra:
            ta, ts = a["train_state"], s["train_state"]
            assert list(ta) == list(ts) and ta["optimizer"]["param_groups"] == ts["optimizer"]["param_groups"]
            assert ta["scheduler"] == ts["scheduler"] and ta["world"] == ts["world"] == 1 and ta["train_deterministic"] is True
            assert torch.equal(ta["torch_rng"], ts["torch_rng"]) and torch.equal(ta["device_rng"], ts["device_rng"])
            assert torch.equal(ta["loader"]["batcher"]["state"], ts["loader"]["batcher"]["state"])
            ma, ms = ta["optimizer"]["state"], ts["optimizer"]["state"]
            assert list(ma) == list(ms) and len(ma) > 0
            for i in ma:
                x, y = ma[i]["momentum_buffer"], ms[i]["momentum_buffer"]
                assert x.stride() == y.stride() and torch.equal(x, y), i
                assert x.untyped_storage().nbytes() == x.numel() * x.element_size(), i
    assert asyn[1]["epoch"] == 3


def test_a_snapshot_waits_for_the_training_side_streams(avt, dev):
    """The query encoder's BatchNorm buffers are written on a side stream.  With work still queued there — a chain of large products,
    then the buffer's update — take() on the step's own stream must hold the updated buffer, as a clone after a device-wide
    synchronisation does."""
    from avtex import models, ops, train_ops

    bn = torch.nn.BatchNorm3d(16).to(dev)
    named = [(k, v) for k, v in bn.state_dict().items()]
    snap = train_ops.StateSnapshot(named)
    side = ops.side_streams(dev, 1)[0]
    assert any(s == side for s in models.training_side_streams(dev))
    a = torch.randn(4096, 4096, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(24):
            a = (a @ a).clamp_(-1, 1)  # a few tens of milliseconds of queued work
        bn.running_mean.add_(a[0, :16].abs() + 1)
        bn.num_batches_tracked.add_(5)
    h = snap.take()  # issued at once, while the side stream is still busy
    busy = not side.query()
    views = h.wait()
    torch.cuda.synchronize()
    want = {k: v.clone().cpu() for k, v in bn.state_dict().items()}
    assert int(want["num_batches_tracked"]) == 5 and bool((want["running_mean"] >= 1).all())
    for k in want:
        assert torch.equal(views[k], want[k]), k
    h.release()
    assert busy, "the side stream had finished before take() was issued: the test did not exercise the ordering"
