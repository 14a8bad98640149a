"""train() as a replayed HIP graph on EVERY rank (--train_graph 1 under torch.distributed.run): the graph ends with the backward and one
launch that packs the gradients (train_ops.GradExchange); one all-reduce and the optimizer follow every replay eagerly.  Two gloo ranks
share cuda:0 (RCCL refuses two ranks on one device).  The fixture of test_gpu_cli_train_hip_sgd (TinySlowFast, 32^2, window 5, stride 2):
three fixed global batches of 4 items per epoch, rank r trains on items [2r, 2r + 1] of each; two epochs, StepLR(step_size 1).

The reference is ONE process, eager, on the same global batches of 4 with bn_replicas = 2 (groups of consecutive items, running
statistics from group 0): its gradient is the mean over the same four items, its buffers are rank 0's.  The bound is the project's own
(test_gpu_cli_train_hip_sgd): max(1e-5 |a| + 1e-7 [parameters] / 1e-6 [buffers], 4 x floor |a|), floor = the largest relative difference
between two single-process eager runs from the same seeds, measured here.

Every GPU process is a child of this one with a timeout; this process itself makes no device call."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_DRIVER = r'''
import contextlib, io, os, sys
from types import SimpleNamespace
import numpy as np, torch
ROOT = %(root)r
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import avtex as avt
from avtex import dist as adist, train_ops
from tiny_encoders import TinySlowFast, seeded
from test_gpu_cli_train_hip_sgd import _video

mode, out = sys.argv[1], sys.argv[2]
BATCHES = [[0, 5, 9, 3], [12, 1, 7, 10], [4, 8, 2, 11]]   # fixed dataset indices: three global batches of 4 items


def cut(x, lo, hi):
    return [cut(v, lo, hi) for v in x] if isinstance(x, (list, tuple)) else x[lo:hi]


def run(dev, rank, world, kind, gamma, train_graph, bn_replicas):
    """Two epochs of avtex.train over a LIST loader (train() only iterates it and takes its len) -> what the rank ends with."""
    args = SimpleNamespace(vdata="/tmp", adata=None, n_negs=10, img_size=32, enc_arch="slowfast", window=0, stride=0,
                           print_freq=100, log_freq=100, train_graph=train_graph, bn_replicas=bn_replicas)
    torch.manual_seed(1)
    ds = avt.AudioVideoSegments(args, "x", split="train", video=(_video(), 10.0))
    assert len(ds) == 13
    np.random.seed(0)
    torch.manual_seed(2)
    full = [torch.utils.data.default_collate([ds[i] for i in idx]) for idx in BATCHES]   # the same draws in every process
    per = 4 // world
    loader = [cut(b, rank * per, (rank + 1) * per) for b in full]
    model = avt.ContrastivePredictionTemporal(seeded(TinySlowFast, 1), seeded(TinySlowFast, 2), None, 1, 128, temp=0.1,
                                              window=5, stride=2, enc_arch="slowfast", img_size=32).to(dev)
    if world > 1:
        with contextlib.redirect_stdout(io.StringIO()):
            train_ops.prepare_ranks(model)
    if kind == "hip":
        opt = train_ops.ArenaSGD(model.parameters(), lr=0.05, momentum=0.9)
    else:
        opt = torch.optim.SGD(model.parameters(), lr=0.05, momentum=0.9)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=gamma)
    train_ops.invalidate_weight_cache()
    losses, calls, after = [], [], []
    for epoch in range(2):
        before = dict(train_ops.CALLS)
        with contextlib.redirect_stdout(io.StringIO()):
            losses.append(avt.train(loader, model, opt, args, epoch))
        sched.step()
        torch.cuda.synchronize()
        calls.append({k: train_ops.CALLS[k] - before[k] for k in ("sgd_multi", "grad_pack_multi")})
        after.append([p.detach().cpu().clone() for p in model.parameters()])
    return {"losses": losses, "calls": calls, "params": after, "buffers": [b.detach().cpu().clone() for b in model.buffers()]}


if mode == "ranks":
    rank, world, local = adist.init_from_env(backend="gloo")
    assert world == 2
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {}
    for kind in ("hip", "torch"):
        for gamma in (0.1, 0.0):
            res[(kind, gamma)] = run(dev, rank, world, kind, gamma, 1, 1)
            print("rank %%d %%s gamma %%s: losses %%s calls %%s" %% (rank, kind, gamma, res[(kind, gamma)]["losses"], res[(kind, gamma)]["calls"]),
                  flush=True)
    torch.save(res, os.path.join(out, "rank%%d.pt" %% rank))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()
elif mode == "ref":
    dev = torch.device("cuda", 0)
    res = {}
    for kind in ("hip", "torch"):
        for again in (0, 1):
            res[(kind, again)] = run(dev, 0, 1, kind, 0.1, 0, 2)
            print("ref %%s run %%d: losses %%s" %% (kind, again, res[(kind, again)]["losses"]), flush=True)
    torch.save(res, os.path.join(out, "ref.pt"))
elif mode == "cli":
    from avtex.main import cli
    from avtex.models import ModelBuilder3D
    rank = int(os.environ["RANK"])
    os.chdir(out)
    ModelBuilder3D._plugins["slowfast"] = lambda img_size, window, pretrained: seeded(TinySlowFast, 1)
    np.random.seed(0)
    torch.manual_seed(0)
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            cli(["-vdata", os.path.join(out, "videos"), "-vl", "clip", "-ea", "slowfast", "-m", "1", "-negs", "10", "-bs", "4", "-size", "32",
                 "-j", "0", "--lr", "0.05", "--lr_steps", "1", "--epochs", "2", "--train_optimizer", "hip", "--train_graph", "1",
                 "--dist_backend", "gloo", "-p", "1", "--logdir", os.path.join(out, "logs"), "--ckpt", os.path.join(out, "ckpt")])
    finally:
        sys.stdout.write("".join("[r%%d] %%s\n" %% (rank, ln) for ln in buf.getvalue().splitlines()))
        sys.stdout.flush()
    torch.cuda.synchronize()
    print("[r%%d] CALLS sgd_multi %%d grad_pack_multi %%d" %% (rank, train_ops.CALLS["sgd_multi"], train_ops.CALLS["grad_pack_multi"]), flush=True)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()
'''


def _launch(script, mode, out, ranks, port):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, str(script), mode, str(out)]
    if ranks > 1:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
               "--master-port", str(port), str(script), mode, str(out)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-6000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-6000:])
    return r


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The two-rank runs (both optimizers, gamma 0.1 and 0) and the single-process reference, each computed once and shared."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = tmp_path_factory.mktemp("ranks")
    script = out / "driver.py"
    script.write_text(_DRIVER % {"root": ROOT})
    _launch(script, "ref", out, 1, 0)
    _launch(script, "ranks", out, 2, 29551)
    load = lambda name: torch.load(out / name, weights_only=False)  # noqa: E731
    return {"ref": load("ref.pt"), 0: load("rank0.pt"), 1: load("rank1.pt")}


def _rel(a, b):
    return float((a.double() - b.double()).abs().max()) / max(float(a.double().abs().max()), 1e-30)


@pytest.mark.parametrize("kind", ["hip", "torch"])
def test_parameters_are_bit_identical_across_the_ranks(runs, kind):
    """Both ranks apply the same all-reduced buffer to the same broadcast start; without the exchange (independent steps on different items)
    they drift apart."""
    for gamma in (0.1, 0.0):
        for epoch in (0, 1):
            a, b = runs[0][(kind, gamma)]["params"][epoch], runs[1][(kind, gamma)]["params"][epoch]
            assert len(a) == len(b) > 0 and all(torch.equal(x, y) for x, y in zip(a, b)), (kind, gamma, epoch)
    # (the ranks did see different items)
    assert runs[0][(kind, 0.1)]["losses"] != runs[1][(kind, 0.1)]["losses"]


@pytest.mark.parametrize("kind", ["hip", "torch"])
def test_ranks_equal_the_single_process_run_on_the_same_global_batches(runs, kind):
    """Rank 0's parameters and buffers and the mean of the ranks' first-epoch losses against one eager process on the batches of 4 — which
    also holds "one step per batch from the first batch": a first batch applied three times lands far outside the bound."""
    ra, rb = runs["ref"][(kind, 0)], runs["ref"][(kind, 1)]
    pe, be, le = ra["params"][1], ra["buffers"], ra["losses"]
    floor = max([_rel(a, b) for a, b in zip(pe + be, rb["params"][1] + rb["buffers"])] + [abs(le[0] - rb["losses"][0]) / abs(le[0])])
    g = runs[0][(kind, 0.1)]
    pg, bg = g["params"][1], g["buffers"]
    lg = [(x + y) / 2 for x, y in zip(g["losses"], runs[1][(kind, 0.1)]["losses"])]
    worst = max([_rel(a, b) for a, b in zip(pe + be, pg + bg)] + [abs(le[0] - lg[0]) / abs(le[0])])
    print("%s: eager-vs-eager floor %.3e, ranks-vs-one-process %.3e, bound max(1e-5 |a| + 1e-7 [parameters] / 1e-6 [buffers], %.3e |a|); "
          "losses one process %s ranks (mean) %s" % (kind, floor, worst, 4 * floor, le, lg))
    assert all(np.isfinite(le + lg)) and len(pe) == len(pg) > 0
    # (this fixture has NO buffers — TinySlowFast is linear layers only — so the buffer loop below compares nothing here; BatchNorm
    #  statistics, channels-last convolution weights and the plane re-make inside the capture are held to the eager loop by
    #  tests/test_gpu_grad_exchange_step.py)
    assert len(be) == len(bg) == 0
    assert abs(le[0] - lg[0]) <= max(1e-5 * max(1.0, abs(le[0])), 4 * floor * abs(le[0])), (le, lg)
    for a, b in zip(pe, pg):
        m = float(a.abs().max())
        assert float((a - b).abs().max()) <= max(1e-5 * m + 1e-7, 4 * floor * m), (floor, worst)
    for a, b in zip(be, bg):
        m = float(a.float().abs().max())
        assert float((a.float() - b.float()).abs().max()) <= max(1e-5 * m + 1e-6, 4 * floor * m), (floor, worst)


@pytest.mark.parametrize("kind", ["hip", "torch"])
def test_rate_zero_before_the_second_epoch_freezes_the_parameters(runs, kind):
    """StepLR(gamma = 0), no weight decay: the second epoch moves no bit of any parameter — with torch's SGD too, whose step is outside
    the capture here."""
    for rank in (0, 1):
        r = runs[rank][(kind, 0.0)]
        assert all(np.isfinite(r["losses"]))
        assert all(torch.equal(a, b) for a, b in zip(r["params"][0], r["params"][1])), (kind, rank)
        going = runs[rank][(kind, 0.1)]
        assert any(not torch.equal(a, b) for a, b in zip(r["params"][1], going["params"][1]))  # (the run with gamma 0.1 did go on training)


def test_launch_counts_per_rank(runs):
    """The optimizer is eager: one ArenaSGD launch per batch (plus the two warm-up steps of the one batch shape); the pack passes the host
    only in the warm-up steps and the capture, replays do not."""
    for rank in (0, 1):
        for gamma in (0.1, 0.0):
            hip, tor = runs[rank][("hip", gamma)]["calls"], runs[rank][("torch", gamma)]["calls"]
            assert [c["sgd_multi"] for c in hip] == [2 + 3, 3], hip
            assert [c["sgd_multi"] for c in tor] == [0, 0], tor
            for calls in (hip, tor):
                assert [c["grad_pack_multi"] for c in calls] == [2 + 1, 0], calls
    for kind in ("hip", "torch"):  # (the one-process eager reference never packs)
        assert all(c["grad_pack_multi"] == 0 for c in runs["ref"][(kind, 0)]["calls"])


def test_cli_trains_two_ranks_as_replayed_graphs(tmp_path):
    """python -m torch.distributed.run --nproc-per-node 2 main.py ... --train_graph 1 --train_optimizer hip --dist_backend gloo: both
    ranks run to the end, rank 0 prints the second epoch's losses and writes the checkpoint, and the model is not wrapped in
    DistributedDataParallel."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_gpu_cli_train_hip_sgd import _video

    (tmp_path / "videos").mkdir()
    np.savez(tmp_path / "videos" / "clip.npz", video=_video().numpy(), fps=10.0)
    script = tmp_path / "driver.py"
    script.write_text(_DRIVER % {"root": ROOT})
    out = _launch(script, "cli", tmp_path, 2, 29552).stdout
    r0 = [ln[5:] for ln in out.splitlines() if ln.startswith("[r0] ")]
    r1 = [ln[5:] for ln in out.splitlines() if ln.startswith("[r1] ")]
    assert any("train_optimizer='hip'" in ln and "dist_backend='gloo'" in ln for ln in r0) and "Training for 2 epochs." in r0
    lines = [ln for ln in r0 if ln.startswith("Epoch: [1][")]
    assert len(lines) == 3 and len([ln for ln in r1 if ln.startswith("Epoch: [1][")]) == 3, out[-3000:]
    assert all(np.isfinite(float(ln.split("Loss ")[1].split()[0])) for ln in lines)
    assert any(ln.startswith("prepare_ranks: 2 rank(s)") and "no DistributedDataParallel wrapper" in ln for ln in r0)
    assert not any(ln.startswith("prepare_ranks") for ln in r1) and "DistributedDataParallel(" not in out
    # two warm-up steps + six batches through the eager optimizer, two warm-up steps + the capture through the pack
    assert "CALLS sgd_multi 8 grad_pack_multi 3" in r0 and "CALLS sgd_multi 8 grad_pack_multi 3" in r1
    assert any(f.endswith("_latest.pth.tar") for f in os.listdir(tmp_path / "ckpt"))
