"""Training batches assembled on the device on EVERY rank (dataset.DeviceSegmentBatcher(rank, world), csrc/negsample.hip
avt_train_batch_plan): the kernel against NumPy's own stream (ds.sample_ids on the host, which fixture G9 pins to the reference), the
ranks' shares against the one-process batcher bit for bit, two gloo ranks sharing cuda:0 under --train_graph 1 against one eager process
on the same global batches, and the command line.

The two-rank runs follow tests/test_gpu_train_graph_ranks.py: every GPU process is a fresh child with a timeout, and the tests that
start them make no device call themselves.  Bound of the training comparison, unchanged from there: max(1e-5 |a| + 1e-7, 4 x floor |a|),
floor = the largest relative difference between two one-process eager runs from the same seeds, measured here and printed."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _u8(n, hw, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, hw, hw, 3), generator=g, dtype=torch.uint8)


def _state_words(st):
    return np.concatenate([np.asarray(st[1], np.uint32), np.array([st[2]], np.uint32)])


def _upload(st, dev):
    return torch.from_numpy(_state_words(st).view(np.int32).copy()).to(dev)


def _host_case(avt, ds, ids, seed):
    """The host's draws for all ids in order after np.random.seed(seed) -> the state before, [pos] + neg per item, the state after."""
    np.random.seed(seed)
    before = np.random.get_state()
    want = [ds.sample_ids(i) for i in ids]
    return {"ds": ds, "ids": ids, "before": before, "after": np.random.get_state(),
            "tgt": [[int(p)] + [int(v) for v in neg] for p, neg in want]}


@pytest.fixture(scope="module")
def long_case(avt):
    """746 items: 745 candidates per item are more than 624 draws, so every item, kept or skipped, crosses a state regeneration."""
    args = SimpleNamespace(vdata="/tmp", adata=None, n_negs=14, img_size=16, enc_arch="slowfast", window=0, stride=0)
    torch.manual_seed(5)
    ds = avt.AudioVideoSegments(args, "x", split="train", video=(_u8(3000, 16, 1), 20.0))
    n = len(ds)
    assert n == 746
    return _host_case(avt, ds, [0, n - 1, 1, n - 2, n // 2, 17, n - 5, 4], 7)


@pytest.fixture(scope="module")
def short_case(avt):
    """13 items, 10 negatives: 11 draws and up per item, 64 items with repeats: several items share one 624-word block and the
    regeneration falls between and inside items."""
    from test_gpu_cli_train_hip_sgd import _video

    args = SimpleNamespace(vdata="/tmp", adata=None, n_negs=10, img_size=32, enc_arch="slowfast", window=0, stride=0)
    torch.manual_seed(1)
    ds = avt.AudioVideoSegments(args, "x", split="train", video=(_video(), 10.0))
    assert len(ds) == 13
    ids = [int(v) for v in torch.randint(0, 13, (64,), generator=torch.Generator().manual_seed(9))]
    ids[:4] = [0, 12, 1, 11]
    case = _host_case(avt, ds, ids, 21)
    assert len(set(ids)) < 64 and case["before"][2] == 624  # a fresh seed: the first draw regenerates
    return case


def _check_plan(avt, dev, case, world, rank):
    ds, ids = case["ds"], case["ids"]
    per = len(ids) // world
    lo = rank * per
    idx = torch.tensor(ids, dtype=torch.int64, device=dev)
    state = _upload(case["before"], dev)
    tgt, starts = avt.ops.train_batch_plan(state, idx, lo, per, len(ds), ds.n_negs, ds.stride)
    assert tgt.shape == (per, 1 + ds.n_negs) and tgt.dtype == torch.int32 and starts.shape == (per * (2 + ds.n_negs),)
    assert tgt.cpu().tolist() == case["tgt"][lo : lo + per]
    # the composition DeviceSegmentBatcher._pack made before this entry existed: cat((idx, tgt.reshape(-1))) * stride as int32
    mine = idx[lo : lo + per]
    want = (torch.cat((mine, tgt.to(torch.int64).reshape(-1))) * ds.stride).to(torch.int32)
    assert starts.dtype == torch.int32 and torch.equal(starts, want)
    assert np.array_equal(state.cpu().numpy().view(np.uint32), _state_words(case["after"]))  # key and position after all B items
    return state


@pytest.mark.parametrize("world,rank", [(1, 0), (2, 0), (2, 1), (8, 0), (8, 7), (4, 2)])
def test_plan_follows_numpy_across_regenerations(avt, dev, long_case, world, rank):
    state = _check_plan(avt, dev, long_case, world, rank)
    # ... and the state of the existing sampler over the same 8 items, whose negatives are the plan's
    old = _upload(long_case["before"], dev)
    neg = avt.ops.negative_sample(old, torch.tensor(long_case["ids"], dtype=torch.int64, device=dev), len(long_case["ds"]), 14)
    assert torch.equal(old, state) and neg.cpu().tolist() == [row[1:] for row in long_case["tgt"]]


@pytest.mark.parametrize("rank", [0, 1, 2, 3])
def test_plan_with_many_short_items(avt, dev, short_case, rank):
    _check_plan(avt, dev, short_case, 4, rank)


def _raw_plan(avt, state, idx, keep_lo, keep_n, ds, tgt, starts):
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    status = avt._lib.lib().avt_train_batch_plan(p(state), p(idx), idx.numel(), keep_lo, keep_n, len(ds), ds.n_negs, ds.stride, p(tgt),
                                                 p(starts), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    avt._lib.check(status, "avt_train_batch_plan")
    torch.cuda.synchronize()


def test_plan_keeping_nothing_advances_the_stream_and_writes_nothing(avt, dev, long_case, short_case):
    for case in (long_case, short_case):
        ds = case["ds"]
        idx = torch.tensor(case["ids"], dtype=torch.int64, device=dev)
        state = _upload(case["before"], dev)
        tgt, starts = avt.ops.train_batch_plan(state, idx, 3, 0, len(ds), ds.n_negs, ds.stride)
        assert tgt.shape == (0, 1 + ds.n_negs) and starts.shape == (0,)
        assert np.array_equal(state.cpu().numpy().view(np.uint32), _state_words(case["after"]))
        # the raw entry over buffers of its own: keep_n = 0 leaves them alone; keep_n = 1 writes its row and nothing next to it
        row = 1 + ds.n_negs
        for keep_n in (0, 1):
            state = _upload(case["before"], dev)
            tgt = torch.full((3 * row,), -7, dtype=torch.int32, device=dev)
            starts = torch.full((3 * (row + 1),), -7, dtype=torch.int32, device=dev)
            _raw_plan(avt, state, idx, 3, keep_n, ds, tgt[row:], starts[row + 1 :])
            assert np.array_equal(state.cpu().numpy().view(np.uint32), _state_words(case["after"]))
            if keep_n == 0:
                assert bool((tgt == -7).all()) and bool((starts == -7).all())
            else:
                want = case["tgt"][3]
                assert tgt.cpu().tolist() == [-7] * row + want + [-7] * row
                assert starts.cpu().tolist() == [-7] * (row + 1) + [case["ids"][3] * ds.stride] + [v * ds.stride for v in want] + \
                    [-7] * (row + 1)


# ---- the batcher's shares against the one-process batcher ----------------------------------------------------------------------------
def _cat(parts):
    if parts[0] is None:
        assert all(p is None for p in parts)
        return None
    if isinstance(parts[0], (list, tuple)):
        return [torch.cat([p[k] for p in parts]) for k in range(len(parts[0]))]
    return torch.cat(parts)


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b)


@pytest.mark.parametrize("arch", ["slowfast", "resnet18"])
def test_shares_of_the_ranks_are_the_one_process_batch(avt, dev, arch):
    """rank / world given by hand in ONE process, no process group: each batcher starts from the same np.random state."""
    from avtex import synth
    from avtex.dataset import DeviceSegmentBatcher

    torch.manual_seed(5)
    if arch == "slowfast":  # 400 frames 24^2 -> 32^2, 9 negatives; audio examples of model type 2's rank (4 dimensions)
        args = SimpleNamespace(vdata="/tmp", adata=None, n_negs=9, img_size=32, enc_arch="slowfast", window=0, stride=0)
        ds = avt.AudioVideoSegments(args, "x", split="train", video=(_u8(400, 24, 2), 20.0))
        ds.audio_eg = torch.rand(len(ds) + 1, 1, 6, 4)
    else:  # the frame-table branch; the dummy [n, 10] audio examples, which only the loader delivers
        args = SimpleNamespace(vdata="/tmp", adata=None, n_negs=8, img_size=32, enc_arch="resnet18", window=0, stride=0)
        ds = avt.AudioVideoSegments(args, "x", split="train", video=(synth.structured_video(3, 120, 32, 32), 40.0))
    n = len(ds)
    ids = torch.tensor([0, n - 1, n // 2, 3])

    def fresh(rank, world):
        np.random.seed(11)
        return DeviceSegmentBatcher(ds, dev, rank=rank, world=world).seed_from_numpy()

    one = fresh(0, 1)
    want = one.batch(ids)
    assert (want[2] is not None) == (arch == "slowfast")
    one_l = fresh(0, 1)
    want_l = next(iter(one_l.loader(4, seed=5)))
    for world in (2, 4):
        bats = [fresh(r, world) for r in range(world)]
        got = [b.batch(ids) for b in bats]
        q0 = got[0][0][0] if arch == "slowfast" else got[0][0]
        assert q0.shape[0] == 4 // world
        for k in range(4):  # q frames, t frames, q audio examples, t audio examples
            assert _same(_cat([g[k] for g in got]), want[k]), (world, k)
        assert all(torch.equal(b.state, one.state) for b in bats)
        pos = [b.sample(ids) for b in bats]  # (a second global batch from the advanced stream)
        assert all(torch.equal(b.state, bats[0].state) for b in bats) and not torch.equal(bats[0].state, one.state)
        assert torch.cat([p[0] for p in pos]).cpu().tolist() == (ids + 1).tolist()
        # the loader form: the same epoch order from the seed, audio examples of either rank indexed with the rank's ids
        bats = [fresh(r, world) for r in range(world)]
        got_l = [next(iter(b.loader(4 // world, seed=5))) for b in bats]
        for k in (0, 2, 3, 5):
            assert _same(_cat([g[k] for g in got_l]), want_l[k]), (world, k)
        assert got_l[0][2].shape[0] == 4 // world and got_l[0][5].shape[:2] == (4 // world, 1 + ds.n_negs)
        assert all(torch.equal(b.state, one_l.state) for b in bats)
    with pytest.raises(ValueError):
        fresh(0, 3).batch(ids)  # 4 items over 3 ranks


# ---- two ranks under --train_graph 1 against one eager process -----------------------------------------------------------------------
_DRIVER = r'''
import contextlib, io, os, sys
from types import SimpleNamespace
import numpy as np, torch
ROOT = %(root)r
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import avtex as avt
from avtex import dist as adist, train_ops
from avtex.dataset import DeviceSegmentBatcher
from tiny_encoders import TinySlowFast, seeded
from test_gpu_cli_train_hip_sgd import _video

mode, out = sys.argv[1], sys.argv[2]


def run(dev, rank, world, train_graph, bn_replicas):
    """Two epochs of avtex.train over the device loader: 2 items per rank at world 2, 4 in one process -> what the process ends with."""
    args = SimpleNamespace(vdata="/tmp", adata=None, n_negs=10, img_size=32, enc_arch="slowfast", window=0, stride=0,
                           print_freq=100, log_freq=100, train_graph=train_graph, bn_replicas=bn_replicas)
    torch.manual_seed(1)
    ds = avt.AudioVideoSegments(args, "x", split="train", video=(_video(), 10.0))
    assert len(ds) == 13
    np.random.seed(0)
    bat = DeviceSegmentBatcher(ds, dev, rank=rank, world=world).seed_from_numpy()
    loader = bat.loader(4 // world, seed=7)
    assert len(loader) == 3
    model = avt.ContrastivePredictionTemporal(seeded(TinySlowFast, 1), seeded(TinySlowFast, 2), None, 1, 128, temp=0.1,
                                              window=5, stride=2, enc_arch="slowfast", img_size=32).to(dev)
    if world > 1:
        with contextlib.redirect_stdout(io.StringIO()):
            train_ops.prepare_ranks(model)
    opt = train_ops.ArenaSGD(model.parameters(), lr=0.05, momentum=0.9)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.1)
    train_ops.invalidate_weight_cache()
    losses, after = [], []
    for epoch in range(2):
        loader.sampler.set_epoch(epoch)
        with contextlib.redirect_stdout(io.StringIO()):
            losses.append(avt.train(loader, model, opt, args, epoch))
        sched.step()
        torch.cuda.synchronize()
        after.append([p.detach().cpu().clone() for p in model.parameters()])
    np.random.seed(12345)  # clobber, then take the device's stream back
    bat.sync_to_numpy()
    st = np.random.get_state()
    return {"losses": losses, "params": after, "mt_key": np.asarray(st[1]).copy(), "mt_pos": int(st[2])}


if mode == "ranks":
    rank, world, local = adist.init_from_env(backend="gloo")
    assert world == 2
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = run(dev, rank, world, 1, 1)
    print("rank %%d: losses %%s, stream position %%d" %% (rank, res["losses"], res["mt_pos"]), flush=True)
    torch.save(res, os.path.join(out, "rank%%d.pt" %% rank))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()
elif mode == "ref":
    dev = torch.device("cuda", 0)
    res = {}
    for again in (0, 1):
        res[again] = run(dev, 0, 1, 0, 2)
        print("ref run %%d: losses %%s, stream position %%d" %% (again, res[again]["losses"], res[again]["mt_pos"]), flush=True)
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
                 "--train_input", "device", "--dist_backend", "gloo", "-p", "1", "--logdir", os.path.join(out, "logs"),
                 "--ckpt", os.path.join(out, "ckpt")])
    finally:
        sys.stdout.write("".join("[r%%d] %%s\n" %% (rank, ln) for ln in buf.getvalue().splitlines()))
        sys.stdout.flush()
    torch.cuda.synchronize()
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()
'''


def _driver(tmp):
    from test_gpu_train_graph_ranks import _launch  # (fresh children with a timeout, HSA_ENABLE_IPC_MODE_LEGACY as set there)

    script = tmp / "driver.py"
    script.write_text(_DRIVER % {"root": ROOT})
    return script, _launch


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The two-rank run and the one-process reference (twice, for the floor), each computed once and shared."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = tmp_path_factory.mktemp("input_ranks")
    script, launch = _driver(out)
    launch(script, "ref", out, 1, 0)
    launch(script, "ranks", out, 2, 29561)
    load = lambda name: torch.load(out / name, weights_only=False)  # noqa: E731
    return {"ref": load("ref.pt"), 0: load("rank0.pt"), 1: load("rank1.pt")}


def _rel(a, b):
    return float((a.double() - b.double()).abs().max()) / max(float(a.double().abs().max()), 1e-30)


def test_two_ranks_hold_the_same_parameters_and_the_same_stream(runs):
    for epoch in (0, 1):
        a, b = runs[0]["params"][epoch], runs[1]["params"][epoch]
        assert len(a) == len(b) > 0 and all(torch.equal(x, y) for x, y in zip(a, b)), epoch
    assert runs[0]["losses"] != runs[1]["losses"]  # (the ranks did see different items)
    # every process walked the stream over every global batch: ranks and one-process runs end with one state
    for other in (runs[1], runs["ref"][0], runs["ref"][1]):
        assert np.array_equal(other["mt_key"], runs[0]["mt_key"]) and other["mt_pos"] == runs[0]["mt_pos"]
    np.random.seed(0)
    assert not np.array_equal(np.random.get_state()[1], runs[0]["mt_key"])  # (and it did move: 6 global batches of draws)


def test_two_ranks_train_like_one_process_on_the_global_batches(runs):
    """Rank 0's parameters and the mean of the ranks' first-epoch losses against one eager process whose device loader delivers the global
    batches of 4 from the same np.random seed and the same epoch orders."""
    ra, rb = runs["ref"][0], runs["ref"][1]
    pe, le = ra["params"][1], ra["losses"]
    floor = max([_rel(a, b) for a, b in zip(pe, rb["params"][1])] + [abs(le[0] - rb["losses"][0]) / abs(le[0])])
    pg = runs[0]["params"][1]
    lg = [(x + y) / 2 for x, y in zip(runs[0]["losses"], runs[1]["losses"])]
    worst = max([_rel(a, b) for a, b in zip(pe, pg)] + [abs(le[0] - lg[0]) / abs(le[0])])
    print("eager-vs-eager floor %.3e, ranks-vs-one-process %.3e, bound max(1e-5 |a| + 1e-7, %.3e |a|); losses one process %s ranks (mean) %s"
          % (floor, worst, 4 * floor, le, lg))
    assert all(np.isfinite(le + lg)) and len(pe) == len(pg) > 0
    assert abs(le[0] - lg[0]) <= max(1e-5 * max(1.0, abs(le[0])), 4 * floor * abs(le[0])), (le, lg)
    for a, b in zip(pe, pg):
        m = float(a.abs().max())
        assert float((a - b).abs().max()) <= max(1e-5 * m + 1e-7, 4 * floor * m), (floor, worst)
    assert any(not torch.equal(a, b) for a, b in zip(ra["params"][0], ra["params"][1]))  # (the second epoch went on training)


def test_cli_trains_two_ranks_from_device_assembled_batches(tmp_path):
    """python -m torch.distributed.run --nproc-per-node 2 main.py ... --train_input device --train_graph 1 --train_optimizer hip
    --dist_backend gloo -bs 4: both ranks run to the end (before the ranks could share the device path, main() raised ValueError)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from test_gpu_cli_train_hip_sgd import _video

    (tmp_path / "videos").mkdir()
    np.savez(tmp_path / "videos" / "clip.npz", video=_video().numpy(), fps=10.0)
    script, launch = _driver(tmp_path)
    out = launch(script, "cli", tmp_path, 2, 29562).stdout
    r0 = [ln[5:] for ln in out.splitlines() if ln.startswith("[r0] ")]
    r1 = [ln[5:] for ln in out.splitlines() if ln.startswith("[r1] ")]
    assert any("train_input='device'" in ln and "train_graph=1" in ln for ln in r0) and "Training for 2 epochs." in r0
    said = [ln for ln in r0 if "assembled on the device" in ln]
    assert len(said) == 1 and "world 2" in said[0] and "per-rank batch 2" in said[0] and "global batch 4" in said[0], r0
    assert "3 steps per epoch" in said[0] and not any("assembled on the device" in ln for ln in r1)
    lines = [ln for ln in r0 if ln.startswith("Epoch: [1][")]
    assert len(lines) == 3 and len([ln for ln in r1 if ln.startswith("Epoch: [1][")]) == 3, out[-3000:]
    assert all(np.isfinite(float(ln.split("Loss ")[1].split()[0])) for ln in lines)
    assert "Training for 2 epochs." in r1 and "DistributedDataParallel(" not in out
    assert any(f.endswith("_latest.pth.tar") for f in os.listdir(tmp_path / "ckpt"))
