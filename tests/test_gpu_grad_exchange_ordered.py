"""The ORDERED gradient exchange (train_ops.GradExchange(ordered=True): one all-gather, then csrc/rank_sum.hip adds the ranks' buffers in
ascending rank order) and what it buys: training that repeats bit for bit ACROSS ranks, and resumes exactly.  Three gloo ranks share
cuda:0 (RCCL refuses several ranks on one device) — three, because with two the one fp32 add is commutative and no test can see an order.

(a) the exchange alone, on gradients with exponents 40 binades apart: every rank's buffer equals the host chain
    fl(fl(fl(g0 s) + fl(g1 s)) + fl(g2 s)), s = float32(1 / 3), bit for bit; handing the gradients out in another order changes bits.
(b) main.cli at world 3 with --train_deterministic (the recipe of test_gpu_train_deterministic_step.py: resnet10 at 32^2, --train_input
    device; a global batch of 3, two epochs across a learning-rate decay), eagerly and as replayed graphs with the HIP optimizer: two runs
    from one seed give rank 0 the same checkpoint and every rank the same losses, and all ranks end with the same parameters.
(c) the same run interrupted after the first epoch and resumed with --ckpt_train_state: rank 0's final checkpoint and every rank's
    second-epoch losses equal the uninterrupted run's.

Every GPU process is a child of this one with a timeout; this process itself makes no device call.  One launch serves (a), one (b) and (c)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD = 3
SHAPES = [(1,), (3,), (4,), (4097,), (6, 4, 2, 3, 3), (5,)]  # the 5-D one is a channels-last weight; the last one gets no gradient
PERMUTED = [2, 0, 1]  # the second hand-out: rank r packs the gradients rank PERMUTED[r] had
FORMS = {"eager": [], "graph": ["--train_graph", "1", "--train_optimizer", "hip"]}

_DRIVER = r'''
import contextlib, hashlib, io, os, sys
import numpy as np, torch
ROOT = %(root)r
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import avtex as avt
import torch.distributed as dist
from avtex import dist as adist, train_ops

mode, out = sys.argv[1], sys.argv[2]
SHAPES, PERMUTED = %(shapes)r, %(permuted)r
rank, world, local = adist.init_from_env(backend="gloo")
assert world == 3
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)


def gradient(r, k, shape):
    """Seeded by (rank, index): randn * 2^randint(-20, 20) per element, in the parameter's memory format."""
    g = torch.Generator().manual_seed(1000 * r + k)
    v = torch.randn(shape, generator=g) * torch.exp2(torch.randint(-20, 21, shape, generator=g).float())
    v = v.to(dev)
    return v.contiguous(memory_format=torch.channels_last_3d) if len(shape) == 5 else v


def exchange_once(ordered, source):
    """bind, pack, exchange, install on fresh parameters whose gradients are rank `source`'s -> what the test compares."""
    params = [torch.nn.Parameter(torch.zeros(s, device=dev)) for s in SHAPES]
    params[4].data = params[4].data.contiguous(memory_format=torch.channels_last_3d)
    for k, p in enumerate(params[:-1]):
        p.grad = gradient(source, k, SHAPES[k])
    ex = train_ops.GradExchange(params, world, ordered=ordered)
    ex.bind()
    ex.pack()
    before, reduces = dict(train_ops.CALLS), []
    real = dist.all_reduce
    dist.all_reduce = lambda *a, **k: (reduces.append(1), real(*a, **k))[1]
    try:
        ex.all_reduce() if not ordered else ex.exchange()
    finally:
        dist.all_reduce = real
    ex.install()
    torch.cuda.synchronize()
    views = all(p.grad.data_ptr() == v.data_ptr() == ex.flat.data_ptr() + 4 * o and p.grad.shape == p.shape and p.grad.stride() == p.stride()
                for p, v, o in zip(ex.params, ex.views, ex.offsets))
    return {"flat": ex.flat.cpu().clone(), "offsets": list(ex.offsets), "total": ex.total, "bound": len(ex.params), "views": views,
            "no_grad_left_alone": params[-1].grad is None, "parts_shape": None if ex.parts is None else tuple(ex.parts.shape),
            "all_reduces": len(reduces), "rank_sums": train_ops.CALLS["rank_sum"] - before["rank_sum"],
            "grads": [p_.cpu().clone() for p_ in (gradient(source, k, SHAPES[k]) for k in range(len(SHAPES) - 1))]}


if mode == "exchange":
    res = {"ordered": exchange_once(True, rank), "permuted": exchange_once(True, PERMUTED[rank]), "unordered": exchange_once(False, rank)}
    # all_reduce() keeps its name: on an ordered exchange it IS the exchange
    train_ops.set_deterministic(True)
    try:
        params = [torch.nn.Parameter(torch.zeros(7, device=dev))]
        params[0].grad = gradient(rank, 0, (7,))
        ex = train_ops.GradExchange(params, world)  # ordered=None: what deterministic() says at bind()
        ex.bind()
        ex.pack()
        n0 = train_ops.CALLS["rank_sum"]
        ex.all_reduce()
        res["default"] = {"ordered": ex.ordered, "rank_sums": train_ops.CALLS["rank_sum"] - n0, "flat": ex.flat.cpu().clone()}
    finally:
        train_ops.set_deterministic(False)
    torch.save(res, os.path.join(out, "exchange.rank%%d.pt" %% rank))
elif mode == "cli":
    import avtex.main as main_mod
    real_train = main_mod.train

    def one(name, extra, seed):
        """One cli() run on all ranks, from `seed` -> rank 0's checkpoint path.  Each rank leaves <name>.rank<r>.pt: its log, its
        epochs' mean losses as train() returned them, a hash of its final parameters and its launch counts."""
        run = os.path.join(out, name)
        os.makedirs(run, exist_ok=True)
        os.chdir(run)  # (main() makes ./ckpt: the folder --ckpt names below)
        np.random.seed(seed)
        torch.manual_seed(seed)
        torch.cuda.manual_seed(seed)
        train_ops.invalidate_weight_cache(drop=True)
        seen = {"losses": []}

        def train(loader, model, *a, **k):
            seen["model"] = model
            seen["losses"].append(real_train(loader, model, *a, **k))
            return seen["losses"][-1]

        main_mod.train = train
        before, buf = dict(train_ops.CALLS), io.StringIO()
        try:
            with contextlib.redirect_stdout(buf):
                main_mod.cli(["-vdata", os.path.join(out, "videos"), "-vl", "clip", "-ea", "resnet10", "-m", "1", "-negs", "8", "-bs", "3",
                              "-size", "32", "--size", "32", "-j", "0", "--lr", "0.01", "--lr_steps", "1", "--train_input", "device",
                              "--train_deterministic", "--ckpt_train_state", "--dist_backend", "gloo", "-p", "1",
                              "--logdir", os.path.join(run, "logs"), "--ckpt", os.path.join(run, "ckpt")] + extra)
        finally:
            main_mod.train = real_train
            train_ops.set_deterministic(False)
            sys.stdout.write("".join("[%%s r%%d] %%s\n" %% (name, rank, ln) for ln in buf.getvalue().splitlines()))
            sys.stdout.flush()
        torch.cuda.synchronize()
        h = hashlib.sha256()
        for p in seen["model"].parameters():
            h.update(p.detach().cpu().contiguous().numpy().tobytes())
        torch.save({"log": buf.getvalue(), "losses": seen["losses"], "hash": h.hexdigest(), "ddp": hasattr(seen["model"], "module"),
                    "calls": {k: train_ops.CALLS[k] - before[k] for k in ("rank_sum", "sgd_multi", "grad_pack_multi")}},
                   os.path.join(out, "%%s.rank%%d.pt" %% (name, rank)))
        dist.barrier()  # (rank 0's checkpoint is on disk before any rank goes on)
        ck = [f for f in os.listdir(os.path.join(run, "ckpt")) if f.endswith("_latest.pth.tar")]
        assert len(ck) == 1, ck
        return os.path.join(run, "ckpt", ck[0])

    for form, how in %(forms)r.items():
        one("a1-" + form, ["--epochs", "2"] + how, 0)
        one("a2-" + form, ["--epochs", "2"] + how, 0)
        half = one("b1-" + form, ["--epochs", "1"] + how, 0)
        one("b2-" + form, ["--epochs", "2", "--resume", half] + how, 77)
dist.barrier()
dist.destroy_process_group()
'''


def _launch(tmp, mode, port, timeout):
    script = tmp / "driver.py"
    script.write_text(_DRIVER % {"root": ROOT, "shapes": SHAPES, "permuted": PERMUTED, "forms": FORMS})
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(WORLD), "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(script), mode, str(tmp)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-8000:])
    if r.returncode != 0:
        print(r.stderr[-8000:])  # (whole lines: the assertion's own report shortens them)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-6000:])


# ---- (a) the exchange -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exchanged(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    tmp = tmp_path_factory.mktemp("ordered_exchange")
    _launch(tmp, "exchange", 29571, 300)
    return [torch.load(tmp / ("exchange.rank%d.pt" % r), weights_only=False) for r in range(WORLD)]


def _layout():
    from avtex import train_ops

    return train_ops.exchange_layout([int(np.prod(s)) for s in SHAPES[:-1]])


def _terms(grads_of_rank):
    """One rank's packed buffer as the host computes it: fl(g * float32(1 / 3)) at exchange_layout's offsets, a channels-last weight in
    its memory order, zeros in the padding."""
    offsets, total = _layout()
    flat = np.zeros(total, np.float32)
    s = np.float32(1.0 / WORLD)
    for g, o in zip(grads_of_rank, offsets):
        mem = g.permute(0, 2, 3, 4, 1) if g.dim() == 5 else g  # channels-last: the channel is the innermost axis in memory
        flat[o : o + g.numel()] = mem.contiguous().numpy().reshape(-1) * s
    return flat


def _chain(terms, order):
    s = terms[order[0]].copy()
    for r in order[1:]:
        s = (s + terms[r]).astype(np.float32)
    return s


def _bits(t):
    return (t.numpy() if isinstance(t, torch.Tensor) else t).view(np.int32)


def test_every_rank_holds_the_ascending_chain_bit_for_bit(exchanged):
    offsets, total = _layout()
    assert total == 4 + 4 + 4 + 4100 + 432
    terms = [_terms(exchanged[r]["ordered"]["grads"]) for r in range(WORLD)]
    want = _chain(terms, [0, 1, 2])
    assert not np.array_equal(_bits(_chain(terms, [2, 1, 0])), _bits(want))  # (the input can tell the orders apart)
    for r in range(WORLD):
        res = exchanged[r]["ordered"]
        assert res["offsets"] == offsets and res["total"] == total and res["bound"] == len(SHAPES) - 1
        assert res["parts_shape"] == (WORLD, total) and res["rank_sums"] == 1 and res["all_reduces"] == 0
        assert res["views"] and res["no_grad_left_alone"]
        assert np.array_equal(_bits(res["flat"]), _bits(exchanged[0]["ordered"]["flat"])), "rank %d differs from rank 0" % r
        bad = np.nonzero(_bits(res["flat"]) != _bits(want))[0]
        assert bad.size == 0, (r, bad.size, bad[:8])
    flat = exchanged[0]["ordered"]["flat"].numpy()
    pad = np.ones(total, bool)
    for s, o in zip(SHAPES[:-1], offsets):
        pad[o : o + int(np.prod(s))] = False
    assert pad.sum() == 3 + 1 + 0 + 3 + 0 and not flat[pad].any() and flat[~pad].all()  # the padding stays zero, nothing else is


def test_another_hand_out_of_the_gradients_changes_bits(exchanged):
    """Rank r packs what rank PERMUTED[r] had: the same three terms per element, added in another order."""
    terms = [_terms(exchanged[r]["ordered"]["grads"]) for r in range(WORLD)]
    for r in range(WORLD):  # (the driver did hand them out that way)
        assert all(torch.equal(a, b) for a, b in zip(exchanged[r]["permuted"]["grads"], exchanged[PERMUTED[r]]["ordered"]["grads"]))
    want = _chain(terms, PERMUTED)
    for r in range(WORLD):
        assert np.array_equal(_bits(exchanged[r]["permuted"]["flat"]), _bits(want)), r
    changed = int((_bits(exchanged[0]["permuted"]["flat"]) != _bits(exchanged[0]["ordered"]["flat"])).sum())
    print("%d of %d elements change with the order of the ranks" % (changed, want.size))
    assert changed >= 1


def test_the_unordered_exchange_is_one_all_reduce_and_no_sum_launch(exchanged):
    terms = [_terms(exchanged[r]["unordered"]["grads"]).astype(np.float64) for r in range(WORLD)]
    exact, mass = sum(terms), sum(np.abs(t) for t in terms)
    for r in range(WORLD):
        res = exchanged[r]["unordered"]
        assert res["all_reduces"] == 1 and res["rank_sums"] == 0 and res["parts_shape"] is None and res["views"]
        # whatever order the backend adds three fp32 terms in: two roundings, each at most 2^-24 of a partial sum <= the terms' mass
        assert (np.abs(res["flat"].numpy().astype(np.float64) - exact) <= 2.0 ** -23 * mass).all()


def test_ordered_defaults_to_the_deterministic_mode_and_all_reduce_keeps_its_name(exchanged):
    for r in range(WORLD):
        res = exchanged[r]["default"]
        assert res["ordered"] is True and res["rank_sums"] == 1
        assert torch.equal(res["flat"], exchanged[0]["default"]["flat"])


# ---- (b), (c) through main.cli ----------------------------------------------------------------------------------------------------------
def _video(n, hw, seed=5):
    g = torch.Generator().manual_seed(seed)
    base = torch.rand((n // 6 + 2, hw, hw, 3), generator=g)
    t = torch.linspace(0, n / 6, n)
    i0 = t.floor().long()
    fr = (t - i0.float()).view(-1, 1, 1, 1)
    return (((1 - fr) * base[i0] + fr * base[i0 + 1]).clamp(0, 1) * 255).to(torch.uint8)


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """Per form: runs a1 and a2 (two epochs, one seed), b1 (one epoch) and b2 (resumed from b1 for the second, from other seeds) ->
    {run name: {"ranks": [what each rank left], "ckpt": rank 0's checkpoint}}."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    tmp = tmp_path_factory.mktemp("ordered_cli")
    (tmp / "videos").mkdir()
    np.savez(tmp / "videos" / "clip.npz", video=_video(124, 32).numpy(), fps=40.0)  # 12 items: 4 global batches of 3 per epoch
    _launch(tmp, "cli", 29572, 1500)
    runs = {}
    for form in FORMS:
        for name in ("a1-", "a2-", "b1-", "b2-"):
            ck = [f for f in os.listdir(tmp / (name + form) / "ckpt") if f.endswith("_latest.pth.tar")]
            assert len(ck) == 1
            runs[name + form] = {"ranks": [torch.load(tmp / ("%s%s.rank%d.pt" % (name, form, r)), weights_only=False) for r in range(WORLD)],
                                 "ckpt": torch.load(tmp / (name + form) / "ckpt" / ck[0], map_location="cpu", weights_only=False)}
    return runs


def _losses(log, epoch):
    """The (val, avg) loss fields of the lines train() printed for `epoch`, as printed."""
    lines = [ln for ln in log.splitlines() if ln.startswith("Epoch: [%d][" % epoch)]
    return [re.search(r"Loss (\S+) \((\S+)\)", ln).groups() for ln in lines]


def _momentum(ck):
    st = ck["train_state"]["optimizer"]["state"]
    return {i: s["momentum_buffer"] for i, s in st.items() if s.get("momentum_buffer") is not None}


def _same_checkpoint(a, b):
    sa, sb = a["state_dict"], b["state_dict"]
    assert list(sa) == list(sb) and len(sa) > 0 and any(k.endswith("running_mean") for k in sa)
    diff = [k for k in sa if not torch.equal(sa[k], sb[k])]  # parameters and buffers
    assert not diff, (len(diff), diff[:5])
    ma, mb = _momentum(a), _momentum(b)
    assert set(ma) == set(mb) and len(ma) > 0
    assert all(torch.equal(ma[i], mb[i]) for i in ma), [i for i in ma if not torch.equal(ma[i], mb[i])][:5]
    assert a["epoch"] == b["epoch"] and a["best_loss"] == b["best_loss"]


@pytest.mark.parametrize("form", list(FORMS))
def test_two_runs_from_one_seed_repeat_across_ranks(trained, form):
    a1, a2 = trained["a1-" + form], trained["a2-" + form]
    _same_checkpoint(a1["ckpt"], a2["ckpt"])
    for r in range(WORLD):
        x, y = a1["ranks"][r], a2["ranks"][r]
        assert len(_losses(x["log"], 0)) == len(_losses(x["log"], 1)) == 4
        assert all(_losses(x["log"], e) == _losses(y["log"], e) for e in (0, 1)), r
        assert all(np.isfinite(x["losses"])) and len(x["losses"]) == 2 and x["losses"] == y["losses"], (r, x["losses"], y["losses"])
        assert x["hash"] == y["hash"]
    for run in (a1, a2):  # all ranks end with the same parameters
        assert len({run["ranks"][r]["hash"] for r in range(WORLD)}) == 1
    # (the ranks did see different items, and the second epoch went on training)
    assert len({tuple(a1["ranks"][r]["losses"]) for r in range(WORLD)}) == WORLD
    assert trained["b1-" + form]["ranks"][0]["hash"] != a1["ranks"][0]["hash"]


@pytest.mark.parametrize("form", list(FORMS))
def test_the_log_shows_the_ranks_form_and_the_launch_counts(trained, form):
    run = trained["a1-" + form]
    log0 = run["ranks"][0]["log"]
    assert any(ln.startswith("prepare_ranks: 3 rank(s)") and "no DistributedDataParallel wrapper" in ln for ln in log0.splitlines())
    said = [ln for ln in log0.splitlines() if "deterministic weight gradients" in ln]
    assert len(said) == 1 and "summed in rank order" in said[0] and "one world size, one build and one GPU type" in said[0], said
    steps = 2 * 4 + (2 if form == "graph" else 0)  # two epochs of four global batches; the graph's two warm-up steps are whole steps
    for r in range(WORLD):
        res = run["ranks"][r]
        assert "DistributedDataParallel(" not in res["log"] and not res["ddp"]
        assert "the all-reduce's order is the backend's" not in res["log"]
        assert res["calls"]["rank_sum"] == steps, res["calls"]
        if form == "graph":  # (the HIP optimizer: one launch per optimizer step, each after one sum)
            assert res["calls"]["sgd_multi"] == steps and res["calls"]["grad_pack_multi"] == 3, res["calls"]
        else:
            assert res["calls"]["sgd_multi"] == 0 and res["calls"]["grad_pack_multi"] == steps, res["calls"]


@pytest.mark.parametrize("form", list(FORMS))
def test_a_run_resumed_at_the_same_world_size_equals_the_uninterrupted_one(trained, form):
    a, b1, b2 = trained["a1-" + form], trained["b1-" + form], trained["b2-" + form]
    assert b1["ckpt"]["epoch"] == 1 and b1["ckpt"]["train_state"]["world"] == WORLD
    said = [ln for ln in b2["ranks"][0]["log"].splitlines() if "restored the training state" in ln]
    assert len(said) == 1 and "learning rate 0.001" in said[0]  # the second epoch trains at the decayed rate
    assert "will not repeat it bit for bit" not in b2["ranks"][0]["log"]
    _same_checkpoint(a["ckpt"], b2["ckpt"])
    for r in range(WORLD):
        x, y = a["ranks"][r], b2["ranks"][r]
        assert not _losses(y["log"], 0) and len(_losses(y["log"], 1)) == 4
        assert _losses(y["log"], 1) == _losses(x["log"], 1), r
        assert len(y["losses"]) == 1 and y["losses"][0] == x["losses"][1], (r, x["losses"], y["losses"])
        assert y["hash"] == x["hash"]
    # the resumed epoch did change the model: equality above is not two copies of b1's checkpoint
    sb = b2["ckpt"]["state_dict"]
    assert any(not torch.equal(b1["ckpt"]["state_dict"][k], sb[k]) for k in sb if k.endswith("weight"))
