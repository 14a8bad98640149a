"""The rank-aware device input path, the parts that need no device: the loader's arithmetic over ranks (a stub batcher whose _pack returns
the rank's ids), the binding and the argument checks of avt_train_batch_plan, and main()'s loader branch for --train_input device under
several ranks (stub batcher, no process group)."""
import re
from types import SimpleNamespace

import pytest
import torch


class _Items:
    """What the loader reads of a dataset: its length, and audio examples whose row i holds i."""

    def __init__(self, n):
        self.n, self.split = n, "train"
        self.audio_eg = torch.arange(n + 1, dtype=torch.int64).view(n + 1, 1)

    def __len__(self):
        return self.n


def _stub(avt, n, rank=0, world=1):
    """A DeviceSegmentBatcher without a device: share() and loader() are the real ones; _pack returns the rank's ids as its frames."""
    from avtex.dataset import DeviceSegmentBatcher

    class Stub(DeviceSegmentBatcher):
        def __init__(self):  # (no video, no device)
            self.ds, self.dev, self.rank, self.world = _Items(n), torch.device("cpu"), rank, world
            self.audio_eg, self._audio_any = None, None

        def _pack(self, idx):
            mine = self.share(idx)
            return mine.clone(), None, (mine + 1).view(-1, 1)

    return Stub()


def _epoch(loader):
    """-> the ids of every step, from the frames field and (the same) from the query audio rows."""
    steps = []
    for q_frames, q_wav, q_ae, t_frames, t_wav, t_ae in loader:
        assert q_wav is None and t_wav is None and t_frames is None
        assert q_ae.view(-1).tolist() == q_frames.tolist() and t_ae.view(-1).tolist() == (q_frames + 1).tolist()
        steps.append(q_frames.tolist())
    return steps


@pytest.mark.parametrize("n,per,world", [(13, 2, 2), (13, 1, 4), (746, 1, 8)])
def test_ranks_cut_the_one_process_batches(avt, n, per, world):
    one = _stub(avt, n).loader(per * world, seed=7)
    ranks = [_stub(avt, n, r, world).loader(per, seed=7) for r in range(world)]
    assert one.sampler is one and all(ld.sampler is ld for ld in ranks)
    orders = []
    for epoch in (0, 1):
        for ld in [one] + ranks:
            ld.sampler.set_epoch(epoch)
        want = _epoch(one)
        got = [_epoch(ld) for ld in ranks]
        assert len(one) == len(want) == n // (per * world) > 0
        for r, g in enumerate(got):
            assert len(ranks[r]) == len(g) == n // (per * world)
            assert all(len(step) == per for step in g)
        for s, step in enumerate(want):
            assert sum((g[s] for g in got), []) == step  # rank k // per holds item k: the contiguous scatter
        flat = sum(want, [])
        assert len(set(flat)) == len(flat) and set(flat) <= set(range(n))  # every id at most once per epoch (the tail is dropped)
        assert _epoch(one) == want  # the same seed and epoch give the same order again
        orders.append(flat)
    assert orders[0] != orders[1]  # set_epoch changes the order
    again = _stub(avt, n, world - 1, world).loader(per, seed=7)
    again.set_epoch(1)
    assert _epoch(again) == [g for g in got[world - 1]]
    other = _stub(avt, n).loader(per * world, seed=8)
    assert sum(_epoch(other), []) != orders[0]


def test_one_process_without_a_seed_keeps_the_global_generator(avt):
    ld = _stub(avt, 13).loader(4)
    torch.manual_seed(3)
    got = sum(_epoch(ld), [])
    torch.manual_seed(3)
    assert got == torch.randperm(13)[:12].tolist()
    assert len(_stub(avt, 13).loader(4, drop_last=False)) == 4 and len(ld) == 3
    assert sum(_epoch(_stub(avt, 13).loader(4, shuffle=False, drop_last=False)), []) == list(range(13))


def test_loader_refuses_what_the_ranks_cannot_share(avt):
    with pytest.raises(ValueError, match="drop_last"):
        _stub(avt, 13, 0, 2).loader(2, drop_last=False, seed=7)
    with pytest.raises(ValueError, match="global batch"):
        _stub(avt, 13, 1, 2).loader(7, seed=7)  # 14 items per step, 13 in the dataset
    with pytest.raises(ValueError, match="global batch"):
        _stub(avt, 3).loader(4)
    with pytest.raises(ValueError, match="seed"):
        _stub(avt, 13, 0, 2).loader(2)  # no process group to agree on an order through
    with pytest.raises(ValueError, match="does not divide"):
        _stub(avt, 13, 0, 2).share(torch.arange(5))
    with pytest.raises(ValueError, match="does not divide"):
        _stub(avt, 13, 1, 4)._pack(torch.arange(6))
    assert _stub(avt, 13, 1, 2).share(torch.arange(6)).tolist() == [3, 4, 5]


def test_batcher_refuses_a_rank_outside_the_world(avt):
    from avtex.dataset import DeviceSegmentBatcher

    ds = SimpleNamespace(split="train")
    for rank, world in ((2, 2), (-1, 2), (0, 0)):
        with pytest.raises(ValueError, match="rank"):
            DeviceSegmentBatcher(ds, "cpu", rank=rank, world=world)


def test_train_batch_plan_is_declared_and_bound(avt):
    src = re.sub(r"/\*.*?\*/", "", open(avt._lib.HEADER_PATH).read(), flags=re.S)
    m = re.search(r"\bint\s+avt_train_batch_plan\s*\(([^)]*)\)", src)
    assert m is not None
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 11 == len(avt._lib.SIGNATURES["avt_train_batch_plan"])
    assert [p.split()[-1].lstrip("*") for p in params] == ["mt_state", "idx", "batch", "keep_lo", "keep_n", "n_len", "n_negs", "stride",
                                                           "tgt_out", "starts_out", "stream"]
    assert hasattr(avt.ops, "train_batch_plan") and "avt_negative_sample_mt19937" in avt._lib.SIGNATURES
    assert "dataset.py:128-139, 181-190" in open(avt._lib.HEADER_PATH).read().split("int avt_train_batch_plan")[0].rsplit("/*", 1)[1]


_OK = dict(batch=8, keep_lo=2, keep_n=2, n_len=99, n_negs=14, stride=6)
_REJECTED = [
    (dict(keep_lo=7, keep_n=2), "avt_train_batch_plan: items 7 .. 7 + 2 are not inside a batch of 8"),
    (dict(keep_lo=-1), "avt_train_batch_plan: items -1 .. -1 + 2 are not inside a batch of 8"),
    (dict(keep_n=-1), "avt_train_batch_plan: items 2 .. 2 + -1 are not inside a batch of 8"),
    (dict(stride=0), "avt_train_batch_plan: need stride >= 1 and (len + 1) * stride < 2^31 (len 99, stride 0)"),
    (dict(stride=1 << 25), "avt_train_batch_plan: need stride >= 1 and (len + 1) * stride < 2^31 (len 99, stride 33554432)"),
    (dict(n_negs=99), "avt_train_batch_plan: need batch >= 0, len >= 3, 1 <= n_negs <= len - 1 (cannot draw 99 of 98)"),
    (dict(n_len=12289, stride=1), "avt_train_batch_plan: more than 12287 candidate segments"),
]


# (with made-up addresses a check that went missing would be a real launch: never where a device is visible)
@pytest.mark.skipif(torch.cuda.is_available(), reason="made-up device addresses: only on a box without a GPU")
@pytest.mark.parametrize("bad,message", _REJECTED, ids=["-".join("%s=%s" % kv for kv in b.items()) for b, _ in _REJECTED])
def test_train_batch_plan_rejects_bad_arguments_before_any_launch(avt, bad, message):
    lib = avt._lib.lib()
    g = dict(_OK, **bad)
    AVT_ERR_ARG = -1  # include/avt.h
    args = [0x10000, 0x20000, g["batch"], g["keep_lo"], g["keep_n"], g["n_len"], g["n_negs"], g["stride"], 0x30000, 0x40000, 0]
    assert lib.avt_train_batch_plan(*args) == AVT_ERR_ARG
    assert lib.avt_last_error().decode() == message


@pytest.mark.skipif(torch.cuda.is_available(), reason="made-up device addresses: only on a box without a GPU")
def test_train_batch_plan_null_pointers_and_the_empty_batch(avt):
    lib = avt._lib.lib()
    tail = [_OK[k] for k in ("keep_lo", "keep_n", "n_len", "n_negs", "stride")]
    for hole in range(4):
        ptrs = [0x10000, 0x20000, 0x30000, 0x40000]
        ptrs[hole] = None
        assert lib.avt_train_batch_plan(ptrs[0], ptrs[1], 8, *tail, ptrs[2], ptrs[3], 0) == -1
        assert lib.avt_last_error().decode() == "avt_train_batch_plan: NULL pointer"
    assert lib.avt_train_batch_plan(0x10000, 0x20000, 0, 0, 0, 99, 14, 6, 0x30000, 0x40000, 0) == 0  # batch 0: no launch, OK


def test_main_builds_the_device_loader_on_every_rank(avt, monkeypatch, capsys):
    """main()'s loader branch for --train_input device at world 2 (no process group, no device: the batcher is a stub that records how
    it was built): no refusal, the per-rank batch of the DataLoader path, and rank 0's line."""
    import avtex.dataset
    from avtex import main as avt_main

    built = []

    class Batcher:
        def __init__(self, dataset, device, dtype=torch.float32, rank=0, world=1):
            self.ds, self.rank, self.world = dataset, rank, world
            built.append(self)

        def loader(self, batch_size, shuffle=True, drop_last=True, seed=None):
            self.asked = (batch_size, shuffle, drop_last, seed)
            return [None] * (len(self.ds) // (batch_size * self.world))

    monkeypatch.setattr(avtex.dataset, "DeviceSegmentBatcher", Batcher)
    args = avt_main.build_parser().parse_args(["--train_input", "device", "-bs", "4", "--train_graph", "1"])
    for rank in (0, 1):
        loader = avt_main.build_train_loader(args, _Items(13), torch.device("cpu"), rank, 2)
        assert len(loader) == 3
        assert (built[-1].rank, built[-1].world, built[-1].asked) == (rank, 2, (2, True, True, None))
        out = capsys.readouterr().out
        if rank == 0:
            assert "assembled on the device" in out and "world 2" in out and "per-rank batch 2" in out and "global batch 4" in out
            assert "3 steps per epoch" in out
        else:
            assert out == ""
    # one process: the whole batch, as before
    avt_main.build_train_loader(args, _Items(13), torch.device("cpu"), 0, 1)
    assert (built[-1].rank, built[-1].world, built[-1].asked[0]) == (0, 1, 4)
    # the host path is still the DataLoader
    host = avt_main.build_train_loader(avt_main.build_parser().parse_args(["-bs", "4", "-j", "0"]), _Items(13), torch.device("cpu"), 0, 1)
    assert isinstance(host, torch.utils.data.DataLoader) and host.batch_size == 4 and len(built) == 3
