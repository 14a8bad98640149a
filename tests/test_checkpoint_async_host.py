"""The host side of --ckpt_async / --ckpt_train_state, without a device: the flat layout of a snapshot (train_ops.state_layout), the
job-table packer against the header's struct, checkpoint.AsyncCheckpointWriter on CPU tensors that are views into one large buffer — its
files against main.save_checkpoint's, the size of every loaded storage, _best only when is_best, a failing write surfacing at close(),
no partial file for a concurrent reader — and the two flags' parser defaults."""
import ctypes
import os
import threading
from collections import OrderedDict

import numpy as np
import pytest
import torch

SIZES = [0, 1, 15, 16, 17, 16383, 16384, 16385]


def test_state_layout_slots_are_aligned_and_disjoint(avt):
    from avtex import train_ops

    offsets, total = train_ops.state_layout(SIZES)
    assert len(offsets) == len(SIZES) and total % 16 == 0
    end = 0
    for o, n in zip(offsets, SIZES):
        assert o % 16 == 0 and o >= end  # 16-byte aligned, not inside the tensor before it
        end = o + n
    assert end <= total == sum((n + 15) // 16 * 16 for n in SIZES)
    assert offsets[0] == offsets[1] == 0  # a zero-size tensor takes no room
    assert train_ops.state_layout([]) == ([], 0) and train_ops.state_layout([0, 0]) == ([0, 0], 0)
    assert train_ops.state_layout([403 * 2 ** 20 + 1, 4]) == ([0, 403 * 2 ** 20 + 16], 403 * 2 ** 20 + 32)  # 64-bit sizes


def test_job_table_packer_writes_the_headers_struct(avt):
    from avtex import train_ops

    class AvtStateJob(ctypes.Structure):  # include/avt.h
        _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("nbytes", ctypes.c_int64), ("blk0", ctypes.c_int32),
                    ("pad", ctypes.c_int32)]

    recs = [(0x7f0000001000, 0x7f1000000000, 1), (0x7f0000002004, 0x7f1000000010, 16384), (0x7f0000003001, 0x7f1000004010, 16385),
            (0x7f0000100000, 0x7f1000008030, 403 * 2 ** 20)]
    raw, blk2job, blocks = train_ops.pack_state_jobs(recs)
    want, blk0, owners = b"", 0, []
    for n, (s, d, nbytes) in enumerate(recs):
        want += bytes(AvtStateJob(s, d, nbytes, blk0, 0))
        nb = -(-nbytes // 16384)
        owners += [n] * nb
        blk0 += nb
    assert raw == want and len(raw) == 32 * len(recs)
    assert blocks == blk0 == 1 + 1 + 2 + 403 * 64 and blk2job.dtype == np.int32 and blk2job.tolist() == owners
    raw0, blk0_, blocks0 = train_ops.pack_state_jobs([])
    assert raw0 == b"" and blocks0 == 0 and blk0_.shape == (0,)


def _views():
    """A state_dict whose tensors are views into ONE buffer, as a snapshot's are: fp32 of several shapes, a channels-last 5-D weight,
    an int64 scalar; with the _metadata a module's state_dict carries."""
    big = torch.arange(4096, dtype=torch.float32) * 0.5 - 7
    ints = big[2048:2050].view(torch.int64)
    ints.fill_(12345)
    cl = torch.as_strided(big, (4, 3, 2, 2, 2), (24, 1, 12, 6, 3), 1024)  # channels_last_3d strides of [4, 3, 2, 2, 2]
    assert cl.is_contiguous(memory_format=torch.channels_last_3d)
    sd = OrderedDict([("enc.weight", cl), ("enc.bias", big[16:20]), ("bn.running_mean", big[32:39]),
                      ("bn.num_batches_tracked", ints[0]), ("fc.weight", big[64:64 + 35].view(5, 7))])
    sd._metadata = OrderedDict([("", {"version": 1}), ("bn", {"version": 2})])
    return big, sd


def _make_state(sd, epoch, best):
    def make(tensors):
        out = type(sd)((k, tensors[k]) for k in sd)
        out._metadata = sd._metadata
        return {"epoch": epoch, "arch": "resnet10", "state_dict": out, "best_loss": best}
    return make


def _same_checkpoint(a, b):
    assert list(a) == list(b) == ["epoch", "arch", "state_dict", "best_loss"]
    assert (a["epoch"], a["arch"], a["best_loss"]) == (b["epoch"], b["arch"], b["best_loss"])
    sa, sb = a["state_dict"], b["state_dict"]
    assert type(sa) is type(sb) and list(sa) == list(sb) and sa._metadata == sb._metadata
    for k in sa:
        assert sa[k].dtype == sb[k].dtype and sa[k].shape == sb[k].shape and sa[k].stride() == sb[k].stride(), k
        assert torch.equal(sa[k], sb[k]), k


def test_writer_files_equal_the_synchronous_ones_and_own_their_storage(avt, tmp_path):
    from avtex.checkpoint import AsyncCheckpointWriter
    from avtex.main import save_checkpoint

    big, sd = _views()
    (tmp_path / "sync").mkdir()
    (tmp_path / "async").mkdir()
    # the synchronous path, on tensors that own their storage as a module's do
    own = type(sd)((k, v.clone()) for k, v in sd.items())
    own._metadata = sd._metadata
    save_checkpoint({"epoch": 3, "arch": "resnet10", "state_dict": own, "best_loss": 0.25}, True, str(tmp_path / "sync" / "run"))
    w = AsyncCheckpointWriter()
    w.submit(dict(sd), _make_state(sd, 3, 0.25), True, str(tmp_path / "async" / "run"))
    w.close()
    assert w.pending() == 0
    assert sorted(os.listdir(tmp_path / "async")) == sorted(os.listdir(tmp_path / "sync")) == ["run_best.pth.tar", "run_latest.pth.tar"]
    for name in ("run_latest.pth.tar", "run_best.pth.tar"):
        a = torch.load(tmp_path / "async" / name, map_location="cpu", weights_only=False)
        b = torch.load(tmp_path / "sync" / name, map_location="cpu", weights_only=False)
        _same_checkpoint(a, b)
        for k, v in a["state_dict"].items():  # a view saved as it is would bring the whole 16 KiB buffer along
            assert v.untyped_storage().nbytes() == v.numel() * v.element_size(), k
    assert os.path.getsize(tmp_path / "async" / "run_latest.pth.tar") < big.numel() * 4


def test_best_is_written_only_when_is_best_and_a_handle_is_released(avt, tmp_path):
    from avtex.checkpoint import AsyncCheckpointWriter

    _, sd = _views()

    class Handle:
        def __init__(self):
            self.waited, self.released = 0, 0

        def wait(self):
            self.waited += 1
            return dict(sd)

        def release(self):
            self.released += 1

    h = Handle()
    w = AsyncCheckpointWriter()
    w.submit(h, _make_state(sd, 1, 0.5), False, str(tmp_path / "run"))
    w.close()
    w.close()  # (twice is fine)
    assert (h.waited, h.released) == (1, 1)
    assert os.listdir(tmp_path) == ["run_latest.pth.tar"]
    with pytest.raises(RuntimeError, match="after close"):
        w.submit(h, _make_state(sd, 1, 0.5), False, str(tmp_path / "run"))


def test_a_failing_write_surfaces_at_close_and_at_the_next_submit(avt, tmp_path):
    from avtex.checkpoint import AsyncCheckpointWriter

    _, sd = _views()
    w = AsyncCheckpointWriter()
    w.submit(dict(sd), _make_state(sd, 1, 0.5), True, str(tmp_path / "no_such_folder" / "run"))
    with pytest.raises(Exception) as e:
        w.close()
    assert "no_such_folder" in str(e.value)
    assert not any(f.endswith(".pth.tar") or ".tmp." in f for f in os.listdir(tmp_path))

    def boom(_tensors):
        raise ValueError("make_state failed")

    w = AsyncCheckpointWriter()
    w.submit(dict(sd), boom, False, str(tmp_path / "run"))
    w.drain()  # (the thread has met the failure)
    with pytest.raises(ValueError, match="make_state failed"):
        w.submit(dict(sd), _make_state(sd, 2, 0.5), False, str(tmp_path / "run"))
    w.close()


def test_a_concurrent_reader_never_sees_a_partial_file(avt, tmp_path):
    from avtex.checkpoint import AsyncCheckpointWriter

    _, sd = _views()
    path = str(tmp_path / "run")
    w = AsyncCheckpointWriter()
    w.submit(dict(sd), _make_state(sd, 0, 1.0), False, path)
    w.drain()  # the first file exists: from here on the reader must always be able to load one
    seen, errors, stop = [], [], threading.Event()

    def reader():
        while not stop.is_set():
            try:
                ck = torch.load(path + "_latest.pth.tar", map_location="cpu", weights_only=False)
                assert list(ck["state_dict"]) == list(sd) and all(torch.equal(ck["state_dict"][k], sd[k]) for k in sd)
                seen.append(ck["epoch"])
            except Exception as e:  # noqa: BLE001
                errors.append(e)
                return

    t = threading.Thread(target=reader)
    t.start()
    for epoch in range(1, 6):
        w.submit(dict(sd), _make_state(sd, epoch, 1.0 / epoch), epoch % 2 == 1, path)
    w.close()
    stop.set()
    t.join()
    assert not errors, errors[:1]
    assert seen == sorted(seen) and set(seen) <= set(range(6))
    assert torch.load(path + "_latest.pth.tar", weights_only=False)["epoch"] == 5
    assert torch.load(path + "_best.pth.tar", weights_only=False)["epoch"] == 5
    assert sorted(os.listdir(tmp_path)) == ["run_best.pth.tar", "run_latest.pth.tar"]  # no temporary file is left


def test_the_two_flags_default_off(avt):
    from avtex.main import build_parser

    p = build_parser()
    d = p.parse_args([])
    assert d.ckpt_async is False and d.ckpt_train_state is False
    on = p.parse_args(["--ckpt_async", "--ckpt_train_state"])
    assert on.ckpt_async is True and on.ckpt_train_state is True


def test_device_loader_state_round_trips_on_the_host(avt):
    """The loader's state_dict / load_state_dict without a device: seed, epoch, the 625 words and the cached gaussian."""
    from avtex.dataset import DeviceSegmentBatcher, _DeviceLoader

    bat = DeviceSegmentBatcher.__new__(DeviceSegmentBatcher)
    bat.dev, bat.world, bat.state, bat._gauss = torch.device("cpu"), 1, torch.arange(625, dtype=torch.int32), (1, 0.75)
    bat.ds = list(range(12))
    ld = _DeviceLoader(bat, 4, True, True, seed=9)
    ld.set_epoch(3)
    sd = ld.state_dict()
    assert sd["seed"] == 9 and sd["epoch"] == 3 and sd["batcher"]["gauss"] == (1, 0.75)
    assert sd["batcher"]["state"].dtype == torch.int32 and sd["batcher"]["state"].tolist() == list(range(625))
    other = DeviceSegmentBatcher.__new__(DeviceSegmentBatcher)
    other.dev, other.world, other.state, other._gauss, other.ds = torch.device("cpu"), 1, None, (0, 0.0), bat.ds
    ld2 = _DeviceLoader(other, 4, True, True)
    assert ld2.state_dict()["batcher"]["state"] is None
    ld2.load_state_dict(sd)
    assert (ld2.seed, ld2.epoch, other._gauss) == (9, 3, (1, 0.75)) and torch.equal(other.state, bat.state)
    assert torch.equal(ld2.order(), ld.order())
    with pytest.raises(ValueError, match="625"):
        other.load_state_dict({"state": torch.zeros(624, dtype=torch.int32), "gauss": (0, 0.0)})
