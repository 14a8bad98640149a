"""train_ops.ArenaSGD without a GPU: what it refuses at construction, the --train_optimizer flag, the job table train_ops.pack_sgd_jobs
packs against the library's own sizeof(AvtSgdJob) and the header's fields, and the state_dict round trip with torch.optim.SGD.  No
device calls here (the kernel itself: tests/test_gpu_arena_sgd.py)."""
import ctypes
import re
import struct

import numpy as np
import pytest
import torch


def _host_arena_sgd(monkeypatch, train_ops, params, **kw):
    """An ArenaSGD over HOST parameters, for the parts of it that never touch the device (state, param_groups): the construction check
    that refuses host tensors is lifted for this one object."""
    monkeypatch.setattr(train_ops.ArenaSGD, "_check_param", staticmethod(lambda p: None))
    return train_ops.ArenaSGD(params, **kw)


def test_refusals_at_construction(avt):
    from avtex import train_ops

    AvtError = avt._lib.AvtError
    w = torch.nn.Parameter(torch.zeros(4, 6))
    with pytest.raises(AvtError, match="device"):
        train_ops.ArenaSGD([w], lr=0.1)  # a host parameter
    check = train_ops.ArenaSGD._check_param
    # the per-parameter checks, on host tensors of a subclass that CLAIMS to be on the device (dtype, layout and strides are real)
    for bad, what in ((torch.zeros(4, 6, dtype=torch.float16), "fp32"), (torch.zeros(4, 6, dtype=torch.float64), "fp32"),
                      (torch.zeros(4, 12)[:, ::2], "contiguous"), (torch.zeros(6, 4).t(), "contiguous")):
        class Claims(torch.Tensor):
            is_cuda = True

        with pytest.raises(AvtError, match=what):
            check(bad.as_subclass(Claims))
    with pytest.raises(AvtError):
        check(torch.zeros(4, 6).to_sparse())
    ok = torch.zeros(4, 6, 2, 3, 3).contiguous(memory_format=torch.channels_last_3d)

    class Claims(torch.Tensor):
        is_cuda = True

    check(ok.as_subclass(Claims))  # the training layout's convolution weights are dense: accepted
    check(torch.zeros(7).as_subclass(Claims))


def test_refuses_dampening_maximize_and_bad_nesterov(avt, monkeypatch):
    from avtex import train_ops

    AvtError = avt._lib.AvtError
    w = [torch.nn.Parameter(torch.zeros(5))]
    with pytest.raises(AvtError, match="dampening"):
        _host_arena_sgd(monkeypatch, train_ops, w, lr=0.1, momentum=0.9, dampening=0.1)
    with pytest.raises(AvtError, match="maximize"):
        _host_arena_sgd(monkeypatch, train_ops, w, lr=0.1, maximize=True)
    with pytest.raises(AvtError, match="Nesterov"):
        _host_arena_sgd(monkeypatch, train_ops, w, lr=0.1, momentum=0.0, nesterov=True)
    with pytest.raises(AvtError, match="dampening"):  # ... also when a group brings its own
        _host_arena_sgd(monkeypatch, train_ops, [{"params": w, "dampening": 0.5}], lr=0.1, momentum=0.9)


def test_train_optimizer_flag(avt):
    p = __import__("avtex.main", fromlist=["x"]).build_parser()
    base = ["-vdata", "v", "-ea", "slowfast"]
    assert p.parse_args(base).train_optimizer == "torch"
    assert p.parse_args(base + ["--train_optimizer", "hip"]).train_optimizer == "hip"
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--train_optimizer", "adam"])


def test_job_table_layout_matches_the_header_and_the_library(avt):
    """AvtSgdJob as the three parties see it: the header's fields mirrored in ctypes, the library's sizeof, train_ops.pack_sgd_jobs."""
    from avtex import train_ops

    class AvtSgdJob(ctypes.Structure):
        _fields_ = [("p", ctypes.c_void_p), ("g", ctypes.c_void_p), ("buf", ctypes.c_void_p), ("numel", ctypes.c_int64),
                    ("group", ctypes.c_int32), ("blk0", ctypes.c_int32)]

    src = open(avt._lib.HEADER_PATH).read()
    body = src[src.index("typedef struct AvtSgdJob {"):src.index("} AvtSgdJob;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b([a-z_0-9]+)\s*;", body) == [f[0] for f in AvtSgdJob._fields_]
    nbytes = avt._lib.lib().avt_sgd_job_bytes()
    assert ctypes.sizeof(AvtSgdJob) == nbytes == struct.calcsize("<3Qq2i") == 40 == avt.ops.sgd_job_bytes()

    recs = [(0x1000, 0x2000, 0x3000, 1, 0), (0x10000, 0x20000, 0, 4096, 1), (0x7f0000000010, 0x7f1000000004, 0x7f2000000008, 4097, 0),
            (0x40, 0x80, 0xc0, (1 << 33) + 5, 2)]
    raw, blk, blocks = train_ops.pack_sgd_jobs(recs)
    assert len(raw) == len(recs) * nbytes
    jobs = [AvtSgdJob.from_buffer_copy(raw, i * nbytes) for i in range(len(recs))]
    per = [1, 1, 2, (1 << 21) + 1]  # ceil(numel / 4096)
    assert blocks == sum(per) == len(blk) and blk.dtype == np.int32
    b0 = 0
    for n, (j, r, nb) in enumerate(zip(jobs, recs, per)):
        assert (j.p, j.g, j.buf or 0, j.numel, j.group, j.blk0) == r[:5] + (b0,)
        assert (blk[b0:b0 + nb] == n).all()  # block b of the launch is block b - blk0 of job blk2job[b]
        b0 += nb


def test_state_dict_round_trip_with_torch_sgd(avt, monkeypatch):
    from avtex import train_ops

    torch.manual_seed(0)
    shapes = [(3, 5), (7,), (2, 3, 1, 2, 2)]
    mk = lambda: [torch.nn.Parameter(torch.randn(s)) for s in shapes]  # noqa: E731
    kw = dict(lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True)

    # torch -> ArenaSGD: buffers of a stepped torch optimizer arrive as this optimizer's state
    pt = mk()
    ot = torch.optim.SGD(pt, **kw)
    for p in pt:
        p.grad = torch.randn_like(p)
    ot.step()
    pa = mk()
    oa = _host_arena_sgd(monkeypatch, train_ops, pa, lr=1.0, momentum=0.5)
    assert all(torch.equal(oa.state[p]["momentum_buffer"], torch.zeros_like(p)) for p in pa)  # zero-initialised, allocated once
    oa.load_state_dict(ot.state_dict())
    g = oa.param_groups[0]
    assert (g["lr"], g["momentum"], g["weight_decay"], g["nesterov"], g["dampening"]) == (0.05, 0.9, 1e-4, True, 0)
    for a, t in zip(pa, pt):
        assert torch.equal(oa.state[a]["momentum_buffer"], ot.state[t]["momentum_buffer"])

    # ArenaSGD -> torch: and back again, a scheduler's rate included
    sched = torch.optim.lr_scheduler.StepLR(oa, step_size=1, gamma=0.1)
    sched.step()
    assert abs(oa.param_groups[0]["lr"] - 0.005) < 1e-12
    sd = oa.state_dict()
    pt2 = mk()
    ot2 = torch.optim.SGD(pt2, lr=1.0)
    ot2.load_state_dict(sd)
    assert abs(ot2.param_groups[0]["lr"] - 0.005) < 1e-12 and ot2.param_groups[0]["momentum"] == 0.9
    for a, t in zip(pa, pt2):
        assert torch.equal(ot2.state[t]["momentum_buffer"], oa.state[a]["momentum_buffer"])
    for p in pt2:
        p.grad = torch.randn_like(p)
    ot2.step()  # torch's own step accepts the state
    sd2 = ot2.state_dict()
    assert sorted(sd2["state"]) == sorted(sd["state"]) == [0, 1, 2]
