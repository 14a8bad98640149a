"""Host side of train_ops.GradExchange (the gradient exchange of train()'s graphed step across ranks): the layout of the flat buffer, the
job table of csrc/grad_pack.hip as the library reads it, and the CLI's --dist_backend.  No device calls."""
import struct

import numpy as np


def _ceil4(n):
    return (n + 3) // 4 * 4


def test_exchange_layout_is_16_byte_aligned_and_disjoint(avt):
    from avtex import train_ops

    numels = [1, 3, 4, 5, 4096, 4097]
    offsets, total = train_ops.exchange_layout(numels)
    assert len(offsets) == len(numels) and all(o % 4 == 0 for o in offsets)
    spans = sorted((o, o + n) for o, n in zip(offsets, numels))
    assert spans[0][0] == 0 and all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= total
    assert total == sum(_ceil4(n) for n in numels) == 4 + 4 + 4 + 8 + 4096 + 4100
    assert train_ops.exchange_layout([]) == ([], 0)


def test_pack_grad_jobs_byte_layout(avt):
    from avtex import train_ops

    numels = [1, 4096, 4097, 3, 8193]
    recs = [(0x1000 * (k + 1) + 4, 0x100000 * (k + 1), n) for k, n in enumerate(numels)]
    raw, blk2job, blocks = train_ops.pack_grad_jobs(recs)
    assert struct.calcsize("<2Qq2i") == 32 and len(raw) == 32 * len(recs)
    assert avt._lib.lib().avt_pack_job_bytes() == 32  # (a host-only entry: no device needed)
    run = 0
    for k, (src, dst, n) in enumerate(recs):
        assert struct.unpack_from("<2Qq2i", raw, 32 * k) == (src, dst, n, run, 0)
        nb = -(-n // 4096)
        assert np.array_equal(blk2job[run : run + nb], np.full(nb, k, np.int32))
        run += nb
    assert blocks == run == 1 + 1 + 2 + 1 + 3 and blk2job.dtype == np.int32 and len(blk2job) == blocks
    raw0, blk0, blocks0 = train_ops.pack_grad_jobs([])
    assert raw0 == b"" and len(blk0) == 0 and blocks0 == 0


def test_parser_takes_a_dist_backend(avt):
    from avtex.main import build_parser

    p = build_parser()
    assert p.parse_args(["-vdata", "x"]).dist_backend is None
    assert p.parse_args(["-vdata", "x", "--dist_backend", "gloo"]).dist_backend == "gloo"
    assert p.parse_args(["-vdata", "x", "--dist_backend", "nccl"]).dist_backend == "nccl"


def test_launch_counter_exists(avt):
    from avtex import train_ops

    assert "grad_pack_multi" in train_ops.CALLS and "sgd_multi" in train_ops.CALLS
