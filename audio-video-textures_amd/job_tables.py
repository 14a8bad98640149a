"""Device job tables.  A training step has launches that each cover many tensors (ops.sgd_multi, ops.grad_pack_multi,
ops.weight_planes_multi, ops.state_copy_multi): the kernel reads a device table of jobs and a block -> job map, both built on the host.
One packer (_pack_jobs) and one owner (_JobTable) serve them, so the rules of a table's lifetime under stream capture are written once.
A leaf module: train_ops (ArenaSGD, GradExchange, StateSnapshot) and weight_planes (the refresh of the plane cache) import it, and with
it the launch counters both of them bump."""
import struct
from collections import namedtuple

import numpy as np
import torch

from . import _lib, ops

# per-process launch counters of the hand-written training kernels (tests assert that the default path really runs them; read as
# train_ops.CALLS)
CALLS = {"conv_fwd_x3": 0, "dgrad_x3": 0, "dgrad_strided_x3": 0, "wgrad_x3": 0, "wgrad_stem_x3": 0, "bn_fwd": 0, "bn_bwd": 0,
         "miopen_dgrad": 0, "miopen_wgrad": 0, "stem_fwd_patch": 0, "wgrad_stem_patch": 0, "maxpool_hip": 0, "pw_f32": 0,
         "bn_fwd_pre": 0, "bn_bwd_pre": 0, "dgrad_bwdstats": 0, "planes_multi": 0, "maxpool3d_hip": 0, "sgd_multi": 0, "grad_pack_multi": 0,
         "wgrad_det": 0,  # (wgrad_det: launches of the deterministic weight-gradient entries, counted next to the rows above)
         "state_copy_multi": 0,
         "rank_sum": 0}  # (rank_sum: launches of the ordered exchange's sum over the ranks, GradExchange.exchange)

_SGD_CHUNK = 4096  # elements per block (csrc/sgd.hip and csrc/grad_pack.hip kChunk)
_SGD_JOB, _PACK_JOB, _PLANE_JOB = "<3Qq2i", "<2Qq2i", "<5Q12i32i"  # AvtSgdJob, AvtPackJob, AvtPlaneJob (include/avt.h)


def _chunks(numel):
    return (int(numel) + _SGD_CHUNK - 1) // _SGD_CHUNK


def _pack_jobs(recs, blocks_of, row):
    """blocks_of(rec) -> blocks of the job, row(rec, blk0) -> the job's struct as bytes -> (job table as bytes, blk2job int32 array,
    blocks): job n owns blocks_of(rec) consecutive blocks from its blk0."""
    raw, blk, b0 = [], [], 0
    for n, rec in enumerate(recs):
        nb = blocks_of(rec)
        raw.append(row(rec, b0))
        blk.append(np.full(nb, n, dtype=np.int32))
        b0 += nb
    return b"".join(raw), (np.concatenate(blk) if blk else np.zeros(0, np.int32)), b0


_Table = namedtuple("_Table", "key jobs blk2job blocks captured keep")  # jobs, blk2job: views of ONE uploaded device buffer


class _JobTable:
    """The device job table of one multi-tensor launch and what keeps it valid:

    * `table`: the table of the last launch.  get() reuses it while the key (the tuple of addresses) is unchanged — the same tensors
      at the same addresses every step: built once — and it was not built under capture: such a table is filled by its own graph's
      replays only, so no later launch uses it.
    * `kept`: every table a stream capture launched with.  A HIP graph holds its address: it outlives every later rebuild.
    * the spare pinned buffer: a table built under capture is uploaded by a copy that is a node of the graph and re-reads its pinned
      source on every replay.  No pinned allocation inside a capture, so reserve() sets the buffer aside before one.

    capture_builds: what a capture does with a key it does not know.  True (the optimizer and the gradient pack: a captured step's
    gradients live in the graph's own pool, their addresses are not known before the capture): build, staged in the spare buffer.
    False (the weight planes: the weights do not move, the warm-up has built the table): get() -> None and the caller does without
    the launch."""

    def __init__(self, who, fmt, sizeof, remedy=None, capture_builds=True):
        # who, remedy: the caller and the calls that reserve for it, for the refusal's text; sizeof(): the library's view of fmt
        self.who, self.fmt, self.sizeof, self.remedy, self.capture_builds = who, fmt, sizeof, remedy, capture_builds
        self.table, self.kept, self._spare, self._alive = None, [], None, []

    def reserve(self, blocks):
        """Outside a capture: a pinned buffer for the largest table the next get() under capture may stage in it.  blocks: the blocks
        of each of its jobs, as the caller's packer counts them (an iterable, read only when no buffer is held)."""
        if self._spare is None:
            blocks = list(blocks)
            nbytes = struct.calcsize(self.fmt) * len(blocks) + 4 * sum(blocks)
            self._spare = torch.empty(max(nbytes, 8), dtype=torch.uint8, pin_memory=True)

    def unreserve(self):
        self._spare = None

    def keep_alive(self, obj):
        """Something else a captured launch read, kept for as long as the tables (not in `kept`: that lists tables only)."""
        self._alive.append(obj)

    def forget(self):
        """The next get() builds anew.  What captures launched with stays."""
        self.table = None

    def get(self, key, device, pack):
        """-> the table for `key` on the current stream, uploaded (one copy) when it had to be built: pack() -> (job table as bytes,
        blk2job, blocks), called for a new table only (the caller's checks of the tensors behind the key belong in it)."""
        capturing = torch.cuda.is_current_stream_capturing()
        tab = self.table
        if tab is None or tab.key != key or tab.captured:
            if capturing and not self.capture_builds:
                return None
            raw, blk, blocks = pack()
            assert len(raw) == len(key) * self.sizeof() == len(key) * struct.calcsize(self.fmt), "%s: job struct layout" % self.who
            data = torch.from_numpy(np.frombuffer(raw + blk.tobytes(), dtype=np.uint8).copy())  # jobs and blk2job: one buffer, one copy
            dev = torch.empty(data.numel(), dtype=torch.uint8, device=device)
            if capturing:
                host, self._spare = self._spare, None  # (this table keeps it from now on: its graph re-reads it on every replay)
                if host is None or host.numel() < data.numel():
                    raise _lib.AvtError("%s under stream capture: no staging buffer is left (two captures in a row: call %s outside a "
                                        "capture between them)" % (self.who, self.remedy))
                host[:data.numel()].copy_(data)
                ops.sgd_upload(dev, host, data.numel())
            else:
                host = data.pin_memory()  # (a new pinned tensor per table: an earlier copy may be in flight)
                dev.copy_(host, non_blocking=True)
            # (keep: not the tensors behind the addresses — held, gradients would never return to the allocator and move every step)
            tab = self.table = _Table(key, dev[:len(raw)], dev[len(raw):].view(torch.int32), blocks, capturing, (host, dev))
        if capturing and not any(t is tab for t in self.kept):
            self.kept.append(tab)
        return tab
