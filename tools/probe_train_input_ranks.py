"""Where the batches of config 5's per-rank step come from, measured: the one-item step (1 query + 15 target clips, SlowFast at 224^2) of
--train_graph 1 in the ranks form (train_ops.prepare_ranks under a ONE-rank process group, AVT_FORCE_PG=1) on one GPU, fed by

  host -j N  the torch DataLoader over AudioVideoSegments with N workers (16 x (process_cv2_inputs + two F.interpolate) per item on the
             CPU, about 385 MB of fp32 clips uploaded per step) — what every rank ran under torch.distributed.run before the device path
             knew ranks
  device     dataset.DeviceSegmentBatcher(rank, world).loader(1): one plan launch and the gather kernels, no host copy

(a) A round is one call of avtex.train() over the first `--steps` batches of an epoch of each variant, between two device
synchronisations; the variants are interleaved.  Printed per variant: the wall time per step over the round (the workers' start and the
first fetch included, as in every epoch), the median of train()'s per-step Time without the first step, train()'s Data meter, and the time
spent inside the loader's own next().  Also the cost of one host item on one thread, the CPU model and the CPUs the process may use.
One rank on one GPU: what 8 ranks sharing a node's CPUs do to the host path is not measured, only what one rank gets from N workers.

(b) avt_train_batch_plan at B = 8, keep_n = 1 (one rank of eight) and keep_n = 8 against avt_negative_sample_mt19937 over the same 8 items
from the same state: device time per launch by events, median over `--launches`, interleaved.

    AVT_FORCE_PG=1 python tools/probe_train_input_ranks.py [--rounds 5] [--steps 32] [--workers 4,15] [--out profiles/r17/probe.log]
"""
import argparse
import contextlib
import io
import os
import re
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

_METERS = re.compile(r"Time ([\d.]+) \(([\d.]+)\)\s+Data ([\d.]+) \(([\d.]+)\)")


class _First:
    """The first `steps` batches of a loader's epoch, with the time spent waiting in the loader's next()."""

    def __init__(self, loader, steps):
        self.loader, self.steps, self.waited = loader, steps, []

    def __len__(self):
        return self.steps

    def __iter__(self):
        it = iter(self.loader)
        self.waited = []
        for _ in range(self.steps):
            t0 = time.perf_counter()
            batch = next(it)
            self.waited.append(time.perf_counter() - t0)
            yield batch
        del it  # (DataLoader workers stop here, not at the next epoch's start)


def _cpu_model():
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--workers", default="4,15", help="DataLoader worker counts of the host variants")
    ap.add_argument("--launches", type=int, default=30, help="timed launches per kernel in (b)")
    ap.add_argument("--out", default=None, help="also write the log to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_train_input_ranks: needs the MI355X (no timing without a device)")
    if os.environ.get("AVT_FORCE_PG") != "1":
        raise SystemExit("probe_train_input_ranks: set AVT_FORCE_PG=1 (the one-rank process group the ranks form runs under)")
    import avtex
    from avtex import dist as adist, ops, synth, train_ops
    from avtex.dataset import DeviceSegmentBatcher
    from avtex.slowfast import SlowFast

    rank, world, local = adist.init_from_env()
    assert world == 1 and torch.distributed.is_initialized()
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    cpus = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else os.cpu_count()
    say("device: %s; process group: %s, world %d; CPU: %s, %d CPUs usable by this process (%d in the machine), torch threads %d" %
        (avtex.ops.device_check(), torch.distributed.get_backend(), world, _cpu_model(), cpus, os.cpu_count(), torch.get_num_threads()))
    dargs = SimpleNamespace(vdata="/tmp", adata=None, n_negs=14, img_size=224, enc_arch="slowfast", window=0, stride=0)
    quiet = io.StringIO()
    with contextlib.redirect_stdout(quiet):
        ds = avtex.AudioVideoSegments(dargs, "synthetic", split="train", video=(synth.structured_video(123, 600, 256, 256), 30.0))
    assert a.steps <= len(ds), "the synthetic video has %d items" % len(ds)
    say("dataset: 600 frames 256^2 at 30 fps, window %d, stride %d, %d items; one item = 16 clips, %.0f MB of fp32 at 224^2" %
        (ds.window, ds.stride, len(ds), 16 * 3 * 40 * 224 * 224 * 4 / 1e6))
    np.random.seed(1)
    torch.manual_seed(3)
    t0 = time.perf_counter()
    for i in (5, 40, 80):
        ds[i]
    item_s = (time.perf_counter() - t0) / 3
    say("one host item (AudioVideoSegments.__getitem__, this process, %d torch threads): %.0f ms" % (torch.get_num_threads(), item_s * 1e3))
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # (what a DataLoader worker runs with)
    t0 = time.perf_counter()
    for i in (6, 41):
        ds[i]
    say("one host item on one thread, as in a DataLoader worker: %.0f ms" % ((time.perf_counter() - t0) / 2 * 1e3))
    torch.set_num_threads(threads)

    # ---- (a) -----------------------------------------------------------------------------------------------------------------------
    train_ops.set_conv_mode("x3")
    torch.manual_seed(0)
    model = avtex.ContrastivePredictionTemporal(SlowFast(), SlowFast(), None, 1, 128, temp=0.1, window=ds.window, stride=ds.stride,
                                                enc_arch="slowfast", img_size=224).to(dev)
    model = train_ops.training_layout(model)
    with contextlib.redirect_stdout(quiet):
        model = train_ops.prepare_ranks(model)
    opt = train_ops.ArenaSGD(model.parameters(), lr=1e-4, momentum=0.9, weight_decay=1e-4)
    targs = SimpleNamespace(print_freq=1, log_freq=10 ** 9, bn_replicas=1, train_graph=1)
    variants = {}
    for w in [int(v) for v in a.workers.split(",") if v]:
        variants["host -j %d" % w] = _First(torch.utils.data.DataLoader(ds, batch_size=1, shuffle=True, num_workers=w, drop_last=True), a.steps)
    variants["device"] = _First(DeviceSegmentBatcher(ds, dev, rank=0, world=1).loader(1, shuffle=True, drop_last=True), a.steps)

    def epoch(first):
        out = io.StringIO()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(out):
            loss = avtex.train(first, model, opt, targs, 0)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) * 1e3 / first.steps
        meters = [[float(v) for v in m.groups()] for m in _METERS.finditer(out.getvalue())]
        assert len(meters) == first.steps, out.getvalue()[-500:]
        return {"wall": wall, "step": statistics.median(m[0] for m in meters[1:]) * 1e3, "data": meters[-1][3] * 1e3,
                "data_rest": statistics.mean(m[2] for m in meters[1:]) * 1e3, "next": statistics.mean(first.waited[1:]) * 1e3,
                "first": first.waited[0] * 1e3, "loss": loss}

    r = epoch(variants["device"])  # warm-up steps, the capture (every variant delivers the same shapes: one graph)
    say("first call (warm-up, capture; device loader): %.1f ms/step, loss %.4f" % (r["wall"], r["loss"]))
    res = {n: [] for n in variants}
    for rnd in range(a.rounds):
        for n, first in variants.items():  # interleaved: a drift of the box lands on all variants alike
            res[n].append(epoch(first))
        say("round %2d: %s" % (rnd, "   ".join("%s %.1f ms/step (Data %.1f)" % (n, res[n][-1]["wall"], res[n][-1]["data"]) for n in variants)))
    say("per variant, medians over %d rounds of %d steps (ms): wall per step over the round | train()'s Time per step, median without the "
        "first step | train()'s Data meter, average over the round | the same without the first step | inside the loader's next(), mean "
        "without the first step | the first next()" % (a.rounds, a.steps))
    for n in variants:
        med = {k: statistics.median(x[k] for x in res[n]) for k in ("wall", "step", "data", "data_rest", "next", "first")}
        walls = [x["wall"] for x in res[n]]
        say("%-10s wall %7.1f (min %.1f, max %.1f) | step %7.1f | Data %7.1f | Data after the first %7.1f | next() %7.2f | first next() %7.1f" %
            (n, med["wall"], min(walls), max(walls), med["step"], med["data"], med["data_rest"], med["next"], med["first"]))
    dev_wall = statistics.median(x["wall"] for x in res["device"])
    for n in variants:
        if n != "device":
            say("%s / device: %.2f x the wall time per step" % (n, statistics.median(x["wall"] for x in res[n]) / dev_wall))

    # ---- (b) -----------------------------------------------------------------------------------------------------------------------
    n_len, n_negs, stride = len(ds), ds.n_negs, ds.stride
    ids = torch.tensor([0, n_len - 1, 1, n_len - 2, n_len // 2, 17, n_len - 5, 4], dtype=torch.int64, device=dev)
    np.random.seed(7)
    st = np.random.get_state()
    start = torch.from_numpy(np.concatenate([np.asarray(st[1], np.uint32), np.array([st[2]], np.uint32)]).view(np.int32).copy()).to(dev)
    state = start.clone()
    kernels = {
        "avt_negative_sample_mt19937, 8 items": lambda: ops.negative_sample(state, ids, n_len, n_negs),
        "avt_train_batch_plan, B 8, keep_n 1 (item 3)": lambda: ops.train_batch_plan(state, ids, 3, 1, n_len, n_negs, stride),
        "avt_train_batch_plan, B 8, keep_n 8": lambda: ops.train_batch_plan(state, ids, 0, 8, n_len, n_negs, stride),
    }
    times = {n: [] for n in kernels}
    ends = {}
    for i in range(3 + a.launches):
        for n, fn in kernels.items():  # interleaved; every launch starts from the same state (the copy is outside the events)
            state.copy_(start)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= 3:
                times[n].append(e0.elapsed_time(e1) * 1e3)
            ends[n] = state.clone()
    names = list(kernels)
    assert all(torch.equal(ends[n], ends[names[0]]) for n in names), "the three launches must leave one state"
    say("sampling kernels, n_len %d (600 frames at 30 fps), n_negs %d, device time per launch by events, %d launches each (us):" %
        (n_len, n_negs, a.launches))
    for n in names:
        say("  %-46s median %7.1f (min %.1f, max %.1f)" % (n, statistics.median(times[n]), min(times[n]), max(times[n])))
    old, new = statistics.median(times[names[0]]), statistics.median(times[names[1]])
    say("  plan (keep_n 1) / negative_sample: %.3f (expected: no more than 1.10)" % (new / old))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
