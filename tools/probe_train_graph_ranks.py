"""Time the one-item training step of config 5's per-rank shape (1 query + 15 target clips, SlowFast at 224^2) through avtex.train's own
machinery, in four forms interleaved in ONE process under a ONE-rank RCCL group (AVT_FORCE_PG=1) on one GPU:

  ranks   --train_graph 1 across ranks: forward, loss, backward and the gradient pack replayed as a HIP graph; one (self) all-reduce of the
          flat buffer and one eager ArenaSGD launch after every replay (train_ops.GradExchange, train_ops.prepare_ranks)
  world1  the one-process form: --train_graph 1 --train_optimizer hip, the optimizer inside the graph
  ddp     the eager step under DistributedDataParallel (main.wrap_ddp) with ArenaSGD
  ordered the ranks form with the ORDERED exchange (train_ops.GradExchange(ordered=True): a (self) all-gather into `parts` and one launch
          of csrc/rank_sum.hip in place of the all-reduce); the weight gradients stay on the default (atomic) path, as in `ranks`, so
          that the difference to `ranks` is the exchange alone.  At one rank it shows the added launch and copy, not the gather

A round is one call of train() over `--steps` prepared one-item batches (device tensors from dataset.DeviceSegmentBatcher, so that no host
preprocessing is timed), between two device synchronisations: wall time per step, train()'s loss.item() per step included in all four.
The first call of each form (warm-up, capture) is not counted.  Prints every round, medians and spreads.  What it cannot measure on one
GPU: any all-reduce between devices (RCCL with world > 1) and the scaling over 8 GPUs.

    AVT_FORCE_PG=1 python tools/probe_train_graph_ranks.py [--rounds 7] [--steps 12] [--out profiles/r15/train_graph_ranks_probe.log]
"""
import argparse
import contextlib
import io
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--forms", default="ranks,world1,ddp,ordered")
    ap.add_argument("--out", default=None, help="also write the log to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_train_graph_ranks: needs the MI355X (no timing without a device)")
    if os.environ.get("AVT_FORCE_PG") != "1":
        raise SystemExit("probe_train_graph_ranks: set AVT_FORCE_PG=1 (the one-rank RCCL group the ranks form and DDP run under)")
    import avtex
    from avtex import dist as adist, synth, train_ops
    from avtex.dataset import DeviceSegmentBatcher
    from avtex.main import wrap_ddp
    from avtex.slowfast import SlowFast

    rank, world, local = adist.init_from_env()
    assert world == 1 and torch.distributed.is_initialized()
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s; process group: %s, world %d" % (avtex.ops.device_check(), torch.distributed.get_backend(), world))
    dargs = SimpleNamespace(vdata="/tmp", adata=None, n_negs=14, img_size=224, enc_arch="slowfast", window=0, stride=0)
    quiet = io.StringIO()
    with contextlib.redirect_stdout(quiet):
        ds = avtex.AudioVideoSegments(dargs, "synthetic", split="train", video=(synth.structured_video(123, 600, 256, 256), 30.0))
    np.random.seed(1)
    torch.manual_seed(3)
    batches = []
    for b in DeviceSegmentBatcher(ds, dev).loader(1, shuffle=True, drop_last=True):
        batches.append(b)
        if len(batches) == a.steps:
            break
    assert len(batches) == a.steps, "the synthetic video has fewer than %d items" % a.steps
    train_ops.set_conv_mode("x3")

    def form(name):
        torch.manual_seed(0)
        model = avtex.ContrastivePredictionTemporal(SlowFast(), SlowFast(), None, 1, 128, temp=0.1, window=ds.window, stride=ds.stride,
                                                    enc_arch="slowfast", img_size=224).to(dev)
        model = train_ops.training_layout(model)
        args = SimpleNamespace(print_freq=10 ** 9, log_freq=10 ** 9, bn_replicas=1, train_graph=0 if name == "ddp" else 1,
                               exchange_ordered=name == "ordered")
        with contextlib.redirect_stdout(quiet):
            if name in ("ranks", "ordered"):
                model = train_ops.prepare_ranks(model)
            elif name == "ddp":
                model = wrap_ddp(model, dev, local)
        opt = train_ops.ArenaSGD(model.parameters(), lr=1e-4, momentum=0.9, weight_decay=1e-4)
        return model, opt, args

    def epoch(f):
        model, opt, args = f
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(quiet):
            loss = avtex.train(batches, model, opt, args, 0)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / len(batches), loss

    def apart(when):
        """Every form takes the same steps on the same batches from the same seed: how far apart the parameters are, pair by pair (the
        world1 / ddp pair is the yardstick: two forms that existed before; fp32 atomic sums are not ordered, and training amplifies)."""
        for i, m in enumerate(names):
            for n in names[i + 1:]:
                pm, pn = [p.detach().double() for p in forms[m][0].parameters()], [p.detach().double() for p in forms[n][0].parameters()]
                num = sum(float((x - y).square().sum()) for x, y in zip(pm, pn)) ** 0.5
                den = sum(float(x.square().sum()) for x in pm) ** 0.5
                worst = max(float((x - y).abs().max()) / max(float(x.abs().max()), 1e-30) for x, y in zip(pm, pn))
                say("parameters %s, %s vs %s: |a - b| / |a| over all tensors %.3e; worst tensor, max|a - b| / max|a| %.3e" %
                    (when, m, n, num / den, worst))

    names = [n for n in a.forms.split(",") if n]
    forms = {}
    for n in names:
        forms[n] = form(n)
        before = dict(train_ops.CALLS)
        ms, loss = epoch(forms[n])  # warm-up steps, the capture
        say("%-7s first call %.1f ms/step (warm-up, capture), loss %.4f; host launches: sgd_multi %d, grad_pack_multi %d, rank_sum %d" %
            (n, ms, loss, train_ops.CALLS["sgd_multi"] - before["sgd_multi"], train_ops.CALLS["grad_pack_multi"] - before["grad_pack_multi"],
             train_ops.CALLS["rank_sum"] - before["rank_sum"]))
    apart("after the first %d steps" % len(batches))
    numel = sum(p.numel() for p in forms[names[0]][0].parameters() if p.requires_grad)
    say("%d trainable elements (%.1f MB); %d one-item batches per round" % (numel, numel * 4 / 1e6, len(batches)))
    times = {n: [] for n in names}
    for r in range(a.rounds):
        for n in names:  # interleaved: a drift of the box lands on all forms alike
            times[n].append(epoch(forms[n])[0])
        say("round %2d: %s" % (r, "   ".join("%s %.2f ms/step" % (n, times[n][-1]) for n in names)))
    for n in names:
        m = statistics.median(times[n])
        say("%-7s median %.2f ms/step (min %.2f, max %.2f, spread %.1f %%): %.1f clips/s per rank" %
            (n, m, min(times[n]), max(times[n]), 100 * (max(times[n]) - min(times[n])) / m, 16e3 / m))
    apart("after %d steps" % ((a.rounds + 1) * len(batches)))
    if "ranks" in times and "world1" in times:
        say("ranks - world1: %+.2f ms/step (one pack launch, one self all-reduce, one eager optimizer launch)" %
            (statistics.median(times["ranks"]) - statistics.median(times["world1"])))
    if "ordered" in times and "ranks" in times:
        say("ordered - ranks: %+.2f ms/step (a self all-gather and one rank_sum launch in place of the self all-reduce)" %
            (statistics.median(times["ordered"]) - statistics.median(times["ranks"])))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
