"""Time csrc/rank_sum.hip — the sum of the ordered gradient exchange (train_ops.GradExchange(ordered=True)) — alone, at config 5's exchange
size: `total` is exchange_layout's over the trainable parameters of the real model (two SlowFast encoders, the checkpoint-only modules
frozen: about 69 M floats), world = 2, 4 and 8 rows.  The kernel reads world * total * 4 bytes and writes total * 4.

The yardstick is measured in the same run, interleaved with the kernel round by round: a plain 16-byte-lane device copy that moves the
SAME number of bytes, (world + 1) * total * 4 in all (half read, half written) — once as this kernel at world = 1 (a row copied through
the same lanes) and once as torch's Tensor.copy_.  Medians of `--rounds` rounds of `--iters` launches between two events.

What it cannot measure on one GPU: the all-gather in front of the sum (world * total * 4 bytes received per rank over xGMI).

    python tools/probe_rank_sum.py [--rounds 7] [--iters 10] [--out profiles/r25/rank_sum_probe.log]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--worlds", default="2,4,8")
    ap.add_argument("--out", default=None, help="also write the log to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_rank_sum: needs the MI355X (no timing without a device)")
    import avtex
    from avtex import ops, train_ops
    from avtex.slowfast import SlowFast

    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    model = avtex.ContrastivePredictionTemporal(SlowFast(), SlowFast(), None, 1, 128, temp=0.1, window=20, stride=4, enc_arch="slowfast",
                                                img_size=224)
    train_ops.freeze_checkpoint_only_modules(model)
    numels = [p.numel() for p in model.parameters() if p.requires_grad]
    _, total = train_ops.exchange_layout(numels)
    del model
    say("device: %s; %d trainable tensors, exchange buffer %d floats (%.1f MB)" % (ops.device_check(), len(numels), total, total * 4 / 1e6))

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.iters  # ms per launch

    for world in [int(w) for w in a.worlds.split(",") if w]:
        nbytes = (world + 1) * total * 4
        parts = torch.randn((world, total), dtype=torch.float32, device=dev)
        out = torch.empty(total, dtype=torch.float32, device=dev)
        half = (world + 1) * total // 2 // 4 * 4  # floats copied: read + written = nbytes (to 16 bytes)
        src = torch.randn((1, half), dtype=torch.float32, device=dev)
        dst = torch.empty(half, dtype=torch.float32, device=dev)
        forms = {"rank_sum": lambda: ops.rank_sum(parts, out), "copy (this kernel, world 1)": lambda: ops.rank_sum(src, dst),
                 "copy (Tensor.copy_)": lambda: dst.copy_(src[0])}
        times = {k: [] for k in forms}
        for _ in range(a.rounds):
            for k, fn in forms.items():  # interleaved: a drift of the box lands on all forms alike
                times[k].append(timed(fn))
        say("world %d: %.0f MB moved per launch" % (world, nbytes / 1e6))
        for k in forms:
            m = statistics.median(times[k])
            moved = nbytes if k == "rank_sum" else 2 * half * 4
            say("  %-28s median %.3f ms (min %.3f, max %.3f): %.0f GB/s" % (k, m, min(times[k]), max(times[k]), moved / m / 1e6))
        say("  rank_sum / copy (this kernel): %.2f; rank_sum / Tensor.copy_: %.2f" %
            (statistics.median(times["rank_sum"]) / statistics.median(times["copy (this kernel, world 1)"]),
             statistics.median(times["rank_sum"]) / statistics.median(times["copy (Tensor.copy_)"])))
        del parts, out, src, dst
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
