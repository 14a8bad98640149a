"""Time train_ops.ArenaSGD.step() (one launch of csrc/sgd.hip over all parameters) next to torch.optim.SGD(fused=True).step() on the
parameter set of config 5: the SlowFast query + target encoders in the training layout (about 69 M fp32 elements), momentum 0.9,
weight decay 1e-4.  The two are interleaved in one process, ten rounds each after a warm-up; a round is `--steps` optimizer steps
between two device events (a step alone is a fraction of a millisecond).  Prints every round, the medians and spreads, and the kernel's
achieved bytes per second against the 20 B per element the update has to move (p, g, buf read; p, buf written).

    python tools/probe_arena_sgd.py [--rounds 10] [--steps 20] [--out profiles/r11/arena_sgd_probe.log]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the log to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_arena_sgd: needs the MI355X (no timing without a device)")
    import avtex
    from avtex import train_ops
    from avtex.slowfast import SlowFast

    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s" % avtex.ops.device_check())
    torch.manual_seed(0)

    def params():
        net = train_ops.training_layout(torch.nn.ModuleList([SlowFast(), SlowFast()]).to(dev))
        ps = [p for p in net.parameters()]
        for p in ps:
            p.grad = torch.randn_like(p) * 0.01
        return ps

    kw = dict(lr=0.01, momentum=0.9, weight_decay=1e-4)
    pa, pt = params(), params()
    oa, ot = train_ops.ArenaSGD(pa, **kw), torch.optim.SGD(pt, fused=True, **kw)
    numel = sum(p.numel() for p in pa)
    say("%d tensors, %d elements (%.1f MB of parameters), %d blocks of 4096 elements" %
        (len(pa), numel, numel * 4 / 1e6, sum((p.numel() + 4095) // 4096 for p in pa)))

    def timed(opt):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            opt.step()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.steps

    for _ in range(3):  # warm-up: code objects, the job table, torch's first-step buffers
        timed(oa)
        timed(ot)
    ta, tt = [], []
    for r in range(a.rounds):
        ta.append(timed(oa))
        tt.append(timed(ot))
        say("round %2d: ArenaSGD %.4f ms/step   torch fused SGD %.4f ms/step" % (r, ta[-1], tt[-1]))
    ma, mt = statistics.median(ta), statistics.median(tt)
    say("ArenaSGD        median %.4f ms/step (min %.4f, max %.4f): %.2f TB/s at 20 B per element" %
        (ma, min(ta), max(ta), numel * 20 / (ma * 1e-3) / 1e12))
    say("torch fused SGD median %.4f ms/step (min %.4f, max %.4f): %.2f TB/s at 20 B per element" %
        (mt, min(tt), max(tt), numel * 20 / (mt * 1e-3) / 1e12))
    say("ratio ArenaSGD / torch %.3f; spread of the torch rounds %.1f %% of their median" % (ma / mt, 100 * (max(tt) - min(tt)) / mt))
    say("launches: ArenaSGD %d (one per step)" % train_ops.CALLS["sgd_multi"])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
