"""What --train_deterministic costs: config 5's SlowFast training step (1 query + 15 targets per item at 224^2, both encoders, InfoNCE,
SGD) at one item and at eight items, the default mode (weight gradients added with fp32 atomics) against the deterministic mode
(partial tiles to a workspace + a fixed-order reduction, train_ops.set_deterministic), INTERLEAVED in one process: every round times
one step of each, after two warm-up steps of each; medians, minima and maxima over the rounds, device time between two events around
the whole step.  Also printed: the largest workspace a weight gradient of the step took, the number of deterministic launches per
step, and — recorded, not asserted — whether two steps from one seed end in the same bits eagerly and as a replayed HIP graph (HIP
optimizer either way), with the first tensor that differs if they do not.

    python tools/probe_train_deterministic.py [--rounds 7] [--items 1,8] [--out profiles/r21/probe_train_deterministic.log]
"""
import argparse
import os
import statistics
import sys
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--items", default="1,8")
    ap.add_argument("--out", default=None, help="also write the log to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("probe_train_deterministic: needs the MI355X (no timing without a device)")
    if a.rounds < 7:
        raise SystemExit("probe_train_deterministic: medians of fewer than seven rounds say little")
    import avtex as avt
    from avtex import ops, synth, train_ops
    from avtex.dataset import DeviceSegmentBatcher
    from avtex.slowfast import SlowFast

    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s" % ops.device_check())
    args = SimpleNamespace(vdata="/tmp", adata=None, n_negs=14, img_size=224, enc_arch="slowfast", window=0, stride=0)
    torch.manual_seed(5)
    ds = avt.AudioVideoSegments(args, "x", split="train", video=(synth.structured_video(3, 600, 64, 64), 30.0))
    crit = avt.InfoNCECriterion()

    def fresh(seed=0):
        torch.manual_seed(seed)
        m = avt.ContrastivePredictionTemporal(SlowFast(), SlowFast(), None, 1, 128, temp=0.1, window=ds.window, stride=ds.stride,
                                              enc_arch="slowfast", img_size=224)
        return train_ops.training_layout(synth.randomise_bn(m, 4, 0.0).to(dev)).train()

    def batch(items):
        np.random.seed(3)
        return DeviceSegmentBatcher(ds, dev).seed_from_numpy().batch(torch.tensor([20 + 7 * i for i in range(items)]))

    for items in [int(v) for v in a.items.split(",")]:
        model = fresh()
        opt = torch.optim.SGD(model.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
        q, t, _, _ = batch(items)
        label = torch.zeros(items, dtype=torch.long, device=dev)

        def step(det):
            train_ops.set_deterministic(det)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            with train_ops.bn_replicas(items):
                loss = crit(model(q, t), label).mean()
            opt.zero_grad()
            loss.backward()
            opt.step()
            train_ops.invalidate_weight_cache()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1)

        for _ in range(2):
            step(False)
            step(True)
        ops.WGRAD_DET_WS_PEAK[0] = 0
        before = train_ops.CALLS["wgrad_det"]
        t_def, t_det = [], []
        for r in range(a.rounds):
            t_def.append(step(False))
            t_det.append(step(True))
            say("%d item(s) round %d: default %.2f ms   deterministic %.2f ms" % (items, r, t_def[-1], t_det[-1]))
        md, mt = statistics.median(t_def), statistics.median(t_det)
        say("%d item(s): default       median %.2f ms/step (min %.2f, max %.2f)" % (items, md, min(t_def), max(t_def)))
        say("%d item(s): deterministic median %.2f ms/step (min %.2f, max %.2f): %+.1f %% of the default's median; the default's own "
            "spread is %.1f %%" % (items, mt, min(t_det), max(t_det), 100 * (mt - md) / md, 100 * (max(t_def) - min(t_def)) / md))
        say("%d item(s): %d deterministic weight-gradient launches per step, largest workspace %.1f MB" %
            (items, (train_ops.CALLS["wgrad_det"] - before) // a.rounds, ops.WGRAD_DET_WS_PEAK[0] / 1e6))
        train_ops.set_deterministic(False)
        del model, opt

    # eager against replayed, deterministic mode, one item: two steps each from one seed
    train_ops.set_deterministic(True)
    q, t, qa, ta = batch(1)
    ends = {}
    for graph in (0, 1):
        train_ops.invalidate_weight_cache(drop=True)
        model = fresh()
        opt = train_ops.ArenaSGD(model.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
        targs = SimpleNamespace(print_freq=1000, log_freq=1000, train_graph=graph)
        zeros = torch.zeros(1, 10, device=dev)
        losses = [avt.train([(q, None, zeros if qa is None else qa, t, None, zeros if ta is None else ta)], model, opt, targs, 0)
                  for _ in range(2)]
        torch.cuda.synchronize()
        ends[graph] = (losses, {k: v.detach().clone() for k, v in model.state_dict().items()})
    train_ops.set_deterministic(False)
    (le, se), (lg, sg) = ends[0], ends[1]
    diff = [k for k in se if not torch.equal(se[k], sg[k])]
    if not diff and le == lg:
        say("deterministic mode, eager vs replayed graph (two steps, HIP optimizer): bit-equal, %d tensors, losses %s" % (len(se), le))
    else:
        k = diff[0] if diff else "(losses only)"
        worst = max([float((se[n].double() - sg[n].double()).abs().max()) for n in diff] + [0.0])
        say("deterministic mode, eager vs replayed graph (two steps, HIP optimizer): NOT bit-equal: %d of %d tensors differ, the first is "
            "%s; largest absolute difference %.3e; losses eager %s replayed %s" % (len(diff), len(se), k, worst, le, lg))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
