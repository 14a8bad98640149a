#!/usr/bin/env python3
"""GPU probe: one training item of the default encoder (resnet18, 1 query + 15 targets, W = 20, 224^2, train mode) — forward + backward
of the q + t pair, timed three ways in ONE process, interleaved round by round:
  (a) x3      the product path: train_ops on the split-plane kernels (main.py --train_layout ndhwc --train_conv x3);
  (b) fp32    set_conv_mode("fp32"): MIOpen convolutions, fused BatchNorm passes and pool;
  (c) stock   every train_ops switch off (_FUSED = _CONV_X3 = _WGRAD_X3 = 0): MIOpen autograd in channels-last.
Then the launch families of one product step (train_ops.CALLS), the device time of its kernels by name (torch.profiler), and the stem
pool pair against its byte count (forward: x + y + the tap bytes, backward: dy + the tap bytes + dx) at 6.3 TB/s.
--input device adds the device-side input path (dataset.DeviceSegmentBatcher over the resident fp32 frame table): the table build of a
600-frame video, one batch() of 8 items against its bytes (output written + table read) at 6.3 TB/s, and the product step fed from the
host dataset (item sliced on the CPU, copied to the device) and from the batcher, interleaved round by round.
usage: probe_resnet3d_train.py [--arch resnet18] [--img 224] [--window 20] [--targets 15] [--rounds 7] [--input randn|device]
                               [--src 256] [--out profiles/r09]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, ".")
import avtex  # noqa: E402
from avtex import resnet3d, synth, train_ops  # noqa: E402

HBM_ACHIEVABLE = 6.3e12  # bytes/s the project treats as achievable

ap = argparse.ArgumentParser()
ap.add_argument("--arch", default="resnet18")
ap.add_argument("--img", type=int, default=224)
ap.add_argument("--window", type=int, default=20)
ap.add_argument("--targets", type=int, default=15)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--input", default="randn", choices=["randn", "device"])
ap.add_argument("--src", type=int, default=256, help="--input device: side of the synthetic source video")
ap.add_argument("--out", default="profiles/r09")
a = ap.parse_args()
dev = torch.device("cuda:0")
hw, W, n = a.img, a.window, a.targets
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


torch.manual_seed(0)
model = avtex.ContrastivePredictionTemporal(resnet3d.build(a.arch, hw, W), resnet3d.build(a.arch, hw, W), None, 1, 512, temp=0.1,
                                            window=W, stride=8, enc_arch=a.arch, img_size=hw)
model = train_ops.training_layout(synth.randomise_bn(model, 4, 0.0).to(dev)).train()
g = torch.Generator().manual_seed(1)
q = torch.randn((1, W, 3, hw, hw), generator=g).to(dev)
t = torch.randn((1, n, W, 3, hw, hw), generator=g).to(dev)
label = torch.zeros(1, dtype=torch.long, device=dev)
crit = avtex.InfoNCECriterion()


def step():
    model.zero_grad(set_to_none=True)
    crit(model(q, t), label).backward()


class mode:
    def __init__(self, name):
        self.name = name

    def __enter__(self):
        self.keep = (train_ops._FUSED, train_ops._CONV_X3, train_ops._WGRAD_X3)
        if self.name == "fp32":
            train_ops.set_conv_mode("fp32")
        elif self.name == "stock":
            train_ops._FUSED = train_ops._CONV_X3 = train_ops._WGRAD_X3 = 0

    def __exit__(self, *exc):
        train_ops._FUSED, train_ops._CONV_X3, train_ops._WGRAD_X3 = self.keep
        return False


def timed(name):
    with mode(name):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)


MODES = ("x3", "fp32", "stock")
say("%s, 1 + %d clips of %d x %d^2, forward + backward of q + t, train mode" % (a.arch, n, W, hw))
for m in MODES:  # warm-up: MIOpen's solver choice, weight planes, allocator
    for _ in range(2):
        timed(m)
times = {m: [] for m in MODES}
for r in range(a.rounds):  # interleaved: every round runs the three once, so drift of the box hits all three alike
    for m in MODES:
        times[m].append(timed(m))
med = {m: sorted(v)[len(v) // 2] for m, v in times.items()}
for m in MODES:
    say("  %-6s median %8.2f ms   (min %8.2f, max %8.2f over %d interleaved rounds)  %6.1f clips/s" % (
        m, med[m], min(times[m]), max(times[m]), a.rounds, (1 + n) / med[m] * 1e3))
say("  x3 / stock = %.3f, x3 / fp32 = %.3f" % (med["x3"] / med["stock"], med["x3"] / med["fp32"]))

before = dict(train_ops.CALLS)
step()
torch.cuda.synchronize()
say("launch families of one product step (train_ops.CALLS):")
for k in sorted(before):
    d = train_ops.CALLS[k] - before[k]
    if d:
        say("  %-20s %4d" % (k, d))

try:
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        step()
        torch.cuda.synchronize()
    rows = [(getattr(ev, "device_time_total", getattr(ev, "cuda_time_total", 0.0)), ev.count, ev.key) for ev in prof.key_averages()]
    rows = sorted((r for r in rows if r[0] > 0 and not r[2].startswith(("aten::", "autograd::", "_"))), reverse=True)
    total = sum(r[0] for r in rows)
    say("device time of one product step by kernel (%.2f ms in all; top 24):" % (total / 1e3))
    for tt, cnt, key in rows[:24]:
        say("  %8.3f ms %5.1f %%  x%-4d %s" % (tt / 1e3, 100.0 * tt / total, cnt, key[:110]))
except Exception as exc:  # a probe: the table is extra, the three times above are the measurement
    say("(torch.profiler kernel table not available here: %r)" % (exc,))

# the stem pool pair alone at the step's shape
pool = torch.nn.MaxPool3d(3, stride=2, padding=1).train()
for b in (1, n):
    x = torch.relu(torch.randn(b, 64, W, hw // 2, hw // 2, device=dev)).contiguous(memory_format=torch.channels_last_3d).requires_grad_(True)
    y = train_ops.max_pool3d(x, pool)
    dy = torch.randn_like(y)
    fw, bw = [], []
    for _ in range(12):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        y = train_ops.max_pool3d(x, pool)
        e[1].record()
        (gx,) = torch.autograd.grad(y, x, dy)
        e[2].record()
        torch.cuda.synchronize()
        fw.append(e[0].elapsed_time(e[1]))
        bw.append(e[1].elapsed_time(e[2]))
    fw, bw = sorted(fw)[len(fw) // 2], sorted(bw)[len(bw) // 2]
    fb = x.numel() * 4 + y.numel() * 5
    bb = y.numel() * 5 + x.numel() * 4
    say("max_pool3d %2d clips: forward %.3f ms = %.2f TB/s (%.0f %% of 6.3), backward %.3f ms = %.2f TB/s (%.0f %% of 6.3); %.1f MB each way"
        % (b, fw, fb / fw / 1e9, 100 * fb / fw / 1e9 / (HBM_ACHIEVABLE / 1e12), bw, bb / bw / 1e9,
           100 * bb / bw / 1e9 / (HBM_ACHIEVABLE / 1e12), fb / 1e6))

if a.input == "device":
    import time
    from types import SimpleNamespace

    import numpy as np

    from avtex.dataset import AudioVideoSegments, DeviceSegmentBatcher

    def med_ms(fn, reps=9):
        out = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1))
        return sorted(out)[len(out) // 2]

    fps = 2.0 * W - 1.0  # the dataset derives its window from the frame rate: ceil(fps / 2) = W
    args = SimpleNamespace(vdata="/tmp", adata=None, n_negs=n - 1, img_size=hw, enc_arch=a.arch, window=0, stride=0)
    t0 = time.time()
    ds = AudioVideoSegments(args, "probe", split="train", video=(synth.structured_video(3, 600, a.src, a.src), fps))
    say("device input path: 600 frames of %d^2 -> %d^2, window %d, stride %d, %d segments; host dataset built in %.2f s (resize + "
        "normalise on the CPU)" % (a.src, hw, ds.window, ds.stride, len(ds), time.time() - t0))
    assert ds.window == W
    u8 = ds.video_u8.to(dev)
    avtex.ops.frames_resize_aa_norm(u8, hw)
    ms = med_ms(lambda: avtex.ops.frames_resize_aa_norm(u8, hw))
    say("  table build, 600 frames %d^2 -> %d^2: %.3f ms (%.1f MB uint8 in, %.1f MB fp32 out)"
        % (a.src, hw, ms, u8.numel() / 1e6, 600 * 3 * hw * hw * 4 / 1e6))
    hd = torch.randint(0, 256, (60, 1080, 1920, 3), dtype=torch.uint8, device=dev)
    avtex.ops.frames_resize_aa_norm(hd, hw)
    ms = med_ms(lambda: avtex.ops.frames_resize_aa_norm(hd, hw))
    say("  table build, 60 frames 1080 x 1920 -> %d^2 (19 and 11 taps): %.3f ms = %.1f us a frame, %.2f TB/s of source bytes; 600 such "
        "frames: %.1f ms" % (hw, ms, ms * 1e3 / 60, hd.numel() / ms / 1e9, ms * 10))
    del hd, u8
    bat = DeviceSegmentBatcher(ds, dev).seed_from_numpy()
    idx8 = torch.arange(8) * 3 + 5
    bat.batch(idx8)
    ms = med_ms(lambda: bat.batch(idx8))
    starts = (torch.arange(8 * (1 + n), dtype=torch.int32) * 3 % (600 - W)).to(dev)
    avtex.ops.clip_gather_frames(bat.table, starts, W)
    gms = med_ms(lambda: avtex.ops.clip_gather_frames(bat.table, starts, W))
    nbytes = 2 * 8 * (1 + n) * W * 3 * hw * hw * 4
    say("  batch() of 8 items (8 x %d clips): %.3f ms, of which the gather %.3f ms = %.2f TB/s over %.1f MB (output written + table read; "
        "%.0f %% of 6.3)" % (1 + n, ms, gms, nbytes / gms / 1e9, nbytes / 1e6, 100 * nbytes / gms / 1e9 / (HBM_ACHIEVABLE / 1e12)))

    def fed(kind, i):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if kind == "host":
            it = ds[i]
            qq, tt = it[0].unsqueeze(0).to(dev), it[3].unsqueeze(0).to(dev)
        else:
            qq, tt, _, _ = bat.batch(torch.tensor([i]))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        model.zero_grad(set_to_none=True)
        crit(model(qq, tt), label).backward()
        torch.cuda.synchronize()
        return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

    np.random.seed(1)
    for kind in ("host", "device"):
        fed(kind, 7)
    res = {"host": [], "device": []}
    for r in range(a.rounds):
        for kind in ("host", "device"):
            res[kind].append(fed(kind, 10 + 3 * r))
    for kind in ("host", "device"):
        inp = sorted(v[0] for v in res[kind])[a.rounds // 2]
        stp = sorted(v[1] for v in res[kind])[a.rounds // 2]
        say("  product step fed from the %-6s: input %8.2f ms + step %8.2f ms (medians of %d interleaved rounds, wall clock)"
            % (kind, inp, stp, a.rounds))

if a.out:
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "resnet3d_train_probe.log"), "w") as f:
        f.write("\n".join(lines) + "\n")
