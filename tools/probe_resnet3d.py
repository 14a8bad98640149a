#!/usr/bin/env python3
"""GPU probe: the 3D-ResNet encoders (q + t, BN-calibrated) through TextureEngine.embed_windows — the nn.Module (MIOpen fp32) against
the contract-grade split-plane kernels (fused_resnet3d.ResNet3dMFMA) — and a per-layer time table of one encoder batch, with each
layer's fraction of the x3 roof (833 TFLOP/s algorithmic: a third of the bf16 dense MFMA rate, as tools/probe_x3.py).
usage: probe_resnet3d.py [--arch resnet18] [--windows 1024] [--window 20] [--stride 4] [--img 224] [--precision f16x3] [--batch 133]"""
import argparse
import sys
import time

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, ".")
import avtex  # noqa: E402,F401
import avtex.fused_slowfast as fsf  # noqa: E402
from avtex import ops, resnet3d, synth  # noqa: E402
from avtex.fused_resnet3d import ResNet3dMFMA  # noqa: E402
from avtex.texture import TextureEngine, max_enc_batch_resnet3d  # noqa: E402

X3_ROOF = 833.3  # TFLOP/s algorithmic

ap = argparse.ArgumentParser()
ap.add_argument("--arch", default="resnet18")
ap.add_argument("--windows", type=int, default=1024)
ap.add_argument("--window", type=int, default=20)
ap.add_argument("--stride", type=int, default=4)
ap.add_argument("--img", type=int, default=224)
ap.add_argument("--precision", default="f16x3")
ap.add_argument("--batch", type=int, default=0, help="encoder batch (0 = texture.max_enc_batch_resnet3d)")
a = ap.parse_args()
dev = torch.device("cuda:0")
W, S, hw, N = a.window, a.stride, a.img, a.windows
batch = a.batch or max_enc_batch_resnet3d(hw, W)

video = synth.structured_video(5, N * S + W, hw, hw, device=dev, variety=1)  # N windows
probe = TextureEngine(nn.Identity(), nn.Identity(), None, window=W, stride=S, img_size=hw, device=dev, enc_arch=a.arch)
probe.set_video(video)
cal = np.linspace(0, N - 1, 8).astype(np.int64)[:, None] * S + np.arange(W)[None, :]
clips = probe._norm_pad.index_select(0, torch.from_numpy(cal.reshape(-1)).to(dev)).view(8, W, 3, hw, hw).permute(0, 2, 1, 3, 4).contiguous()
del probe
mods = []
for seed in (10, 11):
    torch.manual_seed(seed)
    m = nn.Sequential(synth.randomise_bn(resnet3d.build(a.arch, hw, W), seed + 100, 0.5), nn.AdaptiveAvgPool3d(1)).to(dev)
    for bn in m.modules():
        if isinstance(bn, nn.BatchNorm3d):
            bn.momentum = 1.0
    m.train()
    with torch.no_grad():
        m(clips)
    mods.append(m.eval())
del clips


def timed_embed(q, t, label, enc_batch):
    eng = TextureEngine(q, t, None, window=W, stride=S, img_size=hw, device=dev, enc_batch=enc_batch, enc_arch=a.arch)
    n = eng.set_video(video)
    starts = np.arange(n, dtype=np.int64) * S
    eng.embed_windows([eng.q_enc, eng.t_enc], starts=starts[: min(n, eng.enc_batch)])  # warm-up (solver search, tables)
    torch.cuda.synchronize()
    best = None
    for _ in range(2):
        t0 = time.time()
        qv, tv = eng.embed_windows([eng.q_enc, eng.t_enc], starts=starts)
        torch.cuda.synchronize()
        dt = time.time() - t0
        best = dt if best is None else min(best, dt)
    print("%-28s %d windows x 2 encoders, enc_batch %d: %.3f s -> %.1f clip-windows/s" % (label, n, eng.enc_batch, best, n / best),
          flush=True)
    return qv, tv, n / best, eng


torch.backends.cudnn.benchmark = False
q32, t32, r_mod, _ = timed_embed(mods[0], mods[1], "module (fp32, MIOpen)", 32)
qe, te = ResNet3dMFMA(mods[0], dev, a.precision), ResNet3dMFMA(mods[1], dev, a.precision)
qv, tv, r_mfma, eng = timed_embed(qe, te, "mfma %s (frame table)" % a.precision, batch)
rel = max(((qv - q32).norm(dim=1) / q32.norm(dim=1)).max().item(), ((tv - t32).norm(dim=1) / t32.norm(dim=1)).max().item())
nq, nt = torch.nn.functional.normalize(qv, dim=1), torch.nn.functional.normalize(tv, dim=1)
nq32, nt32 = torch.nn.functional.normalize(q32, dim=1), torch.nn.functional.normalize(t32, dim=1)
ds = ((nq @ nt.T - nq32 @ nt32.T).abs().max() / 0.1).item()
print("speed-up %.2fx; rel embedding error %.2e, max |d score| %.2e over the %d x %d matrix" % (r_mfma / r_mod, rel, ds, len(qv), len(tv)))

# ---- per-layer table: one encoder batch of the query encoder, HIP events around every launch -------------------------------------
recs = []


def ev(name, launch, flops, nbytes):
    b0, b1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    b0.record()
    r = launch()
    b1.record()
    recs.append((name, b0, b1, flops, nbytes))
    return r


names, j = [], 0  # the forward's launch order: per block [downsample], conv1, conv2
for k, n_blocks in enumerate(qe.layers):
    for i in range(n_blocks):
        if qe.blocks[j][2] is not None:
            names.append("layer%d.%d.downsample" % (k + 1, i))
        names += ["layer%d.%d.conv1" % (k + 1, i), "layer%d.%d.conv2" % (k + 1, i)]
        j += 1
conv_names = iter(names)
fsf.PROFILER = lambda sym, launch, flops, nbytes: ev("%s  %s" % (next(conv_names), sym.replace("<f16>", "").replace("<bf16>", "")),
                                                     launch, flops, nbytes)
orig_stem, orig_pool, orig_mean = ops.stem_conv_x3, ops.maxpool3d_k3s2_x3, ops.mean_positions_x3


def stem(x_ptrs, wt_hi, wt_lo, bias, wscale, out_ptrs, b, t, h, pw, cout, kt, st, pt, pd, **kw):
    fl = 2.0 * b * t * (h // 2) * pw * cout * kt * 7 * 7 * 3
    return ev("conv1 (stem, patch-resident, frame table)", lambda: orig_stem(x_ptrs, wt_hi, wt_lo, bias, wscale, out_ptrs, b, t, h, pw,
                                                                             cout, kt, st, pt, pd, **kw), fl, 4.0 * b * t * (h // 2) * pw * cout)


def pool(x_ptrs, out_ptrs, b, t, h, w, c, ldi, ldo, pd):
    nb = 4.0 * b * c * (t * h * w + ((t + 1) // 2) * ((h + 1) // 2) * ((w + 1) // 2))
    return ev("maxpool 3x3x3/2", lambda: orig_pool(x_ptrs, out_ptrs, b, t, h, w, c, ldi, ldo, pd), 0.0, nb)


def mean(x_ptrs, b, p, c, ldi, out, col0, pd):
    return ev("avgpool (mean over positions)", lambda: orig_mean(x_ptrs, b, p, c, ldi, out, col0, pd), 0.0, 4.0 * b * p * c)


ops.stem_conv_x3, ops.maxpool3d_k3s2_x3, ops.mean_positions_x3 = stem, pool, mean
fidx = torch.from_numpy((np.arange(batch)[:, None] * S + np.arange(W)[None, :]).reshape(-1).astype(np.int32)).to(dev)
qe.forward_frames(eng._table[0], eng._table[1], fidx, batch, W)  # warm
torch.cuda.synchronize()
recs.clear()
conv_names = iter(names)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
qe.forward_frames(eng._table[0], eng._table[1], fidx, batch, W)
e1.record()
torch.cuda.synchronize()
tot = e0.elapsed_time(e1)
timed = sum(r[1].elapsed_time(r[2]) for r in recs)
fl_all = sum(r[3] for r in recs)
print("\nper-layer, one encoder batch of %d clips (%s %d^2, W = %d, %s): forward %.2f ms (%.1f clips/s per encoder), launches %.2f ms, "
      "%.1f GMAC per clip, %.3f of the x3 roof overall" % (batch, a.arch, hw, W, a.precision, tot, batch / tot * 1e3, timed,
                                                          fl_all / 2 / batch / 1e9, fl_all / tot / 1e9 / X3_ROOF))
print("%9s %6s %9s %8s %8s  %s" % ("ms", "share", "TFLOP/s", "of roof", "GB/s", "layer"))
for name, b0, b1, fl, nb in recs:
    t = b0.elapsed_time(b1)
    print("%9.3f %6.3f %9.1f %8.3f %8.0f  %s" % (t, t / timed, fl / t / 1e9, fl / t / 1e9 / X3_ROOF, nb / t / 1e6, name))
