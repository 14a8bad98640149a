"""The 3D-ResNet encoders (the CLI's default --enc_arch resnet18) in the TRAINING step on the hand-written passes of train_ops:
launch accounting of one item, the step against fp64 next to the stock fp32 step (the form and constants of
test_gpu_train_step.test_config5_default_step_at_size_runs_the_hand_written_kernels), the --train_conv fp32 switch, and twenty SGD
steps next to the stock path with the trained weights handed to ResNet3dMFMA.

Items come from AudioVideoSegments.__getitem__ + a batch axis — the ResNet training path's own input (train.py feeds the DataLoader's
[B,W,3,H,W] / [B,1+negs,W,3,H,W] tensors): DeviceSegmentBatcher packs SlowFast's two-pathway clips only and refuses other encoders.
A 40 fps clip gives the dataset's window of 20 frames (window = ceil(fps / 2))."""
import copy
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

W = 20


def _grad_dist(g, g64):
    per = {k: float((g[k] - g64[k]).norm()) / (float(g64[k].norm()) + 1e-30) for k in g64}
    num = sum(float((g[k] - g64[k]).norm()) ** 2 for k in g64)
    den = sum(float(g64[k].norm()) ** 2 for k in g64)
    return (num / den) ** 0.5, max(per.values())


def _dataset(avt, hw, n_negs=14, frames=200):
    from avtex import synth

    args = SimpleNamespace(vdata="/tmp", adata=None, n_negs=n_negs, img_size=hw, enc_arch="resnet18", window=0, stride=0)
    torch.manual_seed(5)
    ds = avt.AudioVideoSegments(args, "x", split="train", video=(synth.structured_video(3, frames, 64, 64), 40.0))
    assert ds.window == W
    return ds


def _item(ds, idx, dev):
    it = ds[idx]
    return it[0].unsqueeze(0).to(dev), it[3].unsqueeze(0).to(dev)  # [1, W, 3, H, W], [1, 1 + negs, W, 3, H, W]


def _model(avt, arch, hw, seed=0):
    from avtex import resnet3d, synth

    torch.manual_seed(seed)
    base = avt.ContrastivePredictionTemporal(resnet3d.build(arch, hw, W), resnet3d.build(arch, hw, W), None, 1, 512, temp=0.1,
                                             window=W, stride=8, enc_arch=arch, img_size=hw)
    return synth.randomise_bn(base, 4, 0.0)


class _stock_ops:
    """Every train_ops switch off: the parent's step (MIOpen autograd)."""

    def __enter__(self):
        from avtex import train_ops

        self.keep = (train_ops._FUSED, train_ops._CONV_X3, train_ops._WGRAD_X3)
        train_ops._FUSED = train_ops._CONV_X3 = train_ops._WGRAD_X3 = 0

    def __exit__(self, *exc):
        from avtex import train_ops

        train_ops._FUSED, train_ops._CONV_X3, train_ops._WGRAD_X3 = self.keep
        return False


def _layer4_positions(arch, hw):
    from avtex import fused_resnet3d

    plan = dict((n, e) for n, e, _ in fused_resnet3d.layer_plan(arch, hw, W))
    last = [n for n in plan if n.startswith("layer4")][-1]
    return int(np.prod(plan[last]))


def test_one_item_runs_the_hand_written_kernels(avt, dev):
    """(a) Launch accounting of one resnet18 item (1 query + 15 targets) at 64^2, both encoders, forward + backward."""
    from avtex import train_ops

    hw = 64
    ds = _dataset(avt, hw)
    np.random.seed(3)
    q, t = _item(ds, 10, dev)
    assert q.shape == (1, W, 3, hw, hw) and t.shape == (1, 15, W, 3, hw, hw)
    m = train_ops.training_layout(_model(avt, "resnet18", hw).to(dev)).train()
    assert train_ops.conv_mode() == "x3"
    before = dict(train_ops.CALLS)
    out = m(q, t)
    avt.InfoNCECriterion()(out, torch.zeros(1, dtype=torch.long, device=dev)).backward()
    torch.cuda.synchronize()
    ran = {k: train_ops.CALLS[k] - before[k] for k in before}
    print("hand-written training launches of one resnet18 item:", ran)
    mods = list(m.q_encoder.modules()) + list(m.t_encoder.modules())
    n_conv = sum(1 for mod in mods if isinstance(mod, nn.Conv3d))
    n_bn = sum(1 for mod in mods if isinstance(mod, nn.BatchNorm3d))
    assert n_conv == 2 * 20 and n_bn == 2 * 20
    assert ran["conv_fwd_x3"] == n_conv, (ran, n_conv)
    assert ran["miopen_wgrad"] == 0 and ran["miopen_dgrad"] == 0, ran  # no MIOpen convolution left in the step
    assert ran["wgrad_x3"] + ran["wgrad_stem_x3"] + ran["wgrad_stem_patch"] == ran["conv_fwd_x3"], ran
    assert ran["maxpool3d_hip"] == 2, ran
    assert ran["bn_bwd"] == ran["bn_fwd"] == n_bn, (ran, n_bn)
    # conv3d_fork adds the projection's input gradient to conv1's after BOTH strided launches (the residue-class launches have no
    # add epilogue): the projection's input gradient is a launch family of its own, 3 stride-2 3x3x3 + 3 stride-2 projections per encoder
    assert ran["dgrad_strided_x3"] == 2 * (3 + 3), ran
    # the 7x7x7 stem shipped on the generic route (the patch-resident weight gradient needs 284 KB of LDS at kt = 7)
    assert ran["stem_fwd_patch"] == 0 and ran["wgrad_stem_patch"] == 0 and ran["wgrad_stem_x3"] == 2, ran
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for n, p in m.named_parameters() if ".fc." not in n)


@pytest.mark.parametrize("arch,hw", [("resnet18", 64), ("resnet10", 64), ("resnet18", 224)])
def test_step_against_fp64(avt, dev, arch, hw):
    """(b) The product step (fp32 tensors, x3 arithmetic, training layout) and the stock fp32 step (MIOpen, torch layout) against the
    stock fp64 step on the same weights and clips.  Bounds: test_gpu_train_step's."""
    from avtex import train_ops

    assert _layer4_positions(arch, hw) >= 1
    ds = _dataset(avt, hw)
    np.random.seed(3)
    q, t = _item(ds, 10, dev)
    base = _model(avt, arch, hw)
    label = torch.zeros(1, dtype=torch.long, device=dev)

    def run(dtype, product):
        m = copy.deepcopy(base).to(dev, dtype).train()
        qq, tt = q.to(dtype), t.to(dtype)
        if product:
            m = train_ops.training_layout(m)
            out = m(qq, tt)  # models._InfoNCELogits (HIP normalise -> bmm -> /temp) + HIP CE
            loss = avt.InfoNCECriterion()(out, label)
        else:  # plain PyTorch in `dtype` (models.py:385-417 restated) on the stock ops
            with _stock_ops():
                qv = m.q_encoder(qq.permute(0, 2, 1, 3, 4).contiguous()).view(1, -1)
                tv = m.t_encoder(tt.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, 3, W, hw, hw)).view(1, 15, -1)
                out = torch.bmm(F.normalize(qv, dim=1).unsqueeze(1), F.normalize(tv, dim=2).permute(0, 2, 1)).view(1, 15) / 0.1
                loss = nn.CrossEntropyLoss()(out, label)
                loss.backward()
        if product:
            loss.backward()
        torch.cuda.synchronize()
        g = {k: p.grad.detach().double().cpu() for k, p in m.named_parameters() if p.grad is not None}
        return out.detach().double().cpu(), float(loss), g

    assert train_ops.conv_mode() == "x3"
    before = dict(train_ops.CALLS)
    out_p, loss_p, g_p = run(torch.float32, True)
    assert train_ops.CALLS["conv_fwd_x3"] - before["conv_fwd_x3"] > 0 and train_ops.CALLS["miopen_dgrad"] == before["miopen_dgrad"]
    before = dict(train_ops.CALLS)
    out_s, loss_s, g_s = run(torch.float32, False)
    out_64, loss_64, g_64 = run(torch.float64, False)
    assert train_ops.CALLS == before  # the two reference steps ran none of the hand-written passes
    d_p, d_s = float((out_p - out_64).abs().max()), float((out_s - out_64).abs().max())
    print("%s %d^2 logits vs fp64: product %.3e, stock fp32 %.3e; loss %.6f / %.6f / %.6f" % (arch, hw, d_p, d_s, loss_p, loss_s, loss_64))
    assert set(g_p) == set(g_64)
    all_p, worst_p = _grad_dist(g_p, g_64)
    all_s, worst_s = _grad_dist(g_s, g_64)
    print("%s %d^2 gradients vs fp64: product %.3e (worst tensor %.3e), stock fp32 %.3e (worst %.3e)" % (arch, hw, all_p, worst_p, all_s, worst_s))
    assert d_p < 1e-3, d_p
    assert abs(loss_p - loss_64) < 1e-4
    assert all_p <= 1.5 * all_s + 1e-4, (all_p, all_s)
    assert worst_p <= 2.0 * worst_s + 1e-3, (worst_p, worst_s)


def test_train_conv_fp32_on_a_resnet3d(avt, dev):
    """(c) set_conv_mode("fp32") keeps meaning "MIOpen convolutions, fused BatchNorm passes" for the 3D-ResNets."""
    from avtex import resnet3d, train_ops

    torch.manual_seed(1)
    net = train_ops.training_layout(resnet3d.build("resnet18", 64, W).to(dev)).train()
    x = torch.randn(2, 3, W, 64, 64, device=dev)
    try:
        assert train_ops.set_conv_mode("fp32") == "fp32"
        before = dict(train_ops.CALLS)
        net(x).square().mean().backward()
        assert all(train_ops.CALLS[k] == before[k] for k in ("conv_fwd_x3", "dgrad_x3", "wgrad_x3", "dgrad_strided_x3", "wgrad_stem_x3"))
        assert train_ops.CALLS["bn_fwd"] > before["bn_fwd"]  # the fused BatchNorm passes stay
        g32 = [p.grad.clone() for p in net.parameters() if p.grad is not None]
    finally:
        train_ops.set_conv_mode("x3")
    net.zero_grad()
    before = dict(train_ops.CALLS)
    net(x).square().mean().backward()
    assert train_ops.CALLS["conv_fwd_x3"] == before["conv_fwd_x3"] + 20
    gx3 = [p.grad for p in net.parameters() if p.grad is not None]
    num = sum(float((a - b).norm()) ** 2 for a, b in zip(g32, gx3))
    den = sum(float(a.norm()) ** 2 for a in g32)
    print("resnet18 64^2: x3 gradients vs MIOpen fp32 convolutions: %.3e of the norm" % (num / den) ** 0.5)
    assert (num / den) ** 0.5 < 5e-2


def test_twenty_sgd_steps_track_the_stock_path(avt, dev):
    """(d) resnet10 at 64^2, SGD as main.py builds it (lr 1e-2, momentum 0.9, weight decay 1e-4), the same seed and batches through the
    product path and through the stock fp32 path in both layouts.  Tolerance on the loss curve: 2 x what the two STOCK runs (ncdhw
    against channels-last) differ by — the factor 2 is x3's bf16-plane gradients next to fp32.
    Then the trained weights on ResNet3dMFMA against the trained module's own eval forward, within the inference tests' bound."""
    from avtex import train_ops
    from avtex.fused_resnet3d import ResNet3dMFMA

    hw, steps = 64, 20
    ds = _dataset(avt, hw, n_negs=8, frames=260)  # an interior item overwrites 8 negatives with its temporal neighbours: 8 is the least
    np.random.seed(9)
    items = [_item(ds, int(i), dev) for i in np.random.randint(4, len(ds) - 5, size=steps)]
    base = _model(avt, "resnet10", hw, seed=2)
    label = torch.zeros(1, dtype=torch.long, device=dev)

    def train(kind):
        m = copy.deepcopy(base).to(dev).train()
        if kind != "ncdhw":
            m = train_ops.training_layout(m)
        train_ops.invalidate_weight_cache()
        opt = torch.optim.SGD(params=m.parameters(), lr=10e-3, momentum=0.9, weight_decay=0.0001)
        crit = avt.InfoNCECriterion()
        losses = []
        for q, t in items:
            opt.zero_grad(set_to_none=True)
            loss = crit(m(q, t), label)
            loss.backward()
            opt.step()
            losses.append(float(loss))
        torch.cuda.synchronize()
        return np.array(losses), m

    before = dict(train_ops.CALLS)
    lp, mp = train("product")
    assert train_ops.CALLS["conv_fwd_x3"] - before["conv_fwd_x3"] == steps * 2 * 12 and train_ops.CALLS["miopen_dgrad"] == before["miopen_dgrad"]
    with _stock_ops():
        l_cl, _ = train("channels_last")
        l_nc, _ = train("ncdhw")
    stock_gap = float(np.abs(l_cl - l_nc).max())
    gap = max(float(np.abs(lp - l_cl).max()), float(np.abs(lp - l_nc).max()))
    tol = 2.0 * stock_gap
    print("20 SGD steps resnet10 64^2: loss %.4f -> %.4f; product vs stock max |d loss| %.3e, stock ncdhw vs channels-last %.3e, tolerance %.3e"
          % (lp[0], lp[-1], gap, stock_gap, tol))
    assert np.isfinite(lp).all()
    assert gap <= tol, (gap, stock_gap, tol)
    # the trained weights on the inference kernels: weight planes and BatchNorm buffers are coherent after training
    mp.eval()
    x = torch.cat([items[0][1][0, :3], items[1][1][0, :1]]).permute(0, 2, 1, 3, 4).contiguous()
    with torch.no_grad():
        ref = mp.q_encoder(x).flatten(1)
    emb = ResNet3dMFMA(mp.q_encoder, dev)(x)
    rel = ((emb - ref).norm(dim=1) / ref.norm(dim=1)).max().item()
    print("trained resnet10 on ResNet3dMFMA (f16x3) vs its own eval forward: rel embedding error %.3e (bound 1e-4)" % rel)
    assert rel <= 1e-4, rel
