"""The kernels of the 3D-ResNet encoders (fused_resnet3d.ResNet3dMFMA) at the shapes the default encoder runs, against float64:
every convolution path of tests/resnet3d_cases.py (the production batch's XL tile, strided 27-tap layers, the tap table in global
memory, the dispatcher's boundaries), and the 7x7x7 stem reading a frame table through frame ids.

The float64 references are computed on the device (explicit patch gather + float64 matmul) and compared over every output row."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from resnet3d_cases import CASES, TOL, bare_symbol, k_all, m_out, n_ksteps, out_dims

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

X3 = {"bf16x3": 0, "f16x3": 1}
# K-steps of 64 of the cases whose tap table placement they pin (kMaxTabSteps = 128: above it the table stays in global memory)
NK = {"layer2_0_downsample": 1, "layer3_conv2_res_xl": 108, "layer4_conv2_res": 216, "layer4_conv2_res_b133": 216,
      "boundary_k8192": 128, "boundary_k8256": 129}


def _fold64(conv, bn):
    """float64 (weight [Cout, K] tap-major with the channel innermost, bias) of conv + eval BN."""
    w = conv.weight.detach().double()
    scale = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    bias = bn.bias.detach().double() - bn.running_mean.detach().double() * scale
    w = w * scale.view(-1, 1, 1, 1, 1)
    return w.permute(0, 2, 3, 4, 1).reshape(w.shape[0], -1), bias


def _conv_rows(x, wm, bias, kernel, stride, pad):
    """x [B, T, H, W, C] on the device, wm [Cout, K] (K = kt * kh * kw * C, tap-major), bias [Cout] -> the convolution as [M, Cout]
    rows ordered (b, t, h, w), in x's dtype: an explicit patch gather and a matmul, a few output frames at a time."""
    (kt, kh, kw), (st, sh, sw), (pt, ph, pw) = kernel, stride, pad
    u = F.pad(x, (0, 0, pw, pw, ph, ph, pt, pt)).unfold(1, kt, st).unfold(2, kh, sh).unfold(3, kw, sw)  # [B,To,Ho,Wo,C,kt,kh,kw]
    b, to, ho, wo = u.shape[:4]
    k = wm.shape[1]
    step = max(1, (1 << 26) // (ho * wo * k))
    out = []
    for i in range(b):
        for t0 in range(0, to, step):
            p = u[i, t0 : t0 + step].permute(0, 1, 2, 4, 5, 6, 3).reshape(-1, k)
            out.append(torch.addmm(bias, p, wm.t()))
    return torch.cat(out)


def _check(got, ref64, ref32, mode, what):
    """Max |got - ref64| against TOL[mode] * max(scale, 1) + 2 * |ref32 - ref64|; prints the margin."""
    scale = ref64.abs().max().item()
    err32 = (ref32.double() - ref64).abs().max().item()
    err = (got.double() - ref64).abs().max().item()
    bound = TOL[mode] * max(scale, 1.0) + 2 * err32
    msg = "%s %s: max err %.3e, bound %.3e (scale %.3f, torch fp32 err %.3e)" % (what, mode, err, bound, scale, err32)
    print(msg)
    assert torch.isfinite(got).all() and err < bound, msg


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_conv_resnet_shape_matches_fp64(avt, dev, case):
    """FusedConv (BN folded, residual + ReLU where the layer has them) at a ResNet encoder shape, both plane types, against float64
    of the same folded arithmetic over every output row; the case lands on the kernel (and K-step count) it names."""
    from avtex.fused_slowfast import Act, FusedConv, fold_bn, split_planes

    torch.manual_seed(CASES.index(case) + 1)
    conv = nn.Conv3d(case.cin, case.cout, case.kernel, stride=case.stride, padding=case.pad, bias=False)
    bn = nn.BatchNorm3d(case.cout)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5); bn.bias.uniform_(-0.5, 0.5)
        bn.running_mean.uniform_(-0.2, 0.2); bn.running_var.uniform_(0.5, 1.5)
    bn.eval()
    od, m = out_dims(case), m_out(case)
    g = torch.Generator(device=dev).manual_seed(17)
    x = torch.randn(case.dims + (case.cin,), device=dev, generator=g)
    r = torch.randn((m, case.cout), device=dev, generator=g) if case.res else None
    wm64, b64 = _fold64(conv, bn)
    w32, b32 = fold_bn(conv, bn)
    wm32 = w32.permute(0, 2, 3, 4, 1).reshape(case.cout, -1)
    refs = []
    for xx, wm, bias in ((x.double(), wm64, b64), (x, wm32, b32)):
        y = _conv_rows(xx, wm.to(dev), bias.to(dev), case.kernel, case.stride, case.pad)
        if r is not None:
            y = y + r.to(y.dtype)
        refs.append(F.relu(y) if case.relu else y)
    assert refs[0].shape == (m, case.cout)
    k = k_all(case.cin, case.kernel)
    for mode in ("bf16x3", "f16x3"):
        pd = X3[mode]
        fc = FusedConv(conv, bn, case.relu, dev, x3=pd)
        assert bare_symbol(fc.kernel_symbol(m)) == case.symbol, (case.name, fc.kernel_symbol(m))
        assert fc.wt.shape[1] == k and n_ksteps(k) == NK.get(case.name, n_ksteps(k))
        assert fc.pw is None and fc.lat is None and fc.group_factor(Act(x.view(-1, case.cin), case.dims), None, None) == 1
        if case.blocked is not None:
            assert (fc.wblk is not None) == case.blocked, case.name
        xh, xl = split_planes(x.view(-1, case.cin), pd)
        res = None
        if r is not None:
            rh, rl = split_planes(r, pd)
            res = Act(rh, od, lo=rl)
        out = fc(Act(xh, case.dims, 0, case.cin, lo=xl), res=res)
        torch.cuda.synchronize()
        assert out.dims == od and out.buf.shape == (m, case.cout)
        _check(out.float(pd), refs[0], refs[1], mode, "%s (%s, M %d, K %d, nk %d)" % (case.name, case.symbol, m, k, n_ksteps(k)))


def _stem_net(hw, window, mode, dev):
    """(randomised-BN ResNet3d-18 at hw^2 / window, its ResNet3dMFMA)."""
    from avtex import resnet3d, synth
    from avtex.fused_resnet3d import ResNet3dMFMA

    torch.manual_seed(21)
    net = synth.randomise_bn(resnet3d.build("resnet18", hw, window), 121, 0.5).eval()
    return net, ResNet3dMFMA(nn.Sequential(net, nn.AdaptiveAvgPool3d(1)), dev, mode)


def _stem_table(hw, n_frames, pd, dev):
    """fp32 frames [n_frames + 1, 3, hw, hw] (the last one zero) and their plane-pair table [n_frames + 1, hw, hw, 4] as
    TextureEngine.set_video writes it (channel 3 zero, the zero frame last)."""
    from avtex import ops

    g = torch.Generator(device=dev).manual_seed(5)
    src = torch.randn((n_frames + 1, 3, hw, hw), device=dev, generator=g)
    src[n_frames] = 0
    hi, lo = ops.clip_planes_f32(src.permute(1, 0, 2, 3).unsqueeze(0), pd)
    return src, hi[0], lo[0]


def _stem_ids(nf, window):
    """Frame-id windows into a table of nf frames + the zero frame (id nf): a plain window; repeated, out-of-order ids; the zero
    frame at the start, in the middle and at the end; the table's last frames."""
    z = nf
    rng = np.random.RandomState(3)
    mixed = rng.randint(0, nf, window)
    mixed[1], mixed[-2] = mixed[0], mixed[-1]
    ids = [np.arange(window) + 2, mixed, np.arange(window) + 5, np.arange(window) + 1, np.arange(window) + nf - window - 3,
           np.arange(nf - window, nf)]
    ids[2][:3] = z
    ids[3][window // 2 - 1 : window // 2 + 2] = z
    ids[4][-3:] = z
    ids = np.stack(ids)
    assert (np.diff(ids[1]) < 0).any() and len(set(ids[1])) < window
    return ids


def _stem_ref(net, src, ids, dev):
    """float64 / fp32 Conv3d [7,7,7] stride (1,2,2) pad 3 + folded BN + ReLU of the gathered clips -> [b * t * ho * wo, 64] each."""
    b, t = ids.shape
    hw = src.shape[-1]
    clips = src.index_select(0, torch.from_numpy(ids.reshape(-1)).to(dev)).view(b, t, 3, hw, hw).permute(0, 1, 3, 4, 2)
    wm64, b64 = _fold64(net.conv1, net.bn1)
    from avtex.fused_slowfast import fold_bn

    w32, b32 = fold_bn(net.conv1, net.bn1)
    wm32 = w32.permute(0, 2, 3, 4, 1).reshape(w32.shape[0], -1)
    return [F.relu(_conv_rows(xx, wm.to(dev), bias.to(dev), (7, 7, 7), (1, 2, 2), (3, 3, 3)))
            for xx, wm, bias in ((clips.double(), wm64, b64), (clips.contiguous(), wm32, b32))]


@pytest.mark.parametrize("mode", ["bf16x3", "f16x3"])
@pytest.mark.parametrize("hw,window", [(224, 20), (64, 8)])
def test_stem_frame_ids_match_fp64(avt, dev, hw, window, mode):
    """The patch-resident 7x7x7 stem (avt_stem_conv_x3, kt 7, pt 3, BN folded, ReLU) reading an engine-shaped frame table through
    frame ids (112 and 32 pixel pairs) == float64 of the gathered clips, elementwise over every output frame (the first and last
    three are where the temporal padding acts)."""
    from avtex import ops
    from avtex.fused_slowfast import Act, new_act

    pd = X3[mode]
    net, enc = _stem_net(hw, window, mode, dev)
    conv, pw = enc.stem, hw // 2
    assert ops.stem_conv_supported(hw, pw, conv.cout) and conv.wt_lds_lo is not None
    assert conv.kernel[0] == 7 and conv.stride[0] == 1 and conv.pad[0] == 3
    nf = 2 * window + 8
    src, th, tl = _stem_table(hw, nf, pd, dev)
    assert th.shape == (nf + 1, hw, hw, 4)
    ids = _stem_ids(nf, window)
    b = len(ids)
    fidx = torch.from_numpy(ids.reshape(-1).astype(np.int32)).to(dev)
    x = Act(th.reshape(-1, 8), (b, window, hw, pw), lo=tl.reshape(-1, 8))
    od = conv.out_dims((b, window, hw, pw))
    assert od == (b, window, hw // 2, hw // 2)
    y = new_act(od[0] * od[1] * od[2] * od[3], conv.cout, od, dev, True)
    ops.stem_conv_x3(x.ptrs, conv.wt_lds, conv.wt_lds_lo, conv.bias, conv.wscale, y.ptrs, b, window, hw, pw, conv.cout,
                     conv.kernel[0], conv.stride[0], conv.pad[0], enc.x3, relu=True, frame_idx=fidx, table_frames=nf + 1)
    torch.cuda.synchronize()
    ref64, ref32 = _stem_ref(net, src, ids, dev)
    _check(y.float(pd), ref64, ref32, mode, "stem %d^2 W=%d frame ids" % (hw, window))


@pytest.mark.parametrize("mode", ["bf16x3", "f16x3"])
def test_stem_general_tile_matches_fp64(avt, dev, mode):
    """At 48^2 (24 pixel pairs: no patch-resident kernel) ResNet3dMFMA.stem runs on the general tile over the clips gathered from
    the frame table, as forward_frames does; == float64 of the same windows."""
    from avtex import ops
    from avtex.fused_slowfast import Act

    pd = X3[mode]
    hw, window = 48, 8
    net, enc = _stem_net(hw, window, mode, dev)
    pw = hw // 2
    assert not ops.stem_conv_supported(hw, pw, enc.stem.cout)
    nf = 2 * window + 8
    src, th, tl = _stem_table(hw, nf, pd, dev)
    ids = _stem_ids(nf, window)
    b = len(ids)
    flat = torch.from_numpy(ids.reshape(-1)).to(dev)
    x = Act(th.index_select(0, flat).reshape(-1, 8), (b, window, hw, pw), lo=tl.index_select(0, flat).reshape(-1, 8))
    y = enc.stem(x)
    torch.cuda.synchronize()
    assert y.dims == (b, window, hw // 2, hw // 2)
    ref64, ref32 = _stem_ref(net, src, ids, dev)
    _check(y.float(pd), ref64, ref32, mode, "stem %d^2 W=%d general tile" % (hw, window))
