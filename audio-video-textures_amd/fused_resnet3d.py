"""The 3D-ResNet encoders (resnet3d.py: resnet10/18/34/50, the reference's default `--enc_arch resnet18`) on the contract-grade
split-plane kernels.

Takes the operator's encoder — nn.Sequential(ResNet3d, AdaptiveAvgPool3d(1)) (models.py:253-260) or a bare ResNet3d — folds every
BatchNorm into its convolution (eval-mode statistics) and runs the network on NDHWC plane pairs (value = hi + lo, include/avt.h):

    conv1 [7,7,7] stride (1,2,2) + BN + ReLU   the patch-resident stem kernel (avt_stem_conv_x3) on a frame table read through a
                                               frame index, or the pixel-pair general tile on shapes that kernel does not cover
    maxpool MaxPool3d(3, 2, 1)                 avt_maxpool3d_k3s2_ndhwc_x3
    BasicBlock                                 conv1 + BN + ReLU; downsample [1,1,1] stride s + BN; conv2 + BN + residual + ReLU
                                               in conv2's epilogue — three (two) avt_conv3d_igemm_x3 launches
    avgpool + AdaptiveAvgPool3d(1)             avt_mean_positions_x3 -> fp32 [B, 512] (layer4's extent IS the AvgPool kernel:
                                               layer_plan checks it); fc is never applied, as in the module.
"""
import math
from types import SimpleNamespace

import torch
import torch.nn as nn

from . import ops
from ._lib import AvtError
from .fused_slowfast import PRECISIONS, Act, FusedConv, new_act, stem_conv
from .resnet3d import LAYERS, ResNet3d

# widths of layer1 .. layer4 and the first-block stride of each (resnet3d.ResNet3d._make)
_WIDTHS = (64, 128, 256, 512)
_STRIDES = (1, 2, 2, 2)
STEM_COUT = 64


def _half(n):
    return (n - 1) // 2 + 1  # a 3-tap (7-tap) stride-2 window with padding 1 (3): ceil(n / 2)


def layer_plan(arch_or_layers, img_size, window):
    """Output extents (t, h, w) and channels of every layer of a ResNet3d at `img_size`^2 and `window` frames, on the host.
    -> list of (name, (t, h, w), channels) from the stem to layer4's last block, then ("avgpool", kernel, 512).  Raises AvtError when
    layer4's extent is not the module's AvgPool3d kernel (ceil(W/16), ceil(hw/32), ceil(hw/32)) — the head's mean over layer4's
    positions is the module's AvgPool3d + AdaptiveAvgPool3d(1) only then."""
    layers = LAYERS[arch_or_layers] if isinstance(arch_or_layers, str) else list(arch_or_layers)
    t, h, w = int(window), _half(int(img_size)), _half(int(img_size))  # conv1: T pad 3 stride 1, H / W stride 2 pad 3
    plan = [("conv1", (t, h, w), STEM_COUT)]
    t, h, w = _half(t), _half(h), _half(w)
    plan.append(("maxpool", (t, h, w), STEM_COUT))
    for k, (n_blocks, c, s) in enumerate(zip(layers, _WIDTHS, _STRIDES)):
        for i in range(n_blocks):
            if i == 0 and s != 1:
                t, h, w = (t - 1) // s + 1, (h - 1) // s + 1, (w - 1) // s + 1
            plan.append(("layer%d.%d" % (k + 1, i), (t, h, w), c))
    kernel = (int(math.ceil(window / 16)), int(math.ceil(img_size / 32)), int(math.ceil(img_size / 32)))
    if (t, h, w) != kernel:
        raise AvtError("ResNet3d plan: layer4 extent %s is not the AvgPool3d kernel %s at %d^2, W = %d" % ((t, h, w), kernel,
                                                                                                        img_size, window))
    plan.append(("avgpool", kernel, _WIDTHS[-1]))
    return plan


def resnet3d_of(model):
    """The ResNet3d inside an operator encoder (bare, or nn.Sequential(ResNet3d, AdaptiveAvgPool3d(1))), else None."""
    if isinstance(model, ResNet3d):
        return model
    if (isinstance(model, nn.Sequential) and len(model) == 2 and isinstance(model[0], ResNet3d) and
            isinstance(model[1], nn.AdaptiveAvgPool3d) and tuple(nn.modules.utils._triple(model[1].output_size)) == (1, 1, 1)):
        return model[0]
    return None


class ResNet3dMFMA(nn.Module):
    """Drop-in for a ResNet3d encoder at inference time: forward([B, 3, T, H, W] fp32) -> fp32 [B, 512], and forward_frames() on a
    frame table of plane pairs (what TextureEngine hands it).  precision "f16x3" (fp16 planes) or "bf16x3" (bf16 planes)."""

    input_layout = "ndhwc4"
    frame_table_input = True  # TextureEngine: pass a plane-pair frame table and int32 frame ids (forward_frames), not clips
    out_dim = 512

    def __init__(self, model, device, precision="f16x3"):
        super().__init__()
        if precision not in ("f16x3", "bf16x3"):
            raise AvtError("ResNet3dMFMA: precision must be f16x3 or bf16x3 (the bf16 fast path covers SlowFast only)")
        net = resnet3d_of(model)
        if net is None:
            raise AvtError("ResNet3dMFMA: expected a ResNet3d or nn.Sequential(ResNet3d, AdaptiveAvgPool3d(1)), got %s"
                           % type(model).__name__)
        net = net.eval()
        self.dev = torch.device(device)
        self.precision = precision
        self.x3 = x3 = PRECISIONS[precision]
        self.planes = precision
        self.layers = [len(l) for l in (net.layer1, net.layer2, net.layer3, net.layer4)]
        self.avg_kernel = tuple(nn.modules.utils._triple(net.avgpool.kernel_size))
        self._anchor = nn.Parameter(torch.zeros(1, device=self.dev), requires_grad=False)  # (fp32: the engine packs fp32 frames)
        self.stem = stem_conv(SimpleNamespace(conv=net.conv1, bn=net.bn1), self.dev, x3=x3)
        self.blocks = []
        for layer in (net.layer1, net.layer2, net.layer3, net.layer4):
            for blk in layer:
                down = None
                if blk.downsample is not None:
                    down = FusedConv(blk.downsample[0], blk.downsample[1], False, self.dev, x3=x3)
                self.blocks.append((FusedConv(blk.conv1, blk.bn1, True, self.dev, x3=x3),
                                    FusedConv(blk.conv2, blk.bn2, True, self.dev, x3=x3),  # + residual, then ReLU (epilogue)
                                    down))

    def plan(self, img_size, window):
        """layer_plan for this network, also checking the module's own AvgPool3d kernel (built for one sample size / duration)."""
        plan = layer_plan(self.layers, img_size, window)
        if plan[-1][1] != self.avg_kernel:
            raise AvtError("ResNet3dMFMA: the module's AvgPool3d kernel %s does not cover layer4's extent %s at %d^2, W = %d"
                           % (self.avg_kernel, plan[-1][1], img_size, window))
        return plan

    @torch.no_grad()
    def forward(self, x):
        """x [B, 3, T, H, W] (the plugin contract, models.py:332) -> fp32 [B, 512]."""
        b, c, t, h, w = x.shape
        hi, lo = ops.clip_planes_f32(x.to(self.dev, torch.float32), self.x3)
        return self.forward_frames(hi.view(b * t, h, w, 4), lo.view(b * t, h, w, 4), None, b, t)

    @torch.no_grad()
    def forward_frames(self, tab_hi, tab_lo, frame_idx, batch, t):
        """tab_* [F, H, W, 4] plane pairs (channel 3 zero; ops.clip_planes_f32); frame_idx int32 [batch * t] on the device: frame t of
        clip b is table frame frame_idx[b * t_total + t] (entries in [0, F)), or None: the table IS the clips [batch, t, ...]."""
        nf, h, w, _ = tab_hi.shape
        self.plan(h, t)  # (raises on shapes whose head would differ from the module's)
        if w % 2 or h != w:
            raise AvtError("ResNet3dMFMA: square frames of even width expected, got %dx%d" % (h, w))
        pw = w // 2
        conv = self.stem
        lds = conv.wt_lds_lo is not None and ops.stem_conv_supported(h, pw, conv.cout)
        if frame_idx is not None and lds and nf * h * pw * 16 >= (1 << 32) - 64:
            # the stem kernel addresses its table with 32-bit byte offsets: hand it only the frames this batch reads
            uniq, inv = torch.unique(frame_idx.long(), return_inverse=True)
            tab_hi, tab_lo = tab_hi.index_select(0, uniq), tab_lo.index_select(0, uniq)
            frame_idx, nf = inv.to(torch.int32).contiguous(), int(uniq.numel())
        if frame_idx is not None and not lds:  # the general tile reads dense clips: gather them
            flat = frame_idx.long()
            tab_hi, tab_lo, frame_idx, nf = tab_hi.index_select(0, flat), tab_lo.index_select(0, flat), None, batch * t
        if frame_idx is None and nf != batch * t:
            raise AvtError("ResNet3dMFMA: %d frames are not %d clips of %d" % (nf, batch, t))
        x = Act(tab_hi.reshape(nf * h * pw, 8), (batch, t, h, pw), lo=tab_lo.reshape(nf * h * pw, 8))
        if lds:
            od = conv.out_dims((batch, t, h, pw))
            y = new_act(od[0] * od[1] * od[2] * od[3], conv.cout, od, self.dev, True)
            ops.stem_conv_x3(x.ptrs, conv.wt_lds, conv.wt_lds_lo, conv.bias, conv.wscale, y.ptrs, batch, t, h, pw, conv.cout,
                             conv.kernel[0], conv.stride[0], conv.pad[0], self.x3, relu=True, frame_idx=frame_idx,
                             table_frames=nf if frame_idx is not None else 0)
        else:
            y = conv(x)
        _, t1, h1, w1 = y.dims
        pd = (batch, _half(t1), _half(h1), _half(w1))
        a = new_act(pd[0] * pd[1] * pd[2] * pd[3], STEM_COUT, pd, self.dev, True)
        ops.maxpool3d_k3s2_x3(y.ptrs, a.ptrs, batch, t1, h1, w1, STEM_COUT, y.ld, a.ld, self.x3)
        del y
        for c1, c2, down in self.blocks:
            r = down(a) if down is not None else a
            a = c2(c1(a), res=r)
        emb = torch.empty((batch, a.C), dtype=torch.float32, device=self.dev)
        ops.mean_positions_x3(a.ptrs, batch, a.buf.shape[0] // batch, a.C, a.ld, emb, 0, self.x3)
        return emb
