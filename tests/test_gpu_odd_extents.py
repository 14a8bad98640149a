"""The whole SlowFast runner at a frame size whose stages reach odd extents, in all three precisions: 72 x 56 clips give res3 an
output of 9 x 7, so res4's first slow block cannot take the strided K-concatenated form (fused_slowfast._BlockBase.scat) and runs
shortcut, a, b, c one by one, the bf16 walk leaves that form's spare columns behind the concat buffer and the split-plane walk
does not, and the stems leave the fused-pool path ((h / 2) % 8 != 0)."""
import copy

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

_SHARED = {}


def _module_inputs_reference(dev):
    """The module, the clips and the fp32 / bf16 module outputs, built once (as test_gpu_conv.test_fused_slowfast_matches_module
    builds them, at 72 x 56) and left unchanged."""
    if not _SHARED:
        from avtex.slowfast import SlowFast

        torch.manual_seed(3)
        m = SlowFast().eval()
        with torch.no_grad():
            for mod in m.modules():
                if isinstance(mod, nn.BatchNorm3d):
                    mod.weight.uniform_(0.6, 1.2); mod.bias.uniform_(-0.1, 0.1)
                    mod.running_mean.uniform_(-0.1, 0.1); mod.running_var.uniform_(0.8, 1.2)
        slow, fast = torch.randn(2, 3, 8, 72, 56), torch.randn(2, 3, 32, 72, 56)
        with torch.no_grad():
            mm = copy.deepcopy(m).to(dev)  # (m itself stays as it is: every case folds the same fp32 weights)
            ref = mm.float()([slow.to(dev), fast.to(dev)]).cpu()
            ref16 = mm.to(torch.bfloat16)([slow.to(dev, torch.bfloat16), fast.to(dev, torch.bfloat16)]).float().cpu()
        _SHARED.update(m=m, slow=slow, fast=fast, ref=ref, ref16=ref16)
    return _SHARED


@pytest.mark.parametrize("mode", ["bf16", "bf16x3", "f16x3"])
def test_odd_extent_encoder_matches_module(avt, dev, mode):
    from avtex.fused_slowfast import SlowFastMFMA

    s = _module_inputs_reference(dev)
    m, slow, fast, ref = s["m"], s["slow"], s["fast"], s["ref"]
    y = SlowFastMFMA(m, dev, precision=mode)([slow.to(dev), fast.to(dev)]).cpu()  # (the runner folds the module's fp32 weights)
    rel = ((y - ref).norm(dim=1) / ref.norm(dim=1)).max().item()
    print("%s runner vs fp32 module at 72 x 56: rel embedding error %.3e" % (mode, rel))
    assert y.shape == (2, 2304) and torch.isfinite(y).all()
    if mode == "bf16":
        # the criterion of test_fused_slowfast_matches_module: the bf16-rounded module is the yardstick
        ref16 = s["ref16"]
        cos = F.cosine_similarity(y, ref, dim=1)
        rel16 = ((ref16 - ref).norm(dim=1) / ref.norm(dim=1)).max().item()
        print("bf16 vs fp32: cos", cos.tolist(), "rel", rel, "| torch bf16 vs fp32: rel", rel16)
        assert cos.min() > 0.999 and rel < max(2.5 * rel16, 0.02)
    else:
        # the criterion of test_gpu_x3.test_x3_encoder_matches_fp32_module
        assert rel < (5e-4 if mode == "bf16x3" else 5e-5)
