"""The training convolutions on the split-plane MFMA kernel (avtex.train_ops.conv3d -> csrc/conv_x3.hip, IO32 form):
forward and stride-1 input gradient against torch's fp32 Conv3d through autograd (what the reference's train() runs,
contrastive_video_textures/train.py:114-141), weight gradient through MIOpen either way."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last_3d)


@pytest.mark.parametrize("cin,cout,kernel,stride,pad,dims,gscale", [
    (64, 64, (1, 3, 3), (1, 1, 1), (0, 1, 1), (2, 4, 14, 14), 1.0),
    (8, 32, (3, 1, 1), (1, 1, 1), (1, 0, 0), (2, 8, 9, 7), 1.0),         # narrow fast-pathway layer, ragged rows
    (256, 64, (1, 1, 1), (1, 1, 1), (0, 0, 0), (2, 2, 7, 7), 1.0),
    (64, 256, (1, 1, 1), (1, 1, 1), (0, 0, 0), (2, 2, 7, 7), 1e-6),      # gradients far below fp16's range
    (32, 64, (7, 1, 1), (4, 1, 1), (3, 0, 0), (1, 16, 6, 6), 1.0),       # lateral fusion: temporal stride 4, dgrad = 4 classes
    (64, 128, (1, 3, 3), (1, 2, 2), (0, 1, 1), (2, 2, 14, 14), 1.0),     # strided 3x3: dgrad = 4 classes of 1 / 2 / 2 / 4 taps
    (64, 128, (1, 1, 1), (1, 2, 2), (0, 0, 0), (2, 3, 14, 10), 1.0),     # strided shortcut: one class, the rest zeros
    (8, 16, (1, 3, 3), (1, 2, 2), (0, 1, 1), (1, 4, 28, 28), 1e-6),      # fast-pathway widths, tiny gradients
    (128, 128, (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 4, 8, 8), 1.0),
    (256, 256, (1, 3, 3), (1, 1, 1), (0, 1, 1), (24, 8, 20, 20), 1.0),   # 76 800 positions: the 256 x 256 tile's IO32 form (fwd + dgrad)
    (512, 256, (3, 1, 1), (1, 1, 1), (1, 0, 0), (41, 8, 15, 15), 1e-6),  # ragged last tile (73 800 rows), long K, tiny gradients
    (256, 1024, (1, 1, 1), (1, 1, 1), (0, 0, 0), (24, 8, 20, 20), 1.0),  # pointwise rows, 4 column tiles; dgrad has K = 1024
    (64, 72, (3, 1, 5), (1, 1, 1), (1, 0, 2), (2, 5, 7, 6), 1.0),        # no two kernel extents / pads / input extents alike: plain tile
    (16, 24, (3, 1, 5), (1, 1, 1), (1, 0, 2), (2, 5, 7, 8), 1.0),        # ... the pixel-grouped form (w % 4 == 0)
])
def test_conv_forward_and_gradients_match_fp32_autograd(cin, cout, kernel, stride, pad, dims, gscale):
    from avtex import train_ops
    torch.manual_seed(cin + cout)
    b, t, h, w = dims
    conv = nn.Conv3d(cin, cout, kernel, stride=stride, padding=pad, bias=False).to(DEV).to(memory_format=torch.channels_last_3d).train()
    x0 = _cl(torch.randn(b, cin, t, h, w, device=DEV))
    assert train_ops.conv_fusable(x0, conv)

    def run(fused):
        conv.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        y = train_ops.conv3d(x, conv) if fused else conv(x)
        gy = _cl(torch.randn(y.shape, device=DEV, generator=torch.Generator(DEV).manual_seed(7)) * gscale)
        y.backward(gy)
        return y.detach(), x.grad, conv.weight.grad.clone()

    before = dict(train_ops.CALLS)
    ya, dxa, dwa = run(True)
    assert train_ops.CALLS["miopen_dgrad"] == before["miopen_dgrad"]  # every input gradient on the HIP kernels, strided ones too
    assert train_ops.CALLS["dgrad_x3"] + train_ops.CALLS["dgrad_strided_x3"] == before["dgrad_x3"] + before["dgrad_strided_x3"] + 1
    ye, dxe, dwe = run(False)
    rel = lambda u, v: float((u - v).norm()) / (float(v.norm()) + 1e-30)
    assert ya.shape == ye.shape
    assert rel(ya, ye) < 2e-6, rel(ya, ye)      # fp16 planes: 2^-22 per product against fp32's own rounding
    assert rel(dxa, dxe) < 2e-5, rel(dxa, dxe)  # bf16 planes (fp32's exponent range): 2^-16 per product, averaged over K
    print("conv %s: fwd %.2e dx %.2e dw %.2e" % ((cin, cout, kernel, stride), rel(ya, ye), rel(dxa, dxe), rel(dwa, dwe)))
    assert rel(dwa, dwe) < 1e-4, rel(dwa, dwe)  # csrc/wgrad_x3.hip: bf16 planes rounded half away, 2^-16 per product


def test_weight_planes_follow_the_optimizer():
    from avtex import train_ops
    conv = nn.Conv3d(16, 16, (1, 3, 3), padding=(0, 1, 1), bias=False).to(DEV).to(memory_format=torch.channels_last_3d).train()
    x = _cl(torch.randn(1, 16, 2, 8, 8, device=DEV))
    y0 = train_ops.conv3d(x, conv).detach()
    with torch.no_grad():
        conv.weight.mul_(2.0)  # in-place, as SGD updates
    y1 = train_ops.conv3d(x, conv).detach()
    assert torch.allclose(y1, 2 * y0, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("kw", [dict(foreach=True), dict(fused=True)])
def test_weight_planes_follow_every_optimizer_step(kw):
    """torch's fused optimizer kernels update the parameters WITHOUT moving Tensor._version (round 6, measured: 0 -> 0 over
    SGD(fused=True).step()): a plane cache keyed on versions alone would serve the old weights to every later convolution.  A global
    optimizer-step hook marks the cache stale; the convolution after the step sees the new weights either way."""
    from avtex import train_ops
    torch.manual_seed(4)
    conv = nn.Conv3d(16, 16, (1, 3, 3), padding=(0, 1, 1), bias=False).to(DEV).to(memory_format=torch.channels_last_3d).train()
    x = _cl(torch.randn(1, 16, 2, 8, 8, device=DEV))
    opt = torch.optim.SGD(conv.parameters(), lr=0.5, **kw)
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        train_ops.conv3d(x, conv).square().mean().backward()
        opt.step()
        want = torch.nn.functional.conv3d(x, conv.weight.detach(), padding=(0, 1, 1))
        got = train_ops.conv3d(x, conv).detach()
        assert float((got - want).abs().max()) <= 3e-6 * float(want.abs().max())


def test_falls_back_outside_its_domain():
    from avtex import train_ops
    stem = nn.Conv3d(3, 64, (1, 7, 7), stride=(1, 2, 2), padding=(0, 3, 3), bias=False).to(DEV).to(memory_format=torch.channels_last_3d).train()
    x = _cl(torch.randn(1, 3, 2, 32, 32, device=DEV))
    assert not train_ops.conv_fusable(x.clone().requires_grad_(True), stem)   # 3 channels AND an input gradient wanted
    conv = nn.Conv3d(16, 16, (1, 3, 3), bias=False).to(DEV).train()
    assert not train_ops.conv_fusable(torch.randn(1, 16, 2, 8, 8, device=DEV), conv)   # model not in the training layout
    conv = conv.to(memory_format=torch.channels_last_3d)
    xn = torch.randn(1, 16, 2, 8, 8, device=DEV)                                       # an NCDHW input is transposed once
    assert train_ops.conv_fusable(xn, conv) and torch.allclose(train_ops.conv3d(xn, conv), conv(xn), rtol=1e-5, atol=1e-5)
    conv.eval()
    assert not train_ops.conv_fusable(_cl(torch.randn(1, 16, 2, 8, 8, device=DEV)), conv)
    xg = x.clone().requires_grad_(True)
    assert torch.equal(train_ops.conv3d(xg, stem), stem(xg))


@pytest.mark.parametrize("kt", [1, 5])
def test_stem_runs_on_zero_padded_channels(kt):
    """The stems (3 input channels, models/models.py:565-584's SlowFast): forward on the kernel over a clip padded to 8
    channels; weight gradient on csrc/wgrad_x3.hip too — 4 of those channels per tap, the [kt,7,7] filter as kt slices of 49
    taps — and, with train_ops._STEM_WGRAD_X3 off, through MIOpen on the original clip."""
    from avtex import train_ops
    torch.manual_seed(kt)
    stem = nn.Conv3d(3, 64 if kt == 1 else 8, (kt, 7, 7), stride=(1, 2, 2), padding=(kt // 2, 3, 3), bias=False).to(DEV)
    stem = stem.to(memory_format=torch.channels_last_3d).train()
    x = torch.randn(2, 3, 4, 32, 32, device=DEV)  # NCDHW, as the batcher hands clips over
    assert train_ops.conv_fusable(x, stem)
    y = train_ops.conv3d(x, stem)
    gy = _cl(torch.randn(y.shape, device=DEV))
    y.backward(gy)
    dwa = stem.weight.grad.clone()
    stem.zero_grad(set_to_none=True)
    ye = stem(x)
    ye.backward(gy)
    rel = lambda u, v: float((u - v).norm()) / float(v.norm())
    # forward: fp16 planes (2^-22); weight gradient: bf16 planes (2^-16 per product, random signs: ~1e-5 of the norm)
    assert rel(y.detach(), ye.detach()) < 2e-6 and rel(dwa, stem.weight.grad) < 1e-4, rel(dwa, stem.weight.grad)
    before = train_ops.CALLS["wgrad_stem_x3"]
    keep, train_ops._STEM_WGRAD_X3 = train_ops._STEM_WGRAD_X3, 0
    try:  # the MIOpen route for the stems' weight gradient stays selectable
        want = stem.weight.grad.clone()
        stem.zero_grad(set_to_none=True)
        y2 = train_ops.conv3d(x, stem)
        y2.backward(gy)
        assert rel(stem.weight.grad, want) < 1e-5 and train_ops.CALLS["wgrad_stem_x3"] == before
    finally:
        train_ops._STEM_WGRAD_X3 = keep


@pytest.mark.parametrize("layout", ["ncdhw", "ndhwc", "view"])
@pytest.mark.parametrize("plane", ["f16", "bf16"])
def test_clip_planes_split_the_clip(layout, plane):
    """avt_clip_planes_f32: [B,3,T,H,W] fp32 of any strides -> hi / lo planes [B,T,H,W,4], value = hi + lo, 4th channel 0."""
    from avtex import ops
    torch.manual_seed(3)
    x = torch.randn(2, 3, 3, 10, 12, device=DEV) * 2.0
    if layout == "ndhwc":
        x = x.contiguous(memory_format=torch.channels_last_3d)
    elif layout == "view":  # a strided window of a larger tensor (the batcher's target stack sliced per clip)
        x = torch.randn(2, 3, 5, 12, 16, device=DEV)[:, :, 1:4, 1:11, 2:14]
    dt = ops.X3_F16 if plane == "f16" else ops.X3_BF16
    hi, lo = ops.clip_planes_f32(x, dt)
    raw = torch.float16 if plane == "f16" else torch.bfloat16
    got = hi.view(raw).float() + lo.view(raw).float()
    want = torch.cat([x.permute(0, 2, 3, 4, 1), torch.zeros_like(x[:, :1]).permute(0, 2, 3, 4, 1)], -1)
    tol = 2.0 ** -21 if plane == "f16" else 2.0 ** -15
    assert got.shape == want.shape and float((got - want).abs().max()) <= tol * float(want.abs().max())
    assert float(got[..., 3].abs().max()) == 0.0
    hi_want = want.to(raw)
    assert torch.equal(hi.view(raw), hi_want)  # the high plane is the rounded value itself


@pytest.mark.parametrize("kt,cout,dims", [
    (5, 8, (2, 8, 64, 64)),     # fast stem: 4 output frames per MFMA tile (time-grouped), 32 pixel pairs per row
    (1, 64, (2, 4, 64, 64)),    # slow stem
    (5, 8, (1, 8, 224, 224)),   # production rows: 112 pairs
    (1, 64, (1, 2, 224, 224)),
    (5, 8, (1, 4, 64, 64)),     # 4 frames: every frame tap meets the clip's ends
])
def test_stems_run_on_the_patch_kernels(kt, cout, dims):
    """The stems of the training step on the patch-resident kernels (csrc/stem_conv.hip with fp32 output, csrc/stem_train.hip):
    forward and weight gradient against fp64 autograd, next to what stock fp32 gives."""
    from avtex import train_ops
    torch.manual_seed(kt + dims[1])
    b, t, h, w = dims
    stem = nn.Conv3d(3, cout, (kt, 7, 7), stride=(1, 2, 2), padding=(kt // 2, 3, 3), bias=False).to(DEV)
    stem = stem.to(memory_format=torch.channels_last_3d).train()
    x = torch.randn(b, 3, t, h, w, device=DEV)
    assert train_ops.conv_fusable(x, stem) and train_ops.stem_patch_ok(x, stem)
    before = dict(train_ops.CALLS)
    y = train_ops.conv3d(x, stem)
    assert y.is_contiguous(memory_format=torch.channels_last_3d)
    gy = _cl(torch.randn(y.shape, device=DEV))
    y.backward(gy)
    ran = {k: train_ops.CALLS[k] - before[k] for k in before}
    assert ran["stem_fwd_patch"] == 1 and ran["wgrad_stem_patch"] == 1 and ran["wgrad_stem_x3"] == 0 and ran["miopen_wgrad"] == 0, ran
    dwa = stem.weight.grad.clone()
    stem64 = nn.Conv3d(3, cout, (kt, 7, 7), stride=(1, 2, 2), padding=(kt // 2, 3, 3), bias=False).to(DEV).double()
    stem64.weight.data.copy_(stem.weight.detach().double())
    y64 = stem64(x.double())
    y64.backward(gy.double())
    stem.zero_grad(set_to_none=True)
    y32 = stem(x)
    y32.backward(gy)
    rel = lambda u, v: float((u.double() - v).norm()) / float(v.norm())
    e_y, e_y32 = rel(y.detach(), y64.detach()), rel(y32.detach(), y64.detach())
    e_w, e_w32 = rel(dwa, stem64.weight.grad), rel(stem.weight.grad, stem64.weight.grad)
    print("stem kt=%d cout=%d %s: forward %.2e (stock fp32 %.2e), weight gradient %.2e (stock fp32 %.2e)" % (kt, cout, dims, e_y, e_y32, e_w, e_w32))
    # forward: fp16 planes (2^-22 per product); weight gradient: bf16 planes (2^-16 per product, random signs)
    assert e_y < 2e-6 and e_w < 1e-4, (e_y, e_w)
    assert float((dwa.double() - stem64.weight.grad).abs().max()) < 2e-4 * float(stem64.weight.grad.abs().max())


def test_stem_patch_path_follows_the_optimizer_and_can_be_switched_off():
    from avtex import train_ops
    torch.manual_seed(9)
    stem = nn.Conv3d(3, 8, (5, 7, 7), stride=(1, 2, 2), padding=(2, 3, 3), bias=False).to(DEV).to(memory_format=torch.channels_last_3d).train()
    x = torch.randn(1, 3, 8, 64, 64, device=DEV)
    y0 = train_ops.conv3d(x, stem).detach().clone()
    with torch.no_grad():
        stem.weight.mul_(2.0)  # an in-place update (optimizer.step()): the cached LDS image must be rebuilt
    y1 = train_ops.conv3d(x, stem).detach()
    assert float((y1 - 2.0 * y0).abs().max()) <= 1e-5 * float(y0.abs().max())
    keep, train_ops._STEM_PATCH = train_ops._STEM_PATCH, 0
    try:
        before = train_ops.CALLS["stem_fwd_patch"]
        y2 = train_ops.conv3d(x, stem).detach()
        assert train_ops.CALLS["stem_fwd_patch"] == before
        assert float((y2 - y1).abs().max()) <= 1e-5 * float(y1.abs().max())
    finally:
        train_ops._STEM_PATCH = keep


@pytest.mark.parametrize("cin,cout,kernel,stride,pad,dims", [
    (16, 8, (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 5, 7)),          # fewer positions than one slab
    (24, 40, (3, 3, 3), (1, 2, 2), (1, 1, 1), (2, 3, 9, 11)),         # ragged everything, channel counts not powers of two
    (136, 264, (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 2, 9, 9)),        # more than one tile on both sides, swapped operands
    (264, 136, (1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 2, 9, 9)),
    # the 256 x 128 pipelined tile (>= 256 x 128 on the two axes, >= 2048 positions): both orientations, ragged tiles on both axes,
    # a position count that is not a multiple of the 32-position step, strides, several chunks of steps
    (64, 136, (1, 3, 3), (1, 1, 1), (0, 1, 1), (2, 3, 21, 19)),       # E = 576 (3 R tiles, the last ragged), cout 136 (2 S tiles), 2394 positions
    (264, 520, (1, 1, 1), (1, 1, 1), (0, 0, 0), (3, 2, 20, 20)),      # swapped: cout 520 on the long axis, E = 264
    (128, 128, (3, 1, 1), (1, 1, 1), (1, 0, 0), (2, 8, 14, 14)),      # temporal taps, exact tiles
    (136, 256, (1, 3, 3), (1, 2, 2), (0, 1, 1), (2, 2, 57, 59)),      # strided, odd extents
    (256, 256, (1, 1, 1), (1, 1, 1), (0, 0, 0), (8, 8, 28, 28)),      # 50 176 positions: many chunks of steps, atomics from all of them
    # the pipelined tile's 64- and 32-wide forms (the narrow layers: one ragged R tile, S tiles of 64 / 32, both orientations)
    (64, 64, (1, 3, 3), (1, 1, 1), (0, 1, 1), (2, 3, 21, 19)),        # E = 576, cout 64: one 64-wide S tile
    (8, 8, (1, 3, 3), (1, 1, 1), (0, 1, 1), (2, 4, 24, 23)),          # E = 72 of a 256-wide R tile, cout 8 of a 32-wide S tile
    (32, 8, (3, 1, 1), (1, 1, 1), (1, 0, 0), (2, 6, 20, 20)),         # E = 96, cout 8
    (8, 32, (1, 1, 1), (1, 1, 1), (0, 0, 0), (2, 5, 22, 22)),         # swapped: cout 32 on the R axis, E = 8 on a 32-wide S tile
    (64, 256, (1, 1, 1), (1, 1, 1), (0, 0, 0), (2, 2, 29, 30)),       # swapped: cout 256, E = 64 (64-wide S tile), ragged positions
    (40, 72, (1, 3, 3), (1, 2, 2), (0, 1, 1), (2, 2, 41, 43)),        # E = 360 (2 R tiles), cout 72 -> 128-wide S, strided
    (16, 48, (3, 1, 1), (1, 1, 1), (1, 0, 0), (3, 5, 15, 16)),        # E = 48, cout 48: equal axes, 64-wide S tile
])
@pytest.mark.parametrize("mode", ["pipelined", "serial", "serial-plain-loads"])
def test_weight_gradient_kernel_edges(cin, cout, kernel, stride, pad, dims, mode):
    """mode: every layer on the pipelined tile at the S width that fits / on the phase-serial 128-wide tile with buffer loads / the
    same with plain loads and mask registers (what tensors of 4 GB and more get) — the default picks among them by measurement."""
    from avtex import _lib, ops
    torch.manual_seed(cin)
    _lib.lib().avt_wgrad_x3_set_xl(2 if mode == "pipelined" else 0)
    _lib.lib().avt_wgrad_x3_set_xl(5 if mode == "serial-plain-loads" else 6)
    b, t, h, w = dims
    x = torch.randn(b, cin, t, h, w, device=DEV)
    wgt = torch.randn(cout, cin, *kernel, device=DEV, requires_grad=True)
    y = torch.nn.functional.conv3d(x, wgt, stride=stride, padding=pad)
    gy = torch.randn_like(y)
    y.backward(gy)
    dw = torch.empty((cout,) + tuple(kernel) + (cin,), device=DEV)
    ops.conv3d_wgrad_x3_f32(gy.permute(0, 2, 3, 4, 1).contiguous(), x.permute(0, 2, 3, 4, 1).contiguous(), dw, (b, t, h, w), cin, cout,
                            kernel, stride, pad, cin, cout)
    _lib.lib().avt_wgrad_x3_set_xl(1)
    _lib.lib().avt_wgrad_x3_set_xl(6)
    exp = wgt.grad.permute(0, 2, 3, 4, 1)
    err = float((dw - exp).norm()) / float(exp.norm())
    assert err < 1e-4, err


def test_weight_plane_cache_is_per_tensor_not_per_address():
    """Two models built one after the other can get the same addresses (and ids) for their weights: the cache must not hand
    the second one the first one's planes."""
    import gc

    from avtex import train_ops
    x = _cl(torch.randn(1, 16, 2, 8, 8, device=DEV))
    outs = []
    for seed in (1, 2):
        torch.manual_seed(seed)
        conv = nn.Conv3d(16, 16, (1, 3, 3), padding=(0, 1, 1), bias=False).to(DEV).to(memory_format=torch.channels_last_3d).train()
        y = train_ops.conv3d(x, conv).detach()
        assert torch.allclose(y, conv(x), rtol=1e-5, atol=1e-5)
        outs.append(y)
        del conv
        gc.collect()
    assert not torch.allclose(outs[0], outs[1])


@pytest.mark.parametrize("stride,cin,cout,kernel,pad,dims", [
    ((1, 1, 1), 32, 64, (1, 3, 3), (0, 1, 1), (2, 3, 10, 10)),
    ((1, 2, 2), 32, 64, (1, 3, 3), (0, 1, 1), (2, 3, 10, 10)),
    ((1, 1, 1), 256, 64, (3, 1, 1), (1, 0, 0), (24, 8, 20, 20)),   # 76 800 positions, dgrad 64 -> 256 over K = 192: the 128-wide tile
    ((1, 1, 1), 256, 256, (3, 1, 1), (1, 0, 0), (24, 8, 20, 20)),  # dgrad 256 -> 256 over K = 768: the 256 x 256 tile's IO32 form + add
])
def test_fork_sums_the_other_path_in_the_kernel(stride, cin, cout, kernel, pad, dims):
    """conv3d_fork: the gradient that reaches x through the alias is added in the epilogue of the convolution's own
    input-gradient kernel (stride 1, both tiles) or after the strided classes — either way dx = dgrad(dy) + d_alias."""
    from avtex import train_ops
    torch.manual_seed(5)
    conv = nn.Conv3d(cin, cout, kernel, stride=stride, padding=pad, bias=False).to(DEV).to(memory_format=torch.channels_last_3d).train()
    x0 = _cl(torch.randn(dims[0], cin, *dims[1:], device=DEV))
    x = x0.clone().requires_grad_(True)
    y, xs = train_ops.conv3d_fork(x, conv)
    gy, gx = _cl(torch.randn_like(y)), _cl(torch.randn_like(x0))
    ((y * gy).sum() + (xs * gx).sum()).backward()
    dwa = conv.weight.grad.clone()
    conv.zero_grad(set_to_none=True)
    xr = x0.clone().requires_grad_(True)
    yr = conv(xr)
    ((yr * gy).sum() + (xr * gx).sum()).backward()
    rel = lambda u, v: float((u - v).norm()) / float(v.norm())
    assert rel(y.detach(), yr.detach()) < 2e-6 and torch.equal(xs.detach(), x0)
    assert rel(x.grad, xr.grad) < 2e-5 and rel(dwa, conv.weight.grad) < 1e-4


def test_training_convolution_at_full_size_scales():
    """Config 5's largest pointwise layer at its real size (15 target clips, slow res2: 376 320 positions, 64 -> 256) under
    a power-of-two scaling of its input.  The input GRADIENT runs on bf16 planes, which keep fp32's exponent: every plane,
    product and partial sum scales exactly, so dx must scale BIT FOR BIT.  The forward runs on fp16 planes, whose low plane
    is subnormal for |x| < 2^-3 (absolute, not relative, precision there: csrc/split_planes.h) — a first version of this test
    claimed bit-exactness for it too and failed — so it is held to the planes' own accuracy; the weight gradient (atomics:
    summation order varies) to rounding."""
    from avtex import train_ops
    torch.manual_seed(0)
    conv = nn.Conv3d(64, 256, 1, bias=False).to(DEV).to(memory_format=torch.channels_last_3d).train()
    x0 = _cl(torch.randn(15, 64, 8, 56, 56, device=DEV))

    def run(scale):
        conv.zero_grad(set_to_none=True)
        x = (x0 * scale).requires_grad_(True)
        y = train_ops.conv3d(x, conv)
        gy = _cl(torch.ones_like(y) * scale)
        y.backward(gy)
        return y.detach(), x.grad, conv.weight.grad.clone()

    y1, dx1, dw1 = run(1.0)
    y4, dx4, dw4 = run(4.0)
    assert torch.equal(dx4, 4 * dx1)
    assert float((y4 - 4 * y1).norm()) <= 1e-6 * float((4 * y1).norm())
    assert float((dw4 - 16 * dw1).norm()) <= 1e-5 * float((16 * dw1).norm())


@pytest.mark.parametrize("passes,single_arena", [(1, False), (3, False), (1, True)])
def test_micro_batch_gradients_equal_autograd_accumulation(passes, single_arena):
    """train_ops.MicroBatchGradients (one multi-tensor add per pass, weight gradients written into slices of one zeroed
    arena) gives the sums autograd's own .grad accumulation gives, step after step (the arena is re-zeroed, not re-used dirty).
    single_arena (round 6): a ONE-pass step takes arena slices too — one memset per step — and an SGD step (torch's fused kernel, as
    bench.py runs it) reads those slices as gradients."""
    from avtex import train_ops

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.c1 = nn.Conv3d(8, 16, (1, 3, 3), padding=(0, 1, 1), bias=False)
            self.b1 = nn.BatchNorm3d(16)
            self.c2 = nn.Conv3d(16, 8, (3, 1, 1), padding=(1, 0, 0), bias=False)
            self.unused = nn.Linear(4, 4)

        def forward(self, x):
            return train_ops.conv3d(train_ops.bn_act(train_ops.conv3d(x, self.c1), self.b1), self.c2)

    torch.manual_seed(passes)
    net = Net().to(DEV).to(memory_format=torch.channels_last_3d).train()
    xs = [_cl(torch.randn(2, 8, 4, 12, 12, device=DEV)) for _ in range(passes)]

    def run(accumulate):
        out = []
        acc = train_ops.MicroBatchGradients(net.parameters(), single_pass_arena=single_arena) if accumulate else None
        for step in range(3):  # the second and third steps meet a used arena / used accumulators
            if acc is not None:
                acc.begin(passes)
            else:
                net.zero_grad(set_to_none=True)
            for k, x in enumerate(xs):
                last = k == passes - 1
                if acc is not None and last:
                    acc.before_last_backward()
                (net(x * (1.0 + step)).square().mean()).backward()
                if acc is not None and not last:
                    acc.after_backward()
            if acc is not None:
                acc.finish()
            torch.cuda.synchronize()
            out.append({k: p.grad.detach().clone() for k, p in net.named_parameters() if p.grad is not None})
        return out

    before = train_ops.CALLS["wgrad_x3"]
    want, got = run(False), run(True)
    assert train_ops.CALLS["wgrad_x3"] - before == 2 * 3 * passes * 2
    assert train_ops._ARENA is None  # switched off again after finish()
    for w, g in zip(want, got):
        assert set(w) == set(g) and "unused.weight" not in g
        for k in w:
            assert float((w[k] - g[k]).abs().max()) <= 2e-5 * float(w[k].abs().max()) + 1e-12, k
    if single_arena:  # the arena's slices as the optimizer's gradients: a fused SGD step equals the multi-tensor one on owned gradients
        import copy

        def sgd(fused, arena):
            m = copy.deepcopy(net)
            opt = torch.optim.SGD(m.parameters(), lr=0.1, momentum=0.9, weight_decay=1e-2, fused=fused)
            acc = train_ops.MicroBatchGradients(m.parameters(), single_pass_arena=arena)
            for step in range(3):
                acc.begin(1)
                (m(xs[0] * (1.0 + step)).square().mean()).backward()
                acc.finish()
                if arena and step:  # (from the second step on the weight gradients are slices of the arena)
                    buf = acc.arena.buf[m.c1.weight.device]
                    assert buf.data_ptr() <= m.c1.weight.grad.data_ptr() < buf.data_ptr() + 4 * buf.numel()
                opt.step()
            torch.cuda.synchronize()
            return [p.detach().clone() for p in m.parameters()]

        for a, b in zip(sgd(True, True), sgd(False, False)):
            assert float((a - b).abs().max()) <= 2e-5 * float(b.abs().max()) + 1e-12


@pytest.mark.parametrize("dims,c", [((2, 3, 12, 12), 8), ((1, 2, 11, 9), 64), ((2, 1, 112, 112), 16)])
def test_stem_max_pool_forward_and_gradient_equal_torch(dims, c):
    """train_ops.max_pool_hw (csrc/stem_train.hip) against nn.MaxPool3d((1,3,3),(1,2,2),(0,1,1)) through autograd: values bit for
    bit, the gradient routed to the same (first) maximum — with ties in the input (a ReLU output has many zeros)."""
    from avtex import train_ops
    torch.manual_seed(dims[2])
    b, t, h, w = dims
    x0 = torch.relu(torch.randn(b, c, t, h, w, device=DEV)).contiguous(memory_format=torch.channels_last_3d)  # zeros: ties
    pool = nn.MaxPool3d((1, 3, 3), stride=(1, 2, 2), padding=(0, 1, 1))
    xa, xb = x0.clone().requires_grad_(True), x0.clone().requires_grad_(True)
    before = train_ops.CALLS["maxpool_hip"]
    ya = train_ops.max_pool_hw(xa, pool)
    assert train_ops.CALLS["maxpool_hip"] == before + 1
    yb = pool(xb)
    gy = _cl(torch.randn_like(yb))
    ya.backward(gy)
    yb.backward(gy)
    assert torch.equal(ya, yb) and ya.is_contiguous(memory_format=torch.channels_last_3d)
    # (an input position can be the maximum of up to four windows: torch adds them with atomics in any order, the gather here
    #  in a fixed one — equal up to fp32 rounding of that sum; a different tie rule would move whole gradients instead)
    assert float((xa.grad - xb.grad).abs().max()) <= 4e-7 * float(xb.grad.abs().max())
    assert train_ops.max_pool_hw(x0, pool).shape == yb.shape and train_ops.CALLS["maxpool_hip"] == before + 1  # no gradient: the module


@pytest.mark.parametrize("dims,c,extra", [((2, 3, 12, 12), 8, 4), ((1, 2, 11, 9), 64, 16)])
def test_stem_max_pool_writes_the_first_slice_of_a_concatenation(dims, c, extra):
    """max_pool_hw(cat_extra): the pooled rows as the first c channels of c + extra wide rows (the slow stem's pool feeds the first
    lateral fusion, train_ops.join_channels), and its backward reading a slice of the concatenation's gradient: bit-equal to the
    pool's own tensor + torch.cat + a contiguous gradient."""
    from avtex import train_ops
    torch.manual_seed(dims[3])
    b, t, h, w = dims
    x0 = torch.relu(torch.randn(b, c, t, h, w, device=DEV)).contiguous(memory_format=torch.channels_last_3d)
    pool = nn.MaxPool3d((1, 3, 3), stride=(1, 2, 2), padding=(0, 1, 1))
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    lat0 = _cl(torch.randn(b, extra, t, ho, wo, device=DEV))
    gy = _cl(torch.randn(b, c + extra, t, ho, wo, device=DEV))

    def run(join):
        x, lat = x0.clone().requires_grad_(True), lat0.clone().requires_grad_(True)
        if join:
            y = train_ops.max_pool_hw(x, pool, cat_extra=extra)
            buf, off = y._avt_cat
            assert off == 0 and buf.shape[1] == c + extra and y.data_ptr() == buf.data_ptr()

            class Fill(torch.autograd.Function):  # stands for the lateral BatchNorm: writes the other slice of the buffer
                @staticmethod
                def forward(ctx, v):
                    o = train_ops._alias(buf, c, extra)
                    o.copy_(v)
                    return o

                @staticmethod
                def backward(ctx, d):
                    return d.contiguous(memory_format=torch.channels_last_3d)

            yl = Fill.apply(lat)
            yl._avt_cat = (buf, c)
            z = train_ops.join_channels(y, yl)
            assert z.data_ptr() == buf.data_ptr()
        else:
            z = torch.cat([train_ops.max_pool_hw(x, pool), lat], 1)
        (z * 1.5).backward(gy)
        return z.detach().clone(), x.grad, lat.grad

    for u, v in zip(run(True), run(False)):
        assert torch.equal(u, v)


def test_vggish_training_convolutions_run_on_the_hand_written_kernels(avt, dev):
    """The m = 2 training branch's audio encoder (reference models/models.py:343-345, 405-407; VERDICT r3 'missing' #6): VGGish's six
    Conv2d forward / input gradient / weight gradient through train_ops.conv2d (the image as a one-frame clip) against the stock
    fp32 autograd of the same module — no MIOpen convolution is launched; the 1-channel first layer runs on its zero-padded copy."""
    import copy

    from avtex import train_ops

    torch.manual_seed(0)
    ref = avt.VGGish().to(dev).train()
    net = copy.deepcopy(ref)
    x = torch.randn(6, 1, 100, 64, device=dev)
    gy = torch.randn(6, 12288, device=dev)
    keep, train_ops._CONV_X3 = train_ops._CONV_X3, 0
    y0 = ref(x)
    y0.backward(gy)
    train_ops._CONV_X3 = keep
    before = dict(train_ops.CALLS)
    y1 = net(x)
    y1.backward(gy)
    torch.cuda.synchronize()
    d = {k: train_ops.CALLS[k] - before.get(k, 0) for k in train_ops.CALLS}
    assert d["conv_fwd_x3"] == 6 and d["wgrad_x3"] == 6 and d["dgrad_x3"] == 5, d
    assert d.get("miopen_wgrad", 0) == 0 and d.get("miopen_dgrad", 0) == 0, d
    assert float((y1 - y0).detach().abs().max()) < 2e-5 * float(y0.detach().abs().max())
    for (k, p0), (_, p1) in zip(ref.named_parameters(), net.named_parameters()):
        if p0.grad is None:
            assert p1.grad is None  # the fc stack is never applied
            continue
        rel = float((p1.grad - p0.grad).norm() / p0.grad.norm())
        assert rel < 2e-4, (k, rel)


@pytest.mark.parametrize("cin,cout,dims,with_fork", [
    (64, 256, (2, 3, 9, 7), False),     # res2 c
    (128, 512, (1, 2, 5, 6), True),     # res3 c, + the fork's add operand in the input gradient of the next test row
    (256, 64, (2, 2, 4, 5), True),      # a reducing layer: its INPUT gradient (64 -> 256 rows) takes the streaming form
    (8, 32, (2, 4, 6, 10), False),      # fast pathway: K = 8 (one partial k-step), two 16-channel tiles
    (32, 128, (1, 3, 7, 4), False),
    (256, 1024, (1, 1, 3, 5), False),   # eight channel chunks
])
def test_pointwise_layers_take_the_streaming_f32_kernel(cin, cout, dims, with_fork):
    """train_ops.conv3d on a 1x1x1 convolution: forward and input gradient on csrc/pw_x3.hip's fp32-in / fp32-out form
    (avt_pw_x3_f32: plain weight planes laid out as fragments by the kernel's prologue) against fp32 autograd on the same tensors,
    ragged row counts included; conv3d_fork's second gradient path is summed in the kernel's epilogue."""
    from avtex import train_ops
    torch.manual_seed(cin + cout)
    b, t, h, w = dims
    conv = nn.Conv3d(cin, cout, 1, bias=False).to(DEV).to(memory_format=torch.channels_last_3d).train()
    x0 = _cl(torch.randn(b, cin, t, h, w, device=DEV))
    gy = _cl(torch.randn(b, cout, t, h, w, device=DEV))
    gx2 = _cl(torch.randn(b, cin, t, h, w, device=DEV)) if with_fork else None

    def run(fused):
        conv.weight.grad = None
        x = x0.clone().requires_grad_(True)
        before = train_ops.CALLS["pw_f32"]
        if fused:
            if with_fork:
                y, xs = train_ops.conv3d_fork(x, conv)
                loss = (y * gy).sum() + (xs * gx2).sum()
            else:
                y = train_ops.conv3d(x, conv)
                loss = (y * gy).sum()
        else:
            y = torch.nn.functional.conv3d(x, conv.weight)
            loss = (y * gy).sum() + ((x * gx2).sum() if with_fork else 0.0)
        loss.backward()
        return y.detach(), x.grad.detach(), conv.weight.grad.detach().clone(), train_ops.CALLS["pw_f32"] - before

    ya, gxa, gwa, calls = run(True)
    ye, gxe, gwe, _ = run(False)
    fwd_pw = train_ops._lib.lib().avt_pw_x3_f32_supported(cin, cout)
    bwd_pw = train_ops._lib.lib().avt_pw_x3_f32_supported(cout, cin)
    assert calls == int(bool(fwd_pw)) + int(bool(bwd_pw)) and calls >= 1
    for got, want, tol in ((ya, ye, 3e-6), (gxa, gxe, 2e-4), (gwa, gwe, 2e-4)):
        assert float((got - want).abs().max()) <= tol * float(want.abs().max()) + 1e-12


@pytest.mark.parametrize("cin,cout,kernel,stride,pad,dims,groups", [
    (64, 64, (1, 3, 3), (1, 1, 1), (0, 1, 1), (4, 2, 14, 14), 2),       # <128,64,64> tile; 784 rows per group = 6.1 tiles: short last tile
    (64, 64, (1, 3, 3), (1, 2, 2), (0, 1, 1), (4, 2, 14, 14), 4),       # strided forward, 98 rows per group < one tile
    (32, 128, (3, 1, 1), (1, 1, 1), (1, 0, 0), (6, 4, 10, 10), 3),      # <128,128,64> tile
    (8, 8, (1, 3, 3), (1, 1, 1), (0, 1, 1), (4, 4, 12, 16), 2),         # pixel-grouped form: 4 columns fold into one channel
    (16, 32, (3, 1, 1), (1, 1, 1), (1, 0, 0), (2, 8, 8, 8), 1),         # grouped temporal layer, one group
    (256, 256, (1, 3, 3), (1, 1, 1), (0, 1, 1), (4, 4, 64, 64), 2),     # the 256 x 256 tile (K = 2304, 65 536 rows)
    (512, 256, (3, 1, 1), (1, 1, 1), (1, 0, 0), (6, 8, 38, 38), 3),     # ... with 23 104 rows per group: a short tile per group
    (320, 64, (1, 1, 1), (1, 1, 1), (0, 0, 0), (4, 2, 14, 14), 2),      # a pointwise layer the streaming kernel does not take (K = 320)
    (64, 256, (1, 1, 1), (1, 1, 1), (0, 0, 0), (4, 2, 14, 14), 2),      # the streaming pointwise kernel <2, 16>: 4 passes of 64 channels
    (128, 512, (1, 1, 1), (1, 1, 1), (0, 0, 0), (6, 1, 7, 7), 3),       # <4, 16>: two channel chunks, 32-wide passes, 49 rows per group
    (8, 32, (1, 1, 1), (1, 1, 1), (0, 0, 0), (4, 4, 12, 12), 4),        # <1, 2>: one 32-wide pass
    (32, 64, (1, 1, 1), (1, 1, 1), (0, 0, 0), (2, 4, 12, 12), 1),       # <1, 4>
    (512, 2048, (1, 1, 1), (1, 1, 1), (0, 0, 0), (4, 1, 7, 7), 2),      # 2048 channels: two rows of partials per wave slot
    (64, 64, (1, 3, 3), (1, 1, 1), (0, 1, 1), (2, 8, 56, 56), 2),       # 196 tiles per group: the partial rows are pre-reduced by 64
    (64, 256, (1, 1, 1), (1, 1, 1), (0, 0, 0), (2, 8, 56, 56), 2),      # ... streaming kernel: a row per wave, 1568 tiles per group
    (256, 2048, (1, 1, 1), (1, 1, 1), (0, 0, 0), (4, 8, 28, 28), 1),    # ... 2048 channels (two row phases) through the pre-reduction
])
def test_batchnorm_statistics_on_the_convolution_epilogue(cin, cout, kernel, stride, pad, dims, groups):
    """conv3d(x, conv, stats=bn) leaves the BatchNorm's batch statistics behind (per-tile partial sums from the
    epilogue, tiles laid per replica group) and bn_act(…) runs without its statistics pass: same convolution output bit for bit,
    BatchNorm output / running statistics / every gradient equal to the two-pass path to fp32 rounding of the sums."""
    import torch.nn as nn

    from avtex import train_ops

    dev = "cuda:0"
    torch.manual_seed(cin + cout)
    b, t, h, w = dims
    x0 = (torch.randn(b, cin, t, h, w, device=dev) * 1.5 + 0.4).contiguous(memory_format=torch.channels_last_3d)

    def run(epi):
        torch.manual_seed(7)
        conv = nn.Conv3d(cin, cout, kernel, stride=stride, padding=pad, bias=False).to(dev).to(memory_format=torch.channels_last_3d).train()
        bn = nn.BatchNorm3d(cout).to(dev).train()
        with torch.no_grad():
            bn.weight.copy_(torch.linspace(0.5, 1.5, cout))
            bn.bias.copy_(torch.linspace(-0.3, 0.3, cout))
        x = x0.clone().requires_grad_(True)
        keep, train_ops._EPI_STATS = train_ops._EPI_STATS, epi
        for k in train_ops.CALLS:
            train_ops.CALLS[k] = 0
        try:
            with train_ops.bn_replicas(groups):
                y0 = train_ops.conv3d(x, conv, stats=bn)
                tagged = hasattr(y0, "_avt_stats")
                y = train_ops.bn_act(y0, bn, relu=True)
            y.square().sum().backward()
        finally:
            train_ops._EPI_STATS = keep
        return (y0.detach(), y.detach(), x.grad, conv.weight.grad, bn.weight.grad, bn.bias.grad, bn.running_mean.clone(),
                bn.running_var.clone(), tagged, dict(train_ops.CALLS))

    a, e = run(1), run(0)
    assert a[8] and not e[8] and a[9]["bn_fwd_pre"] == 1 and e[9]["bn_fwd_pre"] == 0
    streaming = kernel == (1, 1, 1) and bool(__import__("avtex.ops", fromlist=["x"]).pw_x3_f32_supported(cin, cout))
    assert a[9]["pw_f32"] == e[9]["pw_f32"] and (not streaming or a[9]["pw_f32"] >= 1)  # (the same kernels either way)
    assert torch.equal(a[0], e[0])  # the convolution itself is untouched by the per-group tile layout
    for k, name in ((1, "y"), (2, "dx"), (3, "dw"), (4, "dgamma"), (5, "dbeta"), (6, "running_mean"), (7, "running_var")):
        err = float((a[k] - e[k]).norm() / e[k].norm().clamp_min(1e-20))
        assert err < 3e-6, (name, err)
    assert float((a[1] - e[1]).abs().max()) < 2e-5 * float(e[1].abs().max())


@pytest.mark.parametrize("c,cout,kernel,pad,dims,groups,res", [
    (64, 64, (1, 3, 3), (0, 1, 1), (4, 2, 14, 14), 2, False),     # a_bn -> b: mask recomputed from x; <128,64,64> tile, short tiles
    (128, 32, (3, 1, 1), (1, 0, 0), (6, 4, 10, 10), 3, True),     # c_bn (+ shortcut: saved mask bits) -> the next block's a; <128,128,64>
    (8, 8, (1, 3, 3), (0, 1, 1), (4, 4, 12, 16), 2, False),       # pixel-grouped input gradient: columns fold into channels
    (32, 16, (3, 1, 1), (1, 0, 0), (2, 8, 8, 8), 1, True),        # grouped temporal layer, one group, mask bits
    (512, 128, (1, 1, 1), (0, 0, 0), (4, 2, 14, 14), 2, False),   # b_bn -> c with K = 512: a pointwise layer on the general tile
    (64, 64, (1, 3, 3), (0, 1, 1), (2, 8, 56, 56), 2, True),      # 196 tiles per group: pre-reduced partial rows
    (256, 64, (1, 1, 1), (0, 0, 0), (4, 2, 14, 14), 2, True),     # the streaming pointwise kernel <2, 16> in two halves, mask bits, + shortcut add
    (512, 128, (1, 1, 1), (0, 0, 0), (6, 1, 7, 7), 3, True),      # <4, 16>: two channel chunks, 32-wide passes, 49 rows per group
    (64, 256, (1, 1, 1), (0, 0, 0), (4, 2, 14, 14), 2, False),    # b_bn -> c (K = 256 -> N = 64: <8, 4>), mask recomputed
    (32, 8, (1, 1, 1), (0, 0, 0), (4, 4, 12, 12), 4, True),       # <1, 2>
    (256, 64, (1, 1, 1), (0, 0, 0), (2, 8, 56, 56), 2, True),     # 1568 tiles per group, a row of partials per wave
])
def test_batchnorm_backward_statistics_on_the_input_gradient_epilogue(c, cout, kernel, pad, dims, groups, res):
    """y = bn_act(x, bn[, res]) -> conv(y).  The convolution's stride-1 input-gradient launch masks its result with
    the BatchNorm's ReLU mask and sums the BatchNorm's backward statistics in its epilogue; the BatchNorm's backward then runs
    finalize + apply only (CALLS['bn_bwd_pre']) and hands the masked gradient itself to the shortcut.  Everything equal to the
    three-pass path to rounding: dx, d(shortcut), dgamma, dbeta, and the convolution's own dW."""
    import torch.nn as nn

    from avtex import train_ops

    dev = "cuda:0"
    torch.manual_seed(c + cout)
    b, t, h, w = dims
    x0 = (torch.randn(b, c, t, h, w, device=dev) * 1.5 + 0.4).contiguous(memory_format=torch.channels_last_3d)
    r0 = torch.randn(b, c, t, h, w, device=dev).contiguous(memory_format=torch.channels_last_3d) if res else None
    gy = torch.randn(b, cout, t, h, w, device=dev).contiguous(memory_format=torch.channels_last_3d)
    ga = torch.randn(b, c, t, h, w, device=dev).contiguous(memory_format=torch.channels_last_3d)

    def run(epi):
        torch.manual_seed(7)
        conv = nn.Conv3d(c, cout, kernel, padding=pad, bias=False).to(dev).to(memory_format=torch.channels_last_3d).train()
        bn = nn.BatchNorm3d(c).to(dev).train()
        with torch.no_grad():
            bn.weight.copy_(torch.linspace(0.5, 1.5, c))
            bn.bias.copy_(torch.linspace(-0.3, 0.3, c))
        x = x0.clone().requires_grad_(True)
        r = r0.clone().requires_grad_(True) if res else None
        keep, train_ops._EPI_BWD = train_ops._EPI_BWD, epi
        for k in train_ops.CALLS:
            train_ops.CALLS[k] = 0
        try:
            with train_ops.bn_replicas(groups):
                y = train_ops.bn_act(x, bn, res=r, relu=True)
                if res:  # the block shape: the consumer is a fork whose alias (the next shortcut) carries a gradient of its own,
                    z, alias = train_ops.conv3d_fork(y, conv)  # summed into the input gradient inside the launch (`add`)
                    loss = (z * gy).sum() + (alias * ga).sum()
                else:
                    loss = (train_ops.conv3d(y, conv) * gy).sum()
            loss.backward()
        finally:
            train_ops._EPI_BWD = keep
        return (x.grad, None if r is None else r.grad, bn.weight.grad, bn.bias.grad, conv.weight.grad, dict(train_ops.CALLS))

    a, e = run(1), run(0)
    assert a[5]["bn_bwd_pre"] == 1 and a[5]["dgrad_bwdstats"] == 1 and e[5]["bn_bwd_pre"] == 0 and e[5]["dgrad_bwdstats"] == 0
    for k, name in ((0, "dx"), (1, "dres"), (2, "dgamma"), (3, "dbeta"), (4, "dw")):
        if a[k] is None:
            assert e[k] is None
            continue
        err = float((a[k] - e[k]).norm() / e[k].norm().clamp_min(1e-20))
        assert err < 5e-6, (name, err)
    if res:  # the shortcut's gradient is the masked gradient itself: bit for bit the three-pass path's
        assert torch.equal(a[1], e[1])


def test_summed_gradients_do_not_take_the_fused_backward_statistics():
    """The BatchNorm output feeds TWO convolutions: autograd sums their input gradients (possibly in place into the first, masked
    one) — the sum must go through the plain backward passes, and come out right."""
    import torch.nn as nn

    from avtex import train_ops

    dev = "cuda:0"
    torch.manual_seed(3)
    x0 = (torch.randn(4, 64, 2, 14, 14, device=dev) + 0.3).contiguous(memory_format=torch.channels_last_3d)

    def run(epi):
        torch.manual_seed(7)
        c1 = nn.Conv3d(64, 64, (1, 3, 3), padding=(0, 1, 1), bias=False).to(dev).to(memory_format=torch.channels_last_3d).train()
        c2 = nn.Conv3d(64, 32, (3, 1, 1), padding=(1, 0, 0), bias=False).to(dev).to(memory_format=torch.channels_last_3d).train()
        bn = nn.BatchNorm3d(64).to(dev).train()
        x = x0.clone().requires_grad_(True)
        keep, train_ops._EPI_BWD = train_ops._EPI_BWD, epi
        for k in train_ops.CALLS:
            train_ops.CALLS[k] = 0
        try:
            with train_ops.bn_replicas(2):
                y = train_ops.bn_act(x, bn, relu=True)
                loss = train_ops.conv3d(y, c1).square().sum() + train_ops.conv3d(y, c2).square().sum()
            loss.backward()
        finally:
            train_ops._EPI_BWD = keep
        return x.grad, bn.weight.grad, dict(train_ops.CALLS)

    a, e = run(1), run(0)
    assert a[2]["bn_bwd_pre"] == 0 and a[2]["dgrad_bwdstats"] == 2  # both launches masked their part; the sum took the plain passes
    assert float((a[0] - e[0]).norm() / e[0].norm()) < 5e-6 and float((a[1] - e[1]).norm() / e[1].norm()) < 5e-6


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
def test_pixel_grouped_statistics_wider_than_a_tile_keep_the_statistics_pass(direction):
    """the pixel-grouped form folds a channel's pixel copies inside ONE N tile (csrc/conv_args.h stat_fold_store).  With
    g * C > 128 columns (Conv3d(16, 64, [1,3,3]): g = 4 -> 256 columns; the input gradient of a 64 -> 16 layer likewise) two N tiles
    would overwrite each other's partial sums, so these layers must keep the BatchNorm's own statistics pass — and give the numbers
    of the two-pass path."""
    import torch.nn as nn

    from avtex import train_ops

    dev = "cuda:0"
    torch.manual_seed(11)
    cin, cout = (16, 64) if direction == "fwd" else (64, 16)
    b, t, h, w = 4, 2, 12, 16
    x0 = (torch.randn(b, cin, t, h, w, device=dev) * 1.5 + 0.4).contiguous(memory_format=torch.channels_last_3d)

    def run(epi):
        torch.manual_seed(7)
        conv = nn.Conv3d(cin, cout, (1, 3, 3), padding=(0, 1, 1), bias=False).to(dev).to(memory_format=torch.channels_last_3d).train()
        bn = nn.BatchNorm3d(cout if direction == "fwd" else cin).to(dev).train()
        x = x0.clone().requires_grad_(True)
        keep = (train_ops._EPI_STATS, train_ops._EPI_BWD)
        train_ops._EPI_STATS = train_ops._EPI_BWD = epi
        for k in train_ops.CALLS:
            train_ops.CALLS[k] = 0
        try:
            with train_ops.bn_replicas(2):
                if direction == "fwd":
                    y = train_ops.bn_act(train_ops.conv3d(x, conv, stats=bn), bn, relu=True)
                else:
                    y = train_ops.conv3d(train_ops.bn_act(x, bn, relu=True), conv)
            y.square().sum().backward()
        finally:
            train_ops._EPI_STATS, train_ops._EPI_BWD = keep
        return y.detach(), x.grad, conv.weight.grad, bn.weight.grad, bn.bias.grad, dict(train_ops.CALLS)

    a, e = run(1), run(0)
    assert a[5]["bn_fwd_pre"] == 0 and a[5]["bn_bwd_pre"] == 0 and a[5]["dgrad_bwdstats"] == 0, a[5]  # the fused forms were NOT taken
    for k in range(5):
        assert torch.equal(a[k], e[k]), k
    # ... and the statistics are right: against torch's own BatchNorm on the same convolution output
    torch.manual_seed(7)
    conv = nn.Conv3d(cin, cout, (1, 3, 3), padding=(0, 1, 1), bias=False).to(dev).train()
    bn = nn.BatchNorm3d(cout if direction == "fwd" else cin).to(dev).train()
    xs = x0.contiguous().chunk(2, 0)
    ref = torch.cat([torch.relu(bn(conv(v))) if direction == "fwd" else conv(torch.relu(bn(v))) for v in xs], 0)
    assert float((a[0] - ref).abs().max()) < 2e-4 * float(ref.abs().max())


def test_backward_releases_what_the_batchnorm_handles_hold():
    """_BNAct / _ConvX3 kept a _BnHandle (the BatchNorm's fp32 input and ReLU mask) as plain ctx attributes, which
    autograd never frees — with the loss still referenced, every fused BatchNorm's input of step k stayed allocated through step
    k + 1's forward.  After backward(), with the loss and the output alive, only the output, the loss and the gradients remain."""
    import gc

    from avtex import train_ops
    from avtex.slowfast import ResBlock

    dev = "cuda:0"
    torch.manual_seed(0)
    blocks = [ResBlock(64, 64, 16, 3, 1).to(dev).to(memory_format=torch.channels_last_3d).train() for _ in range(3)]
    x = torch.randn(2, 64, 4, 24, 24, device=dev).contiguous(memory_format=torch.channels_last_3d).requires_grad_(True)
    for _ in range(2):  # (the first pass sizes the caches: weight planes, workspaces, tap tables)
        for m in blocks:
            m.zero_grad(set_to_none=True)
        x.grad = None
        gc.collect()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        with train_ops.bn_replicas(1):
            y = x
            for m in blocks:
                y = m(y)
        loss = y.square().mean()
        torch.cuda.synchronize()
        peak_fwd = torch.cuda.memory_allocated() - base
        loss.backward()
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated() - base
    grads = sum(p.grad.numel() * 4 for m in blocks for p in m.parameters() if p.grad is not None) + x.grad.numel() * 4
    expect = y.numel() * 4 + grads
    act = x.numel() * 4  # one full-width activation
    assert peak_fwd > expect + 4 * act  # (the forward did keep activations: the test can see a leak)
    assert held <= expect + act, (held, expect, act)  # at most one activation's worth of allocator slack / cached workspaces


@pytest.mark.parametrize("cin", [64, 320])  # 64 -> 64: the streaming pointwise kernel's STATS form; 320 -> 64: the general tile's epilogue
def test_epilogue_statistics_with_a_large_mean_stay_within_the_fp32_partials_bound(cin):
    """the convolution epilogues sum x and x^2 per thread in fp32 over 8-16 rows before the fp64 fold (the statistics
    pass squares in fp64).  With var = E[x^2] - mean^2 that costs 2^-24 (mean / std)^2 of relative variance error: for activations
    whose mean is 100 standard deviations (far from anything a BatchNorm input of SlowFast shows: the largest ratio in the trained pair
    is below 3) the two paths' normalised outputs may differ by ~1e-3, and must not differ by more."""
    import torch.nn as nn

    from avtex import train_ops

    dev = "cuda:0"
    torch.manual_seed(21)
    x0 = (torch.randn(4, cin, 2, 14, 14, device=dev) * 0.05 + 1.0).contiguous(memory_format=torch.channels_last_3d)

    def run(epi):
        torch.manual_seed(7)
        # (pointwise: no zero padding at the frame border, which would spread the outputs and hide the effect)
        conv = nn.Conv3d(cin, 64, 1, bias=False).to(dev).to(memory_format=torch.channels_last_3d).train()
        with torch.no_grad():
            conv.weight.abs_()  # every output is a positive sum: mean >> spread
        bn = nn.BatchNorm3d(64).to(dev).train()
        keep, train_ops._EPI_STATS = train_ops._EPI_STATS, epi
        try:
            with torch.no_grad(), train_ops.bn_replicas(2):
                y0 = train_ops.conv3d(x0, conv, stats=bn)
                y = train_ops.bn_act(y0, bn, relu=False)
        finally:
            train_ops._EPI_STATS = keep
        return y0, y

    (y0a, ya), (y0e, ye) = run(1), run(0)
    ratio = float((y0e.mean(dim=(0, 2, 3, 4)).abs() / y0e.std(dim=(0, 2, 3, 4))).max())
    assert ratio > 20.0, ratio  # the input really is of the hard kind
    err = float((ya - ye).abs().max())
    assert err < 2.0 ** -24 * ratio * ratio * 8.0 + 1e-5, (err, ratio)  # normalised units: the variance's relative error, with slack


@pytest.mark.parametrize("shape,g", [((8, 8, 1, 3, 3), 4), ((32, 8, 3, 1, 1), 4), ((16, 16, 1, 3, 3), 4), ((32, 32, 1, 3, 3), 2), ((64, 16, 1, 1, 1), 4)])
@pytest.mark.parametrize("transposed", [False, True])
def test_grouped_planes_by_one_gather_equal_the_torch_assembly(shape, g, transposed):
    """Round 6: the pixel-grouped planes of a few-channel layer's weight (forward filter / input-gradient filter) by ONE launch —
    ops.weight_planes_gather_f32 through a cached map of storage offsets — are bit for bit what the torch assembly (flip, cat, index,
    permute, copy) + weight_planes_f32 produced, scales included; channels-last and contiguous weights."""
    from avtex import ops, train_ops, weight_planes

    dev = "cuda:0"
    torch.manual_seed(sum(shape) + g)
    for cl in (True, False):
        w = torch.randn(shape, device=dev)
        if cl:
            w = w.contiguous(memory_format=torch.channels_last_3d)
        pd = ops.X3_BF16 if transposed else ops.X3_F16
        out = []
        for flag in (1, 0):
            keep, weight_planes._GROUP_GATHER = weight_planes._GROUP_GATHER, flag
            train_ops.invalidate_weight_cache(drop=True)
            try:
                out.append(weight_planes._grouped_planes(w, g, transposed, pd))
            finally:
                weight_planes._GROUP_GATHER = keep
        (pa, ka, ra), (pb, kb, rb) = out
        assert ka == kb and ra == rb
        for a, b in zip(pa, pb):
            assert (a is None and b is None) or torch.equal(a, b)
    train_ops.invalidate_weight_cache(drop=True)


def _flat_tensors(v, out):
    if torch.is_tensor(v):
        out.append(v)
    elif isinstance(v, (tuple, list)):
        for e in v:
            _flat_tensors(e, out)
    return out


@pytest.mark.gpu
def test_stale_weight_planes_are_remade_by_one_launch_bit_for_bit():
    """Round 6: after the optimizer step every cached set of weight planes is stale; the first lookup of the next step re-makes ALL of
    them in place with ONE launch (avt_weight_planes_multi over a device table of the single launches' own arguments).  The planes must
    be, bit for bit and scale for scale, what the one-by-one launches produce from the same weights: plain rows (fp16, row-scaled),
    transposed + tap-selected (the input gradient's filters, stride 1 and the strided layers' residue classes) and the gathered rows of
    the pixel-grouped few-channel layers."""
    from avtex import train_ops, weight_planes
    from avtex.slowfast import ResBlock

    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    net = torch.nn.Sequential(ResBlock(16, 64, 16, 3, 1), ResBlock(64, 128, 32, 1, 2), ResBlock(128, 128, 32, 3, 1))
    net = net.to(dev).to(memory_format=torch.channels_last_3d).train()
    x = torch.randn(2, 16, 4, 16, 16, device=dev).contiguous(memory_format=torch.channels_last_3d).requires_grad_(True)

    def fwd_bwd():
        net.zero_grad(set_to_none=True)
        with train_ops.bn_replicas(1):
            net(x).square().mean().backward()

    train_ops.invalidate_weight_cache(drop=True)
    keep, weight_planes._PLANES_MULTI = weight_planes._PLANES_MULTI, 1
    try:
        fwd_bwd()                                    # every entry made one by one
        own = {id(p) for p in net.parameters()}
        mine = {k: e for k, e in weight_planes.CACHE.entries.items() if e.ref() is not None and id(e.ref()) in own}
        kinds = sorted({j["fields"][4] for e in mine.values() if e.jobs for j in e.jobs})
        assert kinds == [0, 1, 2], kinds             # rows, transposed, gathered rows all occur in this net
        assert any(k[1] == "strided" and e.jobs for k, e in mine.items() if isinstance(k[1], str))
        with torch.no_grad():
            for p in net.parameters():
                p.mul_(1.03).add_(0.001)             # "the optimizer step": versions move, the tensors stay
        n0 = train_ops.CALLS["planes_multi"]
        fwd_bwd()
        assert train_ops.CALLS["planes_multi"] == n0 + 1   # ONE launch for the whole step (forward and backward filters alike)
        torch.cuda.synchronize()
        multi = {k: [t.clone() for t in _flat_tensors(e.value, [])] for k, e in mine.items() if e.jobs}
        assert all(not e.stale(e.ref()) for e in mine.values())
        weight_planes._PLANES_MULTI = 0
        train_ops.invalidate_weight_cache(drop=True)
        fwd_bwd()                                    # the same weights, one launch per plane set
        torch.cuda.synchronize()
        assert train_ops.CALLS["planes_multi"] == n0 + 1
        checked = 0
        for k, ts in multi.items():
            ref = _flat_tensors(weight_planes.CACHE.entries[k].value, [])
            assert len(ref) == len(ts)
            for a, b in zip(ts, ref):
                assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), k
                checked += 1
        assert checked >= 2 * len(multi)
    finally:
        weight_planes._PLANES_MULTI = keep
        train_ops.invalidate_weight_cache(drop=True)


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout,kernel,stride,pad,dims,groups", [
    (32, 128, (3, 1, 1), (1, 1, 1), (1, 0, 0), (6, 4, 10, 10), 3),       # 800 rows per group: 12.5 tiles of 64, 6.25 of 128
    (256, 256, (1, 3, 3), (1, 1, 1), (0, 1, 1), (2, 4, 14, 14), 2),      # res4 b at a small batch (K = 2304, two column tiles)
    (1024, 256, (3, 1, 1), (1, 1, 1), (1, 0, 0), (1, 8, 14, 14), 1),     # res4 a on ONE clip: 1568 rows, K = 3072
    (128, 256, (1, 3, 3), (1, 2, 2), (0, 1, 1), (2, 2, 14, 14), 1),      # strided: the input gradient by residue classes (row remap)
    (2048, 512, (3, 1, 1), (1, 1, 1), (1, 0, 0), (3, 8, 7, 7), 3),       # res5 a: 392 rows per group, K = 6144 (the table leaves the LDS)
])
def test_the_64_row_tile_equals_the_128_row_tile(cin, cout, kernel, stride, pad, dims, groups):
    """Round 6: wide layers at small batches run 64-row tiles (twice the workgroups: config 5 at one item per rank).  Every output
    element is the same sum in the same order as on the 128-row tile — the convolution and its input gradient are bit-identical — and
    the BatchNorm statistics both epilogues leave behind (forward: of the output; backward: of the masked gradient) differ only in how
    the rows are grouped into fp32 partial sums."""
    import torch.nn as nn

    from avtex import ops, train_ops

    dev = "cuda:0"
    torch.manual_seed(cin + cout)
    b, t, h, w = dims
    x0 = (torch.randn(b, cin, t, h, w, device=dev) * 1.5 + 0.4).contiguous(memory_format=torch.channels_last_3d)

    def run(small):
        torch.manual_seed(7)
        conv = nn.Conv3d(cin, cout, kernel, stride=stride, padding=pad, bias=False).to(dev).to(memory_format=torch.channels_last_3d).train()
        bn_in, bn_out = nn.BatchNorm3d(cin).to(dev).train(), nn.BatchNorm3d(cout).to(dev).train()
        with torch.no_grad():
            for bn in (bn_in, bn_out):
                bn.weight.copy_(torch.linspace(0.5, 1.5, bn.num_features))
                bn.bias.copy_(torch.linspace(-0.3, 0.3, bn.num_features))
        x = x0.clone().requires_grad_(True)
        was = ops.conv_x3_set_small_tile(small)
        for k in train_ops.CALLS:
            train_ops.CALLS[k] = 0
        try:
            with train_ops.bn_replicas(groups):
                y = train_ops.bn_act(x, bn_in, relu=True)
                z0 = train_ops.conv3d(y, conv, stats=bn_out)
                z = train_ops.bn_act(z0, bn_out, relu=True)
            z.square().sum().backward()
            torch.cuda.synchronize()
        finally:
            ops.conv_x3_set_small_tile(was)
        return (z0.detach(), z.detach(), x.grad, conv.weight.grad, bn_in.weight.grad, bn_in.bias.grad, bn_out.weight.grad, bn_out.bias.grad,
                bn_out.running_mean.clone(), bn_out.running_var.clone(), dict(train_ops.CALLS))

    a, e = run(1), run(0)
    m = z0_rows = a[0].numel() // cout
    assert ops._lib.lib().avt_conv3d_igemm_x3_f32_stat_rows(cout, cin * kernel[0] * kernel[1] * kernel[2], m, groups) >= 1 and z0_rows
    assert a[10]["conv_fwd_x3"] == e[10]["conv_fwd_x3"] == 1 and a[10]["bn_fwd_pre"] == e[10]["bn_fwd_pre"] == 1
    assert a[10]["dgrad_bwdstats"] == e[10]["dgrad_bwdstats"] and a[10]["dgrad_strided_x3"] == e[10]["dgrad_strided_x3"]
    assert torch.equal(a[0], e[0])  # the convolution: the same sums in the same order
    for k, name in ((1, "z"), (2, "dx"), (3, "dw"), (4, "dgamma_in"), (5, "dbeta_in"), (6, "dgamma_out"), (7, "dbeta_out"),
                    (8, "running_mean"), (9, "running_var")):
        err = float((a[k] - e[k]).norm() / e[k].norm().clamp_min(1e-20))
        assert err < (2e-4 if name == "dw" else 5e-6), (name, err)  # (dw: fp32 atomics, run-to-run order)
