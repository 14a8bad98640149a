"""Contract-grade encoder mode (csrc/conv_x3.hip: split-plane "x3" MFMA convolutions) against plain PyTorch fp32, and
the end-to-end contract of BASELINE.json's north_star ON THE SAME FRAMES: similarity scores within 1e-3 of the fp32
encoders' (contrastive_video_textures/models/models.py:335, 399), survivor sets / stitch walks compared under fixed
host RNG seeds (validate.py:554, 570-572)."""
import json

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

X3 = {"bf16x3": 0, "f16x3": 1}
# |x - hi - lo| per operand and the dropped lo*lo term: bf16 planes <= 3 * 2^-16 (random signs: far less), fp16 planes <= 3 * 2^-22 (+ 2^-24 absolute)
TOL = {"bf16x3": 2e-5, "f16x3": 2e-6}


def _planes(x, pd, dev):
    from avtex.fused_slowfast import split_planes

    hi, lo = split_planes(x, pd)
    return hi.to(dev), lo.to(dev)


@pytest.mark.parametrize("mode", ["bf16x3", "f16x3"])
@pytest.mark.parametrize("cin,cout,k,s,p,dims,with_res", [
    (64, 64, (1, 3, 3), (1, 1, 1), (0, 1, 1), (2, 4, 14, 14), False),     # Cout = 64 tile
    (128, 128, (1, 3, 3), (1, 2, 2), (0, 1, 1), (1, 3, 14, 14), True),    # strided, residual
    (80, 64, (1, 1, 1), (1, 1, 1), (0, 0, 0), (2, 4, 7, 9), True),        # pointwise, Cin = 80, ragged M
    (320, 136, (3, 1, 1), (1, 1, 1), (1, 0, 0), (1, 8, 5, 5), False),     # temporal, Cout not a tile multiple
    (8, 16, (7, 1, 1), (4, 1, 1), (3, 0, 0), (2, 32, 6, 6), False),       # lateral fusion conv, Cout <= 32 tile
    (24, 32, (3, 3, 3), (1, 1, 1), (1, 1, 1), (2, 5, 6, 7), True),        # 27 taps, K tail
    (1024, 256, (3, 1, 1), (1, 1, 1), (1, 0, 0), (1, 4, 5, 5), True),     # long K (table in global memory above 128 steps: no)
    (512, 2048, (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 2, 7, 7), True),      # 32 channel chunks: stays on the general tile
    # pointwise layers on the streaming kernel (csrc/pw_x3.hip): every (K steps, chunk width) form the encoder uses
    (64, 256, (1, 1, 1), (1, 1, 1), (0, 0, 0), (2, 3, 9, 11), True),       # res2 c + residual: K1S 2, one chunk of 16 tiles
    (128, 512, (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 4, 7, 9), True),       # res3 c: two chunks
    (256, 1024, (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 2, 7, 7), True),      # res4 c: eight chunks of 8 tiles
    (256, 64, (1, 1, 1), (1, 1, 1), (0, 0, 0), (2, 2, 10, 9), False),      # res2 a: K1S 8
    (320, 128, (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 3, 9, 9), False),      # res3 first a (after fusion): K1S 10
    (512, 128, (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 2, 9, 9), False),      # K1S 16
    (32, 128, (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 4, 6, 10), True),       # fast pathway (pixel-grouped): K1S 1
    (80, 256, (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 3, 7, 9), False),       # shortcut conv after the first fusion: K 80 -> 96
    # the XL tile (256 x 256 per workgroup; Cout % 256 == 0, K >= 512, M >= 16384): ragged M, residual, taps, strides
    (512, 256, (3, 1, 1), (1, 1, 1), (1, 0, 0), (1, 8, 46, 46), True),      # temporal taps, M = 16928 = 66.1 tiles
    (64, 256, (1, 3, 3), (1, 2, 2), (0, 1, 1), (1, 4, 130, 130), False),    # strided 3x3, K = 576 (18 half-steps)
    (520, 512, (1, 1, 1), (1, 2, 2), (0, 0, 0), (1, 8, 92, 92), True),      # strided pointwise, K = 520: a 32-step tail of 8
    # appended last so that the ids of the rows above keep their index
    (24, 40, (2, 1, 3), (1, 2, 1), (1, 0, 2), (2, 5, 8, 6), True),        # no two extents / pads alike, output 6 x 4 x 8: a swapped pair shows
])
def test_conv_x3_matches_fp32(avt, dev, mode, cin, cout, k, s, p, dims, with_res):
    from avtex.fused_slowfast import Act, FusedConv

    pd = X3[mode]
    torch.manual_seed(cin * 7 + cout)
    conv = nn.Conv3d(cin, cout, k, stride=s, padding=p, bias=False)
    bn = nn.BatchNorm3d(cout)
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5); bn.bias.uniform_(-0.5, 0.5)
        bn.running_mean.uniform_(-0.2, 0.2); bn.running_var.uniform_(0.5, 1.5)
    bn.eval()
    b, t, h, w = dims
    x = torch.randn(b, cin, t, h, w)
    fc = FusedConv(conv, bn, True, dev, x3=pd)
    m_in = b * t * h * w
    xh, xl = _planes(x.permute(0, 2, 3, 4, 1).reshape(m_in, cin), pd, dev)
    od = fc.out_dims(dims)
    m_out = od[0] * od[1] * od[2] * od[3]
    with torch.no_grad():
        ref = bn(conv(x.double().float()))
    res = None
    if with_res:
        r = torch.randn(m_out, cout)
        rh, rl = _planes(r, pd, dev)
        res = Act(rh, od, lo=rl)
        ref = ref + r.view(od[0], od[1], od[2], od[3], cout).permute(0, 4, 1, 2, 3)
    ref = F.relu(ref)
    out = fc(Act(xh, dims, 0, cin, lo=xl), res=res)
    torch.cuda.synchronize()
    got = out.float(pd).cpu().view(od[0], od[1], od[2], od[3], cout).permute(0, 4, 1, 2, 3)
    # fp64 reference of the same folded arithmetic
    with torch.no_grad():
        ref64 = bn.double()(conv.double()(x.double()))
        if with_res:
            ref64 = ref64 + r.double().view(od[0], od[1], od[2], od[3], cout).permute(0, 4, 1, 2, 3)
        ref64 = F.relu(ref64)
    scale = ref64.abs().max().item()
    err = (got.double() - ref64).abs().max().item()
    err32 = (ref.double() - ref64).abs().max().item()  # what torch's own fp32 conv is off by
    assert err < TOL[mode] * max(scale, 1.0) + 2 * err32, (err, err32, scale)


@pytest.mark.parametrize("mode", ["bf16x3", "f16x3"])
def test_pool_mean_pack_x3(avt, dev, mode):
    """Plane-pair max-pool, head mean and clip packing against torch on the joined fp32 values."""
    from avtex import ops

    pd = X3[mode]
    torch.manual_seed(1)
    bt, h, w, c = 3, 9, 10, 16
    x = torch.randn(bt, h, w, c)
    xh, xl = _planes(x.reshape(-1, c), pd, dev)
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    oh = torch.empty((bt * ho * wo, c), dtype=torch.bfloat16, device=dev)
    ol = torch.empty_like(oh)
    ops.maxpool_hw3s2_x3((xh.data_ptr(), xl.data_ptr()), (oh.data_ptr(), ol.data_ptr()), bt, h, w, c, c, c, pd)
    dt = torch.float16 if pd == 1 else torch.bfloat16
    joined = (xh.view(dt).float() + xl.view(dt).float()).cpu().view(bt, h, w, c)
    ref = F.max_pool2d(joined.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).reshape(-1, c)
    got = (oh.view(dt).float() + ol.view(dt).float()).cpu()
    assert torch.equal(got, ref)  # a max of representable values is representable: exact
    emb = torch.zeros((bt, 40), dtype=torch.float32, device=dev)
    ops.mean_positions_x3((xh.data_ptr(), xl.data_ptr()), bt, h * w, c, c, emb, 8, pd)
    assert torch.allclose(emb[:, 8:24].cpu(), joined.view(bt, h * w, c).mean(1), rtol=0, atol=1e-6)
    # clip packing: the joined planes equal the fp32 packing up to the plane format
    g = torch.Generator().manual_seed(9)
    W, S, n = 20, 4, 3
    frames = torch.randint(0, 256, ((n - 1) * S + W, 40, 52, 3), generator=g, dtype=torch.uint8).to(dev)
    starts = np.arange(n) * S
    s32, f32 = ops.clip_pack(frames, starts, W, out_hw=64, dtype=torch.float32)
    sx, fx = ops.clip_pack(frames, starts, W, out_hw=64, layout="ndhwc4", planes=mode)
    for ref32, got in ((s32, sx), (f32, fx)):
        j = got.float()
        assert (j[..., 3] == 0).all()
        d = (j[..., :3].permute(0, 4, 1, 2, 3) - ref32).abs().max().item()
        assert d < (1e-5 if pd == 0 else 1e-6) * 3


@pytest.mark.parametrize("mode", ["bf16x3", "f16x3"])
def test_pw_x3_slices_and_agreement_with_general_tile(avt, dev, mode):
    """The streaming pointwise kernel reads and writes channel slices of wider row buffers (the lateral-fusion concat) and
    leaves their neighbours alone; its result agrees with the general x3 tile's to the last few bits of fp32."""
    import avtex.fused_slowfast as fsf

    pd = X3[mode]
    torch.manual_seed(4)
    conv = nn.Conv3d(80, 64, (1, 1, 1), bias=False)
    dims, m = (2, 3, 7, 5), 2 * 3 * 7 * 5
    x = torch.randn(m, 96)
    xh, xl = _planes(x, pd, dev)
    outs = []
    for flag in (1, 0):
        keep, fsf._PW_X3 = fsf._PW_X3, flag
        fc = fsf.FusedConv(conv, None, True, dev, x3=pd)
        fsf._PW_X3 = keep
        assert (fc.pw is not None) == bool(flag)
        wide = fsf.new_act(m, 160, dims, dev, True)
        wide.buf.fill_(3.0)
        wide.lo.fill_(3.0)
        fc(fsf.Act(xh, dims, 8, 80, lo=xl), out=fsf.Act(wide.buf, dims, 32, 64, lo=wide.lo))
        torch.cuda.synchronize()
        assert (wide.buf[:, :32] == 3).all() and (wide.buf[:, 96:] == 3).all() and (wide.lo[:, :32] == 3).all()
        outs.append(fsf.Act(wide.buf, dims, 32, 64, lo=wide.lo).float(pd).cpu())
    ref = torch.relu(x[:, 8:88].double() @ conv.weight.detach().view(64, 80).double().t())
    assert (outs[0].double() - ref).abs().max() < TOL[mode] * max(ref.abs().max().item(), 1.0)
    assert (outs[0] - outs[1]).abs().max() < 2 * TOL[mode] * max(ref.abs().max().item(), 1.0)


@pytest.mark.parametrize("mode", ["bf16x3", "f16x3"])
def test_stem_x3_patch_kernel_equals_general_tile(avt, dev, mode):
    """Both stems + pools at the production clip size: the patch-resident plane-pair stem kernel (csrc/stem_conv.hip, PL > 0)
    against the same layers on the general x3 tile, and against the fp32 module's stems."""
    import avtex.fused_slowfast as fsf
    from avtex import ops
    from avtex.slowfast import SlowFast

    pd = X3[mode]
    torch.manual_seed(2)
    m = SlowFast().eval()
    with torch.no_grad():
        for mod in m.s1.modules():
            if isinstance(mod, nn.BatchNorm3d):
                mod.weight.uniform_(0.6, 1.2); mod.bias.uniform_(-0.2, 0.2)
                mod.running_mean.uniform_(-0.1, 0.1); mod.running_var.uniform_(0.8, 1.2)
    enc = fsf.SlowFastMFMA(m, dev, precision=mode)
    slow32, fast32 = torch.randn(1, 3, 8, 224, 224), torch.randn(1, 3, 32, 224, 224)
    with torch.no_grad():
        ref = m.s1([slow32, fast32])

    def cl4(v):
        f = torch.zeros((v.shape[0], v.shape[2], 224, 224, 4), dtype=torch.float32, device=dev)
        f[..., :3] = v.to(dev).permute(0, 2, 3, 4, 1)
        hi, lo = fsf.split_planes(f, pd)
        return ops.SplitClip(hi, lo, pd)

    outs = {}
    for flag in (1, 0):
        keep, fsf._STEM_LDS = fsf._STEM_LDS, flag
        outs[flag] = [enc._stem_x3(c, clip)[0].float(pd).cpu() for c, clip in ((enc.stem_s, cl4(slow32)), (enc.stem_f, cl4(fast32)))]
        fsf._STEM_LDS = keep
        torch.cuda.synchronize()
    # ... and into a channel slice of a wider buffer (the first lateral fusion's concat buffer)
    from avtex.fused_slowfast import Act, new_act
    wide = new_act(1 * 8 * 56 * 56, 64 + 16, (1, 8, 56, 56), dev, True)
    wide.buf.zero_(); wide.lo.zero_()
    enc._stem_x3(enc.stem_s, cl4(slow32), out=Act(wide.buf, wide.dims, 0, 64, lo=wide.lo))
    torch.cuda.synchronize()
    assert torch.equal(wide.float(pd).cpu()[:, :64], outs[1][0]) and float(wide.float(pd)[:, 64:].abs().max()) == 0.0
    for k in range(2):
        want = ref[k].permute(0, 2, 3, 4, 1).reshape(-1, ref[k].shape[1])
        scale = want.abs().max().item()
        assert (outs[1][k] - want).abs().max().item() < 5 * TOL[mode] * scale  # vs torch's own fp32 conv
        assert (outs[1][k] - outs[0][k]).abs().max().item() < 2 * TOL[mode] * scale


def _calibrated_pair(dev, n, hw_src=128):
    from avtex import ops, synth
    from avtex.slowfast import SlowFast

    W, S = 20, 4
    video = synth.structured_video(5, n * S + W, hw_src, hw_src)
    torch.manual_seed(0)
    q_mod = synth.randomise_bn(SlowFast().eval(), 10, 0.5).to(dev)
    torch.manual_seed(1)
    t_mod = synth.randomise_bn(SlowFast().eval(), 11, 0.5).to(dev)
    cal = np.linspace(0, n - 1, 8).astype(np.int64) * S
    slow, fast = ops.clip_pack(video.to(dev), cal, W, out_hw=224, dtype=torch.float32)
    synth.calibrate_bn(q_mod, slow, fast)
    synth.calibrate_bn(t_mod, slow, fast)
    return video, q_mod.eval(), t_mod.eval(), W, S


def _tables(dev, video, qe, te, W, S, batch):
    from avtex.texture import TextureEngine

    eng = TextureEngine(qe, te, None, window=W, stride=S, temp=0.1, img_size=224, model_type=1, device=dev,
                        enc_batch=batch)
    eng.set_video(video)
    qv, tv = eng.build_tables()
    torch.cuda.synchronize()
    return qv.clone(), tv.clone()


@pytest.mark.parametrize("mode", ["bf16x3", "f16x3"])
def test_x3_encoder_matches_fp32_module(avt, dev, mode):
    """Whole SlowFast-8x8-R50 on the split-plane kernels vs the PyTorch module in fp32 (MIOpen), same clips."""
    from avtex.fused_slowfast import SlowFastMFMA

    video, q_mod, _, W, S = _calibrated_pair(dev, 8)
    enc = SlowFastMFMA(q_mod, dev, precision=mode)
    from avtex import ops
    starts = np.arange(4) * S
    slow, fast = ops.clip_pack(video.to(dev), starts, W, out_hw=224, dtype=torch.float32)
    with torch.no_grad():
        ref = q_mod([slow, fast])
    y_plugin = enc([slow, fast])  # the plugin contract (fp32 NCTHW in): split on the fly
    sx, fx = ops.clip_pack(video.to(dev), starts, W, out_hw=224, layout="ndhwc4", planes=mode)
    y = enc.forward_ndhwc4(sx, fx)
    rel = ((y - ref).norm(dim=1) / ref.norm(dim=1)).max().item()
    relp = ((y_plugin - ref).norm(dim=1) / ref.norm(dim=1)).max().item()
    print("%s encoder vs fp32 module: rel embedding error %.3e (plugin entry %.3e)" % (mode, rel, relp))
    # measured on MI355X: bf16x3 1.3e-4, f16x3 1.5e-5 (two fp32 implementations, oneDNN vs MIOpen, differ by 6e-6)
    tol = 5e-4 if mode == "bf16x3" else 5e-5
    assert y.shape == (4, 2304) and rel < tol and relp < tol


def test_contract_on_the_same_frames(avt, dev):
    """north_star: outputs match the reference fp32 path ON THE SAME FRAMES (scores within 1e-3).  Real SlowFast x2,
    BN randomised and calibrated, structured video, 256 windows at 224^2: the contract-grade MFMA encoders vs the fp32
    nn.Module encoders; the fast bf16 mode is measured beside them (it does NOT meet the contract, by two orders)."""
    from avtex import agreement
    from avtex.fused_slowfast import SlowFastMFMA

    n = 256
    video, q_mod, t_mod, W, S = _calibrated_pair(dev, n)
    q32, t32 = _tables(dev, video, q_mod.float(), t_mod.float(), W, S, 16)
    report = {}
    for mode in ("f16x3", "bf16x3", "bf16"):
        kw = {} if mode == "bf16" else {"precision": mode}
        qv, tv = _tables(dev, video, SlowFastMFMA(q_mod, dev, **kw), SlowFastMFMA(t_mod, dev, **kw), W, S, 32)
        report[mode] = agreement.compare_tables(qv, tv, q32, t32, 0.1, W, S)
    print("CONTRACT " + json.dumps(report))
    for mode in ("f16x3", "bf16x3"):  # f16x3 = the mode validate() defaults to and bench.py headlines
        r = report[mode]
        assert r["score_spread"] > 1.0  # non-degenerate inputs: the scores spread over more than 1.0
        assert r["max_abs_dscore"] < 1e-3, (mode, r)  # the stated tolerance: BASELINE.json north_star
        assert r["thresholds"]["0.0"]["rows_identical_survivors"] >= 0.98
        assert r["thresholds"]["0.3"]["rows_identical_survivors"] >= 0.90
        assert report["bf16"]["max_abs_dscore"] > r["max_abs_dscore"]
    # the default mode is held to more: survivors of EVERY row and the frames lists of three host-RNG seeds identical to the
    # fp32 modules' at th = 0.0 (the discriminating leg: one survivor per row) and at th = 0.3
    d = report["f16x3"]
    assert d["max_abs_dscore"] < 1e-4, d  # measured 2.4e-5
    for th in ("0.0", "0.3"):
        assert d["thresholds"][th]["rows_identical_survivors"] == 1.0, d
        assert d["thresholds"][th]["frames_lists_identical"] == "3/3", d


def test_th0_exact_ties_on_the_config4_calibration(avt, dev):
    """Threshold 0.0 keeps the candidates that tie EXACTLY with the row maximum (validate.py:553-554).  bench.py --config 4 /
    --windows 2048 calibrates the synthetic BatchNorms on 8 clips spread over 2048 windows, which leaves a block of the first 128
    windows with every feature dead: they embed to one constant vector and the fp32 reference ITSELF has rows with several
    bit-identical maxima — there a "0/3 frames lists at th 0.0" says nothing about the kernels.  This pins
    what does hold on that calibration: wherever the survivors differ, the reference's own scores of the candidates involved lie
    within twice the arithmetics' distance of each other (exact ties or near ties of the dead-feature block); th 0.3 is identical
    everywhere."""
    import os
    import sys

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from avtex import agreement
    from avtex.fused_slowfast import SlowFastMFMA

    args = bench.build_parser().parse_args(["--windows", "2048"])
    video, q_mod, t_mod = bench.build_inputs(args, 0, dev)
    n, W, S = 128, 20, 4
    sub = video[: n * S + W]
    q32, t32 = _tables(dev, sub, q_mod.float(), t_mod.float(), W, S, 16)
    qv, tv = _tables(dev, sub, SlowFastMFMA(q_mod, dev, precision="f16x3"), SlowFastMFMA(t_mod, dev, precision="f16x3"), W, S, 32)
    r = agreement.compare_tables(qv, tv, q32, t32, 0.1, W, S)
    print("TH0-TIES " + json.dumps(r))
    t0, t3 = r["thresholds"]["0.0"], r["thresholds"]["0.3"]
    assert r["max_abs_dscore"] < 1e-4, r
    assert t0["rows_with_exact_ties_ref"] > 0, "the calibration no longer produces exact ties in the fp32 reference: re-derive this test"
    # measured (profiles/r06/th0_ties_config4_calibration_first_run.log): 37 of 128 reference rows have exact ties, 35 of them keep a
    # subset of the tied candidates; 3 of the other 91 rows differ too — NEAR ties of the same block of dead-feature windows.  What
    # holds for every differing row: the reference separates its own maximum from what the other arithmetic kept by no more than
    # twice the two arithmetics' distance (3e-5), thirty times inside the contract's score tolerance (1e-3)
    assert t0["max_ref_gap_on_differing_rows"] <= 2.0 * r["max_abs_dscore"] + 1e-6, r
    assert t0["max_ref_gap_on_differing_rows"] < 1e-4, r
    k, m = (int(v) for v in t0["tie_rows_survivors_subset_of_ref_ties"].split("/"))
    assert m == t0["rows_with_exact_ties_ref"] and k >= 0.8 * m, r
    assert t0["rows_identical_survivors_outside_tie_rows"] >= 0.9, r
    assert t3["rows_identical_survivors"] == 1.0 and t3["frames_lists_identical"] == "3/3", r


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_x3_fp16_planes_propagate_nan_and_inf(avt, dev, bad):
    """A poisoned activation must reach the output: the fp16-plane split clamps FINITE values to 65504 but keeps a NaN a NaN
    and an infinity an infinity (csrc/split_planes.h; fminf / fmaxf alone would turn a NaN into -65504), and the kernels'
    ReLU keeps a NaN like torch.relu does (fmaxf(NaN, 0) would return 0).  An infinite input comes out NON-FINITE (inf
    times a weight's low plane of either sign is -inf or +inf: the accumulator may hold a NaN) — never a plausible number.
    Checked through both contract-grade convolution kernels: the general tile (3x3) and the streaming pointwise kernel."""
    import torch.nn as nn

    from avtex import ops
    from avtex.fused_slowfast import Act, FusedConv, split_planes

    torch.manual_seed(3)
    dims = (1, 2, 8, 8)
    m = dims[0] * dims[1] * dims[2] * dims[3]
    for k, cin, cout in (((1, 3, 3), 32, 64), ((1, 1, 1), 64, 256)):
        conv = nn.Conv3d(cin, cout, k, padding=tuple(x // 2 for x in k), bias=False)
        with torch.no_grad():
            conv.weight.abs_()  # positive weights: an infinity cannot meet its opposite
        fc = FusedConv(conv, None, True, dev, x3=ops.X3_F16)
        x = torch.rand((m, cin)) + 0.5
        x[5, 7] = bad
        hi, lo = split_planes(x, ops.X3_F16)
        if bad != bad:
            assert torch.isnan(hi.view(torch.float16)[5, 7])
        y = fc(Act(hi.to(dev), dims, lo=lo.to(dev))).float(ops.X3_F16).cpu()
        # position 5 = (frame 0, row 0, col 5): its own output row is poisoned in every channel; far rows stay finite
        assert (torch.isnan(y[5]).all() if bad != bad else (~torch.isfinite(y[5])).all()), (k, y[5][:8])
        assert torch.isfinite(y[m - 1]).all()


@pytest.mark.parametrize("scale", [2.0 ** 12, 2.0 ** -16])
def test_x3_fp16_planes_at_the_edges_of_their_range(avt, dev, scale):
    """Network-level range test of the fp16 planes: a residual block's worth of layers ([3,1,1] -> [1,3,3] -> [1,1,1] + residual)
    with activations scaled to ~2^12 (their 4.5-sigma tail and the layers' outputs stay a factor 2-3 under the fp16 clamp at
    65504; at 2^14 the tails ARE clamped, and the test's first form measured exactly that) and to ~2^-16 (below 2^-14 the planes go from
    relative to ABSOLUTE precision, 2^-24 per element) against fp64 on the same weights.  Large: full 2^-22-grade relative
    accuracy.  Tiny: the error is bounded by the absolute floor — 2^-24 per input element times the layer's gain — and the
    test asserts that bound, i.e. documents where fp16 planes stop being fp32-grade (bf16 planes do not have this floor)."""
    import torch.nn as nn

    from avtex import ops
    from avtex.fused_slowfast import Act, FusedConv, split_planes

    torch.manual_seed(11)
    dims = (2, 4, 14, 14)
    m = dims[0] * dims[1] * dims[2] * dims[3]
    c, cm = 128, 32
    a = nn.Conv3d(c, cm, (3, 1, 1), padding=(1, 0, 0), bias=False)
    b = nn.Conv3d(cm, cm, (1, 3, 3), padding=(0, 1, 1), bias=False)
    cc = nn.Conv3d(cm, c, (1, 1, 1), bias=False)
    for conv in (a, b, cc):  # unit-gain layers, so that every intermediate stays at the input's magnitude
        fan = conv.weight[0].numel()
        nn.init.normal_(conv.weight, std=(2.0 / fan) ** 0.5)
    x = (torch.randn((m, c)) * scale).float()
    x5 = x.view(dims + (c,)).permute(0, 4, 1, 2, 3).double()
    with torch.no_grad():
        r = torch.relu(a.double()(x5))
        r = torch.relu(b.double()(r))
        ref = torch.relu(cc.double()(r) + x5).permute(0, 2, 3, 4, 1).reshape(m, c)
    for mode in (ops.X3_F16, ops.X3_BF16):
        fa, fb, fc = (FusedConv(v.float(), None, True, dev, x3=mode) for v in (a, b, cc))
        hi, lo = split_planes(x, mode)
        xa = Act(hi.to(dev), dims, lo=lo.to(dev))
        y = fc(fb(fa(xa)), res=xa, relu=True).float(mode).cpu().double()
        err = (y - ref).abs().max().item()
        rel = err / ref.abs().max().item()
        print("x3 range test scale 2^%d planes %s: max abs err %.3e, relative to the output range %.3e"
              % (int(np.log2(scale)), "f16" if mode == ops.X3_F16 else "bf16", err, rel))
        assert torch.isfinite(y).all()
        if mode == ops.X3_BF16 or scale > 1:
            assert rel < (2e-4 if mode == ops.X3_BF16 else 2e-6), rel  # relative precision at every magnitude / in range
        else:
            # fp16 planes under 2^-14: absolute floor 2^-24 per element (+ the weights' own 2^-22): a few 2^-24 after 3 layers
            assert err < 16 * 2.0 ** -24, err


def test_validate_default_path_is_contract_grade(avt, dev, capsys):
    """validate() with the CLI defaults (--enc_impl auto, --enc_dtype fp32) must not silently run the bf16 encoder: it
    runs the contract-grade MFMA mode, and its frames list equals the oracle's walk over tables built by the fp32
    nn.Module encoders (the reference's arithmetic, models.py:335, 399) from the same frames."""
    import os
    import sys
    from types import SimpleNamespace

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import cref, ref_py

    from avtex.main import build_parser

    L = 20
    video, q_mod, t_mod, W, S = _calibrated_pair(dev, L + 1, hw_src=64)
    video = video[: L * S + W + 1]
    model = avt.ContrastivePredictionTemporal(q_mod, t_mod, None, 1, 128, 0.1, W, S, 0.3, mini_batchsize=8,
                                              enc_arch="slowfast", img_size=224).to(dev).eval()
    defaults = build_parser().parse_args(["-vdata", "x"])
    assert defaults.enc_dtype == "fp32" and defaults.enc_impl == "auto"
    args = SimpleNamespace(vdata=None, adata=None, dadata=None, subsample_rate=1, fps=4, stride=S, window=W,
                           enc_arch="slowfast", img_size=224, model_type=1, mini_batchsize=8, threshold=0.3, alpha=0.5,
                           temp=0.1, driving_audio=None, da_feats="VGG", interpolation=False, new_video_length=16,
                           results_folder=None, logname="exp", batch_size=24, stitch_mode="aligned", enc_batch=8,
                           enc_impl=defaults.enc_impl, enc_dtype=defaults.enc_dtype)
    np.random.seed(7)
    frames = avt.validate(model, args, video_name="x", model_type=1, video=(video, 4.0))
    out = capsys.readouterr().out
    assert "precision f16x3 (contract grade)" in out
    # the reference's arithmetic: fp32 module encoders (MIOpen) -> oracle normalise / similarity / select / walk
    q32, t32 = _tables(dev, video, q_mod.float(), t_mod.float(), W, S, 8)
    qn, _, _ = cref.l2norm_rows(q32.cpu().numpy(), want_split=False)
    tn, _, _ = cref.l2norm_rows(t32.cpu().numpy(), want_split=False)
    sim = cref.sim_f32(qn, tn, 0.1)

    def row_fn(q):
        o = cref.row_transition(sim[q : q + 1], q_ids=np.array([q]), n_seg=L, threshold=0.3, cap=L)
        return o["idx"][0, : o["cnt"][0]], ref_py.target_segment_ids(q, L)

    ref_frames, _, _ = ref_py.stitch_walk(row_fn, len(video), W, S, 64, q_id=10, rng=np.random.RandomState(7))
    assert frames == ref_frames


def _fast_block(cin, c, cm, seed, stride=1):
    """A fast-pathway bottleneck as slowfast.ResBlock builds it ([3,1,1] -> [1,3,3] -> [1,1,1]), BatchNorms randomised."""
    from avtex.slowfast import ResBlock

    torch.manual_seed(seed)
    blk = ResBlock(cin, c, cm, 3, stride).eval()
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, nn.BatchNorm3d):
                m.weight.uniform_(0.5, 1.5); m.bias.uniform_(-0.3, 0.3)
                m.running_mean.uniform_(-0.2, 0.2); m.running_var.uniform_(0.5, 1.5)
    return blk


@pytest.mark.parametrize("mode", ["bf16x3", "f16x3"])
@pytest.mark.parametrize("cin,c,cm,dims,tchunk", [
    (32, 32, 8, (2, 7, 13, 12), 4),      # res2 identity form, small: ragged strips (13 rows / 5), ragged frame chunks (7 / 4)
    (64, 64, 16, (1, 5, 9, 10), 16),     # res3 form: partial tiles, two k-steps per frame tap
    (128, 128, 32, (2, 4, 7, 6), 3),     # res4 form: 32-wide bottleneck (one tap per k-step)
    (8, 32, 8, (2, 6, 11, 12), 4),       # res2's first block: 8 input channels, shortcut conv, lane-rotated operand
    (32, 32, 8, (1, 8, 56, 56), 16),     # production shapes
    (8, 32, 8, (1, 8, 56, 56), 16),
    (64, 64, 16, (1, 6, 28, 28), 16),
    (128, 128, 32, (1, 6, 14, 14), 32),
    (32, 64, 16, (2, 5, 10, 12), 4),     # strided first block (res3's form), small: ragged strips (5 output rows / 3)
    (64, 128, 32, (1, 4, 6, 8), 3),      # res4's form
    (32, 64, 16, (1, 6, 56, 56), 8),     # ... at the production shapes
    (64, 128, 32, (1, 6, 28, 28), 8),
])
def test_bneck_x3_matches_fp64_and_the_per_layer_kernels(avt, dev, mode, cin, c, cm, dims, tchunk):
    """csrc/bneck_x3.hip (a whole fast-pathway bottleneck in one kernel, register-resident frame ring) against the same block
    in fp64 on PyTorch, and against the four per-layer split-plane launches it replaces."""
    import avtex.fused_slowfast as fsf
    from avtex import ops
    from avtex.fused_slowfast import Act, _BlockX3, split_planes

    pd = X3[mode]
    st = 2 if (cin != c and cin != 8) else 1
    blk = _fast_block(cin, c, cm, 17 * cin + c, stride=st)
    b, t, h, w = dims
    m = b * t * h * w
    torch.manual_seed(5)
    x = torch.randn((m, cin)) * 1.5
    hi, lo = split_planes(x, pd)
    xq = (hi.view(torch.float16 if pd == 1 else torch.bfloat16).double() + lo.view(torch.float16 if pd == 1 else torch.bfloat16).double())
    with torch.no_grad():
        ref = blk.double()(xq.view(b, t, h, w, cin).permute(0, 4, 1, 2, 3)).permute(0, 2, 3, 4, 1).reshape(m // (st * st), c)
    blk = blk.float()
    assert ops.bneck_x3_supported(cin, c, w)
    old = fsf._FUSE_TCHUNK_X3
    fsf._FUSE_TCHUNK_X3 = tchunk
    try:
        fused = _BlockX3(blk, dev, pd)
        assert fused.fused is not None
        xa = Act(hi.to(dev), dims, lo=lo.to(dev))
        y = fused(xa)
        yf = y.float(pd).cpu().double()
    finally:
        fsf._FUSE_TCHUNK_X3 = old
    fsf._FUSE_BLOCK_X3, keep = 0, fsf._FUSE_BLOCK_X3
    try:
        plain = _BlockX3(blk, dev, pd)
        assert plain.fused is None
        yp = plain(xa).float(pd).cpu().double()
    finally:
        fsf._FUSE_BLOCK_X3 = keep
    scale = ref.abs().max().item()
    err_f, err_p = (yf - ref).abs().max().item() / scale, (yp - ref).abs().max().item() / scale
    print("bneck_x3 %s cin %d c %d dims %s: fused %.2e, per-layer %.2e of the output range from fp64" % (mode, cin, c, dims, err_f, err_p))
    tol = 3 * TOL[mode]  # three layers deep
    assert err_f < tol and err_p < tol, (err_f, err_p)
    assert (yf - yp).abs().max().item() / scale < tol


@pytest.mark.parametrize("mode", ["bf16x3", "f16x3"])
def test_vggish_x3_matches_fp32_module(avt, dev, mode):
    """Contract-grade VGGish (audio_models/vggish.py:15-46 on csrc/conv_x3.hip + the plane-pair 2x2 max-pool) against the fp32
    plugin module on MIOpen: [n, 12288] in the NHWC flatten order, relative error <= 5e-5 (fp16 planes) / 5e-4 (bf16
    planes) — config 3's default path then has no MIOpen convolution."""
    from avtex.fused_vggish import VGGishMFMA
    from avtex.vggish import VGGish

    torch.manual_seed(6)
    m = VGGish().eval()
    with torch.no_grad():
        for mod in m.features:
            if isinstance(mod, nn.Conv2d):
                nn.init.kaiming_normal_(mod.weight, nonlinearity="relu")
                mod.bias.uniform_(-0.1, 0.1)
    x = torch.randn(5, 1, 100, 64) * 2 - 1  # log-mel range
    y = VGGishMFMA(m, dev, precision=mode)(x).cpu()
    with torch.no_grad():
        ref64 = m.double()(x.double())
        ref32 = m.float().to(dev)(x.to(dev)).cpu()
    assert y.shape == (5, 12288) and torch.isfinite(y).all()
    rel = ((y.double() - ref64).norm(dim=1) / ref64.norm(dim=1)).max().item()
    rel32 = ((ref32.double() - ref64).norm(dim=1) / ref64.norm(dim=1)).max().item()
    print("vggish %s vs fp64: rel %.3e (fp32 module on MIOpen vs fp64: %.3e)" % (mode, rel, rel32))
    assert rel < (5e-4 if mode == "bf16x3" else 5e-5)


def test_validate_m2_default_path_runs_vggish_on_the_split_plane_kernels(avt, dev, capsys, monkeypatch):
    """Config 3 with the CLI defaults (--enc_dtype fp32 = f16x3): SlowFast x2 AND VGGish run on the contract-grade kernels —
    the audio encoder validate() hands the engine is a VGGishMFMA in the same precision, not the MIOpen module."""
    from types import SimpleNamespace

    import avtex.texture as texture
    from avtex.fused_vggish import VGGishMFMA
    from avtex.slowfast import SlowFast

    torch.manual_seed(0)
    model = avt.ContrastivePredictionTemporal(SlowFast(), SlowFast(), avt.VGGish(), 2, 128, temp=0.1, window=5, stride=2,
                                              threshold=0.3, mini_batchsize=8, enc_arch="slowfast", img_size=64)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm3d):
                m.weight.uniform_(0.5, 1.0)
    model = model.to(dev).eval()
    seen = {}
    real = texture.TextureEngine

    def spy(q_enc, t_enc, a_enc, **kw):
        seen["a"], seen["q"] = a_enc, q_enc
        return real(q_enc, t_enc, a_enc, **kw)

    monkeypatch.setattr(texture, "TextureEngine", spy)
    rng = np.random.default_rng(3)
    wave = (0.1 * rng.standard_normal(7 * 16000)).astype(np.float32)
    g = torch.Generator().manual_seed(2)
    video = torch.randint(0, 256, (70, 48, 48, 3), generator=g, dtype=torch.uint8)
    args = SimpleNamespace(vdata=None, adata=None, dadata=None, subsample_rate=1, fps=10, stride=2, window=5,
                           enc_arch="slowfast", img_size=64, model_type=2, mini_batchsize=8, threshold=0.3, alpha=0.5,
                           temp=0.1, driving_audio=None, da_feats="VGG", interpolation=False, new_video_length=2,
                           results_folder=None, logname="exp", batch_size=8, stitch_mode="aligned", ref_num_gpus=1,
                           enc_batch=8, enc_impl="auto", enc_dtype="fp32")
    np.random.seed(5)
    frames = avt.validate(model, args, video_name="x", model_type=2, video=(video.numpy(), 10.0), audio=(wave, 16000))
    assert len(frames) >= 10
    assert isinstance(seen["a"], VGGishMFMA) and seen["a"].precision == "f16x3" and seen["q"].precision == "f16x3"


@pytest.mark.parametrize("mode", ["bf16x3", "f16x3"])
@pytest.mark.parametrize("dims,ldi,ldo", [((2, 3, 9, 11), 64, 64), ((1, 2, 56, 56), 64, 144), ((1, 4, 7, 5), 80, 64)])
def test_conv33_x3_direct_operand_kernel(avt, dev, mode, dims, ldi, ldo):
    """csrc/conv33_x3.hip (slow res2's [1,3,3] 64 -> 64 + BN + ReLU, activations as MFMA operands straight from global memory,
    zero padding by out-of-range offsets, persistent workgroups over 32-position tiles) against fp64 on PyTorch and the
    general x3 tile: ragged tile counts, row / frame borders inside a tile, input and output as channel slices of wider rows."""
    from avtex import ops
    from avtex.fused_slowfast import Act, FusedConv, pack_c33_x3, split_planes

    pd = X3[mode]
    torch.manual_seed(dims[2] * 7 + ldi)
    conv = nn.Conv3d(64, 64, (1, 3, 3), padding=(0, 1, 1), bias=False)
    bn = nn.BatchNorm3d(64).eval()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5); bn.bias.uniform_(-0.5, 0.5)
        bn.running_mean.uniform_(-0.2, 0.2); bn.running_var.uniform_(0.5, 1.5)
    b, t, h, w = dims
    m = b * t * h * w
    xw = torch.randn(m, ldi)
    hi, lo = split_planes(xw, pd)
    dt = torch.float16 if pd == 1 else torch.bfloat16
    xq = (hi.view(dt).double() + lo.view(dt).double())[:, :64]
    with torch.no_grad():
        ref = F.relu(bn.double()(conv.double()(xq.view(b, t, h, w, 64).permute(0, 4, 1, 2, 3)))).permute(0, 2, 3, 4, 1).reshape(m, 64)
    fc = FusedConv(conv.float(), bn.float(), True, dev, x3=pd)
    packed = pack_c33_x3(fc._folded[0], fc._folded[1], pd, dev)
    xa = Act(hi.to(dev), dims, 0, 64, lo=lo.to(dev))
    ob = torch.full((m, ldo), 7.0)
    oh, ol = split_planes(ob, pd)
    out = Act(oh.to(dev), dims, ldo - 64, 64, lo=ol.to(dev))
    ops.conv33_x3(xa.ptrs, packed, out.ptrs, b, t, h, w, ldi, ldo, pd, relu=True)
    torch.cuda.synchronize()
    got = out.float(pd).cpu().double()
    gen = fc(xa).float(pd).cpu().double()
    scale = ref.abs().max().item()
    err, err_g = (got - ref).abs().max().item() / scale, (gen - ref).abs().max().item() / scale
    print("conv33_x3 %s %s: direct %.2e, general tile %.2e of the output range from fp64" % (mode, dims, err, err_g))
    assert err < TOL[mode] and err_g < TOL[mode]
    if ldo > 64:  # the columns in front of the slice are untouched
        whole = Act(out.buf, dims, 0, ldo, lo=out.lo).float(pd).cpu()
        assert torch.equal(whole[:, : ldo - 64], torch.full((m, ldo - 64), 7.0))


@pytest.mark.parametrize("mode", ["bf16x3", "f16x3"])
def test_pw_chain_x3_is_bit_identical_to_the_two_launches(avt, dev, mode):
    """csrc/pw_x3.hip's chained form (slow res2: c of block i + residual + ReLU -> a of block i + 1 in one pass, y handed over in
    registers) against the two pointwise launches it replaces: the same rounded planes feed the second GEMM in the same k
    order, so y AND z are bit-identical; and the whole encoder's embedding does not change by a bit."""
    import avtex.fused_slowfast as fsf
    from avtex import ops
    from avtex.fused_slowfast import Act, FusedConv, new_act, split_planes

    pd = X3[mode]
    torch.manual_seed(9)
    c = nn.Conv3d(64, 256, 1, bias=False)
    a2 = nn.Conv3d(256, 64, 1, bias=False)
    bnc, bna = nn.BatchNorm3d(256).eval(), nn.BatchNorm3d(64).eval()
    with torch.no_grad():
        for bn in (bnc, bna):
            bn.weight.uniform_(0.5, 1.5); bn.bias.uniform_(-0.5, 0.5)
            bn.running_mean.uniform_(-0.2, 0.2); bn.running_var.uniform_(0.5, 1.5)
    fc, fa = FusedConv(c, bnc, True, dev, x3=pd), FusedConv(a2, bna, True, dev, x3=pd)
    assert fc.pw is not None and fa.pw is not None and ops.pw_chain_x3_supported(64, 256, 64)
    dims = (2, 3, 9, 11)  # 594 rows: a ragged last 16-row tile
    m = dims[0] * dims[1] * dims[2] * dims[3]
    xh, xl = _planes(torch.randn(m, 64), pd, dev)
    rh, rl = _planes(torch.randn(m, 256), pd, dev)
    x, res = Act(xh, dims, lo=xl), Act(rh, dims, lo=rl)
    y_ref = fc(x, res=res, relu=True)
    z_ref = fa(y_ref)
    y, z = new_act(m, 256, dims, dev, True), new_act(m, 64, dims, dev, True)
    ops.pw_chain_x3(x.ptrs, x.ld, 64, fc.pw, fc.bias, fc.wscale, res.ptrs, res.ld, y.ptrs, y.ld, 256, True, fa.pw, fa.bias, fa.wscale,
                    z.ptrs, z.ld, 64, m, pd)
    torch.cuda.synchronize()
    for got, want in ((y, y_ref), (z, z_ref)):
        assert torch.equal(got.buf, want.buf) and torch.equal(got.lo, want.lo)
    # the encoder with and without the chained pass
    from avtex.slowfast import SlowFast
    torch.manual_seed(1)
    net = SlowFast().eval()
    sx = ops.SplitClip(*split_planes(torch.randn(1, 8, 224, 224, 4, device=dev), pd), pd)
    fx = ops.SplitClip(*split_planes(torch.randn(1, 32, 224, 224, 4, device=dev), pd), pd)
    outs = []
    for flag in (1, 0):
        keep, fsf._CHAIN_X3 = fsf._CHAIN_X3, flag
        try:
            outs.append(fsf.SlowFastMFMA(net, dev, precision=mode).forward_ndhwc4(sx, fx).clone())
        finally:
            fsf._CHAIN_X3 = keep
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("dims,sliced", [((2, 2, 6, 12), False), ((1, 3, 5, 12), True), ((3, 1, 9, 56), False), ((1, 2, 56, 56), True),
                                         ((5, 8, 56, 56), False)])
def test_res2_x3_fused_block_equals_the_three_launches(avt, dev, dims, sliced):
    """csrc/res2_x3.hip (round 6): a slow-res2 identity bottleneck (256 -> 64 -> [1,3,3] 64 -> 256, + x, ReLU) as ONE launch against the
    launches it replaces (pw_x3 a, conv33_x3 b, pw_x3 c + residual).  Phase B is conv33_x3's arithmetic in conv33_x3's order; phases A
    and C run 32 x 32 x 16 MFMAs where pw_x3 runs 16 x 16 x 32, so the fp32 accumulation order inside a product differs: equal to fp32
    rounding (2^-22 products, a few 1e-7 relative), not bit for bit.  Covers: several 256-position steps and workgroups, ragged last
    step, frame borders inside a step (zero padding in every direction), rows as channel slices of wider buffers (the lateral
    fusion's concatenation on the output side), width 12 (test shape) and 56 (production)."""
    import avtex.fused_slowfast as fsf
    from avtex import ops
    from avtex.fused_slowfast import Act, new_act
    from avtex.slowfast import ResBlock

    pd = ops.X3_F16
    torch.manual_seed(17)
    blk = ResBlock(256, 256, 64, 1, 1).eval()
    with torch.no_grad():
        for bn in (blk.branch2.a_bn, blk.branch2.b_bn, blk.branch2.c_bn):
            bn.weight.uniform_(0.5, 1.5); bn.bias.uniform_(-0.5, 0.5)
            bn.running_mean.uniform_(-0.2, 0.2); bn.running_var.uniform_(0.5, 1.5)
    keep, fsf._RES2_X3 = fsf._RES2_X3, 1
    try:
        fused = fsf._BlockX3(blk, dev, pd)
        fsf._RES2_X3 = 0
        plain = fsf._BlockX3(blk, dev, pd)
    finally:
        fsf._RES2_X3 = keep
    assert fused.res2 is not None and plain.res2 is None
    m = dims[0] * dims[1] * dims[2] * dims[3]
    ldi = 320 if sliced else 256
    xf = torch.randn(m, ldi) * 1.5 + 0.2
    xh, xl = _planes(xf, pd, dev)
    x = Act(xh, dims, 32 if sliced else 0, 256, lo=xl)
    out = None
    if sliced:  # the output as the first 256 channels of a 320-wide concatenation buffer, pre-filled to catch stray stores
        ob = new_act(m, 320, dims, dev, True)
        ob.buf.fill_(7.0); ob.lo.fill_(7.0)
        out = Act(ob.buf, dims, 0, 256, lo=ob.lo)
    y = fused(x, out=out)
    y_ref = plain(x)
    torch.cuda.synchronize()
    got, want = y.float(pd), y_ref.float(pd)
    # also against the fp32 module itself (NCDHW)
    with torch.no_grad():
        xt = x.float(pd).cpu().view(*dims, 256).permute(0, 4, 1, 2, 3).contiguous()
        ref32 = blk(xt).permute(0, 2, 3, 4, 1).reshape(m, 256)
    scale = float(want.abs().max())
    assert float((got - want).abs().max()) <= 3e-6 * scale, float((got - want).abs().max()) / scale
    assert float((got.cpu() - ref32).abs().max()) <= 2e-5 * scale
    assert float((want.cpu() - ref32).abs().max()) <= 2e-5 * scale
    if sliced:
        assert bool((ob.buf[:, 256:].float() == 7.0).all()) and bool((ob.lo[:, 256:].float() == 7.0).all())


def test_res2_x3_in_the_encoder(avt, dev):
    """The whole contract-grade encoder with the slow res2 identity blocks fused (round 6) and as three launches: embeddings equal to
    fp32 rounding of the two blocks (the fused phases A / C accumulate in another MFMA shape's order)."""
    import avtex.fused_slowfast as fsf
    from avtex import ops
    from avtex.fused_slowfast import split_planes
    from avtex.slowfast import SlowFast

    pd = ops.X3_F16
    torch.manual_seed(1)
    net = synth_randomised(SlowFast().eval())
    sx = ops.SplitClip(*split_planes(torch.randn(2, 8, 224, 224, 4, device=dev), pd), pd)
    fx = ops.SplitClip(*split_planes(torch.randn(2, 32, 224, 224, 4, device=dev), pd), pd)
    outs, launches = [], []
    for flag in (1, 0):
        keep, fsf._RES2_X3 = fsf._RES2_X3, flag
        names = []
        fsf.PROFILER = lambda name, launch, fl, nb: (names.append(name), launch())
        try:
            outs.append(fsf.SlowFastMFMA(net, dev, precision="f16x3").forward_ndhwc4(sx, fx).clone())
        finally:
            fsf._RES2_X3, fsf.PROFILER = keep, None
        launches.append(names)
    assert launches[0].count("res2_x3_kernel") == 2 and "res2_x3_kernel" not in launches[1]
    assert "pw_chain_x3_kernel" not in launches[0] and launches[1].count("pw_chain_x3_kernel") == 1
    rel = float(((outs[0] - outs[1]).norm(dim=1) / outs[1].norm(dim=1)).max())
    assert rel < 2e-6, rel


def synth_randomised(net):
    from avtex import synth

    return synth.randomise_bn(net, 3, 0.5)


@pytest.mark.parametrize("mode,W,S", [("bf16x3", 20, 4), ("f16x3", 20, 4), ("f16x3", 15, 6), ("f16x3", 33, 5)])
def test_frame_table_equals_dense_clips(avt, dev, mode, W, S):
    """ops.clip_pack_frames (every distinct frame packed once + the windows' sampling index, read by the stem kernel through
    avt_stem_conv_x3's frame_idx) against dense per-window clips (ops.clip_pack): the table's rows equal the dense clips' frames
    bit for bit, and the encoder's embeddings are identical — W = 20, S = 4 windows (the fast pathway repeats frames, windows
    overlap by 16 of 20), ragged window starts, and the explicit-gather fallback for a shape the table kernel does not cover."""
    import avtex.fused_slowfast as fsf
    import avtex.texture as texture
    from avtex import ops, synth
    from avtex.slowfast import SlowFast

    # (W = 15, S = 6: what main.py derives from 30 fps, more repeats; W = 33: no repeated frame, nothing to merge)
    video = synth.structured_video(3, 100, 48, 56).to(dev)
    starts = np.array([0, S, 2 * S, 3 * S, 21, 33, 60], dtype=np.int64)
    slow_d, fast_d = ops.clip_pack(video, starts, W, out_hw=224, layout="ndhwc4", planes=mode)
    slow_t, fast_t = ops.clip_pack_frames(video, starts, W, out_hw=224, planes=mode)
    assert slow_t.shape == tuple(slow_d.shape) and fast_t.shape == tuple(fast_d.shape) and slow_t.table_frames == 100
    for dense, tab in ((slow_d, slow_t), (fast_d, fast_t)):
        g = tab.dense()
        assert torch.equal(g.hi, dense.hi) and torch.equal(g.lo, dense.lo)
    torch.manual_seed(0)
    enc = fsf.SlowFastMFMA(synth.randomise_bn(SlowFast().eval(), 3, 0.5), dev, precision=mode)
    e_dense = enc.forward_ndhwc4(slow_d, fast_d)
    keep, fsf._STEM_MERGE = fsf._STEM_MERGE, 0
    e_table = enc.forward_ndhwc4(slow_t, fast_t)
    fsf._STEM_MERGE = keep
    assert torch.equal(e_dense, e_table)  # the table is only another way to address the same frames
    # ... with the fast stem's taps of one source frame merged (5 weight slabs per output-frame group instead of 8 at W = 20):
    # the same function, the summed weights rounded once more (2^-22 / 2^-16 relative per product)
    e_merged = enc.forward_ndhwc4(slow_t, fast_t)
    rel = float(((e_merged - e_dense).norm(dim=1) / e_dense.norm(dim=1)).max())
    assert rel < (2e-6 if mode == "f16x3" else 1e-4) and (rel > 0) == (W < 32), rel
    f_d = enc._stem_x3(enc.stem_f, fast_d)[0].float(X3[mode])
    f_m = enc._stem_x3(enc.stem_f, fast_t)[0].float(X3[mode])
    assert float((f_m - f_d).abs().max()) < (2e-6 if mode == "f16x3" else 1e-4) * float(f_d.abs().max())
    # ... and through the engine (texture.FRAME_TABLE on / off), batches of 3 windows
    from avtex.texture import TextureEngine

    outs = []
    for flag in (True, False):
        keep, texture.FRAME_TABLE = texture.FRAME_TABLE, flag
        eng = TextureEngine(enc, enc, None, window=W, stride=S, temp=0.1, img_size=224, model_type=1, device=dev, enc_batch=3)
        eng.set_video(video)
        outs.append(eng.embed_windows([enc], starts=starts)[0].clone())
        texture.FRAME_TABLE = keep
    assert float((outs[0] - outs[1]).abs().max()) < 1e-4 * float(outs[1].abs().max()) and torch.equal(outs[1], e_dense)


@pytest.mark.parametrize("mode", ["bf16x3", "f16x3"])
@pytest.mark.parametrize("cin,cout,dims", [(32, 64, (2, 32, 9, 7)), (8, 16, (1, 32, 12, 12)), (64, 128, (2, 13, 5, 6))])
def test_lateral_x3_streaming_form_equals_the_general_tile(avt, dev, mode, cin, cout, dims):
    """avt_lateral_x3 (Conv3d [7,1,1] stride 4 + bias + ReLU as one streaming pass with a gathered operand: SlowFast's lateral
    connections) against the same FusedConv on the general split-plane tile and against torch's fp32 convolution: clip ends
    (temporal zero padding), a frame count that is not a multiple of the stride, a 16-channel output (half a tile pair), writes
    into a channel slice of a wider buffer."""
    import avtex.fused_slowfast as fsf
    from avtex.fused_slowfast import Act, new_act

    pd = X3[mode]
    torch.manual_seed(cin + cout)
    conv = nn.Conv3d(cin, cout, (7, 1, 1), stride=(4, 1, 1), padding=(3, 0, 0), bias=False)
    bn = nn.BatchNorm3d(cout).eval()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5); bn.bias.uniform_(-0.3, 0.3); bn.running_mean.uniform_(-0.2, 0.2); bn.running_var.uniform_(0.5, 1.5)
    b, t, h, w = dims
    x = torch.randn(b, cin, t, h, w)
    with torch.no_grad():
        ref = torch.relu(bn(conv(x)))  # [b, cout, to, h, w]
    want = ref.permute(0, 2, 3, 4, 1).reshape(-1, cout)
    xa = new_act(b * t * h * w, cin, dims, dev, True)
    hi, lo = fsf.split_planes(x.permute(0, 2, 3, 4, 1).reshape(-1, cin).to(dev), pd)
    xa.buf.copy_(hi); xa.lo.copy_(lo)
    outs = {}
    for flag in ("all", set()):
        keep, fsf._LATERAL_X3 = fsf._LATERAL_X3, flag
        fc = fsf.FusedConv(conv, bn, True, dev, x3=pd)
        fsf._LATERAL_X3 = keep
        assert (fc.lat is not None) == (flag == "all")
        od = fc.out_dims(dims)
        wide = new_act(od[0] * od[1] * od[2] * od[3], cout + 24, od, dev, True)
        wide.buf.zero_(); wide.lo.zero_()
        fc(xa, out=Act(wide.buf, od, 8, cout, lo=wide.lo))
        torch.cuda.synchronize()
        full = wide.float(pd).cpu()
        assert float(full[:, :8].abs().max()) == 0.0 and float(full[:, 8 + cout:].abs().max()) == 0.0  # nothing outside the slice
        outs[str(flag)] = full[:, 8 : 8 + cout]
    tol = (2e-6 if mode == "f16x3" else 1e-4) * float(want.abs().max())
    assert float((outs["all"] - want).abs().max()) < 4 * tol and float((outs["all"] - outs["set()"]).abs().max()) < 2 * tol
