"""Contract-grade first blocks of slow res3 / res4 / res5 with the strided shortcut folded into c's GEMM (fused_slowfast._BlockX3.scat):
b ([1,3,3], stride 2) writes behind x's channels in x's own rows (2 ho, 2 wo), c and the shortcut are one stride-2 pointwise GEMM over
K = [x | b-output].  Checked against the four-launch form (_FUSE_SCAT_X3 = 0) and the fp32 nn.Module block, with the spare columns
pre-filled with NaN (a b row written to the wrong place, or not written, reaches the output); the fall-back to the four launches; NaN /
infinity propagation; and the launcher's frame ranges on input planes past 2^32 bytes (csrc/conv_x3.hip, igemm_x3_impl).

Which tiles run: the 256 x 256 tile takes a layer from 16 384 output rows (avt_conv3d_igemm_x3_xl_picked), so at the tiny extents the
merged GEMM and every b run on conv_x3_kernel<128,128,64>; the cases at 128 x 128 positions (16 384 output rows) put the merged GEMMs
of res3 / res4 and res4's 256 -> 256 b on the 256 x 256 tile with K-blocked weights, as the production batch does."""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

X3 = {"bf16x3": 0, "f16x3": 1}
# Block outputs against the fp32 module, relative to the output range: fp16 planes 2e-5 (the bound of
# test_gpu_x3.test_res2_x3_fused_block_equals_the_three_launches), bf16 planes 3 * 2e-5 (test_gpu_x3's `3 * TOL[mode]`, three layers
# deep).  The same bound holds between the two x3 forms.
BLOCK_TOL = {"bf16x3": 6e-5, "f16x3": 2e-5}
# (cin, c, cm, temporal taps of a) of the three first blocks
STAGES = {"res3": (320, 512, 128, 1), "res4": (640, 1024, 256, 3), "res5": (1280, 2048, 512, 3)}


def _first_block(stage):
    from avtex.slowfast import ResBlock

    cin, c, cm, kt = STAGES[stage]
    torch.manual_seed(11 * cin + c)
    blk = ResBlock(cin, c, cm, kt, 2).eval()
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, nn.BatchNorm3d):
                m.weight.uniform_(0.5, 1.5); m.bias.uniform_(-0.3, 0.3)
                m.running_mean.uniform_(-0.2, 0.2); m.running_var.uniform_(0.5, 1.5)
    return blk


def _build(blk, dev, pd, scat):
    import avtex.fused_slowfast as fsf

    keep, fsf._FUSE_SCAT_X3 = fsf._FUSE_SCAT_X3, scat
    try:
        return fsf._BlockX3(blk, dev, pd)
    finally:
        fsf._FUSE_SCAT_X3 = keep


def _wide_input(x, extra, dims, pd, dev):
    """x [m, C] fp32 -> Act over a [m, C + extra] plane pair, the spare columns NaN."""
    from avtex.fused_slowfast import Act, split_planes

    hi, lo = split_planes(x, pd)
    m, c = x.shape
    bh = torch.full((m, c + extra), float("nan"), dtype=torch.bfloat16)
    bl = torch.full((m, c + extra), float("nan"), dtype=torch.bfloat16)
    bh[:, :c], bl[:, :c] = hi, lo
    return Act(bh.to(dev), dims, 0, c, lo=bl.to(dev))


def _module_ref(blk, xa, pd, dims, cin):
    b, t, h, w = dims
    with torch.no_grad():
        xt = xa.float(pd).cpu().view(b, t, h, w, cin).permute(0, 4, 1, 2, 3).contiguous()
        y = blk(xt).permute(0, 2, 3, 4, 1)
    return y.reshape(-1, y.shape[-1])


@pytest.mark.parametrize("mode", ["f16x3", "bf16x3"])
@pytest.mark.parametrize("dims", [(2, 2, 8, 8), (2, 2, 6, 10)])
@pytest.mark.parametrize("stage", ["res3", "res4", "res5"])
def test_scat_x3_block_matches_the_four_launches_and_the_fp32_module(avt, dev, stage, dims, mode):
    pd = X3[mode]
    cin, c, cm, _ = STAGES[stage]
    blk = _first_block(stage)
    fused, plain = _build(blk, dev, pd, 1), _build(blk, dev, pd, 0)
    assert fused.scat is not None and fused.extra == cm and plain.scat is None and plain.extra == 0
    m = dims[0] * dims[1] * dims[2] * dims[3]
    torch.manual_seed(5)
    x = torch.randn((m, cin)) * 1.5
    xa = _wide_input(x, cm, dims, pd, dev)
    assert fused._scat_ok(xa)
    yf = fused(xa).float(pd).cpu()
    xb = _wide_input(x, cm, dims, pd, dev)
    yp = plain(xb).float(pd).cpu()
    assert bool(torch.isnan(xb.buf[:, cin:].float()).all())  # the four-launch form leaves the spare columns alone
    ref = _module_ref(blk, xb, pd, dims, cin)
    scale = float(ref.abs().max())
    err_f, err_p, err_fp = (float((yf - ref).abs().max()) / scale, float((yp - ref).abs().max()) / scale,
                            float((yf - yp).abs().max()) / scale)
    print("scat_x3 %s %s %s: fused %.2e, four launches %.2e of the output range from the fp32 module; fused - four launches %.2e"
          % (stage, dims, mode, err_f, err_p, err_fp))
    assert yf.shape == ref.shape and bool(torch.isfinite(yf).all())
    tol = BLOCK_TOL[mode]
    assert err_f < tol and err_p < tol, (err_f, err_p)
    assert err_fp < tol, err_fp


@pytest.mark.parametrize("stage,with_module", [("res3", True), ("res4", False)])
def test_scat_x3_block_on_the_256_tile(avt, dev, stage, with_module):
    """16 384 output rows: the merged GEMM (K = 448 / 896, K-blocked weights) and res4's b run on the 256 x 256 tile.  res4 is compared
    with the four launches only (its [3,1,1] a conv makes the fp32 module on the host cost more than the rest of this file)."""
    from avtex import ops

    pd = ops.X3_F16
    cin, c, cm, _ = STAGES[stage]
    dims = (1, 1, 256, 256) if stage == "res3" else (1, 4, 128, 128)
    blk = _first_block(stage)
    fused, plain = _build(blk, dev, pd, 1), _build(blk, dev, pd, 0)
    m = dims[0] * dims[1] * dims[2] * dims[3]
    assert fused.scat.wblk is not None and fused.scat.kernel_symbol(m // 4).startswith("conv_x3_xl_kernel")
    torch.manual_seed(6)
    x = torch.randn((m, cin)) * 1.5
    xa = _wide_input(x, cm, dims, pd, dev)
    yf = fused(xa).float(pd)
    xb = _wide_input(x, cm, dims, pd, dev)
    yp = plain(xb).float(pd)
    scale = float(yp.abs().max())
    err_fp = float((yf - yp).abs().max()) / scale
    print("scat_x3 %s %s on the 256 tile: fused - four launches %.2e of the output range" % (stage, dims, err_fp))
    assert bool(torch.isfinite(yf).all()) and err_fp < BLOCK_TOL["f16x3"], err_fp
    if with_module:
        ref = _module_ref(blk, xb, pd, dims, cin)
        err_f = float((yf.cpu() - ref).abs().max()) / float(ref.abs().max())
        print("    fused %.2e from the fp32 module" % err_f)
        assert err_f < BLOCK_TOL["f16x3"], err_f


@pytest.mark.parametrize("case", ["no_spare_columns", "odd_height", "odd_width"])
def test_scat_x3_falls_back_to_the_four_launches(avt, dev, case):
    """No spare columns behind x, or an odd H / W: the block built with the scat form runs the four launches, bit for bit."""
    from avtex import ops
    from avtex.fused_slowfast import Act, split_planes

    pd = ops.X3_F16
    cin, c, cm, _ = STAGES["res3"]
    dims = {"no_spare_columns": (1, 2, 8, 8), "odd_height": (1, 2, 7, 8), "odd_width": (1, 2, 8, 9)}[case]
    blk = _first_block("res3")
    fused, plain = _build(blk, dev, pd, 1), _build(blk, dev, pd, 0)
    m = dims[0] * dims[1] * dims[2] * dims[3]
    torch.manual_seed(7)
    x = torch.randn((m, cin)) * 1.5
    if case == "no_spare_columns":
        hi, lo = split_planes(x, pd)
        mk = lambda: Act(hi.to(dev), dims, lo=lo.to(dev))
    else:
        mk = lambda: _wide_input(x, cm, dims, pd, dev)
    xa = mk()
    assert fused.scat is not None and not fused._scat_ok(xa)
    yf, yp = fused(xa).float(pd), plain(mk()).float(pd)
    ref = _module_ref(blk, xa, pd, dims, cin)
    assert torch.equal(yf, yp)
    assert float((yf.cpu() - ref).abs().max()) < BLOCK_TOL["f16x3"] * float(ref.abs().max())


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_scat_x3_propagates_nan_and_inf(avt, dev, bad):
    """split2's contract through the fused form: a NaN in x is a NaN in every channel of its output position (it reaches all of them
    through the shortcut's columns of the merged GEMM), an infinity comes out non-finite; positions b's 3 x 3 window does not
    connect to it stay finite."""
    from avtex import ops

    pd = ops.X3_F16
    cin, c, cm, _ = STAGES["res3"]
    dims = (1, 2, 8, 8)
    blk = _first_block("res3")
    fused = _build(blk, dev, pd, 1)
    m = dims[0] * dims[1] * dims[2] * dims[3]
    torch.manual_seed(8)
    x = torch.randn((m, cin)) * 1.5
    x[(0 * 8 + 2) * 8 + 4, 7] = bad  # frame 0, row 2, column 4 -> output position (0, 1, 2)
    xa = _wide_input(x, cm, dims, pd, dev)
    assert fused._scat_ok(xa)
    y = fused(xa).float(pd).cpu().view(2, 4, 4, c)
    hit = y[0, 1, 2]
    assert bool(torch.isnan(hit).all()) if bad != bad else bool((~torch.isfinite(hit)).all()), hit[:8]
    assert bool(torch.isfinite(y[1]).all()) and bool(torch.isfinite(y[0, 3, 0]).all())


def test_x3_launcher_walks_frame_ranges_past_4_gib(avt, dev):
    """Slow res3's first block at the production batch: 448-column input rows, planes past 2^32 bytes.  The launcher walks the frames
    of a layer without temporal taps in ranges whose planes stay below the 32-bit limit; a layer with temporal taps over such a plane
    is rejected.  1536 frames of 56 x 56 x 448 (4.32 GB per plane, two launches of 768 frames): the pointwise a conv (general tile),
    the remapped-row b (general tile) and the strided merged GEMM (256 x 256 tile) run over the whole buffer, zeros everywhere but
    in the first frame, the frames on both sides of the range boundary, the frame that straddles byte 2^32 and the last frame;
    those frames are checked against the same layers on a small copy (b: bit for bit, the same tile) and in float64."""
    from avtex import ops
    from avtex._lib import AvtError
    from avtex.fused_slowfast import Act, FusedConv, new_act, split_planes

    pd, dt = ops.X3_F16, torch.float16
    cin, c, cm, _ = STAGES["res3"]
    ld, h, w, nf = cin + cm, 56, 56, 1536
    fr = h * w
    rows = nf * fr
    assert rows * ld * 2 > (1 << 32)
    need = 2 * rows * ld * 2 + 4 * rows * cm * 2 + 2 * (rows // 4) * c * 2 + (2 << 30)
    free = torch.cuda.mem_get_info(dev)[0]
    if free < need:
        pytest.skip("needs %.1f GB of device memory, %.1f GB free" % (need / 1e9, free / 1e9))
    straddle = (1 << 32) // (fr * ld * 2)
    frames = [0, nf // 2 - 1, nf // 2, straddle, nf - 1]
    assert straddle * fr * ld * 2 < (1 << 32) < (straddle + 1) * fr * ld * 2 and nf // 2 < straddle < nf - 1
    blk = _first_block("res3")
    t = blk.branch2
    a = FusedConv(t.a, t.a_bn, True, dev, x3=pd)
    b = FusedConv(t.b, t.b_bn, True, dev, x3=pd)
    scat = _build(blk, dev, pd, 1).scat
    dims = (nf // 8, 8, h, w)
    big = Act(torch.zeros((rows, ld), dtype=torch.bfloat16, device=dev), dims, 0, cin,
              lo=torch.zeros((rows, ld), dtype=torch.bfloat16, device=dev))
    sdims = (len(frames), 1, h, w)
    small = new_act(len(frames) * fr, ld, sdims, dev, True)
    small.buf.zero_(); small.lo.zero_()
    torch.manual_seed(9)
    xs = torch.randn((len(frames) * fr, cin), device=dev) * 1.5
    hi, lo = split_planes(xs, pd)
    small.buf[:, :cin], small.lo[:, :cin] = hi, lo
    for i, f in enumerate(frames):
        big.buf[f * fr:(f + 1) * fr, :cin] = hi[i * fr:(i + 1) * fr]
        big.lo[f * fr:(f + 1) * fr, :cin] = lo[i * fr:(i + 1) * fr]
    join = lambda act: act.buf.view(dt)[:, act.c0:act.c0 + act.C].double() + act.lo.view(dt)[:, act.c0:act.c0 + act.C].double()
    tol = 2e-6  # one layer on fp16 planes (test_gpu_x3.TOL)

    # a: pointwise 320 -> 128 over the 448-wide rows (input planes past 2^32: two frame ranges)
    ya = a(Act(big.buf, dims, 0, cin, lo=big.lo))
    ya_s = a(Act(small.buf, sdims, 0, cin, lo=small.lo))
    wa, ba = a._folded
    ref_a = torch.relu(join(Act(small.buf, sdims, 0, cin, lo=small.lo)) @ wa.view(cm, cin).double().t().to(dev) + ba.double().to(dev))
    sc = float(ref_a.abs().max())
    assert float((join(ya_s) - ref_a).abs().max()) < tol * sc
    for i, f in enumerate(frames):
        assert torch.equal(ya.buf[f * fr:(f + 1) * fr], ya_s.buf[i * fr:(i + 1) * fr]), ("a", f)
        assert torch.equal(ya.lo[f * fr:(f + 1) * fr], ya_s.lo[i * fr:(i + 1) * fr]), ("a", f)
    # b: [1,3,3] stride 2 into columns 320 .. 447 of the rows (2 ho, 2 wo) (output offsets past 2^32)
    b(ya, out=Act(big.buf, dims, cin, cm, lo=big.lo), out_rows=(2, h, w))
    b(ya_s, out=Act(small.buf, sdims, cin, cm, lo=small.lo), out_rows=(2, h, w))
    for i, f in enumerate(frames):
        assert torch.equal(big.buf[f * fr:(f + 1) * fr], small.buf[i * fr:(i + 1) * fr]), ("b", f)
        assert torch.equal(big.lo[f * fr:(f + 1) * fr], small.lo[i * fr:(i + 1) * fr]), ("b", f)
    got_b = small.buf.view(dt)[:, cin:].view(len(frames), h, w, cm)
    assert bool((got_b[:, 1::2] == 0).all()) and bool((got_b[:, :, 1::2] == 0).all()) and float(got_b[:, ::2, ::2].abs().max()) > 0
    # the merged GEMM: stride-2 pointwise over K = 448 (input planes past 2^32: two frame ranges on the 256 x 256 tile)
    y = scat(Act(big.buf, dims, 0, ld, lo=big.lo))
    assert scat.kernel_symbol(rows // 4).startswith("conv_x3_xl_kernel")
    wm, bm = scat._folded
    xin = join(Act(small.buf, sdims, 0, ld, lo=small.lo)).view(len(frames), h, w, ld)[:, ::2, ::2].reshape(-1, ld)
    ref = torch.relu(xin @ wm.view(c, ld).double().t().to(dev) + bm.double().to(dev))
    sc = float(ref.abs().max())
    fo = fr // 4
    for i, f in enumerate(frames):
        got = (y.buf[f * fo:(f + 1) * fo].view(dt).double() + y.lo[f * fo:(f + 1) * fo].view(dt).double())
        err = float((got - ref[i * fo:(i + 1) * fo]).abs().max()) / sc
        print("merged GEMM, frame %d: %.2e of the output range from float64" % (f, err))
        assert err < tol, (f, err)
    # a frame whose x is zero, between them (its b columns hold b(relu(a's bias))): from its own rows in float64
    zin = (big.buf[fr:2 * fr].view(dt).double() + big.lo[fr:2 * fr].view(dt).double()).view(h, w, ld)[::2, ::2].reshape(-1, ld)
    zref = torch.relu(zin @ wm.view(c, ld).double().t().to(dev) + bm.double().to(dev))
    z = y.buf[fo:2 * fo].view(dt).double() + y.lo[fo:2 * fo].view(dt).double()
    assert float((z - zref).abs().max()) < tol * sc
    # temporal taps over a plane past the limit: rejected, not addressed wrongly
    conv = nn.Conv3d(cin, cm, (3, 1, 1), padding=(1, 0, 0), bias=False)
    with pytest.raises(AvtError, match="too large for 32-bit offsets"):
        FusedConv(conv, None, True, dev, x3=pd)(Act(big.buf, dims, 0, cin, lo=big.lo), out=ya)
