"""The 3D-ResNet encoders (resnet10/18/34; the reference's default --enc_arch resnet18) on the contract-grade split-plane kernels
(fused_resnet3d.ResNet3dMFMA): the new 3D max-pool against torch, the whole encoder against the fp32 nn.Module, the engine's
frame-table path (at the production batch of 133 clips, and over a table above 4 GiB), and validate() dispatch end to end."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import cref, ref_py

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

X3 = {"bf16x3": 0, "f16x3": 1}
_CACHE = {}


def _planes(x, pd, dev):
    from avtex.fused_slowfast import split_planes

    hi, lo = split_planes(x, pd)
    return hi.to(dev), lo.to(dev)


def _joined(hi, lo, pd):
    dt = torch.float16 if pd == 1 else torch.bfloat16
    return hi.view(dt).float() + lo.view(dt).float()


@pytest.mark.parametrize("mode", ["bf16x3", "f16x3"])
@pytest.mark.parametrize("dims,c,ldi,ldo", [((2, 5, 7, 9), 16, 16, 16), ((1, 4, 8, 6), 8, 24, 16), ((3, 1, 1, 2), 64, 72, 64),
                                             ((1, 20, 56, 56), 64, 64, 64)])
def test_maxpool3d_k3s2_bit_equal_to_torch(avt, dev, mode, dims, c, ldi, ldo):
    """avt_maxpool3d_k3s2_ndhwc_x3 == F.max_pool3d(x, 3, 2, 1) on the fp32 values hi + lo, bit for bit; channel slices of wider rows
    (ldi > c: the channels beyond c are never read into the result, ldo > c: the columns beyond c are left alone); NaN propagates."""
    from avtex import ops

    pd = X3[mode]
    b, t, h, w = dims
    torch.manual_seed(3)
    x = torch.randn(b, t, h, w, ldi) * 4
    x[0, t // 2, h // 2, w // 2, 1] = float("nan")  # one poisoned activation
    x[..., c:] = 1e4  # outside the slice: must never win
    xh, xl = _planes(x.reshape(-1, ldi), pd, dev)
    to, ho, wo = (t - 1) // 2 + 1, (h - 1) // 2 + 1, (w - 1) // 2 + 1
    oh = torch.full((b * to * ho * wo, ldo), 7, dtype=torch.bfloat16, device=dev)
    ol = oh.clone()
    ops.maxpool3d_k3s2_x3((xh.data_ptr(), xl.data_ptr()), (oh.data_ptr(), ol.data_ptr()), b, t, h, w, c, ldi, ldo, pd)
    joined = _joined(xh, xl, pd).cpu().view(b, t, h, w, ldi)[..., :c]
    ref = F.max_pool3d(joined.permute(0, 4, 1, 2, 3), 3, 2, 1).permute(0, 2, 3, 4, 1).reshape(-1, c)
    got = _joined(oh, ol, pd).cpu()
    assert torch.equal(got[:, :c].isnan(), ref.isnan()) and ref.isnan().any()
    fin = ~ref.isnan()
    assert torch.equal(got[:, :c][fin], ref[fin])  # a max of representable values is representable: exact
    if ldo > c:
        assert (oh[:, c:] == 7).all() and (ol[:, c:] == 7).all()


def _calibrated(arch, hw, window, seed, clips):
    """A ResNet3d wrapped as the operator wraps it (models.py:253-260), BatchNorms randomised and then calibrated on `clips` (one
    train-mode forward with momentum 1: running statistics = the statistics of the actual activations)."""
    from avtex import resnet3d, synth

    torch.manual_seed(seed)
    net = synth.randomise_bn(resnet3d.build(arch, hw, window), seed + 100, 0.5)
    mod = nn.Sequential(net, nn.AdaptiveAvgPool3d((1, 1, 1))).to(clips.device)
    moms = {}
    for m in mod.modules():
        if isinstance(m, nn.BatchNorm3d):
            moms[m], m.momentum = m.momentum, 1.0
    mod.train()
    with torch.no_grad():
        mod(clips)
    for m, v in moms.items():
        m.momentum = v
    return mod.eval()


def _setup(dev, arch, hw, window, stride=4, n_win=12):
    """(video uint8, module engine, q / t fp32 modules): a structured video, the modules calibrated on its own clips."""
    key = (arch, hw, window, stride, n_win)
    if key not in _CACHE:
        from avtex import synth
        from avtex.texture import TextureEngine

        video = synth.structured_video(5, (n_win - 1) * stride + window + 1, hw, hw)
        probe = TextureEngine(nn.Identity(), nn.Identity(), None, window=window, stride=stride, img_size=hw, device=dev,
                              enc_arch=arch)
        probe.set_video(video)
        ids = np.arange(0, n_win, max(1, n_win // 6))[:, None] * stride + np.arange(window)[None, :]
        clips = probe._norm_pad.index_select(0, torch.from_numpy(ids.reshape(-1)).to(dev)).view(len(ids), window, 3, hw, hw)
        clips = clips.permute(0, 2, 1, 3, 4).contiguous()
        q = _calibrated(arch, hw, window, 10, clips)
        t = _calibrated(arch, hw, window, 11, clips)
        _CACHE[key] = (video, q, t)
    return _CACHE[key]


def _module_clips(eng, ids):
    """The module path's clips for frame-id windows (texture.TextureEngine's generic branch): _norm_pad gathered, -1 = zero frame."""
    flat = torch.from_numpy(np.where(ids < 0, eng.F, ids).reshape(-1)).to(eng.dev)
    x = eng._norm_pad.index_select(0, flat).view(len(ids), eng.W, 3, eng.hw, eng.hw)
    return x.permute(0, 2, 1, 3, 4).contiguous()


def _rel(y, ref):
    return ((y - ref).norm(dim=1) / ref.norm(dim=1)).max().item()


@pytest.mark.parametrize("arch,hw,window,mode", [
    ("resnet18", 224, 20, "f16x3"),   # the reference's default encoder at its default shape: the stem's patch-resident kernel
    ("resnet10", 224, 20, "f16x3"),
    ("resnet18", 224, 20, "bf16x3"),
    ("resnet18", 48, 8, "f16x3"),     # 24 pixel pairs: the stem on the general tile
    ("resnet10", 48, 8, "bf16x3"),
    ("resnet34", 48, 8, "f16x3"),
    ("resnet18", 64, 8, "f16x3"),     # 32 pixel pairs: the patch-resident stem at a small shape
])
def test_encoder_matches_fp32_module(avt, dev, arch, hw, window, mode):
    """ResNet3dMFMA vs the fp32 nn.Module (MIOpen) on the same clips: embeddings and the cosine scores of the contract."""
    from avtex.fused_resnet3d import ResNet3dMFMA
    from avtex.texture import TextureEngine

    video, q_mod, t_mod = _setup(dev, arch, hw, window)
    eng = TextureEngine(q_mod, t_mod, None, window=window, stride=4, img_size=hw, device=dev, enc_arch=arch)
    eng.set_video(video)
    ids = np.arange(4)[:, None] * 3 + np.arange(window)[None, :]
    x = _module_clips(eng, ids)
    qe, te = ResNet3dMFMA(q_mod, dev, mode), ResNet3dMFMA(t_mod, dev, mode)
    with torch.no_grad():
        q32, t32 = q_mod(x).flatten(1), t_mod(x).flatten(1)
    q, t = qe(x), te(x)
    assert q.shape == (4, 512) and q.dtype == torch.float32
    rel = max(_rel(q, q32), _rel(t, t32))
    s = F.normalize(q, dim=1) @ F.normalize(t, dim=1).T / 0.1
    s32 = F.normalize(q32, dim=1) @ F.normalize(t32, dim=1).T / 0.1
    ds = (s - s32).abs().max().item()
    msg = "%s %d^2 W=%d %s: rel embedding error %.3e, max |d score| %.3e (score spread %.3f)" % (
        arch, hw, window, mode, rel, ds, (s32.max() - s32.min()).item())
    print(msg)
    assert rel <= (1e-4 if mode == "f16x3" else 5e-4), msg
    assert ds <= 1e-3, msg


@pytest.mark.parametrize("hw,window", [(224, 20), (48, 8)])
def test_frame_table_embed_windows_equals_module(avt, dev, hw, window):
    """The engine's frame-table path (no clip gathered per window) == the module run on _norm_pad-gathered clips: window starts,
    and explicit frame ids with zero-padded (negative) entries, across an encoder batch boundary."""
    from avtex.fused_resnet3d import ResNet3dMFMA
    from avtex.texture import TextureEngine

    arch = "resnet18"
    video, q_mod, t_mod = _setup(dev, arch, hw, window)
    eng = TextureEngine(ResNet3dMFMA(q_mod, dev), ResNet3dMFMA(t_mod, dev), None, window=window, stride=4, img_size=hw,
                        device=dev, enc_batch=3, enc_arch=arch)
    assert eng.frame_table and eng.n_streams == 1 and eng.layout == "ndhwc4"
    n = eng.set_video(video)
    assert eng._table[0].shape == (eng.F + 1, hw, hw, 4)
    assert (_joined(*eng._table, 1)[..., 3] == 0).all()
    starts = np.arange(n)[:5] * 4
    ids = starts[:, None] + np.arange(window)[None, :]
    ids[1, -3:] = -1
    ids[3, :] = -1
    ids[4, ::2] = -1
    for kw, win in (({"starts": starts}, starts[:, None] + np.arange(window)[None, :]), ({"ids": ids}, ids)):
        q, t = eng.embed_windows([eng.q_enc, eng.t_enc], **kw)
        x = _module_clips(eng, win)
        with torch.no_grad():
            q32, t32 = q_mod(x).flatten(1), t_mod(x).flatten(1)
        rel = max(_rel(q, q32), _rel(t, t32))
        ds = (F.normalize(q, dim=1) @ F.normalize(t, dim=1).T - F.normalize(q32, dim=1) @ F.normalize(t32, dim=1).T).abs().max().item() / 0.1
        assert rel <= 1e-4 and ds <= 1e-3, "%s: rel %.3e, max |d score| %.3e" % (list(kw), rel, ds)


def _mod_compare(q, t, q32, t32):
    """(rel embedding error, max |d score|) of q / t against the fp32 module's q32 / t32."""
    rel = max(_rel(q, q32), _rel(t, t32))
    ds = (F.normalize(q, dim=1) @ F.normalize(t, dim=1).T - F.normalize(q32, dim=1) @ F.normalize(t32, dim=1).T).abs().max().item() / 0.1
    return rel, ds


@pytest.mark.parametrize("mode", ["f16x3", "bf16x3"])
def test_production_batch_embeds_like_module(avt, dev, mode):
    """The default encoder at its production batch: enc_batch 249 is cut to 133 clips at 224^2, W = 20, where layer3's 3x3x3
    convolutions run on the XL tile and the stem output is just under 2^31 - 64 elements.  140 windows (one full batch + a ragged
    batch of 7) against the fp32 module on a subset (clips 131 and 132 own the stem rows nearest 2^31), and the same subset
    re-embedded as one small batch (layer3 on the 128 x 128 tile) agrees with the full batch."""
    from avtex import ops
    from avtex.fused_resnet3d import ResNet3dMFMA
    from avtex.texture import TextureEngine
    from resnet3d_cases import TOL

    hw, W, S = 224, 20, 4
    video, q_mod, t_mod = _setup(dev, "resnet18", hw, W, S, 141)
    eng = TextureEngine(ResNet3dMFMA(q_mod, dev, mode), ResNet3dMFMA(t_mod, dev, mode), None, window=W, stride=S, img_size=hw,
                        device=dev, enc_batch=249, enc_arch="resnet18")
    assert eng.frame_table and eng.enc_batch == 133
    assert 133 * W * (hw // 2) ** 2 * 64 < (1 << 31) - 64 <= 134 * W * (hw // 2) ** 2 * 64
    plan = dict((n, e) for n, e, _ in eng.q_enc.plan(hw, W))
    for (c1, c2, _), name in zip(eng.q_enc.blocks[4:6], ("layer3.0", "layer3.1")):
        m1 = int(np.prod(plan[name]))
        for fc in (c1, c2):
            assert ops.conv3d_igemm_x3_xl_picked(fc.cout, fc.wt.shape[1], 133 * m1), name
            assert not ops.conv3d_igemm_x3_xl_picked(fc.cout, fc.wt.shape[1], 5 * m1), name
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    assert eng.set_video(video) == 140
    starts = np.arange(140) * S
    q, t = eng.embed_windows([eng.q_enc, eng.t_enc], starts=starts)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev)
    assert q.shape == (140, 512) and torch.isfinite(q).all() and torch.isfinite(t).all()
    sub = np.array([0, 66, 131, 132, 137])
    ids = starts[sub][:, None] + np.arange(W)[None, :]
    x = _module_clips(eng, ids)
    with torch.no_grad():
        q32, t32 = q_mod(x).flatten(1), t_mod(x).flatten(1)
    rel, ds = _mod_compare(q[sub], t[sub], q32, t32)
    q5, t5 = eng.embed_windows([eng.q_enc, eng.t_enc], ids=ids)
    d = max((q5 - q[sub]).abs().max().item(), (t5 - t[sub]).abs().max().item())
    scale = max(q[sub].abs().max().item(), t[sub].abs().max().item())
    msg = ("resnet18 224^2 W=20 %s batch 133: rel embedding error %.3e (bound %.0e), max |d score| %.3e (bound 1e-3); batch 133 vs "
           "batch 5 max |d| %.3e (bound %.3e = TOL x scale %.3f); peak device memory %.2f GB (%.2f GB above the %.2f GB before "
           "set_video)" % (mode, rel, 1e-4 if mode == "f16x3" else 5e-4, ds, d, TOL[mode] * scale, scale, peak / 1e9,
                           (peak - base) / 1e9, base / 1e9))
    print(msg)
    assert rel <= (1e-4 if mode == "f16x3" else 5e-4), msg
    assert ds <= 1e-3, msg
    assert d <= TOL[mode] * scale, msg


def test_frame_table_above_4gib(avt, dev):
    """A 10750-frame video at 224^2: the plane-pair frame table passes 2^32 - 64 bytes, so forward_frames hands the stem kernel
    only the frames a batch reads (torch.unique + remapped ids).  One batch mixing frames below and above the 2^32-byte mark and
    the zero frame == the fp32 module; the stem kernel itself refuses the whole table on the host."""
    from avtex import ops, synth
    from avtex._lib import AvtError
    from avtex.fused_resnet3d import ResNet3dMFMA
    from avtex.fused_slowfast import Act, new_act
    from avtex.texture import TextureEngine

    hw, W, S, n_frames = 224, 20, 4, 10750
    _, q_mod, t_mod = _setup(dev, "resnet18", hw, W, S, 141)
    frame_bytes = hw * (hw // 2) * 16  # one frame of one plane: 16-byte pixel pairs
    mark = -(-(1 << 32) // frame_bytes)  # the first frame that starts past byte 2^32 of a plane (10700)
    eng = TextureEngine(ResNet3dMFMA(q_mod, dev), ResNet3dMFMA(t_mod, dev), None, window=W, stride=S, img_size=hw, device=dev,
                        enc_batch=249, enc_arch="resnet18")
    video = synth.structured_video(9, n_frames, hw, hw, device=dev)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    eng.set_video(video)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev)
    assert eng._table[0].shape == (n_frames + 1, hw, hw, 4)
    assert (eng.F + 1) * frame_bytes >= (1 << 32) - 64 and eng.F > mark
    ids = np.stack([np.arange(W), np.arange(W) + mark - W // 2, np.arange(W) + n_frames - W, np.arange(W) + mark + 15])
    ids[3, ::3] = -1
    ids[3, 1] = 7
    assert (ids[1] < mark).any() and (ids[1] >= mark).any() and ids.max() == n_frames - 1
    q, t = eng.embed_windows([eng.q_enc, eng.t_enc], ids=ids)
    x = _module_clips(eng, ids)
    with torch.no_grad():
        q32, t32 = q_mod(x).flatten(1), t_mod(x).flatten(1)
    rel, ds = _mod_compare(q, t, q32, t32)
    msg = ("%d-frame table (%.2f GiB per plane): rel embedding error %.3e (bound 1e-4), max |d score| %.3e (bound 1e-3); set_video "
           "peak device memory %.2f GB (%.2f GB above the %.2f GB before)" % (n_frames + 1, (n_frames + 1) * frame_bytes / 2 ** 30,
                                                                            rel, ds, peak / 1e9, (peak - base) / 1e9, base / 1e9))
    print(msg)
    assert rel <= 1e-4 and ds <= 1e-3, msg
    # the whole table through the stem kernel: refused on the host (32-bit byte offsets), before any launch
    conv = eng.q_enc.stem
    tab = Act(eng._table[0].reshape(-1, 8), (1, W, hw, hw // 2), lo=eng._table[1].reshape(-1, 8))
    y = new_act(W * (hw // 2) ** 2, conv.cout, (1, W, hw // 2, hw // 2), dev, True)
    fidx = torch.arange(W, dtype=torch.int32, device=dev)
    with pytest.raises(AvtError, match="too large for 32-bit offsets"):
        ops.stem_conv_x3(tab.ptrs, conv.wt_lds, conv.wt_lds_lo, conv.bias, conv.wscale, y.ptrs, 1, W, hw, hw // 2, conv.cout,
                         conv.kernel[0], conv.stride[0], conv.pad[0], eng.q_enc.x3, relu=True, frame_idx=fidx,
                         table_frames=eng.F + 1)
    del eng, video, tab
    torch.cuda.empty_cache()


def _validate_args(hw, W, S, **kw):
    a = dict(vdata=None, adata=None, dadata=None, subsample_rate=1, fps=4, stride=S, window=W, enc_arch="resnet18", img_size=hw,
             model_type=1, mini_batchsize=8, threshold=0.3, alpha=0.5, temp=0.1, driving_audio=None, da_feats="VGG",
             interpolation=False, new_video_length=16, results_folder=None, logname="exp", batch_size=24, stitch_mode="aligned",
             enc_batch=8, enc_impl="mfma", enc_dtype="fp32")
    a.update(kw)
    return SimpleNamespace(**a)


def _model(avt, dev, q_mod, t_mod, W, S, hw, m=1):
    vgg = None
    if m == 2:
        torch.manual_seed(5)
        vgg = avt.VGGish()
    return avt.ContrastivePredictionTemporal(q_mod[0], t_mod[0], vgg, m, 512, 0.1, W, S, 0.3, mini_batchsize=8,
                                             enc_arch="resnet18", img_size=hw).to(dev).eval()


def test_validate_resnet18_mfma_matches_oracle_walk(avt, dev, capsys):
    """validate() with --enc_arch resnet18 --enc_impl mfma --enc_dtype fp32 runs the ResNet3d encoders on the contract-grade
    kernels, and its frames list equals the oracle's walk over tables built by the fp32 nn.Module encoders from the same frames."""
    from avtex.fused_resnet3d import ResNet3dMFMA
    from avtex.texture import TextureEngine

    hw, W, S, L = 64, 8, 4, 20
    video, q_mod, t_mod = _setup(dev, "resnet18", hw, W, S, L + 1)
    video = video[: L * S + W + 1]
    model = _model(avt, dev, q_mod, t_mod, W, S, hw)
    np.random.seed(7)
    frames = avt.validate(model, _validate_args(hw, W, S), video_name="x", model_type=1, video=(video, 4.0))
    out = capsys.readouterr().out
    assert "Encoders: ResNet3d on the MFMA kernels, precision f16x3 (contract grade)" in out
    assert isinstance(avt.validate.last_engine.q_enc, ResNet3dMFMA) and avt.validate.last_engine.frame_table
    # the reference's arithmetic: fp32 module encoders -> oracle normalise / similarity / select / walk
    ref_eng = TextureEngine(q_mod, t_mod, None, window=W, stride=S, img_size=hw, device=dev, enc_batch=8, enc_arch="resnet18")
    assert ref_eng.set_video(video) == L
    q32, t32 = ref_eng.build_tables()
    qn, _, _ = cref.l2norm_rows(q32.cpu().numpy(), want_split=False)
    tn, _, _ = cref.l2norm_rows(t32.cpu().numpy(), want_split=False)
    sim = cref.sim_f32(qn, tn, 0.1)
    assert sim.max() - sim.min() > 1.0  # non-degenerate scores

    def row_fn(q):
        o = cref.row_transition(sim[q : q + 1], q_ids=np.array([q]), n_seg=L, threshold=0.3, cap=L)
        return o["idx"][0, : o["cnt"][0]], ref_py.target_segment_ids(q, L)

    ref_frames, _, _ = ref_py.stitch_walk(row_fn, len(video), W, S, 64, q_id=10, rng=np.random.RandomState(7))
    assert frames == ref_frames


def test_validate_resnet_m2_runs_vggish_on_mfma(avt, dev, capsys):
    """m = 2 with ResNet encoders and --enc_impl mfma: VGGish moves to VGGishMFMA in the same precision."""
    from avtex.fused_resnet3d import ResNet3dMFMA
    from avtex.fused_vggish import VGGishMFMA

    hw, W, S, L = 48, 8, 4, 12
    video, q_mod, t_mod = _setup(dev, "resnet18", hw, W, S, L + 1)
    video = video[: L * S + W + 1]
    model = _model(avt, dev, q_mod, t_mod, W, S, hw, m=2)
    wave = (0.1 * np.random.RandomState(3).randn(int(16000 * len(video) / 4.0) + 16000)).astype(np.float32)
    np.random.seed(7)
    frames = avt.validate(model, _validate_args(hw, W, S, model_type=2, enc_dtype="bf16x3", new_video_length=8),
                          video_name="x", model_type=2, video=(video, 4.0), audio=(wave, 16000))
    out = capsys.readouterr().out
    eng = avt.validate.last_engine
    assert "Encoders: ResNet3d on the MFMA kernels, precision bf16x3 (contract grade)" in out and len(frames) >= 32
    assert isinstance(eng.q_enc, ResNet3dMFMA) and isinstance(eng.a_enc, VGGishMFMA) and eng.a_enc.precision == "bf16x3"


def test_validate_resnet_refusals_and_auto_default(avt, dev, capsys):
    """--enc_dtype bf16 with --enc_impl mfma and ResNet encoders is refused (the bf16 fast path is SlowFast's); --enc_impl auto keeps
    the nn.Module for ResNets."""
    hw, W, S, L = 48, 8, 4, 12
    video, q_mod, t_mod = _setup(dev, "resnet18", hw, W, S, L + 1)
    video = video[: L * S + W + 1]
    model = _model(avt, dev, q_mod, t_mod, W, S, hw)
    with pytest.raises(avt._lib.AvtError, match="SlowFast"):
        avt.validate(model, _validate_args(hw, W, S, enc_dtype="bf16"), video_name="x", model_type=1, video=(video, 4.0))
    capsys.readouterr()
    np.random.seed(7)
    avt.validate(model, _validate_args(hw, W, S, enc_impl="auto", new_video_length=8), video_name="x", model_type=1,
                 video=(video, 4.0))
    out = capsys.readouterr().out
    eng = avt.validate.last_engine
    assert "Encoders:" not in out and eng.q_enc is model.q_encoder and not eng.frame_table
