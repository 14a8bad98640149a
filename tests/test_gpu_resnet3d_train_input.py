"""The 3D-ResNet encoders' training input assembled on the device: the antialiased resize + normalise pass that builds the resident
frame table (csrc/frame_table.hip, avt_frames_resize_aa_norm_u8), the window gather over it (avt_clip_gather_frames_f32),
DeviceSegmentBatcher's non-SlowFast branch against the host dataset (dataset/dataset.py:44-58, 121-253), the batch in the model, and
the loader form train() iterates.

Resize bound: with r64 = the dataset's formula in float64 on the CPU, e_torch = max |dataset's fp32 tensor - r64| and e_hip =
max |kernel - r64|, the tests assert e_hip <= 2 e_torch + 2^-22 (the kernel may sum its taps in another order than ATen's separable
CPU passes, each order carrying rounding of the same size; 2^-22 is one ulp at the top of the value range, |x| <= 2.3).
Measured on an MI355X (e_torch / e_hip): see profiles/r10/README.md."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

MEAN, STD = [0.4345, 0.4051, 0.3775], [0.2768, 0.2713, 0.2737]


def _u8(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, tuple(shape) + (3,), generator=g, dtype=torch.uint8)


def _dataset_video(u8, hw, dtype=torch.float32):
    """AudioVideoSegments.__init__ for a non-SlowFast encoder (dataset.py:44-58 restated), in `dtype`."""
    mean = torch.tensor(MEAN).view(1, 3, 1, 1).to(dtype)
    std = torch.tensor(STD).view(1, 3, 1, 1).to(dtype)
    v = u8.permute(0, 3, 1, 2).to(dtype) / 255
    if v.shape[-1] != hw or v.shape[-2] != hw:
        v = F.interpolate(v, size=(hw, hw), mode="bilinear", antialias=True)
    return (v - mean) / std


def _bound_check(what, got, ref32, ref64):
    e_torch = float((ref32.double() - ref64).abs().max())
    e_hip = float((got.double() - ref64).abs().max())
    print("%s: e_torch %.3e, e_hip %.3e, bound %.3e" % (what, e_torch, e_hip, 2 * e_torch + 2.0 ** -22))
    assert e_hip <= 2 * e_torch + 2.0 ** -22, (what, e_hip, e_torch)


def _args(hw, n_negs, arch="resnet18"):
    return SimpleNamespace(vdata="/tmp", adata=None, n_negs=n_negs, img_size=hw, enc_arch=arch, window=0, stride=0)


def test_table_without_resize_is_the_datasets_bits(avt, dev):
    u8 = _u8((30, 32, 32), 1)
    torch.manual_seed(5)
    ds = avt.AudioVideoSegments(_args(32, 8), "x", split="train", video=(u8, 4.0))
    assert torch.equal(ds.video, _dataset_video(u8, 32))  # the helper of the filter cases is the dataset's own arithmetic
    table = avt.ops.frames_resize_aa_norm(u8.to(dev), 32)
    assert table.shape == (30, 3, 32, 32) and table.dtype == torch.float32
    assert torch.equal(table.cpu(), ds.video)


@pytest.mark.parametrize("shape,hw", [((6, 50, 70), 32),        # non-square, non-integer ratios 1.5625 and 2.1875
                                      ((6, 20, 24), 32),        # upscale
                                      ((6, 33, 31), 16),        # odd extents, borders where xmin / xmax clamp
                                      ((2, 1080, 1920), 224),   # 11 and 19 taps
                                      ((6, 64, 64), 30)])       # a size the gather tests use too
def test_table_resize_within_the_reference_error(avt, dev, shape, hw):
    u8 = _u8(shape, 2)
    got = avt.ops.frames_resize_aa_norm(u8.to(dev), hw).cpu()
    assert got.shape == (shape[0], 3, hw, hw)
    _bound_check("resize %s -> %d" % (shape, hw), got, _dataset_video(u8, hw), _dataset_video(u8, hw, torch.float64))


def test_table_resize_one_axis_only_and_wide_outputs(avt, dev):
    """H == hw but W != hw still filters both axes (the identity weights on y); an output wider than one 256-column tile."""
    for shape, hw in (((3, 32, 40), 32), ((2, 300, 700), 320)):
        u8 = _u8(shape, 3)
        got = avt.ops.frames_resize_aa_norm(u8.to(dev), hw).cpu()
        _bound_check("resize %s -> %d" % (shape, hw), got, _dataset_video(u8, hw), _dataset_video(u8, hw, torch.float64))


def test_resize_refuses_what_it_cannot_hold(avt, dev):
    with pytest.raises(avt._lib.AvtError):  # 37 taps x 256 lanes + a 3840-pixel row buffer: over the 64 KiB of include/avt.h
        avt.ops.frames_resize_aa_norm(torch.zeros((1, 8, 3840, 3), dtype=torch.uint8, device=dev), 224)


@pytest.mark.parametrize("src,hw,W", [((46, 64, 64), 30, 20), ((46, 64, 64), 30, 13), ((40, 33, 31), 15, 13), ((44, 32, 32), 32, 20)])
def test_gather_is_a_slice_of_the_table(avt, dev, src, hw, W):
    """hw = 15: 3 hw^2 = 675 floats, not a multiple of 4 — frames start at every alignment and the copy has a scalar tail."""
    table = avt.ops.frames_resize_aa_norm(_u8(src, 4).to(dev), hw)
    n_frames = src[0]
    last = n_frames - W
    starts = [0, last, 7, 7, 8, 9, last + 5]  # first, last valid, a repeat, two neighbours, one past the end
    out = avt.ops.clip_gather_frames(table, torch.tensor(starts, dtype=torch.int32, device=dev), W)
    assert out.shape == (len(starts), W, 3, hw, hw)
    for n, s in enumerate(starts[:-1]):
        assert torch.equal(out[n], table[s : s + W]), (n, s)
    want = torch.cat((table[last + 5 :], table[-1:].expand(5, -1, -1, -1)))  # the frames past the end are the clamped last frame
    assert torch.equal(out[-1], want)


def test_table_and_gather_past_2_31_elements(avt, dev):
    """14300 frames at 224^2 are 2.15e9 table elements; 720 windows of 20 frames are 2.17e9 output elements."""
    hw, W, n_frames, n_win = 224, 20, 14300, 720
    g = torch.Generator(device=dev).manual_seed(6)
    u8 = torch.randint(0, 256, (n_frames, hw, hw, 3), generator=g, dtype=torch.uint8, device=dev)
    table = avt.ops.frames_resize_aa_norm(u8, hw)
    assert table.numel() > 2 ** 31
    pick = [0, 14266, 14267, n_frames - 1]  # both sides of element 2^31
    assert torch.equal(table[pick].cpu(), _dataset_video(u8[pick].cpu(), hw))
    del u8
    starts = torch.arange(n_win, dtype=torch.int32) * 19
    starts[-1] = n_frames - W
    out = avt.ops.clip_gather_frames(table, starts.to(dev), W)
    assert out.numel() > 2 ** 31
    for n in (0, 712, 713, 714, n_win - 1):
        s = int(starts[n])
        assert torch.equal(out[n], table[s : s + W]), n


def _host_and_device_items(avt, dev, src_hw, hw, idxs, seed):
    from avtex import synth
    from avtex.dataset import DeviceSegmentBatcher

    torch.manual_seed(5)
    ds = avt.AudioVideoSegments(_args(hw, 9), "x", split="train", video=(synth.structured_video(3, 200, src_hw, src_hw), 40.0))
    assert ds.window == 20 and ds.stride == 8
    idxs = [i if i >= 0 else len(ds) + i for i in idxs]
    np.random.seed(seed)
    plans = [ds.segment_plan(i) for i in idxs]  # the window starts of the same draws
    np.random.seed(seed)
    items = [ds[i] for i in idxs]
    host_state = np.random.get_state()
    np.random.seed(seed)
    bat = DeviceSegmentBatcher(ds, dev).seed_from_numpy()
    qf, tf, qa, ta = bat.batch(torch.tensor(idxs))
    assert qf.shape == (len(idxs), 20, 3, hw, hw) and tf.shape == (len(idxs), 10, 20, 3, hw, hw) and qa is None and ta is None
    assert qf.is_contiguous() and tf.is_contiguous()
    np.random.seed(0)  # clobber, then take the device's state back
    bat.sync_to_numpy()
    got_state = np.random.get_state()
    assert np.array_equal(got_state[1], host_state[1]) and got_state[2] == host_state[2]
    return ds, plans, items, qf.cpu(), tf.cpu()


def test_batcher_equals_the_host_dataset(avt, dev):
    """The test that fails without the feature: the parent's DeviceSegmentBatcher raises ValueError for resnet18."""
    _, _, items, qf, tf = _host_and_device_items(avt, dev, 64, 64, [3, 10, -1], 11)
    for b, it in enumerate(items):
        assert torch.equal(qf[b], it[0]) and torch.equal(tf[b], it[3]), b


def test_batcher_with_a_resize_is_within_the_reference_error(avt, dev):
    ds, plans, items, qf, tf = _host_and_device_items(avt, dev, 48, 32, [3, 10, -1], 12)
    r64 = _dataset_video(ds.video_u8, 32, torch.float64)
    W = ds.window
    for b, (it, (q0, t0)) in enumerate(zip(items, plans)):
        q64 = r64[q0 : q0 + W]
        t64 = torch.stack([r64[int(s) : int(s) + W] for s in t0])
        _bound_check("item %d query" % b, qf[b], it[0], q64)
        _bound_check("item %d targets" % b, tf[b], it[3], t64)


def test_batcher_refuses_other_dtypes_for_the_table(avt, dev):
    from avtex import synth
    from avtex.dataset import DeviceSegmentBatcher

    torch.manual_seed(5)
    ds = avt.AudioVideoSegments(_args(32, 8), "x", split="train", video=(synth.structured_video(3, 120, 32, 32), 40.0))
    with pytest.raises(ValueError):
        DeviceSegmentBatcher(ds, dev, dtype=torch.bfloat16)


def test_batch_into_the_model(avt, dev):
    """resnet10 at 64^2, W = 20, one item, train mode in the training layout: equal input bits and a forward without atomics give
    equal logits whichever way the item reached the device; backward runs."""
    from avtex import resnet3d, synth, train_ops
    from avtex.dataset import DeviceSegmentBatcher

    hw, W = 64, 20
    torch.manual_seed(5)
    ds = avt.AudioVideoSegments(_args(hw, 9, "resnet10"), "x", split="train", video=(synth.structured_video(3, 200, 64, 64), 40.0))
    torch.manual_seed(0)
    base = avt.ContrastivePredictionTemporal(resnet3d.build("resnet10", hw, W), resnet3d.build("resnet10", hw, W), None, 1, 512,
                                             temp=0.1, window=W, stride=8, enc_arch="resnet10", img_size=hw)
    m = train_ops.training_layout(synth.randomise_bn(base, 4, 0.0).to(dev)).train()
    np.random.seed(3)
    it = ds[10]
    q_h, t_h = it[0].unsqueeze(0).to(dev), it[3].unsqueeze(0).to(dev)
    np.random.seed(3)
    q_d, t_d, _, _ = DeviceSegmentBatcher(ds, dev).seed_from_numpy().batch(torch.tensor([10]))
    assert torch.equal(q_d, q_h) and torch.equal(t_d, t_h)
    out_h = m(q_h, t_h).detach()
    out_d = m(q_d, t_d)
    assert out_d.shape == (1, 10) and torch.equal(out_d, out_h)
    avt.InfoNCECriterion()(out_d, torch.zeros(1, dtype=torch.long, device=dev)).backward()
    torch.cuda.synchronize()
    grads = [p.grad for n, p in m.named_parameters() if ".fc." not in n]
    assert all(g is not None and torch.isfinite(g).all() for g in grads)


def test_loader_epochs_and_one_train_epoch(avt, dev):
    from avtex import resnet3d, synth, train_ops
    from avtex.dataset import DeviceSegmentBatcher
    from avtex.train import train

    hw, W = 32, 20
    torch.manual_seed(5)
    ds = avt.AudioVideoSegments(_args(hw, 8, "resnet10"), "x", split="train", video=(synth.structured_video(3, 508, 32, 32), 40.0))
    assert len(ds) == 60
    bat = DeviceSegmentBatcher(ds, dev)
    assert len(bat.loader(7)) == 8 and len(bat.loader(7, drop_last=False)) == 9
    assert sum(1 for _ in bat.loader(7, drop_last=False)) == 9
    loader = bat.loader(2)
    assert len(loader) == 30
    audio = ds.audio_eg  # [61, 10] random rows: a query's row names its index
    orders = []
    for epoch in range(2):
        seen = []
        for batch_data in loader:
            q_frames, q_audio_wav, q_audio_eg, t_frames, t_audio_wav, t_audio_eg = batch_data  # as train() unpacks them
            assert q_audio_wav is None and t_audio_wav is None
            assert q_frames.shape == (2, W, 3, hw, hw) and t_frames.shape == (2, 9, W, 3, hw, hw)
            assert q_audio_eg.shape == (2, 10) and t_audio_eg.shape == (2, 9, 10) and q_audio_eg.is_cuda
            for b in range(2):
                idx = int((audio == q_audio_eg[b].cpu()).all(dim=1).nonzero()[0, 0])
                assert torch.equal(t_audio_eg[b, 0].cpu(), audio[idx + 1])
                assert torch.equal(q_frames[b], bat.table[idx * ds.stride : idx * ds.stride + W])
                seen.append(idx)
        assert sorted(seen) == list(range(60))
        orders.append(seen)
    assert orders[0] != orders[1]  # shuffled per epoch
    # SlowFast's branch through the same loader
    torch.manual_seed(5)
    sf = avt.AudioVideoSegments(_args(16, 8, "slowfast"), "x", split="train", video=(synth.structured_video(3, 120, 16, 16), 40.0))
    q_frames, _, q_ae, t_frames, _, t_ae = next(iter(DeviceSegmentBatcher(sf, dev).loader(3)))
    assert q_frames[0].shape == (3, 3, 8, 16, 16) and t_frames[1].shape == (3, 9, 3, 32, 16, 16) and t_ae.shape == (3, 9, 10)
    # one epoch of train() fed by the loader
    torch.manual_seed(0)
    model = avt.ContrastivePredictionTemporal(resnet3d.build("resnet10", hw, W), resnet3d.build("resnet10", hw, W), None, 1, 512,
                                              temp=0.1, window=W, stride=8, enc_arch="resnet10", img_size=hw)
    model = train_ops.training_layout(synth.randomise_bn(model, 4, 0.0).to(dev))
    opt = torch.optim.SGD(params=model.parameters(), lr=10e-3, momentum=0.9, weight_decay=0.0001)
    loss = train(bat.loader(10), model, opt, SimpleNamespace(print_freq=1000, log_freq=1000), 0, None)
    assert math.isfinite(loss)
