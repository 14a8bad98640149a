"""slowmo.Interpolator on frames whose extents are not multiples of 32: the resize to the networks' size and back runs on the device
(ops.resize_u8) and gives, byte for byte, what Pillow's resize around the same networks gives (interpolate.py:43, 137).  Pillow is
the oracle only: with `Image.resize` patched to raise, the product path still runs."""
import numpy as np
import pytest
import torch

import pil_resize_ref as ref
from interp_weights import frame_pair, unet_state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _oracle_resize(x, size, filt):
    """Pillow where it can be imported, else the restatement test_pil_resize_host.py holds equal to it"""
    try:
        import PIL  # noqa: F401
    except ImportError:
        return ref.resize(x, size, filt)
    return ref.pil_resize(x, size, filt)


def _forbid_pillow(monkeypatch):
    """Any Pillow resize from here on is an error (nothing to patch where Pillow is not installed)."""
    try:
        from PIL import Image
    except ImportError:
        return

    def refuse(*a, **k):
        raise AssertionError("the product resized a frame with Pillow")

    monkeypatch.setattr(Image.Image, "resize", refuse)


def _interpolator(h, w, sf):
    from avtex import slowmo
    it = slowmo.Interpolator(h, w, sf, DEV)
    it.flow_comp.load_state_dict(unet_state(6, 4, 31, head_gain=20.0))
    it.arb_time.load_state_dict(unet_state(20, 5, 32, head_gain=5.0))
    return it


def test_other_sizes_equal_pillow_around_the_same_networks(dev, monkeypatch):
    f0, f1 = frame_pair(9, 45, 70)
    # the chain: Pillow Lanczos of both frames on the host, the networks at 32 x 64 (unchanged code, deterministic), Pillow bilinear back
    small = [torch.from_numpy(_oracle_resize(f.numpy(), (32, 64), ref.LANCZOS)).to(DEV) for f in (f0, f1)]
    mid = _interpolator(32, 64, 3)(*small)
    torch.cuda.synchronize()
    exp = _oracle_resize(mid.cpu().numpy(), (45, 70), ref.BILINEAR)
    assert exp.shape == (2, 45, 70, 3)
    # the product, with Pillow's resize out of reach
    _forbid_pillow(monkeypatch)
    out = _interpolator(45, 70, 3)(f0.to(DEV), f1.to(DEV))
    torch.cuda.synchronize()
    assert out.dtype == torch.uint8 and tuple(out.shape) == (2, 45, 70, 3)
    assert np.array_equal(out.cpu().numpy(), exp)
    assert not np.array_equal(exp[0], exp[1])  # two different intermediate frames


def test_validate_interpolates_a_video_of_another_size(dev, tmp_path, capsys, monkeypatch):
    """`main.py -e` with interpolation on over a 72 x 100 video (networks at 64 x 96): the Frames list of the plain run, SF - 1 new frames
    per jump, no Pillow."""
    from types import SimpleNamespace

    _forbid_pillow(monkeypatch)
    import avtex as avt
    from avtex.slowfast import SlowFast
    torch.manual_seed(0)
    W, S, L = 20, 4, 14
    g = torch.Generator().manual_seed(3)
    video = torch.randint(0, 256, (L * S + W + 1, 72, 100, 3), generator=g, dtype=torch.uint8)
    q_mod, t_mod = SlowFast().eval(), SlowFast().eval()
    with torch.no_grad():
        for m in list(q_mod.modules()) + list(t_mod.modules()):
            if isinstance(m, torch.nn.BatchNorm3d):
                m.weight.uniform_(0.5, 1.0)
    model = avt.ContrastivePredictionTemporal(q_mod, t_mod, None, 1, 128, 0.1, W, S, 0.3, mini_batchsize=8,
                                              enc_arch="slowfast", img_size=224).to(DEV).eval()

    def run(interpolation, folder):
        args = SimpleNamespace(vdata=None, adata=None, dadata=None, subsample_rate=1, fps=4, stride=S, window=W,
                               enc_arch="slowfast", img_size=224, model_type=1, mini_batchsize=8, threshold=0.3, alpha=0.5,
                               temp=0.1, driving_audio=None, da_feats="VGG", interpolation=interpolation, new_video_length=12,
                               results_folder=folder, logname="exp", batch_size=24, stitch_mode="aligned", enc_batch=8,
                               enc_impl="mfma", enc_dtype="bf16", SF=5, slomo_ckpt="random")
        np.random.seed(7)
        return avt.validate(model, args, video_name="x", model_type=1, video=(video, 4.0))

    plain = run(False, None)
    capsys.readouterr()
    frames = run(True, str(tmp_path))
    out = capsys.readouterr().out
    assert frames == plain
    assert out.count("Added 4 intermediate frames.") >= 1 and "Saving Interpolated Video." in out
