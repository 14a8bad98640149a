"""The kaiser_best windowed-sinc resampler on the MI355X (csrc/resample.hip): the kernel against the scalar restatement
(tests/audio_resample_ref.py) bit for bit, the device chain waveform -> resample -> log-mel -> examples against the host's, and one
validate() run whose audio is loaded and resampled on the device against the same run fed the host-prepared waveforms."""
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_resample_ref as R  # noqa: E402
from tiny_encoders import TinySlowFast, seeded  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _n_in_for(n_out, sr_in, sr_out):
    """The shortest input whose resampling has n_out outputs."""
    n_in = int(n_out * sr_in / sr_out)
    while R.n_out_of(n_in, sr_in, sr_out) < n_out:
        n_in += 1
    assert R.n_out_of(n_in, sr_in, sr_out) == n_out
    return n_in


# n_out on both sides of one wave (64 lanes) and of one workgroup (ops.RESAMPLE_BLOCK = 256 outputs): the last lanes of a partial
# wave / block, a full one, the first lane of the next
_EDGES = [(_n_in_for(n_out, 44100, 16000), 44100, 16000) for n_out in (63, 64, 65, 255, 256, 257)]


def _run(avt, dev, x, sr_in, sr_out, out_dtype):
    """x: a device tensor -> ops.resample_sinc with the plan and the tables audio_frontend builds."""
    from avtex import audio_frontend as af

    p = af.sinc_plan(int(x.numel()), sr_in, sr_out)
    win, delta = torch.from_numpy(p["win"].copy()).to(dev), torch.from_numpy(p["delta"].copy()).to(dev)
    return avt.ops.resample_sinc(x, win, delta, p["num_table"], p["scale"], p["inc"], p["step"], p["n_out"], out_dtype)


def test_block_size_is_the_kernels(avt):
    src = open(os.path.join(os.path.dirname(avt._lib.LIB_PATH), "csrc", "resample.hip")).read()
    assert "constexpr int kThreads = %d;" % avt.ops.RESAMPLE_BLOCK in src and avt.ops.RESAMPLE_BLOCK == 256
    assert [R.n_out_of(*s) for s in _EDGES] == [63, 64, 65, 255, 256, 257]


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("n_in,sr_in,sr_out", R.SHAPES + _EDGES)
def test_kernel_equals_the_scalar_restatement(avt, dev, n_in, sr_in, sr_out, dtype):
    x, want = R.case(n_in, sr_in, sr_out, dtype)
    xd = torch.from_numpy(x.copy()).to(dev)
    y64 = _run(avt, dev, xd, sr_in, sr_out, torch.float64)
    assert y64.dtype == torch.float64 and tuple(y64.shape) == want.shape
    assert torch.equal(y64.cpu(), torch.from_numpy(want.copy()))
    y32 = _run(avt, dev, xd, sr_in, sr_out, torch.float32)  # the fp64 sum rounded once, to nearest even
    assert y32.dtype == torch.float32 and torch.equal(y32.cpu(), torch.from_numpy(want.astype(np.float32)))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_input_as_an_offset_view_of_its_storage(avt, dev, dtype):
    """x one element into its storage: a float32 waveform then starts 4 bytes off any wider alignment."""
    x, want = R.case(700, 44100, 16000, dtype)
    buf = torch.full((x.shape[0] + 1,), 7.0, dtype=getattr(torch, dtype), device=dev)
    buf[1:] = torch.from_numpy(x.copy()).to(dev)
    view = buf[1:]
    assert view.storage_offset() == 1 and view.is_contiguous()
    assert torch.equal(_run(avt, dev, view, 44100, 16000, torch.float64).cpu(), torch.from_numpy(want.copy()))
    assert torch.equal(_run(avt, dev, view, 44100, 16000, torch.float32).cpu(), torch.from_numpy(want.astype(np.float32)))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_silence_gives_zeros(avt, dev, dtype):
    for out_dtype in (torch.float64, torch.float32):
        y = _run(avt, dev, torch.zeros(700, dtype=dtype, device=dev), 44100, 16000, out_dtype)
        assert y.shape == (253,) and torch.equal(y, torch.zeros_like(y))


def test_wrapper_checks(avt, dev):
    from avtex import audio_frontend as af

    p = af.sinc_plan(100, 44100, 16000)
    win, delta = torch.from_numpy(p["win"].copy()).to(dev), torch.from_numpy(p["delta"].copy()).to(dev)
    x = torch.zeros(100, dtype=torch.float64, device=dev)
    args = (p["num_table"], p["scale"], p["inc"], p["step"], p["n_out"])
    with pytest.raises(avt._lib.AvtError):
        avt.ops.resample_sinc(x.cpu(), win, delta, *args)
    with pytest.raises(avt._lib.AvtError):
        avt.ops.resample_sinc(x.half(), win, delta, *args)
    with pytest.raises(avt._lib.AvtError):
        avt.ops.resample_sinc(x, win.float(), delta, *args)
    with pytest.raises(avt._lib.AvtError):
        avt.ops.resample_sinc(x, win, delta[:-1], *args)
    with pytest.raises(avt._lib.AvtError, match="lies past"):  # one output more than the input covers
        avt.ops.resample_sinc(x, win, delta, p["num_table"], p["scale"], p["inc"], p["step"], 38)
    assert avt.ops.resample_sinc(x, win, delta, *args).shape == (36,)


@functools.lru_cache(maxsize=None)
def _chain_case():
    """3 s of 0.3 * N(0, 1) at 44.1 kHz and what the host makes of it; computed once, not to be written to."""
    from avtex import audio_frontend as af

    x = R.wave(3 * 44100, np.float64, seed=11)
    y16 = af.resample_sinc(x, 44100, 16000)
    lm = af.log_mel_spectrogram(y16, 16000)
    y22 = af.resample_sinc(x, 44100, 22050).astype(np.float32)
    for a in (x, y16, lm, y22):
        a.setflags(write=False)
    return x, y16, lm, y22


def test_device_chain_matches_the_host_chain(avt, dev):
    from avtex import audio_frontend as af

    x, y16, lm_host, _ = _chain_case()
    y = af.resample_sinc_device(x, 44100, 16000, dev)
    assert y.dtype == torch.float64 and torch.equal(y.cpu(), torch.from_numpy(y16.copy()))
    tables = dict(af._SINC_DEVICE)
    assert len(tables) >= 1
    af.resample_sinc_device(x[:1000], 44100, 16000, dev)
    assert len(af._SINC_DEVICE) == len(tables) and all(af._SINC_DEVICE[k][0] is v[0] for k, v in tables.items())  # resident: one upload
    lm = af.log_mel_device(x, 44100, dev, resampler="kaiser_best")
    assert lm.dtype == torch.float64 and tuple(lm.shape) == lm_host.shape == (298, 64)
    err = np.abs(lm.cpu().numpy() - lm_host).max()
    print("max |device log-mel - host log-mel| = %.3e" % err)
    assert err <= 1e-10  # the bound tests/test_gpu_audio.py holds the log-mel kernel to
    ex = af.waveform_to_examples_device(x, 44100, dev, resampler="kaiser_best")
    want = af.frame(lm_host, 100, 10).astype(np.float32)
    assert ex.dtype == torch.float32 and tuple(ex.shape) == want.shape == (20, 100, 64)
    err32 = np.abs(ex.cpu().numpy().astype(np.float64) - want.astype(np.float64)).max()
    print("max |device examples - host examples| = %.3e (2^-20 = %.3e)" % (err32, 2.0 ** -20))
    assert err32 <= 2.0 ** -20  # one fp32 ulp below magnitude 8
    # the same waveform handed over as a device tensor: nothing goes through the host
    assert torch.equal(af.log_mel_device(torch.from_numpy(x.copy()).to(dev), 44100, dev, resampler="kaiser_best"), lm)
    # the default is today's chain: scipy's polyphase resampler on the host, then the same kernels
    lm0 = af.log_mel_device(x, 44100, dev)
    assert torch.equal(lm0, af.log_mel_device(af._resample(x, 44100, 16000), 16000, dev))
    assert (lm0 - lm).abs().max() > 1e-3


def test_load_audio_on_the_device(avt, dev):
    from avtex.validate import load_audio

    x, _, _, y22 = _chain_case()
    w, sr = load_audio((x, 44100), load_sr=22050, resampler="kaiser_best", device=dev)
    assert sr == 22050 and torch.is_tensor(w) and w.is_cuda and w.dtype == torch.float32
    assert torch.equal(w.cpu(), torch.from_numpy(y22.copy()))
    w32, _ = load_audio((x.astype(np.float32), 44100), load_sr=22050, resampler="kaiser_best", device=dev)
    from avtex import audio_frontend as af

    assert torch.equal(w32.cpu(), torch.from_numpy(af.resample_sinc(x.astype(np.float32), 44100, 22050).astype(np.float32)))
    same, sr0 = load_audio((x, 44100), device=dev)
    assert same is x and sr0 == 44100


def test_dataset_device_path_builds_its_examples_on_the_device(avt, dev):
    """AudioVideoSegments with --train_input device and kaiser_best: waveform and examples stay in HBM; the host path's values."""
    video = (torch.zeros((40, 8, 8, 3), dtype=torch.uint8), 20.0)
    x = R.wave(int(2.2 * 44100), np.float32, seed=7)
    kw = dict(vdata="/tmp", adata=None, n_negs=2, img_size=8, enc_arch="slowfast", window=0, stride=0,
              audio_resample="kaiser_best", audio_load_sr=22050)
    host = avt.AudioVideoSegments(SimpleNamespace(**kw), "x", split="train", video=video, audio=(x, 44100))
    ds = avt.AudioVideoSegments(SimpleNamespace(train_input="device", **kw), "x", split="train", video=video, audio=(x, 44100))
    assert ds.sr == 22050 and ds.apf == host.apf == 1102
    assert ds.audio_w.is_cuda and ds.audio_eg.is_cuda and not host.audio_eg.is_cuda
    assert torch.equal(ds.audio_w.cpu(), host.audio_w)
    assert ds.audio_eg.shape == host.audio_eg.shape and ds.audio_eg.dtype == torch.float32
    assert (ds.audio_eg.cpu().double() - host.audio_eg.double()).abs().max() <= 2.0 ** -20


def test_validate_loads_and_resamples_on_the_device(avt, dev, capsys):
    """-m 2 with driving audio on the tiny plugin encoders, 44.1 kHz source and driving waveforms, --audio_resample kaiser_best
    --audio_load_sr 22050: the Frames list of the run that loads on the device equals the run that is handed the host-prepared
    22 050 Hz float32 waveforms at rate 22 050 (and is at that rate already: its load step is the identity)."""
    from avtex import audio_frontend as af

    g = np.load(os.path.join(GOLD, "g5_validate_sf_da.npz"), allow_pickle=True)
    s = [int(v) for v in g["seeds"]]
    n_frames, W, S, mbs, G, hw, L, nvl, fps, _ = [int(v) for v in g["cfg"]]
    th, alpha, temp = [float(v) for v in g["th_alpha_temp"]]
    model = avt.ContrastivePredictionTemporal(seeded(TinySlowFast, s[0]), seeded(TinySlowFast, s[1]), seeded(avt.VGGish, s[2]), 2, 128,
                                              temp, W, S, th, mini_batchsize=mbs, enc_arch="slowfast", img_size=hw).to(dev).eval()
    args = SimpleNamespace(vdata=None, adata=None, dadata=None, subsample_rate=1, fps=fps, stride=S, window=W, enc_arch="slowfast",
                           img_size=hw, model_type=2, mini_batchsize=mbs, threshold=th, alpha=alpha, temp=temp, driving_audio=None,
                           da_feats="VGG", interpolation=False, new_video_length=nvl, results_folder=None, logname="exp",
                           batch_size=24, stitch_mode="compat", ref_num_gpus=G, enc_batch=16, audio_resample="kaiser_best",
                           audio_load_sr=22050)
    # 6.2 s of source audio for 6 s of video (the [: n_in * apf] cut applies, on a device tensor), 3 s of driving audio
    src = R.wave(int(6.2 * 44100), np.float32, seed=21)
    drv = R.wave(3 * 44100, np.float32, seed=22)

    def run(audio, driving):
        np.random.seed(1234)
        torch.manual_seed(4321)
        frames = avt.validate(model, args, video_name="gold", model_type=2, video=(g["video"], float(fps)), audio=audio,
                              driving_audio=driving)
        out = capsys.readouterr().out
        listed = [ln for ln in out.splitlines() if ln.startswith("Frames list: ")]
        assert len(listed) == 1
        return frames, listed[0]

    frames, listed = run((src, 44100), (drv, 44100))
    src22 = af.resample_sinc(src, 44100, 22050).astype(np.float32)
    drv22 = af.resample_sinc(drv, 44100, 22050).astype(np.float32)
    frames_host, listed_host = run((src22, 22050), (drv22, 22050))
    assert len(frames) > W and frames == frames_host and listed == listed_host
