"""The kaiser_best windowed-sinc resampler on the host: audio_frontend's vectorised NumPy against the scalar restatement
(tests/audio_resample_ref.py) bit for bit, against an analytic band-limited signal, and everything that must not have moved: both
options default off, the default chain is still scipy's polyphase resampler, and the new C entry has the documented signature."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_resample_ref as R  # noqa: E402


def test_filter_table(avt):
    from avtex import audio_frontend as af

    win, num_table = af.sinc_filter("kaiser_best")
    assert win.shape == (32769,) and win.dtype == np.float64 and num_table == 512
    assert win[0] == R.ROLLOFF == af.SINC_FILTERS["kaiser_best"]["rolloff"]  # sinc(0) and the window's centre are exactly 1
    assert np.array_equal(win, R.kaiser_best()[0])
    assert af.sinc_filter() is af.sinc_filter("kaiser_best")  # built once
    with pytest.raises(ValueError):
        af.sinc_filter("kaiser_fast")


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("n_in,sr_in,sr_out", R.SHAPES)
def test_host_resample_equals_the_scalar_restatement(avt, n_in, sr_in, sr_out, dtype):
    from avtex import audio_frontend as af

    x, want = R.case(n_in, sr_in, sr_out, dtype)
    got = af.resample_sinc(x, sr_in, sr_out)
    assert got.dtype == np.float64 and got.shape == (int(n_in * (float(sr_out) / sr_in)),) == want.shape
    assert np.array_equal(got, want)
    plan = af.sinc_plan(n_in, sr_in, sr_out)
    assert plan["n_out"] == want.shape[0] and plan["step"] == int(min(1.0, sr_out / sr_in) * 512)


def test_expected_output_counts():
    """What the issue's list says about its own shapes: three empty outputs, one output, 400 taps a wing."""
    assert [R.n_out_of(*s) for s in R.SHAPES[:4]] == [0, 0, 0, 1]
    assert (32769 - 0) // int(16000 / 96000 * 512) >= 385 and int(16000 / 96000 * 512) == 85
    inc = 1.0 / (16000.0 / 48000)
    assert all(float(t * inc).is_integer() for t in range(R.n_out_of(701, 48000, 16000)))  # tr is an integer at every output


def test_chunks_of_the_host_loop_join_exactly(avt, monkeypatch):
    """Ten minutes of audio are resampled a chunk of outputs at a time; the chunk size changes no bit."""
    from avtex import audio_frontend as af

    x, want = R.case(700, 44100, 16000, "float64")
    monkeypatch.setattr(af, "_SINC_CHUNK", 37)
    assert np.array_equal(af.resample_sinc(x, 44100, 16000), want)


def test_upsampling_interpolates_a_band_limited_signal(avt):
    """8 kHz -> 16 kHz of two sines below the 4 kHz Nyquist: away from the ends (400 outputs = 200 inputs > the filter's 64 zero
    crossings) the outputs are the analytic signal at the new instants.  1e-6 is far above the filter's own error (3.4e-8 measured
    with the prototype): the margin is for the reader, the check is that this is an interpolator and not merely self-consistent."""
    from avtex import audio_frontend as af

    def sig(t):
        return np.sin(2 * np.pi * 1000 * t) + 0.5 * np.sin(2 * np.pi * 3137 * t + 0.3)

    y = af.resample_sinc(sig(np.arange(8000) / 8000.0), 8000, 16000)
    assert y.shape == (16000,)
    err = np.abs(y - sig(np.arange(16000) / 16000.0))[400:-400].max()
    print("max |resampled - analytic| on outputs 400 .. n-400: %.3e" % err)
    assert err < 1e-6


def test_both_options_default_off(avt):
    import inspect

    from avtex import audio_frontend as af
    from avtex.main import build_parser
    from avtex.validate import load_audio

    args = build_parser().parse_args([])
    assert args.audio_resample == "scipy" and args.audio_load_sr == 0
    for fn in (af.waveform_to_examples, af.log_mel_device, af.waveform_to_examples_device):
        assert inspect.signature(fn).parameters["resampler"].default == "scipy"
    sig = inspect.signature(load_audio).parameters
    assert sig["load_sr"].default == 0 and sig["resampler"].default == "scipy" and sig["device"].default is None
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--audio_resample", "sinc"])
    got = build_parser().parse_args(["--audio_resample", "kaiser_best", "--audio_load_sr", "22050"])
    assert got.audio_resample == "kaiser_best" and got.audio_load_sr == 22050


def test_default_chain_is_still_the_polyphase_resampler(avt):
    from scipy.signal import resample_poly

    from avtex import audio_frontend as af

    x = R.wave(44100 + 4410, seed=5)
    want = af.frame(af.log_mel_spectrogram(resample_poly(x, 160, 441), 16000), 100, 10)
    got = af.waveform_to_examples(x, 44100)
    assert got.shape == want.shape == (1, 100, 64) and np.array_equal(got, want)
    assert np.array_equal(af.waveform_to_examples(x, 44100, resampler="scipy"), want)
    sinc = af.waveform_to_examples(x, 44100, resampler="kaiser_best")
    assert np.array_equal(sinc, af.frame(af.log_mel_spectrogram(af.resample_sinc(x, 44100, 16000), 16000), 100, 10))
    assert np.abs(sinc - want).max() > 1e-3  # the two resamplers differ by far more than rounding
    with pytest.raises(ValueError):
        af.waveform_to_examples(x, 44100, resampler="sinc")


def test_load_audio_on_the_host(avt):
    from avtex import audio_frontend as af
    from avtex.validate import load_audio

    x = R.wave(4410, np.float32, seed=6)
    w, sr = load_audio((x, 44100))
    assert w is x and sr == 44100  # load_sr = 0: the pair as read
    w, sr = load_audio((x, 44100), load_sr=44100, resampler="kaiser_best")
    assert w is x and sr == 44100  # already at the rate
    w, sr = load_audio((x, 44100), load_sr=22050, resampler="kaiser_best")
    assert sr == 22050 and w.dtype == np.float32 and np.array_equal(w, af.resample_sinc(x, 44100, 22050).astype(np.float32))
    stereo = np.stack([x, -0.5 * x], axis=1)
    w2, _ = load_audio((stereo, 44100), load_sr=22050, resampler="kaiser_best")
    assert np.array_equal(w2, af.resample_sinc(stereo.mean(axis=1), 44100, 22050).astype(np.float32))
    w3, sr3 = load_audio((x, 44100), load_sr=22050)  # the default resampler, to the asked rate
    assert sr3 == 22050 and w3.dtype == np.float32 and np.array_equal(w3, af._resample(x, 44100, 22050).astype(np.float32))


def test_dataset_host_path_honours_both_options(avt):
    """AudioVideoSegments without --train_input device: examples from the host chain at the loaded rate, apf from that rate."""
    from avtex import audio_frontend as af

    video = (torch.zeros((40, 8, 8, 3), dtype=torch.uint8), 20.0)
    x = R.wave(int(2.2 * 44100), np.float32, seed=7)
    args = SimpleNamespace(vdata="/tmp", adata=None, n_negs=2, img_size=8, enc_arch="slowfast", window=0, stride=0,
                           audio_resample="kaiser_best", audio_load_sr=22050)
    ds = avt.AudioVideoSegments(args, "x", split="train", video=video, audio=(x, 44100))
    assert ds.sr == 22050 and ds.apf == 1102
    w = af.resample_sinc(x, 44100, 22050).astype(np.float32)[: 40 * 1102]
    assert torch.equal(ds.audio_w, torch.from_numpy(w))
    want = af.frame(af.log_mel_spectrogram(af.resample_sinc(w, 22050, 16000), 16000), 100, 10)
    assert ds.audio_eg.dtype == torch.float32 and torch.equal(ds.audio_eg, torch.from_numpy(want).unsqueeze(1).float())
    plain = SimpleNamespace(vdata="/tmp", adata=None, n_negs=2, img_size=8, enc_arch="slowfast", window=0, stride=0)
    ds0 = avt.AudioVideoSegments(plain, "x", split="train", video=video, audio=(x, 44100))
    assert ds0.sr == 44100 and ds0.apf == 2205
    assert torch.equal(ds0.audio_eg, torch.from_numpy(af.waveform_to_examples(x[: 40 * 2205], 44100)).unsqueeze(1).float())


def test_header_declares_the_entry(avt):
    C = ctypes
    i, i64, d, vp = C.c_int, C.c_int64, C.c_double, C.c_void_p
    with open(avt._lib.HEADER_PATH) as f:
        text = f.read()
    table = avt._lib.parse_header(text)
    assert table["avt_resample_sinc_f64"] == (i, [vp, i, i64, vp, vp, i, i, d, d, i, vp, i, i64, vp])
    assert avt._lib.SIGNATURES["avt_resample_sinc_f64"] == table["avt_resample_sinc_f64"][1]
    assert avt._lib.abi_version(text) >= 10 and avt._lib.lib().avt_abi_version() == avt._lib.ABI_VERSION >= 10
    mk =open(os.path.join(os.path.dirname(avt._lib.LIB_PATH), "csrc", "Makefile")).read()
    assert " resample.hip" in mk


# one bad argument each; every check runs before the first HIP call and no pointer is ever dereferenced on the host
_OK = dict(x=0x10000, x_is_f64=1, n_in=100, win=0x20000, delta=0x30000, n_win=32769, num_table=512, scale=1.0, inc=1.0, step=512,
           y=0x40000, y_is_f64=1, n_out=100)
_BAD = [dict(x=None), dict(win=None), dict(delta=None), dict(y=None), dict(step=0), dict(n_win=0), dict(n_in=-1), dict(n_out=-1),
        dict(num_table=0), dict(scale=0.0), dict(scale=1.5), dict(inc=0.0), dict(inc=1.25), dict(n_win=512)]


# (with made-up addresses a check that went missing would be a real launch: never where a device is visible)
@pytest.mark.skipif(torch.cuda.is_available(), reason="made-up device addresses: only on a box without a GPU")
@pytest.mark.parametrize("bad", _BAD, ids=["-".join("%s=%s" % kv for kv in b.items()) for b in _BAD])
def test_bad_arguments_are_rejected_before_any_launch(avt, bad):
    a = dict(_OK, **bad)
    lib = avt._lib.lib()
    status = lib.avt_resample_sinc_f64(a["x"], a["x_is_f64"], a["n_in"], a["win"], a["delta"], a["n_win"], a["num_table"], a["scale"],
                                       a["inc"], a["step"], a["y"], a["y_is_f64"], a["n_out"], None)
    assert status == -1 and lib.avt_last_error().decode().startswith("avt_resample_sinc_f64: ")  # AVT_ERR_ARG


def test_no_outputs_launch_nothing(avt):
    """n_out == 0 returns before any pointer is looked at: NULL pointers are fine then, and no device is needed."""
    assert avt._lib.lib().avt_resample_sinc_f64(None, 0, 2, None, None, 32769, 512, 1.0, 1.0, 512, None, 1, 0, None) == 0
    with pytest.raises(avt._lib.AvtError):
        avt.ops.resample_sinc(torch.zeros(4), torch.zeros(8, dtype=torch.float64), torch.zeros(8, dtype=torch.float64), 512, 1.0, 1.0,
                              512, 4)  # CPU tensors are rejected, not emulated
