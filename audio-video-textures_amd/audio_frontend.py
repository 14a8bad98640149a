"""Waveform -> VGGish log-mel examples, once per video.

`waveform_to_examples_device` is what validate() runs: the STFT / mel / log / framing arithmetic on the MI355X
(csrc/logmel.hip, float64 like the reference) from tables built here.  `waveform_to_examples` is the same arithmetic
in host NumPy for CPU-side callers (the training DataLoader's workers, dataset.py) where no device is bound.

Same arithmetic as the reference's TF-VGGish front-end
(contrastive_video_textures/utils/vggish_utils.py:27-69, mel_features.py:21-205,
vggish_params.py:27-38): 16 kHz mono, STFT 25 ms / 10 ms with a periodic Hann,
512-point FFT magnitude, 64 HTK-mel bands 125-7500 Hz, log(mel + 0.01), framed
into examples of 1.0 s (100 frames) at a hop of 0.1 s (10 frames) [quirk Q5:
the segment stride is 0.2 s, the audio hop 0.1 s].  Returns float64 like the
reference; callers cast to fp32 (validate.py:160-161).
"""
import numpy as np

SAMPLE_RATE = 16000
STFT_WINDOW_SECONDS = 0.025
STFT_HOP_SECONDS = 0.010
NUM_MEL_BINS = 64
MEL_MIN_HZ = 125.0
MEL_MAX_HZ = 7500.0
LOG_OFFSET = 0.01
EXAMPLE_WINDOW_SECONDS = 1.0
EXAMPLE_HOP_SECONDS = 0.1
_MEL_BREAK_HZ = 700.0
_MEL_Q = 1127.0


def frame(data, window_length, hop_length):
    """[n, ...] -> [num_frames, window_length, ...] strided view; incomplete tail dropped."""
    n = data.shape[0]
    num = 1 + int(np.floor((n - window_length) / hop_length))
    shape = (num, window_length) + data.shape[1:]
    strides = (data.strides[0] * hop_length,) + data.strides
    return np.lib.stride_tricks.as_strided(data, shape=shape, strides=strides)


def _hz_to_mel(hz):
    return _MEL_Q * np.log(1.0 + (hz / _MEL_BREAK_HZ))


def mel_matrix(num_mel_bins, num_spec_bins, sample_rate, lo_hz, hi_hz):
    nyq = sample_rate / 2.0
    if lo_hz < 0.0 or lo_hz >= hi_hz or hi_hz > nyq:
        raise ValueError("bad mel band edges %.1f..%.1f (nyquist %.1f)" % (lo_hz, hi_hz, nyq))
    spec_mel = _hz_to_mel(np.linspace(0.0, nyq, num_spec_bins))
    edges = np.linspace(_hz_to_mel(lo_hz), _hz_to_mel(hi_hz), num_mel_bins + 2)
    m = np.empty((num_spec_bins, num_mel_bins))
    for i in range(num_mel_bins):
        lo, ce, hi = edges[i : i + 3]
        up = (spec_mel - lo) / (ce - lo)
        down = (hi - spec_mel) / (hi - ce)
        m[:, i] = np.maximum(0.0, np.minimum(up, down))
    m[0, :] = 0.0  # HTK drops the DC bin
    return m


def log_mel_spectrogram(data, sample_rate=SAMPLE_RATE):
    win = int(round(sample_rate * STFT_WINDOW_SECONDS))
    hop = int(round(sample_rate * STFT_HOP_SECONDS))
    fft_len = 2 ** int(np.ceil(np.log(win) / np.log(2.0)))
    hann = 0.5 - (0.5 * np.cos(2 * np.pi / win * np.arange(win)))  # periodic
    spec = np.abs(np.fft.rfft(frame(data, win, hop) * hann, int(fft_len)))
    mel = np.dot(spec, mel_matrix(NUM_MEL_BINS, spec.shape[1], sample_rate, MEL_MIN_HZ, MEL_MAX_HZ))
    return np.log(mel + LOG_OFFSET)


def waveform_to_examples(data, sample_rate, resampler="scipy"):
    """-> float64 [num_examples, 100, 64].  resampler: how input at another rate is brought to 16 kHz — "scipy" (_resample) or
    "kaiser_best" (resample_sinc, the reference's filter)."""
    data = np.asarray(data)
    if data.ndim > 1:
        data = np.mean(data, axis=1)
    if sample_rate != SAMPLE_RATE:
        data = _resampler(resampler)(data, sample_rate, SAMPLE_RATE)
    log_mel = log_mel_spectrogram(data, SAMPLE_RATE)
    rate = 1.0 / STFT_HOP_SECONDS
    return frame(log_mel, int(round(EXAMPLE_WINDOW_SECONDS * rate)), int(round(EXAMPLE_HOP_SECONDS * rate)))


def _resample(data, sr_in, sr_out):
    """The default resampler ("scipy"): scipy's polyphase resampler, on the host.  The reference calls resampy's kaiser_best
    windowed sinc instead, and the two differ by far more than rounding (log-mel rows by up to 0.16 in the top band on noise at
    44.1 kHz): resampler="kaiser_best" (resample_sinc here, resample_sinc_device on the MI355X) computes the reference's."""
    from fractions import Fraction

    from scipy.signal import resample_poly

    fr = Fraction(int(sr_out), int(sr_in)).limit_denominator(1000)
    return resample_poly(data, fr.numerator, fr.denominator)


# ---- resampy 0.4's windowed-sinc resampler, filter "kaiser_best" ----------------------------------------------------------------
# Built from the published algorithm and the documented filter design (sinc_filter's arguments below), not from resampy's files:
# the interpolation table is recomputed here.  fp64 throughout; for float32 input resampy accumulates into a float32 output array,
# here the sum is fp64 and rounded once (DESIGN.md section 3E says what is and is not claimed).
RESAMPLERS = ("scipy", "kaiser_best")
SINC_FILTERS = {"kaiser_best": dict(num_zeros=64, precision=9, beta=14.769656459379492, rolloff=0.9475937167399596)}
_SINC_CHUNK = 1 << 16  # outputs per pass of the host loop over taps: ~4 MB of temporaries whatever the clip's length
_SINC_CACHE = {}


def _resampler(name):
    if name not in RESAMPLERS:
        raise ValueError("unknown resampler %r (one of %s)" % (name, ", ".join(RESAMPLERS)))
    return _resample if name == "scipy" else resample_sinc


def sinc_filter(name="kaiser_best"):
    """-> (win, num_table): the right half of the Kaiser-windowed sinc, num_table samples per zero crossing (num_zeros * num_table
    + 1 entries, 32 769 for kaiser_best), float64, built once.  The array is shared: not to be written to."""
    if name not in SINC_FILTERS:
        raise ValueError("unknown sinc filter %r (one of %s)" % (name, ", ".join(SINC_FILTERS)))
    if name not in _SINC_CACHE:
        from scipy.signal.windows import kaiser

        f = SINC_FILTERS[name]
        num_table = 2 ** f["precision"]
        n = num_table * f["num_zeros"]
        sinc_win = f["rolloff"] * np.sinc(f["rolloff"] * np.linspace(0, f["num_zeros"], n + 1))
        taper = kaiser(2 * n + 1, f["beta"])[n:]
        win = taper * sinc_win
        win.setflags(write=False)
        _SINC_CACHE[name] = (win, num_table)
    return _SINC_CACHE[name]


def sinc_plan(n_in, sr_in, sr_out, filter="kaiser_best"):  # noqa: A002 — resampy's argument name
    """Everything one call fixes on the host, for the NumPy loop and for the kernel alike -> dict(win, delta, num_table, scale, inc,
    step, n_out).  win is scaled by the ratio when downsampling; step = int(scale * num_table) truncates as resampy's does (about
    4e-3 of amplitude from 44.1 or 48 kHz down to 16 kHz) and is kept."""
    win, num_table = sinc_filter(filter)
    ratio = float(sr_out) / sr_in
    n_out = int(n_in * ratio)
    key = (filter, ratio)
    if key not in _SINC_CACHE:
        w = win * ratio if ratio < 1 else win
        delta = np.zeros_like(w)
        delta[:-1] = np.diff(w)
        for arr in (w, delta):
            arr.setflags(write=False)
        _SINC_CACHE[key] = (w, delta)
    w, delta = _SINC_CACHE[key]
    scale = min(1.0, ratio)
    return dict(win=w, delta=delta, num_table=num_table, scale=scale, inc=1.0 / ratio, step=int(scale * num_table), n_out=n_out)


def resample_sinc(data, sr_in, sr_out, filter="kaiser_best"):  # noqa: A002
    """Mono waveform [n_in] at sr_in -> float64 [int(n_in * sr_out / sr_in)] at sr_out: every output is the sum of its left-wing
    taps, then its right-wing taps, each in ascending order — vectorised over a chunk of outputs, one pass per tap, so each output
    sees exactly the additions of the scalar algorithm (and of csrc/resample.hip) in their order."""
    x = np.ascontiguousarray(data, dtype=np.float64)
    if x.ndim != 1:
        raise ValueError("resample_sinc: mono waveform expected, got shape %s" % (x.shape,))
    n_in = x.shape[0]
    p = sinc_plan(n_in, sr_in, sr_out, filter)
    win, delta, num_table, scale, inc, step = p["win"], p["delta"], p["num_table"], p["scale"], p["inc"], p["step"]
    n_win = win.shape[0]
    y = np.zeros(p["n_out"], dtype=np.float64)
    for lo in range(0, p["n_out"], _SINC_CHUNK):
        t = np.arange(lo, min(lo + _SINC_CHUNK, p["n_out"]), dtype=np.int64)
        tr = t * inc  # the product, not a running sum: the two pick another int(tr) now and then
        n = tr.astype(np.int64)
        frac = scale * (tr - n)
        acc = np.zeros(t.shape[0], dtype=np.float64)
        # (first sample of the wing, direction, samples available on that side)
        for first, sign, avail in ((n, -1, n + 1), (n + 1, 1, n_in - n - 1)):
            idx = frac * num_table
            off = idx.astype(np.int64)
            eta = idx - off
            count = np.minimum(avail, (n_win - off) // step)
            for i in range(int(count.max(initial=0))):
                live = np.flatnonzero(i < count)
                w = off[live] + i * step
                acc[live] += (win[w] + eta[live] * delta[w]) * x[first[live] + sign * i]
            frac = scale - frac
        y[lo : lo + t.shape[0]] = acc
    return y


_SINC_DEVICE = {}


def resample_sinc_device(wave, sr_in, sr_out, device, out_dtype=None, filter="kaiser_best"):  # noqa: A002
    """resample_sinc on the MI355X (csrc/resample.hip), bit-equal to it.  wave: a host array or a device tensor, mono float32 /
    float64 [n_in] -> device tensor [n_out], float64 (default) or float32 (the fp64 sum rounded once).  The filter tables stay
    resident per device and ratio, like _device_tables' own."""
    import torch

    from . import ops

    if not isinstance(wave, torch.Tensor):
        wave = np.asarray(wave)
        if wave.dtype not in (np.float32, np.float64):
            wave = wave.astype(np.float64)
        wave = torch.from_numpy(np.ascontiguousarray(wave))
    wave = wave.to(device)
    if wave.dim() != 1:
        raise ValueError("resample_sinc_device: mono waveform expected, got shape %s" % (tuple(wave.shape),))
    p = sinc_plan(int(wave.numel()), sr_in, sr_out, filter)
    key = (str(device), filter, p["inc"])
    if key not in _SINC_DEVICE:
        _SINC_DEVICE[key] = tuple(torch.from_numpy(p[k].copy()).to(device) for k in ("win", "delta"))  # (the cached arrays are read-only)
    win, delta = _SINC_DEVICE[key]
    return ops.resample_sinc(wave, win, delta, p["num_table"], p["scale"], p["inc"], p["step"], p["n_out"],
                             torch.float64 if out_dtype is None else out_dtype)


_TABLES = {}


def _device_tables(device):
    """Periodic Hann window and HTK mel matrix (float64) resident on `device`."""
    key = str(device)
    if key not in _TABLES:
        import torch

        win = int(round(SAMPLE_RATE * STFT_WINDOW_SECONDS))
        fft_len = 2 ** int(np.ceil(np.log(win) / np.log(2.0)))
        hann = 0.5 - (0.5 * np.cos(2 * np.pi / win * np.arange(win)))
        mel = mel_matrix(NUM_MEL_BINS, fft_len // 2 + 1, SAMPLE_RATE, MEL_MIN_HZ, MEL_MAX_HZ)
        _TABLES[key] = (torch.from_numpy(hann).to(device), torch.from_numpy(np.ascontiguousarray(mel)).to(device), fft_len)
    return _TABLES[key]


def log_mel_device(data, sample_rate, device, resampler="scipy"):
    """-> float64 device tensor [num_frames, 64] (mel_features.log_mel_spectrogram on the GPU).  data: a host array, or a mono
    float32 / float64 device tensor.  resampler="kaiser_best": input at another rate is uploaded as it is and resampled on the
    device, and the fp64 result feeds the log-mel kernel directly; "scipy" resamples on the host first."""
    import torch

    from . import ops

    if resampler not in RESAMPLERS:
        raise ValueError("unknown resampler %r (one of %s)" % (resampler, ", ".join(RESAMPLERS)))
    hann, mel, fft_len = _device_tables(device)
    if isinstance(data, torch.Tensor) and data.is_cuda:
        if data.dim() > 1:
            data = data.mean(dim=1)
        if sample_rate != SAMPLE_RATE and resampler == "scipy":
            raise ValueError("log_mel_device: a device waveform at %d Hz needs resampler='kaiser_best'" % sample_rate)
        wave = data.contiguous()
    else:
        data = np.asarray(data)
        if data.ndim > 1:
            data = np.mean(data, axis=1)
        if sample_rate != SAMPLE_RATE and resampler == "scipy":
            data = _resample(data, sample_rate, SAMPLE_RATE)
        if data.dtype not in (np.float32, np.float64):
            data = data.astype(np.float64)
        wave = torch.from_numpy(np.ascontiguousarray(data)).to(device)
    if sample_rate != SAMPLE_RATE and resampler == "kaiser_best":
        wave = resample_sinc_device(wave, sample_rate, SAMPLE_RATE, device)
    return ops.logmel(wave, hann, mel, int(round(SAMPLE_RATE * STFT_HOP_SECONDS)), fft_len, LOG_OFFSET)


def waveform_to_examples_device(data, sample_rate, device, resampler="scipy"):
    """-> float32 device tensor [num_examples, 100, 64]: waveform_to_examples + the .float() of validate.py:160-161."""
    from . import ops

    rate = 1.0 / STFT_HOP_SECONDS
    return ops.logmel_examples(log_mel_device(data, sample_rate, device, resampler), int(round(EXAMPLE_WINDOW_SECONDS * rate)),
                               int(round(EXAMPLE_HOP_SECONDS * rate)))
