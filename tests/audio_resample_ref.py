"""Scalar restatement of resampy 0.4's windowed-sinc resampler with the documented `kaiser_best` design: one Python loop per output
and per tap, fp64 throughout, written from the published algorithm and independent of audio_frontend's vectorised code and of
csrc/resample.hip.  The product must reproduce it bit for bit (same operations, same order); the tests compare with array_equal."""
import functools

import numpy as np
import scipy.signal

NUM_ZEROS, PRECISION = 64, 9
BETA, ROLLOFF = 14.769656459379492, 0.9475937167399596

# (n_in, sr_in, sr_out): empty outputs, one output, ragged tails, integer tr at every output (48 k -> 16 k), up- and down-sampling,
# 400 taps a wing (96 k -> 16 k)
SHAPES = [(0, 44100, 16000), (1, 44100, 16000), (2, 44100, 16000), (3, 48000, 16000), (700, 44100, 16000), (701, 48000, 16000),
          (333, 22050, 16000), (257, 8000, 16000), (500, 16000, 22050), (300, 11025, 16000), (400, 96000, 16000)]


@functools.lru_cache(maxsize=None)
def kaiser_best():
    """-> (win [32769] fp64, num_table)."""
    num_table = 2 ** PRECISION
    n = num_table * NUM_ZEROS
    sinc_win = ROLLOFF * np.sinc(ROLLOFF * np.linspace(0, NUM_ZEROS, n + 1))
    taper = scipy.signal.windows.kaiser(2 * n + 1, BETA)[n:]
    return taper * sinc_win, num_table


def n_out_of(n_in, sr_in, sr_out):
    return int(n_in * (float(sr_out) / sr_in))


def resample(x, sr_in, sr_out):
    """x [n_in] (any float type; taken to fp64 exactly) -> y [int(n_in * ratio)] fp64."""
    x = [float(v) for v in np.asarray(x, dtype=np.float64)]
    n_in = len(x)
    win, num_table = kaiser_best()
    ratio = float(sr_out) / sr_in
    n_out = int(n_in * ratio)
    if ratio < 1:
        win = win * ratio
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    win, delta = [float(v) for v in win], [float(v) for v in delta]
    n_win = len(win)
    scale = min(1.0, ratio)
    inc = 1.0 / ratio
    step = int(scale * num_table)
    y = np.zeros(n_out, dtype=np.float64)
    for t in range(n_out):
        tr = t * inc
        n = int(tr)
        frac = scale * (tr - n)
        acc = 0.0
        idx = frac * num_table
        off = int(idx)
        eta = idx - off
        for i in range(min(n + 1, (n_win - off) // step)):
            acc += (win[off + i * step] + eta * delta[off + i * step]) * x[n - i]
        frac = scale - frac
        idx = frac * num_table
        off = int(idx)
        eta = idx - off
        for k in range(min(n_in - n - 1, (n_win - off) // step)):
            acc += (win[off + k * step] + eta * delta[off + k * step]) * x[n + k + 1]
        y[t] = acc
    return y


def wave(n_in, dtype=np.float64, seed=None):
    """The tests' input of a shape: 0.3 * N(0, 1), seeded by the length."""
    rng = np.random.default_rng(1000 + n_in if seed is None else seed)
    return (0.3 * rng.standard_normal(n_in)).astype(dtype)


@functools.lru_cache(maxsize=None)
def case(n_in, sr_in, sr_out, dtype_name):
    """-> (x, y): the input of a shape in `dtype_name` and its fp64 resampling; computed once per session, not to be written to."""
    x = wave(n_in, np.dtype(dtype_name))
    y = resample(x, sr_in, sr_out)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y
