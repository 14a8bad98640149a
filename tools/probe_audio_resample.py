"""Waveform -> VGGish examples for 600 s of mono float32 audio at 44.1 and at 48 kHz, two chains in one process, alternating:

  device: upload the waveform as decoded, resample on the MI355X by the kaiser_best windowed sinc (csrc/resample.hip), log-mel, examples
          (audio_frontend.waveform_to_examples_device(..., resampler="kaiser_best"));
  parent: scipy.signal.resample_poly on the host, upload, log-mel, examples (the default chain, resampler="scipy").

Each call runs between two device synchronisations; medians of --reps calls after one warm-up call of each, plus the resampling
kernel alone by device events.  The two chains do NOT compute the same thing (that is the point of the option): the probe says
what the reference's arithmetic costs next to today's, not which of two equal results is faster.  Numbers: profiles/r27/README.md.

    python tools/probe_audio_resample.py [--seconds 600] [--reps 5] [--out timing.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from avtex import audio_frontend as af  # noqa: E402
from avtex import ops  # noqa: E402

DEV = torch.device("cuda:0")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures the MI355X: no device, no number"
    print("device:", ops.device_check())
    result = {"seconds": a.seconds, "reps": a.reps, "rates": {}}
    for sr in (44100, 48000):
        rng = np.random.default_rng(sr)
        x = (0.1 * rng.standard_normal(int(a.seconds * sr))).astype(np.float32)
        chains = {"device": lambda: af.waveform_to_examples_device(x, sr, DEV, resampler="kaiser_best"),
                  "parent": lambda: af.waveform_to_examples_device(x, sr, DEV, resampler="scipy")}
        shapes = {k: tuple(timed(fn)[1].shape) for k, fn in chains.items()}  # warm-up: code objects, tables, allocator
        ms = {k: [] for k in chains}
        for _ in range(a.reps):
            for k, fn in chains.items():
                ms[k].append(timed(fn)[0])
        # the resampling kernel alone, on a waveform already in HBM
        xd = torch.from_numpy(x).to(DEV)
        p = af.sinc_plan(x.shape[0], sr, af.SAMPLE_RATE)
        y = af.resample_sinc_device(xd, sr, af.SAMPLE_RATE, DEV)
        kern = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            af.resample_sinc_device(xd, sr, af.SAMPLE_RATE, DEV)
            e1.record()
            e1.synchronize()
            kern.append(e0.elapsed_time(e1))
        taps = 2 * ((p["win"].shape[0] - 1) // p["step"]) + 1
        row = {"n_in": int(x.shape[0]), "n_out": int(y.numel()), "taps_per_output": taps, "examples": shapes,
               "device_chain_ms": statistics.median(ms["device"]), "parent_chain_ms": statistics.median(ms["parent"]),
               "device_chain_all_ms": ms["device"], "parent_chain_all_ms": ms["parent"],
               "resample_kernel_ms": statistics.median(kern), "resample_kernel_all_ms": kern}
        row["resample_gtaps_per_s"] = row["n_out"] * taps / (row["resample_kernel_ms"] * 1e-3) / 1e9
        result["rates"][str(sr)] = row
        print("%d Hz, %.0f s: device chain %.1f ms, parent chain %.1f ms (medians of %d); resample kernel alone %.2f ms "
              "(%d outputs x %d taps, %.1f G taps/s); examples %s / %s" % (
                  sr, a.seconds, row["device_chain_ms"], row["parent_chain_ms"], a.reps, row["resample_kernel_ms"], row["n_out"], taps,
                  row["resample_gtaps_per_s"], shapes["device"], shapes["parent"]))
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
