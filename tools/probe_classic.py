"""The classic baseline's device chain (classic.texture_device) stage by stage at N frames of hw x hw x 3 from
synth.structured_video: D1 (pairwise_l2), P1, D2 (diag_filter, 16 taps), P2, pow, the future-cost sweeps (with their count)
and P3 with the threshold.  Each stage between two device synchronisations, medians of 5 after 2 warm-ups; the sweeps also as
time per sweep and as the rate at which D3 is read (n^2 * 4 bytes a sweep).  At N <= 1024 the host classic.q_learning on the same
D2 is timed once for comparison: before the wide kernel it was the only path past 200 rows.  Numbers: profiles/r18/README.md.

    python tools/probe_classic.py N [hw]"""
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from avtex import classic, ops, synth  # noqa: E402

DEV = torch.device("cuda:0")
SIGMA_FACTOR, FILTER, P, ALPHA, TH = 0.1, 16, 0.7, 0.997, 0.75


def timed(fn, n=5, warm=2):
    out, ts = None, []
    for k in range(warm + n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if k >= warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    return out, statistics.median(ts)


def main():
    n = int(sys.argv[1])
    hw = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    print(ops.device_check(), "| N = %d frames of %d x %d x 3" % (n, hw, hw), flush=True)
    frames = synth.structured_video(5, n, hw, hw)
    f = frames.float().reshape(n, -1).contiguous().to(DEV)
    w = torch.tensor((np.poly1d([0.5, 0.5]) ** (FILTER - 1)).coeffs, dtype=torch.float32, device=DEV)
    rows = []
    d1, t = timed(lambda: ops.pairwise_l2(f))
    rows.append(("D1 pairwise_l2 [%d x %d]" % (n, f.shape[1]), t))
    _, t = timed(lambda: ops.classic_p(d1, SIGMA_FACTOR))
    rows.append(("P1 classic_p", t))
    d2, t = timed(lambda: ops.diag_filter(d1, w))
    rows.append(("D2 diag_filter", t))
    _, t = timed(lambda: ops.classic_p(d2, SIGMA_FACTOR))
    rows.append(("P2 classic_p", t))
    d3_in, t = timed(lambda: (d2 ** P).contiguous())
    rows.append(("pow", t))
    (d3, iters), t_sweeps = timed(lambda: ops.q_learning_wide(d3_in, ALPHA, 10e-3, 1000))
    sweeps, m = int(iters.item()), d3_in.shape[0]
    rows.append(("sweeps q_learning_wide (%d sweeps, m = %d)" % (sweeps, m), t_sweeps))
    _, t = timed(lambda: ops.classic_p(d3, SIGMA_FACTOR, threshold=TH))
    rows.append(("P3 classic_p + threshold", t))
    _, t_all = timed(lambda: classic.texture_device(frames, SIGMA_FACTOR, filter_size=FILTER, device=DEV), n=3, warm=1)
    for name, t in rows:
        print("%-52s %10.3f ms" % (name, t))
    print("%-52s %10.3f ms" % ("sum of the stages", sum(t for _, t in rows)))
    print("%-52s %10.3f ms" % ("texture_device, frames on the host to matrices", t_all))
    # a sweep in steady state: tol = -1 never stops, so exactly FORCED sweeps run in FORCED + 2 launches (the residual lags the
    # minima by one launch, the decision by two); the few sweeps above are mostly the call's fixed cost (the workspace memset, one
    # read-back of the stop word for every 16 launches, the launch that writes the matrix)
    forced = 200
    (_, it_f), t_forced = timed(lambda: ops.q_learning_wide(d3_in, ALPHA, -1.0, forced))
    assert int(it_f.item()) == forced
    per = t_forced / (forced + 2)
    print("%-52s %10.3f ms" % ("%d forced sweeps (tol = -1, max_iter = %d)" % (forced, forced), t_forced))
    print("per sweep launch: %.2f us, D3 read at %.0f GB/s (%d bytes a sweep)" % (per * 1e3, m * m * 4 / (per * 1e-3) / 1e9, m * m * 4))
    # P tail as the parent computed it (classic._p_from_d: nonzero, sum, exp, cat, normalise in torch ops) for comparison
    if n <= 4096:
        _, t = timed(lambda: classic._p_from_d(d3, SIGMA_FACTOR))
        print("%-52s %10.3f ms" % ("P3 by classic._p_from_d (torch ops, no threshold)", t))
    if n <= 1024:
        d2_host = d2.cpu()
        t0 = time.perf_counter()
        h3, _, _, _ = classic.q_learning(d2_host, SIGMA_FACTOR, p=P, alpha=ALPHA, thresholding=TH)
        t_host = (time.perf_counter() - t0) * 1e3
        print("%-52s %10.3f ms" % ("host classic.q_learning (pow, sweeps, P3), one run", t_host))
        print("max |device D3 - host D3| = %.3e (host pow and device pow differ in the last ulp)" % float((d3.cpu() - h3).abs().max()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
