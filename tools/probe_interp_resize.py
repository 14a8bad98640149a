"""slowmo.Interpolator.__call__ at 360 x 640, SF 5 on frames whose extents are not multiples of 32: the device resize (ops.resize_u8)
against the host route it replaced (device -> host, Pillow, host -> device around the same networks), and the networks alone at 352 x 640.
Alternating calls in one process, each between two device synchronisations; medians of 20 after warm-up.  Checks first that the two
routes give the same bytes.  Numbers: profiles/r16/README.md.

    python tools/probe_interp_resize.py [--out timing.json]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from avtex import ops, slowmo  # noqa: E402
from avtex.fused_slowfast import new_act  # noqa: E402
from interp_weights import frame_pair, unet_state  # noqa: E402

DEV = torch.device("cuda:0")
H, W, SF = 360, 640, 5


class ParentInterpolator(slowmo.Interpolator):
    """__call__ with the resizes on the host, as before ops.resize_u8: a round trip through Pillow per frame."""

    def _resize(self, frame, size, lanczos):
        from PIL import Image
        img = Image.fromarray(frame.cpu().numpy())
        img = img.resize(size, Image.LANCZOS if lanczos else Image.BILINEAR)
        return torch.from_numpy(np.array(img.convert("RGB"))).to(self.dev)

    def __call__(self, frame0, frame1):
        if self._fc is None:
            self._fc, self._at = slowmo.UNetX3(self.flow_comp, self.dev), slowmo.UNetX3(self.arb_time, self.dev)
        h, w, sf, pd = self.nh, self.nw, self.sf, ops.X3_F16
        if (h, w) != (self.h, self.w):
            frame0, frame1 = self._resize(frame0, (w, h), True), self._resize(frame1, (w, h), True)
        frame0, frame1 = frame0.contiguous(), frame1.contiguous()
        img = torch.empty((2, h, w, 4), dtype=torch.float32, device=self.dev)
        x = new_act(h * w, 8, (1, 1, h, w), self.dev, True)
        ops.interp_pack_pair(frame0, frame1, slowmo.MEAN, img, x.ptrs, pd)
        flow = self._fc.forward(x)
        nt = sf - 1
        xin = new_act(nt * h * w, 24, (nt, 1, h, w), self.dev, True)
        ft = torch.empty((nt, h, w, 4), dtype=torch.float32, device=self.dev)
        ops.interp_mid_input(img, flow.ptrs, h, w, sf, xin.ptrs, ft, pd)
        o = self._at.forward(xin)
        out = torch.empty((nt, h, w, 3), dtype=torch.uint8, device=self.dev)
        ops.interp_final(img, ft, o.ptrs, h, w, sf, slowmo.MEAN, out, pd)
        if (h, w) != (self.h, self.w):
            out = torch.stack([self._resize(f, (self.w, self.h), False) for f in out])
        return out


def make(cls, h, w):
    it = cls(h, w, SF, DEV)
    it.flow_comp.load_state_dict(unet_state(6, 4, 31, head_gain=20.0))
    it.arb_time.load_state_dict(unet_state(20, 5, 32, head_gain=5.0))
    return it


def timed(fn, n):
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def main():
    print(ops.device_check(), flush=True)
    f0, f1 = (f.to(DEV) for f in frame_pair(9, H, W))
    new, old, core = make(slowmo.Interpolator, H, W), make(ParentInterpolator, H, W), make(slowmo.Interpolator, 352, 640)
    c0, c1 = f0[:352].contiguous(), f1[:352].contiguous()
    a, b = new(f0, f1), old(f0, f1)
    torch.cuda.synchronize()
    equal = bool(torch.equal(a, b))
    print("device route == host route, byte for byte:", equal, flush=True)
    for _ in range(3):
        new(f0, f1), old(f0, f1), core(c0, c1)
    t_new, t_old, t_core = [], [], []
    for _ in range(20):  # alternating
        t_new += timed(lambda: new(f0, f1), 1)
        t_old += timed(lambda: old(f0, f1), 1)
        t_core += timed(lambda: core(c0, c1), 1)
    pair, four = torch.stack((f0, f1)), a[:, :352].contiguous()
    t_down = timed(lambda: ops.resize_u8(pair, (352, 640), "lanczos"), 30)[10:]
    t_up = timed(lambda: ops.resize_u8(four, (H, W), "bilinear"), 30)[10:]
    t_hdown = timed(lambda: [old._resize(f, (640, 352), True) for f in (f0, f1)], 15)[5:]
    t_hup = timed(lambda: [old._resize(f, (W, H), False) for f in four], 15)[5:]
    med = statistics.median
    res = {"shape": [H, W], "sf": SF, "calls": 20, "routes_equal": equal,
           "interpolator_device_resize_ms": {"median": med(t_new), "min": min(t_new), "max": max(t_new)},
           "interpolator_host_resize_ms": {"median": med(t_old), "min": min(t_old), "max": max(t_old)},
           "interpolator_352x640_no_resize_ms": {"median": med(t_core), "min": min(t_core), "max": max(t_core)},
           "resize_only_ms": {"device_lanczos_2_frames": med(t_down), "device_bilinear_4_frames": med(t_up),
                              "host_lanczos_2_frames": med(t_hdown), "host_bilinear_4_frames": med(t_hup)}}
    if len(sys.argv) == 3 and sys.argv[1] == "--out":
        json.dump(res, open(sys.argv[2], "w"), indent=1)
    print(json.dumps(res, indent=1))
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
