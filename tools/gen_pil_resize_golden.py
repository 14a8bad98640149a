"""Writes tests/golden/pil_resize.npz from Pillow: inputs and `Image.resize` outputs for the small cases of tests/pil_resize_ref.py,
so that the GPU tests of ops.resize_u8 do not depend on the Pillow version of the machine they run on.

    python tools/gen_pil_resize_golden.py

Per case NAME: NAME_in uint8 [H, W, 3] (random bytes, a third of the rows 0 / 255 noise), NAME_down = LANCZOS to (h, w),
NAME_up = BILINEAR of NAME_down back to (H, W).  up4 = BILINEAR of the four 32 x 64 `down` frames, as one batch, to 45 x 70 — the
SF - 1 frames of a jump.  `pillow_version` records what wrote it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pil_resize_ref as ref  # noqa: E402


def main():
    import PIL
    out = {"pillow_version": np.array(PIL.__version__)}
    for seed, (name, big, small) in enumerate(ref.CASES):
        x = ref.noisy_frames(100 + seed, big + (3,))
        down = ref.pil_resize(x, small, ref.LANCZOS)
        out[name + "_in"], out[name + "_down"], out[name + "_up"] = x, down, ref.pil_resize(down, big, ref.BILINEAR)
    batch = np.stack([out[name + "_down"] for name, _, small in ref.CASES if small == (32, 64)][:ref.UP_BATCH])
    assert batch.shape == (ref.UP_BATCH, 32, 64, 3)
    out["up4"] = ref.pil_resize(batch, (45, 70), ref.BILINEAR)
    path = os.path.join(ROOT, "tests", "golden", "pil_resize.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
