"""Writes tests/golden/render_gngf_256x257.npz: the literal oracle (oracle.gngf_oracle.gngf_forward) of the first render test
model in GNGF mode on the 256 x 257 lattice — the one expected value of tests/test_gpu_render.py that is too heavy to compute
inside the test (the oracle evaluates the HPD per instance: 65792 pixels x 64 vertices x T = 256 dense distributions, in
chunks of 2048 pixels here; the decoder and the interpolation are per pixel, so chunking changes nothing).
    python tools/make_render_golden.py          (CPU only, a few minutes)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import test_gpu_render as tr
    from collision_handling_in_instantngp_amd import train
    c = tr.cfg(tr.FIRST, "gngf", 256)
    p = tr.render_params(c)
    coords = train.lattice_coordinates(256, 257, 256)
    rgb = np.concatenate([tr.oracle_rgb(c, p, coords[lo:lo + 2048]) for lo in range(0, coords.shape[0], 2048)])
    assert rgb.shape == (256 * 257, 3) and rgb.dtype == np.float32
    np.savez_compressed(tr.GOLDEN_256, rgb=rgb)
    print(tr.GOLDEN_256, os.path.getsize(tr.GOLDEN_256), "bytes")


if __name__ == "__main__":
    main()
