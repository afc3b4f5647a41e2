#!/usr/bin/env python3
"""tools/make_denoise_albedo_asset.py -- writes the texture fixture of DESIGN section 5r.  Deterministic: run again, the same bytes.

    tests/golden/textures/checker8.png     8 x 8 RGBA, a grey checker of single texels, bytes 51 and 204: 0.2 and 0.8 under the linear
                                           encoding (51 / 255 and 204 / 255 in binary32), alpha 255

tests/test_gpu_denoise_albedo.py lays it over a quad that fills the frame, nearest-filtered: the albedo edge the denoiser must keep."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def checker8():
    y, x = np.mgrid[0:8, 0:8]
    img = np.zeros((8, 8, 4), dtype=np.uint8)
    img[..., :3] = np.where((x + y) % 2 == 0, 51, 204)[..., None]
    img[..., 3] = 255
    return img


def main():
    import __graft_entry__ as graft
    png = graft.load_package().png
    png.write_png(os.path.join(ROOT, "tests", "golden", "textures", "checker8.png"), checker8(), filters=[0])


if __name__ == "__main__":
    main()
