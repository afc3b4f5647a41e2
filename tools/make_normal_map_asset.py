#!/usr/bin/env python3
"""tools/make_normal_map_asset.py -- writes the small normal-map assets of DESIGN section 5q.  Deterministic: run again, the same bytes.

    tests/golden/textures/ripples.png      32 x 32 RGB, a tangent-space normal map: concentric ripples about the picture's centre that
                                           fade out towards its border, so that it tiles; byte = round(128 + 127 c) per component, the
                                           inverse of the decode table (128 is exactly 0), and the border texels are exactly flat
    assets/scenes/cornell_bumpy.json       cornell_textured.json's room with both boxes under that map beside their colour textures,
                                           "normal_maps": true

The PNG lives under tests/golden/ because this repository keeps every binary file there; the scene names it by a path relative to
itself."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N = 32


def ripples():
    """[32, 32, 4], row 0 the BOTTOM of the picture: the normal of the height field h = a(r) cos(2 pi 3 r), r the distance from the centre
    in picture widths, a = 0.035 (1 - (r / 0.46)^2)^2 for r < 0.46 and 0 outside, which leaves the border texels exactly flat;
    derivatives by central differences on a grid eight times finer, averaged per texel"""
    fine = 8 * N
    c = (np.arange(fine) + 0.5) / fine - 0.5
    x, y = np.meshgrid(c, c)
    r = np.sqrt(x * x + y * y)
    h = np.where(r < 0.46, 0.035 * (1.0 - (r / 0.46) ** 2) ** 2, 0.0) * np.cos(2.0 * np.pi * 3.0 * r)
    dy, dx = np.gradient(h, 1.0 / fine)
    dx = dx.reshape(N, 8, N, 8).mean(axis=(1, 3))
    dy = dy.reshape(N, 8, N, 8).mean(axis=(1, 3))
    n = np.stack([-dx, -dy, np.ones_like(dx)], axis=-1)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    img = np.full((N, N, 4), 255, dtype=np.uint8)
    img[..., :3] = np.clip(np.rint(128.0 + 127.0 * n), 0, 255).astype(np.uint8)
    return img


def main():
    import __graft_entry__ as graft
    png = graft.load_package().png
    tex = os.path.join(ROOT, "tests", "golden", "textures")
    png.write_png(os.path.join(tex, "ripples.png"), ripples(), filters=[0, 1, 2, 3, 4], alpha=False)
    with open(os.path.join(ROOT, "assets", "scenes", "cornell_textured.json")) as f:
        scene = json.load(f)
    for m in scene["materials"]:
        if "texture" in m:
            m["normal_map"] = {"file": "../../tests/golden/textures/ripples.png"}
    scene["normal_maps"] = True
    with open(os.path.join(ROOT, "assets", "scenes", "cornell_bumpy.json"), "w") as f:
        json.dump(scene, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
