#!/usr/bin/env python3
"""tools/make_texture_asset.py -- writes the small texture assets of DESIGN section 5o.  Deterministic: run again, the same bytes.

    tests/golden/textures/checker.png      16 x 16 RGBA, a coloured checker with a bright corner mark at the picture's TOP left (so that a
                                           missing row flip shows), scanline filters 0 .. 4 in turn
    tests/golden/textures/stripes.png      12 x 5 RGB (colour type 2), diagonal stripes, scanline filters 4 .. 0 in turn
    tests/golden/textures/filter_<k>.png   7 x 6 RGBA, the same random texels five times, every row with scanline filter k
    tests/golden/textures/grey16.png, palette.png, interlaced.png, truncated.png    files a reader must refuse: 16 bits a channel, colour
                                           type 3, Adam7, and a file cut short
    assets/models/box_uv.obj               a unit box, quads, with `vt` records: every face shows the whole picture, so the eight
                                           corners are shared by three faces with three different coordinates each (seams)
    assets/scenes/cornell_textured.json    cornell_mesh.json's room with the box in place of its meshes, once diffuse under the checker
                                           and once metal under the stripes, "textures": true

The PNGs live under tests/golden/ because this repository keeps every binary file there; the scene names them by a path relative to
itself."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def checker():
    """[16, 16, 4], row 0 the BOTTOM of the picture"""
    y, x = np.mgrid[0:16, 0:16]
    on = ((x // 4) + (y // 4)) % 2 == 0
    img = np.zeros((16, 16, 4), dtype=np.uint8)
    img[..., 0] = np.where(on, 230, 40 + 8 * x)
    img[..., 1] = np.where(on, 200 - 6 * y, 60)
    img[..., 2] = np.where(on, 90, 160 + 5 * y)
    img[..., 3] = 255 - x
    img[12:, :4] = (255, 255, 0, 255)  # the top left of the picture
    return img


def stripes():
    y, x = np.mgrid[0:5, 0:12]
    k = (x + 2 * y) % 6
    img = np.zeros((5, 12, 4), dtype=np.uint8)
    img[..., 0] = 30 + 40 * k
    img[..., 1] = 250 - 35 * k
    img[..., 2] = 128 + 20 * (k % 3)
    img[..., 3] = 255
    return img


BOX = """# a unit box with texture coordinates: every face shows the whole picture
v -0.5 -0.5 -0.5
v 0.5 -0.5 -0.5
v 0.5 0.5 -0.5
v -0.5 0.5 -0.5
v -0.5 -0.5 0.5
v 0.5 -0.5 0.5
v 0.5 0.5 0.5
v -0.5 0.5 0.5
vt 0 0
vt 1 0
vt 1 1
vt 0 1
f 5/1 6/2 7/3 8/4
f 2/1 1/2 4/3 3/4
f 6/1 2/2 3/3 7/4
f 1/1 5/2 8/3 4/4
f 8/1 7/2 3/3 4/4
f 1/1 2/2 6/3 5/4
"""


def main():
    import __graft_entry__ as graft
    png = graft.load_package().png
    tex = os.path.join(ROOT, "tests", "golden", "textures")
    os.makedirs(tex, exist_ok=True)
    png.write_png(os.path.join(tex, "checker.png"), checker(), filters=[0, 1, 2, 3, 4])
    png.write_png(os.path.join(tex, "stripes.png"), stripes(), filters=[4, 3, 2, 1, 0], alpha=False)
    same = np.random.default_rng(7).integers(0, 256, (6, 7, 4), dtype=np.uint8)
    for k in range(5):
        png.write_png(os.path.join(tex, f"filter_{k}.png"), same, filters=[k])
    png.write_png(os.path.join(tex, "grey16.png"), same, header=(16, 0, 0, 0, 0))
    png.write_png(os.path.join(tex, "palette.png"), same, header=(8, 3, 0, 0, 0))
    png.write_png(os.path.join(tex, "interlaced.png"), same, header=(8, 6, 0, 0, 1))
    with open(os.path.join(tex, "filter_0.png"), "rb") as f:
        whole = f.read()
    with open(os.path.join(tex, "truncated.png"), "wb") as f:
        f.write(whole[:len(whole) // 2])
    with open(os.path.join(ROOT, "assets", "models", "box_uv.obj"), "w") as f:
        f.write(BOX)
    with open(os.path.join(ROOT, "assets", "scenes", "cornell_mesh.json")) as f:
        scene = json.load(f)
    for m in scene["materials"]:
        if m["name"] == "bunny":
            m["texture"] = {"file": "../../tests/golden/textures/checker.png"}
        if m["name"] == "bunny2":
            m["albedo"] = [0.9, 0.9, 0.9]
            m["texture"] = {"file": "../../tests/golden/textures/stripes.png", "encoding": "linear", "filter": "nearest", "wrap": "clamp"}
    for s in scene["surfaces"]:
        if s["type"] == "mesh":
            s["filename"] = "../models/box_uv.obj"
            if s["material"] == "bunny":
                s["transform"] = [{"rotate": 30, "axis": [0, 1, 0]}, {"translate": [0.9, -0.5, -0.4]}]
            else:
                s["transform"] = [{"scale": 0.6}, {"rotate": -25, "axis": [0.2, 1, 0]}, {"translate": [-0.9, -0.7, 0.3]}]
    scene["textures"] = True
    with open(os.path.join(ROOT, "assets", "scenes", "cornell_textured.json"), "w") as f:
        json.dump(scene, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
