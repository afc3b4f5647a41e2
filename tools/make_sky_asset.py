#!/usr/bin/env python3
"""tools/make_sky_asset.py -- writes the small environment asset of DESIGN section 5j: tests/golden/environment/sky_dusk.hdr, a procedural
equirectangular sky (96 x 48, Radiance RGBE, run-length encoded: a few KiB -- a low sun over a warm horizon, a dark ground), and
assets/scenes/spheres_sky.json, three balls on a floor under it.  Deterministic: run again, the same bytes.
With --sun it writes the asset of section 5k instead and leaves the first alone: tests/golden/environment/sky_sun.hdr (48 x 24, under
1 KiB: a flat sky with a sun of a few pixels, some thousand times the sky) and assets/scenes/spheres_sun.json, the same balls under it
with a fourth that shades one of them, "environment": {"light": true}.

    tools/make_sky_asset.py [--sun]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sky(width=96, height=48):
    """[height, width, 3]: row 0 up, the picture's centre the direction -z (u = atan2(x, -z) / 2 pi + 0.5, v = acos(y) / pi)"""
    u = (np.arange(width) + 0.5) / width
    v = (np.arange(height) + 0.5) / height
    phi, theta = (u[None, :] - 0.5) * 2.0 * np.pi, v[:, None] * np.pi
    d = np.stack([np.sin(theta) * np.sin(phi), np.cos(theta) * np.ones_like(phi), -np.sin(theta) * np.cos(phi)], axis=-1)
    up = np.clip(d[..., 1], 0.0, 1.0)[..., None]
    img = np.array([1.0, 0.55, 0.3]) * (1.0 - up) ** 3 + np.array([0.08, 0.16, 0.45]) * up
    img = np.where(d[..., 1:2] < 0.0, np.array([0.05, 0.045, 0.04]), img)
    sun = np.array([-0.45, 0.25, -0.85])
    sun /= np.linalg.norm(sun)
    img = img + 30.0 * np.clip(d @ sun, 0.0, 1.0)[..., None] ** 200 * np.array([1.0, 0.8, 0.55])
    return img.astype(np.float32)


def sun_sky(width=48, height=24):
    """a flat blue sky over a dark ground (long runs: a small file) and a sun of a pixel or two, high in the south-west"""
    u = (np.arange(width) + 0.5) / width
    v = (np.arange(height) + 0.5) / height
    phi, theta = (u[None, :] - 0.5) * 2.0 * np.pi, v[:, None] * np.pi
    d = np.stack([np.sin(theta) * np.sin(phi), np.cos(theta) * np.ones_like(phi), -np.sin(theta) * np.cos(phi)], axis=-1)
    img = np.where(d[..., 1:2] < 0.0, np.array([0.05, 0.045, 0.04]), np.array([0.25, 0.375, 0.75]))
    sun = np.array([-0.5, 0.6, 0.35])
    sun /= np.linalg.norm(sun)
    img = np.where((d @ sun)[..., None] > np.cos(np.radians(5.0)), np.array([3000.0, 2750.0, 2250.0]), img)
    return img.astype(np.float32)


def sun_scene():
    s = scene()
    s["environment"] = {"file": "../../tests/golden/environment/sky_sun.hdr", "scale": 1.0, "size": 32, "light": True}
    s["camera"]["resolution"] = [192, 144]
    s["materials"].append({"name": "panel", "type": "lambertian", "albedo": [0.7, 0.3, 0.2]})
    s["surfaces"].append({"type": "sphere", "radius": 0.3, "material": "panel", "transform": {"translate": [-0.55, 0.55, -0.2]}})
    return s


def scene():
    ball = lambda x, z, material: {"type": "sphere", "radius": 0.5, "material": material, "transform": {"translate": [x, -0.5, z]}}
    return {
        "camera": {"transform": {"from": [0.0, 0.4, 4.0], "at": [0.0, -0.3, 0.0], "up": [0, 1, 0]}, "vfov": 45, "resolution": [256, 192]},
        "sampler": {"type": "independent", "samples": 64},
        "environment": {"file": "../../tests/golden/environment/sky_dusk.hdr", "scale": 1.0, "size": 64},
        "materials": [{"name": "floor", "type": "lambertian", "albedo": [0.6, 0.6, 0.6]},
                      {"name": "ball_diffuse", "type": "lambertian", "albedo": [0.1, 0.2, 0.5]},
                      {"name": "ball_metal", "type": "metal", "albedo": [0.8, 0.6, 0.2], "fuzz": 0.05},
                      {"name": "ball_glass", "type": "dielectric", "refraction_index": 1.5}],
        "surfaces": [{"type": "sphere", "radius": 1000.0, "material": "floor", "transform": {"translate": [0.0, -1001.0, 0.0]}},
                     ball(0.0, -0.6, "ball_diffuse"), ball(1.1, 0.1, "ball_metal"), ball(-1.1, 0.2, "ball_glass")],
    }


def main():
    import __graft_entry__ as graft
    pkg = graft.load_package()
    out = os.path.join(ROOT, "assets", "scenes")
    if sys.argv[1:] == ["--sun"]:
        picture = os.path.join(ROOT, "tests", "golden", "environment", "sky_sun.hdr")
        pkg.hdr.write_hdr(picture, sun_sky(), rle=True)
        with open(os.path.join(out, "spheres_sun.json"), "w") as f:
            json.dump(sun_scene(), f, indent=1)
            f.write("\n")
        print(os.path.getsize(picture), "bytes of sky_sun.hdr")
        return
    picture = os.path.join(ROOT, "tests", "golden", "environment", "sky_dusk.hdr")  # (binary files live under tests/golden/)
    os.makedirs(os.path.dirname(picture), exist_ok=True)
    pkg.hdr.write_hdr(picture, sky(), rle=True)
    with open(os.path.join(out, "spheres_sky.json"), "w") as f:
        json.dump(scene(), f, indent=1)
        f.write("\n")
    print(os.path.getsize(picture), "bytes of sky_dusk.hdr")


if __name__ == "__main__":
    main()
