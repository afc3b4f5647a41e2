#!/usr/bin/env python3
"""tools/denoise_variance_sweep.py -- the two CPU measurements of DESIGN section 5s (profiles/denoise_variance.txt), from the float64
restatement (tests/denoise_variance_ref.py); no GPU.

    denoise_variance_sweep.py sigma     the default's sweep: a 1-iteration render of assets/scenes/cornell_textured.json at 64 x 64, 4
                                        bounces, by the CPU oracle; the guided passes at filter size 16 on its irradiance (the colour over
                                        the first-hit albedo, section 5r) for sigma 4, 8 and 16, remodulated, against the oracle's
                                        1024-iteration render of the same frame: one RMSE each, and the plain passes' for scale.  The
                                        oracle has no textures, so both renders and the albedo plane are the scene's without them.
    denoise_variance_sweep.py edge      the table of the issue: the 64 x 64 edge image at noise 0.02, 0.1 and 0.3, filter size 16 --
                                        RMSE against the clean image of the noisy input, the plain passes (c_phi 0.45) and the guided
                                        passes at each sigma, whole frame / edge band, and the ratios plain / guided."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def sigma_sweep(pkg, orc, dr, vr, dm):
    w = h = 64
    sc = pkg.json_parser.scene_from_json(os.path.join(ROOT, "assets", "scenes", "cornell_textured.json"))
    flat = sc.build_scene()
    one = orc.render_megakernel(flat, sc.camera, w, h, 0, 1, 4)
    many = orc.render_megakernel(flat, sc.camera, w, h, 0, 1024, 4)
    # the first-hit albedo of the pixel-centre rays: the material's colour at a diffuse or metal hit, else ones (section 5r)
    matrix, vfov = dr.gpu_camera(orc, sc.camera, w, h)
    ys, xs = np.mgrid[0:h, 0:w]
    origin, dirs = dr.view_rays(matrix, vfov, w, h, xs + 0.5, ys + 0.5)
    rays = np.zeros((w * h, 8), dtype=np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = origin, 1e-4, dirs.reshape(-1, 3), np.inf
    recs, hit = orc.intersect_rays(flat, rays)
    albedo = np.ones((w * h, 3))
    mats = flat.materials
    for i in np.nonzero(hit)[0]:
        m = mats[int(recs["material_id"][i])]
        if int(m["type"]) <= 1:
            albedo[i] = [float(x) for x in m["p"][:3]]
    albedo = albedo.reshape(h, w, 3)
    e = dm.effective_f64(albedo.astype(np.float32))
    irr = dm.irradiance_f64(one["color"], albedo.astype(np.float32))
    truth = many["color"].astype(np.float64)
    print(f"sigma sweep: cornell_textured.json {w} x {h}, 4 bounces, filter size 16, albedo plane on; RMSE against 1024 iterations")
    print(f"  1-iteration input            {vr.rmse(one['color'], truth):.5f}")
    plain = dm.demodulated_denoise(orc, sc.camera, w, h, one["color"], albedo.astype(np.float32), one["normal"], one["depth"], 16)
    print(f"  plain passes (c_phi 0.45)    {vr.rmse(plain, truth):.5f}")
    for sigma in vr.SIGMAS:
        _, out = vr.guided(orc, sc.camera, w, h, irr, one["normal"], one["depth"], 16, sigma)
        print(f"  guided, sigma {sigma:4.0f}           {vr.rmse(out * e, truth):.5f}")


def edge_table(pkg, orc, dr, vr):
    cam = dr.low_camera(pkg)
    n = vr.EDGE_SIZE
    print("edge image 64 x 64, 0.5 | 0.65, filter size 16: RMSE against the clean image, whole frame / 6-pixel band around the edge")
    for noise in vr.EDGE_NOISES:
        clean, noisy, normal, depth, band = vr.edge_image(noise)
        plain = dr.denoise(orc, cam, n, n, noisy, normal, depth, 16)
        row = f"  noise {noise:4.2f}: input {vr.rmse(noisy, clean):.4f} | plain {vr.rmse(plain, clean):.4f} / {vr.rmse(plain, clean, band):.4f}"
        for sigma in vr.SIGMAS:
            _, g = vr.guided(orc, cam, n, n, noisy, normal, depth, 16, sigma)
            row += (f" | sigma {sigma:.0f}: {vr.rmse(g, clean):.4f} / {vr.rmse(g, clean, band):.4f}"
                    f" (x{vr.rmse(plain, clean) / vr.rmse(g, clean):.2f} / x{vr.rmse(plain, clean, band) / vr.rmse(g, clean, band):.2f})")
        print(row)


def main():
    import __graft_entry__ as graft
    pkg, orc = graft.load_package(), graft.load_oracle()
    import demodulate_ref as dm
    import denoise_ref as dr
    import denoise_variance_ref as vr
    if sys.argv[1] == "sigma":
        sigma_sweep(pkg, orc, dr, vr, dm)
    else:
        edge_table(pkg, orc, dr, vr)


if __name__ == "__main__":
    main()
