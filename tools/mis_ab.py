#!/usr/bin/env python3
"""tools/mis_ab.py -- what multiple importance sampling in the megakernel costs and buys; profiles/mis.txt holds
its output.

    tools/mis_ab.py [--iterations N] [--repeats R] [--variance-only]
    tools/mis_ab.py --cpu            no GPU: the spread of block means on the low-panel scene from the numpy restatement (tests/mis_ref.py)

Time, section 5g's method: two contexts, "mis" 0 and 1, the light parameters on in both; after a warm-up of both, R repeats ALTERNATING
between them: N iterations from a restart, wall clock around the ptc_trace calls and the synchronise that ends them; ms per iteration =
the median repeat / N, N raised after the warm-up until a repeat lasts half a second.  Scenes: scenes.cornell_lit(with_mesh=True) at 1280 x 720 under "direct_light", assets/scenes/spheres_sun.json
under "environment_light", and low_panel_scene (below) under "direct_light"; 8 bounces.
Variance at equal time: 16 blocks per mode from cleared framebuffers, 256 iterations a block with "mis" 0 and round(256 / time ratio)
with 1 -- the time ratio measured on that scene at the blocks' own size -- per channel the variance of the block image means.
low_panel_scene (tests/test_gpu_mis.py): an emissive quad three hundredths above a diffuse floor, the case the area sample serves worst (cos_l / d^2 under the
panel); spheres_sun: the sky with a sun over the stock spheres."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))


def _tests():
    """tests/test_gpu_mis.py, whose low_panel_scene this tool measures"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("t", os.path.join(ROOT, "tests", "test_gpu_mis.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    return t


def low_panel_scene(pkg):
    return _tests().low_panel_scene(pkg)


def cases(pkg):
    sun = pkg.json_parser.scene_from_json(os.path.join(ROOT, "assets", "scenes", "spheres_sun.json"))
    return (("cornell_lit(with_mesh)", pkg.scenes.cornell_lit(resolution=(1280, 720), with_mesh=True), (1280, 720), None, True, False),
            ("spheres_sun.json", sun, tuple(sun.resolution), sun.environment, False, True),
            ("low_panel_scene", low_panel_scene(pkg), (1280, 720), None, True, False))


def tracers_of(pkg, flat, size, env, direct, env_light, mb):
    out = []
    for mode in (0, 1):
        pt = pkg.PathTracer(device=0, max_bounces=mb)
        pt.current_gpu_method = pkg.GPUMethod.megakernel
        pt.direct_light, pt.environment_light, pt.mis = direct, env_light, bool(mode)
        pt.environment = env
        pt.create_buffers(size, flat)
        out.append(pt)
    return out


def time_ratio(pkg, name, scene, size, env, direct, env_light, n, repeats, mb=8):
    flat = scene.build_scene(distinct_meshes=True)
    tracers = tracers_of(pkg, flat, size, env, direct, env_light, mb)

    def run(pt, n):
        pt.restart()
        pt.max_iterations = n
        pt.synchronize()
        before = pt.stats()["rays_total"]
        t0 = time.perf_counter()
        for _ in range(n):
            pt.path_trace(scene.camera)
        pt.synchronize()
        return (time.perf_counter() - t0) * 1e3, pt.stats()["rays_total"] - before

    warm = [run(pt, n)[0] for pt in tracers]  # warm-up; then a window of at least half a second for the slower mode
    n = min(16384, max(n, int(n * 500.0 / max(warm)) + 1))
    ms, rays = [[], []], [0, 0]
    for _ in range(repeats):
        for mode, pt in enumerate(tracers):
            took, rays[mode] = run(pt, n)
            ms[mode].append(took / n)
    loop = (tracers[1].direct_loop_stats(), tracers[1].environment_light_loop_stats(), tracers[1].mis_loop_stats())
    for pt in tracers:
        pt.close()
    med = [statistics.median(v) for v in ms]
    print(f"{name} {size[0]} x {size[1]}, {mb} bounces, megakernel, direct_light {int(direct)}, environment_light {int(env_light)}, "
          f"{n} iterations per repeat, {repeats} alternating repeats")
    for mode in (0, 1):
        spread = (max(ms[mode]) - min(ms[mode])) / med[mode]
        print(f"  mis {mode}: {med[mode]:.4f} ms per iteration (median; repeats {' '.join(f'{x:.4f}' for x in ms[mode])}; spread "
              f"{100 * spread:.1f} %), {rays[mode]} rays per repeat")
    print(f"  mis 1 per repeat: {loop[0]['shadow_rays']} lamp shadow rays, {loop[1]['shadow_rays']} environment shadow rays, "
          f"{loop[2]['weighted_emitter_hits']} weighted emitter hits, {loop[2]['weighted_misses']} weighted misses")
    print(f"  time ratio (1 / 0): {med[1] / med[0]:.3f}")
    return med[1] / med[0]


def variance(pkg, name, scene, size, env, direct, env_light, ratio, blocks=16, per_block=256, mb=8):
    flat = scene.build_scene(distinct_meshes=True)
    tracers = tracers_of(pkg, flat, size, env, direct, env_light, mb)
    counts = (per_block, max(1, round(per_block / ratio)))
    means = np.zeros((2, blocks, 3))
    start, bad = [0, 0], [0, 0]  # bad: pixels of a block whose mean is not finite, left out of that block's image mean
    for b in range(blocks):
        for mode, pt in enumerate(tracers):
            pt.resize_image(size)
            pt.restart()
            pt.set_iteration(start[mode])
            # the running mean after k iterations that began at iteration s with cleared buffers holds (sum of the samples) / (s + k)
            pt.max_iterations = start[mode] + counts[mode]
            for _ in range(counts[mode]):
                pt.path_trace(scene.camera)
            scale = (start[mode] + counts[mode]) / counts[mode]
            color = pt.download("color").astype(np.float64).reshape(-1, 3)
            finite = np.isfinite(color).all(axis=1)
            bad[mode] += int((~finite).sum())
            means[mode, b] = color[finite].mean(axis=0) * scale
            start[mode] += counts[mode]
    for pt in tracers:
        pt.close()
    print(f"{name} {size[0]} x {size[1]}, {mb} bounces: {blocks} blocks per mode, {counts[0]} iterations a block with mis 0, {counts[1]} with mis 1 "
          f"(equal time at the time ratio {ratio:.3f}); pixels left out as not finite: {bad[0]} / {bad[1]}")
    for c, ch in enumerate("rgb"):
        v0, v1 = means[0, :, c].var(ddof=1), means[1, :, c].var(ddof=1)
        print(f"  {ch}: mean {means[0, :, c].mean():.5f} / {means[1, :, c].mean():.5f}, variance of the block means {v0:.3e} / {v1:.3e}: "
              f"mis 1 / mis 0 = {v1 / v0:.3f}")


def cpu(pkg, orc):
    """the restatement's block means on low_panel_scene, 24 x 16, 16 blocks of 8 iterations per mode: the ratio of spreads"""
    import loop_ref
    scene = low_panel_scene(pkg)
    flat = scene.build_scene(distinct_meshes=True)
    sh = orc.SceneHandle(flat)
    means = np.zeros((2, 16, 3))
    for mode in (0, 1):
        for b in range(16):
            r = loop_ref.render_megakernel(orc, flat, scene.camera, 24, 16, 8 * b, 8, 8, direct=True, mis=bool(mode), scene_handle=sh)
            means[mode, b] = r["color"].astype(np.float64).reshape(-1, 3).mean(axis=0) * (b + 1)
    sd = means.std(axis=1, ddof=1)
    print("low_panel_scene on the restatement, 24 x 16, 8 bounces, 16 blocks of 8 iterations: image mean", means.mean(axis=1)[0], "/",
          means.mean(axis=1)[1], "spread of the block means", sd[0], "/", sd[1], "ratio of spreads (mis 1 / mis 0)", sd[1] / sd[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--variance-only", action="store_true")
    args = ap.parse_args()
    import __graft_entry__ as graft
    pkg = graft.load_package()
    if args.cpu:
        return cpu(pkg, graft.load_oracle())
    for name, scene, size, env, direct, env_light in (() if args.variance_only else cases(pkg)):
        time_ratio(pkg, name, scene, size, env, direct, env_light, args.iterations, args.repeats)
    small = (160, 120)
    sun = pkg.json_parser.scene_from_json(os.path.join(ROOT, "assets", "scenes", "spheres_sun.json"))
    for name, scene, env, direct, env_light in (("low_panel_scene", low_panel_scene(pkg), None, True, False),
                                                ("spheres_sun.json", sun, sun.environment, False, True)):
        ratio = time_ratio(pkg, name, scene, small, env, direct, env_light, 256, 3)
        variance(pkg, name, scene, small, env, direct, env_light, ratio)


if __name__ == "__main__":
    main()
