#!/usr/bin/env python3
"""tools/env_ab.py -- what environment lighting costs; profiles/environment.txt holds its output.

    tools/env_ab.py [--iterations N] [--repeats R] [--size S]

scenes.heightfield_scene (the benchmark's scene: the 1,000,000-triangle heightfield under an open sky) at 1920 x 1080, max_bounces 8,
streaming method, and an S x S (default 1024) octahedral map of a procedural sky: a horizon glow, a darker zenith, a broad sun.  Two
contexts, environment off and on; after a warm-up of both, R repeats ALTERNATING between them: N iterations from a restart, wall clock
around the ptc_trace calls and the synchronise that ends them; ms per iteration = the median repeat / N, with the repeats and their
spread beside it, and rays_total per repeat (an environment changes only colour: the counts must be equal)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def sky_map(n):
    """[n, n, 3] float32: the texel centres' directions by the inverse of the octahedral chart, a smooth sky there"""
    k = (np.arange(n) + 0.5) / n * 2.0 - 1.0
    qx, qz = np.meshgrid(k, k)  # row j along z, column i along x
    y = 1.0 - np.abs(qx) - np.abs(qz)
    lower = y < 0.0
    x = np.where(lower, (1.0 - np.abs(qz)) * np.where(qx < 0, -1.0, 1.0), qx)
    z = np.where(lower, (1.0 - np.abs(qx)) * np.where(qz < 0, -1.0, 1.0), qz)
    d = np.stack([x, y, z], axis=-1)
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    up = np.clip(d[..., 1], 0.0, 1.0)[..., None]
    base = np.array([0.9, 0.8, 0.7]) * (1.0 - up) + np.array([0.2, 0.4, 0.9]) * up
    base = np.where(d[..., 1:2] < 0.0, np.array([0.15, 0.13, 0.1]), base)
    sun = np.array([0.5, 0.6, -0.62])
    sun /= np.linalg.norm(sun)
    glow = np.clip(d @ sun, 0.0, 1.0)[..., None] ** 64
    return (base + 20.0 * glow * np.array([1.0, 0.9, 0.7])).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--size", type=int, default=1024)
    args = ap.parse_args()
    import __graft_entry__ as graft
    pkg = graft.load_package()
    w, h, n = 1920, 1080, args.iterations
    print(f"heightfield_scene, {w} x {h}, max_bounces 8, streaming, {n} iterations per repeat, {args.repeats} alternating repeats, "
          f"environment off against on ({args.size} x {args.size} texels)")
    scene = pkg.scenes.heightfield_scene((w, h))
    flat = scene.build_scene()
    tracers = []
    for on in (False, True):
        pt = pkg.PathTracer(device=0, max_bounces=8)
        if on:
            pt.environment = sky_map(args.size)
        pt.create_buffers((w, h), flat)
        pt.max_iterations = n
        tracers.append(pt)

    def run(pt):
        pt.restart()
        pt.synchronize()
        before = pt.stats()["rays_total"]  # (ptc_restart does not reset the count: the repeat's own rays are the difference)
        t0 = time.perf_counter()
        for _ in range(n):
            pt.path_trace(scene.camera)
        pt.synchronize()
        return (time.perf_counter() - t0) * 1e3, pt.stats()["rays_total"] - before

    for pt in tracers:
        run(pt)  # warm-up
    ms, rays = [[], []], [0, 0]
    for _ in range(args.repeats):
        for mode, pt in enumerate(tracers):
            took, rays[mode] = run(pt)
            ms[mode].append(took / n)
    for pt in tracers:
        pt.close()
    med = [statistics.median(v) for v in ms]
    for mode, label in enumerate(("off", "on ")):
        spread = (max(ms[mode]) - min(ms[mode])) / med[mode]
        print(f"  environment {label}: {med[mode]:.3f} ms per iteration (median; repeats {' '.join(f'{x:.3f}' for x in ms[mode])}; spread "
              f"{100 * spread:.1f} %), {rays[mode]} rays per repeat, {rays[mode] / n / med[mode] / 1e3:.0f} Mrays/s")
    print(f"  time ratio (on / off): {med[1] / med[0]:.3f}, rays ratio: {rays[1] / rays[0]:.3f}")


if __name__ == "__main__":
    main()
