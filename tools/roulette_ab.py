#!/usr/bin/env python3
"""tools/roulette_ab.py -- what Russian roulette returns and costs; profiles/roulette.txt is its output.

    tools/roulette_ab.py [--iterations N] [--repeats R] [--roulette K] [--no-variance]

Time: scenes.cornell_lit(with_mesh=True) at 1280 x 720, max_bounces 8 and 32, under both methods.  Per setting two contexts,
roulette 0 and K (default 3); after a warm-up of both, R repeats ALTERNATING between them: N iterations from a restart, wall clock
around the ptc_trace calls and the synchronise that ends them; ms per iteration = the median repeat / N, with the repeats and
their spread beside it.  Recorded with it: rays_total per repeat (a ray = one closest-hit query) and the live paths per bounce of
the last frame (streaming: ptc_stats.last_live).
Variance: the statistical test's own blocks (tests/test_gpu_roulette.py, stat_blocks: the closed room with one small lamp, 32 x 24,
24 bounces, roulette 2, 16 blocks of 256 iterations per mode) -- per channel the variance of the block means with / without
roulette, the rays ratio, and (variance ratio) x (rays ratio): the variance per ray traced.  The time ratios are cornell_lit's, the
variance ratio the small-lamp room's: two scenes, not one workload."""
import argparse
import importlib.util
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))  # the test module below imports its helpers from there


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--roulette", type=int, default=3)
    ap.add_argument("--no-variance", action="store_true")
    args = ap.parse_args()
    import __graft_entry__ as graft
    pkg = graft.load_package()
    w, h, n = 1280, 720, args.iterations
    scene = pkg.scenes.cornell_lit(resolution=(w, h), with_mesh=True)
    flat = scene.build_scene()
    print(f"cornell_lit(with_mesh) {w} x {h}, {n} iterations per repeat, {args.repeats} alternating repeats, roulette 0 against {args.roulette}")
    for method in ("streaming", "megakernel"):
        for mb in (8, 32):
            timing(pkg, scene, flat, w, h, mb, n, args.repeats, method, args.roulette)
    if args.no_variance:
        return
    spec = importlib.util.spec_from_file_location("t", os.path.join(ROOT, "tests", "test_gpu_roulette.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    for method in ("streaming", "megakernel"):
        variance(pkg, t, method)


def timing(pkg, scene, flat, w, h, mb, n, repeats, method, k):
    tracers = []
    for mode in (0, k):
        pt = pkg.PathTracer(device=0, max_bounces=mb)
        pt.current_gpu_method = getattr(pkg.GPUMethod, method)
        pt.roulette = mode
        pt.create_buffers((w, h), flat)
        pt.max_iterations = n
        tracers.append(pt)

    def run(pt):
        pt.restart()
        pt.reset_profile()
        pt.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            pt.path_trace(scene.camera)
        pt.synchronize()
        took = (time.perf_counter() - t0) * 1e3
        st = pt.stats()
        return took, st["rays_total"], st["last_live"]

    for pt in tracers:
        run(pt)  # warm-up
    ms = [[], []]
    rays = [0, 0]
    live = [None, None]
    for _ in range(repeats):
        for mode, pt in enumerate(tracers):
            took, rays[mode], live[mode] = run(pt)
            ms[mode].append(took / n)
    for pt in tracers:
        pt.close()
    med = [statistics.median(v) for v in ms]
    print(f"{method}, max_bounces {mb}")
    for mode, name in enumerate((0, k)):
        spread = (max(ms[mode]) - min(ms[mode])) / med[mode]
        print(f"  roulette {name}: {med[mode]:.3f} ms per iteration (median; repeats {' '.join(f'{x:.3f}' for x in ms[mode])}; spread "
              f"{100 * spread:.1f} %), {rays[mode]} rays per repeat, {rays[mode] / n / med[mode] / 1e3:.0f} Mrays/s")
        if method == "streaming":
            print(f"    live paths per bounce, last frame: {' '.join(str(x) for x in live[mode])}")
    print(f"  time ratio ({k} / 0): {med[1] / med[0]:.3f}, rays ratio: {rays[1] / rays[0]:.3f}")


def variance(pkg, t, method):
    t0 = time.perf_counter()
    means, rays = t.stat_blocks(pkg, getattr(pkg.GPUMethod, method))
    ray_ratio = rays[1] / rays[0]
    print(f"small_lamp_room 32 x 24, {t.scenes.STAT_BOUNCES} bounces, {method}, roulette 0 / {t.STAT_K}, {t.STAT_BLOCKS} blocks of {t.STAT_PER_BLOCK} "
          f"iterations per mode ({time.perf_counter() - t0:.1f} s); rays {rays[0]} / {rays[1]}: ratio {ray_ratio:.3f}")
    for c, name in enumerate("rgb"):
        v0, v1 = means[0, :, c].var(ddof=1), means[1, :, c].var(ddof=1)
        d = means[1, :, c] - means[0, :, c]
        print(f"  {name}: mean {means[0, :, c].mean():.5f} / {means[1, :, c].mean():.5f}, mean(D) {d.mean():+.2e} (bound "
              f"{4.073 * d.std(ddof=1) / 4.0:.2e}), variance of the block means {v0:.3e} / {v1:.3e}: ratio (roulette / plain) {v1 / v0:.2f}, "
              f"per ray traced {v1 / v0 * ray_ratio:.2f}")


if __name__ == "__main__":
    main()
