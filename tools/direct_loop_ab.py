#!/usr/bin/env python3
"""tools/direct_loop_ab.py -- what direct lighting in the megakernel costs and buys; profiles/direct_loop.txt
is its output.

    tools/direct_loop_ab.py [--iterations N] [--repeats R] [--no-variance]
    tools/direct_loop_ab.py --self-shadow          no GPU: shadow rays blocked by the wall they start on, per room, on the CPU oracle

Time: scenes.cornell_lit(with_mesh=True) at 1280 x 720, 8 bounces, the megakernel method.  Two contexts, direct_light 0 and 1;
after a warm-up of both, R repeats ALTERNATING between them: N iterations from a restart, wall clock around the ptc_trace calls
and the synchronise that ends them (DESIGN section 6's definitions: a ray = one closest-hit query, so Mrays/s counts the path's
own rays in both modes and the shadow rays in neither); ms per iteration = the median repeat / N.
Variance: the statistical test's own blocks (tests/test_gpu_direct_loop.py, stat_blocks: the closed room with one small lamp,
32 x 24, 16 blocks of 256 iterations per mode) -- per channel the variance of the block means without / with direct light.
The quotient (variance ratio) / (time ratio) is the variance reduction per unit of time.  The time ratio is cornell_lit's, the
variance ratio the small-lamp room's: two scenes, not one workload.  The same blocks are then run on the room built from the
stock scenes' radius-1000 wall spheres, where the shadow epsilon self-shadows (--self-shadow counts it): a record, not a test."""
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
    ap.add_argument("--no-variance", action="store_true")
    ap.add_argument("--self-shadow", action="store_true")
    args = ap.parse_args()
    import __graft_entry__ as graft
    pkg = graft.load_package()
    spec = importlib.util.spec_from_file_location("t", os.path.join(ROOT, "tests", "test_gpu_direct_loop.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    if args.self_shadow:
        return self_shadow(pkg, graft.load_oracle())
    w, h, mb, n = 1280, 720, 8, args.iterations
    scene = pkg.scenes.cornell_lit(resolution=(w, h), with_mesh=True)
    flat = scene.build_scene()
    tracers = []
    for mode in (0, 1):
        pt = pkg.PathTracer(device=0, max_bounces=mb)
        pt.current_gpu_method = pkg.GPUMethod.megakernel
        pt.direct_light = bool(mode)
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
        return (time.perf_counter() - t0) * 1e3, pt.stats()["rays_total"]

    for pt in tracers:
        run(pt)  # warm-up
    ms = [[], []]
    rays = [0, 0]
    for _ in range(args.repeats):
        for mode, pt in enumerate(tracers):
            took, rays[mode] = run(pt)
            ms[mode].append(took / n)
    loop = tracers[1].direct_loop_stats()
    for pt in tracers:
        pt.close()
    med = [statistics.median(v) for v in ms]
    print(f"cornell_lit(with_mesh) {w} x {h}, {mb} bounces, megakernel, {n} iterations per repeat, {args.repeats} alternating repeats")
    for mode in (0, 1):
        spread = (max(ms[mode]) - min(ms[mode])) / med[mode]
        print(f"  direct_light {mode}: {med[mode]:.3f} ms per iteration (median; repeats {' '.join(f'{x:.3f}' for x in ms[mode])}; spread "
              f"{100 * spread:.1f} %), {rays[mode]} rays per repeat, {rays[mode] / n / med[mode] / 1e3:.0f} Mrays/s")
    print(f"  direct_light 1 per repeat: {loop['diffuse_hits']} diffuse hits, {loop['shadow_rays']} shadow rays, {loop['unoccluded']} unoccluded")
    time_ratio = med[1] / med[0]
    print(f"  time ratio (1 / 0): {time_ratio:.3f}")
    if args.no_variance:
        return
    for room in (t.scenes.small_lamp_room, t.scenes.small_lamp_sphere_room):
        variance(pkg, t, room, time_ratio)


def variance(pkg, t, room, time_ratio):
    t0 = time.perf_counter()
    means, geometry = t.stat_blocks(pkg, room=room)
    print(f"{room.__name__} 32 x 24, {t.scenes.STAT_BOUNCES} bounces, 16 blocks of 256 iterations per mode ({time.perf_counter() - t0:.1f} s); "
          f"normal / depth equal in every block: {all(geometry)}")
    for c, name in enumerate("rgb"):
        v0, v1 = means[0, :, c].var(ddof=1), means[1, :, c].var(ddof=1)
        d = means[1, :, c] - means[0, :, c]
        print(f"  {name}: mean {means[0, :, c].mean():.5f} / {means[1, :, c].mean():.5f}, mean(D) {d.mean():+.2e} (bound "
              f"{4.073 * d.std(ddof=1) / 4.0:.2e}), variance of the block means {v0:.3e} / {v1:.3e}: ratio {v0 / v1:.1f}, "
              f"per unit of time {v0 / v1 / time_ratio:.1f}")


def self_shadow(pkg, orc):
    """Per room: 4 iterations of the restatement at 32 x 24, every sampled shadow ray once more through the oracle's closest hit;
    a hit within 0.05 of the origin is the wall the ray starts on (the rooms are convex: nothing else is that near on the way to
    the lamp)."""
    import numpy as np

    import direct_loop_scenes as scenes
    import loop_ref
    for room in (scenes.small_lamp_room, scenes.small_lamp_sphere_room):
        scene = room(pkg)
        flat = scene.build_scene()
        sh = orc.SceneHandle(flat)
        record = []
        loop_ref.render_megakernel(orc, flat, scene.camera, 32, 24, 0, 4, scenes.STAT_BOUNCES, direct=True, scene_handle=sh, record=record)
        rays = near = 0
        light = lost = 0.0
        for e in (e for e in record if e["kind"] == "light"):
            sel = np.nonzero(e["sample"]["sampled"])[0]
            if len(sel) == 0:
                continue
            recs, hit = orc.intersect_rays(flat, e["sample"]["rays"][sel], scene_handle=sh)
            own = (hit != 0) & (recs["t"] < 0.05)
            far = (hit != 0) & ~own   # the lamp's own far side
            c = e["sample"]["contribution"][sel].sum(axis=1)
            rays += len(sel)
            near += int(own.sum())
            light += float(c[~far].sum())
            lost += float(c[own].sum())
        print(f"{room.__name__}: {rays} shadow rays, {near} blocked within 0.05 of their origin ({100.0 * near / rays:.2f} %), "
              f"carrying {100.0 * lost / light:.2f} % of the unshadowed contribution that is not on the lamp's far side")


if __name__ == "__main__":
    main()
