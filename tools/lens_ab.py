#!/usr/bin/env python3
"""tools/lens_ab.py -- what the thin lens costs; profiles/lens.txt holds its output.

    tools/lens_ab.py [--iterations N] [--repeats R]

Two scenes at 1280 x 720, max_bounces 8, streaming method: assets/scenes/cornell_dof.json (spheres only; its own lens) and
scenes.heightfield_scene (the 1,000,000-triangle heightfield: bounce 0 opens with a traversal launch over one mesh object, so a
pinhole frame gets entry points, "beam", and a lens frame does not -- the line that shows what losing them costs; lens 0.05 / 4).
Per scene two contexts, lens off and on; after a warm-up of both, R repeats ALTERNATING between them: N iterations from a restart,
wall clock around the ptc_trace calls and the synchronise that ends them; ms per iteration = the median repeat / N, with the repeats
and their spread beside it, and rays_total per repeat (a lens frame traces other rays: the counts differ)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import __graft_entry__ as graft
    pkg = graft.load_package()
    w, h, n = 1280, 720, args.iterations
    print(f"{w} x {h}, max_bounces 8, streaming, {n} iterations per repeat, {args.repeats} alternating repeats, lens off against on")
    dof = pkg.json_parser.scene_from_json(os.path.join(ROOT, "assets", "scenes", "cornell_dof.json"))
    timing(pkg, "cornell_dof", dof, (dof.camera.lens_radius, dof.camera.focus_distance), w, h, n, args.repeats)
    timing(pkg, "heightfield_scene", pkg.scenes.heightfield_scene((w, h)), (0.05, 4.0), w, h, n, args.repeats)


def timing(pkg, name, scene, lens, w, h, n, repeats):
    flat = scene.build_scene()
    tracers = []
    for on in (False, True):
        pt = pkg.PathTracer(device=0, max_bounces=8)
        if on:
            pt.lens = lens
        pt.create_buffers((w, h), flat)
        pt.max_iterations = n
        tracers.append(pt)

    def run(pt):
        pt.restart()
        pt.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            pt.path_trace(scene.camera)
        pt.synchronize()
        return (time.perf_counter() - t0) * 1e3, pt.stats()["rays_total"]

    for pt in tracers:
        run(pt)  # warm-up
    ms, rays = [[], []], [0, 0]
    for _ in range(repeats):
        for mode, pt in enumerate(tracers):
            took, rays[mode] = run(pt)
            ms[mode].append(took / n)
    for pt in tracers:
        pt.close()
    med = [statistics.median(v) for v in ms]
    print(f"{name}, lens {lens[0]:g} / {lens[1]:g}")
    for mode, label in enumerate(("off", "on ")):
        spread = (max(ms[mode]) - min(ms[mode])) / med[mode]
        print(f"  lens {label}: {med[mode]:.3f} ms per iteration (median; repeats {' '.join(f'{x:.3f}' for x in ms[mode])}; spread "
              f"{100 * spread:.1f} %), {rays[mode]} rays per repeat, {rays[mode] / n / med[mode] / 1e3:.0f} Mrays/s")
    print(f"  time ratio (on / off): {med[1] / med[0]:.3f}, rays ratio: {rays[1] / rays[0]:.3f}")


if __name__ == "__main__":
    main()
