#!/usr/bin/env python3
"""tools/normal_map_ab.py -- what normal maps in the megakernel cost; profiles/normal_maps.txt holds its output.

    tools/normal_map_ab.py [--iterations N] [--repeats R]     the frame time of assets/scenes/cornell_bumpy.json, "normal_maps" 0 and 1

The scene's own pictures, map and `vt` coordinates (PathTracer.load_scene_textures): cornell_textured.json's two boxes, both under the
32 x 32 bilinear ripple map beside their colour textures; "textures" is 1 in both contexts, as the scene says.  With "normal_maps" 0
the frame is cornell_textured.json's (the scene without the new keys is that file): tools/texture_ab.py's "textures 1" figure, on
this tree and on its parent, is the other half of the comparison.
Time, tools/texture_ab.py's method: two contexts, "normal_maps" 0 and 1, the scene at its own resolution in the megakernel method, 8
bounces; after a warm-up of both, R repeats ALTERNATING between them: N iterations from a restart, wall clock around the ptc_trace
calls and the synchronise that ends them; ms per iteration = the median repeat / N, N raised after the warm-up until a repeat lasts half
a second."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frame_times(pkg, n, repeats, mb=8):
    scene = pkg.json_parser.scene_from_json(os.path.join(ROOT, "assets", "scenes", "cornell_bumpy.json"))
    flat = scene.build_scene()
    size = tuple(scene.resolution)
    tracers = []
    for mode in (0, 1):
        pt = pkg.PathTracer(device=0, max_bounces=mb)
        pt.current_gpu_method = pkg.GPUMethod.megakernel
        pt.create_buffers(size, flat)
        pt.textures = True
        pt.normal_maps = bool(mode)
        pt.load_scene_textures(flat)
        tracers.append(pt)

    def run(pt, n):
        pt.restart()
        pt.max_iterations = n
        pt.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            pt.path_trace(scene.camera)
        pt.synchronize()
        return (time.perf_counter() - t0) * 1e3

    warm = [run(pt, n) for pt in tracers]
    n = min(16384, max(n, int(n * 500.0 / max(warm)) + 1))
    ms = [[], []]
    for _ in range(repeats):
        for k, pt in enumerate(tracers):
            ms[k].append(run(pt, n) / n)
    stats = [{**pt.normal_map_loop_stats(), "lookups": pt.texture_loop_stats()["lookups"],
              **{k: pt.smooth_loop_stats()[k] for k in ("absorbed", "culled_light_samples")}} for pt in tracers]
    for pt in tracers:
        pt.close()
    med = [statistics.median(v) for v in ms]
    print(f"cornell_bumpy.json {size[0]} x {size[1]}, {mb} bounces, megakernel, {n} iterations per repeat, {repeats} alternating repeats")
    for mode in (0, 1):
        spread = (max(ms[mode]) - min(ms[mode])) / med[mode]
        print(f"  normal_maps {mode}: {med[mode]:.4f} ms per iteration (median; repeats {' '.join(f'{x:.4f}' for x in ms[mode])}; spread {100 * spread:.1f} %)")
        print(f"    counters of the last repeat, per frame: " + ", ".join(f"{k} {v / n:.0f}" for k, v in stats[mode].items()))
    print(f"  time ratio (1 / 0): {med[1] / med[0]:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import __graft_entry__ as graft
    frame_times(graft.load_package(), args.iterations, args.repeats)


if __name__ == "__main__":
    main()
