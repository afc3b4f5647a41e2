#!/usr/bin/env python3
"""tools/texture_ab.py -- what image textures in the megakernel cost; profiles/textures.txt holds its output.

    tools/texture_ab.py [--iterations N] [--repeats R]     the frame time of assets/scenes/cornell_textured.json, "textures" 0 and 1
    tools/texture_ab.py --plain-only                       ... with 0 alone (what a tree without the parameter can run: the parent's figure;
                                                           the scene is read without its texture keys, which such a tree does not know)

The scene's own pictures and `vt` coordinates (PathTracer.load_scene_textures): a 16 x 16 sRGB bilinear checker on the diffuse box and
a 12 x 5 linear nearest picture on the metal one.
Time, section 5g's method: two contexts, "textures" 0 and 1, the scene at its own resolution in the megakernel method, 8 bounces; after a
warm-up of both, R repeats ALTERNATING between them: N iterations from a restart, wall clock around the ptc_trace calls and the
synchronise that ends them; ms per iteration = the median repeat / N, N raised after the warm-up until a repeat lasts half a second."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def read_scene(pkg, plain):
    """the asset; plain: a copy without the texture keys beside it in a temporary folder of the scenes' folder's depth"""
    path = os.path.join(ROOT, "assets", "scenes", "cornell_textured.json")
    if not plain:
        return pkg.json_parser.scene_from_json(path)
    import json
    import tempfile
    with open(path) as f:
        j = json.load(f)
    j.pop("textures", None)
    for m in j["materials"]:
        m.pop("texture", None)
    for s in j["surfaces"]:
        if "filename" in s:
            s["filename"] = os.path.normpath(os.path.join(os.path.dirname(path), s["filename"]))
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "plain.json"), "w") as f:
            json.dump(j, f)
        return pkg.json_parser.scene_from_json(os.path.join(d, "plain.json"))


def frame_times(pkg, n, repeats, modes, mb=8):
    scene = read_scene(pkg, plain=modes == (0,))
    flat = scene.build_scene()
    size = tuple(scene.resolution)
    tracers = []
    for mode in modes:
        pt = pkg.PathTracer(device=0, max_bounces=mb)
        pt.current_gpu_method = pkg.GPUMethod.megakernel
        pt.create_buffers(size, flat)
        if mode:
            pt.textures = True
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
    ms = [[] for _ in modes]
    for _ in range(repeats):
        for k, pt in enumerate(tracers):
            ms[k].append(run(pt, n) / n)
    stats = tracers[-1].texture_loop_stats() if modes[-1] else None
    for pt in tracers:
        pt.close()
    med = [statistics.median(v) for v in ms]
    print(f"cornell_textured.json {size[0]} x {size[1]}, {mb} bounces, megakernel, {n} iterations per repeat, {repeats} alternating repeats")
    for k, mode in enumerate(modes):
        spread = (max(ms[k]) - min(ms[k])) / med[k]
        print(f"  textures {mode}: {med[k]:.4f} ms per iteration (median; repeats {' '.join(f'{x:.4f}' for x in ms[k])}; spread {100 * spread:.1f} %)")
    if stats:
        print(f"  textures 1 per repeat of {n} iterations: {stats}; lookups per frame {stats['lookups'] / n:.0f}")
    if len(modes) == 2:
        print(f"  time ratio (1 / 0): {med[1] / med[0]:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--plain-only", action="store_true")
    args = ap.parse_args()
    import __graft_entry__ as graft
    pkg = graft.load_package()
    frame_times(pkg, args.iterations, args.repeats, (0,) if args.plain_only else (0, 1))


if __name__ == "__main__":
    main()
