#!/usr/bin/env python3
"""tools/smooth_ab.py -- what smooth shading in the megakernel costs; profiles/smooth.txt holds its output.

    tools/smooth_ab.py [--iterations N] [--repeats R]     the frame time of assets/scenes/cornell_mesh.json, "smooth_normals" 0 and 1
    tools/smooth_ab.py --flat-only                        ... with 0 alone (what a tree without the parameter can run: the parent's figure)
    tools/smooth_ab.py --host                             no GPU: ptc_compute_vertex_normals on the benchmark's million-triangle heightfield

Time, section 5g's method: two contexts, "smooth_normals" 0 and 1 (the second with the host's vertex normals set), the scene at its own
resolution in the megakernel method, 8 bounces; after a warm-up of both, R repeats ALTERNATING between them: N iterations from a restart,
wall clock around the ptc_trace calls and the synchronise that ends them; ms per iteration = the median repeat / N, N raised after the
warm-up until a repeat lasts half a second."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frame_times(pkg, n, repeats, modes, mb=8):
    scene = pkg.json_parser.scene_from_json(os.path.join(ROOT, "assets", "scenes", "cornell_mesh.json"))
    flat = scene.build_scene()
    size = tuple(scene.resolution)
    tracers = []
    for mode in modes:
        pt = pkg.PathTracer(device=0, max_bounces=mb)
        pt.current_gpu_method = pkg.GPUMethod.megakernel
        pt.create_buffers(size, flat)
        if mode:
            pt.smooth_normals = True
            pt.vertex_normals = pkg.compute_vertex_normals(flat)
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
    stats = tracers[-1].smooth_loop_stats() if modes[-1] else None
    for pt in tracers:
        pt.close()
    med = [statistics.median(v) for v in ms]
    print(f"cornell_mesh.json {size[0]} x {size[1]}, {mb} bounces, megakernel, {n} iterations per repeat, {repeats} alternating repeats")
    for k, mode in enumerate(modes):
        spread = (max(ms[k]) - min(ms[k])) / med[k]
        print(f"  smooth_normals {mode}: {med[k]:.4f} ms per iteration (median; repeats {' '.join(f'{x:.4f}' for x in ms[k])}; spread {100 * spread:.1f} %)")
    if stats:
        print(f"  smooth_normals 1 per repeat: {stats}")
    if len(modes) == 2:
        print(f"  time ratio (1 / 0): {med[1] / med[0]:.3f}")


def host_normals(pkg, repeats=3):
    mesh = pkg.scenes.heightfield_mesh()
    took = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        n = pkg.compute_vertex_normals(mesh.positions, mesh.indices)
        took.append(time.perf_counter() - t0)
    print(f"ptc_compute_vertex_normals, heightfield_mesh(): {len(mesh.positions)} vertices, {len(mesh.indices) // 3} triangles: "
          f"{min(took):.4f} s (best of {repeats}: {' '.join(f'{t:.4f}' for t in took)}); {int((n != 0).any(axis=1).sum())} vertices with a normal")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--flat-only", action="store_true")
    ap.add_argument("--host", action="store_true")
    args = ap.parse_args()
    import __graft_entry__ as graft
    pkg = graft.load_package()
    if args.host:
        host_normals(pkg)
    else:
        frame_times(pkg, args.iterations, args.repeats, (0,) if args.flat_only else (0, 1))


if __name__ == "__main__":
    main()
