#!/usr/bin/env python3
"""tools/occlusion_ab.py -- any-hit against closest-hit on the same rays, a fixed workload in the style of
run_frames.py.

    tools/occlusion_ab.py [--rays N] [--repeats R]            the workload; one JSON line per ray set
    tools/occlusion_ab.py --summarise <rocpd .db> [--repeats R]   per-set kernel sums of a rocprofv3 --kernel-trace run of it

Scene: config 3 (1,000,000-triangle heightfield + three spheres).  Rays: 4,147,200 (two 1080p bounces' worth) seeded
origins a hair above the terrain, as two sets -- "shadow": towards a point light, t_max = the distance; "spread": the same
origins with cosine-spread directions, t_max = FLT_MAX (tests/occlusion_rays.py: terrain_rays).  After a warm-up of both
paths on both sets, ptc_occluded_rays and ptc_intersect_rays alternate R times per set in one process.  Every repeat
compares occluded == (t >= 0) on every ray; a mismatch prints AGREEMENT FAILED instead of a number (as ab.py's parity leg).
Times printed here: wall clock of the calls (host packing and copies included) and, for the any-hit call, the HIP events
around its launches (ptc_occlusion_stats.kernel_ms).  Kernel times proper come from a rocprofv3 run of this program and
--summarise: k_occlude* against k_spheres + k_traverse4* + k_tail_count, per set and repeat."""
import argparse
import json
import os
import sqlite3
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SETS = ("shadow", "spread")
WARMUP = len(SETS)   # calls of each kind before the timed ones


def spread_of(v):
    return (max(v) - min(v)) / (sum(v) / len(v)) if v else 0.0


def workload(n, repeats):
    import numpy as np
    import __graft_entry__ as g
    import occlusion_rays as R
    pkg = g.load_package()
    scene = pkg.scenes.heightfield_scene((1920, 1080))
    flat = scene.build_scene()
    flat.bvh, _ = pkg.bvh_from_mesh(list(scene.mesh_map_.values())[0])
    rays = dict(zip(SETS, R.terrain_rays(pkg, n)))
    ok = True
    with pkg.PathTracer() as pt:
        pt.create_buffers((64, 64), flat)
        pt.set_profiling(True, False)
        for name in SETS:                       # warm-up: code objects, allocations, both paths, both sets (alternating, as below)
            pt.occluded_rays(rays[name])
            pt.intersect_rays(rays[name])
        res = {name: {"any_wall_ms": [], "any_event_ms": [], "closest_wall_ms": [], "redone": []} for name in SETS}
        for _ in range(repeats):
            for name in SETS:
                r = res[name]
                before = pt.occlusion_stats()
                t0 = time.perf_counter()
                occ = pt.occluded_rays(rays[name])
                r["any_wall_ms"].append(1e3 * (time.perf_counter() - t0))
                after = pt.occlusion_stats()
                r["any_event_ms"].append(after["kernel_ms"] - before["kernel_ms"])
                r["redone"].append(after["redone"] - before["redone"])
                t0 = time.perf_counter()
                t = pt.intersect_rays(rays[name])[0]
                r["closest_wall_ms"].append(1e3 * (time.perf_counter() - t0))
                same = bool(np.array_equal(occ, (t >= 0).astype(np.uint8)))
                r["agree"] = r.get("agree", True) and same
                r["occluded_share"] = float(occ.mean())
    for name in SETS:
        r = res[name]
        if not r["agree"]:
            ok = False
            print("%s: AGREEMENT FAILED -- occluded != (closest hit found), numbers void" % name, flush=True)
            continue
        out = {"set": name, "rays": n, "repeats": repeats, "library": os.environ.get("PTCORE_LIB", "default"),
               "occluded_share": round(r["occluded_share"], 4), "redone": r["redone"][-1],
               "any_event_ms": [round(x, 3) for x in r["any_event_ms"]], "any_event_spread": round(spread_of(r["any_event_ms"]), 4),
               "any_wall_ms": [round(x, 1) for x in r["any_wall_ms"]], "closest_wall_ms": [round(x, 1) for x in r["closest_wall_ms"]],
               "agree": True}
        print(json.dumps(out), flush=True)
    return 0 if ok else 1


def summarise(db, repeats):
    """Dispatches in start order; a run of k_occlude* dispatches is one any-hit call, a run of k_spheres / k_traverse4* /
    k_tail_count dispatches one closest-hit call.  The first WARMUP calls of each kind are the warm-up; after that call i of a
    kind belongs to repeat i // 2, set i % 2."""
    c = sqlite3.connect(db)
    rows = c.execute("select name, duration from kernels order by start").fetchall()
    calls = {"any": [], "closest": []}
    last = None
    for name, dur in rows:
        base = name.replace("void ", "")
        kind = "any" if "k_occlude" in base else ("closest" if any(k in base for k in ("k_spheres", "k_traverse4", "k_tail_count")) else None)
        if kind is None:
            continue
        if kind != last:
            calls[kind].append(0.0)
        calls[kind][-1] += dur / 1e6
        last = kind
    print("# %s: %d any-hit calls, %d closest-hit calls (the first %d of each: warm-up)" % (db, len(calls["any"]), len(calls["closest"]), WARMUP))
    if len(calls["any"]) != WARMUP + repeats * len(SETS) or len(calls["closest"]) != len(calls["any"]):
        print("# unexpected call counts: not the trace of this program with --repeats %d" % repeats)
        return 1
    print("%-8s %-34s %-34s %8s %8s %8s" % ("set", "any-hit kernel ms per repeat", "closest-hit kernel ms per repeat", "any", "closest", "ratio"))
    for k, name in enumerate(SETS):
        a = [calls["any"][WARMUP + r * len(SETS) + k] for r in range(repeats)]
        b = [calls["closest"][WARMUP + r * len(SETS) + k] for r in range(repeats)]
        ma, mb = sum(a) / len(a), sum(b) / len(b)
        print("%-8s %-34s %-34s %8.3f %8.3f %8.3f   spread any %.1f %% closest %.1f %%" % (
            name, " ".join("%.3f" % x for x in a), " ".join("%.3f" % x for x in b), ma, mb, ma / mb, 100 * spread_of(a), 100 * spread_of(b)))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rays", type=int, default=4147200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--summarise")
    a = ap.parse_args()
    return summarise(a.summarise, a.repeats) if a.summarise else workload(a.rays, a.repeats)


if __name__ == "__main__":
    sys.exit(main())
