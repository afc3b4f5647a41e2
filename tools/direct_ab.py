#!/usr/bin/env python3
"""tools/direct_ab.py -- what the direct-light query costs next to the occlusion walk it feeds, a fixed
workload in the style of occlusion_ab.py.

    tools/direct_ab.py [--points N] [--repeats R]                 the workload; one JSON line per scene
    tools/direct_ab.py --summarise <rocpd .db> [--repeats R]      per-scene kernel sums of a rocprofv3 --kernel-trace run of it

Scenes: "cornell" = scenes.cornell_lit(with_mesh=True); "terrain" = config 3's scene (1,000,000-triangle heightfield + three
spheres) with a panel lamp added above the terrain.  Points: 4,147,200 (two 1080p frames' worth) surface points and face-forward
normals from ptc_intersect_rays primary hits of a pinhole camera at the scene's view point (two jittered rays per pixel; rays that
miss are replaced by repeating hits).  Per scene, after a warm-up of every path: R times ptc_direct_light (host arrays, rays and
visibility asked for) alternating with ptc_occluded_rays on the very rays that call produced -- every repeat checks
visible == generated and not occluded on every point, a mismatch prints AGREEMENT FAILED instead of numbers -- then R
device-pointer calls on torch tensors (wall clock: no host copies in it).  Times printed here: wall clock and the HIP events
around the launches (ptc_direct_stats.kernel_ms: sample + occlusion + resolve; ptc_occlusion_stats.kernel_ms: the occlusion
launches of the stand-alone call).  Kernel times proper come from a rocprofv3 run of this program and --summarise:
k_light_sample + k_light_resolve next to the k_occlude* dispatches of the same call and of the stand-alone call."""
import argparse
import json
import os
import sqlite3
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SCENES = ("cornell", "terrain")
SAMPLE_INDEX = 1


def spread_of(v):
    return (max(v) - min(v)) / (sum(v) / len(v)) if v and sum(v) else 0.0


def build_scene(pkg, name):
    """-> (FlatScene, eye, look-at point, vertical field of view in degrees)"""
    if name == "cornell":
        return pkg.scenes.cornell_lit((1920, 1080), with_mesh=True).build_scene(), (0.0, 0.0, 4.0), (0.0, -0.1, 0.0), 45.0
    s = pkg.scenes.heightfield_scene((1920, 1080))
    s.add_material("panel", pkg.EmissiveMaterial((6.0, 6.0, 5.5)))
    panel = s.add_mesh("models/light_panel.obj", pkg.scenes.light_panel_mesh(-1.0, 1.0, -0.5, 0.5, 2.5))
    s.add_object(panel, pkg.glmlite.identity(), "panel")
    return s.build_scene(distinct_meshes=True), (0.0, 2.5, 5.0), (0.0, 0.0, 0.0), 50.0


def surface_points(np, pt, n, eye, at, vfov_deg, seed):
    """n points on the scene's surfaces as a camera sees them: primary hits of ptc_intersect_rays."""
    rng = np.random.default_rng(seed)
    w, h = 1920, 1080
    per_pixel = -(-n // (w * h))
    eye, at = np.asarray(eye, dtype=np.float64), np.asarray(at, dtype=np.float64)
    fwd = (at - eye) / np.linalg.norm(at - eye)
    right = np.cross(fwd, (0.0, 1.0, 0.0))
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    half_h = np.tan(np.radians(vfov_deg) / 2.0)
    half_w = half_h * w / h
    px = np.tile(np.arange(w * h), per_pixel)[:max(n, w * h)]
    x = ((px % w) + rng.uniform(size=len(px))) / w * 2.0 - 1.0
    y = 1.0 - ((px // w) + rng.uniform(size=len(px))) / h * 2.0
    d = fwd[None, :] + (x * half_w)[:, None] * right[None, :] + (y * half_h)[:, None] * up[None, :]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((len(px), 8), dtype=np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = eye, 1e-4, d, np.finfo(np.float32).max
    t, nrm, _, _ = pt.intersect_rays(rays)
    hit = t >= 0
    p = (rays[:, 0:3] + rays[:, 4:7] * t[:, None])[hit]
    nn = nrm[hit]
    back = np.sum(nn * rays[hit, 4:7], axis=1) > 0
    nn[back] = -nn[back]
    reps = -(-n // len(p))
    return np.tile(p, (reps, 1))[:n].astype(np.float32), np.tile(nn, (reps, 1))[:n].astype(np.float32), float(hit.mean())


def workload(n, repeats):
    import numpy as np
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    ok = True
    for name in SCENES:
        flat, eye, at, vfov = build_scene(pkg, name)
        with pkg.PathTracer() as pt:
            pt.create_buffers((64, 64), flat)
            pts, nrm, hit_share = surface_points(np, pt, n, eye, at, vfov, seed=9)
            pt.set_profiling(True, False)
            dev = torch.device("cuda:0")
            t_pts, t_nrm = torch.from_numpy(pts).to(dev), torch.from_numpy(nrm).to(dev)
            t_rad = torch.zeros((n, 3), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            # warm-up: code objects, allocations, every path
            _, rays, _ = pt.direct_light(pts, nrm, SAMPLE_INDEX, want_rays=True)
            pt.occluded_rays(rays)
            pt.direct_light_dev(t_pts.data_ptr(), t_nrm.data_ptr(), n, SAMPLE_INDEX, t_rad.data_ptr())
            r = {"direct_wall_ms": [], "direct_event_ms": [], "occlude_wall_ms": [], "occlude_event_ms": [], "redone": [], "dev_wall_ms": [],
                 "dev_event_ms": []}
            agree = True
            for _ in range(repeats):
                d0 = pt.direct_stats()
                t0 = time.perf_counter()
                radiance, rays, visible = pt.direct_light(pts, nrm, SAMPLE_INDEX, want_rays=True)
                r["direct_wall_ms"].append(1e3 * (time.perf_counter() - t0))
                d1 = pt.direct_stats()
                r["direct_event_ms"].append(d1["kernel_ms"] - d0["kernel_ms"])
                o0 = pt.occlusion_stats()
                t0 = time.perf_counter()
                occ = pt.occluded_rays(rays)
                r["occlude_wall_ms"].append(1e3 * (time.perf_counter() - t0))
                o1 = pt.occlusion_stats()
                r["occlude_event_ms"].append(o1["kernel_ms"] - o0["kernel_ms"])
                r["redone"].append(o1["redone"] - o0["redone"])
                made = rays[:, 7] > 0
                agree = agree and bool(np.array_equal(visible, (made & (occ == 0)).astype(np.uint8)))
                agree = agree and d1["sampled"] - d0["sampled"] == int(made.sum()) and d1["unoccluded"] - d0["unoccluded"] == int(visible.sum())
            for _ in range(repeats):
                d0 = pt.direct_stats()
                t0 = time.perf_counter()
                pt.direct_light_dev(t_pts.data_ptr(), t_nrm.data_ptr(), n, SAMPLE_INDEX, t_rad.data_ptr())
                r["dev_wall_ms"].append(1e3 * (time.perf_counter() - t0))
                r["dev_event_ms"].append(pt.direct_stats()["kernel_ms"] - d0["kernel_ms"])
            agree = agree and bool(np.array_equal(t_rad.cpu().numpy(), radiance))
            info = pt.light_info()
        if not agree:
            ok = False
            print("%s: AGREEMENT FAILED -- visible != generated and not occluded, or the device call's bytes differ; numbers void" % name,
                  flush=True)
            continue
        out = {"scene": name, "points": n, "repeats": repeats, "library": os.environ.get("PTCORE_LIB", "default"), "lights": info["lights"],
               "primary_hit_share": round(hit_share, 4), "sampled_share": round(float(made.mean()), 4),
               "visible_share": round(float(visible.mean()), 4), "redone": r["redone"][-1]}
        for k in ("direct_event_ms", "occlude_event_ms", "dev_event_ms"):
            out[k] = [round(x, 3) for x in r[k]]
            out[k.replace("_ms", "_spread")] = round(spread_of(r[k]), 4)
        for k in ("direct_wall_ms", "occlude_wall_ms", "dev_wall_ms"):
            out[k] = [round(x, 1) for x in r[k]]
        out["agree"] = True
        print(json.dumps(out), flush=True)
    return 0 if ok else 1


def summarise(db, repeats):
    """Dispatches in start order.  k_light_sample opens a direct-light call and k_light_resolve closes it; k_occlude* dispatches
    inside belong to it, a run of them outside is one stand-alone ptc_occluded_rays call.  Per scene the program makes
    1 + R + 1 + R direct-light calls (warm-up, host repeats, device warm-up, device repeats) and 1 + R stand-alone calls."""
    c = sqlite3.connect(db)
    rows = c.execute("select name, duration from kernels order by start").fetchall()
    direct, alone = [], []   # direct: [sample + resolve ms, occlusion ms]; alone: ms
    inside, last_alone = False, False
    for name, dur in rows:
        ms = dur / 1e6
        if "k_light_sample" in name:
            direct.append([ms, 0.0])
            inside, last_alone = True, False
        elif "k_light_resolve" in name:
            direct[-1][0] += ms
            inside = False
        elif "k_occlude" in name:
            if inside:
                direct[-1][1] += ms
            else:
                if not last_alone:
                    alone.append(0.0)
                alone[-1] += ms
                last_alone = True
            continue
        else:
            last_alone = False
    per_direct, per_alone = 2 + 2 * repeats, 1 + repeats
    print("# %s: %d direct-light calls, %d stand-alone occlusion calls" % (db, len(direct), len(alone)))
    if len(direct) != per_direct * len(SCENES) or len(alone) != per_alone * len(SCENES):
        print("# unexpected call counts: not the trace of this program with --repeats %d" % repeats)
        return 1
    for k, name in enumerate(SCENES):
        host = direct[k * per_direct + 1:k * per_direct + 1 + repeats]
        devc = direct[k * per_direct + 2 + repeats:(k + 1) * per_direct]
        occ = alone[k * per_alone + 1:(k + 1) * per_alone]
        for label, calls in (("host arrays", host), ("device pointers", devc)):
            sr, oc = [x[0] for x in calls], [x[1] for x in calls]
            print("%-8s %-15s k_light_sample + k_light_resolve ms: %s  mean %.3f spread %.1f %%" % (
                name, label, " ".join("%.3f" % x for x in sr), sum(sr) / len(sr), 100 * spread_of(sr)))
            print("%-8s %-15s k_occlude* of the same call ms:      %s  mean %.3f spread %.1f %%   ratio %.3f" % (
                name, label, " ".join("%.3f" % x for x in oc), sum(oc) / len(oc), 100 * spread_of(oc), sum(sr) / sum(oc)))
        print("%-8s %-15s k_occlude* of ptc_occluded_rays ms:  %s  mean %.3f spread %.1f %%" % (
            name, "same rays", " ".join("%.3f" % x for x in occ), sum(occ) / len(occ), 100 * spread_of(occ)))
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", type=int, default=4147200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--summarise")
    a = ap.parse_args()
    return summarise(a.summarise, a.repeats) if a.summarise else workload(a.points, a.repeats)


if __name__ == "__main__":
    sys.exit(main())
