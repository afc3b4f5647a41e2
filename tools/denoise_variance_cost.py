#!/usr/bin/env python3
"""tools/denoise_variance_cost.py -- what a ptc_denoise call costs at 1920 x 1080 with and without "denoise_variance" (DESIGN section 5s;
profiles/denoise_variance.txt).

    denoise_variance_cost.py <scene: heightfield | cornell> <switch: off | on | none> [calls]

One traced frame (4 iterations, 8 bounces) of config 5's heightfield scene (streaming) or of assets/scenes/cornell_textured.json (megakernel,
"textures" 1) at 1920 x 1080, ten denoise calls to warm up, then `calls` (default 200) timed ones with events enabled.  Prints one JSON
line: per call the A-Trous passes' denoise_ms (ptc_get_profile: the plain passes under off / none, the guided ones under on), the estimate
stage's stage_ms (ptc_get_denoise_variance_stats: k_variance_estimate and k_variance_prefilter) and the host's wall clock around the calls
and a synchronise; under `on` the stage's counters as well.  `none` never names the parameter: the form that also runs in a checkout from
before it existed (the comparison with the parent commit)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import __graft_entry__ as graft
    pkg = graft.load_package()
    scene_name, switch = sys.argv[1], sys.argv[2]
    calls = int(sys.argv[3]) if len(sys.argv) > 3 else 200
    w, h = 1920, 1080
    mega = scene_name == "cornell"
    if mega:
        sc = pkg.json_parser.scene_from_json(os.path.join(ROOT, "assets", "scenes", "cornell_textured.json"))
    else:
        sc = pkg.scenes.heightfield_scene((w, h))
    flat = sc.build_scene()
    with pkg.PathTracer(max_bounces=8) as pt:
        pt.set_param("frames_in_flight", 1)
        if mega:
            pt.current_gpu_method = pkg.GPUMethod.megakernel
            pt.textures = True
        pt.create_buffers((w, h), flat)
        if mega:
            pt.load_scene_textures(flat)
        if switch != "none":
            pt.set_param("denoise_variance", 1 if switch == "on" else 0)
        pt.set_profiling(time_trace_kernel=True)
        pt.max_iterations = 1 << 30
        for _ in range(4):
            pt.path_trace(sc.camera)
        for _ in range(10):
            pt.denoise()
        pt.synchronize()
        pt.reset_profile()
        s0 = pt.denoise_variance_stats()["stage_ms"] if switch != "none" else 0.0
        t0 = time.perf_counter()
        for _ in range(calls):
            pt.denoise()
        pt.synchronize()
        wall = (time.perf_counter() - t0) * 1e3
        p = pt.profile()
        st = pt.denoise_variance_stats() if switch != "none" else {"stage_ms": 0.0}
        out = {"scene": scene_name, "switch": switch, "calls": calls, "passes_per_call": p["denoise_passes"] / calls,
               "denoise_ms_per_call": p["denoise_ms"] / calls, "stage_ms_per_call": (st["stage_ms"] - s0) / calls,
               "wall_ms_per_call": wall / calls}
        if switch == "on":
            out.update({k: st[k] for k in ("pixels", "floored")})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
