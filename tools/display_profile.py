#!/usr/bin/env python3
"""The display kernels at 1920 x 1080 beside k_preview on the same buffer, for ONE kernel-trace run:
    rocprofv3 --kernel-trace --stats -d OUT -o display -- python3 tools/display_profile.py
    python3 tools/display_profile.py --summarise OUT/display_results.db          (profiles/display.txt, section 2)
A rendered frame of cornell_lit presented under the reference display (k_preview), under metered ACES (k_meter, k_meter_level,
k_tonemap) and under manual ACES (k_tonemap), then ptc_tonemap_buffer on device buffers: a log-normal frame and the all-one-bin
frame, float4 and packed.  Every phase is WARM warm-up calls and REPS timed ones; the summary tells the phases apart by the order of
the dispatches and gives the median, minimum and maximum of each kernel over a phase's timed calls.  The host clock's figures
(synchronised presents) are printed by the run itself."""
import os
import sqlite3
import sys
import time

WARM, REPS = 10, 50
PHASES = [("rendered frame, reference display", 1), ("rendered frame, ACES metered", 3), ("rendered frame, ACES manual", 1),
          ("lognormal float4, ACES metered", 3), ("lognormal packed, ACES metered", 3), ("one-bin float4, ACES metered", 3),
          ("one-bin packed, ACES metered", 3)]  # in the order main() runs them: (title, display kernels per call)


def summarise(db):
    c = sqlite3.connect(db)
    rows = c.execute("select name, duration from kernels where name like '%k_meter%' or name like '%k_tonemap%' or name like '%k_preview%' "
                     "order by start").fetchall()
    at = 0
    print("# per phase: median / min / max microseconds of each kernel over the last %d of %d calls" % (REPS, WARM + REPS))
    for title, per in PHASES:
        chunk = rows[at: at + per * (WARM + REPS)]
        at += per * (WARM + REPS)
        by = {}
        for name, dur in chunk[per * WARM:]:
            by.setdefault(name.split("(")[0].replace("void ", "").replace("pt::", ""), []).append(dur / 1e3)
        for k, v in by.items():
            v.sort()
            print(f"{title:<36} {k:<18} n {len(v):>3}  median {v[len(v) // 2]:8.2f}  min {v[0]:8.2f}  max {v[-1]:8.2f}")
    print("kernels in the trace:", len(rows), "consumed:", at)


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import numpy as np
    import __graft_entry__ as g
    import display_ref as ref

    pkg = g.load_package()
    import torch
    W, H = 1920, 1080
    N = W * H
    T = pkg.DisplayBufferType
    aces = pkg.Display(curve=2, metering=1)
    scene = pkg.scenes.cornell_lit(resolution=(W, H), with_mesh=True)
    with pkg.PathTracer(device=0, max_bounces=8) as pt:
        pt.create_buffers((W, H), scene.build_scene())
        pt.max_iterations = 4
        for _ in range(4):
            pt.path_trace(scene.camera)
        pbo = torch.zeros((N, 4), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for name, d in (("reference", pkg.Display()), ("aces_metered", aces), ("aces_manual", pkg.Display(curve=2, exposure=1.5))):
            pt.display = d
            for _ in range(WARM):
                pt.send_to_preview(dev_pbo=pbo.data_ptr(), display_type=T.color)
            t0 = time.perf_counter()
            for _ in range(REPS):
                pt.send_to_preview(dev_pbo=pbo.data_ptr(), display_type=T.color)
            dt = (time.perf_counter() - t0) / REPS
            print(f"present of the rendered frame, {name}: {dt * 1e6:.1f} us per present (host clock, synchronised)")
            if d.metering:
                info = pt.exposure_info()
                print("  info:", {k: v for k, v in info.items() if k != "histogram"})
        pt.display = aces
        images = {"lognormal": ref.lognormal_image(N, seed=1), "one_bin": np.full((N, 3), 1.4, dtype=np.float32)}
        for iname, img in images.items():
            for ch in (4, 3):
                src = img if ch == 3 else np.concatenate([img, np.zeros((N, 1), dtype=np.float32)], axis=1)
                t = torch.from_numpy(np.ascontiguousarray(src)).cuda()
                torch.cuda.synchronize()
                for _ in range(WARM):
                    pt.tonemap_buffer_dev(t.data_ptr(), ch, N, pbo.data_ptr())
                t0 = time.perf_counter()
                for _ in range(REPS):
                    info = pt.tonemap_buffer_dev(t.data_ptr(), ch, N, pbo.data_ptr())
                dt = (time.perf_counter() - t0) / REPS
                print(f"tonemap_buffer {iname} {ch} channels: {dt * 1e6:.1f} us per call (host clock, synchronised); level_bin {info['level_bin']}")
    print("done")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--summarise":
        summarise(sys.argv[2])
    else:
        main()
