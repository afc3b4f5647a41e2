"""The per-path generator at its edges, on the GPU.

1. ptc_selftest_rng (k_selftest_rng: csrc/pt_rng.hpp per element) against rocThrust's recorded answers, the oracle's generator
   and the big-integer restatement, on the inputs of tests/test_rng_edges_cpu.py -- and against the host twin, word for word.
2. Frames on constructed seeds (tests/seed_cases.py): single iterations of a 64 x 48 frame of a closed room whose (pixel,
   iteration) makes path_seed one of the seeds Minstd::seed treats specially, or makes a draw of the jitter or of a material
   exactly 0.0, exactly 1.0f or the largest value below 1 -- where phi = 2 pi u1 reaches the end of det_sincos' range, cos_theta is
   +-1 and the jittered ray lies on the edge of its pixel, of its 8 x 8 beam tile and of the frame.  Colour, normal and depth must be
   the oracle's bit patterns (a NaN equal to the same NaN), ray and live counts the oracle's, under the default schedule, its
   alternatives, and the megakernel.  Every case is proved on the CPU first (frame_cases asserts through the oracle's generator
   that the target is met; tests/test_rng_edges_cpu.py).
3. The same seeds and draws for the direct-light queries, whose sample_index is a free 32-bit argument, against
   tests/direct_ref.py by the comparison of tests/test_gpu_direct_light.py."""
import json
import os

import numpy as np
import pytest

import direct_ref as D
import seed_cases as sc

pytestmark = pytest.mark.gpu
W, H, MB = sc.W, sc.H, sc.MB


def test_device_generator_against_the_three_references(pkg, orc, golden_dir):
    kat = json.load(open(os.path.join(golden_dir, "rng_kat.json")))["cases"]
    seeds, discards, fixed = sc.rng_inputs(kat)
    with pkg.PathTracer(device=0) as pt:
        words = pt.selftest_rng(seeds, discards)
        assert pt.selftest_rng(seeds[:1], discards[:1]).tolist() == [sc.selftest_words(int(seeds[0]), int(discards[0]))]
        assert pt.selftest_rng(seeds[:0], discards[:0]).shape == (0, 6)
    sc.check_rng_words(orc, kat, seeds, discards, fixed, words)
    host = np.zeros_like(words)
    assert pkg.lib().ptc_check_rng(seeds.ctypes.data, discards.ctypes.data, len(seeds), host.ctypes.data) == 0
    assert np.array_equal(words, host)


# ---- frames ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[False, True], ids=["mesh_first", "walls_first"])
def frames(request, pkg, orc):
    """The room (the mesh object first, or two walls in front of it), its cases, and the oracle's frame of every case -- streaming
    for all, megakernel for the seed and jitter cases; computed once."""
    room = sc.Room(pkg, orc, leading_spheres=request.param)
    cases = sc.frame_cases(room)
    assert len(cases) == 69
    streaming = [orc.render_streaming(room.flat, room.camera, W, H, c["iteration"], 1, MB, scene_handle=room.handle) for c in cases]
    for c, ref in zip(cases, streaming):
        if c["name"].startswith("bounce"):   # no path has left the compaction: the slot replayed by frame_cases is the pixel's
            assert ref["live"][0].tolist() == [W * H] * MB, c
    mega = {c["name"]: orc.render_megakernel(room.flat, room.camera, W, H, c["iteration"], 1, MB, scene_handle=room.handle)
            for c in sc.jitter_and_seed_cases(cases)}
    return {"room": room, "cases": cases, "streaming": streaming, "mega": mega, "walls_first": request.param}


def _bits_equal(got, ref, what):
    for k in ("color", "normal", "depth"):
        a, b = np.ascontiguousarray(got[k]).view(np.uint32), np.ascontiguousarray(ref[k]).view(np.uint32)
        assert a.shape == b.shape and np.array_equal(a, b), (what, k, np.argwhere(a != b)[:5].tolist())
    assert got["rays"] == ref["rays"], (what, got["rays"], ref["rays"])


def _trace_case(pkg, pt, room, case):
    """one iteration from zeroed framebuffers (ptc_resize clears them and the counters)"""
    pt.resize_image((W, H))
    pt.set_iteration(case["iteration"])
    pt.max_iterations = case["iteration"] + 1
    pt.path_trace(room.camera)
    got = {k: pt.download(k) for k in ("color", "normal", "depth")}
    st = pt.stats()
    assert pt.iteration() == case["iteration"] + 1
    got["rays"], got["live"] = st["rays_total"], st["last_live"]
    return got


SCHEDULES = [("default", ()), ("frames_in_flight 1", (("frames_in_flight", 1),)), ("fused_shade 0", (("fused_shade", 0),)),
             ("beam 0 filter_rays 0", (("beam", 0), ("filter_rays", 0))),
             # (a batch of one frame takes the persistent launch only when asked to)
             ("persist 1", (("persist", 1), ("persist_min_frames", 1))), ("prefold 0", (("prefold", 0),))]


@pytest.mark.parametrize("what,params", SCHEDULES, ids=[s[0].replace(" ", "_") for s in SCHEDULES])
def test_frames_on_constructed_seeds(pkg, frames, what, params):
    room = frames["room"]
    if frames["walls_first"] and what not in ("default", "prefold 0", "fused_shade 0"):
        params = params + (("sphere_fold", 0),)   # (the walls in front: the same schedules once more, over the plain k_spheres)
    with pkg.PathTracer(device=0, max_bounces=MB) as pt:
        for k, v in params:
            pt.set_param(k, v)
        pt.create_buffers((W, H), room.flat)
        pt.reset_profile()
        for case, ref in zip(frames["cases"], frames["streaming"]):
            got = _trace_case(pkg, pt, room, case)
            _bits_equal(got, ref, (what, case["name"]))
            assert got["live"][:MB] == ref["live"][0].tolist(), (what, case["name"])
        prof = pt.profile()
    # the schedule ran: the persistent launch where it can (one mesh object with nothing in front of it), never elsewhere
    wants_persist = what == "persist 1" and not frames["walls_first"]
    assert (prof["persist_launches"] == len(frames["cases"])) if wants_persist else prof["persist_launches"] == 0


def test_seed_and_jitter_cases_under_the_megakernel(pkg, frames):
    room = frames["room"]
    cases = sc.jitter_and_seed_cases(frames["cases"])
    assert len(cases) == 53
    with pkg.PathTracer(device=0, max_bounces=MB) as pt:
        pt.current_gpu_method = pkg.GPUMethod.megakernel
        pt.create_buffers((W, H), room.flat)
        for case in cases:
            got = _trace_case(pkg, pt, room, case)
            _bits_equal(got, frames["mega"][case["name"]], ("megakernel", case["name"]))


# ---- direct-light queries ----------------------------------------------------------------------------------------------------
def test_direct_light_on_constructed_seeds(pkg, orc):
    """(point index, sample_index) pairs whose seed is one of the four special ones or whose u0 / u1 / u2 is at an edge: shadow
    rays, visibility and radiance of all 256 points of the call equal the restatement's bits, and visibility is the oracle's
    hit flag of the very rays returned -- the comparison of tests/test_gpu_direct_light.py::test_bits."""
    cases = sc.light_cases(orc)
    assert len(cases) == 16
    scenes = [pkg.scenes.cornell_lit((64, 64), with_mesh=True).build_scene(), D.two_instance_scene(pkg).build_scene()]
    pts, nrm = D.room_points(sc.LIGHT_POINTS, seed=17, lamp_points=D.cornell_lamp_points())
    for flat in scenes:
        sh = orc.SceneHandle(flat)
        table = D.light_table(flat)
        with pkg.PathTracer() as pt:
            pt.create_buffers((32, 32), flat)
            for c in cases:
                want_rad, want_rays, want_vis, want_sampled = D.query(orc, flat, pts, nrm, c["sample_index"], table=table, scene_handle=sh)
                radiance, rays, visible = pt.direct_light(pts, nrm, c["sample_index"], want_rays=True)
                assert rays.tobytes() == want_rays.tobytes(), (c, np.nonzero(np.any(rays.view(np.uint32) != want_rays.view(np.uint32), axis=1))[0][:10])
                assert np.array_equal(visible, want_vis), c
                assert radiance.tobytes() == want_rad.tobytes(), c
                _, hit = orc.intersect_rays(flat, rays, scene_handle=sh)
                made = rays[:, 7] > 0
                assert np.array_equal(made, want_sampled) and np.array_equal(visible[made], (1 - hit[made]).astype(np.uint8)), c
                assert not visible[~made].any() and not radiance[visible == 0].any(), c
