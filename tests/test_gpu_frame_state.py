"""The frame side of a context: everything a ptc_resize decides is one ptc_frame_state, built beside the
context and assigned in ONE place, and released by one function.  Three checks on tiny frames: a resize A, B, A in one context
leaves nothing of the frame before behind -- under three sizing plans, with the per-slot cache of primary-ray entry points live;
a refused resize keeps the frame the context has; the views (download / gather, present / gathered present) read a ptc_buffer
and a ptc_display in one way.  A resize that fails half-way (an allocation) is not provoked here: that it leaves "no frame" is
what the local-state-then-commit structure of ptc_resize says."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZE_A, SIZE_B, ITERS, MB = (64, 48), (40, 30), 3, 4
BUFFERS = ("color", "normal", "depth")


def _scene(pkg):
    """a small heightfield in the box of cornell_spheres, FIRST in the object list: bounce 0 opens with a traversal launch over
    that one mesh object -- the case that takes the entry points of "beam" -- and the box's spheres are the run that ends the list"""
    sc = pkg.SceneDescription()
    mesh_data = pkg.scenes.heightfield_mesh(9, 5, 2.0, 1.0, seed=1)
    mesh = sc.add_mesh("grid", mesh_data)
    sc.add_material("grid", pkg.DiffuseMateral((0.8, 0.3, 0.2)))
    sc.add_object(mesh, pkg.glmlite.translate((0.0, -0.8, 0.6)), "grid")
    pkg.scenes._add_box_and_balls(sc)
    sc.camera = pkg.scenes._camera_from_look_at((0.0, 0.0, 4.0), (0.0, -0.3, 0.0), vfov_deg=45.0)
    return sc, mesh_data


def _cam_c(pkg, camera):
    cam = pkg._capi.ptc_camera()
    cam.position[:] = [float(x) for x in camera.position]
    cam.rotation_wxyz[:] = [float(x) for x in camera.rotation]
    cam.vfov = float(camera.vfov)
    return cam


def _entries(pkg, pt, flat, mesh, camera, size):
    """"beam" took effect, as test_gpu_beam.py checks it: the entries k_beam computes for this context's frame are the host's, and
    there are some"""
    w, h = size
    lib, cam = pkg.lib(), _cam_c(pkg, camera)
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    host, dev = np.zeros(tiles * 32, dtype=np.float32), np.zeros(tiles * 32, dtype=np.float32)
    pos = np.ascontiguousarray(mesh.positions, dtype=np.float32)
    idx = np.ascontiguousarray(mesh.indices, dtype=np.uint32)
    m = np.ascontiguousarray(np.array(flat.objects[0]["m"], dtype=np.float32).reshape(16))
    stats = (C.c_uint64 * 5)()
    assert lib.ptc_check_beam(pos.ctypes.data, len(pos), idx.ctypes.data, len(idx), m.ctypes.data, C.byref(cam), w, h, 4, stats,
                              host.ctypes.data) == 0
    assert lib.ptc_debug_beam_entries(pt._ctx, C.byref(cam), dev.ctypes.data, dev.size) == 0
    assert np.array_equal(host.view(np.uint32), dev.view(np.uint32)), size
    assert stats[2] > 0 and stats[1] < stats[0], (size, list(stats))


def _look(pkg, pt, camera, iters):
    """iters iterations from a restarted frame: the three buffers, the RGBA of every display type, the stats"""
    pt.max_iterations = iters
    assert pt.iteration() == 0
    for _ in range(iters):
        pt.path_trace(camera)
    out = {k: pt.download(k) for k in BUFFERS}
    for d in pkg.DisplayBufferType:
        out["rgba_" + d.name] = pt.send_to_preview(display_type=d)
    return out, pt.stats()


def _same_arrays(got, want, what):
    assert got.keys() == want.keys(), what
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)


def _same_stats(got, want, frames, what):
    """ptc_stats of two visits of a frame: everything but `frames`, which counts the context's frames since it was created"""
    assert got["frames"] == frames, (what, got["frames"], frames)
    assert {k: v for k, v in got.items() if k != "frames"} == {k: v for k, v in want.items() if k != "frames"}, (what, got, want)


# ---- 1. a resize leaves nothing behind ------------------------------------------------------------------------------------

@pytest.mark.parametrize("params,iters", [((), ITERS), ((("frames_in_flight", 1),), ITERS),
                                          ((("frames_in_flight", 5), ("batch_frames", 2)), 7)],
                         ids=["default", "unstaged", "short_last_batch_and_singles"])
def test_resize_in_one_context_leaves_nothing_behind(pkg, params, iters):
    """A, B, A in one context with one camera: the first and the third state agree bit for bit, and B is B of a fresh context --
    colour, normal, depth, the RGBA of all four display types, the stats.  The cache of entry points a slot keeps is keyed by
    cameras, scene and object, not by the resolution: a slot that survived the resize would trace B from A's entries."""
    sc, mesh = _scene(pkg)
    flat = sc.build_scene()
    assert flat.objects[0]["type"] == 1 and len(flat.indices) // 3 == 64

    def fresh():
        pt = pkg.PathTracer(device=0, max_bounces=MB)
        for k, v in params:
            pt.set_param(k, v)
        return pt

    with fresh() as pt:
        pt.create_buffers(SIZE_A, flat)
        first_a, first_a_stats = _look(pkg, pt, sc.camera, iters)
        _entries(pkg, pt, flat, mesh, sc.camera, SIZE_A)
        pt.resize_image(SIZE_B)
        then_b, then_b_stats = _look(pkg, pt, sc.camera, iters)
        _entries(pkg, pt, flat, mesh, sc.camera, SIZE_B)
        pt.resize_image(SIZE_A)
        again_a, again_a_stats = _look(pkg, pt, sc.camera, iters)
    with fresh() as pt:
        pt.create_buffers(SIZE_B, flat)
        fresh_b, fresh_b_stats = _look(pkg, pt, sc.camera, iters)
    assert first_a["color"].shape == (48, 64, 3) and then_b["rgba_depth"].shape == (30, 40, 4)
    assert first_a_stats["rays_total"] > 0 and first_a_stats["frames"] == iters
    _same_arrays(again_a, first_a, "A after B")
    _same_stats(again_a_stats, first_a_stats, 3 * iters, "A after B")
    _same_arrays(then_b, fresh_b, "B after A")
    _same_stats(then_b_stats, fresh_b_stats, 2 * iters, "B after A")


# ---- 2. refused resizes keep the old frame ---------------------------------------------------------------------------------

def test_refused_resizes_keep_the_old_frame(pkg):
    """After each refusal -- code and words as ever -- the context goes on accumulating bit for bit like a control context that
    never saw it."""
    sc, _ = _scene(pkg)
    flat = sc.build_scene()
    refusals = [((1, 5), "resolution must be at least 2x2"), ((65536, 65536), "too many pixels")]
    with pkg.PathTracer(device=0, max_bounces=MB) as ctl, pkg.PathTracer(device=0, max_bounces=MB) as pt:
        for p in (ctl, pt):
            p.create_buffers(SIZE_A, flat)
            p.max_iterations = ITERS * (len(refusals) + 1)

        def step(what):
            for p in (ctl, pt):
                for _ in range(ITERS):
                    p.path_trace(sc.camera)
            _same_arrays({k: pt.download(k) for k in BUFFERS}, {k: ctl.download(k) for k in BUFFERS}, what)
            assert pt.stats() == ctl.stats(), what
            assert pt.iteration() == ctl.iteration(), what

        step("before any refusal")
        for size, words in refusals:
            with pytest.raises(pkg.PtcError) as e:
                pt.resize_image(size)
            assert e.value.code == pkg._capi.PTC_ERR_INVALID and words in str(e.value), (size, str(e.value))
            step(size)
        assert pt.iteration() == ITERS * (len(refusals) + 1)


# ---- 3. the views agree with each other ------------------------------------------------------------------------------------

def test_the_views_agree_with_each_other(pkg):
    """One context that owns the whole frame, no peers: a gathered frame is the download, a gathered present is the present --
    but for PTC_DISPLAY_FINAL, which gathers the accumulated colour (a denoised buffer exists only for a context that owns the
    whole frame: include/ptcore.h).  An unknown buffer or display is refused with the same words by every entry point."""
    capi, lib = pkg._capi, pkg.lib()
    display = pkg.DisplayBufferType
    sc, _ = _scene(pkg)
    flat = sc.build_scene()
    w, h = SIZE_A
    with pkg.PathTracer(device=0, max_bounces=MB) as pt:
        pt.create_buffers(SIZE_A, flat)
        pt.max_iterations = ITERS
        for _ in range(ITERS):
            pt.path_trace(sc.camera)
        for stage in ("traced", "denoised"):
            if stage == "denoised":
                pt.denoise()
                assert not np.array_equal(pt.download("final"), pt.download("color"))
            for which in BUFFERS + ("final",):
                got, want = pt.gather_frame(which), pt.download(which)
                assert got.shape == want.shape == ((h, w) if which == "depth" else (h, w, 3)), (stage, which)
                assert np.array_equal(got, want), (stage, which)
            for d in (display.color, display.normal, display.depth):
                assert np.array_equal(pt.gather_present(d), pt.send_to_preview(display_type=d)), (stage, d)
            assert np.array_equal(pt.gather_present(display.final), pt.send_to_preview(display_type=display.color)), stage
        assert not np.array_equal(pt.send_to_preview(display_type=display.final), pt.send_to_preview(display_type=display.color))

        pt.band_export()
        floats = np.zeros(w * h * 3, dtype=np.float32)
        rgba = np.zeros(w * h, dtype=np.uint32)
        calls = [("ptc_download", lambda: lib.ptc_download(pt._ctx, 7, floats.ctypes.data, 0), "unknown buffer"),
                 ("ptc_band_publish", lambda: lib.ptc_band_publish(pt._ctx, 7), "unknown buffer"),
                 ("ptc_gather_frame", lambda: lib.ptc_gather_frame(pt._ctx, 7, floats.ctypes.data, 0), "unknown buffer"),
                 ("ptc_present_rgba8", lambda: lib.ptc_present_rgba8(pt._ctx, rgba.ctypes.data, 0, 7), "unknown display type"),
                 ("ptc_gather_present_rgba8", lambda: lib.ptc_gather_present_rgba8(pt._ctx, rgba.ctypes.data, 0, 7), "unknown display type")]
        for name, call, words in calls:
            with pytest.raises(pkg.PtcError) as e:
                capi.check(call(), pt._ctx)
            assert e.value.code == capi.PTC_ERR_INVALID and words in str(e.value), (name, str(e.value))
        pt.band_publish("color")   # the exported buffer is there ...
        pt.resize_image(SIZE_B)    # ... and dies with the frame
        with pytest.raises(pkg.PtcError) as e:
            pt.band_publish("color")
        assert e.value.code == capi.PTC_ERR_INVALID and "ptc_band_export first" in str(e.value)
