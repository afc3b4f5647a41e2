"""The camera's range on the GPU, over tests/camera_cases.py's table (telephoto views down to a tile angle of 1e-5 rad, wide and
degenerate vertical fields, axis-aligned and scaled rotations, eyes inside, on and far from the mesh, small and ragged frames, hostile
object matrices): the entry points k_beam computes against the host's (the same shared rule: same bits), the primary rays against
their restatement (lit_ref._primary), and frames against the oracle bit for bit -- under the default parameters, without entry
points, unstaged, batched, and in the megakernel; one batch with three unlike cameras; an interleaved rank; and the entry cache of
ptcore_trace.cpp through every way its key can change.  Frames are rendered only with cameras whose restated primary rays are all
finite.  The host-side soundness of the same table: tests/test_camera_cases_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import camera_cases as cc
import lit_ref

pytestmark = pytest.mark.gpu

PLANES = ("color", "normal", "depth")
MB, ITERS = 3, 2
GROUPS = ("telephoto", "sweep", "vfov", "rotation", "rotation_scaled", "position", "position_far", "frame", "matrix")
# the cases frames are rendered with (each under five sets of parameters); test_the_frame_cases_are_the_table_s holds it against the table
FRAME_CASES = ("tele_hf_a", "tele_hf_b", "tele_ball_a", "tele_ball_b",
               "vfov_120deg", "vfov_170deg", "vfov_179deg", "vfov_179.999deg", "vfov_pi_f32", "vfov_3.5", "vfov_2pi", "vfov_zero", "vfov_minus_half",
               "vfov_1e-8",
               "rot_identity", "rot_x_plus", "rot_x_minus", "rot_y_quarter", "rot_y_half", "rot_diagonal", "rot_generic",
               "rot_generic_x2", "rot_generic_x0.001", "rot_generic_x1000", "rot_generic_x-1", "rot_generic_x0",
               "pos_inside_box", "pos_on_box_face", "pos_on_vertex", "pos_far_10000", "pos_far_1e+06", "pos_far_1e+08",
               "frame_2x2", "frame_7x130", "frame_257x4",
               "matrix_mirror", "matrix_scale_1e-4", "matrix_scale_1e4", "matrix_flattened_1e-5", "matrix_singular", "matrix_translated_1e4",
               "matrix_needle_rotated", "matrix_rotated_scaled")
PARAMS = {"default": (), "no_beam": (("beam", 0),), "unstaged": (("frames_in_flight", 1),), "batched": (("batch_frames", 2), ("frames_in_flight", 4))}
_cache = {}


def _flat(pkg, mesh_name, matrix=None):
    """one mesh object under `matrix`, diffuse: bounce 0 opens with a launch over one mesh object, which is where entry points apply"""
    key = (mesh_name, None if matrix is None else np.asarray(matrix, dtype=np.float32).tobytes())
    if key not in _cache:
        scene = pkg.SceneDescription()
        mesh = cc.meshes(pkg)[mesh_name]
        scene.add_mesh(mesh_name, mesh)
        scene.add_material("white", pkg.DiffuseMateral((0.7, 0.7, 0.7)))
        scene.add_object(mesh, pkg.glmlite.identity() if matrix is None else matrix, "white")
        _cache[key] = scene.build_scene()
    return _cache[key]


def _tracer(pkg, flat, w, h, params=(), mega=False):
    pt = pkg.PathTracer(device=0, max_bounces=MB)
    for k, v in params:
        pt.set_param(k, v)
    if mega:
        pt.current_gpu_method = pkg.GPUMethod.megakernel
    pt.create_buffers((w, h), flat)
    return pt


def _same(got, ref, what):
    for p in PLANES:
        a = np.ascontiguousarray(got[p]).view(np.uint32)
        b = np.ascontiguousarray(ref[p], dtype=np.float32).reshape(got[p].shape).view(np.uint32)
        assert np.array_equal(a, b), (what, p, int(np.sum(a != b)), np.argwhere(a != b)[:4].tolist())
    if "rays" in got:
        assert got["rays"] == ref["rays"], (what, got["rays"], ref["rays"])


def _render(pkg, flat, cameras, w, h, params=(), mega=False):
    """iteration i with cameras[i]"""
    with _tracer(pkg, flat, w, h, params, mega) as pt:
        pt.max_iterations = len(cameras)
        for cam in cameras:
            pt.path_trace(cam)
        out = {p: pt.download(p) for p in PLANES}
        out["rays"] = pt.stats()["rays_total"]
    return out


def _rays_bits_equal(rays, o, d):
    """bit for bit, NaN where the restatement has NaN"""
    for got, want in ((rays[:, 0:3], o), (rays[:, 4:7], d)):
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan)
        assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])


# ---- 1. entries --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_device_entries_are_the_host_entries(pkg, group):
    """ptc_debug_beam_entries (k_beam) against ptc_check_beam's entries_out, as uint32, for every case of the group -- the NaN and
    infinite vertical fields included.  One context per (mesh, matrix, frame size)."""
    lib = pkg.lib()
    cases = [c for c in cc.cases(pkg) if c.group == group]
    assert cases and not any(c.cpu_only for c in cases)
    contexts = {}
    entries = 0
    try:
        for c in cases:
            key = (c.mesh, cc.matrix16(c).tobytes(), c.w, c.h)
            if key not in contexts:
                contexts[key] = _tracer(pkg, _flat(pkg, c.mesh, c.matrix), c.w, c.h)
            bad, st, host = cc.beam_check(pkg, c, stride=8, entries=True)
            assert bad == 0, (c.name, bad)
            dev = np.zeros_like(host)
            cam = cc.camera_c(pkg, c.camera)
            assert lib.ptc_debug_beam_entries(contexts[key]._ctx, C.byref(cam), dev.ctypes.data, dev.size) == 0
            diff = host.view(np.uint32) != dev.view(np.uint32)
            assert not diff.any(), (c.name, int(diff.sum()))
            entries += st[2]
    finally:
        for pt in contexts.values():
            pt.close()
    assert entries > 0


# ---- 2. primary rays ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS + ("fullhd",))
def test_primary_rays_against_the_restatement(pkg, orc, group):
    """ptc_generate_rays with the lens off == lit_ref._primary at iterations 0 and 2^31 - 6, for every camera of the group (the full-HD
    cameras on a 64 x 40 frame); the sweep's cameras on every fifth pixel (the restatement is a Python loop), all others on every
    pixel.  And the table's render flag is what it says: True exactly where every restated ray is finite."""
    cases = [c for c in cc.cases(pkg) if c.group == group]
    contexts = {}
    try:
        for c in cases:
            w, h = (64, 40) if c.cpu_only else (c.w, c.h)
            if (w, h) not in contexts:
                contexts[(w, h)] = _tracer(pkg, _flat(pkg, "two_triangles"), w, h)
            pt = contexts[(w, h)]
            pixels = np.arange(w * h)[::5 if group == "sweep" else 1]
            finite = True
            for iteration in (0, 2 ** 31 - 6):
                rays = pt.generate_rays(c.camera, iteration)
                assert rays.shape == (w * h, 8)
                o, d, _, _ = lit_ref._primary(orc, c.camera, w, h, pixels, iteration)
                _rays_bits_equal(rays[pixels], o, d)
                assert np.all(rays[:, 3] == np.float32(1e-4)) and np.all(rays[:, 7] == np.finfo(np.float32).max)
                finite = finite and bool(np.isfinite(rays[:, 0:3]).all() and np.isfinite(rays[:, 4:7]).all())
            assert finite == c.render, (c.name, finite)
            assert pt.iteration() == 0 and pt.stats()["rays_total"] == 0
    finally:
        for pt in contexts.values():
            pt.close()


# ---- 3. frames ---------------------------------------------------------------------------------------------------------------------
def test_the_frame_cases_are_the_table_s(pkg):
    table = {c.name: c for c in cc.cases(pkg)}
    assert all(n in table and table[n].render and not table[n].cpu_only for n in FRAME_CASES)
    covered = {table[n].group for n in FRAME_CASES}
    assert covered == set(GROUPS) - {"sweep"}
    for g in ("telephoto", "rotation", "position_far", "matrix"):   # every case of these groups; of the others every one that may render
        assert {c.name for c in table.values() if c.group == g} <= set(FRAME_CASES)
    for g in ("vfov", "rotation_scaled"):
        assert {c.name for c in table.values() if c.group == g and c.render} <= set(FRAME_CASES)


@pytest.mark.parametrize("name", FRAME_CASES)
def test_frames_are_the_oracle_s(pkg, orc, name):
    """colour, normal, depth and ray count, 2 iterations of 3 bounces, bit for bit: default parameters, ("beam", 0), frames_in_flight 1,
    batch_frames 2 with frames_in_flight 4, and the megakernel"""
    c = cc.by_name(pkg, name)
    assert c.render
    flat = _flat(pkg, c.mesh, c.matrix)
    ref = orc.render_streaming(flat, c.camera, c.w, c.h, 0, ITERS, MB)
    for label, params in PARAMS.items():
        _same(_render(pkg, flat, [c.camera] * ITERS, c.w, c.h, params), ref, (name, label))
    ref = orc.render_megakernel(flat, c.camera, c.w, c.h, 0, ITERS, MB)
    _same(_render(pkg, flat, [c.camera] * ITERS, c.w, c.h, mega=True), ref, (name, "megakernel"))


@pytest.mark.parametrize("params", [(), (("batch_frames", 3), ("frames_in_flight", 3)), (("beam", 0),)], ids=["default", "batch3", "no_beam"])
def test_one_batch_of_a_telephoto_an_ordinary_and_a_179_degree_camera(pkg, orc, params):
    """three distinct entry sets in one launch: iteration i with camera i, the running mean of three unlike views"""
    w, h = 64, 40
    flat = _flat(pkg, "hf")
    cams = [cc.by_name(pkg, n).camera for n in ("tele_hf_a", "rot_generic", "vfov_179deg")]
    prev = None
    for i, cam in enumerate(cams):
        prev = orc.render_streaming(flat, cam, w, h, i, 1, MB, prev=prev)
    got = _render(pkg, flat, cams, w, h, params)
    del got["rays"]
    _same(got, prev, params)


# ---- 4. an interleaved rank --------------------------------------------------------------------------------------------------------
def test_a_telephoto_camera_as_an_interleaved_rank(pkg, orc):
    """rank 1 of 3, blocks of 8 rows, slot_offset = rank * w * h (tests/test_gpu_beam.py: test_interleaved_rows_with_entry_points)"""
    c = cc.by_name(pkg, "tele_ball_b")
    flat = _flat(pkg, c.mesh)
    rank, world, block = 1, 3, 8
    want = orc.render_interleaved(flat, c.camera, c.w, c.h, rank, world, block, rank * c.w * c.h, 0, ITERS, MB)
    with _tracer(pkg, flat, c.w, c.h) as pt:
        pt.set_interleave(rank, world, block)
        pt.set_param("slot_offset", rank * c.w * c.h)
        pt.max_iterations = ITERS
        for _ in range(ITERS):
            pt.path_trace(c.camera)
        _same({p: pt.download(p) for p in PLANES}, want, "rank 1 of 3")


# ---- 5. the entry cache ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", [(), (("frames_in_flight", 1),)], ids=["default", "one_frame_in_flight"])
def test_the_entry_cache_follows_camera_scene_and_size(pkg, orc, params):
    """The entries of a slot are kept while camera, scene serial and mesh object stay (ptcore_trace.cpp).  One context: camera A, camera
    B, A again (the running mean of the three goes on); restart; a second scene with another mesh in the same place of the object list,
    same camera; the first scene again; another frame size with the same camera, and back.  After every step the iteration just traced
    has the oracle's bits.  With one frame in flight every step meets the slot the step before left its entries in."""
    w, h = 64, 40
    flat_a, flat_b = _flat(pkg, "hf"), _flat(pkg, "ball")
    cam_a, cam_b = cc.by_name(pkg, "tele_hf_a").camera, cc.by_name(pkg, "rot_generic").camera
    with _tracer(pkg, flat_a, w, h, params) as pt:
        pt.max_iterations = 16

        def step(what, camera, flat, size, iteration, prev):
            pt.path_trace(camera)
            ref = orc.render_streaming(flat, camera, size[0], size[1], iteration, 1, MB, prev=prev)
            _same({p: pt.download(p) for p in PLANES}, ref, what)
            return ref

        prev = step("camera A", cam_a, flat_a, (w, h), 0, None)
        prev = step("camera B", cam_b, flat_a, (w, h), 1, prev)
        prev = step("camera A again", cam_a, flat_a, (w, h), 2, prev)
        pt.restart()
        step("after restart", cam_a, flat_a, (w, h), 0, None)
        desc_b = flat_b.to_c()
        pt._check(pt._lib.ptc_upload_scene(pt._ctx, C.byref(desc_b)))
        pt.restart()
        step("second scene, same camera", cam_a, flat_b, (w, h), 0, None)
        desc_a = flat_a.to_c()
        pt._check(pt._lib.ptc_upload_scene(pt._ctx, C.byref(desc_a)))
        pt.restart()
        step("first scene again", cam_a, flat_a, (w, h), 0, None)
        pt.resize_image((101, 67))
        pt.restart()
        step("resized", cam_a, flat_a, (101, 67), 0, None)
        pt.resize_image((w, h))
        pt.restart()
        step("resized back", cam_a, flat_a, (w, h), 0, None)
