"""What a long viewing session reaches and a test run of a few hundred iterations never does.

High sample indices: running_mean and k_accumulate compute (float)(iteration + 1), which rounds from 2^24 on (sc - 1.0f may
equal sc); the iteration is uint32_t in DBatchInfo, int in the context and uint64_t in the oracle.  After iterations 0 and 1
(non-zero buffers) the context jumps to N and traces four more; the oracle does the same from the state after 0 and 1.  The
top of the counter: ptc_trace stops at max_iterations = INT_MAX, and ptc_trace_begin refuses iteration == INT_MAX (ptc_trace_end
would overflow the int).

The wrap of the look-back epoch (ptcore_trace.cpp, next_epoch): a tile descriptor is trusted when its 30-bit epoch equals the
launch's; after 2^30 - 1 the epochs start at 1 again behind a clear of the slot's descriptors.  "debug_shade_epoch" puts a
context k launches before the wrap.  Which launch takes epoch 1 follows from the launch plan (one epoch per look-back launch):
  mesh first (the room of tests/seed_cases.py): ray generation's listing launch, then one k_shade_fused per bounce -- 1 + 6 per batch;
  under "persist" ray generation's, then the persistent launch's run of 6;
  walls first: k_list_flags and k_shade_fused per bounce -- 12 per batch ("prefold": ray generation lists nothing); with
  "prefold" 0 ray generation's, then k_spheres and k_shade_fused per bounce -- 13 per batch.
Only the wrap path is run: no stale descriptor is made to meet a reused epoch (a wrong prefix would be an out-of-range slot)."""
import numpy as np
import pytest

import seed_cases as sc

pytestmark = pytest.mark.gpu
INT_MAX = 2**31 - 1
MAX_EPOCH = 0x3FFFFFFF


def _bits_equal(got, ref, what):
    for k in ("color", "normal", "depth"):
        a, b = np.ascontiguousarray(got[k]).view(np.uint32), np.ascontiguousarray(ref[k]).view(np.uint32)
        assert a.shape == b.shape and np.array_equal(a, b), (what, k, np.argwhere(a != b)[:5].tolist())


# ---- high sample indices ---------------------------------------------------------------------------------------------------
W, H, MB = sc.W, sc.H, 4
STARTS = [2**24 - 2, 2**24 + 1, 2**25 + 3, 2**31 - 6]   # (the four iterations from the first straddle 2^24)


@pytest.fixture(scope="module")
def high(pkg, orc):
    """The room seen from inside and -- the same scene -- from above its ceiling, looking up: a frame that is all sky.  Per camera
    and start N the oracle's state after iterations 0, 1, N .. N + 3, streaming and megakernel."""
    room = sc.Room(pkg, orc)
    cams = {"room": room.camera, "sky": pkg.scenes._camera_from_look_at((0.0, 2500.0, 0.0), (0.0, 5000.0, 1.0), vfov_deg=40.0)}
    refs = {}
    for name, cam in cams.items():
        for method, render in (("streaming", orc.render_streaming), ("megakernel", orc.render_megakernel)):
            first = render(room.flat, cam, W, H, 0, 2, MB, scene_handle=room.handle)
            assert first["color"].std() > 0
            for n in STARTS:
                ref = render(room.flat, cam, W, H, n, 4, MB, prev=first, scene_handle=room.handle)
                ref["rays"] += first["rays"]
                refs[(name, method, n)] = ref
    sky = refs[("sky", "streaming", STARTS[0])]
    assert sky["rays"] == 6 * W * H and not sky["live"][:, 1:].any()   # every primary ray of that camera misses
    return {"room": room, "cams": cams, "refs": refs}


PATHS = [("unstaged", "room", (("frames_in_flight", 1),), False),
         ("batches of 2", "room", (("frames_in_flight", 4), ("batch_frames", 2)), False),
         ("a batch of 4", "room", (("frames_in_flight", 4), ("batch_frames", 4)), False),
         ("default", "room", (), False),
         ("all sky, unstaged", "sky", (("frames_in_flight", 1),), False),
         ("all sky, a batch of 4", "sky", (("frames_in_flight", 4), ("batch_frames", 4)), False),
         ("persist 1", "room", (("frames_in_flight", 4), ("batch_frames", 4), ("persist", 1)), False),
         ("megakernel", "room", (), True)]


@pytest.mark.parametrize("what,cam,params,mega", PATHS, ids=[p[0].replace(" ", "_").replace(",", "") for p in PATHS])
def test_high_sample_indices(pkg, high, what, cam, params, mega):
    room, camera = high["room"], high["cams"][cam]
    for n in STARTS:
        with pkg.PathTracer(device=0, max_bounces=MB) as pt:
            for k, v in params:
                pt.set_param(k, v)
            if mega:
                pt.current_gpu_method = pkg.GPUMethod.megakernel
            pt.create_buffers((W, H), room.flat)
            pt.max_iterations = INT_MAX
            pt.reset_profile()
            for _ in range(2):
                pt.path_trace(camera)
            pt.set_iteration(n)
            for _ in range(4):
                pt.path_trace(camera)
            assert pt.iteration() == n + 4
            got = {k: pt.download(k) for k in ("color", "normal", "depth")}
            st, prof = pt.stats(), pt.profile()
        ref = high["refs"][(cam, "megakernel" if mega else "streaming", n)]
        _bits_equal(got, ref, (what, n))
        assert st["rays_total"] == ref["rays"] and st["frames"] == 6, (what, n)
        if what == "persist 1":
            assert prof["persist_launches"] == 2, (what, n)   # iterations 0, 1 and the batch of four


def test_the_top_of_the_iteration_counter(pkg, orc, high):
    room, camera = high["room"], high["cams"]["room"]
    ref = orc.render_streaming(room.flat, camera, W, H, INT_MAX - 1, 1, MB, scene_handle=room.handle)
    for params in ((("frames_in_flight", 1),), ()):
        with pkg.PathTracer(device=0, max_bounces=MB) as pt:
            for k, v in params:
                pt.set_param(k, v)
            pt.create_buffers((W, H), room.flat)
            # ptc_trace: gated by max_iterations -- one iteration runs, the next call is a no-op
            pt.max_iterations = INT_MAX
            pt.set_iteration(INT_MAX - 1)
            pt.path_trace(camera)
            assert pt.iteration() == INT_MAX
            got = {k: pt.download(k) for k in ("color", "normal", "depth")}
            _bits_equal(got, ref, ("INT_MAX - 1", params))
            frames = pt.stats()["frames"]
            pt.path_trace(camera)
            assert pt.iteration() == INT_MAX and pt.stats()["frames"] == frames == 1
            _bits_equal({k: pt.download(k) for k in ("color", "normal", "depth")}, ref, ("no-op", params))
            # the stepwise calls: refused at INT_MAX with a message, and the context goes on working
            with pytest.raises(pkg.PtcError) as e:
                pt.trace_begin(camera)
            assert e.value.code == pkg._capi.PTC_ERR_INVALID and "INT_MAX" in str(e.value)
            assert pt.iteration() == INT_MAX
            with pytest.raises(pkg.PtcError):
                pt.trace_end()   # no frame was begun
            # ... and run at INT_MAX - 1, where ptc_trace_end counts up to INT_MAX
            pt.resize_image((W, H))
            pt.set_iteration(INT_MAX - 1)
            pt.trace_begin(camera)
            for b in range(MB):
                pt.trace_bounce(b)
            pt.trace_end()
            assert pt.iteration() == INT_MAX
            _bits_equal({k: pt.download(k) for k in ("color", "normal", "depth")}, ref, ("stepwise", params))
            pt.restart()
            assert pt.iteration() == 0


# ---- the epoch wrap ------------------------------------------------------------------------------------------------------------
EW, EH, EMB = 100, 67, 6


@pytest.fixture(scope="module")
def rooms(pkg, orc):
    out = {}
    for walls_first in (False, True):
        scene = sc.room_scene(pkg, (EW, EH), leading_spheres=walls_first)
        flat = scene.build_scene()
        out[walls_first] = (scene, flat, orc.render_streaming(flat, scene.camera, EW, EH, 0, 6, EMB))
    return out


ONE = (("frames_in_flight", 1),)                              # every iteration a batch of its own, all on one slot
THREE = (("frames_in_flight", 3), ("batch_frames", 3))        # one slot of three frames: two batches of three iterations
# (walls first?, parameters, k, the launch that takes epoch 1)
WRAPS = [(False, ONE, 0, "ray generation's listing launch, the context's first launch"),
         (False, ONE, 7, "between two batches: ray generation of iteration 1"),
         (False, ONE, 3, "between two bounces: k_shade_fused of bounce 2, iteration 0"),
         (False, ONE, 16, "k_shade_fused of bounce 1, iteration 2"),
         (False, THREE, 7, "between the two batches of three: ray generation of the second"),
         (False, THREE, 4, "k_shade_fused of bounce 3, first batch"),
         (False, THREE + (("persist", 1),), 3, "inside the persistent launch's run: it starts at 1 (ray generation took 2^30 - 3)"),
         (False, THREE + (("persist", 1),), 7, "ray generation of the second batch; its persistent run is 2 .. 7"),
         (False, THREE + (("persist", 1),), 0, "ray generation of the first batch"),
         (True, ONE, 0, "k_list_flags of bounce 0"),
         (True, ONE, 3, "between the list and the shade pass of a bounce: k_shade_fused of bounce 1"),
         (True, ONE, 12, "between two batches: k_list_flags of iteration 1"),
         (True, ONE + (("prefold", 0),), 1, "k_spheres of bounce 0 (ray generation took 2^30 - 1)"),
         (True, ONE + (("prefold", 0),), 2, "k_shade_fused of bounce 0 behind k_spheres"),
         (True, THREE, 17, "k_shade_fused of bounce 2, second batch")]


@pytest.fixture(scope="module")
def never_wrapped(pkg, rooms):
    """per (walls first?, parameters): the frames of a context whose epochs start at 0 as ever"""
    cache = {}

    def get(walls_first, params):
        if (walls_first, params) not in cache:
            cache[(walls_first, params)] = _six_iterations(pkg, rooms[walls_first], params, None)
        return cache[(walls_first, params)]
    return get


def _six_iterations(pkg, room, params, k):
    scene, flat, _ = room
    with pkg.PathTracer(device=0, max_bounces=EMB) as pt:
        for name, v in params:
            pt.set_param(name, v)
        pt.create_buffers((EW, EH), flat)
        if k is not None:
            pt.set_param("debug_shade_epoch", MAX_EPOCH - k)   # valid after ptc_resize
        pt.max_iterations = 6
        pt.reset_profile()
        out = []
        for _ in range(2):      # three iterations across the wrap, three more after it
            for _ in range(3):
                pt.path_trace(scene.camera)
            got = {n: pt.download(n) for n in ("color", "normal", "depth")}
            st = pt.stats()     # raises if a look-back gave up waiting (the dispatch-order flag) or a persistent launch stalled
            got["rays"], got["live"] = st["rays_total"], st["last_live"]
            out.append(got)
        out[-1]["persist_launches"] = pt.profile()["persist_launches"]
    return out


@pytest.mark.parametrize("walls_first,params,k,takes_one", WRAPS,
                         ids=[f"{'walls' if w else 'mesh'}_first-{'-'.join(f'{n}{v}' for n, v in p)}-k{k}" for w, p, k, _ in WRAPS])
def test_the_epoch_wrap(pkg, rooms, never_wrapped, walls_first, params, k, takes_one):
    ref = rooms[walls_first][2]
    base = never_wrapped(walls_first, params)
    got = _six_iterations(pkg, rooms[walls_first], params, k)
    for step in range(2):
        _bits_equal(got[step], base[step], (takes_one, step))
        assert got[step]["rays"] == base[step]["rays"] and got[step]["live"] == base[step]["live"], (takes_one, step)
    _bits_equal(got[1], ref, takes_one)
    assert got[1]["rays"] == ref["rays"] and got[1]["live"][:EMB] == ref["live"][-1].tolist()
    assert got[1]["persist_launches"] == base[1]["persist_launches"] == (2 if ("persist", 1) in params else 0)

