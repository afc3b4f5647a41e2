"""Sphere objects at their limits (tests/sphere_cases.py; proved on the host by tests/test_sphere_cases_cpu.py) on every road a
sphere can take, against the oracle's bits: hit flag, t, the normal with its signed zeros, material and side -- for occlusion,
the flag.

  * ptc_intersect_rays and ptc_occluded_rays with the run as the whole object list, in front of a small heightfield and behind
    it: the default schedule, "sphere_fold" 0, the trace variants 0 and 1;
  * the per-lane form (sphere_run_lanes, what the kernels that end a bounce run for a trailing run of translated spheres) through
    ptc_debug_sphere_lanes, with one ray per lane (every object held against the smallest cap) and with the fused kernel's rays per
    lane: the oracle's records, and every object the reference's in-order walk accepts at its turn a candidate
    (pt_kernels_common.inc, above sphere_run_lanes); the runs the form must refuse; n around the wavefront and the workgroup;
  * the float64 truth on the rays it calls robust;
  * frames with a sphere of negative radius, a clipped box, an ellipsoid and a scale of 1e3 under four schedules.

Found by the degenerate family and the frames "neg_trailing" and "clipped" (before sphere_ball_of bounded the inner ball by the
stored box): a ray through a translated sphere that the reference never hits -- a negative radius, whose box has min > max, or the
part of a sphere outside a caller's clipped box -- was a sure hit for sphere_candidates, capped the list, and the sphere behind it,
later in the list, was never tested: the ray ended as a miss."""
import numpy as np
import pytest

import closest_hit_f64 as f64
import sphere_cases as sc

pytestmark = pytest.mark.gpu

FUSE_SLOTS = 2     # kFuseK (csrc/pt_kernels_common.inc): the rays a lane of k_shade_fused holds
_cache = {}


def case(pkg, orc, run, placement="whole"):
    """the run's families dealt out in turn, and the oracle's answer to them: computed once, shared, left unchanged"""
    key = (run, placement)
    if key not in _cache:
        flat, first = sc.build(pkg, run, placement)
        if ("rays", run) not in _cache:
            whole, first_w = sc.build(pkg, run)
            _cache[("rays", run)] = sc.interleave([sc.family(pkg, orc, run, fam, whole, first_w)[0] for fam in sc.FAMILIES[run]])
        rays, fam = _cache[("rays", run)]
        recs, hit = orc.intersect_rays(flat, rays)
        for a in (rays, fam, recs, hit):
            a.setflags(write=False)
        _cache[key] = (flat, first, rays, fam, recs, hit.astype(bool))
    return _cache[key]


def differing(run, fam, bad):
    """family name -> rays that differ"""
    return {name: int(bad[fam == j].sum()) for j, name in enumerate(sc.FAMILIES[run]) if bad[fam == j].any()}


def check_records(run, fam, recs, hit, got, what):
    t, nrm, mat, side = got
    bad = (t >= 0) != hit
    both = hit & ~bad
    bad |= both & (t.view(np.uint32) != recs["t"].view(np.uint32))
    bad |= both & np.any(nrm.view(np.uint32) != np.ascontiguousarray(recs["normal"]).view(np.uint32), axis=1)    # signs of zeros included
    bad |= both & (mat != recs["material_id"].astype(np.uint32))
    bad |= both & (side != recs["side"])
    assert not bad.any(), (run, what, differing(run, fam, bad), np.nonzero(bad)[0][:8])


@pytest.mark.parametrize("placement", ["whole", "leading", "trailing"])
@pytest.mark.parametrize("run", sorted(sc.FAMILIES))
def test_rays_on_every_road(pkg, orc, run, placement):
    flat, first, rays, fam, recs, hit = case(pkg, orc, run, placement)
    assert 0.05 < hit.mean() <= 1.0
    with pkg.PathTracer() as pt:
        pt.create_buffers((16, 16), flat)
        roads = (("default", lambda: None), ("sphere_fold 0", lambda: pt.set_param("sphere_fold", 0)),
                 ("variant 0", lambda: pt.set_trace_variant(0)), ("variant 1", lambda: pt.set_trace_variant(1)))
        for what, switch in roads:
            switch()
            got = pt.intersect_rays(rays)
            check_records(run, fam, recs, hit, got, (placement, what))
            occluded = pt.occluded_rays(rays).astype(bool)
            assert np.array_equal(occluded, hit), (run, placement, what, "occlusion", differing(run, fam, occluded != hit))
            if what == "default" and placement == "whole" and "general" in sc.FAMILIES[run]:
                sel = fam == sc.FAMILIES[run].index("general")
                ref = f64.closest_hits(flat, rays[sel])
                assert ref["robust"].mean() >= 0.9
                bad = f64.compare(ref, got[0][sel] >= 0, got[0][sel], got[1][sel])
                assert len(bad) == 0, (run, "float64", bad[:8])


def candidate_bits(cand, count):
    return ((cand[:, None] >> np.arange(count)[None, :]) & 1).astype(bool)


@pytest.mark.parametrize("slots", [1, FUSE_SLOTS])
@pytest.mark.parametrize("run", sc.LANES_RUNS)
def test_per_lane_form(pkg, orc, run, slots):
    flat, first, rays, fam, recs, hit = case(pkg, orc, run)
    count = len(sc.runs(pkg)[run])
    with pkg.PathTracer() as pt:
        pt.create_buffers((16, 16), flat)
        t, nrm, mat, side, cand = pt.debug_sphere_lanes(rays, slots, want_candidates=True)
        plain = pt.debug_sphere_lanes(rays, slots)
    check_records(run, fam, recs, hit, (t, nrm, mat, side), ("lanes", slots))
    check_records(run, fam, recs, hit, plain, ("lanes without the masks", slots))
    assert not np.any(cand >> count), "a candidate beyond the run"
    bits = candidate_bits(cand, count)
    winner = recs["material_id"].astype(np.int64)        # material k belongs to object k
    assert np.all(bits[hit, winner[hit]]), "the winner is a candidate"
    if slots != 1:
        # held against the caps of the objects BEFORE it only: whatever the reference's walk accepts at its turn is a candidate
        # (one ray per lane holds every object against the smallest cap of all, and may drop what a later object overwrites)
        accepted, _ = sc.walk(orc, pkg, flat, first, count, rays)
        missing = accepted & ~bits
        assert not missing.any(), (run, differing(run, fam, missing.any(axis=1)), np.nonzero(missing.any(axis=1))[0][:8])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_per_lane_form_sizes(pkg, orc, n):
    """fewer rays than a wavefront, than a workgroup's tile, one more: the slots beyond n hold no ray"""
    flat, first, rays, fam, recs, hit = case(pkg, orc, "radii")
    with pkg.PathTracer() as pt:
        pt.create_buffers((16, 16), flat)
        for slots in (1, FUSE_SLOTS):
            t, nrm, mat, side, cand = pt.debug_sphere_lanes(rays[:n], slots, want_candidates=True)
            assert len(t) == len(cand) == n
            check_records("radii", fam[:n], recs[:n], hit[:n], (t, nrm, mat, side), (n, slots))


@pytest.mark.parametrize("run", sc.REFUSED_RUNS)
def test_per_lane_form_refuses(pkg, orc, run):
    """nine objects, two classes of matrices, a scaled member, ellipsoids: lanes_run_of refuses, the hook says so"""
    flat, first, rays, fam, recs, hit = case(pkg, orc, run)
    with pkg.PathTracer() as pt:
        pt.create_buffers((16, 16), flat)
        for slots in (1, FUSE_SLOTS):
            with pytest.raises(pkg.PtcError) as e:
                pt.debug_sphere_lanes(rays[:64], slots)
            assert e.value.code == pkg._capi.PTC_ERR_INVALID
        check_records(run, fam, recs, hit, pt.intersect_rays(rays), "still answered object by object")


def test_per_lane_form_arguments(pkg, orc):
    flat, first, rays, fam, recs, hit = case(pkg, orc, "two")
    other = case(pkg, orc, "other_class")
    with pkg.PathTracer() as pt:
        pt.create_buffers((16, 16), other[0])      # the class "two_classes" mixes with the plain one is taken on its own
        check_records("other_class", other[3], other[4], other[5], pt.debug_sphere_lanes(other[2], FUSE_SLOTS), "other class")
    with pkg.PathTracer() as pt:
        with pytest.raises(pkg.PtcError):
            pt.debug_sphere_lanes(rays[:64], 1)     # no scene
        pt.create_buffers((16, 16), flat)
        for slots in (0, 3, 4, -1):
            if slots == FUSE_SLOTS:
                continue
            with pytest.raises(pkg.PtcError) as e:
                pt.debug_sphere_lanes(rays[:64], slots)
            assert e.value.code == pkg._capi.PTC_ERR_INVALID
        for column, value in ((3, 1e-3), (3, 0.0), (7, -1.0), (7, np.nan), (0, np.inf), (5, np.nan)):
            odd = rays[:64].copy()
            odd[5, column] = value
            with pytest.raises(pkg.PtcError) as e:
                pt.debug_sphere_lanes(odd, 1)
            assert e.value.code == pkg._capi.PTC_ERR_INVALID
        pt.set_param("sphere_lanes", 0)
        with pytest.raises(pkg.PtcError) as e:
            pt.debug_sphere_lanes(rays[:64], 1)
        assert e.value.code == pkg._capi.PTC_ERR_INVALID
        pt.set_param("sphere_lanes", 1)
        check_records("two", fam[:64], recs[:64], hit[:64], pt.debug_sphere_lanes(rays[:64], 1), "after the refusals")


SCHEDULES = {"default": (), "sphere_lanes 0": (("sphere_lanes", 0),), "persist 1": (("persist", 1),), "megakernel": None}


@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
@pytest.mark.parametrize("kind", ["neg_trailing", "neg_leading", "clipped", "ellipsoids"])
def test_frames(pkg, orc, kind, schedule):
    key = ("frame", kind)
    if key not in _cache:
        scene, flat = sc.frame_scene(pkg, kind)
        _cache[key] = (scene, flat, orc.render_streaming(flat, scene.camera, 64, 48, 0, 2, 6), orc.render_megakernel(flat, scene.camera, 64, 48, 0, 2, 6))
    scene, flat, streaming, mega = _cache[key]
    ref = mega if schedule == "megakernel" else streaming
    with pkg.PathTracer(device=0, max_bounces=6) as pt:
        if schedule == "megakernel":
            pt.current_gpu_method = pkg.GPUMethod.megakernel
        else:
            for k, v in SCHEDULES[schedule]:
                pt.set_param(k, v)
        pt.create_buffers((64, 48), flat)
        pt.max_iterations = 2
        for _ in range(2):
            pt.path_trace(scene.camera)
        got = {k: pt.download(k) for k in ("color", "normal", "depth")}
        rays = pt.stats()["rays_total"]
    for k in ("color", "normal", "depth"):
        assert np.array_equal(got[k], ref[k]), (kind, schedule, k, int(np.sum(got[k] != ref[k])))
    assert rays == ref["rays"]
