"""Direct-light queries on the GPU (ptc_direct_light: k_light_sample, the occlusion launches, k_light_resolve)
against tests/direct_ref.py: shadow rays, visibility and radiance equal the binary32 restatement bit for bit on every point;
independently of any restatement, visible == 1 - the oracle's hit flag of the very rays the library returned; sizes; a
16,384-triangle emitter; the float64 truths; the cross-check variants; scenes without lamps and with a lamp that cannot be
sampled; device pointers; no side effects on a running accumulation."""
import numpy as np
import pytest

import direct_ref as D

pytestmark = pytest.mark.gpu
N_BITS = 20000


def _query(pkg, flat, points, normals, sample_index, params=(), variant=None, size=(32, 32)):
    with pkg.PathTracer() as pt:
        for k, v in params:
            pt.set_param(k, v)
        pt.create_buffers(size, flat)
        if variant is not None:
            pt.set_trace_variant(variant)
        radiance, rays, visible = pt.direct_light(points, normals, sample_index, want_rays=True)
        st = pt.direct_stats()
    n = len(points)
    assert radiance.shape == (n, 3) and rays.shape == (n, 8) and visible.shape == (n,) and set(np.unique(visible)) <= {0, 1}
    return radiance, rays, visible, st


def _same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _check_against_oracle(orc, flat, rays, visible, radiance, sh=None):
    """Needs no restatement: a ray that was generated (t_max > 0) arrives iff the oracle finds nothing on it."""
    _, hit = orc.intersect_rays(flat, rays, scene_handle=sh)
    made = rays[:, 7] > 0
    assert np.array_equal(visible[made], (1 - hit[made]).astype(np.uint8)), np.nonzero(made & (visible != 1 - hit))[0][:10]
    assert not visible[~made].any() and not radiance[visible == 0].any()
    assert np.all(rays[~made, 4:8] == 0) and np.all(rays[:, 3] == np.float32(1e-4))
    return made


@pytest.fixture(scope="module")
def bit_cases(pkg, orc):
    """scene name -> (flat, points, normals, sample index, the restatement's (radiance, rays, visible, sampled)); computed once."""
    out = {}
    for name, scene, lamp_points, si in (("cornell_lit", pkg.scenes.cornell_lit((64, 64), with_mesh=True), D.cornell_lamp_points(), 3),
                                         ("two_instances", D.two_instance_scene(pkg), (), 11)):
        flat = scene.build_scene()
        pts, nrm = D.room_points(N_BITS, seed=17, lamp_points=lamp_points)
        out[name] = (flat, pts, nrm, si, D.query(orc, flat, pts, nrm, si))
    return out


@pytest.mark.parametrize("name", ["cornell_lit", "two_instances"])
def test_bits(pkg, orc, bit_cases, name):
    """3: 20,000 seeded points on the room's surfaces and balls (a fifth with the normal flipped, a few on a lamp's surface)."""
    flat, pts, nrm, si, (want_rad, want_rays, want_vis, want_sampled) = bit_cases[name]
    radiance, rays, visible, st = _query(pkg, flat, pts, nrm, si)
    assert _same_bits(rays, want_rays), np.nonzero(np.any(rays.view(np.uint32) != want_rays.view(np.uint32), axis=1))[0][:10]
    assert np.array_equal(visible, want_vis), np.nonzero(visible != want_vis)[0][:10]
    assert _same_bits(radiance, want_rad), np.nonzero(np.any(radiance.view(np.uint32) != want_rad.view(np.uint32), axis=1))[0][:10]
    made = _check_against_oracle(orc, flat, rays, visible, radiance)
    assert np.array_equal(made, want_sampled)                       # the culled set is the restatement's ...
    culled = int((~made).sum())
    assert N_BITS // 10 < culled < N_BITS // 2, culled              # ... it exists, and is under half of the points
    assert 0.1 < visible.mean() < 0.9 and radiance.max() > 0
    assert st == dict(st, points=N_BITS, sampled=N_BITS - culled, unoccluded=int(visible.sum())) and st["kernel_ms"] == 0.0
    assert st["launches"] == (4 if name == "cornell_lit" else 5)    # sample, spheres, one any-hit launch per mesh object, resolve


def test_sizes(pkg, orc, bit_cases):
    """3: n = 0, 1, 63, 64, 65 and 100,003: bits against the restatement on the first 2,000 (point i draws from index i,
    whatever n is), the oracle's flag on all."""
    flat, pts, nrm, si, (want_rad, want_rays, want_vis, _) = bit_cases["cornell_lit"]
    more_p, more_n = D.room_points(80003, seed=29)
    pts, nrm = np.concatenate([pts, more_p]), np.concatenate([nrm, more_n])
    assert len(pts) == 100003
    sh = orc.SceneHandle(flat)
    with pkg.PathTracer() as pt:
        pt.create_buffers((32, 32), flat)
        empty = pt.direct_light(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), si, want_rays=True)
        assert [a.shape for a in empty] == [(0, 3), (0, 8), (0,)] and pt.direct_stats()["points"] == 0
        assert pkg.lib().ptc_direct_light(pt._ctx, None, None, 0, 0, None, None, None, 0) == pkg._capi.PTC_OK
        for n in (1, 63, 64, 65, 100003):
            radiance, rays, visible = pt.direct_light(pts[:n], nrm[:n], si, want_rays=True)
            k = min(n, 2000)
            assert _same_bits(rays[:k], want_rays[:k]) and np.array_equal(visible[:k], want_vis[:k]), n
            assert _same_bits(radiance[:k], want_rad[:k]), n
            _check_against_oracle(orc, flat, rays, visible, radiance, sh)
            alone = pt.direct_light(pts[:n], nrm[:n], si)              # radiance only: the optional outputs left out
            assert _same_bits(alone, radiance), n
        assert pt.direct_stats()["points"] == 2 * (1 + 63 + 64 + 65 + 100003)


def test_sample_index(pkg, bit_cases):
    """3: another sample index gives other samples; the same index twice gives the same bytes."""
    flat, pts, nrm, si, _ = bit_cases["cornell_lit"]
    with pkg.PathTracer() as pt:
        pt.create_buffers((32, 32), flat)
        a = pt.direct_light(pts, nrm, si, want_rays=True)
        b = pt.direct_light(pts, nrm, si + 1, want_rays=True)
        assert pt.direct_stats()["kernel_ms"] == 0.0
        pt.set_profiling(True, False)
        c = pt.direct_light(pts, nrm, si, want_rays=True)
        assert pt.direct_stats()["kernel_ms"] > 0.0      # only while timing is on
    assert all(_same_bits(x, y) for x, y in zip(a, c))
    made = (a[1][:, 7] > 0) & (b[1][:, 7] > 0)
    assert made.sum() > N_BITS // 3 and np.mean(np.any(a[1][made, 4:8] != b[1][made, 4:8], axis=1)) > 0.999


def test_a_large_emitter(pkg, orc):
    """4: 16,384 emissive triangles (the heightfield mesh at 129 x 65) above a floor: the search runs 14 steps.  5,000 points."""
    flat = D.big_emitter_scene(pkg).build_scene()
    rng = np.random.default_rng(5)
    n = 5000
    pts = np.stack([rng.uniform(-1.9, 1.9, n), rng.uniform(-1.0, 0.9, n), rng.uniform(-1.6, 0.9, n)], axis=1).astype(np.float32)
    nrm = rng.normal(size=(n, 3)) + np.array([0.0, 1.5, 0.0])
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    table = D.light_table(flat)
    assert table[1]["lights"] == 16384 and len(np.unique(table[0]["cdf"])) > 16000
    want_rad, want_rays, want_vis, want_sampled = D.query(orc, flat, pts, nrm, 2, table=table)
    radiance, rays, visible, st = _query(pkg, flat, pts, nrm, 2)
    assert _same_bits(rays, want_rays) and np.array_equal(visible, want_vis) and _same_bits(radiance, want_rad)
    _check_against_oracle(orc, flat, rays, visible, radiance)
    assert len(np.unique(D.sample(orc, flat, pts[:500], nrm[:500], 2, table=table)["lamp"])) > 400   # the lamps picked are spread
    assert 0.3 < want_sampled.mean() and 0.2 < visible.mean()
    with pkg.PathTracer() as pt:
        pt.create_buffers((32, 32), flat)
        assert pt.light_info() == table[1]


@pytest.mark.parametrize("name", ["sphere", "panel", "penumbra", "umbra"])
def test_truths(pkg, orc, name):
    """5: the four cases of tests/test_direct_light_cpu.py through ptc_direct_light, with the same tolerance: the mean of 16,384
    samples within 5 standard errors (of the float64 estimator's samples) of the truth; exact zeros in full umbra."""
    scene, case = D.truth_cases(pkg)[name]
    flat = scene.build_scene()
    n = D.SAMPLES
    pts = np.tile(np.float32(case["p"]), (n, 1))
    nrm = np.tile(np.float32(case["n"]), (n, 1))
    radiance, rays, visible, st = _query(pkg, flat, pts, nrm, D.SAMPLE_INDEX)
    want = D.truth(case)
    est = D.estimate_f64(case, n, seed=1)
    se = est.std(axis=0, ddof=1) / np.sqrt(n)
    mean = radiance.astype(np.float64).mean(axis=0)
    print(name, "truth", want, "GPU mean", mean, "standard error", se)
    assert st["sampled"] == n
    if name == "umbra":
        assert not radiance.any() and not visible.any() and st["unoccluded"] == 0
        return
    assert np.all(np.abs(mean - want) <= 5.0 * se), (mean, want, se)


@pytest.mark.parametrize("label,params,variant", [("variant 0", (), 0), ("variant 1", (), 1), ("force_slow 1", (("debug_force_slow", 1),), None)],
                         ids=["variant_0", "variant_1", "force_slow_1"])
def test_other_paths_give_the_same_bytes(pkg, bit_cases, label, params, variant):
    """6: under trace variants 0 and 1 the generated rays go through the exact closest-hit kernel; debug_force_slow 1 sends every
    ray through the any-hit launch's exact redo."""
    flat, pts, nrm, si, (want_rad, want_rays, want_vis, _) = bit_cases["cornell_lit"]
    radiance, rays, visible, st = _query(pkg, flat, pts, nrm, si, params=params, variant=variant)
    assert _same_bits(rays, want_rays) and np.array_equal(visible, want_vis) and _same_bits(radiance, want_rad), label
    assert st["launches"] == (3 if variant is not None else 4)


def test_scenes_without_lamps(pkg):
    """6: no lamp at all, and a single lamp whose emission is 0: zeros, the empty ray from every point, and no launch."""
    dark = pkg.scenes.cornell_spheres((64, 64))
    dark.add_material("dark", pkg.EmissiveMaterial((0.0, 0.0, 0.0)))
    dark.add_object(pkg.Sphere((0, 0, 0), 0.25), pkg.glmlite.translate((0.9, 1.5, -1.2)), "dark")
    pts, nrm = D.room_points(1000, seed=3)
    for scene, lights in ((pkg.scenes.cornell_spheres((64, 64)), 0), (dark, 1)):
        with pkg.PathTracer() as pt:
            pt.create_buffers((32, 32), scene.build_scene())
            radiance, rays, visible = pt.direct_light(pts, nrm, 1, want_rays=True)
            st = pt.direct_stats()
            assert pt.light_info()["lights"] == lights and pt.light_info()["total_weight"] == 0.0
        assert not radiance.any() and not visible.any()
        assert np.array_equal(rays[:, 0:3], pts) and np.all(rays[:, 3] == np.float32(1e-4)) and not rays[:, 4:8].any()
        assert st == {"points": 1000, "sampled": 0, "unoccluded": 0, "kernel_ms": 0.0, "launches": 0}


def test_a_sphere_lamp_that_cannot_be_sampled(pkg):
    """6: an emissive sphere under scale(0.45, 0.3, 0.4) uploads and renders as ever; the query fails with PTC_ERR_INVALID and
    names the object; the context renders afterwards what a context that was never asked renders."""
    glm = pkg.glmlite
    scene = pkg.scenes.cornell_spheres((48, 32))
    scene.add_material("lamp", pkg.EmissiveMaterial((4.0, 3.0, 2.0)))
    scene.add_object(pkg.Sphere((0, 0, 0), 1.0), glm.compose([glm.scale((0.45, 0.3, 0.4)), glm.translate((0.3, 0.9, -0.5))]), "lamp")
    flat = scene.build_scene()
    pts, nrm = D.room_points(100, seed=3)

    def render(ask):
        with pkg.PathTracer(max_bounces=4) as pt:
            pt.create_buffers((48, 32), flat)
            if ask:
                with pytest.raises(pkg.PtcError) as e:
                    pt.direct_light(pts, nrm, 0)
                assert e.value.code == pkg._capi.PTC_ERR_INVALID and "object 7" in str(e.value)
                assert pt.light_info()["lights"] == 0 and pt.direct_stats()["points"] == 0
            pt.max_iterations = 2
            for _ in range(2):
                pt.path_trace(scene.camera)
            return pt.download("color"), pt.stats()

    a, sa = render(False)
    b, sb = render(True)
    assert np.array_equal(a, b) and sa == sb and a.max() > 1.0   # (the lamp is in the picture)


def test_device_pointers(pkg, bit_cases):
    """7: torch tensors in, torch tensors out: the bytes of the host call."""
    import torch
    flat, pts, nrm, si, (want_rad, want_rays, want_vis, _) = bit_cases["two_instances"]
    n = 12345
    dev = torch.device("cuda:0")
    t_pts, t_nrm = torch.from_numpy(pts[:n]).to(dev), torch.from_numpy(nrm[:n]).to(dev)
    t_rad = torch.full((n, 3), -1.0, dtype=torch.float32, device=dev)
    t_rays = torch.full((n, 8), -1.0, dtype=torch.float32, device=dev)
    t_vis = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with pkg.PathTracer() as pt:
        pt.create_buffers((32, 32), flat)
        pt.direct_light_dev(t_pts.data_ptr(), t_nrm.data_ptr(), n, si, t_rad.data_ptr())
        assert _same_bits(t_rad.cpu().numpy(), want_rad[:n])
        t_rad.fill_(-1.0)
        torch.cuda.synchronize()
        pt.direct_light_dev(t_pts.data_ptr(), t_nrm.data_ptr(), n, si, t_rad.data_ptr(), t_rays.data_ptr(), t_vis.data_ptr())
        st = pt.direct_stats()
    assert _same_bits(t_rad.cpu().numpy(), want_rad[:n]) and _same_bits(t_rays.cpu().numpy(), want_rays[:n])
    assert np.array_equal(t_vis.cpu().numpy(), want_vis[:n])
    assert st["points"] == 2 * n and st["unoccluded"] == 2 * int(want_vis[:n].sum())


def test_no_side_effects_on_a_running_accumulation(pkg, bit_cases):
    """8: three accumulated iterations with a query between them: frames, stats(), the counting fields of profile() and
    occlusion_stats() equal those of the same run without the query; direct_stats() counts the query's points."""
    scene = pkg.scenes.cornell_lit((96, 64), with_mesh=True)
    flat, pts, nrm, si, (_, want_rays, want_vis, want_sampled) = bit_cases["cornell_lit"]

    def run(ask):
        with pkg.PathTracer(max_bounces=6) as pt:
            pt.create_buffers((96, 64), flat)
            pt.max_iterations = 3
            pt.reset_profile()
            for i in range(3):
                pt.path_trace(scene.camera)
                pt.stats()
                if ask and i < 2:
                    assert pt.direct_light(pts[:5000], nrm[:5000], si).shape == (5000, 3)
            out = {k: pt.download(k) for k in ("color", "normal", "depth")}
            prof = {k: v for k, v in pt.profile().items() if not k.endswith("_ms")}
            return out, pt.stats(), prof, pt.occlusion_stats(), pt.direct_stats()

    a, sa, pa, oa, da = run(False)
    b, sb, pb, ob, db = run(True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert sa == sb and pa == pb and oa == ob and oa["rays"] == 0
    assert da["points"] == 0 and da["launches"] == 0
    assert db["points"] == 10000 and db["sampled"] == 2 * int(want_sampled[:5000].sum())
    assert db["unoccluded"] == 2 * int(want_vis[:5000].sum()) and db["launches"] == 8
