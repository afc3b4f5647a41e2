"""Direct-light queries without a GPU: the lamp table of ptc_light_table against its numpy restatement
(tests/direct_ref.py (a)) and against float64, the selection rule, the refusals; and the checker itself -- the binary32
restatement of the sample (b) against float64 truths (c), so that the GPU test's inputs are known to keep the reference inside
the tolerance it is then held to."""
import ctypes as C

import numpy as np
import pytest

import direct_ref as D

SCENES = {
    "cornell_lit": lambda pkg: pkg.scenes.cornell_lit((64, 64), with_mesh=True),
    "two_instances": D.two_instance_scene,
    "dark_lamps": D.dark_lamp_scene,
    "degenerate_triangles": D.degenerate_scene,
    "rotated_scaled_sphere": D.sphere_lamp_scene,
}
WANT = {"cornell_lit": (3, 1, 2, 2), "two_instances": (4, 0, 4, 2), "dark_lamps": (5, 3, 2, 4), "degenerate_triangles": (4, 0, 4, 1),
        "rotated_scaled_sphere": (1, 1, 0, 1)}   # lights, sphere_lights, triangle_lights, emissive_objects


@pytest.mark.parametrize("name", list(SCENES))
def test_table_against_the_restatement_and_float64(pkg, name):
    flat = SCENES[name](pkg).build_scene()
    got, info = pkg.light_table(flat)
    want, want_info, weights, last = D.light_table(flat)
    assert got.dtype.itemsize == 64 and got.tobytes() == want.tobytes(), name
    assert info == want_info
    assert (info["lights"], info["sphere_lights"], info["triangle_lights"], info["emissive_objects"]) == WANT[name]
    # order: emissive objects in object-list order, a mesh's triangles in index order
    assert np.all(np.diff(got["object"].astype(np.int64)) >= 0)
    # cdf: non-decreasing, ends at exactly 1, one rounding from the binary64 value
    cdf = got["cdf"]
    assert np.all(np.diff(cdf) >= 0) and cdf[-1] == np.float32(1.0) and np.all(cdf[last:] == np.float32(1.0))
    exact = np.cumsum(weights) / np.sum(weights)   # (pairwise against sequential summation: far inside the bound at these sizes)
    assert np.max(np.abs(cdf.astype(np.float64) - exact)) <= 2.0 ** -24
    lum = np.array([max(flat.materials["p"][k & 0x7FFFFFFF][:3]) for k in got["kind_material"]], dtype=np.float64)
    live = lum > 0
    assert np.array_equal(got["inv_pdf"][~live], np.zeros(int((~live).sum()), dtype=np.float32))
    assert np.allclose(got["inv_pdf"][live], info["total_weight"] / lum[live], rtol=2.0 ** -23, atol=0)
    # areas from the records against areas from a float64 transform of the vertices: 1e-5 relative
    # (4 * 2^-24 |p| / |e| per edge difference, coordinates <= 2 and edges >= 0.1 in these fixtures)
    k = 0
    for i, obj in enumerate(flat.objects):
        if flat.materials["type"][flat.object_material_indices[i]] != 3:
            continue
        m = np.asarray(obj["m"], dtype=np.float64).reshape(4, 4)   # m[col, row]
        if obj["type"] == 0:
            sp = flat.spheres[obj["index"]].astype(np.float64)
            area = 4.0 * np.pi * (np.linalg.norm(m[0, :3]) * sp[3]) ** 2
            rec_area = 4.0 * np.pi * float(got["e1"][k, 0]) ** 2
            assert abs(rec_area - area) <= 1e-5 * area
            centre = (np.append(sp[:3], 1.0) @ m)[:3]
            assert np.max(np.abs(got["p0"][k] - centre)) <= 1e-6
            k += 1
            continue
        tri = np.asarray(flat.indices).reshape(-1, 3)
        v = np.concatenate([flat.positions.astype(np.float64), np.ones((len(flat.positions), 1))], axis=1) @ m
        v = v[:, :3] / v[:, 3:4]
        assert np.max(np.abs(v)) <= 2.0
        for t in tri:
            area = 0.5 * np.linalg.norm(np.cross(v[t[1]] - v[t[0]], v[t[2]] - v[t[0]]))
            e1, e2 = got["e1"][k].astype(np.float64), got["e2"][k].astype(np.float64)
            rec_area = 0.5 * np.linalg.norm(np.cross(e1, e2))
            if area > 1e-9:
                assert min(np.linalg.norm(v[t[1]] - v[t[0]]), np.linalg.norm(v[t[2]] - v[t[0]])) >= 0.1
                assert abs(rec_area - area) <= 1e-5 * area, (name, k)
            else:
                assert rec_area <= 1e-6   # a triangle of area 0
            k += 1
    assert k == len(got)
    # selection, from the raw first draw in integers: every record of weight > 0 is picked, none of weight 0 -- by the restatement
    # and by the library's own header (ptc_check_light_sample), at both ends of the generator's range and around every threshold
    t = D.thresholds(weights).astype(np.int64)
    v = np.concatenate([[1, D.STATES], t, t + 1, t + 2])
    v = np.unique(v[(v >= 1) & (v <= D.STATES)]).astype(np.uint32)
    picked = D.select(weights, last, v)
    assert np.all(weights[picked] > 0.0), (name, v[weights[picked] <= 0.0])
    assert set(picked) == set(np.nonzero(weights > 0.0)[0])
    lib = pkg.check_light_sample(flat, np.zeros((len(v), 3)), np.tile(np.float32([0, 1, 0]), (len(v), 1)), v, np.full((len(v), 2), 0.5))
    assert np.array_equal(lib["lamp"], picked)
    assert picked[0] == np.nonzero(weights > 0.0)[0][0] and picked[-1] == last


def test_a_scene_without_lamps_has_an_empty_table(pkg):
    got, info = pkg.light_table(pkg.scenes.cornell_spheres((64, 64)))
    assert len(got) == 0 and info["lights"] == 0 and info["total_weight"] == 0.0
    # every lamp dark: the records are there, nothing can be picked
    s = pkg.SceneDescription()
    s.add_material("dark", pkg.EmissiveMaterial((0.0, 0.0, 0.0)))
    s.add_object(pkg.Sphere((0, 0, 0), 0.5), pkg.glmlite.translate((0.0, 1.0, 0.0)), "dark")
    got, info = pkg.light_table(s)
    assert len(got) == 1 and info["lights"] == 1 and info["total_weight"] == 0.0 and info["total_area"] > 3.0
    assert got["cdf"][0] == 0.0 and got["inv_pdf"][0] == 0.0
    assert got.tobytes() == D.light_table(s.build_scene())[0].tobytes()


def test_refusals(pkg):
    glm = pkg.glmlite
    inv = pkg._capi.PTC_ERR_INVALID
    squashed = D.sphere_lamp_scene(pkg, glm.compose([glm.scale((0.45, 0.3, 0.4)), glm.translate((0.0, 1.0, 0.0))]))
    with pytest.raises(pkg.PtcError) as e:
        pkg.light_table(squashed)
    assert e.value.code == inv and "object 1" in str(e.value) and "sphere" in str(e.value)
    sheared = D.sphere_lamp_scene(pkg, glm.compose([glm.scale(0.5), glm.rotate(0.3, (0, 0, 1)), glm.scale((1.0, 1.0001, 1.0))]))
    with pytest.raises(pkg.PtcError) as e:
        pkg.light_table(sheared)
    assert e.value.code == inv and "object 1" in str(e.value)
    flat = D.sphere_lamp_scene(pkg).build_scene()
    assert len(pkg.light_table(flat)[0]) == 1
    flat.objects["m"][1][7] = 0.01   # a projective bottom row
    with pytest.raises(pkg.PtcError) as e:
        pkg.light_table(flat)
    assert e.value.code == inv and "object 1" in str(e.value)
    # the same matrices on a MESH lamp are fine: its records are world-space triangles
    s = D.two_instance_scene(pkg)
    assert len(pkg.light_table(s)[0]) == 4
    # NULL arguments, a capacity that is too small
    flat = pkg.scenes.cornell_lit((64, 64), with_mesh=True).build_scene()
    desc = flat.to_c()
    out = np.zeros(4, dtype=pkg.LIGHT_DTYPE)
    lib = pkg.lib()
    ptr = out.ctypes.data_as(C.POINTER(pkg._capi.ptc_light))
    assert lib.ptc_light_table(None, ptr, 4, None) == inv
    assert lib.ptc_light_table(C.byref(desc), None, 4, None) == inv
    assert lib.ptc_light_table(C.byref(desc), ptr, 2, None) == inv and b"capacity" in lib.ptc_last_error(None)
    assert lib.ptc_light_table(C.byref(desc), ptr, 3, None) == 3
    with pytest.raises(pkg.PtcError):
        pkg.light_table(flat, capacity=1)


@pytest.fixture(scope="module")
def cases(pkg):
    return D.truth_cases(pkg)


@pytest.mark.parametrize("name", ["sphere", "panel", "penumbra", "umbra"])
def test_the_reference_against_the_truths(orc, cases, name):
    """16,384 samples of one floor point (indices 0 .. 16383 of one call, sample index D.SAMPLE_INDEX): the mean of the binary32
    restatement within 5 standard errors of the truth -- closed form Le (R / D)^2 cos(theta) under the lone sphere lamp, a 1024^2
    midpoint quadrature under the panel, the same with the analytic sphere test in the penumbra of a blocker; in full umbra every
    sample is exactly 0.  The standard error is that of the float64 estimator's own samples.  Seeds are fixed."""
    scene, case = cases[name]
    flat = scene.build_scene()
    n = D.SAMPLES
    pts = np.tile(np.float32(case["p"]), (n, 1))
    nrm = np.tile(np.float32(case["n"]), (n, 1))
    radiance, rays, visible, sampled = D.query(orc, flat, pts, nrm, D.SAMPLE_INDEX)
    want = D.truth(case)
    est = D.estimate_f64(case, n, seed=1)
    se = est.std(axis=0, ddof=1) / np.sqrt(n)
    mean = radiance.astype(np.float64).mean(axis=0)
    print(name, "truth", want, "binary32 mean", mean, "float64 mean", est.mean(axis=0), "standard error", se)
    assert sampled.all()
    if name == "umbra":
        assert np.all(want == 0.0) and np.all(est == 0.0)
        assert not radiance.any() and not visible.any()
        return
    assert np.all(want > 0.01) and np.all(se > 0) and np.all(se < 0.02 * want)
    assert np.all(np.abs(est.mean(axis=0) - want) <= 5.0 * se)      # the float64 estimator is unbiased
    assert np.all(np.abs(mean - want) <= 5.0 * se), (mean, want, se)
    if name == "sphere":
        assert 0.4 < visible.mean() < 0.55    # the lamp's far side is hidden by the lamp itself: the shadow ray decides
    if name == "panel":
        assert visible.all()
    if name == "penumbra":
        assert 0.2 < visible.mean() < 0.8
