"""The constructed sphere cases (tests/sphere_cases.py), proved on the host through the oracle alone: every family sits where it
claims to -- the oracle's answer flips inside it, and both sides are populated -- the float64 truth with the stored-box gate
(tests/closest_hit_f64.py) agrees with the oracle on every ray it calls robust, and at least 90 % of a "general" family is robust.
Prints the shares (pytest -s)."""
import numpy as np
import pytest

import closest_hit_f64 as f64
import sphere_cases as sc

CASES = [(run, fam) for run in sc.FAMILIES for fam in sc.FAMILIES[run]]


def one(orc, pkg, flat, first, target, rays):
    """the one-object oracle of every ray's own target: hit, t"""
    hit = np.zeros(len(rays), dtype=bool)
    t = np.full(len(rays), -1.0, dtype=np.float32)
    for k in np.unique(target):
        sel = target == k
        recs, h = orc.intersect_rays(sc.subset(pkg, flat, [first + int(k)]), rays[sel])
        hit[sel], t[sel] = h.astype(bool), recs["t"]
    return hit, t


def both_sides(share, least, what):
    assert least <= share <= 1.0 - least, (what, share)


@pytest.mark.parametrize("run,fam", CASES, ids=["%s-%s" % c for c in CASES])
def test_family_sits_where_it_claims(pkg, orc, run, fam):
    flat, first = sc.build(pkg, run)
    rays, info = sc.family(pkg, orc, run, fam, flat, first)
    assert rays.shape == (sc.N, 8) and rays.dtype == np.float32 and np.all(np.isfinite(rays))
    assert np.all((rays[:, 3] == np.float32(1e-4)) | (rays[:, 3] == np.float32(1e-5))) and np.all(rays[:, 7] >= 0)
    assert np.array_equal(rays, sc.family(pkg, orc, run, fam)[0])          # the same rays every time
    recs, hit = orc.intersect_rays(flat, rays)
    hit = hit.astype(bool)
    shares = {"hit": hit.mean()}
    if fam == "graze":
        h, _ = one(orc, pkg, flat, first, info["target"], rays)
        shares["target hit"] = h.mean()
        both_sides(h.mean(), 0.25, "grazing rays on both sides of the silhouette")
        fine = np.abs(info["rel"]) <= 2.0 ** -16
        shares["target hit within 2^-16"] = h[fine].mean()
        both_sides(h[fine].mean(), 0.1, "... and among those within 2^-16 of it")
        if run == "radii":   # (far from the origin the float grid is coarser than 2^-12 r: the sides mix)
            coarse = np.abs(info["rel"]) >= 2.0 ** -12
            assert np.array_equal(h[coarse], info["rel"][coarse] < 0), "a ray 2^-12 r off the silhouette is on its side of it"
    elif fam == "tmin":
        h, t = one(orc, pkg, flat, first, info["target"], rays)
        took = h & (t < 4.0 * rays[:, 3])
        shares["root at t_min accepted"] = took.mean()
        both_sides(took.mean(), 0.2, "the root at t_min accepted and rejected")
        for tmin in (1e-4, 1e-5):
            sel = rays[:, 3] == np.float32(tmin)
            both_sides(took[sel].mean(), 0.2, tmin)
        wide = np.abs(info["tau"] / rays[:, 3].astype(np.float64) - 1.0) >= 0.25     # k = 1, 2: far from the float grid's noise
        small = wide & np.isin(info["target"], (0, 1))                                # (coordinates of a unit or so)
        assert np.array_equal(took[small], info["tau"][small] > rays[small, 3]), "a root a quarter of t_min off is on its side"
    elif fam == "tmax":
        h, t = one(orc, pkg, flat, first, info["target"], rays)
        shares["target within the carried t_max"] = h.mean()
        both_sides(h.mean(), 0.15, "the target's root within and beyond the carried closest hit")
        tie = h & (t == rays[:, 7])
        shares["ties"] = tie.mean()
        assert tie.sum() >= 50, "rays whose carried closest hit is exactly the target's t"
    elif fam == "direction":
        d = rays[:, 4:7]
        lengths = np.linalg.norm(d.astype(np.float64), axis=1)
        for want in (1e-3, 0.5, 2.0, 1e3):
            assert (np.abs(lengths / want - 1.0) < 0.01).sum() >= 500, want
        bits = rays.view(np.uint32)
        for what, cols, pattern in (("+0 direction", slice(4, 7), 0), ("-0 direction", slice(4, 7), 0x80000000),
                                    ("+0 origin", slice(0, 3), 0), ("-0 origin", slice(0, 3), 0x80000000)):
            per_axis = (bits[:, cols] == pattern).sum(axis=0)
            shares[what] = (bits[:, cols] == pattern).any(axis=1).mean()
            assert np.all(per_axis >= 100), (what, per_axis)
        zero_dir = (d == 0).any(axis=1)
        assert hit[zero_dir].mean() > 0.5 and hit.mean() > 0.5
    elif fam == "planes":
        i = np.arange(sc.N)
        back = hit & (recs["side"] == 1) & (recs["material_id"] == info["target"])
        comp = np.ascontiguousarray(recs["normal"]).view(np.uint32)[i, info["axis"]]
        shares.update({"back face of the target": back.mean(), "normal component +0": (back & (comp == 0)).mean(),
                       "normal component -0": (back & (comp == 0x80000000)).mean()})
        assert np.all(np.abs(rays[i, 4 + info["axis"]]) == np.float32(1e-30))
        # outward +0, turned to -0 for the back face; transform_normal's sums of products with zeros then give it the sign the
        # OTHER components leave it: both signs occur (from inside the sphere in front, the x rays meet that one first)
        for axis in (1, 2):
            assert (back & ((comp << 1) == 0) & (info["axis"] == axis)).sum() >= 1000, axis
        assert (back & (comp == 0)).sum() >= 300 and (back & (comp == 0x80000000)).sum() >= 300
    elif fam == "box":
        gate = np.zeros(sc.N, dtype=bool)
        for k in np.unique(info["target"]):
            sel = info["target"] == k
            gate[sel] = sc.box_gate(orc, flat, first + int(k), rays[sel])
        inside, outside, beyond = info["kind"] == 1, info["kind"] == -1, info["kind"] == 2
        shares.update({"edge rays": (inside | outside).mean(), "gate passes inside the edge": gate[inside].mean(),
                       "gate passes outside the edge": gate[outside].mean(), "rays at the part outside the box": beyond.mean()})
        assert gate[inside].mean() >= 0.9 and gate[outside].mean() <= 0.1
        h, _ = one(orc, pkg, flat, first, info["target"], rays)
        assert not np.any(h & ~gate), "no hit without the box"
        if run == "ell_rot":
            assert beyond.sum() >= 300
            cut = beyond & ~gate
            shares["... that miss the box"] = cut.mean()
            assert cut.sum() >= 100, "rays that meet the ellipsoid outside its stored box and miss the box"
    elif fam == "units":
        h, t = one(orc, pkg, flat, first, info["target"], rays)
        reach = info["world_t"] < rays[:, 7]
        big, small = info["target"] == 3, info["target"] == 2
        shares.update({"1e3: world hit within t_max": reach[big].mean(), "1e3: oracle hits": h[big].mean(),
                       "1e-3: world hit within t_max": reach[small].mean(), "1e-3: oracle hits": h[small].mean()})
        assert reach[big].mean() > 0.9 and not h[big & reach].any(), "below t_min in object units: the reference rejects"
        between = small & reach & (rays[:, 7] < 200.0)
        beyond = small & reach & (rays[:, 7] >= 1e3)
        assert between.sum() > 500 and beyond.sum() > 500
        assert not h[between].any() and h[beyond].all(), "t_max in object units"
        assert np.all(np.abs(t[beyond] / info["world_t"][beyond] - 1.0) < 1e-3), "... but t is the world distance"
    elif fam == "degenerate":
        g = info["ghosts"]
        h, _ = one(orc, pkg, flat, first, info["target"], rays)
        for kind in ("negative", "empty_y", "zero"):
            assert not h[info["target"] == g[kind]].any(), kind
        clipped = info["target"] == g["half"]
        shares["clipped box: hit"] = h[clipped].mean()
        both_sides(h[clipped].mean(), 0.2, "the clipped box")
        assert hit.all(), "the wall behind"
    print("\n%-14s %-10s " % (run, fam) + "  ".join("%s %.4f" % kv for kv in shares.items()))
    # the float64 truth with the stored-box gate
    ref = f64.closest_hits(flat, rays)
    bad = f64.compare(ref, hit, recs["t"], recs["normal"])
    print("%-14s %-10s robust %.4f  disagree on robust %d" % (run, fam, ref["robust"].mean(), len(bad)))
    assert len(bad) == 0, (run, fam, bad[:8])
    if fam == "general":
        assert ref["robust"].mean() >= 0.9, (run, ref["robust"].mean())


@pytest.mark.parametrize("run", ["neg_before", "neg_after"])
def test_negative_radius_and_empty_box_are_invisible(pkg, orc, run):
    """the reference tests the stored box first (path_tracer.cu:84): a sphere of negative radius gets min > max on every axis, and
    every ray answers bit for bit as if it, and the object whose box is empty on one axis, were not in the list"""
    flat, first = sc.build(pkg, run)
    g = sc.ghost_objects(pkg, run)
    assert np.all(flat.objects[first + g["negative"]]["aabb_min"] > flat.objects[first + g["negative"]]["aabb_max"])
    count = len(sc.runs(pkg)[run])
    keep = [first + k for k in range(count) if k not in (g["negative"], g["empty_y"])]
    without = sc.subset(pkg, flat, keep)
    for fam in sc.FAMILIES[run]:
        rays, _ = sc.family(pkg, orc, run, fam, flat, first)
        a, ha = orc.intersect_rays(flat, rays)
        b, hb = orc.intersect_rays(without, rays)
        assert np.array_equal(ha, hb) and ha.mean() > 0.5
        for key in ("t", "normal", "material_id", "side"):
            assert np.array_equal(a[key][ha > 0].view(np.uint8), b[key][hb > 0].view(np.uint8)), (fam, key)


def test_walk_restates_the_oracle(pkg, orc):
    """the in-order walk from the one-object answers (the candidate test's yardstick) ends where the oracle's own loop ends"""
    for run in ("pairs", "radii", "neg_before"):
        flat, first = sc.build(pkg, run)
        count = len(sc.runs(pkg)[run])
        rays, _ = sc.interleave([sc.family(pkg, orc, run, fam, flat, first)[0] for fam in sc.FAMILIES[run]])
        accepted, t = sc.walk(orc, pkg, flat, first, count, rays)
        recs, hit = orc.intersect_rays(flat, rays)
        assert np.array_equal(accepted.any(axis=1), hit.astype(bool))
        assert np.array_equal(t[hit > 0], recs["t"][hit > 0])
        last = count - 1 - np.argmax(accepted[:, ::-1], axis=1)
        assert np.array_equal(last[hit > 0].astype(np.uint64), recs["material_id"][hit > 0])


def test_gate_leaves_contained_spheres_alone(pkg, orc):
    """a box that contains its sphere changes nothing: the same answers with the gate as with a box of the whole space"""
    flat, first = sc.build(pkg, "radii")
    rays, _ = sc.family(pkg, orc, "radii", "general", flat, first)
    ref = f64.closest_hits(flat, rays)
    flat.objects["aabb_min"][:] = -1e30
    flat.objects["aabb_max"][:] = 1e30
    wide = f64.closest_hits(flat, rays)
    for key in ("hit", "t", "obj"):
        assert np.array_equal(ref[key], wide[key]), key
    assert (ref["robust"] != wide["robust"]).mean() < 0.01


def test_frame_scenes(pkg):
    for kind in ("neg_trailing", "neg_leading", "clipped", "ellipsoids"):
        scene, flat = sc.frame_scene(pkg, kind)
        assert len(flat.objects) >= 4 and scene.resolution == (64, 48)
    _, flat = sc.frame_scene(pkg, "neg_trailing")
    assert flat.objects[0]["type"] == 1 and np.all(flat.objects[1]["aabb_min"] > flat.objects[1]["aabb_max"]) and flat.objects[2]["type"] == 0
    _, flat = sc.frame_scene(pkg, "neg_leading")
    assert np.all(flat.objects[0]["aabb_min"] > flat.objects[0]["aabb_max"]) and flat.objects[-1]["type"] == 1
    _, flat = sc.frame_scene(pkg, "clipped")
    assert flat.objects[1]["aabb_max"][0] == 0.0 and flat.objects[1]["aabb_min"][0] == -0.5
