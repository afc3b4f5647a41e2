"""The entry points of primary rays ("beam": pt_beam_rules.hpp, the functions k_beam runs) over the camera's range, on the host:
tests/camera_cases.py's table through ptc_check_beam (root walk against entry walk) and ptc_check_beam_frustum (the tile
frustums against a float64 statement of the pyramid they stand for), and a condition that the cull still culls.  No GPU.

Found with this table: a frustum whose plane normals were cross products of NEIGHBOURING corner directions of the tile lost hits
below a tile angle of about 5e-4 rad (telephoto views).  test_entry_points_are_sound_for_every_camera and
test_tile_frustums_contain_their_pyramid both fail on that construction."""
import ctypes as C

import numpy as np
import pytest

import camera_cases as cc

U = 2.0 ** -24          # unit roundoff of binary32
ORDINARY_ANGLE = 1e-3   # tile angle from which a camera counts as ordinary (rad)


def test_the_table_covers_what_it_says(pkg):
    cases = cc.cases(pkg)
    count = {}
    for c in cases:
        count[c.group] = count.get(c.group, 0) + 1
    assert count == {"telephoto": 4, "sweep": len(cc.SWEEP_ANGLES) * 2 * 2 * cc.SWEEP_DIRECTIONS, "fullhd": 42, "vfov": 12, "rotation": 7,
                     "rotation_scaled": 5, "position": 3, "position_far": 3, "frame": 9, "matrix": 8}
    assert [c.name for c in cases if not c.render] == ["vfov_nan", "vfov_inf"]
    assert all(c.cpu_only == (c.group == "fullhd") for c in cases)
    # the sweep's tile angles are what its names say, the four telephoto cameras are at or below 1e-4 rad
    for c in cases:
        if c.group == "sweep":
            assert abs(cc.tile_angle(c) / float(c.name.split("_")[1]) - 1.0) < 1e-5, c.name
        if c.group == "telephoto":
            assert cc.tile_angle(c) <= 1.0001e-4, c.name


def test_entry_points_are_sound_for_every_camera(pkg):
    """ptc_check_beam == 0 for every case: stride 1 on the small frames, 3 at full HD.  Not vacuous: every telephoto, sweep and
    full-HD case has hits and entries."""
    failed = []
    for c in cc.cases(pkg):
        bad, st, _ = cc.beam_check(pkg, c, stride=3 if c.cpu_only else 1)
        tiles, empty, entries, rays, hits = st
        assert bad >= 0 and tiles == ((c.w + 7) // 8) * ((c.h + 7) // 8) and entries <= 4 * (tiles - empty) and rays > 0, (c.name, bad, st)
        if bad:
            failed.append((c.name, bad))
        if c.group in ("telephoto", "sweep", "fullhd"):
            assert hits > 0 and entries > 0, (c.name, st)
    assert not failed, (len(failed), sum(b for _, b in failed), failed[:8])


def test_the_case_that_looks_away_keeps_nothing(pkg):
    look = pkg.scenes._camera_from_look_at
    away = cc.Case("away", "away", "hf", None, look((0.0, 2.0, 6.0), (0.0, 3.0, 12.0), vfov_deg=50.0), 64, 40, True, False)
    bad, st, _ = cc.beam_check(pkg, away)
    assert bad == 0 and st[1] == st[0] and st[2] == 0 and st[4] == 0


# ---- the frustum against float64 -----------------------------------------------------------------------------------------------
def _acr(a, b):
    """|a| x |b| with every term added: the bound of a cross product's terms"""
    return np.stack([a[..., 1] * b[..., 2] + b[..., 1] * a[..., 2], a[..., 2] * b[..., 0] + b[..., 2] * a[..., 0],
                     a[..., 0] * b[..., 1] + b[..., 0] * a[..., 1]], axis=-1)


def _xf(m, v, ev):
    """m v in float64, and the bound of what binary32 makes of it: the error carried in, plus three roundings per product (the
    product itself and at most two of the sums it passes through: (c0 x + c1 y) + (c2 z + c3 0))"""
    return v @ m.T, ev @ np.abs(m).T + 3.0 * U * (np.abs(v) @ np.abs(m).T)


def frustum_check(pkg, case):
    """-> (the worst n . d + m + slack over the case's usable tiles, planes and five directions -- >= 0 when every plane has the
    tile's pyramid on its inside --, usable tiles, tiles)"""
    lib = pkg.lib()
    tiles_x, tiles_y = (case.w + 7) // 8, (case.h + 7) // 8
    T = tiles_x * tiles_y
    out = np.zeros(T * 16, dtype=np.float32)
    consts = np.zeros(39, dtype=np.float32)
    cam = cc.camera_c(pkg, case.camera)
    m16 = cc.matrix16(case)
    assert lib.ptc_check_beam_frustum(m16.ctypes.data, C.byref(cam), case.w, case.h, out.ctypes.data, out.size, consts.ctypes.data) == T
    fr = out.reshape(T, 16).astype(np.float64)
    usable = fr[:, 3] == 1.0
    if not usable.any():
        return 0.0, 0, T
    k64 = consts.astype(np.float64)
    cm, im = k64[:16].reshape(4, 4).T[:3, :3], k64[23:39].reshape(4, 4).T[:3, :3]
    vw, vh, llx, lly = k64[19:23]
    w, h = case.w, case.h
    tx, ty = np.arange(T) % tiles_x, np.arange(T) // tiles_x
    e = float(np.float32(0.05))
    with np.errstate(all="ignore"):
        side = {}
        for name, x in (("x0", tx * 8.0 - e), ("x1", (tx + 1) * 8.0 + e)):
            u = x / (w - 1.0)
            d = llx + vw * u
            side[name] = (d, U * (3.0 * np.abs(vw * u) + np.abs(d)))    # roundings: x itself, the division, the product; the sum
        for name, y in (("y0", ty * 8.0 - e), ("y1", (ty + 1) * 8.0 + e)):
            v = (h - y) / (h - 1.0)
            d = lly + vh * v
            side[name] = (d, U * (4.0 * np.abs(vh * v) + np.abs(d)))    # ... and h - y
        zero, one = np.zeros(T), np.ones(T)
        lin = im @ cm
        dirs = [np.stack([dx, dy, -one], axis=-1) @ lin.T
                for dx, dy in ((side["x0"][0], side["y0"][0]), (side["x1"][0], side["y0"][0]), (side["x0"][0], side["y1"][0]),
                               (side["x1"][0], side["y1"][0]), (0.5 * (side["x0"][0] + side["x1"][0]), 0.5 * (side["y0"][0] + side["y1"][0])))]
        worst = np.inf
        for k, name in enumerate(("x0", "x1", "y0", "y1")):
            d, ed = side[name]
            a = np.stack([d, zero, -one], axis=-1) if k < 2 else np.stack([zero, d, -one], axis=-1)
            ea = np.stack([ed, zero, zero], axis=-1) if k < 2 else np.stack([zero, ed, zero], axis=-1)
            b = np.broadcast_to(np.array([0.0, 1.0, 0.0] if k < 2 else [1.0, 0.0, 0.0]), (T, 3))
            a2, ea2 = _xf(im, *_xf(cm, a, ea))
            b2, eb2 = _xf(im, *_xf(cm, b, np.zeros((T, 3))))
            # a cross product's component p - q: the two products and the difference round once each
            en = 2.0 * U * _acr(np.abs(a2), np.abs(b2)) + _acr(ea2, np.abs(b2)) + _acr(np.abs(a2), eb2)
            n = fr[:, 4 + 3 * k:7 + 3 * k]
            # the bound is the construction's, for a normal of the construction's length |A x B|; a plane is its normal's direction,
            # so a normal of another length is granted the same TILT: the bound times |n| / |A x B|
            scale = np.linalg.norm(n, axis=-1) / np.linalg.norm(np.cross(a2, b2), axis=-1)
            for dv in dirs:
                terms = n * dv
                val = terms.sum(axis=-1)
                margin = 1e-4 * np.abs(terms).sum(axis=-1) + 1e-30
                slack = 1.01 * (en * np.abs(dv)).sum(axis=-1) * scale
                # relative to the allowance, so that cases of any scale compare
                rel = (val + margin + slack) / (margin + slack)
                rel = rel[usable & np.isfinite(margin + slack)]
                if len(rel):
                    worst = min(worst, float(np.min(rel)))
    return worst, int(usable.sum()), T


def test_tile_frustums_contain_their_pyramid(pkg):
    """What the cull relies on, stated without a mesh.  The float64 truth of a tile is the pyramid over its pixel rectangle, widened by
    the 0.05 px (as binary32 has it) on each side: directions inv_m cam (dx, dy, -1) with dx = llx + vw x / (w - 1), dy = lly + vh (h - y)
    / (h - 1), the binary32 constants llx, lly, vw, vh, cam and inv_m taken as exact.  For its four corner directions and its centre d,
    every binary32 normal n of the tile (ptc_check_beam_frustum: as the shared rule builds them) must satisfy

        n . d >= -(m + slack),      m = 1e-4 sum |n_i d_i| + 1e-30, the margin outside() itself grants.

    slack is the rounding of the construction, bounded operation by operation to first order (unit roundoff u = 2^-24) and not fitted:
      - a side's coordinate dx: x0 = 8 tx - 0.05 rounds, x0 / (w - 1) rounds, vw * that rounds, llx + that rounds:
        |delta dx| <= u (3 |vw x / (w - 1)| + |dx|); dy has one more rounding, h - y: 4 in place of 3;
      - a spanning vector v = (dx, 0, -1), (0, dy, -1) or an axis through a matrix M (cam, then inv_m): every product rounds and passes
        through at most two sums, so |delta (M v)| <= |M| |delta v| + 3 u |M| |v|, componentwise with absolute values;
      - a component p - q of the cross product A x B: 2 u (|p| + |q|) for its own three roundings, plus |delta A| x |B| + |A| x |delta B|
        with every term taken positive;
      - slack = 1.01 sum_i |delta n_i| |d_i| |n| / |A x B|   (1 % for the second-order terms; turning a normal round is exact; the
        last factor, 1 for this construction, states the bound as a tilt of the plane, whatever the length of the normal).
    A normal built from two neighbouring corner directions of a tile of angle theta has |n| ~ theta and an absolute rounding error of
    about 5e-8, against m <= 1e-4 theta |d|: it fails here below theta ~ 5e-4 (the parent, on every telephoto case)."""
    failed, checked = [], 0
    for c in cc.cases(pkg):
        worst, usable, tiles = frustum_check(pkg, c)
        if c.group in ("telephoto", "sweep", "fullhd", "rotation", "frame", "position"):
            assert usable == tiles, (c.name, usable, tiles)     # (the check is not vacuous where the cull matters)
        checked += usable
        if worst < 0.0:
            failed.append((c.name, worst))
    assert checked > 1_000_000
    assert not failed, (len(failed), failed[:8])


# ---- the cull still culls ---------------------------------------------------------------------------------------------------------
def legacy_cases(pkg):
    """the eight cameras of tests/test_abi_cpu.py::test_entry_points_of_primary_rays_are_sound, restated (checked at stride 3 there)"""
    glm = pkg.glmlite
    look = pkg.scenes._camera_from_look_at
    cam0 = pkg.scenes.heightfield_scene((96, 64), nx=65, nz=33).camera
    rows = [
        ("hf", cam0, 96, 64, None), ("hf", cam0, 101, 67, None),
        ("hf", look((0.0, 0.05, 0.0), (1.0, 0.0, 0.3), vfov_deg=70.0), 80, 48, None),
        ("hf", look((0.0, 3.0, 0.0), (0.0, 0.0, 0.01), vfov_deg=40.0), 64, 64, None),
        ("hf", look((0.0, 2.0, 6.0), (0.0, 3.0, 12.0), vfov_deg=50.0), 64, 40, None),
        ("ball", look((0.0, 0.0, 0.0), (0.3, 0.2, -1.0), vfov_deg=90.0), 72, 56, None),
        ("ball", look((0.5, 0.4, 2.5), (0.0, 0.0, 0.0), vfov_deg=35.0), 64, 64, cc.matrices(pkg)["rotated_scaled"]),
        ("two_triangles", look((0.2, 1.0, 0.9), (0.0, 0.0, 0.0)), 32, 24, None),
    ]
    return [cc.Case(f"legacy_{k}", "legacy", mesh, m, cam, w, h, True, False) for k, (mesh, cam, w, h, m) in enumerate(rows)]


def ordinary_cases(pkg):
    """the table's ordinary cameras: a vertical field inside (0, pi), a tile angle of at least 1e-3 rad, finite rays"""
    return [c for c in cc.cases(pkg) if c.render and 0.0 < float(c.camera.vfov) < np.pi and cc.tile_angle(c) >= ORDINARY_ANGLE
            and c.group not in ("rotation_scaled", "position_far")]


# {case: (tiles, tiles without entries, entries)} of ptc_check_beam at the PARENT commit (the frustum from neighbouring corner
# directions), from a host build of that commit: the check is deterministic and needs no GPU.
PARENT_CULL = {
    "legacy_0": (96, 41, 179),
    "legacy_1": (117, 61, 183),
    "legacy_2": (60, 0, 240),
    "legacy_3": (64, 0, 228),
    "legacy_4": (40, 40, 0),
    "legacy_5": (63, 0, 252),
    "legacy_6": (64, 38, 94),
    "legacy_7": (12, 0, 24),
    "vfov_120deg": (40, 36, 12),
    "vfov_170deg": (40, 38, 6),
    "vfov_179deg": (40, 39, 4),
    "vfov_179.999deg": (40, 39, 4),
    "rot_identity": (40, 32, 26),
    "rot_x_plus": (40, 0, 129),
    "rot_x_minus": (40, 0, 133),
    "rot_y_quarter": (40, 32, 23),
    "rot_y_half": (40, 32, 27),
    "rot_diagonal": (40, 30, 32),
    "rot_generic": (40, 11, 102),
    "pos_inside_box": (40, 0, 146),
    "pos_on_box_face": (40, 5, 123),
    "pos_on_vertex": (40, 0, 144),
    "frame_2x2": (1, 0, 4),
    "frame_2x64": (8, 3, 18),
    "frame_64x2": (8, 6, 6),
    "frame_3x3": (1, 0, 4),
    "frame_8x8": (1, 0, 4),
    "frame_9x9": (4, 2, 6),
    "frame_7x130": (17, 8, 33),
    "frame_257x4": (33, 31, 8),
    "frame_101x67": (117, 60, 192),
    "matrix_mirror": (40, 26, 49),
    "matrix_scale_1e-4": (40, 27, 43),
    "matrix_scale_1e4": (40, 27, 43),
    "matrix_flattened_1e-5": (40, 27, 50),
    "matrix_singular": (40, 0, 160),
    "matrix_translated_1e4": (40, 27, 43),
    "matrix_needle_rotated": (40, 14, 104),
    "matrix_rotated_scaled": (40, 25, 55),
}


@pytest.mark.parametrize("which", ["legacy", "ordinary"])
def test_the_cull_still_culls(pkg, which):
    """A condition on the new frustum, not a measurement of it: over the eight cameras the suite had and over this table's ordinary
    cameras, the tiles without entries in total are no fewer than the parent's minus 1 % of the tiles, and the entries in total no
    more than the parent's plus 1 %.  (Moving a plane by its rounding alone flips only boxes within outside()'s allowance of it.)"""
    cases = legacy_cases(pkg) if which == "legacy" else ordinary_cases(pkg)
    assert len(cases) == (8 if which == "legacy" else 31), [c.name for c in cases]
    tiles = empty = entries = p_empty = p_entries = 0
    for c in cases:
        bad, st, _ = cc.beam_check(pkg, c, stride=3)
        assert bad == 0, (c.name, bad)
        assert st[0] == PARENT_CULL[c.name][0]
        tiles, empty, entries = tiles + st[0], empty + st[1], entries + st[2]
        p_empty, p_entries = p_empty + PARENT_CULL[c.name][1], p_entries + PARENT_CULL[c.name][2]
    print(f"{which}: tiles {tiles}, without entries {empty} (parent {p_empty}), entries {entries} (parent {p_entries})")
    assert empty >= p_empty - 0.01 * tiles
    assert entries <= 1.01 * p_entries
