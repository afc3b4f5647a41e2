"""The thin lens (ptc_set_lens) without a GPU: the numpy restatement tests/lens_ref.py -- the checker of
tests/test_gpu_lens.py -- against the oracle's pinhole, against the truth in float64 and against the uniform distribution on the disk;
that the lens stream leaves the path stream alone; the edge draws; the binding, hip_pt's refusals and the two scene readers."""
import math
import os
import subprocess

import numpy as np
import pytest

import lens_ref
import lit_ref
import seed_cases as sc
from ref_f32 import F, stream_draws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_PT = os.path.join(ROOT, "cuda-path-tracer_amd", "host", "hip_pt")
EPS = 2.0 ** -24  # the relative error of one correctly rounded binary32 operation


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _cameras(pkg):
    """(name, camera): at the origin looking down -z (the matrix is the identity); at the origin, rotated; 1e4 from the origin, rotated"""
    look = pkg.scenes._camera_from_look_at
    far = (6000.0, -8000.0, 0.0)
    return [("origin", pkg.Camera(vfov=float(np.float32(math.radians(45.0))))),
            ("origin_rotated", look((0.0, 0.0, 0.0), (1.0, -0.5, -2.0), vfov_deg=60.0)),
            ("far_rotated", look(far, (far[0] - 3.0, far[1] + 1.0, far[2] - 2.0), vfov_deg=45.0))]


@pytest.mark.parametrize("iteration", [0, 1, 2 ** 31 - 6])
def test_radius_0_is_lit_ref_s_primary(pkg, orc, iteration):
    """lens None and radius 0 hand back lit_ref._primary's arrays bit for bit; and the parts the lens rule is built from -- dx, dy, the
    matrix product, the normalisation -- put together as the pinhole give the oracle's ray bit for bit, so they are the oracle's."""
    w, h = 64, 48
    camera = pkg.scenes.cornell_spheres((w, h)).camera
    pixels = np.arange(w * h)
    ref = lit_ref._primary(orc, camera, w, h, pixels, iteration)
    for lens in (None, (0.0, 1.0), (0.0, 0.0)):
        got = lens_ref.primary(orc, camera, w, h, pixels, iteration, lens)
        for a, b in zip(got, ref):
            assert np.array_equal(_bits(a) if a.dtype == np.float32 else a, _bits(b) if b.dtype == np.float32 else b), lens
    for _, cam in [("cornell", camera)] + _cameras(pkg):
        ref = lit_ref._primary(orc, cam, w, h, pixels, iteration)
        parts = lens_ref.pinhole_from_parts(orc, cam, w, h, pixels, iteration)
        assert np.array_equal(parts[0], ref[0]) and np.array_equal(_bits(parts[1]), _bits(ref[1]))
        assert np.array_equal(parts[2], ref[2]) and np.array_equal(parts[3], ref[3])


def _truth(orc, camera, w, h, pixels, iteration, focus):
    """float64, from the binary32 inputs taken as exact (the matrix, the viewport constants, the jittered pixel position):
    -> (focus point of every pixel in world space [n, 3], pinhole origin [3], unit normal of the lens plane [3])"""
    m = lens_ref.camera_matrix(orc, camera, w, h).astype(np.float64).reshape(4, 4).T  # column-major -> m[row, col]
    llx, lly, vw, vh = (float(v) for v in lens_ref.viewport(camera, w, h))
    u = stream_draws(orc, pixels, iteration, 0, 0, 2)
    fx = (np.float32(pixels % w) + u[:, 0]).astype(np.float64)  # (the jitter sum is a binary32 operation of the rule: an input here)
    fy = (np.float32(pixels // w) + u[:, 1]).astype(np.float64)
    dx = llx + vw * (fx / (w - 1))
    dy = lly + vh * ((h - fy) / (h - 1))
    f = float(np.float32(focus))
    p = np.stack([dx * f, dy * f, np.full_like(dx, -f), np.ones_like(dx)], axis=-1) @ m.T
    n = np.cross(m[:3, 0], m[:3, 1])
    return p[:, :3], m[:3, 3], n / np.linalg.norm(n)


def _bound(w, h, vw, vh, pos, r, f):
    """How far a binary32 lens ray may pass from the float64 focus point of its pixel, and its origin lie from the lens plane.

    Every operation of section 5i's list is correctly rounded: relative error EPS = 2^-24.  With hx = vw (1/2 + 1/(w - 1)) >= |dx|
    and hy likewise (fx <= w), V = max(vw, vh), |entries of the rotation| <= 1 (+ 2^-20, folded into the last factor):
      origin    o = (m0 lx + m4 ly) + (m8 0 + m12): two products, their sum, the sum with the translation -- per row at most
                EPS (3 (|lx| + |ly|) + |pos_row|); over three rows, |lx| + |ly| <= sqrt(2) r:  e_o = EPS (8 r + 2 |pos|)
                (3 sqrt(2) sqrt(3) = 7.4 <= 8, sqrt(3) max|pos_row| <= 2 |pos|); the division by w = 1 is exact.
      target    x = (dx f) - lx: dx carries 3 roundings of magnitude vw (the quotient, the product, the sum), the product with f one
                more, the difference one of f |dx| + r -- EPS (5 f V + r) per axis, two axes:   e_c = EPS sqrt(2) (5 f V + r)
      matrix    per row three products, two sums: 3 EPS (|x| + |y| + |z|), three rows:           e_m = EPS 3 sqrt(3) T,
                T = f (hx + hy + 1) + 2 r
      normalise the factor 1 / sqrt(dot) is common to the components (it moves no line); the three products with it round once
                each: an angle of EPS over the length L = f sqrt(1 + hx^2 + hy^2) + r:              e_n = EPS L
    The point o + (the computed vector) lies within e_o + e_c + e_m of the focus point, the rounded direction turns it by e_n more.
    (1 + 2^-10) covers the second-order terms and the rotation's own rounding.  -> (the ray's bound, the origin's bound e_o)"""
    hx, hy = vw * (0.5 + 1.0 / (w - 1)), vh * (0.5 + 1.0 / (h - 1))
    e_o = 8.0 * r + 2.0 * float(np.linalg.norm(pos))
    e_c = math.sqrt(2.0) * (5.0 * f * max(vw, vh) + r)
    e_m = 3.0 * math.sqrt(3.0) * (f * (hx + hy + 1.0) + 2.0 * r)
    e_n = f * math.sqrt(1.0 + hx * hx + hy * hy) + r
    slack = 1.0 + 2.0 ** -10
    return EPS * (e_o + e_c + e_m + e_n) * slack, EPS * e_o * slack


def _line_distance(o, d, p):
    o, d = o.astype(np.float64), d.astype(np.float64)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    v = p - o
    return np.linalg.norm(v - np.sum(v * d, axis=1, keepdims=True) * d, axis=1)


def test_every_ray_passes_its_focus_point_in_float64(pkg, orc):
    """4096 rays (64 x 64 pixels, iteration 3) per radius, focus distance and camera.  Every ray's line passes the float64 focus point
    of its pixel within _bound (derived there: counts of operations x 2^-24 x the magnitudes f, |position|, r; not fitted); every
    origin lies in the lens plane within the origin's part of it, and within r (1 + 2^-22) of the pinhole origin -- taken plus that
    same part, which is 0 for the camera at the origin and is what binary32 can hold at all for the camera 1e4 away (its ulp there,
    2^-10, is the smallest radius); the camera-space lens point itself is held to r (1 + 2^-22) with nothing added.  Directions have
    unit length within 2^-22 (the dot product, the root, the reciprocal, the product)."""
    w = h = 64
    pixels = np.arange(w * h)
    iteration = 3
    worst = 0.0
    for name, camera in _cameras(pkg):
        llx, lly, vw, vh = (float(v) for v in lens_ref.viewport(camera, w, h))
        for r in (1e-3, 0.05, 0.5, 5.0):
            lx, ly, _ = lens_ref.lens_points(orc, pixels, iteration, r)
            r32 = float(np.float32(r))
            assert np.all(np.hypot(lx.astype(np.float64), ly.astype(np.float64)) <= r32 * (1.0 + 2.0 ** -22)), (name, r)
            for f in (0.1, 1.0, 10.0, 1000.0):
                o, d, tmin, _ = lens_ref.primary(orc, camera, w, h, pixels, iteration, (r, f))
                assert np.all(np.isfinite(o)) and np.all(np.isfinite(d)) and np.all(tmin == F(1e-4))
                assert np.all(np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1.0) <= 2.0 ** -22), (name, r, f)
                p, origin, normal = _truth(orc, camera, w, h, pixels, iteration, f)
                ray_bound, origin_bound = _bound(w, h, vw, vh, camera.position, r32, float(np.float32(f)))
                dist = _line_distance(o, d, p)
                assert np.all(dist <= ray_bound), (name, r, f, float(dist.max()), ray_bound)
                worst = max(worst, float((dist / ray_bound).max()))
                off = o.astype(np.float64) - origin
                assert np.all(np.abs(off @ normal) <= origin_bound), (name, r, f, float(np.abs(off @ normal).max()), origin_bound)
                assert np.all(np.linalg.norm(off, axis=1) <= r32 * (1.0 + 2.0 ** -22) + origin_bound), (name, r, f)
    print(f"largest distance / bound over all cases: {worst:.3f}")
    assert worst > 0.0


def test_lens_points_are_uniform_on_the_disk(orc):
    """The 4096 lens points of the pixels of a 64 x 64 frame at iteration 0: (rho / r)^2 in 8 equal bins and the angle in 8 equal bins,
    each chi-square below 24.32 (the 99.9 % quantile for 7 degrees of freedom).  Fixed inputs: the outcome was decided when this was
    written (5.113 and 5.723 -- asserted below to within the printing, so that a change of the stream shows)."""
    r = 0.5
    lx, ly, _ = lens_ref.lens_points(orc, np.arange(4096), 0, r)
    lx, ly = lx.astype(np.float64), ly.astype(np.float64)
    area = (lx * lx + ly * ly) / (r * r)
    angle = np.mod(np.arctan2(ly, lx), 2.0 * np.pi) / (2.0 * np.pi)
    chi = []
    for x in (area, angle):
        counts = np.bincount(np.minimum((x * 8.0).astype(np.int64), 7), minlength=8)
        assert counts.sum() == 4096
        chi.append(float(np.sum((counts - 512.0) ** 2 / 512.0)))
    print("chi-square (rho^2, angle):", chi)
    assert chi[0] < 24.32 and chi[1] < 24.32, chi
    assert abs(chi[0] - CHI_SEEN[0]) < 0.01 and abs(chi[1] - CHI_SEEN[1]) < 0.01, chi


CHI_SEEN = (5.113, 5.723)


def test_the_lens_stream_leaves_the_path_stream_alone(pkg, orc):
    """The generator state primary returns -- the megakernel's material draws go on from it -- is the pinhole's for every pixel, and
    the lens stream's seeds differ from the path, light and roulette streams' by their constants."""
    w, h = 64, 48
    camera = pkg.scenes.cornell_spheres((w, h)).camera
    pixels = np.arange(w * h)
    for iteration in (0, 7):
        pin = lit_ref._primary(orc, camera, w, h, pixels, iteration)
        got = lens_ref.primary(orc, camera, w, h, pixels, iteration, (0.3, 4.0))
        assert np.array_equal(got[3], pin[3])
        assert not np.array_equal(got[0], pin[0]) and not np.array_equal(got[1], pin[1])
    assert lens_ref.LENS_XOR == 0x4C454E53 == int.from_bytes(b"LENS", "big")
    assert len({0, lens_ref.LENS_XOR, lit_ref.ROULETTE_XOR, sc.XOR_LIGHT}) == 4


EDGES = (("u1 = 0.0", 1, sc.STATE_ZERO, 0.0), ("u1 = 1.0f", 1, sc.STATE_ONE_LO, 1.0), ("u2 = 0.0", 2, sc.STATE_ZERO, 0.0),
         ("u2 = 1.0f", 2, sc.STATE_ONE_HI, 1.0))


@pytest.mark.parametrize("name,draw,state,value", EDGES)
def test_edge_draws(pkg, orc, name, draw, state, value):
    """seed_cases' inversion puts the draw on a pixel of the 64 x 48 frame: (pixel, iteration) whose lens stream yields exactly 0.0 or
    1.0f as its first or second draw.  The ray is finite and of unit length; u1 = 0 is the lens centre, whose origin is the
    pinhole's and whose direction lies within the bound of test_every_ray_passes_its_focus_point_in_float64 of the pinhole's (both
    pass the focus point within it, a distance f or more away: 2 bound / f); u1 = 1.0f lies on the rim, rho = r exactly."""
    w, h, r, f = 64, 48, 0.25, 3.0
    camera = pkg.scenes.cornell_spheres((w, h)).camera
    pixel, iteration, _ = sc.place(sc.seeds_for_draw(state, draw), range(w * h), xor=lens_ref.LENS_XOR)
    px = np.array([pixel])
    lx, ly, u = lens_ref.lens_points(orc, px, iteration, r)
    assert float(u[0, draw - 1]) == value, (name, u)
    o, d, _, _ = lens_ref.primary(orc, camera, w, h, px, iteration, (r, f))
    assert np.all(np.isfinite(o)) and np.all(np.isfinite(d))
    assert abs(np.linalg.norm(d[0].astype(np.float64)) - 1.0) <= 2.0 ** -22
    llx, lly, vw, vh = (float(v) for v in lens_ref.viewport(camera, w, h))
    bound, _ = _bound(w, h, vw, vh, camera.position, r, f)
    p, _, _ = _truth(orc, camera, w, h, px, iteration, f)
    assert _line_distance(o, d, p)[0] <= bound
    rho = math.hypot(float(lx[0]), float(ly[0]))
    if name == "u1 = 0.0":
        po, pd, _, _ = lit_ref._primary(orc, camera, w, h, px, iteration)
        assert lx[0] == 0.0 and ly[0] == 0.0 and np.array_equal(o, po)
        assert _line_distance(po, pd, p)[0] <= bound
        assert np.linalg.norm(d[0].astype(np.float64) - pd[0].astype(np.float64)) <= 2.0 * bound / f
    elif name == "u1 = 1.0f":
        assert abs(rho - r) <= r * 2.0 ** -22
    elif name == "u2 = 0.0":
        assert ly[0] == 0.0 and lx[0] > 0.0   # the angle 0: cos 1, sin 0
    else:
        assert abs(float(ly[0])) <= rho * 2.0 ** -20 and lx[0] > 0.0   # the angle 2 pi, through det_sincos' reduction


def test_the_binding_and_the_python_mirror(pkg):
    lib = pkg.lib()
    for name in ("ptc_set_lens", "ptc_get_lens", "ptc_generate_rays"):
        assert hasattr(lib, name) and name in pkg._capi.SIGNATURES
    assert lib.ptc_abi_version() == 3
    assert pkg.Camera().lens_radius == 0.0 and pkg.Camera().focus_distance == 0.0


def _hip_pt(*args):
    if not os.path.exists(HIP_PT):
        subprocess.run(["make"], cwd=os.path.dirname(HIP_PT), check=True, stdout=subprocess.DEVNULL)
    return subprocess.run([HIP_PT, *args], cwd=ROOT, capture_output=True, text=True)


@pytest.mark.parametrize("args,says", [(("--lens-radius", "-0.5", "--focus-distance", "2"), "'-0.5' is not a finite number >= 0"),
                                       (("--lens-radius", "nan", "--focus-distance", "2"), "'nan' is not a finite number >= 0"),
                                       (("--lens-radius", "0.1", "--focus-distance", "nan"), "'nan' is not a finite number > 0"),
                                       (("--lens-radius", "0.1", "--focus-distance", "0"), "'0' is not a finite number > 0"),
                                       (("--lens-radius", "0.1"), "needs a focus distance")])
def test_hip_pt_refuses_a_bad_lens_before_it_touches_a_gpu(tmp_path, args, says):
    """Exit 1 with the offending value named, at argument parsing (the radius without a focus distance: once the scene file, which
    might have given one, is read) -- with -o, so that only the refusal stands between the command and a render."""
    r = _hip_pt("assets/scenes/cornell_spheres.json", "-o", str(tmp_path / "x.png"), *args)
    assert r.returncode == 1 and says in r.stderr, (r.returncode, r.stderr)
    assert not (tmp_path / "x.png").exists()


def test_both_scene_readers_give_the_same_lens(pkg, tmp_path):
    """cornell_dof.json: both readers give its lens; a file without the keys gives none, and hip_pt's scene dump is the one it was."""
    dof = pkg.json_parser.scene_from_json(os.path.join(ROOT, "assets", "scenes", "cornell_dof.json"))
    plain = pkg.json_parser.scene_from_json(os.path.join(ROOT, "assets", "scenes", "cornell_spheres.json"))
    assert (dof.camera.lens_radius, dof.camera.focus_distance) == (float(np.float32(0.2)), float(np.float32(4.2)))
    assert (plain.camera.lens_radius, plain.camera.focus_distance) == (0.0, 0.0)
    assert dof.camera.position == plain.camera.position and dof.camera.rotation == plain.camera.rotation
    dumps = {}
    for name in ("cornell_dof", "cornell_spheres"):
        path = tmp_path / (name + ".bin")
        r = _hip_pt("--dump-scene", str(path), f"assets/scenes/{name}.json")
        assert r.returncode == 0, r.stderr
        dumps[name] = path.read_bytes()
    # (the dump: the arrays, the camera, resolution and spp; two floats more when the camera has a lens)
    assert len(dumps["cornell_dof"]) == len(dumps["cornell_spheres"]) + 8
    lens = np.frombuffer(dumps["cornell_dof"][-8:], dtype="<f4")
    assert (float(lens[0]), float(lens[1])) == (dof.camera.lens_radius, dof.camera.focus_distance)
    assert dumps["cornell_dof"][:-20] == dumps["cornell_spheres"][:-12]   # (all but spp, which the two files set differently)
    for bad in ('"lens_radius": -1', '"lens_radius": "wide"', '"focus_distance": 0', '"focus_distance": -2'):
        text = open(os.path.join(ROOT, "assets", "scenes", "cornell_spheres.json")).read().replace('"vfov": 45,', f'"vfov": 45, {bad},')
        assert bad in text
        scene = tmp_path / "bad.json"
        scene.write_text(text)
        with pytest.raises(ValueError):
            pkg.json_parser.scene_from_json(str(scene))
        r = _hip_pt("--dump-scene", str(tmp_path / "bad.bin"), str(scene))
        assert r.returncode == 1 and bad.split('"')[1] in r.stderr, r.stderr


def test_the_python_mirror_checks_the_lens(pkg):
    with pkg.PathTracer.__new__(pkg.PathTracer) as pt:
        pt._ctx = None
        pt._lens = (0.0, 1.0)
        for bad in ((-1.0, 1.0), (float("nan"), 1.0), (0.1, 0.0), (0.1, float("inf")), (0.1, -2.0)):
            with pytest.raises(ValueError):
                pt.lens = bad
            assert pt.lens == (0.0, 1.0)
        pt.lens = (0.0, 0.0)  # the pinhole asks nothing of the focus distance
        pt.lens = (0.25, 3.0)
        assert pt.lens == (0.25, 3.0)
