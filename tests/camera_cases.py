"""One table of cameras at and beyond the limits of what a camera can be, for the entry points of primary rays ("beam":
pt_beam_rules.hpp, k_beam) and for ray generation.  TEST INFRASTRUCTURE, used by tests/test_camera_cases_cpu.py (the host
checks) and tests/test_gpu_camera_range.py (entries, rays and frames on the GPU).

A case names a mesh, an object matrix (or None), a camera, a frame size and two flags:
  render    frames may be rendered with it: its restated primary rays are all finite (the GPU suite checks the flag against
            the restatement).  False for a NaN or infinite vfov: entries and rays only.
  cpu_only  a full-HD frame: the host checks only.
Groups: "telephoto" (the four cameras found unsound at the parent), "sweep" (seeded: tile angles 3e-4 .. 1e-5 rad, both meshes,
both frame sizes, 12 directions each), "fullhd" (CPU only), "vfov", "rotation", "position", "frame", "matrix".

tile_angle(case): the angle an 8-pixel tile subtends at the frame's centre, 8 * vfov / h to first order -- what decides how
well conditioned a frustum built from neighbouring corner rays is."""
import collections
import math

import numpy as np

Case = collections.namedtuple("Case", "name group mesh matrix camera w h render cpu_only")

TARGET = (0.1, 0.0, -0.1)         # what the seeded cameras look at
SWEEP_ANGLES = (3e-4, 1e-4, 5e-5, 1e-5)
SWEEP_DIRECTIONS = 12
SMALL_FRAMES = ((64, 40), (101, 67))
VISIBLE = {"hf": 7.3, "ball": 2.45}   # vertical extent in view at the look-at target: the mesh fills the frame

_cache = {}


def meshes(pkg):
    if "meshes" not in _cache:
        _cache["meshes"] = {"hf": pkg.scenes.heightfield_mesh(65, 33, 8.0, 4.0, seed=7), "ball": pkg.scenes.displaced_sphere_mesh(16, 32),
                            "two_triangles": pkg.scenes.heightfield_mesh(2, 2, 1.0, 1.0, seed=1)}
    return _cache["meshes"]


def tile_angle(case):
    return 8.0 * float(case.camera.vfov) / case.h


def _telescope(pkg, direction, vfov, mesh):
    """a camera along `direction` from TARGET at the distance at which `mesh` fills a frame of vertical field vfov (radians)"""
    dist = VISIBLE[mesh] / (2.0 * math.tan(0.5 * vfov))
    eye = tuple(TARGET[k] + dist * float(direction[k]) for k in range(3))
    return pkg.scenes._camera_from_look_at(eye, TARGET, vfov_deg=math.degrees(vfov))


def _quat_forward(q):
    """where the camera of quaternion q (w, x, y, z; float64, normalised here) looks: R(q) (0, 0, -1)"""
    w, x, y, z = (float(v) for v in q)
    n = math.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    return (-(2.0 * (x * z + w * y)), -(2.0 * (y * z - w * x)), -(1.0 - 2.0 * (x * x + y * y)))


def _facing(pkg, q, vfov_deg, dist=6.0, scale=1.0):
    """the camera with rotation q * scale that sees the origin from `dist` away: with an axis-aligned q its eye lies on an axis"""
    f = _quat_forward(q)
    return pkg.Camera(position=tuple(-dist * c + 0.0 for c in f), rotation=tuple(float(np.float32(c) * np.float32(scale)) for c in q),
                      vfov=float(np.float32(math.radians(vfov_deg))))


def _world_view(pkg, mesh, m, direction=(0.3, 0.5, 1.0), vfov_deg=40.0):
    """a camera that sees `mesh` under the object matrix m: its transformed box's centre from 2.5 half-diagonals away"""
    p = np.concatenate([mesh.positions.astype(np.float64), np.ones((len(mesh.positions), 1))], axis=1) @ np.asarray(m, dtype=np.float64).reshape(4, 4)
    lo, hi = p[:, :3].min(axis=0), p[:, :3].max(axis=0)
    c, r = 0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo))
    d = np.asarray(direction, dtype=np.float64) / np.linalg.norm(direction)
    return pkg.scenes._camera_from_look_at(tuple(c + 2.5 * r * d), tuple(c), vfov_deg=vfov_deg)


def matrices(pkg):
    glm = pkg.glmlite
    return {
        "mirror": glm.scale((-1.0, 1.0, 1.0)),
        "scale_1e-4": glm.scale(1e-4),
        "scale_1e4": glm.scale(1e4),
        "flattened_1e-5": glm.scale((1.0, 1e-5, 1.0)),
        "singular": glm.scale((1.0, 0.0, 1.0)),
        "translated_1e4": glm.translate((1e4, -1e4, 1e4)),
        "needle_rotated": glm.compose([glm.scale((1e3, 1.0, 1e-3)), glm.rotate(np.float32(0.6), (0.4, 1.0, 0.3))]),
        "rotated_scaled": glm.compose([glm.rotate(np.float32(0.7), (0.3, 1.0, 0.2)), glm.scale((0.8, 0.5, 1.2)), glm.translate((0.1, -0.2, 0.3))]),
    }


def cases(pkg):
    """every case of the table, in a fixed order"""
    if "cases" in _cache:
        return _cache["cases"]
    look = pkg.scenes._camera_from_look_at
    Camera = pkg.Camera
    out = []

    def add(name, group, mesh, camera, w=64, h=40, matrix=None, render=True):
        out.append(Case(name, group, mesh, matrix, camera, w, h, render, w * h > 101 * 67))

    # ---- telephoto: the four small cameras found unsound at the parent, as found
    for name, mesh, w, h, eye, deg in (("tele_hf_a", "hf", 64, 40, (-1005.33, 13032.12, 6411.88), 0.028648),
                                       ("tele_hf_b", "hf", 64, 40, (-44948.73, -18282.77, 672.14), 0.0085944),
                                       ("tele_ball_a", "ball", 64, 40, (-3243.68, -6195.59, -566.68), 0.020054),
                                       ("tele_ball_b", "ball", 101, 67, (-4124.24, -112.88, -4167.54), 0.023993)):
        add(name, "telephoto", mesh, look(eye, TARGET, vfov_deg=deg), w, h)
    # ---- the seeded sweep: per tile angle, mesh and frame size, SWEEP_DIRECTIONS random unit directions
    for angle in SWEEP_ANGLES:
        for mesh in ("hf", "ball"):
            for w, h in SMALL_FRAMES:
                rng = np.random.default_rng(2026)
                for k in range(SWEEP_DIRECTIONS):
                    d = rng.normal(size=3)
                    d /= np.linalg.norm(d)
                    add(f"sweep_{angle:g}_{mesh}_{w}x{h}_{k}", "sweep", mesh, _telescope(pkg, d, angle * h / 8.0, mesh), w, h)
    # ---- full HD (CPU only): 40 seeded cameras with vfov uniform in [0.3, 1.6] degrees, and the two named ones
    rng = np.random.default_rng(2026)
    for k in range(40):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        add(f"fullhd_{k}", "fullhd", "hf", _telescope(pkg, d, math.radians(rng.uniform(0.3, 1.6)), "hf"), 1920, 1080)
    add("fullhd_named_a", "fullhd", "hf", look((-26.314, -316.849, 637.178), TARGET, vfov_deg=0.5857), 1920, 1080)
    add("fullhd_named_b", "fullhd", "hf", look((20.950, -409.025, -260.715), TARGET, vfov_deg=0.8591), 1920, 1080)
    # ---- wide and degenerate vertical fields
    base = look((0.0, 2.0, 4.5), (0.0, 0.0, 0.0), vfov_deg=50.0)

    def with_vfov(v):
        return Camera(position=base.position, rotation=base.rotation, vfov=float(v))

    for name, v in (("120deg", math.radians(120.0)), ("170deg", math.radians(170.0)), ("179deg", math.radians(179.0)),
                    ("179.999deg", math.radians(179.999)), ("pi_f32", float(np.float32(np.pi))), ("3.5", 3.5), ("2pi", 2.0 * math.pi),
                    ("zero", 0.0), ("minus_half", -0.5), ("1e-8", 1e-8)):
        add("vfov_" + name, "vfov", "hf", with_vfov(np.float32(v)))
    add("vfov_nan", "vfov", "hf", with_vfov(float("nan")), render=False)
    add("vfov_inf", "vfov", "hf", with_vfov(float("inf")), render=False)
    # ---- rotations: the identity, the six axis-aligned ones from eyes on the axes, a generic one and its multiples
    r = math.sqrt(0.5)
    for name, q in (("identity", (1.0, 0.0, 0.0, 0.0)), ("x_plus", (r, r, 0.0, 0.0)), ("x_minus", (r, -r, 0.0, 0.0)), ("y_quarter", (r, 0.0, r, 0.0)),
                    ("y_half", (0.0, 0.0, 1.0, 0.0)), ("diagonal", (0.5, 0.5, 0.5, 0.5))):
        add("rot_" + name, "rotation", "hf", _facing(pkg, q, 50.0))
    generic = look((2.0, 2.5, 3.5), (0.2, 0.0, -0.3), vfov_deg=50.0)
    add("rot_generic", "rotation", "hf", generic)
    for s in (2.0, 1e-3, 1e3, -1.0):
        add(f"rot_generic_x{s:g}", "rotation_scaled", "hf",
            Camera(position=generic.position, rotation=tuple(float(np.float32(c) * np.float32(s)) for c in generic.rotation), vfov=generic.vfov))
    # (the zero quaternion: mat4_cast does not normalise, the rotation it gives is the identity and every ray is finite)
    add("rot_generic_x0", "rotation_scaled", "hf", Camera(position=generic.position, rotation=(0.0, 0.0, 0.0, 0.0), vfov=generic.vfov))
    # ---- positions
    hf = meshes(pkg)["hf"]
    vertex = tuple(float(c) for c in hf.positions[len(hf.positions) // 2 + 7])
    add("pos_inside_box", "position", "hf", look((0.5, 0.05, 0.3), (3.0, 0.0, -1.0), vfov_deg=70.0))
    add("pos_on_box_face", "position", "hf", look((4.0, 0.02, 0.5), (0.0, 0.0, 0.0), vfov_deg=60.0))
    add("pos_on_vertex", "position", "hf", look(vertex, (vertex[0] + 1.0, vertex[1] - 0.1, vertex[2] + 0.5), vfov_deg=60.0))
    far = np.array([0.3, 0.5, 0.8]) / np.linalg.norm([0.3, 0.5, 0.8])
    for dist in (1e4, 1e6, 1e8):
        add(f"pos_far_{dist:g}", "position_far", "hf", look(tuple(dist * far), (0.0, 0.0, 0.0), vfov_deg=math.degrees(2.0 * math.atan(0.5 * VISIBLE["hf"] / dist))))
    # ---- frame sizes at an ordinary camera
    for w, h in ((2, 2), (2, 64), (64, 2), (3, 3), (8, 8), (9, 9), (7, 130), (257, 4), (101, 67)):
        add(f"frame_{w}x{h}", "frame", "hf", base, w, h)
    # ---- object matrices, each seen by a camera that looks at the transformed mesh
    for name, m in matrices(pkg).items():
        mesh = "ball" if name == "rotated_scaled" else "hf"
        # (the needle is 8000 long and 0.004 thick: seen whole it falls between the pixels, so its camera stands close to its middle)
        camera = look((0.5, 1.5, 2.5), (0.0, 0.0, 0.0), vfov_deg=40.0) if name == "needle_rotated" else _world_view(pkg, meshes(pkg)[mesh], m)
        add("matrix_" + name, "matrix", mesh, camera, matrix=m)
    assert len({c.name for c in out}) == len(out)
    _cache["cases"] = out
    return out


def by_name(pkg, name):
    return next(c for c in cases(pkg) if c.name == name)


def camera_c(pkg, camera):
    cam = pkg._capi.ptc_camera()
    cam.position[:] = [float(x) for x in camera.position]
    cam.rotation_wxyz[:] = [float(x) for x in camera.rotation]
    cam.vfov = float(camera.vfov)
    return cam


def matrix16(case):
    """the case's object matrix as 16 contiguous binary32 values (the identity where it has none)"""
    m = np.eye(4, dtype=np.float32) if case.matrix is None else np.asarray(case.matrix, dtype=np.float32)
    return np.ascontiguousarray(m.reshape(16))


def beam_check(pkg, case, stride=1, entries=False):
    """ptc_check_beam on the case -> (disagreeing rays, [tiles, tiles without entries, entries, rays, hits], entries or None)"""
    import ctypes as C
    mesh = meshes(pkg)[case.mesh]
    pos = np.ascontiguousarray(mesh.positions, dtype=np.float32)
    idx = np.ascontiguousarray(mesh.indices, dtype=np.uint32)
    cam = camera_c(pkg, case.camera)
    m = matrix16(case)
    stats = (C.c_uint64 * 5)()
    tiles = ((case.w + 7) // 8) * ((case.h + 7) // 8)
    ent = np.zeros(tiles * 32, dtype=np.float32) if entries else None
    bad = pkg.lib().ptc_check_beam(pos.ctypes.data, len(pos), idx.ctypes.data, len(idx), m.ctypes.data, C.byref(cam), case.w, case.h, stride, stats,
                                   ent.ctypes.data if entries else None)
    return bad, [int(x) for x in stats], ent
