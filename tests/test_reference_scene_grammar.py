"""The reference's OWN scene files through both front-ends (Python json_parser.py, C++ host/scene_description.cpp via
hip_pt --dump-scene): the reference's assets/scenes/{bunny,ajax-white,three_balls}.json, stored unchanged as test
fixtures under tests/golden/reference_scenes/.  Their meshes are git-LFS pointers, so `../models/*.obj` is served by this
repository's small stand-in OBJ; what is pinned is the GRAMMAR (assets/json_parser.cpp:40-95,174-224): a transform array
applies its commands left to right as elem * mat, from/at/up builds the camera frame, vfov is in degrees, materials are
indexed in name order, "background" / "accelerator" are ignored, and three_balls.json's camera key "o" is an error in
the reference too.  Expected matrices are computed here in float64 from the formulas, not by the
code under test."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_SCENES = os.path.join(ROOT, "tests", "golden", "reference_scenes")
HIP_PT = os.path.join(ROOT, "cuda-path-tracer_amd", "host", "hip_pt")


def T(v):
    m = np.eye(4)
    m[:3, 3] = v
    return m


def S(s):
    return np.diag([s, s, s, 1.0])


def R(deg, axis):
    a = np.radians(deg)
    x, y, z = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    c, s = np.cos(a), np.sin(a)
    k = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    m = np.eye(4)
    m[:3, :3] = c * np.eye(3) + s * k + (1 - c) * np.outer([x, y, z], [x, y, z])
    return m


def colmajor(m16):
    """16 floats in glm's column-major order -> a 4x4 matrix in the usual row/column notation"""
    return np.asarray(m16, dtype=np.float64).reshape(4, 4).T


def quat_matrix(w, x, y, z):
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


@pytest.fixture(scope="module")
def staged(tmp_path_factory):
    """assets/scenes/<the reference's files> + assets/models/<stand-in meshes> under a temporary directory"""
    base = tmp_path_factory.mktemp("refscenes")
    scenes, models = base / "assets" / "scenes", base / "assets" / "models"
    scenes.mkdir(parents=True)
    models.mkdir()
    for name in ("bunny.json", "ajax-white.json", "three_balls.json"):
        shutil.copy(os.path.join(REF_SCENES, name), scenes / name)
    stand_in = os.path.join(ROOT, "assets", "models", "displaced_sphere_small.obj")
    for name in ("bunny.obj", "ajax.obj"):
        shutil.copy(stand_in, models / name)
    return scenes


def cpp_dump(path, pkg, tmp_path):
    if not os.path.exists(HIP_PT):
        subprocess.run(["make"], cwd=os.path.dirname(HIP_PT), check=True, stdout=subprocess.DEVNULL)
    out = tmp_path / "dump.bin"
    r = subprocess.run([HIP_PT, "--dump-scene", str(out), str(path)], capture_output=True, text=True)
    if r.returncode != 0:
        return None, r.stderr
    data = open(out, "rb").read()
    n = struct.unpack_from("<Q", data, 0)[0]
    objects = np.frombuffer(data, dtype=pkg.scene_description.OBJECT_DTYPE, count=n, offset=8)
    off = 8 + n * 160
    n2 = struct.unpack_from("<Q", data, off)[0]
    mats = np.frombuffer(data, dtype="<u4", count=n2, offset=off + 8)
    cam = np.frombuffer(data, dtype="<f4", count=8, offset=len(data) - 44)
    tail = np.frombuffer(data, dtype="<i4", count=3, offset=len(data) - 12)
    return {"objects": objects, "object_material_indices": mats, "camera": cam, "tail": tail}, r.stderr


def test_bunny_json(pkg, staged, tmp_path):
    """bunny.json:37-57: a sphere, a mesh with one command, a mesh with an ARRAY [scale 0.5, translate]: m = T * S"""
    py = pkg.json_parser.scene_from_json(str(staged / "bunny.json"))
    flat = py.build_scene()
    want = [T([0.0, -100.5, -1.0]), T([1.0, -0.5, -2.0]), T([-1.0, -0.5, -2.0]) @ S(0.5)]
    assert [int(t) for t in flat.objects["type"]] == [0, 1, 1]
    for k in range(3):
        assert np.allclose(colmajor(flat.objects["m"][k]), want[k], atol=1e-6), k
        assert np.allclose(colmajor(flat.objects["inv_m"][k]), np.linalg.inv(want[k]), atol=1e-5), k
    # the order matters: translate-then-scale would put the second bunny at (-0.5, -0.25, -1)
    assert not np.allclose(colmajor(flat.objects["m"][2]), S(0.5) @ T([-1.0, -0.5, -2.0]), atol=1e-3)
    # materials in NAME order (std::map, scene_description.cpp:59-66): bunny, bunny2, ground
    assert [int(i) for i in flat.object_material_indices] == [2, 0, 1]
    assert np.allclose(flat.materials["p"][0][:3], [0.8, 0.8, 0.5]) and np.allclose(flat.materials["p"][2][:3], [0.8, 0.8, 0.8])
    # no camera transform: default camera; vfov in degrees; resolution; sampler.samples; "background" is ignored
    assert np.allclose(py.camera.position, [0, 0, 0]) and np.allclose(py.camera.rotation, [1, 0, 0, 0])
    assert np.isclose(py.camera.vfov, np.radians(60.0)) and tuple(py.resolution) == (1920, 1080) and py.spp == 10
    # one mesh per scene whatever the file says (scene_description.cpp:42,95): both mesh objects instantiate it
    assert flat.mesh_ranges is None and len(flat.spheres) == 1 and np.isclose(flat.spheres[0][3], 100.0)
    cpp, err = cpp_dump(staged / "bunny.json", pkg, tmp_path)
    assert cpp is not None, err
    assert np.array_equal(cpp["object_material_indices"], flat.object_material_indices)
    for k in range(3):
        assert np.allclose(colmajor(cpp["objects"]["m"][k]), want[k], atol=1e-6), k
    assert tuple(cpp["tail"]) == (1920, 1080, 10) and np.isclose(cpp["camera"][7], np.radians(60.0))


def test_ajax_white_json(pkg, staged, tmp_path):
    """ajax-white.json:3-7: camera from/at/up; :33-47: an array of four commands (translate, scale, rotate, translate)"""
    py = pkg.json_parser.scene_from_json(str(staged / "ajax-white.json"))
    flat = py.build_scene()
    want = T([0, 0, -0.25]) @ R(150.0, [0, 1, 0]) @ S(0.2) @ T([-0.053126335, 0.030193329, 17.283958])
    assert np.allclose(colmajor(flat.objects["m"][0]), want, atol=2e-6)
    # json_parser.cpp:58-70: dir = normalize(from - at), left = normalize(cross(up, dir)), new_up = normalize(cross(dir, left));
    # columns (left, new_up, dir, from); the camera gets the translation and the rotation of that matrix (:190-203)
    frm, at, up = np.array([6.0, 5.5, 0.0]), np.array([0.0, 3.5, 0.0]), np.array([0.0, 1.0, 0.0])
    d = (frm - at) / np.linalg.norm(frm - at)
    left = np.cross(up, d) / np.linalg.norm(np.cross(up, d))
    new_up = np.cross(d, left) / np.linalg.norm(np.cross(d, left))
    frame = np.stack([left, new_up, d], axis=1)
    assert np.allclose(py.camera.position, frm, atol=1e-6)
    assert np.allclose(quat_matrix(*[float(v) for v in py.camera.rotation]), frame, atol=1e-6)
    assert np.isclose(py.camera.vfov, np.radians(80.0)) and tuple(py.resolution) == (720, 1280)
    cpp, err = cpp_dump(staged / "ajax-white.json", pkg, tmp_path)
    assert cpp is not None, err
    assert np.allclose(colmajor(cpp["objects"]["m"][0]), want, atol=2e-6)
    assert np.allclose(cpp["camera"][:3], frm, atol=1e-6)
    assert np.allclose(quat_matrix(*[float(v) for v in cpp["camera"][3:7]]), frame, atol=1e-6)
    assert tuple(cpp["tail"]) == (720, 1280, 10)


def test_three_balls_json_is_an_error_like_in_the_reference(pkg, staged, tmp_path):
    """three_balls.json:3-9: the camera transform uses the key "o": json_parser.cpp:71-74 panics with
    "Unrecognized transform command" (SURVEY section 0); both front-ends report the same"""
    with pytest.raises(ValueError, match="Unrecognized transform command"):
        pkg.json_parser.scene_from_json(str(staged / "three_balls.json"))
    cpp, err = cpp_dump(staged / "three_balls.json", pkg, tmp_path)
    assert cpp is None and "Unrecognized transform command" in err
