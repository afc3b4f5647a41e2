"""Image textures without a GPU (ptc_texture_decode_table, ptc_check_texture_lookup): the decode tables against their
formula, the host twin of the lookup against the numpy restatement tests/texture_ref.py bit for bit and against an independent float64
bilinear, and the restatement's loop against the loop it extends."""
import ctypes as C

import numpy as np
import pytest

import env_light_ref
import loop_ref
import smooth_ref
import texture_ref

ENV = smooth_ref.ENV
W, H = 33, 17
PLANES = ("color", "normal", "depth")
_cache = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. the table ------------------------------------------------------------------------------------------------------------------------
def test_the_linear_table_is_k_over_255_rounded(pkg):
    got = pkg.texture_decode_table("linear")
    want = np.arange(256, dtype=np.float32) / np.float32(255.0)  # numpy's binary32 division: one rounding of the exact quotient
    assert np.array_equal(_bits(got), _bits(want))


def test_the_srgb_table_is_within_one_ulp_of_the_curve(pkg):
    got = pkg.texture_decode_table("srgb")
    want = texture_ref.table_f64(texture_ref.SRGB)
    ulp = np.spacing(want.astype(np.float32)).astype(np.float64)
    assert (np.abs(got.astype(np.float64) - want) <= ulp).all()


@pytest.mark.parametrize("encoding", ["linear", "srgb"])
def test_the_table_is_monotone_from_0_to_1(pkg, encoding):
    t = pkg.texture_decode_table(encoding)
    assert t[0] == 0.0 and t[255] == 1.0 and (np.diff(t) > 0).all()
    assert np.array_equal(t, pkg.texture_decode_table({"linear": 0, "srgb": 1}[encoding]))


def test_the_table_refuses_an_unknown_encoding(pkg):
    out = np.zeros(256, np.float32)
    assert pkg.lib().ptc_texture_decode_table(2, out.ctypes.data_as(C.c_void_p)) == -1
    assert pkg.lib().ptc_texture_decode_table(0, None) == -1


# ---- 2. the lookup against the restatement -------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (2, 2), (3, 5), (4096, 2), (2, 4096)]


@pytest.mark.parametrize("width,height", SIZES)
def test_lookup_against_the_restatement(pkg, width, height):
    st = texture_ref.coordinate_set(width, height)
    for filt in ("nearest", "bilinear"):
        for wrap in ("repeat", "clamp"):
            for enc in ("linear", "srgb"):
                tex = texture_ref.random_texture(pkg, width, height, 7 * width + height, encoding=enc, filter=filt, wrap=wrap)
                got, rej = pkg.check_texture_lookup(tex, st)
                want, wrej = texture_ref.lookup(pkg, tex, st)
                bad = np.argwhere(_bits(got) != _bits(want))
                assert len(bad) == 0, (filt, wrap, enc, st[bad[:4, 0]].tolist(), got[bad[:4, 0]].tolist(), want[bad[:4, 0]].tolist())
                assert np.array_equal(rej, wrej)
                finite = np.isfinite(st).all(axis=1)
                assert np.array_equal(rej, ~finite)  # FLT_MAX is looked up; an infinity and a NaN are not
                assert not got[rej].any() and (got >= 0).all() and (got <= 1).all()


def test_what_the_special_coordinates_give(pkg):
    """a 2 x 2 texture with four different texels, nearest, so that the texel a coordinate picks can be read off the result"""
    texels = np.zeros((2, 2, 4), np.uint8)
    texels[..., 0] = [[10, 20], [30, 40]]  # [row t][column s]
    pick = lambda wrap, s, t: int(round(float(pkg.check_texture_lookup(pkg.Texture(texels, "linear", "nearest", wrap), [[s, t]])[0][0, 0]) * 255))
    assert pick("repeat", 0.25, 0.25) == 10 and pick("repeat", 0.75, 0.25) == 20 and pick("repeat", 0.25, 0.75) == 30  # row 0 is t = 0
    assert pick("repeat", 1.0, 0.0) == 10 and pick("clamp", 1.0, 0.0) == 20  # 1 wraps to 0 under repeat and is the last texel under clamp
    assert pick("repeat", -1e-30, 0.0) == 10  # x - floor(x) rounds to 1: taken as 0
    assert pick("repeat", np.float32(1.0) - np.float32(2.0 ** -24), 0.0) == 20
    assert pick("repeat", -0.25, 0.0) == 20 and pick("clamp", -0.25, 0.0) == 10 and pick("clamp", 7.0, 9.0) == 40
    assert pick("repeat", -0.0, 0.0) == 10


def test_lookup_refusals(pkg):
    ok = texture_ref.random_texture(pkg, 2, 2, 1)
    st = np.zeros((1, 2), np.float32)
    out = np.zeros((1, 3), np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)

    def rc(**kw):
        d = ok._desc()
        for k, v in kw.items():
            setattr(d, k, v)
        return pkg.lib().ptc_check_texture_lookup(C.byref(d), vp(st), 1, vp(out), None)

    assert rc() == 0
    for kw in ({"width": 0}, {"height": 4097}, {"rgba8": None}, {"encoding": 2}, {"filter": 2}, {"wrap": 2}):
        assert rc(**kw) == -1, kw
    assert pkg.lib().ptc_check_texture_lookup(None, vp(st), 1, vp(out), None) == -1


# ---- 3. the lookup against an independent float64 bilinear -------------------------------------------------------------------------------
@pytest.mark.parametrize("width,height", [(2, 2), (3, 5), (64, 3)])
@pytest.mark.parametrize("wrap", ["repeat", "clamp"])
def test_bilinear_against_float64(pkg, width, height, wrap):
    """The bound, from the rule's operations on a coordinate |x| <= 3 and decoded texels in [0, 1], with e = 2^-24:
      - f = x - floor(x) is exact for such x (the difference is a multiple of ulp(x) below 1); the clamp is exact;
      - g = f n rounds once: |dg| <= n e; h = g - 0.5 and a = h - floor(h) round once each, results below 1: |da| <= n e + 2 e;
      - the result is piecewise bilinear and continuous in (g_s, g_t) with slopes at most the largest texel difference, 1: the weights'
        errors move it by at most |da_s| + |da_t| <= (w + h + 4) e, across a texel boundary too;
      - a mix is four roundings of values in [0, 1] (1 - a, two products, one sum): 4 e; the outer mix passes the inner two on with
        weights that sum to 1 and adds its own: 8 e;
      - the table entry is one rounding of the float64 curve: e, passed on with weights that sum to 1.
    Together (w + h + 13) e."""
    st = np.random.default_rng(5).uniform(-3.0, 3.0, (512, 2)).astype(np.float32)
    bound = (width + height + 13) * 2.0 ** -24
    for enc in ("linear", "srgb"):
        tex = texture_ref.random_texture(pkg, width, height, 3 * width + height, encoding=enc, filter="bilinear", wrap=wrap)
        got = pkg.check_texture_lookup(tex, st)[0].astype(np.float64)
        err = np.abs(got - texture_ref.lookup_f64(tex, st)).max()
        print("bilinear vs float64", width, height, wrap, enc, "max error", err, "bound", bound)
        assert err <= bound


# ---- 4. the loop restatement -------------------------------------------------------------------------------------------------------------
def _sheet(pkg):
    if "sheet" not in _cache:
        scene = smooth_ref.sheet_scene(pkg, ("diffuse", "metal"))
        flat = scene.build_scene(distinct_meshes=True)
        binding = texture_ref.bind(scene, flat, {"sheet": 0, "diffuse": 1, "metal": 2, "floor": 1})
        _cache["sheet"] = (scene, flat, texture_ref.pool(pkg), binding, texture_ref.random_texcoords(flat), smooth_ref.scene_vertex_normals(flat))
    return _cache["sheet"]


def test_loop_off_is_the_loop_it_extends(pkg, orc):
    scene, flat, textures, binding, st, nrm = _sheet(pkg)
    entries = env_light_ref.table_of(pkg, ENV)[0]
    kw = dict(env=ENV, entries=entries, env_light=True, normals=nrm, smooth=True)
    want = loop_ref.render_megakernel(orc, flat, scene.camera, W, H, 0, 1, 4, **kw)
    for tx in (dict(textures=textures, binding=binding, texcoords=st, textured=False), dict(textures=None, texcoords=st, textured=True),
               dict(textures=textures, binding=binding, texcoords=None, textured=True)):
        got = loop_ref.render_megakernel(orc, flat, scene.camera, W, H, 0, 1, 4, pkg=pkg, **tx, **kw)
        for k in want:
            assert np.array_equal(got[k], want[k]), k
        assert all(got[k] == 0 for k in texture_ref.COUNTERS)


@pytest.mark.parametrize("smooth", [False, True])
@pytest.mark.parametrize("lights", ["none", "env", "env_mis"])
def test_white_textures_give_the_bits_of_the_loop_it_extends(pkg, orc, smooth, lights):
    """every texel 255 under the linear table is the factor 1.0f: the loop with the option on, under smooth shading or not, walks to the
    bits of the loop without it -- the winners, the lookup and the material copies change nothing but the albedo"""
    scene, flat, _, binding, st, nrm = _sheet(pkg)
    white = [pkg.Texture(np.full((2, 3, 4), 255, np.uint8), "linear", "nearest", "repeat")] * 3
    entries = env_light_ref.table_of(pkg, ENV)[0]
    kw = dict(normals=nrm, smooth=smooth)
    if lights != "none":
        kw.update(env=ENV, entries=entries, env_light=True, mis=lights == "env_mis")
    want = loop_ref.render_megakernel(orc, flat, scene.camera, W, H, 0, 1, 4, **kw)
    got = loop_ref.render_megakernel(orc, flat, scene.camera, W, H, 0, 1, 4, textures=white, binding=binding, texcoords=st, textured=True, pkg=pkg, **kw)
    for k in set(want) - set(texture_ref.COUNTERS):  # everything but the texture's own two counters
        assert np.array_equal(got[k], want[k]), k
    assert got["lookups"] > 0


def test_loop_on_changes_the_colour_alone(pkg, orc):
    scene, flat, textures, binding, st, _ = _sheet(pkg)
    off = loop_ref.render_megakernel(orc, flat, scene.camera, W, H, 0, 1, 4)
    on = loop_ref.render_megakernel(orc, flat, scene.camera, W, H, 0, 1, 4, textures=textures, binding=binding, texcoords=st, textured=True, pkg=pkg)
    assert (on["color"] != off["color"]).any()
    assert np.array_equal(on["normal"], off["normal"]) and np.array_equal(on["depth"], off["depth"]) and on["rays"] == off["rays"]


def test_the_counters_move_on_the_gpu_tests_scenes(pkg, orc):
    """what test_gpu_texture.py compares on these scenes is not a row of zeros"""
    scene, flat, textures, binding, st, _ = _sheet(pkg)
    bad = st.copy()
    bad[::7, 0] = np.nan
    bad[3::11, 1] = np.inf
    out = loop_ref.render_megakernel(orc, flat, scene.camera, 65, 33, 0, 1, 8, textures=textures, binding=binding, texcoords=bad, textured=True, pkg=pkg)
    assert all(out[k] > 0 for k in texture_ref.COUNTERS), {k: out[k] for k in texture_ref.COUNTERS}


# ---- 5. the readers: OBJ `vt`, PNG, the scene keys ----------------------------------------------------------------------------------------
import json  # noqa: E402
import os  # noqa: E402
import subprocess  # noqa: E402
import sys  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_PT = os.path.join(ROOT, "cuda-path-tracer_amd", "host", "hip_pt")
TEXTURES = os.path.join(ROOT, "tests", "golden", "textures")

OBJ = """# a seam, negative indices, faces without vt, a polygon fan
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
v 2 0.5 0
vt 0 0
vt 1 0
vt 1 1
vt 0 1
vt 0.25 0.75
f 1/1 2/2 3/3
f 1/5 3/3 4/4
f 1 2 3
f 1//1 2//1 3//1
f -5/-5 -4/-4 5/-1 -3/-3 -2/-2
f 1/9 2/2 3/3
"""
# per corner, by hand: vertex 1 carries vt 1 in the first face and vt 5 in the second (a seam); the third and fourth face have no vt; the
# fifth is a pentagon (three triangles about its first corner) in negative indices; vt 9 does not exist
OBJ_INDICES = [0, 1, 2, 0, 2, 3, 0, 1, 2, 0, 1, 2, 0, 1, 4, 0, 4, 2, 0, 2, 3, 0, 1, 2]
OBJ_ST = [(0, 0), (1, 0), (1, 1), (.25, .75), (1, 1), (0, 1), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0),
          (0, 0), (1, 0), (.25, .75), (0, 0), (.25, .75), (1, 1), (0, 0), (1, 1), (0, 1), (0, 0), (1, 0), (1, 1)]


def _scene_json(path, obj, materials, extra=None):
    """a one-mesh scene file at `path` (its mesh and textures named relative to it)"""
    rel = lambda p: os.path.relpath(p, os.path.dirname(path))
    j = {"camera": {"vfov": 45, "resolution": [8, 8]}, "materials": [], "surfaces": []}
    for name, (kind, tex) in materials.items():
        m = {"name": name, "type": kind}
        m.update({"albedo": [0.5, 0.5, 0.5]} if kind in ("lambertian", "metal") else {"refraction_index": 1.5})
        if kind == "metal":
            m["fuzz"] = 0.1
        if tex is not None:
            m["texture"] = dict(tex, file=rel(tex["file"])) if isinstance(tex, dict) and "file" in tex else tex
        j["materials"].append(m)
        j["surfaces"].append({"type": "mesh", "filename": rel(obj), "material": name, "transform": {"translate": [0, 0, -3]}})
    j.update(extra or {})
    with open(path, "w") as f:
        json.dump(j, f)
    return path


def _hip_pt(*args):
    if not os.path.exists(HIP_PT):
        pytest.fail("hip_pt is not built (build() makes it)")
    return subprocess.run([HIP_PT, *args], cwd=ROOT, capture_output=True, text=True)


def _read_dump(path):
    """hip_pt --dump-scene: six arrays (a uint64 count and the bytes each), the camera, resolution and spp, and -- for a scene with
    texture coordinates or textures -- the tag TEX0, the coordinates, the binding and the decoded textures
    -> dict(positions, indices, texcoords or None, material_texture, textures [(w, h, encoding, filter, wrap, rgba)])"""
    data = open(path, "rb").read()
    at, arrays = 0, []
    for size, dtype in ((160, np.uint8), (4, np.uint32), (16, np.float32), (20, np.uint8), (4, np.float32), (4, np.uint32)):
        n = int(np.frombuffer(data, np.uint64, 1, at)[0])
        arrays.append(np.frombuffer(data, dtype, n * size // np.dtype(dtype).itemsize, at + 8))
        at += 8 + n * size
    at += 32 + 12  # ptc_camera, resolution and spp (no lens in these scenes)
    out = {"positions": arrays[4].reshape(-1, 3), "indices": arrays[5], "texcoords": None, "material_texture": None, "textures": []}
    if at == len(data):
        return out
    assert data[at:at + 4] == b"TEX0"
    at += 4
    n = int(np.frombuffer(data, np.uint64, 1, at)[0])
    out["texcoords"] = np.frombuffer(data, np.float32, n, at + 8).reshape(-1, 2)
    at += 8 + 4 * n
    n = int(np.frombuffer(data, np.uint64, 1, at)[0])
    out["material_texture"] = np.frombuffer(data, np.int32, n, at + 8)
    at += 8 + 4 * n
    count = int(np.frombuffer(data, np.uint64, 1, at)[0])
    at += 8
    for _ in range(count):
        w, h, enc, filt, wrap = (int(x) for x in np.frombuffer(data, np.uint32, 5, at))
        n = int(np.frombuffer(data, np.uint64, 1, at + 20)[0])
        out["textures"].append((w, h, enc, filt, wrap, np.frombuffer(data, np.uint8, n, at + 28).reshape(h, w, 4)))
        at += 28 + n
    assert at == len(data)
    return out


def test_obj_vt_in_both_readers(pkg, tmp_path):
    obj = tmp_path / "seam.obj"
    obj.write_text(OBJ)
    mesh = pkg.json_parser.load_obj(str(obj))
    assert mesh.indices.tolist() == OBJ_INDICES
    assert np.array_equal(mesh.texcoords, np.float32(OBJ_ST))
    assert np.array_equal(mesh.positions, np.float32([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [2, 0.5, 0]]))
    scene = _scene_json(str(tmp_path / "seam.json"), str(obj), {"a": ("lambertian", None)})
    flat = pkg.json_parser.scene_from_json(scene).build_scene()
    assert np.array_equal(flat.texcoords, mesh.texcoords) and flat.texture_sources is None
    r = _hip_pt("--dump-scene", str(tmp_path / "seam.bin"), scene)
    assert r.returncode == 0, r.stderr
    dump = _read_dump(str(tmp_path / "seam.bin"))
    assert np.array_equal(dump["positions"], mesh.positions) and np.array_equal(dump["indices"], mesh.indices)
    assert np.array_equal(dump["texcoords"], mesh.texcoords) and len(dump["textures"]) == 0 and len(dump["material_texture"]) == 0


def test_existing_files_read_as_before(pkg, tmp_path):
    """a file without `vt` records: positions and faces are those of a reader that knows only `v` and `f` (restated here), there are no
    coordinates, and hip_pt's dump of its scene has no texture tail"""
    path = os.path.join(ROOT, "assets", "models", "displaced_sphere_small.obj")
    pos, faces = [], []
    for line in open(path):
        if line.startswith("v "):
            pos.append([float(x) for x in line.split()[1:4]])
        elif line.startswith("f "):
            idx = [int(t.split("/")[0]) - 1 for t in line.split()[1:]]
            for k in range(1, len(idx) - 1):
                faces += [idx[0], idx[k], idx[k + 1]]
    mesh = pkg.json_parser.load_obj(path)
    assert mesh.texcoords is None
    assert np.array_equal(mesh.positions, np.float32(pos)) and mesh.indices.tolist() == faces  # (the file uses every vertex)
    flat = pkg.json_parser.scene_from_json(os.path.join(ROOT, "assets", "scenes", "cornell_mesh.json")).build_scene()
    assert flat.texcoords is None and flat.texture_sources is None and flat.material_texture is None
    r = _hip_pt("--dump-scene", str(tmp_path / "mesh.bin"), "assets/scenes/cornell_mesh.json")
    assert r.returncode == 0, r.stderr
    dump = _read_dump(str(tmp_path / "mesh.bin"))
    assert dump["texcoords"] is None and np.array_equal(dump["positions"], flat.positions) and np.array_equal(dump["indices"], flat.indices)


def _fixtures():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_texture_asset as gen
    same = np.random.default_rng(7).integers(0, 256, (6, 7, 4), dtype=np.uint8)
    rgb = gen.stripes()
    out = {"checker.png": gen.checker(), "stripes.png": rgb}
    out.update({f"filter_{k}.png": same for k in range(5)})
    return out


def test_png_fixtures_through_both_readers(pkg, tmp_path):
    """every fixture (all five scanline filters, RGB and RGBA) decodes to the generator's texels in both readers, rows flipped: the
    checker's bright mark, at the TOP left of the picture, ends in the texture's last rows"""
    want = _fixtures()
    for name, texels in want.items():
        got = pkg.png.read_png(os.path.join(TEXTURES, name))
        assert np.array_equal(got, texels), name
    assert (want["checker.png"][12:, :4, :3] == (255, 255, 0)).all() and not (want["checker.png"][:4, :4, :3] == (255, 255, 0)).all()
    raw = open(os.path.join(TEXTURES, "filter_0.png"), "rb").read()
    assert {open(os.path.join(TEXTURES, f"filter_{k}.png"), "rb").read() for k in range(5)}.__len__() == 5 and raw[:4] == b"\x89PNG"
    obj = tmp_path / "seam.obj"
    obj.write_text(OBJ)
    names = sorted(want)
    materials = {f"m{k}": ("metal" if k % 2 else "lambertian", {"file": os.path.join(TEXTURES, n), "encoding": "linear", "wrap": "clamp"})
                 for k, n in enumerate(names)}
    scene = _scene_json(str(tmp_path / "png.json"), str(obj), materials)
    flat = pkg.json_parser.scene_from_json(scene).build_scene()
    assert [os.path.basename(s.file) for s in flat.texture_sources] == names and flat.material_texture.tolist() == list(range(len(names)))
    assert all((s.encoding, s.filter, s.wrap) == ("linear", "bilinear", "clamp") for s in flat.texture_sources)
    r = _hip_pt("--method", "megakernel", "--dump-scene", str(tmp_path / "png.bin"), scene)
    assert r.returncode == 0, r.stderr
    dump = _read_dump(str(tmp_path / "png.bin"))
    assert dump["material_texture"].tolist() == flat.material_texture.tolist() and len(dump["textures"]) == len(names)
    for name, (w, h, enc, filt, wrap, rgba) in zip(names, dump["textures"]):
        assert (enc, filt, wrap) == (0, 1, 1) and np.array_equal(rgba, want[name]), name


@pytest.mark.parametrize("name,word", [("grey16.png", "bit depth 16"), ("palette.png", "colour type 3"), ("interlaced.png", "interlace 1"),
                                       ("truncated.png", "truncated"), ("missing.png", "missing.png")])
def test_png_refusals_name_the_file(pkg, tmp_path, name, word):
    path = os.path.join(TEXTURES, name)
    with pytest.raises((ValueError, OSError)) as e:
        pkg.png.read_png(path)
    assert name in str(e.value) and (word in str(e.value) or name == "missing.png")
    obj = tmp_path / "seam.obj"
    obj.write_text(OBJ)
    scene = _scene_json(str(tmp_path / "bad.json"), str(obj), {"a": ("lambertian", {"file": path})})
    r = _hip_pt("--method", "megakernel", "--dump-scene", str(tmp_path / "bad.bin"), scene)
    assert r.returncode != 0 and name in r.stderr and (word in r.stderr or name == "missing.png"), r.stderr


def test_the_scene_keys_in_both_readers(pkg, tmp_path):
    """defaults srgb, bilinear, repeat; the path relative to the scene file; "textures": true; and what both readers refuse"""
    obj = tmp_path / "seam.obj"
    obj.write_text(OBJ)
    tex = {"file": os.path.join(TEXTURES, "checker.png")}
    scene = _scene_json(str(tmp_path / "ok.json"), str(obj), {"a": ("lambertian", tex), "b": ("metal", dict(tex, filter="nearest")), "c": ("dielectric", None)},
                        {"textures": True})
    sd = pkg.json_parser.scene_from_json(scene)
    flat = sd.build_scene()
    assert sd.textures is True and flat.material_texture.tolist() == [0, 1, -1]
    assert [(s.encoding, s.filter, s.wrap) for s in flat.texture_sources] == [("srgb", "bilinear", "repeat"), ("srgb", "nearest", "repeat")]
    assert flat.texture_sources[0].file == os.path.join(TEXTURES, "checker.png")
    r = _hip_pt("--method", "megakernel", "--dump-scene", str(tmp_path / "ok.bin"), scene)
    assert r.returncode == 0, r.stderr
    dump = _read_dump(str(tmp_path / "ok.bin"))
    assert [t[2:5] for t in dump["textures"]] == [(1, 1, 0), (1, 0, 0)] and dump["material_texture"].tolist() == [0, 1, -1]
    # without the method that renders them: the key and a material's texture are refused once the scene is read, the flag at once
    for extra, word in (({"textures": True}, '"textures": true'), ({}, 'a material with a "texture"')):
        scene = _scene_json(str(tmp_path / "m.json"), str(obj), {"a": ("lambertian", tex if not extra else None)}, extra)
        r = _hip_pt("--dump-scene", str(tmp_path / "m.bin"), scene)
        assert r.returncode != 0 and word in r.stderr and "--method megakernel" in r.stderr, r.stderr
    r = _hip_pt("--textures", "--dump-scene", str(tmp_path / "m.bin"), "assets/scenes/cornell_mesh.json")
    assert r.returncode != 0 and "--textures needs --method megakernel" in r.stderr
    bad = [({"a": ("dielectric", tex)}, {}, "only a lambertian or a metal"), ({"a": ("lambertian", dict(tex, encoding="gamma"))}, {}, '"encoding"'),
           ({"a": ("lambertian", dict(tex, filter=1))}, {}, '"filter"'), ({"a": ("lambertian", dict(tex, wrap="mirror"))}, {}, '"wrap"'),
           ({"a": ("lambertian", dict(tex, mip=True))}, {}, '"texture" must be an object'), ({"a": ("lambertian", "checker.png")}, {}, '"texture" must be an object'),
           ({"a": ("lambertian", None)}, {"textures": 1}, '"textures" must be true or false')]
    for materials, extra, word in bad:
        scene = _scene_json(str(tmp_path / "bad.json"), str(obj), materials, extra)
        with pytest.raises(ValueError) as e:
            pkg.json_parser.scene_from_json(scene)
        assert word in str(e.value), (word, str(e.value))
        r = _hip_pt("--method", "megakernel", "--dump-scene", str(tmp_path / "bad.bin"), scene)
        assert r.returncode != 0 and word in r.stderr, (word, r.stderr)


def test_the_asset_scene(pkg):
    """assets/scenes/cornell_textured.json: a box whose every corner is a seam, a diffuse and a metal instance, each under a picture"""
    sd = pkg.json_parser.scene_from_json(os.path.join(ROOT, "assets", "scenes", "cornell_textured.json"))
    flat = sd.build_scene()
    assert sd.textures is True and flat.texcoords.shape == (36, 2) and len(flat.positions) == 8 and len(flat.texture_sources) == 2
    assert sorted(flat.material_texture.tolist()) == [-1, -1, -1, -1, -1, 0, 1]
    corner_sets = {}
    for v, st in zip(flat.indices.tolist(), map(tuple, flat.texcoords.tolist())):
        corner_sets.setdefault(v, set()).add(st)
    assert all(len(s) >= 2 for s in corner_sets.values())  # one vertex, several coordinates: seams without split vertices
