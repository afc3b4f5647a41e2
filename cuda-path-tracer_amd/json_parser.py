"""Python mirror of the reference's scene front-end: scene_from_json (assets/json_parser.cpp:174-224) and
load_obj (assets/model_loader.cpp:11-44, there through assimp; here a plain OBJ reader: `v` and `f` records,
fan triangulation, bounding box from the vertices).  Same grammar as host/scene_description.cpp."""
import json
import math
import os

import numpy as np

from . import glmlite as glm
from . import hdr
from .scene_description import (Camera, DielectricMaterial, DiffuseMateral, EmissiveMaterial, Mesh, MetalMaterial, SceneDescription,
                                Sphere, TextureSource)


def load_obj(filename):
    """model_loader.cpp:11-44 keeps assimp's mMeshes[0] only.  assimp's OBJ importer opens a new mesh at every `o` / `g` that
    names another object or group and at every `usemtl` that names another material, and drops meshes without faces: the
    first chunk that holds a face is kept, with the vertices its faces use (file order); fan triangulation.  The same rule
    as host/scene_description.cpp (tests/test_cli_frontend.py compares the two).
    Texture coordinates (an extension): `vt` records and the second field of an `f a/b/c` token are collected into
    Mesh.texcoords, one (s, t) pair per triangle corner, fan-triangulated with the faces; negative indices count from the last `vt`
    read, a corner without a `vt` (or with one the file does not hold) gets (0, 0); a file without `vt` records gives None."""
    positions, faces = [], []
    vts, corners = [], []
    cur = {"o": "", "g": "", "usemtl": ""}
    closed = False
    with open(filename) as f:
        for line in f:
            if line.startswith("v "):
                positions.append([float(x) for x in line.split()[1:4]])
                continue
            if line.startswith("vt "):
                vals = [float(x) for x in line.split()[1:3]]
                vts.append((vals + [0.0, 0.0])[:2])
                continue
            key = line.split(None, 1)[0] if line.strip() else ""
            if key in cur and line[len(key):len(key) + 1] in (" ", "\t"):
                name = line[len(key):].strip()
                if name != cur[key] and faces:
                    closed = True
                cur[key] = name
            elif line.startswith("f ") and not closed:
                face, st = [], []
                for tok in line.split()[1:]:
                    fields = tok.split("/")
                    idx = int(fields[0])
                    face.append(len(positions) + idx if idx < 0 else idx - 1)
                    t = int(fields[1]) if len(fields) > 1 and fields[1] else 0
                    t = len(vts) + t if t < 0 else t - 1
                    st.append(vts[t] if 0 <= t < len(vts) else [0.0, 0.0])
                for k in range(1, len(face) - 1):
                    faces += [face[0], face[k], face[k + 1]]
                    corners += [st[0], st[k], st[k + 1]]
    if not positions or not faces:
        raise ValueError(f"Unable to load {filename}")
    positions = np.array(positions, dtype=np.float32)
    faces = np.array(faces, dtype=np.int64)
    if faces.min() < 0 or faces.max() >= len(positions):
        raise ValueError(f"Unable to load {filename}: face index out of range")
    used = np.zeros(len(positions), dtype=bool)
    used[faces] = True
    remap = np.cumsum(used) - 1
    return Mesh(positions[used], remap[faces].astype(np.uint32), texcoords=np.array(corners, dtype=np.float32) if vts else None)


def _command(j):
    """One transform command, json_parser.cpp:40-75."""
    if "translate" in j:
        return glm.translate(j["translate"])
    if "scale" in j:
        s = j["scale"]
        return glm.scale(s if isinstance(s, (int, float)) else s)
    if "rotate" in j:
        return glm.rotate(np.float32(np.float32(j["rotate"]) * np.float32(0.01745329251994329576923690768489)), j["axis"])
    if "from" in j and "at" in j and "up" in j:
        return glm.look_at(j["from"], j["at"], j["up"])
    raise ValueError(f"Json parser: Unrecognized transform command: {j}")


def _transform(j):
    """json_parser.cpp:78-95: an object is one command, an array applies its commands left to right."""
    if isinstance(j, dict):
        return _command(j)
    if isinstance(j, list):
        return glm.compose([_command(e) for e in j])
    raise ValueError("Json Parser: Transform must be either an object or an array!")


def _emission(m):
    """An emissive material's "emission": an array of three finite numbers >= 0 (scene_description.cpp, the same rule)."""
    e = m.get("emission")
    if (not isinstance(e, list) or len(e) != 3 or
            not all(isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) and v >= 0 for v in e)):
        raise ValueError(f"Json Parser: emissive material {m.get('name')!r} needs \"emission\": three finite numbers >= 0")
    return tuple(e)


def _texture(m, file_dir, key="texture"):
    """A diffuse or metal material's optional "texture" (an extension; scene_description.cpp, the same rule):
    {"file": a PNG, relative to the scene file; "encoding": "srgb" | "linear"; "filter": "bilinear" | "nearest"; "wrap": "repeat" |
    "clamp"}, defaults srgb, bilinear, repeat -- or its "normal_map" (section 5q): the same without "encoding", which a normal map does
    not have.  -> a TextureSource, or None without the key"""
    if key not in m:
        return None
    j = m[key]
    choices = {"encoding": ("srgb", "linear"), "filter": ("bilinear", "nearest"), "wrap": ("repeat", "clamp")}
    if key == "normal_map":
        del choices["encoding"]
    if not isinstance(j, dict) or not isinstance(j.get("file"), str) or set(j) - {"file", *choices}:
        raise ValueError(f"Json Parser: material {m.get('name')!r}: \"{key}\" must be an object with \"file\" (a string) and optionally "
                         + ", ".join(f'"{c}"' for c in choices))
    for c, allowed in choices.items():
        if j.get(c, allowed[0]) not in allowed:
            raise ValueError(f"Json Parser: material {m.get('name')!r}: {key} \"{c}\" must be \"{allowed[0]}\" or \"{allowed[1]}\"")
    return TextureSource(os.path.normpath(os.path.join(file_dir, j["file"])), j.get("encoding", "srgb" if key == "texture" else "linear"),
                         j.get("filter", "bilinear"), j.get("wrap", "repeat"))


def _lens_value(cam, key, positive):
    """An optional camera key of the thin lens (an extension; scene_description.cpp, the same rule): a finite number, >= 0
    ("lens_radius") or > 0 ("focus_distance").  Absent: 0."""
    if key not in cam:
        return 0.0
    v = cam[key]
    if not isinstance(v, (int, float)) or isinstance(v, bool) or not math.isfinite(v) or v < 0 or (positive and v == 0):
        raise ValueError(f"Json Parser: camera \"{key}\" must be a finite number {'> 0' if positive else '>= 0'}, got {v!r}")
    return float(np.float32(v))


def _environment(j, file_dir):
    """The optional scene key "environment" (an extension; scene_description.cpp, the same rule):
    {"file": a Radiance .hdr, equirectangular, relative to the scene file; "scale": a finite number >= 0, default 1; "size": the
    octahedral map's size, an integer in [2,4096], default the image's height, at most 4096; "light": a boolean, default false --
    sample the environment as a light under the megakernel method}.
    -> (the map [n, n, 3] float32, the entry as read: file (absolute), scale, size, and light if the file gives it)"""
    if not isinstance(j, dict) or not isinstance(j.get("file"), str) or set(j) - {"file", "scale", "size", "light"}:
        raise ValueError("Json Parser: \"environment\" must be an object with \"file\" (a string) and optionally \"scale\", \"size\", \"light\"")
    if not isinstance(j.get("light", False), bool):
        raise ValueError(f"Json Parser: environment \"light\" must be true or false, got {j['light']!r}")
    scale = j.get("scale", 1.0)
    if not isinstance(scale, (int, float)) or isinstance(scale, bool) or not math.isfinite(scale) or scale < 0:
        raise ValueError(f"Json Parser: environment \"scale\" must be a finite number >= 0, got {scale!r}")
    size = j.get("size")
    if size is not None and (not isinstance(size, int) or isinstance(size, bool) or not 2 <= size <= 4096):
        raise ValueError(f"Json Parser: environment \"size\" must be an integer in [2,4096], got {size!r}")
    path = os.path.normpath(os.path.join(file_dir, j["file"]))
    image = hdr.read_hdr(path)
    n = size if size is not None else min(image.shape[0], 4096)
    if n < 2:
        raise ValueError(f"Json Parser: environment image {path} is too small for a map (height {image.shape[0]}); give \"size\"")
    return hdr.environment_from_equirect(image, n, scale), {"file": path, "scale": float(scale), "size": int(n), **({"light": j["light"]} if "light" in j else {})}


def scene_from_json(filename):
    with open(filename) as f:
        root = json.load(f)
    file_dir = os.path.dirname(os.path.abspath(filename))
    scene = SceneDescription()
    scene.filename = filename
    for m in root["materials"]:
        t = m["type"]
        if t == "lambertian":
            scene.add_material(m["name"], DiffuseMateral(tuple(m["albedo"]), _texture(m, file_dir), _texture(m, file_dir, "normal_map")))
        elif t == "dielectric":
            scene.add_material(m["name"], DielectricMaterial(m["refraction_index"]))
        elif t == "metal":
            scene.add_material(m["name"], MetalMaterial(tuple(m["albedo"]), m["fuzz"], _texture(m, file_dir), _texture(m, file_dir, "normal_map")))
        elif t == "emissive":  # an extension: the reference's grammar has no emitters
            scene.add_material(m["name"], EmissiveMaterial(_emission(m)))
        else:
            raise ValueError(f"Json Parser: Unsupported material type {t}")
        for key in ("texture", "normal_map"):
            if key in m and t not in ("lambertian", "metal"):
                raise ValueError(f"Json Parser: material {m['name']!r}: only a lambertian or a metal material may carry a \"{key}\"")
    for s in root["surfaces"]:
        transform = _transform(s["transform"])
        if s["type"] == "sphere":
            scene.add_object(Sphere((0.0, 0.0, 0.0), s["radius"]), transform, s["material"])
        elif s["type"] == "mesh":
            path = os.path.normpath(os.path.join(file_dir, s["filename"]))
            mesh = scene.get_mesh(path) or scene.add_mesh(path, load_obj(path))
            scene.add_object(mesh, transform, s["material"])
        else:
            raise ValueError(f"Json Parser: Not supported surface type {s['type']}")
    cam = root["camera"]
    camera = Camera()
    if "transform" in cam:
        m = _transform(cam["transform"])
        camera.position = tuple(float(v) for v in m[3, 0:3])
        camera.rotation = tuple(float(v) for v in glm.quat_from_matrix(m))
    camera.vfov = float(np.float32(np.float32(cam["vfov"]) * np.float32(0.01745329251994329576923690768489)))
    camera.lens_radius = _lens_value(cam, "lens_radius", False)
    camera.focus_distance = _lens_value(cam, "focus_distance", True)
    scene.camera = camera
    if "resolution" in cam:
        scene.resolution = (int(cam["resolution"][0]), int(cam["resolution"][1]))
    scene.spp = int(root["sampler"]["samples"]) if "sampler" in root else 1
    if "smooth_normals" in root:  # (an extension; scene_description.cpp, the same rule)
        if not isinstance(root["smooth_normals"], bool):
            raise ValueError('Json Parser: "smooth_normals" must be true or false')
        scene.smooth_normals = root["smooth_normals"]
    if "textures" in root:  # (an extension; scene_description.cpp, the same rule)
        if not isinstance(root["textures"], bool):
            raise ValueError('Json Parser: "textures" must be true or false')
        scene.textures = root["textures"]
    if "normal_maps" in root:  # (an extension; scene_description.cpp, the same rule)
        if not isinstance(root["normal_maps"], bool):
            raise ValueError('Json Parser: "normal_maps" must be true or false')
        scene.normal_maps = root["normal_maps"]
    if "environment" in root:
        scene.environment, scene.environment_source = _environment(root["environment"], file_dir)
    return scene
