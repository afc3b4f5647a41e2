"""Python mirror of the reference's `class PathTracer` (src/lib/path_tracer.hpp:60-99) over the C ABI.

Same public surface: fields ``max_iterations``, ``current_gpu_method``, ``atrous_denoiser``; methods
``restart``, ``iteration``, ``resize_image``, ``create_buffers``, ``path_trace``, ``denoise``,
``send_to_preview``.  Everything runs in libptcore.so on the GPU; this file only marshals arguments."""
import ctypes as C
from dataclasses import dataclass
from enum import IntEnum

import numpy as np

from . import _capi
from .scene_description import Camera, FlatScene, SceneDescription


class GPUMethod(IntEnum):  # path_tracer.hpp:57
    megakernel = 0
    streaming = 1


class DisplayBufferType(IntEnum):  # path_tracer.hpp:19
    final = 0
    color = 1
    normal = 2
    depth = 3


@dataclass
class EdgeAvoidingATrousDenoiser:  # denoising/edge_avoiding_a_trous_denoiser.hpp:7-12
    filter_size: int = 10
    color_weight: float = 0.45
    normal_weight: float = 0.30
    position_weight: float = 0.25


LIGHT_DTYPE = np.dtype([("p0", "<f4", (3,)), ("e1", "<f4", (3,)), ("e2", "<f4", (3,)), ("n", "<f4", (3,)), ("cdf", "<f4"),
                        ("inv_pdf", "<f4"), ("object", "<u4"), ("kind_material", "<u4")])
assert LIGHT_DTYPE.itemsize == 64


def _light_info_dict(info):
    return {"lights": int(info.lights), "sphere_lights": int(info.sphere_lights), "triangle_lights": int(info.triangle_lights),
            "emissive_objects": int(info.emissive_objects), "total_area": float(info.total_area),
            "total_weight": float(info.total_weight)}


def light_table(scene, capacity=None):
    """The lamp table of a scene (ptc_light_table; host-side, no GPU needed): one 64-byte record per primitive of every
    emissive object.  scene: a SceneDescription or a FlatScene.  -> (records [LIGHT_DTYPE], info dict).  capacity: records
    the output may hold (default: every primitive of the scene)."""
    flat = scene.build_scene() if isinstance(scene, SceneDescription) else scene
    desc = flat.to_c()
    if capacity is None:
        capacity = 0
        for obj, mat in zip(flat.objects, flat.object_material_indices):
            if mat < len(flat.materials) and flat.materials["type"][mat] == 3:
                if obj["type"] == 0:
                    capacity += 1
                elif flat.mesh_ranges is None:
                    capacity += len(flat.indices) // 3
                elif obj["index"] < len(flat.mesh_ranges):
                    capacity += int(np.asarray(flat.mesh_ranges).reshape(-1, 6)[obj["index"], 3]) // 3
    out = np.zeros(max(int(capacity), 1), dtype=LIGHT_DTYPE)
    info = _capi.ptc_light_info()
    rc = _capi.check(_capi.lib().ptc_light_table(C.byref(desc), out.ctypes.data_as(C.POINTER(_capi.ptc_light)), int(capacity),
                                                 C.byref(info)))
    return out[:rc].copy(), _light_info_dict(info)


def light_material_pdf(scene, capacity=None):
    """Per material of a scene the inv_pdf its lamp records carry (ptc_light_material_pdf; host-side, no GPU needed), 0 for a
    material that is no lamp: what "mis" weighs a lamp hit with.  -> float32 [materials]"""
    flat = scene.build_scene() if isinstance(scene, SceneDescription) else scene
    desc = flat.to_c()
    capacity = len(flat.materials) if capacity is None else int(capacity)
    out = np.zeros(max(capacity, 1), dtype=np.float32)
    rc = _capi.check(_capi.lib().ptc_light_material_pdf(C.byref(desc), out.ctypes.data, capacity))
    return out[:rc].copy()


def check_light_sample(scene, points, normals, v, u):
    """One light sample per point from explicit draws (ptc_check_light_sample; host-side, no GPU needed): the header the device runs,
    against the lamp table of `scene` (a SceneDescription or a FlatScene).  points, normals [n, 3]; v uint32 [n], the raw first draw
    (1 .. 2^31 - 2: it picks the lamp); u [n, 2]: u1, u2.  -> dict(lamp uint32 [n], rays [n, 8], contribution [n, 3], sampled bool [n])"""
    flat = scene.build_scene() if isinstance(scene, SceneDescription) else scene
    desc = flat.to_c()
    p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    v = np.ascontiguousarray(v, dtype=np.uint32).reshape(-1)
    u = np.ascontiguousarray(u, dtype=np.float32).reshape(-1, 2)
    n = len(p)
    if not (len(nrm) == n and len(v) == n and len(u) == n):
        raise ValueError("points, normals, v and u must have one row per point")
    lamp = np.zeros(n, dtype=np.uint32)
    rays = np.zeros((n, 8), dtype=np.float32)
    contribution = np.zeros((n, 3), dtype=np.float32)
    sampled = np.zeros(n, dtype=np.uint8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    _capi.check(_capi.lib().ptc_check_light_sample(C.byref(desc), ptr(p), ptr(nrm), ptr(v), ptr(u), n, ptr(lamp), ptr(rays), ptr(contribution),
                                                   ptr(sampled)))
    return {"lamp": lamp, "rays": rays, "contribution": contribution, "sampled": sampled.astype(bool)}


_ENCODINGS = {"linear": 0, "srgb": 1}
_FILTERS = {"nearest": 0, "bilinear": 1}
_WRAPS = {"repeat": 0, "clamp": 1}


class Texture:
    """One image texture (ptc_texture_desc): rgba8 [height, width, 4] uint8 with row 0 at t = 0 -- the BOTTOM of the
    picture in OBJ's convention (a file reader flips rows) --, encoding "srgb" | "linear", filter "bilinear" | "nearest", wrap "repeat" |
    "clamp" (or their numbers, which are passed on unchecked: the library refuses)."""

    def __init__(self, rgba8, encoding="srgb", filter="bilinear", wrap="repeat"):
        a = np.array(rgba8, dtype=np.uint8, order="C")
        if a.ndim != 3 or a.shape[2] != 4:
            raise ValueError("a texture is [height, width, 4] uint8, got shape %r" % (a.shape,))
        a.setflags(write=False)
        self.rgba8 = a
        self.encoding = _ENCODINGS.get(encoding, encoding)
        self.filter = _FILTERS.get(filter, filter)
        self.wrap = _WRAPS.get(wrap, wrap)

    @property
    def height(self):
        return self.rgba8.shape[0]

    @property
    def width(self):
        return self.rgba8.shape[1]

    def _desc(self):
        return _capi.ptc_texture_desc(self.rgba8.ctypes.data, self.width, self.height, int(self.encoding), int(self.filter), int(self.wrap))


def texture_decode_table(encoding):
    """The 256-entry decode table of an encoding ("linear" | "srgb" or 0 | 1; ptc_texture_decode_table; host-side, no GPU needed)"""
    out = np.zeros(256, dtype=np.float32)
    _capi.check(_capi.lib().ptc_texture_decode_table(int(_ENCODINGS.get(encoding, encoding)), out.ctypes.data_as(C.c_void_p)))
    return out


def check_texture_lookup(texture, st):
    """The texture lookup of DESIGN section 5o on the host (ptc_check_texture_lookup; no GPU needed): st [n, 2] ->
    (rgb float32 [n, 3], rejected bool [n])"""
    st = np.ascontiguousarray(st, dtype=np.float32).reshape(-1, 2)
    rgb, rej = np.zeros((len(st), 3), dtype=np.float32), np.zeros(len(st), dtype=np.uint8)
    d = texture._desc()
    _capi.check(_capi.lib().ptc_check_texture_lookup(C.byref(d), st.ctypes.data_as(C.c_void_p), len(st), rgb.ctypes.data_as(C.c_void_p),
                                                     rej.ctypes.data_as(C.c_void_p)))
    return rgb, rej.astype(bool)


def check_demodulate(colour, albedo):
    """The denoiser's albedo rule of DESIGN section 5r on the host (ptc_check_demodulate; no GPU needed), elementwise on two float32
    arrays of one shape -> (irradiance, effective albedo), float32 of that shape"""
    c = np.ascontiguousarray(colour, dtype=np.float32)
    a = np.ascontiguousarray(albedo, dtype=np.float32)
    if c.shape != a.shape:
        raise ValueError("check_demodulate: the arrays differ in shape")
    irr, eff = np.zeros_like(c), np.zeros_like(c)
    _capi.check(_capi.lib().ptc_check_demodulate(c.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), c.size,
                                                 irr.ctypes.data_as(C.c_void_p), eff.ctypes.data_as(C.c_void_p)))
    return irr, eff


def check_denoise_variance(colour, normal, depth, camera, filter_size=10, normal_weight=0.30, position_weight=0.25, sigma=16.0):
    """The whole "denoise_variance" mode of DESIGN section 5s on the host (ptc_check_denoise_variance; no GPU needed) from caller
    planes: colour and normal float32 [h, w, 3], depth float32 [h, w], camera a Camera -> (variance float32 [h, w]: the estimate,
    result float32 [h, w, 3]: the last guided pass's colour, or None when filter_size < 1)"""
    c = np.ascontiguousarray(colour, dtype=np.float32)
    n = np.ascontiguousarray(normal, dtype=np.float32)
    d = np.ascontiguousarray(depth, dtype=np.float32)
    if c.ndim != 3 or c.shape[2] != 3 or n.shape != c.shape or d.shape != c.shape[:2]:
        raise ValueError("check_denoise_variance: colour and normal are [h, w, 3], depth is [h, w]")
    h, w = d.shape
    cam = camera.to_c()
    prm = _capi.ptc_denoiser_params(int(filter_size), 0.0, float(normal_weight), float(position_weight))
    var, out = np.zeros((h, w), dtype=np.float32), np.zeros((h, w, 3), dtype=np.float32)
    _capi.check(_capi.lib().ptc_check_denoise_variance(c.ctypes.data_as(C.c_void_p), n.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p),
                                                       C.cast(C.byref(cam), C.c_void_p), w, h, C.cast(C.byref(prm), C.c_void_p), float(sigma),
                                                       var.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return var, (out if int(filter_size) >= 1 else None)


def normal_map_decode_table():
    """The 256-entry decode table of a normal map (ptc_normal_map_decode_table; host-side, no GPU needed)"""
    out = np.zeros(256, dtype=np.float32)
    _capi.check(_capi.lib().ptc_normal_map_decode_table(out.ctypes.data_as(C.c_void_p)))
    return out


def check_normal_map(texture, p0, p1, p2, st0, st1, st2, u, v, m16, b, g, d):
    """The normal map's rule of DESIGN section 5q on the host (ptc_check_normal_map; no GPU needed).  Per case the corners' object-space
    positions [n, 3], their coordinate pairs [n, 2], the hit's u, v [n], the base normal, the geometric normal and the ray direction
    [n, 3]; m16 the object matrix, column-major -> (normal float32 [n, 3], outcome uint8 [n]: 2 bent, 3 flat, 4 kept)"""
    a3 = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 3) for a in (p0, p1, p2, b, g, d)]
    a2 = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 2) for a in (st0, st1, st2)]
    a1 = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in (u, v)]
    n = len(a1[0])
    if any(len(a) != n for a in a3 + a2 + a1):
        raise ValueError("check_normal_map: the arrays differ in length")
    m = np.ascontiguousarray(m16, dtype=np.float32).reshape(16)
    out, how = np.zeros((n, 3), dtype=np.float32), np.zeros(n, dtype=np.uint8)
    desc = texture._desc()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    _capi.check(_capi.lib().ptc_check_normal_map(C.byref(desc), ptr(a3[0]), ptr(a3[1]), ptr(a3[2]), ptr(a2[0]), ptr(a2[1]), ptr(a2[2]), ptr(a1[0]),
                                                 ptr(a1[1]), ptr(m), ptr(a3[3]), ptr(a3[4]), ptr(a3[5]), n, ptr(out), ptr(how)))
    return out, how


def check_megakernel_instance2(direct=False, env=False, env_lit=False, smooth=False, textured=False, weigh=False, lens=False, plays=None,
                               emitters=False, bent=False, roulette=0, max_bounces=50):
    """check_megakernel_instance with the tenth fact, bent (ptc_check_megakernel_instance2)"""
    name, arg = C.create_string_buffer(64), C.c_int(0)
    _capi.check(_capi.lib().ptc_check_megakernel_instance2(int(direct), int(env), int(env_lit), int(smooth), int(textured), int(weigh), int(lens),
                                                           -1 if plays is None else int(plays), int(emitters), int(bent), int(roulette),
                                                           int(max_bounces), name, len(name), C.byref(arg)))
    return name.value.decode(), arg.value


def check_megakernel_instance(direct=False, env=False, env_lit=False, smooth=False, textured=False, weigh=False, lens=False, plays=None,
                              emitters=False, roulette=0, max_bounces=50):
    """The megakernel's instance rule on the host (ptc_check_megakernel_instance; no GPU): the nine facts of a frame -> (the kernel's
    name as a profile prints it, its roulette argument).  plays None: the library's own reading of roulette under max_bounces."""
    name, arg = C.create_string_buffer(64), C.c_int(0)
    _capi.check(_capi.lib().ptc_check_megakernel_instance(int(direct), int(env), int(env_lit), int(smooth), int(textured), int(weigh), int(lens),
                                                          -1 if plays is None else int(plays), int(emitters), int(roulette), int(max_bounces),
                                                          name, len(name), C.byref(arg)))
    return name.value.decode(), arg.value


def compute_vertex_normals(positions, indices=None, mesh_ranges=None):
    """Area-weighted vertex normals (ptc_compute_vertex_normals; host-side, no GPU needed).  positions [v, 3] and
    indices [t * 3] of one mesh, or -- with mesh_ranges, a mesh table's rows (first_vertex, vertex_count, first_index, index_count, ...)
    -- of a whole scene, mesh by mesh.  A FlatScene or SceneDescription in place of positions brings all three.  -> float32 [v, 3], a
    zero vector for a vertex no triangle uses or whose sum has no direction."""
    if isinstance(positions, SceneDescription):
        positions = positions.build_scene()
    if isinstance(positions, FlatScene):
        positions, indices, mesh_ranges = positions.positions, positions.indices, getattr(positions, "mesh_ranges", None)
    pos = np.ascontiguousarray(positions, dtype=np.float32).reshape(-1, 3)
    idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
    out = np.zeros_like(pos)
    rows = [(0, len(pos), 0, len(idx))] if mesh_ranges is None else [tuple(int(x) for x in r[:4]) for r in np.asarray(mesh_ranges).reshape(-1, 6)]
    for fv, nv, fi, ni in rows:
        p, i, o = np.ascontiguousarray(pos[fv:fv + nv]), np.ascontiguousarray(idx[fi:fi + ni]), np.zeros((nv, 3), dtype=np.float32)
        _capi.check(_capi.lib().ptc_compute_vertex_normals(p.ctypes.data_as(C.c_void_p), nv, i.ctypes.data_as(C.c_void_p), ni,
                                                          o.ctypes.data_as(C.c_void_p)))
        out[fv:fv + nv] = o
    return out


class ToneCurve(IntEnum):  # ptc_curve
    clamp = 0
    reinhard = 1
    aces = 2


@dataclass(frozen=True)
class Display:
    """The display transform (ptc_display_params).  The default is the reference display: clamp and gamma only."""
    curve: int = ToneCurve.clamp
    metering: int = 0            # 0 manual, 1 histogram
    exposure: float = 1.0        # linear factor, > 0
    key: float = 0.18            # what the metered level is mapped to
    white: float = 4.0           # Reinhard's white point
    low_permille: int = 50       # the trimmed mean keeps the ranks between the two
    high_permille: int = 950

    def to_c(self):
        return _capi.ptc_display_params(int(self.curve), int(self.metering), float(self.exposure), float(self.key), float(self.white),
                                        int(self.low_permille), int(self.high_permille))


def _exposure_info(info):
    return {"pixels": int(info.pixels), "counted": int(info.counted), "below": int(info.below), "rejected": int(info.rejected),
            "level_bin": int(info.level_bin), "level": np.float32(info.level), "scale": np.float32(info.scale),
            "histogram": np.ctypeslib.as_array(info.histogram).astype(np.uint32)}


class _DirectLight:
    """What PathTracer.direct_light is.  The name was the direct-light QUERY's (ptc_direct_light) before it became the render
    loop's switch as well (the field the C++ PathTracer has), so it is both: its truth value is the switch -- assign True or False
    to PathTracer.direct_light --, and called it is the query, as before."""

    def __init__(self, tracer):
        self._tracer = tracer

    def __bool__(self):
        return self._tracer._direct_light

    def __call__(self, points, normals, sample_index=0, want_rays=False):
        return self._tracer._direct_light_query(points, normals, sample_index, want_rays)


class _EnvironmentLight:
    """What PathTracer.environment_light is, in _DirectLight's manner: its truth value is the render loop's switch (ptc_set_param
    "environment_light") -- assign True or False --, and called with points and normals it is the query (ptc_environment_light)."""

    def __init__(self, tracer):
        self._tracer = tracer

    def __bool__(self):
        return self._tracer._environment_light

    def __call__(self, points, normals, sample_index=0, want_rays=False):
        return self._tracer._environment_light_query(points, normals, sample_index, want_rays)


class PathTracer:
    def __init__(self, device=0, max_bounces=50):
        self._lib = _capi.lib()
        self.max_iterations = 1
        self.current_gpu_method = GPUMethod.streaming
        self._direct_light = False  # PathTracer.direct_light = True: a light sample at every diffuse hit (megakernel method only)
        self._environment_light = False  # PathTracer.environment_light = True: an environment sample at every diffuse hit (megakernel only)
        self._mis = False  # PathTracer.mis = True: the balance heuristic between light samples and the path (megakernel only)
        self._smooth_normals = False  # PathTracer.smooth_normals = True: interpolated vertex normals at triangle hits (megakernel only)
        self._vertex_normals = None  # PathTracer.vertex_normals = [v, 3] float32, parallel to the uploaded scene's positions (None: none)
        self._roulette = 0  # PathTracer.roulette = k: Russian roulette at every bounce >= k but the last (0 = off)
        self._lens = (0.0, 1.0)  # PathTracer.lens = (radius, focus_distance): the thin lens (radius 0 = the pinhole)
        self._environment = None  # PathTracer.environment = [n, n, 3] float32: an octahedral HDR sky (None = the reference's gradient)
        self.atrous_denoiser = EdgeAvoidingATrousDenoiser()
        self.max_bounces = max_bounces  # reference: compile-time 50 (path_tracer.cu:27)
        cfg = _capi.ptc_config(device=device, max_bounces=max_bounces, method=int(self.current_gpu_method), reserved=0)
        handle = C.c_void_p()
        _capi.check(self._lib.ptc_create(C.byref(cfg), C.byref(handle)))
        self._ctx = handle
        self._resolution = None
        self._rows = None
        self._direct_light_pushed = False
        self._environment_light_pushed = False
        self._mis_pushed = False
        self._smooth_normals_pushed = False
        self._textures = False  # PathTracer.textures = True: bound materials take their colour from their texture (megakernel only)
        self._textures_pushed = False
        self._texture_table = None  # PathTracer.texture_table = (textures, material_texture) (None: none)
        self._normal_maps = False  # PathTracer.normal_maps = True: bound materials take their normal from their map (megakernel only)
        self._normal_maps_pushed = False
        self._normal_map_table = None  # PathTracer.normal_map_table = material_normal_map (None: none)
        self._texcoords = None  # PathTracer.texcoords = [index_count, 2] float32, parallel to the uploaded scene's indices (None: none)
        self._roulette_pushed = 0
        self._lens_pushed = (0.0, 1.0)
        self._environment_pushed = None

    # -- lifetime -------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.ptc_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        return _capi.check(rc, self._ctx)

    @property
    def direct_light(self):
        """The switch of direct lighting in the megakernel (ptc_set_param "direct_light"; assign True / False, read with bool())
        and, called with points and normals, the direct-light query (ptc_direct_light)."""
        return _DirectLight(self)

    @direct_light.setter
    def direct_light(self, on):
        self._direct_light = bool(on)

    @property
    def environment_light(self):
        """The switch of environment light sampling in the megakernel (ptc_set_param "environment_light"; assign
        True / False, read with bool()) and, called with points and normals, the environment-light query (ptc_environment_light)."""
        return _EnvironmentLight(self)

    @environment_light.setter
    def environment_light(self, on):
        self._environment_light = bool(on)

    @property
    def mis(self):
        """Multiple importance sampling in the megakernel (ptc_set_param "mis"): True = every light sample of
        direct_light / environment_light at a diffuse hit is combined with the path's own continuation ray by the balance heuristic.
        The same expectation, another spread; changes nothing in a frame that samples neither light."""
        return self._mis

    @mis.setter
    def mis(self, on):
        self._mis = bool(on)

    @property
    def smooth_normals(self):
        """Smooth shading in the megakernel (ptc_set_param "smooth_normals"): True = a triangle hit is shaded with
        the normal interpolated from vertex_normals.  Changes nothing while no vertex normals are set."""
        return self._smooth_normals

    @smooth_normals.setter
    def smooth_normals(self, on):
        self._smooth_normals = bool(on)

    @property
    def textures(self):
        """Image textures in the megakernel (ptc_set_param "textures"): True = a triangle hit on a diffuse or metal
        material with a texture bound takes its colour from the texel at the interpolated coordinate.  Changes nothing while
        texture_table or texcoords is not set."""
        return self._textures

    @textures.setter
    def textures(self, on):
        self._textures = bool(on)

    @property
    def texture_table(self):
        """The scene's textures and their bindings (ptc_set_textures): a pair (list of Texture, material_texture) with
        material_texture[m] = -1 or the texture of material m of the uploaded scene; None removes them.  Assignment uploads at once --
        after create_buffers, which starts every scene without textures -- and a refusal raises PtcError and leaves what was set."""
        return self._texture_table

    @texture_table.setter
    def texture_table(self, value):
        if value is None:
            self._check(self._lib.ptc_set_textures(self._ctx, None, 0, None, 0))
            self._texture_table = self._normal_map_table = None
            return
        textures, binding = value
        textures = list(textures)
        b = np.array(binding, dtype=np.int32, order="C").reshape(-1)
        descs = (_capi.ptc_texture_desc * max(len(textures), 1))(*[t._desc() for t in textures])
        self._check(self._lib.ptc_set_textures(self._ctx, descs if textures else None, len(textures), b.ctypes.data_as(C.c_void_p), len(b)))
        b.setflags(write=False)
        self._texture_table = (tuple(textures), b)
        self._normal_map_table = None  # (its indices named the old pool: the library dropped it)

    @property
    def normal_maps(self):
        """Normal maps in the megakernel (ptc_set_param "normal_maps"): True = a triangle hit on a diffuse or metal
        material with a normal map bound shades with the map's normal.  Independent of `textures`.  Changes nothing while
        texture_table, texcoords or normal_map_table is not set."""
        return self._normal_maps

    @normal_maps.setter
    def normal_maps(self, on):
        self._normal_maps = bool(on)

    @property
    def normal_map_table(self):
        """The scene's normal-map binding (ptc_set_normal_maps): material_normal_map[m] = -1 or the texture of texture_table that is
        material m's normal map; None removes it.  Assignment uploads at once, after texture_table -- every assignment to texture_table
        drops it -- and a refusal raises PtcError and leaves what was set."""
        return self._normal_map_table

    @normal_map_table.setter
    def normal_map_table(self, value):
        if value is None:
            self._check(self._lib.ptc_set_normal_maps(self._ctx, None, 0))
            self._normal_map_table = None
            return
        b = np.array(value, dtype=np.int32, order="C").reshape(-1)
        self._check(self._lib.ptc_set_normal_maps(self._ctx, b.ctypes.data_as(C.c_void_p), len(b)))
        b.setflags(write=False)
        self._normal_map_table = b

    def load_scene_textures(self, flat):
        """What a scene file says about textures, after create_buffers: reads the pictures of flat.texture_sources (png.read_png, which
        flips rows) and sets texture_table, normal_map_table (flat.material_normal_map) and texcoords from them and from flat.texcoords.
        A scene without any sets nothing."""
        from . import png
        if flat.texture_sources:
            self.texture_table = ([Texture(png.read_png(s.file), s.encoding, s.filter, s.wrap) for s in flat.texture_sources], flat.material_texture)
            if flat.material_normal_map is not None:
                self.normal_map_table = flat.material_normal_map
        if flat.texcoords is not None:
            self.texcoords = flat.texcoords

    @property
    def texcoords(self):
        """The scene's texture coordinates (ptc_set_texcoords): [index_count, 2] float32 (s, t), one pair per triangle corner, parallel
        to the uploaded scene's indices; None removes them.  Assignment uploads at once, as vertex_normals does."""
        return self._texcoords

    @texcoords.setter
    def texcoords(self, value):
        if value is None:
            self._check(self._lib.ptc_set_texcoords(self._ctx, None, 0))
            self._texcoords = None
            return
        st = np.array(value, dtype=np.float32, order="C").reshape(-1, 2)
        self._check(self._lib.ptc_set_texcoords(self._ctx, st.ctypes.data_as(C.c_void_p), len(st)))
        st.setflags(write=False)
        self._texcoords = st

    @property
    def vertex_normals(self):
        """The scene's vertex normals (ptc_set_vertex_normals): [v, 3] float32 parallel to the uploaded scene's positions, object space,
        any length; None removes them.  Assignment uploads at once -- after create_buffers, which starts every scene without normals --
        and a refusal (no scene, another vertex count) raises PtcError and leaves what was set."""
        return self._vertex_normals

    @vertex_normals.setter
    def vertex_normals(self, value):
        if value is None:
            self._check(self._lib.ptc_set_vertex_normals(self._ctx, None, 0))
            self._vertex_normals = None
            return
        n = np.array(value, dtype=np.float32, order="C").reshape(-1, 3)
        self._check(self._lib.ptc_set_vertex_normals(self._ctx, n.ctypes.data_as(C.c_void_p), len(n)))
        n.setflags(write=False)
        self._vertex_normals = n

    @property
    def roulette(self):
        """Russian roulette (ptc_set_param "roulette"): 0 = off (the default); k >= 1 = a path may end by chance at
        every bounce >= k except the last, unbiased, in both render methods.  An int in [0, 64]."""
        return self._roulette

    @roulette.setter
    def roulette(self, k):
        k = int(k)
        if not 0 <= k <= 64:
            raise ValueError("roulette must be in [0,64]")
        self._roulette = k

    @property
    def lens(self):
        """The thin lens (ptc_set_lens): (lens_radius, focus_distance) in world units.  Radius 0 (the default) is the
        pinhole; under a radius > 0 the plane at camera-space depth focus_distance is sharp and everything else blurs with the radius,
        in both render methods."""
        return self._lens

    @lens.setter
    def lens(self, value):
        radius, focus = (float(np.float32(v)) for v in value)
        if not np.isfinite(radius) or radius < 0.0:
            raise ValueError(f"lens radius must be finite and not negative, got {radius}")
        if not np.isfinite(focus) or (radius > 0.0 and not focus > 0.0):
            raise ValueError(f"focus distance must be finite, and positive under a lens radius > 0, got {focus}")
        self._lens = (radius, focus)

    @property
    def environment(self):
        """Environment lighting (ptc_set_environment): None (the default: the reference's gradient) or an octahedral
        HDR map, [n, n, 3] float32 with 2 <= n <= 4096, texel [j, i] = row j along z, column i along x, +y up, every component finite
        and >= 0.  Every path that leaves the scene then takes the map's value in its direction, in both render methods.  The array
        is copied at assignment; it is uploaded at the next trace, and only when it has been assigned since the last one."""
        return self._environment

    @environment.setter
    def environment(self, value):
        if value is None:
            self._environment = None
            return
        m = np.array(value, dtype=np.float32, order="C")
        if m.ndim != 3 or m.shape[0] != m.shape[1] or m.shape[2] != 3 or not 2 <= m.shape[0] <= 4096:
            raise ValueError(f"environment must be [n, n, 3] with n in [2,4096], got shape {m.shape}")
        if not np.all(np.isfinite(m)) or np.any(m < 0.0):
            raise ValueError("environment components must be finite and not negative")
        m.setflags(write=False)
        self._environment = m

    @property
    def display(self):
        """The display transform (ptc_set_display): a Display.  It applies where radiance is shown -- send_to_preview and
        gather_present of the final and colour views -- as exposure (manual, or metered from a log-luminance histogram of the shown
        buffer), a tone curve and the reference's gamma encoding.  Assignment takes effect at once and survives create_buffers and
        resize_image; a value the library refuses raises PtcError naming the field, and the display that was set stays."""
        d = _capi.ptc_display_params()
        self._check(self._lib.ptc_get_display(self._ctx, C.byref(d)))
        return Display(ToneCurve(d.curve), int(d.metering), float(d.exposure), float(d.key), float(d.white), int(d.low_permille),
                       int(d.high_permille))

    @display.setter
    def display(self, value):
        d = value.to_c()
        self._check(self._lib.ptc_set_display(self._ctx, C.byref(d)))

    def exposure_info(self):
        """Of the last send_to_preview / gather_present that went through the display transform (ptc_get_exposure_info): a dict of
        pixels, counted, below, rejected, level_bin, level, scale and histogram ([256] uint32)."""
        info = _capi.ptc_exposure_info()
        self._check(self._lib.ptc_get_exposure_info(self._ctx, C.byref(info)))
        return _exposure_info(info)

    def tonemap_buffer(self, image, want_mapped=False):
        """The display transform on an array of the caller's (ptc_tonemap_buffer): image [..., 3] or [..., 4] float32 (the fourth
        channel is ignored) -> (rgba [..., 4] uint8, mapped [..., 3] float32 or None, the exposure info as exposure_info gives it)."""
        a = np.ascontiguousarray(image, dtype=np.float32)
        ch = a.shape[-1]
        n = a.size // ch
        rgba = np.empty((n, 4), dtype=np.uint8)
        mapped = np.empty((n, 3), dtype=np.float32) if want_mapped else None
        info = _capi.ptc_exposure_info()
        self._check(self._lib.ptc_tonemap_buffer(self._ctx, a.ctypes.data_as(C.c_void_p), ch, n, 0, rgba.ctypes.data_as(C.c_void_p),
                                                 mapped.ctypes.data_as(C.c_void_p) if want_mapped else None, 0, C.byref(info)))
        shape = a.shape[:-1]
        return rgba.reshape(shape + (4,)), (mapped.reshape(shape + (3,)) if want_mapped else None), _exposure_info(info)

    def tonemap_buffer_dev(self, src_ptr, channels, pix_count, rgba_ptr, mapped_ptr=None):
        """... on device pointers (a torch tensor's data_ptr()): src of `channels` (3 or 4) floats a pixel, rgba 4 bytes a pixel, mapped
        (optional) 3 floats a pixel.  Returns the exposure info."""
        info = _capi.ptc_exposure_info()
        self._check(self._lib.ptc_tonemap_buffer(self._ctx, C.c_void_p(int(src_ptr)), int(channels), int(pix_count), 1,
                                                 C.c_void_p(int(rgba_ptr)), C.c_void_p(int(mapped_ptr)) if mapped_ptr else None, 1,
                                                 C.byref(info)))
        return _exposure_info(info)

    def sample_environment(self, directions):
        """The environment's value in `directions` ([k, 3], not normalised) as the device computes it for a miss -> [k, 3] float32
        (ptc_sample_environment).  Needs an environment."""
        self._push_fields()
        d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
        out = np.empty_like(d)
        self._check(self._lib.ptc_sample_environment(self._ctx, d.ctypes.data_as(C.c_void_p), len(d), out.ctypes.data_as(C.c_void_p)))
        return out

    def _push_fields(self):
        self._check(self._lib.ptc_set_max_iterations(self._ctx, int(self.max_iterations)))
        self._check(self._lib.ptc_set_method(self._ctx, int(self.current_gpu_method)))
        if self._direct_light != self._direct_light_pushed:  # (ptc_set_param flushes queued frames: only on a change)
            self._check(self._lib.ptc_set_param(self._ctx, b"direct_light", 1 if self._direct_light else 0))
            self._direct_light_pushed = self._direct_light
        if self._environment_light != self._environment_light_pushed:
            self._check(self._lib.ptc_set_param(self._ctx, b"environment_light", 1 if self._environment_light else 0))
            self._environment_light_pushed = self._environment_light
        if self._mis != self._mis_pushed:
            self._check(self._lib.ptc_set_param(self._ctx, b"mis", 1 if self._mis else 0))
            self._mis_pushed = self._mis
        if self._smooth_normals != self._smooth_normals_pushed:
            self._check(self._lib.ptc_set_param(self._ctx, b"smooth_normals", 1 if self._smooth_normals else 0))
            self._smooth_normals_pushed = self._smooth_normals
        if self._textures != self._textures_pushed:
            self._check(self._lib.ptc_set_param(self._ctx, b"textures", 1 if self._textures else 0))
            self._textures_pushed = self._textures
        if self._normal_maps != self._normal_maps_pushed:
            self._check(self._lib.ptc_set_param(self._ctx, b"normal_maps", 1 if self._normal_maps else 0))
            self._normal_maps_pushed = self._normal_maps
        if self._roulette != self._roulette_pushed:
            self._check(self._lib.ptc_set_param(self._ctx, b"roulette", self._roulette))
            self._roulette_pushed = self._roulette
        if self._lens != self._lens_pushed:
            self._check(self._lib.ptc_set_lens(self._ctx, self._lens[0], self._lens[1]))
            self._lens_pushed = self._lens
        if self._environment is not self._environment_pushed:  # (a new array at every assignment: identity tells a change)
            env = self._environment
            self._check(self._lib.ptc_set_environment(self._ctx, env.ctypes.data_as(C.c_void_p) if env is not None else None,
                                                      env.shape[0] if env is not None else 0))
            self._environment_pushed = env
        self._check(self._lib.ptc_set_max_bounces(self._ctx, int(self.max_bounces)))
        d = self.atrous_denoiser
        p = _capi.ptc_denoiser_params(int(d.filter_size), float(d.color_weight), float(d.normal_weight),
                                      float(d.position_weight))
        self._check(self._lib.ptc_set_denoiser_params(self._ctx, C.byref(p)))

    # -- reference API --------------------------------------------------------------------------
    def restart(self):
        self._check(self._lib.ptc_restart(self._ctx))

    def iteration(self):
        return self._lib.ptc_iteration(self._ctx)

    def resize_image(self, resolution):
        w, h = resolution
        self._check(self._lib.ptc_resize(self._ctx, int(w), int(h)))
        self._resolution = (int(w), int(h))
        self._rows = (0, int(h))

    def create_buffers(self, resolution, scene):
        """scene: a SceneDescription (flattened with build_scene(), like the reference) or a FlatScene."""
        flat = scene.build_scene() if isinstance(scene, SceneDescription) else scene
        assert isinstance(flat, FlatScene)
        desc = flat.to_c()
        self._check(self._lib.ptc_upload_scene(self._ctx, C.byref(desc)))
        self._vertex_normals = None  # (a new scene starts without normals)
        self._texture_table = self._texcoords = self._normal_map_table = None  # (... and without textures, coordinates and normal maps)
        self.resize_image(resolution)

    def path_trace(self, camera, resolution=None):
        if resolution is not None and tuple(resolution) != self._resolution:
            raise ValueError("resolution differs from the allocated buffers (call resize_image first)")
        self._push_fields()
        cam = camera.to_c() if isinstance(camera, Camera) else camera
        self._check(self._lib.ptc_trace(self._ctx, C.byref(cam)))

    def denoise(self, resolution=None):
        self._push_fields()
        self._check(self._lib.ptc_denoise(self._ctx))

    def denoise_albedo(self):
        """The albedo stage of set_param("denoise_albedo", 1) alone (ptc_denoise_albedo), whatever the parameter
        says -> dict(albedo float32 [h, w, 3]: the first-hit albedo of the pixel-centre ray, ones at glass, an emitter and on a miss;
        irradiance float32 [h, w, 3]: the accumulated colour over the effective albedo; rays float32 [h * w, 8]: the rays the kernel
        walked, hit_surface's layout).  Needs a traced frame and the whole frame in this context."""
        self._push_fields()
        w, h = self._resolution
        alb, irr = np.zeros((h, w, 3), dtype=np.float32), np.zeros((h, w, 3), dtype=np.float32)
        rays = np.zeros((h * w, 8), dtype=np.float32)
        self._check(self._lib.ptc_denoise_albedo(self._ctx, alb.ctypes.data_as(C.c_void_p), irr.ctypes.data_as(C.c_void_p),
                                                 rays.ctypes.data_as(C.c_void_p)))
        return {"albedo": alb, "irradiance": irr, "rays": rays}

    @property
    def denoise_variance_sigma(self):
        """sigma of set_param("denoise_variance", 1) (ptc_set_denoise_variance): the prefiltered variance is
        multiplied by it under the colour distance.  Finite and > 0; default 16."""
        s = C.c_float(0.0)
        self._check(self._lib.ptc_get_denoise_variance(self._ctx, C.byref(s)))
        return float(s.value)

    @denoise_variance_sigma.setter
    def denoise_variance_sigma(self, sigma):
        self._check(self._lib.ptc_set_denoise_variance(self._ctx, float(sigma)))

    def denoise_variance(self):
        """The estimate stage of set_param("denoise_variance", 1) alone (ptc_denoise_variance), whatever the parameter
        says, on the plane denoise() would filter now -> dict(variance float32 [h, w]: the 7 x 7 weighted variance of that plane;
        prefiltered float32 [h, w]: its 3 x 3 Gaussian, what the first pass divides by).  Needs a traced frame and the whole frame in
        this context."""
        self._push_fields()
        w, h = self._resolution
        var, pre = np.zeros((h, w), dtype=np.float32), np.zeros((h, w), dtype=np.float32)
        self._check(self._lib.ptc_denoise_variance(self._ctx, var.ctypes.data_as(C.c_void_p), pre.ctypes.data_as(C.c_void_p)))
        return {"variance": var, "prefiltered": pre}

    def denoise_variance_stats(self):
        """Counters of the last call that ran the estimate stage (denoise under "denoise_variance" 1, or denoise_variance): pixels, those
        whose first prefiltered variance is below the floor; stage_ms: the stage's launches since restart, while events are enabled."""
        s = _capi.ptc_denoise_variance_stats()
        self._check(self._lib.ptc_get_denoise_variance_stats(self._ctx, C.byref(s)))
        return {"pixels": int(s.pixels), "floored": int(s.floored), "stage_ms": float(s.stage_ms)}

    def denoise_albedo_stats(self):
        """Counters of the last call that ran the albedo stage (denoise under "denoise_albedo" 1, or denoise_albedo): pixels, those whose
        first hit is diffuse or metal, those that took a texel, channels on the albedo floor; stage_ms: the stage's launches since
        restart, while events are enabled."""
        s = _capi.ptc_denoise_albedo_stats()
        self._check(self._lib.ptc_get_denoise_albedo_stats(self._ctx, C.byref(s)))
        return {"pixels": int(s.pixels), "surface_hits": int(s.surface_hits), "texel_lookups": int(s.texel_lookups),
                "floored": int(s.floored), "stage_ms": float(s.stage_ms)}

    def send_to_preview(self, dev_pbo=None, resolution=None, display_type=DisplayBufferType.final):
        """With dev_pbo=None returns an [h, w, 4] uint8 array; otherwise writes RGBA8 to the device pointer."""
        if dev_pbo is not None:
            self._check(self._lib.ptc_present_rgba8(self._ctx, C.c_void_p(int(dev_pbo)), 1, int(display_type)))
            return None
        out = np.empty((self.pixel_count(), 4), dtype=np.uint8)
        self._check(self._lib.ptc_present_rgba8(self._ctx, out.ctypes.data_as(C.c_void_p), 0, int(display_type)))
        return out.reshape(self._rows[1] - self._rows[0], self._resolution[0], 4)

    # -- additions (no reference equivalent) ----------------------------------------------------------
    def set_rows(self, row_begin, row_end):
        self._check(self._lib.ptc_set_rows(self._ctx, int(row_begin), int(row_end)))
        self._rows = (int(row_begin), int(row_end))

    def set_interleave(self, rank, nranks, block_rows):
        """Rows dealt in blocks of block_rows round-robin over nranks contexts (load-balanced multi-GPU split)."""
        self._check(self._lib.ptc_set_interleave(self._ctx, int(rank), int(nranks), int(block_rows)))
        h = self._resolution[1]
        blocks = (h + block_rows - 1) // block_rows
        rows = sum(min(block_rows, h - gb * block_rows) for gb in range(rank, blocks, nranks))
        self._rows = (0, rows)

    def pixel_count(self):
        return (self._rows[1] - self._rows[0]) * self._resolution[0]

    def set_iteration(self, it):
        self._check(self._lib.ptc_set_iteration(self._ctx, int(it)))

    def set_stream(self, hip_stream):
        self._check(self._lib.ptc_set_stream(self._ctx, C.c_void_p(int(hip_stream)) if hip_stream else None))

    def trace_begin(self, camera):
        self._push_fields()
        cam = camera.to_c() if isinstance(camera, Camera) else camera
        self._check(self._lib.ptc_trace_begin(self._ctx, C.byref(cam)))

    def trace_bounce(self, bounce, slot_base_dev=None):
        self._check(self._lib.ptc_trace_bounce(self._ctx, int(bounce), C.c_void_p(int(slot_base_dev)) if slot_base_dev else None))

    def trace_end(self):
        self._check(self._lib.ptc_trace_end(self._ctx))

    def live_count_dev(self, bounce):
        p = C.c_void_p()
        self._check(self._lib.ptc_live_count_dev(self._ctx, int(bounce), C.byref(p)))
        return p.value

    def copy_live_count(self, bounce, dst_dev):
        self._check(self._lib.ptc_copy_live_count(self._ctx, int(bounce), C.c_void_p(int(dst_dev))))

    def read_live_count(self, bounce):
        """Host value of the live-path count entering `bounce` of the frame being built (synchronises its stream)."""
        v = C.c_uint32(0)
        self._check(self._lib.ptc_read_live_count(self._ctx, int(bounce), C.byref(v)))
        return int(v.value)

    # -- several GPUs: bands over HIP inter-process memory (include/ptcore.h) -----------------------------------
    def band_export(self):
        """bytes of this rank's ptc_band_handle (to be sent to the root over the application's own channel)"""
        h = _capi.ptc_band_handle()
        self._check(self._lib.ptc_band_export(self._ctx, C.byref(h)))
        return bytes(h)

    def band_import(self, rank, handle_bytes):
        h = _capi.ptc_band_handle.from_buffer_copy(handle_bytes)
        self._check(self._lib.ptc_band_import(self._ctx, int(rank), C.byref(h)))

    def band_publish(self, which="color"):
        sel = {"color": _capi.BUF_COLOR, "normal": _capi.BUF_NORMAL, "depth": _capi.BUF_DEPTH, "final": _capi.BUF_FINAL}[which]
        self._check(self._lib.ptc_band_publish(self._ctx, sel))

    def gather_frame(self, which="color", dev_ptr=None):
        """root: the whole frame [h, w, 3] (or [h, w] for depth) from its own rows and the published rows of the
        imported ranks; into a device pointer when given"""
        sel = {"color": _capi.BUF_COLOR, "normal": _capi.BUF_NORMAL, "depth": _capi.BUF_DEPTH, "final": _capi.BUF_FINAL}[which]
        w, h = self._resolution
        if dev_ptr is not None:
            self._check(self._lib.ptc_gather_frame(self._ctx, sel, C.c_void_p(int(dev_ptr)), 1))
            return None
        ch = 1 if which == "depth" else 3
        out = np.empty(w * h * ch, dtype=np.float32)
        self._check(self._lib.ptc_gather_frame(self._ctx, sel, out.ctypes.data_as(C.c_void_p), 0))
        return out.reshape(h, w) if ch == 1 else out.reshape(h, w, 3)

    def gather_last_us(self):
        """root: device time of the most recent gather launch, in microseconds"""
        us = C.c_float(0.0)
        self._check(self._lib.ptc_gather_last_us(self._ctx, C.byref(us)))
        return float(us.value)

    def gather_present(self, display_type=DisplayBufferType.final):
        w, h = self._resolution
        out = np.empty((h * w, 4), dtype=np.uint8)
        self._check(self._lib.ptc_gather_present_rgba8(self._ctx, out.ctypes.data_as(C.c_void_p), 0, int(display_type)))
        return out.reshape(h, w, 4)

    def synchronize(self):
        self._check(self._lib.ptc_synchronize(self._ctx))

    def download(self, which):
        """which: 'color' | 'normal' | 'depth' | 'final' -> float32 array [rows, w, 3] (or [rows, w] for depth)."""
        sel = {"color": _capi.BUF_COLOR, "normal": _capi.BUF_NORMAL, "depth": _capi.BUF_DEPTH, "final": _capi.BUF_FINAL}[which]
        n = self.pixel_count()
        ch = 1 if which == "depth" else 3
        out = np.empty(n * ch, dtype=np.float32)
        self._check(self._lib.ptc_download(self._ctx, sel, out.ctypes.data_as(C.c_void_p), 0))
        rows, w = self._rows[1] - self._rows[0], self._resolution[0]
        return out.reshape(rows, w) if ch == 1 else out.reshape(rows, w, 3)

    def download_to_device(self, which, dev_ptr):
        sel = {"color": _capi.BUF_COLOR, "normal": _capi.BUF_NORMAL, "depth": _capi.BUF_DEPTH, "final": _capi.BUF_FINAL}[which]
        self._check(self._lib.ptc_download(self._ctx, sel, C.c_void_p(int(dev_ptr)), 1))

    def stats(self):
        s = _capi.ptc_stats()
        self._check(self._lib.ptc_get_stats(self._ctx, C.byref(s)))
        return {"rays_total": int(s.rays_total), "frames": int(s.frames),
                "last_live": [int(x) for x in s.last_live[: self.max_bounces]],
                "bvh_node_count": int(s.bvh_node_count), "bvh_max_depth": int(s.bvh_max_depth),
                "triangle_count": int(s.triangle_count), "stack_capacity": int(s.stack_capacity)}

    def build_bvh(self, mesh):
        """bvh_from_mesh (accelerators/bvh.cpp:211-253) on this context's GPU (ptc_build_bvh_device): the nodes the
        host builder (scene_description.bvh_from_mesh) returns.  -> (nodes structured array, max_depth)"""
        from .scene_description import BVH_NODE_DTYPE
        t = mesh.triangle_count()
        nodes = np.zeros(max(2 * t - 1, 1), dtype=BVH_NODE_DTYPE)
        depth = C.c_uint32(0)
        rc = self._lib.ptc_build_bvh_device(self._ctx, mesh.positions.ctypes.data_as(C.POINTER(C.c_float)), len(mesh.positions),
                                            mesh.indices.ctypes.data_as(C.POINTER(C.c_uint32)), len(mesh.indices),
                                            nodes.ctypes.data_as(C.POINTER(_capi.ptc_bvh_node)), C.byref(depth))
        if rc < 0:
            self._check(rc)
        return nodes[:rc], depth.value

    def upload_times(self):
        """milliseconds of the last scene upload by stage (ptc_upload_times)"""
        t = _capi.ptc_upload_times()
        self._check(self._lib.ptc_get_upload_times(self._ctx, C.byref(t)))
        return {k: (int(getattr(t, k)) if k.endswith("on_device") else round(float(getattr(t, k)), 2)) for k, _ in t._fields_}

    LAYOUTS = {"bvh4q": 0, "leaf_parent": 1, "tris": 2, "wide": 3, "bvh": 4}

    def download_layout(self, which):
        """bytes of one device-resident traversal array of the uploaded scene (ptc_download_layout)"""
        n = C.c_uint64(0)
        self._check(self._lib.ptc_download_layout(self._ctx, self.LAYOUTS[which], None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint8)
        self._check(self._lib.ptc_download_layout(self._ctx, self.LAYOUTS[which], out.ctypes.data, n.value, None))
        return out

    def set_trace_variant(self, variant):
        self._check(self._lib.ptc_set_trace_variant(self._ctx, int(variant)))

    def set_param(self, name, value):
        self._check(self._lib.ptc_set_param(self._ctx, name.encode(), int(value)))

    def set_profiling(self, time_trace_kernel=False, count_tests=False):
        self._check(self._lib.ptc_set_profiling(self._ctx, int(time_trace_kernel), int(count_tests)))

    def reset_profile(self):
        self._check(self._lib.ptc_reset_profile(self._ctx))

    def profile(self):
        p = _capi.ptc_profile()
        self._check(self._lib.ptc_get_profile(self._ctx, C.byref(p)))
        n = self.max_bounces
        return {"paths": [int(x) for x in p.paths[:n]], "box_tests": [int(x) for x in p.box_tests[:n]],
                "tri_tests": [int(x) for x in p.tri_tests[:n]], "trace_ms": [float(x) for x in p.trace_ms[:n]],
                "trace_launches": [int(x) for x in p.trace_launches[:n]],
                "max_box_tests": [int(x) for x in p.max_box_tests[:n]],
                "listed_rays": [int(x) for x in p.listed_rays[:n]],
                "slow_rays": [int(x) for x in p.slow_rays[:n]],
                "node_visits": [int(x) for x in p.node_visits[:n]],
                "denoise_ms": float(p.denoise_ms), "denoise_passes": int(p.denoise_passes),
                "persist_launches": int(p.persist_launches)}

    def intersect_rays(self, rays):
        """rays: [n, 8] float32 (origin, t_min, direction, t_max).  Returns t, normal, material, side."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = len(rays)
        t = np.empty(n, dtype=np.float32)
        nrm = np.empty((n, 3), dtype=np.float32)
        mat = np.empty(n, dtype=np.uint32)
        side = np.empty(n, dtype=np.uint8)
        self._check(self._lib.ptc_intersect_rays(
            self._ctx, rays.ctypes.data_as(C.POINTER(C.c_float)), n, t.ctypes.data_as(C.POINTER(C.c_float)),
            nrm.ctypes.data_as(C.POINTER(C.c_float)), mat.ctypes.data_as(C.POINTER(C.c_uint32)),
            side.ctypes.data_as(C.POINTER(C.c_uint8))))
        return t, nrm, mat, side

    def generate_rays(self, camera, iteration=0):
        """The primary rays of `iteration` for every pixel of this context in slot order, under the current lens: [n, 8] float32
        (origin, t_min, direction, t_max), what intersect_rays and occluded_rays take.  Moves neither stats nor the iteration."""
        self._push_fields()
        cam = camera.to_c() if isinstance(camera, Camera) else camera
        rays = np.empty((self.pixel_count(), 8), dtype=np.float32)
        self._check(self._lib.ptc_generate_rays(self._ctx, C.byref(cam), int(iteration), rays.ctypes.data_as(C.c_void_p), rays.size))
        return rays

    def occluded_rays(self, rays):
        """rays: [n, 8] float32 (origin, t_min, direction, t_max).  Returns uint8[n]: 1 where anything lies on the ray within
        [t_min, t_max] (the reference's ray_scene_intersection_test reports a hit), else 0."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = len(rays)
        occluded = np.zeros(n, dtype=np.uint8)
        self._check(self._lib.ptc_occluded_rays(
            self._ctx, rays.ctypes.data_as(C.POINTER(C.c_float)), n, occluded.ctypes.data_as(C.POINTER(C.c_uint8))))
        return occluded

    def debug_sphere_lanes(self, rays, slots, want_candidates=False):
        """The per-lane form of the trailing sphere run on the device (ptc_debug_sphere_lanes; test hook).  rays as for
        intersect_rays with t_min 1e-4 or 1e-5 and t_max >= 0; slots: 1 or the fused kernel's rays per lane.  Returns t, normal,
        material, side, and with want_candidates the candidate mask uint8[n] (bit k: object k of the run)."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = len(rays)
        t = np.empty(n, dtype=np.float32)
        nrm = np.empty((n, 3), dtype=np.float32)
        mat = np.empty(n, dtype=np.uint32)
        side = np.empty(n, dtype=np.uint8)
        cand = np.zeros(n, dtype=np.uint8) if want_candidates else None
        self._check(self._lib.ptc_debug_sphere_lanes(self._ctx, rays.ctypes.data, n, int(slots), t.ctypes.data, nrm.ctypes.data,
                                                     mat.ctypes.data, side.ctypes.data, cand.ctypes.data if want_candidates else None))
        return (t, nrm, mat, side, cand) if want_candidates else (t, nrm, mat, side)

    def occlusion_stats(self):
        """Counters of occluded_rays since reset_profile / creation."""
        s = _capi.ptc_occlusion_stats()
        self._check(self._lib.ptc_get_occlusion_stats(self._ctx, C.byref(s)))
        return {"rays": int(s.rays), "occluded": int(s.occluded), "redone": int(s.redone), "kernel_ms": float(s.kernel_ms),
                "launches": int(s.launches)}

    @staticmethod
    def light_table(scene, capacity=None):
        """The module function light_table (ptc_light_table): the lamp table of a scene, on the host."""
        return light_table(scene, capacity)

    def light_info(self):
        """Counts, total area and total weight of the uploaded scene's lamp table (ptc_get_light_info)."""
        info = _capi.ptc_light_info()
        self._check(self._lib.ptc_get_light_info(self._ctx, C.byref(info)))
        return _light_info_dict(info)

    def _direct_light_query(self, points, normals, sample_index=0, want_rays=False):
        """One light sample per surface point (ptc_direct_light).  points, normals: [n, 3] float32 (finite points, unit
        normals).  Returns radiance [n, 3]: what the lamps send to a white Lambertian surface there by this sample; with
        want_rays also the shadow rays [n, 8] (origin, t_min, direction, t_max) and visible uint8[n]."""
        points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        n = len(points)
        if len(normals) != n:
            raise ValueError("points and normals differ in length")
        radiance = np.zeros((n, 3), dtype=np.float32)
        rays = np.zeros((n, 8), dtype=np.float32) if want_rays else None
        visible = np.zeros(n, dtype=np.uint8) if want_rays else None
        self._check(self._lib.ptc_direct_light(
            self._ctx, points.ctypes.data, normals.ctypes.data, n, int(sample_index), radiance.ctypes.data,
            rays.ctypes.data if want_rays else None, visible.ctypes.data if want_rays else None, 0))
        return (radiance, rays, visible) if want_rays else radiance

    def direct_light_dev(self, points_ptr, normals_ptr, n, sample_index, radiance_ptr, rays_ptr=None, visible_ptr=None):
        """direct_light on device memory (torch tensors' data_ptr()): 3 floats per point in and out; optionally 8 floats
        per point of shadow rays (16-byte aligned) and one byte of visibility.  Synchronises like download."""
        self._check(self._lib.ptc_direct_light(
            self._ctx, C.c_void_p(int(points_ptr)), C.c_void_p(int(normals_ptr)), int(n), int(sample_index),
            C.c_void_p(int(radiance_ptr)), C.c_void_p(int(rays_ptr)) if rays_ptr else None,
            C.c_void_p(int(visible_ptr)) if visible_ptr else None, 1))

    def direct_stats(self):
        """Counters of direct_light since reset_profile / creation."""
        s = _capi.ptc_direct_stats()
        self._check(self._lib.ptc_get_direct_stats(self._ctx, C.byref(s)))
        return {"points": int(s.points), "sampled": int(s.sampled), "unoccluded": int(s.unoccluded),
                "kernel_ms": float(s.kernel_ms), "launches": int(s.launches)}

    def direct_loop_stats(self):
        """Counters of the direct-lit megakernel (direct_light = True) since restart: hits on a diffuse material, shadow rays
        traced, shadow rays that arrived."""
        s = _capi.ptc_direct_loop_stats()
        self._check(self._lib.ptc_get_direct_loop_stats(self._ctx, C.byref(s)))
        return {"diffuse_hits": int(s.diffuse_hits), "shadow_rays": int(s.shadow_rays), "unoccluded": int(s.unoccluded)}

    def _environment_light_query(self, points, normals, sample_index=0, want_rays=False):
        """One environment sample per surface point (ptc_environment_light), in _direct_light_query's shapes: radiance [n, 3] is what
        the environment sends to a white Lambertian surface there by this sample.  Needs an environment."""
        self._push_fields()
        points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        normals = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
        n = len(points)
        if len(normals) != n:
            raise ValueError("points and normals differ in length")
        radiance = np.zeros((n, 3), dtype=np.float32)
        rays = np.zeros((n, 8), dtype=np.float32) if want_rays else None
        visible = np.zeros(n, dtype=np.uint8) if want_rays else None
        self._check(self._lib.ptc_environment_light(
            self._ctx, points.ctypes.data, normals.ctypes.data, n, int(sample_index), radiance.ctypes.data,
            rays.ctypes.data if want_rays else None, visible.ctypes.data if want_rays else None, 0))
        return (radiance, rays, visible) if want_rays else radiance

    def environment_light_dev(self, points_ptr, normals_ptr, n, sample_index, radiance_ptr, rays_ptr=None, visible_ptr=None):
        """environment_light on device memory, as direct_light_dev."""
        self._push_fields()
        self._check(self._lib.ptc_environment_light(
            self._ctx, C.c_void_p(int(points_ptr)), C.c_void_p(int(normals_ptr)), int(n), int(sample_index),
            C.c_void_p(int(radiance_ptr)), C.c_void_p(int(rays_ptr)) if rays_ptr else None,
            C.c_void_p(int(visible_ptr)) if visible_ptr else None, 1))

    def environment_light_stats(self):
        """Counters of the environment-light query since reset_profile / creation."""
        s = _capi.ptc_environment_light_stats()
        self._check(self._lib.ptc_get_environment_light_stats(self._ctx, C.byref(s)))
        return {"points": int(s.points), "sampled": int(s.sampled), "unoccluded": int(s.unoccluded),
                "kernel_ms": float(s.kernel_ms), "launches": int(s.launches)}

    def environment_light_loop_stats(self):
        """Counters of the megakernel under environment_light = True since restart: hits on a diffuse material that drew an
        environment sample, its shadow rays traced, those that arrived."""
        s = _capi.ptc_environment_light_loop_stats()
        self._check(self._lib.ptc_get_environment_light_loop_stats(self._ctx, C.byref(s)))
        return {"diffuse_hits": int(s.diffuse_hits), "shadow_rays": int(s.shadow_rays), "unoccluded": int(s.unoccluded)}

    def mis_loop_stats(self):
        """Counters of the megakernel under mis = True since restart: emitter hits and misses behind a diffuse vertex that counted
        with the continuation ray's weight."""
        s = _capi.ptc_mis_loop_stats()
        self._check(self._lib.ptc_get_mis_loop_stats(self._ctx, C.byref(s)))
        return {"weighted_emitter_hits": int(s.weighted_emitter_hits), "weighted_misses": int(s.weighted_misses)}

    def smooth_loop_stats(self):
        """Counters of the megakernel under smooth_normals = True with vertex normals set, since restart: triangle hits shaded with the
        interpolated normal, those that fell back to the geometric one, paths whose new direction entered the geometry, light samples
        culled because theirs did."""
        s = _capi.ptc_smooth_loop_stats()
        self._check(self._lib.ptc_get_smooth_loop_stats(self._ctx, C.byref(s)))
        return {"shading_normals": int(s.shading_normals), "fallbacks": int(s.fallbacks), "absorbed": int(s.absorbed),
                "culled_light_samples": int(s.culled_light_samples)}

    def texture_loop_stats(self):
        """Counters of the megakernel under textures = True with textures and coordinates set, since restart: texel lookups, and hits
        that kept the material's colour because their interpolated coordinate was not finite."""
        s = _capi.ptc_texture_loop_stats()
        self._check(self._lib.ptc_get_texture_loop_stats(self._ctx, C.byref(s)))
        return {"lookups": int(s.lookups), "fallbacks": int(s.fallbacks)}

    def normal_map_loop_stats(self):
        """Counters of the megakernel under normal_maps = True with a binding, textures and coordinates set, since restart: hits whose
        normal the map replaced, and hits where the rule fell back to the base normal (a flat texel counts in neither)."""
        s = _capi.ptc_normal_map_loop_stats()
        self._check(self._lib.ptc_get_normal_map_loop_stats(self._ctx, C.byref(s)))
        return {"bent": int(s.bent), "kept": int(s.kept)}

    def hit_shading_normal(self, rays):
        """The normal the megakernel's loop would shade with at the closest hit (ptc_hit_shading_normal) of rays [n, 8], from what is
        set -> dict(normal float32 [n, 3], zeros on a miss; outcome uint8 [n]: 0 miss, 1 no map applied, 2 bent, 3 flat, 4 kept)"""
        self._push_fields()
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        nrm, how = np.zeros((len(r), 3), dtype=np.float32), np.zeros(len(r), dtype=np.uint8)
        self._check(self._lib.ptc_hit_shading_normal(self._ctx, r.ctypes.data_as(C.c_void_p), len(r), nrm.ctypes.data_as(C.c_void_p),
                                                     how.ctypes.data_as(C.c_void_p)))
        return {"normal": nrm, "outcome": how}

    def sample_texture(self, texture, st):
        """The lookup of texture `texture` of texture_table on the device, without rendering (ptc_sample_texture): st [n, 2] ->
        (rgb float32 [n, 3], zeros where the rule refuses the pair; rejected bool [n])"""
        self._push_fields()
        st = np.ascontiguousarray(st, dtype=np.float32).reshape(-1, 2)
        rgb, rej = np.zeros((len(st), 3), dtype=np.float32), np.zeros(len(st), dtype=np.uint8)
        self._check(self._lib.ptc_sample_texture(self._ctx, int(texture), st.ctypes.data_as(C.c_void_p), len(st), rgb.ctypes.data_as(C.c_void_p),
                                                 rej.ctypes.data_as(C.c_void_p)))
        return rgb, rej.astype(bool)

    def hit_surface(self, rays):
        """The closest hit's texture coordinate and albedo (ptc_hit_surface) of rays [n, 8] -> dict(st float32 [n, 2], albedo float32
        [n, 3]: texel x colour where a texture applies, else the material's colour; zeros on a miss)"""
        self._push_fields()
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        st, alb = np.zeros((len(r), 2), dtype=np.float32), np.zeros((len(r), 3), dtype=np.float32)
        self._check(self._lib.ptc_hit_surface(self._ctx, r.ctypes.data_as(C.c_void_p), len(r), st.ctypes.data_as(C.c_void_p),
                                              alb.ctypes.data_as(C.c_void_p)))
        return {"st": st, "albedo": alb}

    def hit_attributes(self, rays):
        """The closest hit's primitive and attributes (ptc_hit_attributes) of rays [n, 8] (origin, t_min, direction, t_max) ->
        dict(object uint32 [n] (0xffffffff: a miss), triangle uint32 [n] (0xffffffff: a sphere or a miss), uv float32 [n, 2],
        normal float32 [n, 3]: the shading normal where vertex normals are set, else the geometric one)."""
        self._push_fields()
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        n = len(r)
        obj, tri = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        uv, nrm = np.zeros((n, 2), dtype=np.float32), np.zeros((n, 3), dtype=np.float32)
        self._check(self._lib.ptc_hit_attributes(self._ctx, r.ctypes.data_as(C.c_void_p), n, obj.ctypes.data_as(C.c_void_p),
                                                 tri.ctypes.data_as(C.c_void_p), uv.ctypes.data_as(C.c_void_p), nrm.ctypes.data_as(C.c_void_p)))
        return {"object": obj, "triangle": tri, "uv": uv, "normal": nrm}

    def environment_light_pdf(self, dirs):
        """The environment sample's solid-angle density (ptc_environment_light_pdf) in unit directions [n, 3] -> float32 [n].  Needs
        an environment."""
        self._push_fields()
        dirs = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
        out = np.zeros(len(dirs), dtype=np.float32)
        self._check(self._lib.ptc_environment_light_pdf(self._ctx, dirs.ctypes.data, len(dirs), out.ctypes.data, 0))
        return out

    def environment_light_pdf_dev(self, dirs_ptr, n, pdf_ptr):
        """environment_light_pdf on device memory."""
        self._push_fields()
        self._check(self._lib.ptc_environment_light_pdf(self._ctx, C.c_void_p(int(dirs_ptr)), int(n), C.c_void_p(int(pdf_ptr)), 1))

    def selftest_math(self, a, b):
        a = np.ascontiguousarray(a, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32)
        outs = [np.empty_like(a) for _ in range(4)]
        fp = C.POINTER(C.c_float)
        self._check(self._lib.ptc_selftest_math(self._ctx, a.ctypes.data_as(fp), b.ctypes.data_as(fp), len(a),
                                                *[o.ctypes.data_as(fp) for o in outs]))
        return outs

    def selftest_rng(self, seeds, discards):
        """The per-path generator on the device (ptc_selftest_rng) -> uint32 [n, 6]: state after the seed, state after the
        discard, two raw values, the bit patterns of the two uniform draws behind them."""
        seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
        discards = np.ascontiguousarray(discards, dtype=np.uint32)
        assert seeds.shape == discards.shape and seeds.ndim == 1
        out = np.zeros((len(seeds), 6), dtype=np.uint32)
        self._check(self._lib.ptc_selftest_rng(self._ctx, seeds.ctypes.data, discards.ctypes.data, len(seeds), out.ctypes.data))
        return out
