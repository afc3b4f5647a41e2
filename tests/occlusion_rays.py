"""Scene and seeded ray generators of the occlusion tests (tests/test_occlusion_cpu.py, tests/test_gpu_occlusion.py) and of
tools/occlusion_ab.py -- TEST INFRASTRUCTURE, numpy only.

occluded(ray) := the reference's ray_scene_intersection_test (path_tracer.cu:110-128) reports a hit, which is the `hit` flag
of the oracle's orc_intersect_rays.  Nothing here computes an expected answer; it only makes inputs."""
import numpy as np

FMAX = np.finfo(np.float32).max
LAMP = (0.2, -0.45, -0.3)    # the point the shadow-style rays of occlusion_scene run towards


def occlusion_scene(pkg, n_lat=108, n_lon=324):
    """Config 2's room (four wall spheres) and its two instances of the displaced-sphere mesh and its small glass sphere,
    plus a scaled sphere whose centre sits in the Sphere struct (object-space t against the world-space t_max)."""
    glm = pkg.glmlite
    s = pkg.scenes.cornell_bunny((64, 64), n_lat=n_lat, n_lon=n_lon)
    s.add_object(pkg.Sphere((0.4, 0.3, -0.2), 1.0), glm.compose([glm.scale((0.45, 0.3, 0.4)), glm.translate((-0.3, 0.55, -0.6))]), "glass")
    return s


def one_object_scenes(pkg, scene):
    """The scene cut into one scene per object (same materials, same mesh): the groups of the OR-over-groups property."""
    names = sorted(scene.material_map_, key=lambda s: s.encode())
    out = []
    for k, (shape, transform) in enumerate(scene.objects_):
        one = pkg.SceneDescription()
        for nm in names:
            one.add_material(nm, scene.material_map_[nm])
        if not isinstance(shape, pkg.Sphere):
            one.add_mesh("only", shape)
        one.add_object(shape, transform, scene.objects_material_mapping_[k])
        out.append(one)
    return out


def _pack(o, d, tmin, tmax):
    rays = np.zeros((len(o), 8), dtype=np.float32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, tmin, d, tmax
    return rays


def shadow_rays(n=60000, seed=11, lamp=LAMP, lo=(-1.95, -0.98, -1.95), hi=(1.95, 1.3, 2.6)):
    """n rays from seeded points of the room towards the lamp point: direction normalised in binary64 and rounded, t_min 1e-4
    or 1e-5, t_max FLT_MAX or 0.5 / 0.999 / 1 / 2 x the distance to the lamp (five equal shares, dealt by index)."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(lo, hi, size=(n, 3))
    d = np.asarray(lamp, dtype=np.float64) - o
    dist = np.linalg.norm(d, axis=1)
    d /= dist[:, None]
    tmin = np.where(rng.uniform(size=n) < 0.5, 1e-4, 1e-5)
    factor = np.array([0.0, 0.5, 0.999, 1.0, 2.0])[np.arange(n) % 5]
    tmax = np.where(factor == 0.0, np.float64(FMAX), factor * dist)
    return _pack(o, d, tmin, tmax)


def towards_points(origins, targets, factors, seed):
    """Shadow rays origin -> target, t_max = factor x distance (factors dealt by index), t_min 1e-4 or 1e-5 (seeded)."""
    rng = np.random.default_rng(seed)
    o = np.asarray(origins, dtype=np.float64)
    d = np.asarray(targets, dtype=np.float64) - o
    dist = np.linalg.norm(d, axis=1)
    d /= dist[:, None]
    n = len(o)
    tmin = np.where(rng.uniform(size=n) < 0.5, 1e-4, 1e-5)
    f = np.asarray(factors, dtype=np.float64)[np.arange(n) % len(factors)]
    return _pack(o, d, tmin, f * dist), f


def terrain_rays(pkg, n, seed=5, light=(0.5, 1.5, 1.0)):
    """The two ray sets of tools/occlusion_ab.py on the heightfield scene (config 3): n origins a hair above seeded points of
    the terrain's analytic surface (scenes.heightfield_mesh: y = 0.15 sin 3x cos 5z, +-0.02 of noise on top), (a) towards a
    point light low above it with t_max = the distance, (b) the same origins with cosine-spread directions about +y, t_max
    FLT_MAX."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-3.98, 3.98, n)
    z = rng.uniform(-1.98, 1.98, n)
    y = 0.15 * np.sin(3.0 * x) * np.cos(5.0 * z) + 0.021 + rng.uniform(0.0, 0.01, n)
    o = np.stack([x, y, z], axis=1)
    d = np.asarray(light, dtype=np.float64) - o
    dist = np.linalg.norm(d, axis=1)
    d /= dist[:, None]
    shadow = _pack(o, d, 1e-4, dist)
    u1, u2 = rng.uniform(size=n), rng.uniform(size=n)
    r, phi = np.sqrt(u1), 2.0 * np.pi * u2
    c = np.stack([r * np.cos(phi), np.sqrt(1.0 - u1), r * np.sin(phi)], axis=1)
    c /= np.linalg.norm(c, axis=1)[:, None]
    spread = _pack(o, c, 1e-4, np.float64(FMAX))
    return shadow, spread


def lamp_rays(n=40000, seed=23):
    """Shadow rays in scenes.cornell_lit(with_mesh=True): origins uniform in the room, the first half aimed at seeded points
    on the sphere lamp's surface (centre (0.9, 1.5, -1.2), radius 0.25), the second at points on the panel lamp (the quad
    x in [-0.5, 0.5], z in [-1.3, -0.3] at y = 1.49); t_max = 0.5 / 0.999 / 1 / 2 x the distance.  Returns (rays, factors)."""
    rng = np.random.default_rng(seed)
    o = rng.uniform((-1.95, -0.95, -1.95), (1.95, 1.45, 2.5), size=(n, 3))
    v = rng.normal(size=(n // 2, 3))
    on_sphere = np.array([0.9, 1.5, -1.2]) + 0.25 * v / np.linalg.norm(v, axis=1)[:, None]
    m = n - n // 2
    on_panel = np.stack([rng.uniform(-0.5, 0.5, m), np.full(m, 1.49), rng.uniform(-1.3, -0.3, m)], axis=1)
    return towards_points(o, np.concatenate([on_sphere, on_panel]), (0.5, 0.999, 1.0, 2.0), seed + 1)
