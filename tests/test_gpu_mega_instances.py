"""Every megakernel instance once (csrc/pt_mega_rules.hpp: 22 kernels): the frame that reaches it renders what the library rendered
before the launch path became one frame description, one rule and one launcher.  The device code of that change is byte for byte the
parent's, so a row tests what the change can break: the host's choice of the kernel and the arguments it hands over.

Each row sets up the facts of one kernel on a shipped scene -- "room": assets/scenes/cornell_textured.json (two textured box meshes,
texture coordinates; vertex normals computed) with one lamp sphere added here, since the asset has no emitter; "balls":
assets/scenes/spheres_sky.json (spheres alone, no emitter); the sky is that scene's tests/golden/environment/sky_dusk.hdr map -- at
32 x 24 pixels, 2 iterations, 4 bounces, and asserts that the CPU rule names the row's kernel for those facts, that the render
succeeds, that colour, normal, depth and rays_total are the recorded ones, and that the loop counters outside the kernel's family
stayed zero.

EXPECTED was recorded with the library of the parent commit (40f42dd, ten launchers and the ladder in ptc_trace) on an MI355X, by
running _render over ROWS with PTCORE_LIB naming that build, before the change was applied; profiles/mega_launch_refactor.txt lists
the same values beside the change's."""
import hashlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, ITERS, BOUNCES = 32, 24, 2, 4
LENS = (0.15, 4.0)
FACTS = ("direct", "env", "env_lit", "smooth", "textured", "weigh", "lens", "plays", "emitters")
_cache = {}


def _row(kernel, scene, roulette=0, **on):
    """on: the options of the context (direct_light, environment_light, mis, smooth_normals, textures), sky, lens"""
    return dict(kernel=kernel, scene=scene, roulette=roulette, **on)


ROWS = [
    _row("k_megakernel_tex<true, true>", "room", 1, textures=1, smooth_normals=1, mis=1, direct_light=1, environment_light=1, sky=1, lens=1),
    _row("k_megakernel_tex<true, false>", "room", 0, textures=1, mis=1, direct_light=1),
    _row("k_megakernel_tex<false, true>", "room", 2, textures=1, smooth_normals=1, environment_light=1, sky=1),
    _row("k_megakernel_tex<false, false>", "room", 0, textures=1),
    _row("k_megakernel_smooth<true>", "room", 0, smooth_normals=1, mis=1, environment_light=1, sky=1),
    _row("k_megakernel_smooth<false>", "room", 3, smooth_normals=1, direct_light=1, lens=1),
    _row("k_megakernel_mis", "room", 1, mis=1, direct_light=1, environment_light=1, sky=1),
    _row("k_megakernel_env_light", "balls", 0, environment_light=1, sky=1, lens=1),
    _row("k_megakernel_env<true>", "room", 0, direct_light=1, sky=1),
    _row("k_megakernel_env<false>", "balls", 2, sky=1),
    _row("k_megakernel_direct_lens<true>", "room", 1, direct_light=1, lens=1),
    _row("k_megakernel_direct_lens<false>", "room", 0, direct_light=1, lens=1),
    _row("k_megakernel_direct<true>", "room", 2, direct_light=1),
    _row("k_megakernel_direct<false>", "room", 3, direct_light=1),
    _row("k_megakernel_lens<true, true>", "room", 1, lens=1),
    _row("k_megakernel_lens<true, false>", "room", 0, lens=1),
    _row("k_megakernel_lens<false, true>", "balls", 2, lens=1),
    _row("k_megakernel_lens<false, false>", "balls", 4, lens=1),
    _row("k_megakernel<true, true>", "room", 2),
    _row("k_megakernel<true, false>", "room", 0),
    _row("k_megakernel<false, true>", "balls", 1),
    _row("k_megakernel<false, false>", "balls", 0),
]

# kernel -> (sha256 of colour + normal + depth, float32 bytes in that order; rays_total)
EXPECTED = {
    "k_megakernel_tex<true, true>": ("6fe4d0dbc4b2decea16785268713b1fcbe4825baa526928982d7ed310c8cb644", 4530),
    "k_megakernel_tex<true, false>": ("1c082ef51c0196ee4a33cb50c2c5dfeba279dd926ef1df7730bbddba822429e2", 5983),
    "k_megakernel_tex<false, true>": ("a03441599c4c80edc670a2552dec033a17a2030580370d3b1c01ec042617ca51", 4976),
    "k_megakernel_tex<false, false>": ("5299ca19d9d26ce333b42c59c02cd5e8a61635255d990e43a91318a9bd2d25db", 5983),
    "k_megakernel_smooth<true>": ("7886f1baa38fe040722c073ef6b1ef26e0876f6e02fbed7b5051b299daa2eb4d", 5847),
    "k_megakernel_smooth<false>": ("1c9ed2adac8c9fa4761d836f7301b9cb99eb1de8bc4bb8019491b3c0b73738dd", 5857),
    "k_megakernel_mis": ("a3f73f6111556c9d0496e2ea568ec8a5ead705751580591aa29d71b260dbcf84", 4717),
    "k_megakernel_env_light": ("9769a1754b7baf6f588a797a9e3ee98974bce93a3b1388dd686be4b51d31faaf", 2881),
    "k_megakernel_env<true>": ("4574a1410ab2f0ea9d2510560c774d5bec25519fe0b74e7ef070b896ae291d6d", 5983),
    "k_megakernel_env<false>": ("d9c4a4cb917d220ccb73df350e88b454ed995db5cbd60297570732939a6aed0b", 2828),
    "k_megakernel_direct_lens<true>": ("fc9c6c2906bf50a40a2ec5ebf5348672a6c8610cce64eb03b4970ae8ed226221", 4723),
    "k_megakernel_direct_lens<false>": ("dd81bf7a6725498940dc05a97b8c06f30672ced790f924797c6668077b329351", 5989),
    "k_megakernel_direct<true>": ("5f3812e28ce7f6c18c984705def9489d2afe290e31966974495af0c6dde48c26", 5157),
    "k_megakernel_direct<false>": ("daafe7f68f70219e53d12e92845123cdb1d0bbc99654cdb3dd3ae8e7afa0e8ff", 5983),
    "k_megakernel_lens<true, true>": ("4b09e9eab04e2218ff6cfee6ddfb77ed0fbfb093a3bb3d60f9d2d4bf604b373b", 4723),
    "k_megakernel_lens<true, false>": ("90fe414c11173f7a8a3000976d3f520b10836c2a9114bd67308e78e27706a72f", 5989),
    "k_megakernel_lens<false, true>": ("bceaf05fea921ee9c4688dbf81bda2f733480ef77120e8bee4461dc885e056a7", 2836),
    "k_megakernel_lens<false, false>": ("410ae748c609130196036e93c8a597deb4a6ed5afe56e230af4f2ecdd4670889", 2881),
    "k_megakernel<true, true>": ("358a172d4579270a862a93c6a49eefd3a898c2a6b2dd66f70b6ea35a97745f61", 5157),
    "k_megakernel<true, false>": ("ed4f686d1a2b4dcb1e72acdf9387555feb38f6cc39bf0652c6d4a040131aa1a9", 5983),
    "k_megakernel<false, true>": ("a83110bf51d57eb77c450efd8e98ee01c6d852331cc5b61c15cc7e61756f8d9e", 2756),
    "k_megakernel<false, false>": ("b052df07e70fa3c797123981a0e2c6f7a0a2eeebf40e55db7cbbb3171ffe3caa", 2870),
}


def _scenes(pkg):
    """name -> dict(scene, flat, normals); the sky map"""
    if not _cache:
        room = pkg.json_parser.scene_from_json(os.path.join(ROOT, "assets", "scenes", "cornell_textured.json"))
        room.add_material("lamp", pkg.EmissiveMaterial((12.0, 11.0, 9.0)))
        room.add_object(pkg.Sphere((0.0, 0.0, 0.0), 0.4), pkg.glmlite.translate((0.2, 1.5, 0.6)), "lamp")
        balls = pkg.json_parser.scene_from_json(os.path.join(ROOT, "assets", "scenes", "spheres_sky.json"))
        for name, scene in (("room", room), ("balls", balls)):
            flat = scene.build_scene()
            _cache[name] = dict(scene=scene, flat=flat, normals=pkg.compute_vertex_normals(flat) if name == "room" else None)
        _cache["sky"] = balls.environment
    return _cache


def facts_of(row):
    """the nine facts ptc_trace derives for the row's frame (the scenes above: "room" has a lamp, normals, coordinates and textures)"""
    room = row["scene"] == "room"
    direct = bool(row.get("direct_light")) and room
    env = bool(row.get("sky"))
    env_lit = bool(row.get("environment_light")) and env
    return dict(direct=direct, env=env, env_lit=env_lit, smooth=bool(row.get("smooth_normals")) and room,
                textured=bool(row.get("textures")) and room, weigh=bool(row.get("mis")) and (direct or env_lit), lens=bool(row.get("lens")),
                plays=1 <= row["roulette"] < BOUNCES - 1, emitters=room)


def _render(pkg, row):
    """-> (sha256 of the three planes, rays_total, the fourteen loop-counter words)"""
    s = _scenes(pkg)[row["scene"]]
    with pkg.PathTracer(device=0, max_bounces=BOUNCES) as pt:
        pt.current_gpu_method = pkg.GPUMethod.megakernel
        for option in ("direct_light", "environment_light", "mis", "smooth_normals", "textures"):
            setattr(pt, option, bool(row.get(option)))
        pt.roulette = row["roulette"]
        if row.get("lens"):
            pt.lens = LENS
        pt.create_buffers((W, H), s["flat"])
        if s["normals"] is not None:  # the room carries everything in every row: the options alone decide
            pt.vertex_normals = s["normals"]
            pt.load_scene_textures(s["flat"])
        pt.environment = _scenes(pkg)["sky"] if row.get("sky") else None
        pt.restart()
        pt.max_iterations = ITERS
        for _ in range(ITERS):
            pt.path_trace(s["scene"].camera)
        h = hashlib.sha256()
        for plane in ("color", "normal", "depth"):
            h.update(np.ascontiguousarray(pt.download(plane), dtype=np.float32).tobytes())
        words = list(pt.direct_loop_stats().values()) + list(pt.environment_light_loop_stats().values()) + list(pt.mis_loop_stats().values())
        words += list(pt.smooth_loop_stats().values()) + list(pt.texture_loop_stats().values())
        return h.hexdigest(), pt.stats()["rays_total"], words


def test_the_rows_are_the_22_kernels():
    assert len({r["kernel"] for r in ROWS}) == 22 and set(EXPECTED) == {r["kernel"] for r in ROWS}


@pytest.mark.parametrize("row", ROWS, ids=[r["kernel"] for r in ROWS])
def test_instance_renders_the_parents_frame(pkg, row):
    facts = facts_of(row)
    name, _ = pkg.check_megakernel_instance(roulette=row["roulette"], max_bounces=BOUNCES, **facts)
    assert name == row["kernel"], (facts, name)
    sha, rays, words = _render(pkg, row)
    print(row["kernel"], sha, rays, words)
    assert len(words) == 14
    assert (sha, rays) == EXPECTED[row["kernel"]]
    # the families of the loop counters: a word outside the frame's families was never added to
    for lo, hi, fact in ((3, 6, "env_lit"), (6, 8, "weigh"), (8, 12, "smooth"), (12, 14, "textured")):
        if not facts[fact]:
            assert not any(words[lo:hi]), (fact, words)
