"""Constructed seeds: the (pixel, iteration) pairs at which the per-path generator (csrc/pt_rng.hpp) meets the edges that
ordinary frames meet about once in 2^30 paths -- the special cases of Minstd::seed and the states whose uniform() is exactly
0.0 or exactly 1.0f -- and the closed room the frames on them are traced in.

hash32 is a bijection of the 32-bit words, so path_seed(pixel, iteration) = hash32(hash32(pixel) ^ iteration) takes a wanted
value s for exactly one iteration per pixel: iteration = hash32_inv(s) ^ hash32(pixel).  Everything here is plain Python
integers (the big-integer restatement of the generator) and numpy binary32; the proofs that a case hits its target go through
the oracle's own generator (tests/test_rng_edges_cpu.py, before a GPU is touched)."""
import ctypes as C

import numpy as np

MASK = 0xFFFFFFFF
M31 = 2**31 - 1            # the modulus m of minstd_rand
A = 48271
A_INV = pow(A, -1, M31)
XOR_LIGHT = 0x4C495445     # ptc_direct_light xors its seeds with this (include/ptcore.h)

# states x (the value next() returns) whose uniform() = float(x - 1) / 2^31 is an edge:
#   x = 1: exactly 0.0;  x - 1 >= 2^31 - 64 rounds to 2^31 (a tie at 2^31 - 64 goes to the even mantissa): exactly 1.0f for the
#   62 states [2^31 - 63, 2^31 - 2];  2^31 - 64 gives the largest binary32 below 1
STATE_ZERO = 1
STATE_ONE_LO = 2**31 - 63
STATE_ONE_HI = 2**31 - 2
STATE_BELOW_ONE = 2**31 - 64
EDGE_STATES = (("0.0", STATE_ZERO), ("1.0f low end", STATE_ONE_LO), ("1.0f high end", STATE_ONE_HI),
               ("largest below 1", STATE_BELOW_ONE))
# the four seeds Minstd::seed treats specially (0, m, 2m -> state 1; 2^32 - 1 -> state 1 after two folds) and their neighbours
SPECIAL_SEEDS = (0, M31, 2 * M31, 2**32 - 1)
SEED_NEIGHBOURS = (1, M31 - 1, M31 + 1)


def hash32(a):
    a = ((a + 0x7ED55D16) + (a << 12)) & MASK
    a = ((a ^ 0xC761C23C) ^ (a >> 19)) & MASK
    a = ((a + 0x165667B1) + (a << 5)) & MASK
    a = ((a + 0xD3A2646C) ^ (a << 9)) & MASK
    a = ((a + 0xFD7046C5) + (a << 3)) & MASK
    a = ((a ^ 0xB55A4F09) ^ (a >> 16)) & MASK
    return a


def _inv_add_shl(y, c, s):      # y = (a + c) + (a << s) = a (1 + 2^s) + c
    return ((y - c) * pow(1 + (1 << s), -1, 1 << 32)) & MASK


def _inv_xor_shr(y, c, s):      # y = (a ^ c) ^ (a >> s): the top s bits are a's, the rest follow from them
    y ^= c
    a = y
    for _ in range(32 // s + 1):
        a = y ^ (a >> s)
    return a & MASK


def _inv_add_xor_shl(y, c, s):  # y = (a + c) ^ (a << s): bit i of y depends on the bits <= i of a only
    a = 0
    for i in range(32):
        for b in (0, 1):
            t = a | (b << i)
            if ((((t + c) & MASK) ^ ((t << s) & MASK)) >> i) & 1 == (y >> i) & 1:
                a = t
                break
    return a


def hash32_inv(y):
    y = _inv_xor_shr(y, 0xB55A4F09, 16)
    y = _inv_add_shl(y, 0xFD7046C5, 3)
    y = _inv_add_xor_shl(y, 0xD3A2646C, 9)
    y = _inv_add_shl(y, 0x165667B1, 5)
    y = _inv_xor_shr(y, 0xC761C23C, 19)
    y = _inv_add_shl(y, 0x7ED55D16, 12)
    return y


def path_seed(index, iteration):
    return hash32(hash32(index & MASK) ^ (iteration & MASK))


# ---- the generator in big integers -----------------------------------------------------------------------------------
def seed_state(s):
    x = s % M31
    return x if x else 1


def advance(x, k):
    """the state k steps on (k raw values later; discard(k))"""
    return x * pow(A, k, M31) % M31


def uniform_bits(x):
    """bit pattern of uniform() when next() has returned x"""
    return int((np.float32(x - 1) / np.float32(2147483648.0)).view(np.uint32))


def selftest_words(s, z):
    """what ptc_check_rng / ptc_selftest_rng write for (seed s, discard z)"""
    x0 = seed_state(s)
    x1 = advance(x0, z)
    r = [advance(x1, k) for k in (1, 2, 3, 4)]
    return [x0, x1, r[0], r[1], uniform_bits(r[2]), uniform_bits(r[3])]


def aliases(state):
    """the seeds that Minstd::seed maps to `state` (1 <= state < m): s and s + m where that fits 32 bits, and for state 1 the
    three seeds that are 0 mod m"""
    out = [state] + ([state + M31] if state + M31 <= MASK else [])
    return out + ([0, M31, 2 * M31] if state == 1 else [])


def seeds_for_draw(state, k):
    """the seeds after which the k-th draw (k >= 1) has next() == state"""
    return aliases(state * pow(A_INV, k, M31) % M31)


def place(target_seed_aliases, pixels, accept=None, xor=0, limit=2**31):
    """-> (pixel, iteration, seed): the first pixel of `pixels` for which some alias is path_seed(pixel, iteration) ^ xor with an
    iteration in [0, limit) -- and, if given, accept(pixel, iteration) holds.  Raises when no candidate is left: a target is never
    skipped; the caller widens `pixels`."""
    pre = [(s, hash32_inv((s ^ xor) & MASK)) for s in target_seed_aliases]
    for p in pixels:
        hp = hash32(int(p))
        for s, q in pre:
            it = q ^ hp
            if it < limit and (accept is None or accept(int(p), it)):
                assert path_seed(int(p), it) ^ xor == s
                return int(p), it, s
    raise AssertionError(f"no pixel of {len(pixels)} reaches one of the seeds {target_seed_aliases}")


# ---- the scene -----------------------------------------------------------------------------------------------------------
W, H, MB = 64, 48, 4
DIFFUSE, METAL, GLASS = 0, 1, 2


def room_scene(pkg, resolution=(W, H), leading_spheres=False):
    """The camera inside a closed room of six diffuse radius-1000 spheres, a metal and a glass ball, and a small diffuse mesh.
    Every ray hits something, so no path ever leaves the compaction: a path's slot is its pixel at every bounce.  The mesh
    object comes first (bounce 0 opens with a traversal launch over one object: entry points per tile, ray generation's work
    list, the persistent launch's plan); leading_spheres puts two walls in front of it (k_spheres / k_list_flags open every
    bounce)."""
    glm = pkg.glmlite
    s = pkg.SceneDescription()
    big = 1000.0
    walls = [("floor", (0.0, -big - 1.0, 0.0), (0.73, 0.73, 0.73)), ("ceiling", (0.0, big + 2.0, 0.0), (0.9, 0.9, 0.8)),
             ("back", (0.0, 0.0, -big - 3.0), (0.7, 0.75, 0.7)), ("front", (0.0, 0.0, big + 2.0), (0.6, 0.6, 0.8)),
             ("left", (-big - 2.0, 0.0, 0.0), (0.65, 0.05, 0.05)), ("right", (big + 2.0, 0.0, 0.0), (0.12, 0.45, 0.15))]
    for name, _, albedo in walls:
        s.add_material(name, pkg.DiffuseMateral(albedo))
    s.add_material("metal", pkg.MetalMaterial((0.8, 0.6, 0.2), 0.3))
    s.add_material("glass", pkg.DielectricMaterial(1.5))
    s.add_material("mesh", pkg.DiffuseMateral((0.8, 0.8, 0.5)))
    mesh = s.add_mesh("ball", pkg.scenes.displaced_sphere_mesh(6, 12))

    def wall(k):
        s.add_object(pkg.Sphere((0, 0, 0), big), glm.translate(walls[k][1]), walls[k][0])

    if leading_spheres:
        wall(0)
        wall(1)
    s.add_object(mesh, glm.compose([glm.scale(0.9), glm.translate((0.0, -0.45, -1.6))]), "mesh")
    for k in range(2 if leading_spheres else 0, 6):
        wall(k)
    s.add_object(pkg.Sphere((0, 0, 0), 0.5), glm.translate((-1.05, -0.5, -1.4)), "metal")
    s.add_object(pkg.Sphere((0, 0, 0), 0.45), glm.translate((1.0, -0.55, -1.2)), "glass")
    s.camera = pkg.scenes._camera_from_look_at((0.0, 0.1, 1.5), (0.0, -0.3, -1.5), vfov_deg=60.0)
    s.resolution = tuple(resolution)
    return s


class Room:
    """The room at 64 x 48 with what the placing needs: the oracle's scene handle and the material kind under a jittered
    primary ray."""

    def __init__(self, pkg, orc, leading_spheres=False):
        from lit_ref import _primary, _rays
        self._primary, self._rays = _primary, _rays
        self.pkg, self.orc = pkg, orc
        self.scene = room_scene(pkg, (W, H), leading_spheres)
        self.flat = self.scene.build_scene()
        self.camera = self.scene.camera
        self.handle = orc.SceneHandle(self.flat)
        self.materials = np.asarray(self.flat.materials)

    def primary_kind(self, pixel, iteration):
        """material type of the closest hit of the primary ray the oracle generates for (pixel, iteration); -1: a miss"""
        o, d, tmin, _ = self._primary(self.orc, self.camera, W, H, [pixel], iteration)
        recs, hit = self.orc.intersect_rays(self.flat, self._rays(o, tmin, d), scene_handle=self.handle)
        return int(self.materials["type"][int(recs["material_id"][0])]) if hit[0] else -1

    def replay(self, pixel, iteration, bounces):
        """The path of `pixel` alone, the oracle's pieces (lit_ref): per bounce 0 .. bounces - 1 the material type it hits and
        the draws its material makes, as (bit pattern, ...).  Valid as the streaming path of SLOT `pixel` while no path of the
        frame has left the compaction (the caller checks the oracle's live counts)."""
        import lit_ref
        lib = self.orc.lib()
        o, d, tmin, _ = self._primary(self.orc, self.camera, W, H, [pixel], iteration)
        color = np.ones((1, 3), dtype=np.float32)
        out = []
        for b in range(bounces):
            recs, hit = self.orc.intersect_rays(self.flat, self._rays(o, tmin, d), scene_handle=self.handle)
            if not hit[0]:
                break
            st = C.c_uint32(lib.orc_rng_seed(lib.orc_path_seed(pixel, iteration)))
            lib.orc_rng_discard(C.byref(st), b)
            draws = _Recorder(self.orc, [st.value])
            lit_ref.shade(self.orc, self.materials, o, d, tmin, recs, np.array([0]), draws, color)
            out.append((int(self.materials["type"][int(recs["material_id"][0])]), tuple(draws.seen)))
        return out


class _Recorder:
    def __init__(self, orc, states):
        from lit_ref import Draws
        self.inner = Draws(orc, states)
        self.seen = []

    def uniform(self, idx):
        u = self.inner.uniform(idx)
        self.seen += [int(x) for x in u.view(np.uint32)]
        return u


def oracle_draws(orc, pixel, iteration, count, xor=0):
    """(seed, [bit patterns of the first `count` draws]) of the oracle's generator for path_seed(pixel, iteration) ^ xor"""
    lib = orc.lib()
    seed = lib.orc_path_seed(pixel, iteration) ^ xor
    st = C.c_uint32(lib.orc_rng_seed(seed))
    return seed, [int(np.float32(lib.orc_rng_uniform(C.byref(st))).view(np.uint32)) for _ in range(count)]


ONE_BITS, ZERO_BITS, BELOW_ONE_BITS = 0x3F800000, 0x00000000, 0x3F7FFFFF


def frame_cases(room):
    """Every constructed frame case: dicts {name, pixel, iteration, seed, proof}; `proof` says what the oracle's generator
    yields there (asserted here: a case that misses its target raises).  Seeds and bounce-0 draws once per material kind under the
    primary ray; the jitter cases on the edges of the 8 x 8 beam tiles and of the frame; the draw pairs of bounces 1 and 2."""
    orc = room.orc
    every = list(range(W * H))
    cases = []

    def add(name, pixel, it, seed, proof):
        cases.append({"name": name, "pixel": pixel, "iteration": it, "seed": seed, "proof": proof})

    kinds = (("diffuse", DIFFUSE), ("metal", METAL), ("glass", GLASS))
    # the special seeds and their neighbours
    for s in SPECIAL_SEEDS + SEED_NEIGHBOURS:
        for kname, kind in kinds:
            p, it, _ = place([s], every, lambda p, it, kind=kind: room.primary_kind(p, it) == kind)
            got, _ = oracle_draws(orc, p, it, 0)
            assert got == s, (s, got)
            st = orc.lib().orc_rng_seed(got)
            assert st == seed_state(s)
            add(f"seed {s:#x} on {kname}", p, it, s, f"orc_path_seed = {got:#x}, state {st}")
    # the first two draws at an edge: the jitter, and at bounce 0 the material's u1 / u2
    for k in (1, 2):
        for vname, state in EDGE_STATES:
            want = uniform_bits(state)
            for kname, kind in kinds:
                # (the glass draws once, and only where it can refract: its u is draw 1; draw 2 is the jitter alone there)
                def makes_it(p, it, kind=kind, k=k, want=want):
                    path = room.replay(p, it, 1)
                    return len(path) == 1 and path[0][0] == kind and ((kind == GLASS and k == 2) or
                                                                      (len(path[0][1]) >= k and path[0][1][k - 1] == want))

                p, it, s = place(seeds_for_draw(state, k), every, makes_it)
                _, u = oracle_draws(orc, p, it, 2)
                assert u[k - 1] == want, (vname, k, u)
                add(f"draw {k} = {vname} on {kname}", p, it, s, f"orc_rng_uniform #{k} = {want:#010x}")
    # ... on the edges of a beam tile and of the frame
    xs, ys = np.arange(W * H) % W, np.arange(W * H) // W
    where = {(1, "0.0"): xs % 8 == 0, (1, "1.0f low end"): xs % 8 == 7, (1, "1.0f high end"): xs == W - 1,
             (1, "largest below 1"): (xs % 8 == 7) & (ys % 8 == 7),
             (2, "0.0"): ys % 8 == 0, (2, "1.0f low end"): ys % 8 == 7, (2, "1.0f high end"): ys == H - 1,
             (2, "largest below 1"): (xs % 8 == 0) & (ys % 8 == 0)}
    for k in (1, 2):
        for vname, state in EDGE_STATES:
            pixels = np.nonzero(where[(k, vname)])[0]
            p, it, s = place(seeds_for_draw(state, k), pixels)
            _, u = oracle_draws(orc, p, it, 2)
            assert u[k - 1] == uniform_bits(state)
            add(f"jitter {'xy'[k - 1]} = {vname} at pixel ({p % W}, {p // W})", p, it, s,
                f"orc_rng_uniform #{k} = {u[k - 1]:#010x}")
    # the draw pairs of bounces 1 and 2: discard(b), then the draws b + 1 and b + 2
    for b in (1, 2):
        for j in (1, 2):
            for vname, state in EDGE_STATES:
                want = uniform_bits(state)

                def makes_it(p, it, b=b, j=j, want=want):
                    path = room.replay(p, it, b + 1)
                    return len(path) == b + 1 and len(path[b][1]) >= j and path[b][1][j - 1] == want

                p, it, s = place(seeds_for_draw(state, b + j), every, makes_it)
                add(f"bounce {b} draw {j} = {vname}", p, it, s, f"slot {p} alive at bounce {b}, its draw {j} there = {want:#010x}")
    return cases


def jitter_and_seed_cases(cases):
    """the cases that mean the same under the megakernel (one generator per pixel: seed, jitter)"""
    return [c for c in cases if not c["name"].startswith("bounce")]


# ---- the generator's self-test (ptc_check_rng on the host, ptc_selftest_rng on the device) -----------------------------------
BIG_DISCARDS = (2**20, 2**31 - 2, 2**32 - 1)
SWEEP = 2**20


def kat_inputs(cases):
    """per record of rng_kat.json two inputs: (seed, discard) itself -- its raw values 1, 2 and uniform draws 3, 4 -- and the
    seed two steps before the state after the discard, so that the raw values and draws 1, 2 of the record come out as words
    2 .. 5 as well"""
    out = []
    for c in cases:
        out.append((c["seed"], c["discard"]))
        out.append((advance(advance(seed_state(c["seed"]), c["discard"]), M31 - 1 - 2), 0))   # (A^(m-1) = 1: m - 3 steps on = 2 back)
    return out


def rng_inputs(kat_cases):
    """(seeds, discards) of the self-test, uint32: the known answers; the special seeds and their neighbours under the discards
    0 .. 50 (the bounce loop's) and three large ones; every state whose uniform() is 0.0 or 1.0f and the neighbour on each side,
    as the third and as the fourth value after the seed (words 4 and 5), under both aliases of the seed; a sweep of 2^20 states
    over [1, m - 1] with the discards 0 .. 50 in turn."""
    pairs = kat_inputs(kat_cases)
    for s in (0, 1, M31 - 1, M31, M31 + 1, 2 * M31 - 1, 2 * M31, 2**32 - 1):
        pairs += [(s, z) for z in list(range(51)) + list(BIG_DISCARDS)]
    edge = [STATE_ZERO, STATE_ZERO + 1] + list(range(STATE_BELOW_ONE - 1, STATE_ONE_HI + 1))   # (m - 1's upper neighbour is 1 again)
    for x in edge:
        for k in (3, 4):
            for z in (0, 7):
                pairs += [(s, z) for s in seeds_for_draw(x, k + z)]
    fixed = len(pairs)
    sweep = 1 + (np.arange(SWEEP, dtype=np.uint64) * np.uint64(M31 - 2)) // np.uint64(SWEEP - 1)
    seeds = np.concatenate([np.array([p[0] for p in pairs], dtype=np.uint64), sweep]).astype(np.uint32)
    discards = np.concatenate([np.array([p[1] for p in pairs], dtype=np.uint64), np.arange(SWEEP, dtype=np.uint64) % 51]).astype(np.uint32)
    assert int(sweep[0]) == 1 and int(sweep[-1]) == M31 - 1
    return seeds, discards, fixed


def big_integer_words(seeds, discards):
    """reference (c): the six words in exact integer arithmetic (numpy uint64: every product is below 2^62), the uniform
    mapping through one rounding to binary32"""
    m = np.uint64(M31)
    x0 = seeds.astype(np.uint64) % m
    x0[x0 == 0] = 1
    mult = np.array([pow(A, int(z), M31) for z in np.unique(discards)], dtype=np.uint64)[np.searchsorted(np.unique(discards), discards)]
    x1 = x0 * mult % m
    r = [x1]
    for _ in range(4):
        r.append(r[-1] * np.uint64(A) % m)
    uni = [((v.astype(np.int64) - 1).astype(np.float64).astype(np.float32) / np.float32(2147483648.0)).view(np.uint32) for v in r[3:5]]
    return np.stack([x0, x1, r[1], r[2], uni[0], uni[1]], axis=1).astype(np.uint32)


def oracle_words(orc, s, z):
    """reference (b): the six words from orc_rng_seed / orc_rng_discard / orc_rng_next / orc_rng_uniform"""
    lib = orc.lib()
    st = C.c_uint32(lib.orc_rng_seed(int(s)))
    out = [st.value]
    lib.orc_rng_discard(C.byref(st), int(z))
    out.append(st.value)
    out += [lib.orc_rng_next(C.byref(st)), lib.orc_rng_next(C.byref(st))]
    out += [int(np.float32(lib.orc_rng_uniform(C.byref(st))).view(np.uint32)) for _ in range(2)]
    return out


def check_rng_words(orc, kat_cases, seeds, discards, fixed, words):
    """`words` (uint32 [n, 6]) of the generator under test against the three references, bit for bit"""
    assert words.shape == (len(seeds), 6) and words.dtype == np.uint32
    # (a) rocThrust's answers: every number of every record
    assert len(kat_cases) >= 50
    for k, c in enumerate(kat_cases):
        a, b = words[2 * k], words[2 * k + 1]
        assert [int(a[2]), int(a[3])] == c["raw"][:2] and [int(a[4]), int(a[5])] == c["uniform_bits"][2:], c
        assert int(b[3]) == int(a[1]) and int(b[3]) * A % M31 == c["raw"][0] and [int(b[4]), int(b[5])] == c["uniform_bits"][:2], c
        assert advance(int(a[3]), 1) == c["raw"][2] and advance(int(a[3]), 2) == c["raw"][3]
    # (c) the big-integer restatement: everything
    want = big_integer_words(seeds, discards)
    bad = np.nonzero(np.any(words != want, axis=1))[0]
    assert len(bad) == 0, [(int(seeds[i]), int(discards[i]), words[i].tolist(), want[i].tolist()) for i in bad[:5]]
    # (b) the oracle's generator: every constructed input and every 16th state of the sweep
    for i in list(range(fixed)) + list(range(fixed, len(seeds), 16)):
        assert words[i].tolist() == oracle_words(orc, seeds[i], discards[i]), (int(seeds[i]), int(discards[i]))
    # ... and the edges are among them: exactly 0.0, and exactly 1.0f from each of its 62 states, as word 4 and as word 5
    for k in (4, 5):
        assert int((words[:fixed, k] == ZERO_BITS).sum()) >= 4 and int((words[:fixed, k] == ONE_BITS).sum()) >= 4 * 62
        assert int((words[:fixed, k] == BELOW_ONE_BITS).sum()) >= 4
    return want


# ---- direct-light queries: seed = path_seed(point index, sample_index) ^ XOR_LIGHT, draws u0 (the lamp), u1, u2 (the point) ---
LIGHT_POINTS = 256


def light_cases(orc):
    """dicts {name, point, sample_index, seed, draw, bits}: the four special seeds, and each of the three draws at 0.0, at both
    ends of the 1.0f range and at the largest value below 1 -- every case on a point of its own"""
    cases = []
    points = list(range(3, LIGHT_POINTS, 7))

    def add(name, seeds, draw, bits):
        p, si, s = place(seeds, points[len(cases):], xor=XOR_LIGHT, limit=2**32)   # (sample_index is a free 32-bit argument)
        cases.append({"name": name, "point": p, "sample_index": si, "seed": s, "draw": draw, "bits": bits})

    for s in SPECIAL_SEEDS:
        add(f"light seed {s:#x}", [s], 0, None)
    for k in (1, 2, 3):
        for vname, state in EDGE_STATES:
            add(f"light u{k - 1} = {vname}", seeds_for_draw(state, k), k, uniform_bits(state))
    return cases


def cases_document(cases_mesh_first, cases_walls_first, lights):
    """tests/seed_cases.md: every constructed case with where it lands and what the oracle's generator yields there"""
    out = ["# Constructed seed cases", "",
           "Generated by `tests/seed_cases.py` (`cases_document`); `tests/test_rng_edges_cpu.py` checks that it is current.",
           "Frames are 64 x 48, pixel = x + 64 y; `max_iterations = iteration + 1`.", ""]
    for title, cases in (("Frame cases, the mesh object first", cases_mesh_first), ("Frame cases, two walls in front of the mesh", cases_walls_first)):
        out += [f"## {title}", "", "| case | pixel | iteration | path_seed | CPU proof (the oracle's generator) |", "|---|---|---|---|---|"]
        out += [f"| {c['name']} | {c['pixel']} | {c['iteration']} | {c['seed']:#010x} | {c['proof']} |" for c in cases]
        out.append("")
    out += ["## Direct-light cases (256 points; seed = path_seed(point, sample_index) ^ 0x4c495445)", "",
            "| case | point | sample_index | seed | draw at the edge |", "|---|---|---|---|---|"]
    out += [f"| {c['name']} | {c['point']} | {c['sample_index']} | {c['seed']:#010x} | "
            f"{'state after the seed = 1' if not c['draw'] else 'orc_rng_uniform #%d = %#010x' % (c['draw'], c['bits'])} |" for c in lights]
    return "\n".join(out) + "\n"
