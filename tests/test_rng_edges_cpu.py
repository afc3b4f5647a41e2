"""The per-path generator (csrc/pt_rng.hpp) at its edges, without a GPU: ptc_check_rng runs the header the kernels run, on the
host, and is compared bit for bit with rocThrust's recorded answers (tests/golden/rng_kat.json), with the oracle's generator and
with a big-integer restatement (tests/seed_cases.py) -- on the seeds Minstd::seed treats specially, on every state whose
uniform() is exactly 0.0 or 1.0f, under the bounce loop's discards and three large ones, and over a sweep of 2^20 states.
Also here: the self-check of tests/seed_cases.py (the inverse of hash32, the placing of a seed on a pixel) and the proof, through
the oracle's own generator, that every constructed frame and direct-light case of the GPU tests meets its target."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest

import direct_ref as D
import seed_cases as sc
from ref_f32 import stream_draws


@pytest.fixture(scope="module")
def kat(golden_dir):
    return json.load(open(os.path.join(golden_dir, "rng_kat.json")))["cases"]


def test_host_generator_against_the_three_references(pkg, orc, kat):
    seeds, discards, fixed = sc.rng_inputs(kat)
    words = np.zeros((len(seeds), 6), dtype=np.uint32)
    assert pkg.lib().ptc_check_rng(seeds.ctypes.data, discards.ctypes.data, len(seeds), words.ctypes.data) == 0
    sc.check_rng_words(orc, kat, seeds, discards, fixed, words)
    assert fixed > 1000 and len(seeds) == fixed + sc.SWEEP
    lib = pkg.lib()
    assert lib.ptc_check_rng(None, None, 0, None) == 0 and lib.ptc_check_rng(None, discards.ctypes.data, 1, words.ctypes.data) == pkg._capi.PTC_ERR_INVALID


def test_edge_states_of_the_uniform_mapping():
    """The big-integer restatement's own edges, from the number formats: 0.0 from one state, 1.0f from 62, the largest
    binary32 below 1 just beneath them."""
    m = sc.M31
    assert sc.uniform_bits(1) == sc.ZERO_BITS and sc.uniform_bits(2) == int(np.float32(2.0**-31).view(np.uint32))
    one = [x for x in range(m - 200, m) if sc.uniform_bits(x) == sc.ONE_BITS]
    assert one == list(range(sc.STATE_ONE_LO, sc.STATE_ONE_HI + 1)) and len(one) == 62
    assert sc.uniform_bits(sc.STATE_BELOW_ONE) == sc.BELOW_ONE_BITS
    assert [sc.seed_state(s) for s in sc.SPECIAL_SEEDS] == [1, 1, 1, 1]
    assert [sc.seed_state(s) for s in sc.SEED_NEIGHBOURS] == [1, m - 1, 1]


def test_hash_inverse_and_placing(orc):
    L = orc.lib()
    assert sc.path_seed(0, 0) == 0x2B4F8145 == L.orc_path_seed(0, 0)
    rnd = random.Random(1)
    for _ in range(20000):
        x = rnd.getrandbits(32)
        assert sc.hash32_inv(sc.hash32(x)) == x and sc.hash32(sc.hash32_inv(x)) == x
    for x in (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 12345):
        assert sc.hash32(x) == L.orc_hash(x)
    # a round trip through orc_path_seed: any wanted seed, on some pixel of the frame, at an iteration below 2^31
    pixels = list(range(sc.W * sc.H))
    for target in list(sc.SPECIAL_SEEDS) + [rnd.getrandbits(32) for _ in range(200)]:
        p, it, s = sc.place([target], pixels)
        assert s == target and 0 <= it < 2**31 and L.orc_path_seed(p, it) == target
        p, it, s = sc.place([target], pixels[100:], xor=sc.XOR_LIGHT)
        assert L.orc_path_seed(p, it) ^ sc.XOR_LIGHT == target and p >= 100
    with pytest.raises(AssertionError):
        sc.place([5], [])
    # the k-th draw after each of seeds_for_draw(x, k) returns x
    for x in (1, sc.STATE_ONE_LO, sc.STATE_ONE_HI, 77):
        for k in (1, 2, 9):
            for s in sc.seeds_for_draw(x, k):
                st = C.c_uint32(L.orc_rng_seed(s))
                assert [L.orc_rng_next(C.byref(st)) for _ in range(k)][-1] == x


def test_every_frame_case_meets_its_target(pkg, orc):
    """frame_cases asserts each case against the oracle's generator while it builds the list; here: the list is complete, and
    for the cases of bounces 1 and 2 the oracle's live counts say that no path has left the compaction before that bounce, so
    the slot whose draws were replayed is the pixel's."""
    room = sc.Room(pkg, orc)
    cases = sc.frame_cases(room)
    names = [c["name"] for c in cases]
    assert len(cases) == 7 * 3 + 8 * 3 + 8 + 16 and len(set(names)) == len(names)
    for c in cases:
        assert 0 <= c["iteration"] < 2**31 and orc.lib().orc_path_seed(c["pixel"], c["iteration"]) == c["seed"], c
        if c["name"].startswith("bounce"):
            ref = orc.render_streaming(room.flat, room.camera, sc.W, sc.H, c["iteration"], 1, sc.MB, scene_handle=room.handle)
            assert ref["live"][0].tolist() == [sc.W * sc.H] * sc.MB, c
    assert len(sc.jitter_and_seed_cases(cases)) == 7 * 3 + 8 * 3 + 8
    # tests/seed_cases.md lists every case as it is placed today
    walls_first = sc.frame_cases(sc.Room(pkg, orc, leading_spheres=True))
    here = os.path.dirname(os.path.abspath(__file__))
    assert open(os.path.join(here, "seed_cases.md")).read() == sc.cases_document(cases, walls_first, sc.light_cases(orc))


def test_every_direct_light_case_meets_its_target(orc):
    cases = sc.light_cases(orc)
    assert len(cases) == 4 + 3 * 4
    for c in cases:
        u = stream_draws(orc, [c["point"]], c["sample_index"], D.SEED_XOR, 0, 3)[0]
        seed = orc.lib().orc_path_seed(c["point"], c["sample_index"]) ^ D.SEED_XOR
        assert seed == c["seed"] and 0 <= c["sample_index"] < 2**32, c
        if c["draw"]:
            assert int(np.float32(u[c["draw"] - 1]).view(np.uint32)) == c["bits"], c
        else:
            assert orc.lib().orc_rng_seed(seed) == 1, c
