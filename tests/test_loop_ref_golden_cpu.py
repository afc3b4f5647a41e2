"""The numpy restatements the bit-exact GPU tests trust (tests/loop_ref.py: the render loops with every option; tests/direct_ref.py:
the light sample) against tests/golden/loop_ref.npz and loop_ref_options.npz, array for array and bit for bit.  Each file was written
when a loop still had one copy per feature, by those copies -- loop_ref.npz for plain, direct lighting and roulette; loop_ref_options.npz
for environment light, MIS, smooth shading, textures, normal maps and the lens --; the generators (tests/golden/make_golden.py,
loop_ref_cases and loop_ref_option_cases) list the cases and assert that each does what it is there for.  A change to a rule of the
restatement changes these files' arrays on purpose, and then says so in the diff of the fixture."""
import importlib.util
import os

import numpy as np
import pytest


@pytest.fixture(scope="module")
def make_golden(golden_dir):
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(golden_dir, "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def cases(make_golden):
    return make_golden.loop_ref_cases()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _reproduced(cases, want):
    assert sorted(cases) == sorted(want.files)
    for name in want.files:
        got, ref = np.asarray(cases[name]), want[name]
        assert got.dtype == ref.dtype and got.shape == ref.shape, (name, got.dtype, ref.dtype, got.shape, ref.shape)
        assert np.array_equal(_bits(got), _bits(ref)), (name, int(np.sum(_bits(got) != _bits(ref))))


def test_every_array_of_the_file_is_reproduced(cases, golden_dir):
    want = np.load(os.path.join(golden_dir, "loop_ref.npz"))
    assert len(want.files) == 12 * 10 + 7 * 8 + 4  # megakernel cases x their keys, streaming cases x theirs, the sample's four
    _reproduced(cases, want)


def test_the_file_holds_what_its_cases_are_there_for(golden_dir):
    """The generator's own assertions, on the stored numbers: they held for the code that wrote the file."""
    f = np.load(os.path.join(golden_dir, "loop_ref.npz"))
    for name in {n.rsplit("_", 1)[0] for n in f.files if n.endswith("_ended")}:
        roulette = int(name.split("_r")[-1][0])
        assert (f[name + "_ended"].sum() > 0) == (roulette >= 1), name
        assert (f[name + "_played"] >= f[name + "_ended"] + f[name + "_skipped"]).all(), name
        if name.startswith("lit_megakernel_d1"):
            assert f[name + "_shadow_rays"] > f[name + "_unoccluded"] > 0, name
        if "_d0_" in name:
            assert (f[name + "_diffuse_hits"], f[name + "_shadow_rays"], f[name + "_unoccluded"]) == (0, 0, 0), name
    assert f["glass_lamp_megakernel_d1_r0_shadow_rays"] > 0 and f["glass_lamp_megakernel_d1_r0_unoccluded"] == 0
    assert f["no_lamp_megakernel_d1_r0_diffuse_hits"] == 0
    assert f["sample_sampled"].any() and not f["sample_sampled"].all()


def test_every_array_of_the_options_file_is_reproduced(make_golden, golden_dir):
    want = np.load(os.path.join(golden_dir, "loop_ref_options.npz"))
    assert len(want.files) == 21 * 23 + 2 * 8  # megakernel cases x (planes, 17 counters, tables), streaming cases x their keys
    assert os.path.getsize(os.path.join(golden_dir, "loop_ref_options.npz")) < 256 * 1024
    _reproduced(make_golden.loop_ref_option_cases(), want)


def test_the_options_file_holds_what_its_cases_are_there_for(make_golden, golden_dir):
    """The generator's own assertions, on the stored numbers: they held for the copies that wrote the file."""
    f = np.load(os.path.join(golden_dir, "loop_ref_options.npz"))
    mega = sorted(n[:-len("_bent")] for n in f.files if n.endswith("_bent"))
    assert len(mega) == 21
    for k in make_golden.LOOP_REF_COUNTERS:  # every counter moves somewhere (tex_fallbacks: only under the refused coordinate)
        assert any(f[f"{name}_{k}"] > 0 for name in mega), k
    assert [name for name in mega if f[name + "_tex_fallbacks"] > 0] == ["dm_all_nan"]
    for name in mega + ["dm_streaming", "lg_streaming"]:
        plays = "_all" in name and "roulette" not in name or name.endswith("_streaming")  # where roulette is on
        assert (f[name + "_ended"].sum() > 0) == plays, name
        assert (f[name + "_played"] >= f[name + "_ended"] + f[name + "_skipped"]).all(), name
    for name in mega:
        lamps = name.startswith("lg_") and ("_all" in name or name == "lg_mis_alone")  # where lamps are sampled
        assert (f[name + "_diffuse_hits"] > 0) == lamps, name
        if lamps:
            assert f[name + "_shadow_rays"] > f[name + "_unoccluded"] > 0, name
            assert (f[name + "_mis_emitter_hits"] > 0) == ("but_smooth_mis" not in name), name
    for name, moves in (("map_alone", ("bent", "kept", "absorbed")), ("texture_alone", ("lookups",)), ("smooth_alone", ("shading_normals", "absorbed")),
                        ("mis_alone", ("mis_misses",)), ("env_light_alone", ("env_unoccluded",))):
        for tag in make_golden.LOOP_REF_PAIRS:
            assert all(f[f"{tag}_{name}_{k}"] > 0 for k in moves), (tag, name)
    assert f["dm_map_alone_shading_normals"] == 0 and f["dm_map_alone_lookups"] == 0  # below the geometry without smooth shading
