"""The numpy restatements the bit-exact GPU tests trust (tests/lit_ref.py: the render loops with every option; tests/direct_ref.py:
the light sample) against tests/golden/loop_ref.npz, array for array and bit for bit.  The file was written when each loop still
had one copy per feature (plain, direct lighting, roulette), by those copies; the generator (tests/golden/make_golden.py,
loop_ref_cases) lists the cases and asserts that each does what it is there for.  A change to a rule of the restatement changes
this file's arrays on purpose, and then says so in the diff of the fixture."""
import importlib.util
import os

import numpy as np
import pytest


@pytest.fixture(scope="module")
def cases(golden_dir):
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(golden_dir, "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.loop_ref_cases()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def test_every_array_of_the_file_is_reproduced(cases, golden_dir):
    want = np.load(os.path.join(golden_dir, "loop_ref.npz"))
    assert sorted(cases) == sorted(want.files)
    assert len(want.files) == 12 * 10 + 7 * 8 + 4  # megakernel cases x their keys, streaming cases x theirs, the sample's four
    for name in want.files:
        got, ref = np.asarray(cases[name]), want[name]
        assert got.dtype == ref.dtype and got.shape == ref.shape, (name, got.dtype, ref.dtype, got.shape, ref.shape)
        assert np.array_equal(_bits(got), _bits(ref)), (name, int(np.sum(_bits(got) != _bits(ref))))


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
