"""The megakernel's instance rule without a GPU: ptc_check_megakernel_instance runs mega_rules::instance (csrc/pt_mega_rules.hpp), the
function launch_megakernel takes its kernel from.  TABLE is the rule as data, written from the specification and not derived from the
library: the first row whose condition holds names the kernel, the row's other facts fill its template arguments in order.  All 2^9
combinations of the nine facts are checked against it -- none is assumed to imply another -- and each of the 22 kernels must come out
of its own row and no other.  The roulette argument is decided by the same rule: `roulette` where some bounce plays, else INT_MAX."""
import itertools

import pytest

FACTS = ("direct", "env", "env_lit", "smooth", "textured", "weigh", "lens", "plays", "emitters")
INT_MAX = 2 ** 31 - 1

# (condition, kernel, the facts that are its template arguments)
TABLE = [
    (lambda f: f["textured"], "k_megakernel_tex", ("weigh", "smooth")),
    (lambda f: f["smooth"], "k_megakernel_smooth", ("weigh",)),
    (lambda f: f["weigh"], "k_megakernel_mis", ()),
    (lambda f: f["env_lit"], "k_megakernel_env_light", ()),
    (lambda f: f["env"], "k_megakernel_env", ("direct",)),
    (lambda f: f["direct"] and f["lens"], "k_megakernel_direct_lens", ("plays",)),
    (lambda f: f["direct"], "k_megakernel_direct", ("plays",)),
    (lambda f: f["lens"], "k_megakernel_lens", ("emitters", "plays")),
    (lambda f: True, "k_megakernel", ("emitters", "plays")),
]


def _expected(f):
    """-> (row of TABLE, the kernel's name as a profile prints it)"""
    for row, (cond, kernel, args) in enumerate(TABLE):
        if cond(f):
            return row, kernel + ("<%s>" % ", ".join("true" if f[a] else "false" for a in args) if args else "")
    raise AssertionError("the table is total")


def _all_facts():
    for bits in itertools.product((False, True), repeat=len(FACTS)):
        yield dict(zip(FACTS, bits))


def test_all_512_combinations(pkg):
    seen = {}
    for f in _all_facts():
        row, want = _expected(f)
        got, arg = pkg.check_megakernel_instance(roulette=2, max_bounces=8, **f)
        assert got == want, (f, got, want)
        assert arg == (2 if f["plays"] else INT_MAX), (f, arg)
        seen.setdefault(got, set()).add(row)
    assert len(seen) == 22, sorted(seen)
    assert all(len(rows) == 1 for rows in seen.values()), seen  # a name comes out of its own row alone
    assert sum(2 ** len(args) for _, _, args in TABLE) == 22 and {name.split("<")[0] for name in seen} == {k for _, k, _ in TABLE}


@pytest.mark.parametrize("roulette,want", [(0, INT_MAX), (1, 1), (2, 2), (3, INT_MAX), (4, INT_MAX)])
def test_the_roulette_argument_under_four_bounces(pkg, roulette, want):
    """max_bounces 4: bounces 1 and 2 can play (never the last); the library's own reading of `plays`, and it picks the instance too"""
    for emitters in (False, True):
        name, arg = pkg.check_megakernel_instance(emitters=emitters, roulette=roulette, max_bounces=4)
        plays = "true" if want != INT_MAX else "false"
        assert arg == want and name == "k_megakernel<%s, %s>" % ("true" if emitters else "false", plays), (roulette, name, arg)
    assert pkg.check_megakernel_instance(textured=True, roulette=roulette, max_bounces=4) == ("k_megakernel_tex<false, false>", want)


def test_refusals(pkg):
    import ctypes as C
    invalid = pkg._capi.PTC_ERR_INVALID
    fn = pkg.lib().ptc_check_megakernel_instance
    name, arg = C.create_string_buffer(64), C.c_int(0)
    assert fn(*([0] * 11), None, 64, C.byref(arg)) == invalid and fn(*([0] * 11), name, 64, None) == invalid
    assert fn(*([0] * 11), name, len("k_megakernel<false, false>"), C.byref(arg)) == invalid  # no room for the terminator
    assert fn(*([0] * 11), name, len("k_megakernel<false, false>") + 1, C.byref(arg)) == 0 and name.value == b"k_megakernel<false, false>"
