"""The sizing rule of ptc_resize without a GPU: ptc_check_frame_plan runs frame_plan (csrc/ptcore_ctx.hpp), the function
ptc_resize takes its slots from.  The rows are literal: each was worked out by hand from the rule -- frames capped at
24 GiB / (181 or 148 bytes x pixels) while the caller has not chosen them, batch = min(batch_frames, frames, 32), whole
batches only under the cap, ceil(frames / batch) batch slots, eight single-frame slots beside batches of more than one frame,
staging for more than one frame in flight -- so a change of the rule or of its divisors shows here, where no gigabyte is
allocated.  At 4K and above the cap decides; 16384 x 16384 ends at one unstaged frame."""
import ctypes as C

import pytest

AUTO, SET = 1, 0

# (width, height, frames_in_flight, auto / set, batch_frames, prefold) -> (frames, batch, big slots, single slots, staged)
ROWS = [
    ((64, 48, 64, AUTO, 32, 1), (64, 32, 2, 8, 1)),
    ((1920, 1080, 64, AUTO, 32, 1), (64, 32, 2, 8, 1)),
    ((2560, 1440, 64, AUTO, 32, 1), (32, 32, 1, 8, 1)),
    ((2560, 1440, 64, AUTO, 20, 1), (20, 20, 1, 8, 1)),
    ((3840, 2160, 64, AUTO, 32, 1), (17, 17, 1, 8, 1)),
    ((3840, 2160, 64, AUTO, 32, 0), (20, 20, 1, 8, 1)),
    ((7680, 4320, 64, AUTO, 32, 1), (4, 4, 1, 8, 1)),
    ((16384, 16384, 64, AUTO, 32, 1), (1, 1, 1, 0, 0)),
    ((64, 48, 1, SET, 32, 1), (1, 1, 1, 0, 0)),
    ((64, 48, 3, SET, 32, 1), (3, 3, 1, 8, 1)),
    ((64, 48, 5, SET, 2, 1), (5, 2, 3, 8, 1)),
    ((64, 48, 64, AUTO, 1, 1), (64, 1, 64, 0, 1)),
]


def _plan(pkg, args):
    out = pkg._capi.ptc_frame_plan()
    rc = pkg.lib().ptc_check_frame_plan(*args, C.byref(out))
    return rc, (out.frames, out.batch, out.big_slots, out.single_slots, out.staged)


@pytest.mark.parametrize("args,want", ROWS, ids=["%dx%d_f%d_%s_b%d_p%d" % (a[0], a[1], a[2], "auto" if a[3] else "set", a[4], a[5])
                                                 for a, _ in ROWS])
def test_frame_plan_rows(pkg, args, want):
    rc, got = _plan(pkg, args)
    assert rc == 0 and got == want, (args, got, want)


def test_frame_plan_refuses_what_resize_refuses(pkg):
    invalid = pkg._capi.PTC_ERR_INVALID
    assert pkg.lib().ptc_check_frame_plan(64, 48, 64, AUTO, 32, 1, None) == invalid
    for w, h in ((1, 5), (5, 1), (65536, 65536)):
        assert _plan(pkg, (w, h, 64, AUTO, 32, 1))[0] == invalid, (w, h)
    assert _plan(pkg, (46340, 46340, 64, AUTO, 32, 1)) == (0, (1, 1, 1, 0, 0))   # 2,147,395,600 pixels: the largest square ptc_resize takes
