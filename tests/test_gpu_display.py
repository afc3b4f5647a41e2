"""The display transform on the device: k_meter / k_meter_level / k_tonemap through ptc_tonemap_buffer on hostile
buffers, and through the presents of rendered frames, against tests/display_ref.py -- histogram, counts, level, scale and the mapped
floats bit for bit; RGBA8 within 1 LSB of the oracle's preview of those mapped floats (powf comes from different math libraries on the
two sides: the criterion of tests/test_gpu_parity.py for the reference display), alpha 255."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import display_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_PT = os.path.join(ROOT, "cuda-path-tracer_amd", "host", "hip_pt")
W, H, ITERS, MB = 64, 48, 3, 5
# one pass of the capped meter grid: kMeterMaxBlocks workgroups of kMeterBlock pixels (csrc/pt_device.hpp); one odd size just above it
ONE_PASS = 2048 * 256
SIZES = [1, 63, 64, 65, 255, 257, 999, 3015, ONE_PASS + 1]


def displays(pkg):
    """every curve under manual and histogram metering, none of them the reference display"""
    D = pkg.Display
    return {"clamp_manual": D(curve=0, exposure=2.0), "reinhard_manual": D(curve=1, exposure=0.7, white=3.0), "aces_manual": D(curve=2, exposure=1.0),
            "clamp_metered": D(curve=0, metering=1), "reinhard_metered": D(curve=1, metering=1, key=0.36, white=2.5, low_permille=100, high_permille=900),
            "aces_metered": D(curve=2, metering=1, exposure=1.5, low_permille=0, high_permille=1000)}


@pytest.fixture(scope="module")
def bare(pkg):
    """a context without a scene or a frame: all ptc_tonemap_buffer needs"""
    with pkg.PathTracer(device=0) as pt:
        yield pt


def one_bin_image(n):
    img = np.full((n, 3), 1.4, dtype=np.float32)
    img[::2] *= np.float32(1.03)
    return img


_IMAGES = {}


def image(name):
    """name -> [n, 3] float32, built once: a size = a log-normal frame of that many pixels with the hostile values laid over its
    start (as many as fit); "hostile" = those alone; "one_bin" = every pixel in bin 131, the worst contention on the LDS histograms"""
    if name not in _IMAGES:
        if name == "hostile":
            img = ref.hostile_pixels()
        elif name == "one_bin":
            img = one_bin_image(70001)
        else:
            n = int(name)
            img = ref.lognormal_image(n, seed=n)
            hostile = ref.hostile_pixels()
            k = min(n // 2, len(hostile))
            img[:k] = hostile[:: max(1, len(hostile) // max(k, 1))][:k]
        img.setflags(write=False)
        _IMAGES[name] = img
    return _IMAGES[name]


_WANT = {}


def want_for(orc, name, dname, d):
    """the restatement's (mapped, info, rgba) of an image under a display, computed once"""
    key = (name, dname)
    if key not in _WANT:
        img = image(name)
        mapped, info = ref.show(img, d)
        _WANT[key] = (mapped, info, orc.preview(mapped, len(img), 1, 0).reshape(-1, 4))
    return _WANT[key]


def check_shown(got_rgba, got_mapped, got_info, want, what):
    mapped, info, rgba = want
    assert ref.same_info(got_info, info), (what, {k: v for k, v in got_info.items() if k != "histogram"},
                                           {k: v for k, v in info.items() if k != "histogram"})
    if got_mapped is not None:
        a, b = np.ascontiguousarray(got_mapped).view(np.uint32).reshape(-1, 3), np.ascontiguousarray(mapped).view(np.uint32).reshape(-1, 3)
        assert np.array_equal(a, b), (what, int(np.sum(a != b)), np.argwhere(a != b)[:4].tolist())
    got_rgba = got_rgba.reshape(-1, 4)
    assert np.all(got_rgba[:, 3] == 255), what
    assert np.max(np.abs(got_rgba.astype(int) - rgba.astype(int))) <= 1, what


def with_alpha(img):
    """four floats a pixel; the fourth is never read (NaN here)"""
    return np.ascontiguousarray(np.concatenate([img, np.full((len(img), 1), np.nan, dtype=np.float32)], axis=1))


# ---- 1. the kernels on a caller's buffer ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [str(n) for n in SIZES] + ["one_bin", "hostile"])
def test_tonemap_buffer_against_the_restatement(pkg, orc, bare, name):
    """Both pixel layouts, host pointers: every display.  Counts are exact on the all-one-bin image, where every lane of a wavefront
    adds to one LDS word, and on a frame one pixel longer than a pass of the capped grid, where the stride loop's second round is one
    thread's."""
    img = image(name)
    for dname, d in displays(pkg).items():
        bare.display = d
        want = want_for(orc, name, dname, d)
        for src in (img, with_alpha(img)):
            rgba, mapped, info = bare.tonemap_buffer(src, want_mapped=True)
            check_shown(rgba, mapped, info, want, (name, dname, src.shape[1]))
    if name == "one_bin":
        assert info["histogram"][131] == len(img) == info["counted"] and info["level_bin"] == 131
    if name == "hostile":
        assert info["below"] > 0 and info["rejected"] > 0 and info["histogram"][255] > 0


@pytest.mark.parametrize("name", ["65", "3015", str(ONE_PASS + 1), "hostile"])
def test_tonemap_buffer_on_device_pointers(pkg, orc, bare, name):
    """... and device pointers (torch tensors), both layouts, with and without the mapped floats"""
    import torch
    img = image(name)
    n = len(img)
    for dname in ("aces_metered", "reinhard_manual"):
        d = displays(pkg)[dname]
        bare.display = d
        want = want_for(orc, name, dname, d)
        for src in (img, with_alpha(img)):
            t = torch.from_numpy(np.array(src)).cuda()
            rgba = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
            mapped = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            info = bare.tonemap_buffer_dev(t.data_ptr(), src.shape[1], n, rgba.data_ptr(), mapped.data_ptr())
            check_shown(rgba.cpu().numpy(), mapped.cpu().numpy(), info, want, (name, dname, src.shape[1], "device"))
            rgba2 = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            info2 = bare.tonemap_buffer_dev(t.data_ptr(), src.shape[1], n, rgba2.data_ptr())
            assert ref.same_info(info2, info) and torch.equal(rgba2, rgba)
    with pytest.raises(pkg.PtcError) as e:  # a float4 source is read sixteen bytes at a time
        bare.tonemap_buffer_dev(t.data_ptr() + 4, 4, n - 1, rgba.data_ptr())
    assert e.value.code == pkg._capi.PTC_ERR_INVALID and "16-byte aligned" in str(e.value)


def test_consecutive_calls_give_the_same_info(pkg, orc, bare):
    """The accumulation words are zero again after every metered call: two calls in a row, a metered call after a manual one and
    the other way round, on two images of different histograms, give what a first call gives."""
    D = displays(pkg)
    a, b = image("3015"), image("one_bin")
    first = {}
    for order in (("aces_metered", a), ("aces_metered", a), ("clamp_manual", a), ("aces_metered", b), ("reinhard_manual", b),
                  ("aces_metered", a), ("clamp_metered", b), ("clamp_metered", b), ("clamp_manual", a), ("aces_metered", b)):
        dname, img = order
        bare.display = D[dname]
        rgba, mapped, info = bare.tonemap_buffer(img, want_mapped=True)
        key = (dname, len(img))
        check_shown(rgba, mapped, info, want_for(orc, "3015" if img is a else "one_bin", dname, D[dname]), order[0])
        if key in first:
            assert ref.same_info(info, first[key][0]) and np.array_equal(rgba, first[key][1]), key
        first[key] = (info, rgba)


# ---- 2. through the render -------------------------------------------------------------------------------------------------------

def _scene(pkg, name):
    if name == "cornell_lit":
        scene = pkg.scenes.cornell_lit(resolution=(W, H), with_mesh=True)
        return scene, scene.build_scene(), None
    scene = pkg.json_parser.scene_from_json(os.path.join(ROOT, "assets", "scenes", "spheres_sun.json"))
    return scene, scene.build_scene(), scene.environment


def _rendered(pkg, name, mega, iters=ITERS):
    scene, flat, env = _scene(pkg, name)
    pt = pkg.PathTracer(device=0, max_bounces=MB)
    if mega:
        pt.current_gpu_method = pkg.GPUMethod.megakernel
        pt.direct_light = name == "cornell_lit"
        pt.environment_light = env is not None
    pt.environment = env
    pt.create_buffers((W, H), flat)
    pt.max_iterations = iters
    for _ in range(iters):
        pt.path_trace(scene.camera)
    return pt, scene


def _same_display(a, b):
    """two Displays as the library holds them: the floats in binary32"""
    ints = ("curve", "metering", "low_permille", "high_permille")
    floats = ("exposure", "key", "white")
    return all(int(getattr(a, k)) == int(getattr(b, k)) for k in ints) and all(np.float32(getattr(a, k)) == np.float32(getattr(b, k)) for k in floats)


def _state(pt):
    out = {k: pt.download(k).copy() for k in ("color", "normal", "depth", "final")}
    out["stats"] = pt.stats()
    return out


def _same_state(a, b, what):
    assert a["stats"] == b["stats"], what
    for k in ("color", "normal", "depth", "final"):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (what, k)


@pytest.mark.parametrize("mega", [True, False], ids=["megakernel", "streaming"])
@pytest.mark.parametrize("name", ["cornell_lit", "spheres_sun"])
def test_presents_of_a_rendered_frame(pkg, orc, name, mega):
    """send_to_preview of FINAL and COLOR under every display against the restatement applied to the download of the same buffer,
    exposure_info() against the restatement's; after denoise() FINAL meters the denoised buffer; NORMAL and DEPTH are the bytes
    they are under the reference display; and no present moves the statistics or the framebuffers."""
    T = pkg.DisplayBufferType
    pt, scene = _rendered(pkg, name, mega)
    with pt:
        plain = {d: pt.send_to_preview(display_type=d) for d in T}
        before = _state(pt)
        assert before["stats"]["rays_total"] > 0
        for stage in ("traced", "denoised"):
            if stage == "denoised":
                pt.denoise()
                before = _state(pt)
                assert not np.array_equal(before["final"], before["color"])
            for dname, d in displays(pkg).items():
                pt.display = d
                for view, buf in ((T.final, "final"), (T.color, "color")):
                    got = pt.send_to_preview(display_type=view)
                    mapped, info = ref.show(before[buf].reshape(-1, 3), d)
                    want = (None, info, orc.preview(mapped, W, H, 0).reshape(-1, 4))
                    check_shown(got, None, pt.exposure_info(), want, (name, mega, stage, dname, buf))
                    if d.metering:
                        assert info["counted"] + info["below"] + info["rejected"] == W * H and info["level_bin"] >= 0
                for view in (T.normal, T.depth):
                    assert np.array_equal(pt.send_to_preview(display_type=view), plain[view]), (stage, dname, view)
                _same_state(_state(pt), before, (name, mega, stage, dname))
        pt.display = pkg.Display()
        assert np.array_equal(pt.send_to_preview(display_type=T.color), plain[T.color])


def test_gathered_present_equals_the_present(pkg):
    """One context that owns the whole frame, no peers: under every display a gathered present is the present of the same buffer
    (FINAL gathers the accumulated colour: include/ptcore.h), and meters the same."""
    T = pkg.DisplayBufferType
    pt, _ = _rendered(pkg, "cornell_lit", False)
    with pt:
        pt.denoise()
        before = _state(pt)
        for dname, d in list(displays(pkg).items()) + [("reference", pkg.Display())]:
            pt.display = d
            for gathered, shown in ((T.color, T.color), (T.final, T.color), (T.normal, T.normal), (T.depth, T.depth)):
                want = pt.send_to_preview(display_type=shown)
                want_info = pt.exposure_info() if dname != "reference" else None
                assert np.array_equal(pt.gather_present(gathered), want), (dname, gathered)
                if want_info is not None:
                    assert ref.same_info(pt.exposure_info(), want_info), (dname, gathered)
        _same_state(_state(pt), before, "gathered presents")


def test_the_display_is_the_contexts_and_leaves_no_trace(pkg):
    """A display and then the reference display again: the bytes of a context that never had one.  The display survives resize_image
    and create_buffers; a refused one leaves the display that was set in place, and the refusal names the field."""
    T = pkg.DisplayBufferType
    aces = displays(pkg)["aces_metered"]
    never, scene = _rendered(pkg, "cornell_lit", False)
    with never:
        want = {d: never.send_to_preview(display_type=d) for d in T}
        with pytest.raises(pkg.PtcError) as e:
            never.exposure_info()
        assert e.value.code == pkg._capi.PTC_ERR_INVALID
    pt, scene = _rendered(pkg, "cornell_lit", False)
    with pt:
        assert _same_display(pt.display, pkg.Display())
        pt.display = aces
        shown = pt.send_to_preview()
        assert not np.array_equal(shown, want[T.final])
        pt.display = pkg.Display()
        for d in T:
            assert np.array_equal(pt.send_to_preview(display_type=d), want[d]), d
        # refusals
        pt.display = aces
        for bad, field in ((pkg.Display(exposure=float("nan")), "exposure"), (pkg.Display(exposure=-2.0), "exposure"),
                           (pkg.Display(key=float("inf")), "key"), (pkg.Display(white=0.0), "white"),
                           (pkg.Display(low_permille=900, high_permille=100), "low_permille"), (pkg.Display(high_permille=2000), "high_permille"),
                           (pkg.Display(curve=7), "curve")):
            with pytest.raises(pkg.PtcError) as e:
                pt._check(pt._lib.ptc_set_display(pt._ctx, C.byref(bad.to_c())))
            assert e.value.code == pkg._capi.PTC_ERR_INVALID and field in str(e.value), (field, str(e.value))
            assert _same_display(pt.display, aces)
        assert np.array_equal(pt.send_to_preview(), shown)
        # the display outlives the frame and the scene
        pt.resize_image((40, 30))
        assert pt.display.curve == aces.curve and pt.display.metering == 1
        pt.create_buffers((W, H), scene.build_scene())
        assert pt.display.curve == aces.curve and pt.display.metering == 1
        pt.restart()
        pt.max_iterations = ITERS
        for _ in range(ITERS):
            pt.path_trace(scene.camera)
        assert np.array_equal(pt.send_to_preview(), shown)


def test_tonemap_buffer_moves_nothing(pkg, bare):
    """ptc_tonemap_buffer on a context with a rendered frame: statistics, live counts and framebuffers stay, and so does
    exposure_info(), which speaks of presents."""
    pt, _ = _rendered(pkg, "spheres_sun", True)
    with pt:
        pt.display = displays(pkg)["reinhard_metered"]
        pt.send_to_preview()
        info = pt.exposure_info()
        before = _state(pt)
        for name in ("999", "one_bin"):
            pt.tonemap_buffer(image(name), want_mapped=True)
            pt.tonemap_buffer(with_alpha(image(name)))
        _same_state(_state(pt), before, "tonemap_buffer")
        assert ref.same_info(pt.exposure_info(), info)


# ---- 3. the command line ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("gpus", [1, 2])
@pytest.mark.parametrize("flags,display", [(["--tonemap", "aces", "--auto-exposure", "--exposure", "0.5"], dict(curve=2, metering=1, exposure=2.0 ** 0.5)),
                                           (["--tonemap", "reinhard", "--white", "2.5", "--exposure", "-1"], dict(curve=1, white=2.5, exposure=0.5)),
                                           (["--auto-exposure", "--key", "0.3"], dict(metering=1, key=0.3))],
                         ids=["aces_auto", "reinhard_manual", "clamp_auto"])
def test_hip_pt_shows_through_the_display(pkg, orc, tmp_path, gpus, flags, display):
    """hip_pt -o with the display's flags, in one process and over two ranks (the root meters the whole gathered frame): the PNG is
    the restatement of the float colour buffer the same run dumps, within 1 LSB; --exposure is in stops."""
    from PIL import Image
    if not os.path.exists(HIP_PT):
        subprocess.run(["make"], cwd=os.path.dirname(HIP_PT), check=True, stdout=subprocess.DEVNULL)
    out, raw = tmp_path / "out.png", tmp_path / "out.raw"
    cmd = [HIP_PT, "scenes/spheres_sun.json", "-o", str(out), "--spp", "2", "--max-bounces", "4", "--dump-raw", str(raw)] + flags
    if gpus > 1:
        cmd += ["--gpus", str(gpus)]
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    data = open(raw, "rb").read()
    assert data[:4] == b"PTRF"
    w, h, ch = struct.unpack_from("<III", data, 4)
    color = np.frombuffer(data, dtype="<f4", offset=16)[:3 * w * h].reshape(h * w, 3)
    d = pkg.Display(**display)
    mapped, info = ref.show(color, d)
    want = orc.preview(mapped, w, h, 0)
    got = np.array(Image.open(out))
    assert got.shape == want.shape and np.all(got[..., 3] == 255)
    assert np.max(np.abs(got.astype(int) - want.astype(int))) <= 1
    assert not d.metering or info["counted"] > 0
