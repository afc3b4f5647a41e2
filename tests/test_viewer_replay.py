"""the interactive front-end, headless.  The viewer's camera controller
(interactive-app/first_person_camera_controller.cpp:12-100) restated in C++ (host/first_person_camera_controller.hpp)
and Python (camera_controller.py), and its frame loop (app.cpp:141-170) replayed from a script of viewer events by
`hip_pt --replay` and `viewer.replay`.  CPU: the controller's arithmetic against hand-computed values and the two
implementations against each other; GPU: the PNG sequence of the C++ replay equals the frames of the Python replay, and
every displayed frame equals what the CPU oracle renders for the viewer's state at that turn (`oracle_replay`: the
reference's PathTracer semantics -- iteration counter, max_iterations, restart, resize, method, denoise, display type,
path_tracer.cu:389-525 -- over orc_render_streaming / orc_render_megakernel / orc_denoise / orc_preview)."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_PT = os.path.join(ROOT, "cuda-path-tracer_amd", "host", "hip_pt")

SCRIPT = {"window": [64, 48], "iterations_per_frame": 2, "events": [
    {"frames": 2}, {"key": "W", "count": 3}, {"frames": 1}, {"mouse": [90, 0]}, {"key": "W"}, {"mouse": [0, 200]},
    {"key": "R", "count": 2}, {"speed": 0.5}, {"key": "A"}, {"mouse": [-400, -30]}, {"key": "S", "count": 2}, {"frames": 2},
    {"position": [1, 2, 3]}, {"key": "D"}, {"reset": True}, {"key": "F"}, {"key": "X"},
    {"display": "normal"}, {"frames": 1}, {"display": "final"}, {"denoise": True}, {"max_iterations": 3}, {"frames": 3},
    {"space": True}, {"method": "megakernel"}, {"frames": 1}, {"resize": [40, 40]}, {"method": "streaming"}, {"denoise": False},
    {"frames": 2}]}


# a third script: the filter size changed while denoising -- one pass, then steps 1..64 (k_denoise_lds<1..32> and the
# L1 / L2 kernel at step 64) -- and back to the default; a camera move and a resize in between
SCRIPT3 = {"window": [48, 36], "iterations_per_frame": 1, "events": [
    {"denoise": True}, {"frames": 1}, {"filter_size": 1}, {"frames": 2}, {"filter_size": 64}, {"frames": 1},
    {"key": "W"}, {"frames": 1}, {"resize": [33, 50]}, {"frames": 1}, {"filter_size": 10}, {"frames": 1},
    {"filter_size": 64}, {"denoise": False}, {"frames": 1}]}


def assert_denoised_frame(got, want, what):
    """a denoised frame on every pixel, the bottom rows included: within 1 LSB of the oracle's, opaque"""
    assert got.shape == want.shape, what
    diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert int(diff.max()) <= 1, (what, int(diff.max()))
    assert np.all(got[..., 3] == 255), what


def _ensure_cli():
    if not os.path.exists(HIP_PT):
        subprocess.run(["make"], cwd=os.path.dirname(HIP_PT), check=True, stdout=subprocess.DEVNULL)


def test_controller_arithmetic(pkg):
    cc = pkg.camera_controller
    cam = pkg.Camera(position=(0.0, 0.0, 0.0), rotation=(1.0, 0.0, 0.0, 0.0), vfov=1.0)
    c = cc.FirstPersonCameraController(cam)
    assert c.yaw == 0 and c.pitch == 0 and np.isclose(c.speed, 0.1)
    # identity: W = -z, S = +z, R = +y, F = -y, A = +x, D = -x (the reference's own signs, cpp:58-76)
    for key, want in (("W", (0, 0, -0.1)), ("S", (0, 0, 0)), ("R", (0, 0.1, 0)), ("F", (0, 0, 0)), ("A", (0.1, 0, 0)), ("D", (0, 0, 0))):
        assert c.on_key_press(key)
        assert np.allclose(cam.position, want, atol=1e-7), key
    assert not c.on_key_press("X") and not c.on_key_press(" ")
    # a quarter turn of yaw: forward is now -x; glm::yawPitchRoll = Ry(yaw) * Rx(pitch)
    c.on_mouse_move(np.pi / 2, 0.0)
    assert np.isclose(c.yaw, np.pi / 2, atol=1e-6)
    c.on_key_press("W")
    assert np.allclose(cam.position, (-0.1, 0, 0), atol=1e-6)
    assert np.allclose(cam.rotation, (np.sqrt(0.5), 0, np.sqrt(0.5), 0), atol=1e-6)      # quat_cast(Ry(pi/2))
    # pitch is clamped to +-pi/2 (cpp:40-43), yaw wraps into [-pi, pi) (cpp:45-52)
    c.on_mouse_move(0.0, 10.0)
    assert np.isclose(c.pitch, np.pi / 2)
    c.on_mouse_move(0.0, -20.0)
    assert np.isclose(c.pitch, -np.pi / 2)
    c.set_pitch(0.0)
    c.set_yaw(3.5)
    assert np.isclose(c.yaw, 3.5 - 2 * np.pi, atol=1e-6)
    c.set_yaw(-3.5)
    assert np.isclose(c.yaw, 2 * np.pi - 3.5, atol=1e-6)
    c.set_yaw(np.pi)
    assert np.isclose(c.yaw, -np.pi, atol=1e-6)
    # reset() reads pitch and yaw back from the camera's quaternion (glm::eulerAngles, cpp:22-27): a round trip
    for yaw, pitch in ((0.3, -0.7), (-2.0, 0.4), (1.2, 1.0)):
        c.set_yaw(yaw)
        c.set_pitch(pitch)
        c.update_camera()
        q = cam.rotation
        # the quaternion is that of Ry(yaw) * Rx(pitch)
        want = (np.cos(yaw / 2) * np.cos(pitch / 2), np.cos(yaw / 2) * np.sin(pitch / 2), np.sin(yaw / 2) * np.cos(pitch / 2),
                -np.sin(yaw / 2) * np.sin(pitch / 2))
        assert np.allclose(q, want, atol=1e-6) or np.allclose(q, [-v for v in want], atol=1e-6)
        c.speed = 7.0
        c.reset()
        assert np.isclose(c.speed, 0.1)
        if abs(yaw) <= np.pi / 2:
            assert np.isclose(c.pitch, pitch, atol=1e-5) and np.isclose(c.yaw, yaw, atol=1e-5)
        else:
            # glm::yaw is an asin and the controller drops the roll glm::eulerAngles reports (cpp:22-27): behind the half
            # turn around the front the reference's Reset comes back with another (yaw, pitch) -- a quirk, kept
            assert abs(c.yaw) <= np.pi / 2 + 1e-6 and np.isclose(abs(c.pitch - pitch), np.pi, atol=1e-5)


def test_cpp_controller_equals_python(pkg, tmp_path):
    """hip_pt --replay SCRIPT --dry-run prints the camera after every controller event (no GPU needed)"""
    _ensure_cli()
    script = tmp_path / "replay.json"
    script.write_text(json.dumps(SCRIPT))
    r = subprocess.run([HIP_PT, "scenes/cornell_mesh.json", "--replay", str(script), "--dry-run"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith(("start:", "event:"))]
    scene = pkg.json_parser.scene_from_json(os.path.join(ROOT, "assets", "scenes", "cornell_mesh.json"))
    import copy
    cam = copy.copy(scene.camera)
    c = pkg.camera_controller.FirstPersonCameraController(cam)

    def state():
        return np.array([*cam.position, c.yaw, c.pitch, *cam.rotation], dtype=np.float64)

    def parsed(tok):
        return np.array([float(tok[i]) for i in (2, 3, 4, 6, 8, 10, 11, 12, 13)])

    assert np.allclose(parsed(lines[0]), state(), atol=1e-7, rtol=1e-7)
    k, restarts = 1, 0
    for ev in SCRIPT["events"]:
        moved = None
        if "key" in ev:
            moved = any([c.on_key_press(ev["key"]) for _ in range(ev.get("count", 1))])
        elif "mouse" in ev:
            moved = c.on_mouse_move(np.float32(np.radians(1)) * np.float32(ev["mouse"][0]), np.float32(np.radians(1)) * np.float32(ev["mouse"][1]))
        elif "speed" in ev:
            c.speed, moved = np.float32(ev["speed"]), False
        elif "position" in ev:
            c.set_position(ev["position"])
            c.update_camera()
            moved = True
        elif "reset" in ev:
            c.reset()
            moved = True
        if moved is None:
            continue
        restarts += 1 if moved else 0
        assert np.allclose(parsed(lines[k]), state(), atol=1e-7, rtol=1e-7), (ev, lines[k])
        assert int(lines[k][-1]) == restarts, ev
        k += 1
    assert k == len(lines) and restarts == 12


def oracle_replay(pkg, orc, scene, script, max_bounces):
    """The viewer loop (app.cpp:141-170, gui.cpp:84-108) with the CPU oracle in the place of the GPU: the state a
    `PathTracer` keeps between calls, restated from path_tracer.cu -- `path_trace` renders iteration_ and counts it only
    while iteration_ < max_iterations and always re-points the result at the colour buffer (:391,:476); `denoise` filters
    the ACCUMULATED buffers and makes its output the result (:479-485); `restart` zeroes the counter (:522-525);
    `resize_image` reallocates and restarts (:527-545); `send_to_preview` shows the result, the normals or 1/depth
    (:487-520); a `filter_size` event sets the denoiser's filter size (gui.cpp:87).  Returns [(rgba, exact_mask,
    denoised)]: exact_mask marks the pixels whose value does not depend on the reference's out-of-bounds A-Trous taps
    (all of them for an undenoised frame).  The oracle defines those taps as the port does, so a denoised frame is
    compared on every pixel too."""
    import copy
    window = tuple(int(v) for v in script.get("window", (800, 800)))
    per_frame = int(script.get("iterations_per_frame", 1))
    camera = copy.copy(scene.camera)
    controller = pkg.camera_controller.FirstPersonCameraController(camera)
    flat = scene.build_scene()
    sh = orc.SceneHandle(flat)
    st = {"iteration": 0, "max_iterations": scene.spp, "method": "streaming", "denoise": False, "display": "final",
          "res": window, "fb": None, "result": None, "touched": None, "filter_size": 10}
    shown = []

    def path_trace():
        w, h = st["res"]
        if st["iteration"] < st["max_iterations"]:
            render = orc.render_megakernel if st["method"] == "megakernel" else orc.render_streaming
            prev = st["fb"] if st["iteration"] > 0 else None
            st["fb"] = render(flat, camera, w, h, st["iteration"], 1, max_bounces, prev=prev, scene_handle=sh)
            st["iteration"] += 1
        st["result"], st["touched"] = st["fb"]["color"], None

    def denoise():
        w, h = st["res"]
        fb = st["fb"]
        st["result"], st["touched"] = orc.denoise(camera, w, h, fb["color"], fb["normal"], fb["depth"], st["filter_size"])

    def turn():
        for _ in range(per_frame):
            path_trace()
            if st["denoise"]:
                denoise()
        w, h = st["res"]
        exact = np.ones((h, w), dtype=bool)
        if st["display"] == "normal":
            rgba = orc.preview(st["fb"]["normal"], w, h, 1)
        elif st["display"] == "depth":
            rgba = orc.preview(st["fb"]["depth"], w, h, 2)
        else:
            rgba = orc.preview(st["result"], w, h, 0)
            if st["touched"] is not None:
                exact = ~st["touched"]
        shown.append((rgba, exact, st["touched"] is not None))

    radians = np.float32(np.radians(1))
    for ev in script["events"]:
        if "frames" in ev:
            for _ in range(int(ev["frames"])):
                turn()
        elif "key" in ev:
            for _ in range(int(ev.get("count", 1))):
                if controller.on_key_press(ev["key"][:1]):
                    st["iteration"] = 0
        elif "mouse" in ev:
            if controller.on_mouse_move(radians * np.float32(ev["mouse"][0]), radians * np.float32(ev["mouse"][1])):
                st["iteration"] = 0
        elif "space" in ev:
            st["iteration"] = 0
        elif "resize" in ev:
            st["res"], st["iteration"] = tuple(int(v) for v in ev["resize"]), 0
        elif "denoise" in ev:
            st["denoise"] = bool(ev["denoise"])
        elif "display" in ev:
            st["display"] = ev["display"]
        elif "method" in ev:
            st["method"] = ev["method"]
        elif "max_iterations" in ev:
            st["max_iterations"] = max(1, int(ev["max_iterations"]))
        elif "filter_size" in ev:
            st["filter_size"] = int(ev["filter_size"])
        elif "speed" in ev:
            controller.speed = np.float32(ev["speed"])
        elif "position" in ev:
            controller.set_position(ev["position"])
            controller.update_camera()
            st["iteration"] = 0
        elif "reset" in ev:
            controller.reset()
            st["iteration"] = 0
        else:
            raise ValueError(ev)
    return shown


@pytest.mark.gpu
def test_replay_frames_against_the_oracle(pkg, orc):
    """Every frame the replayed viewer displays, against the CPU oracle driven through the same script: exact for
    undenoised frames (final, normal view, megakernel), within 1 LSB for denoised ones on every pixel, and on the
    pixels that do not depend on the reference's out-of-bounds taps also with few differing.  Round 3 compared the two front-ends with each
    other only -- the same HIP path twice."""
    scene = pkg.json_parser.scene_from_json(os.path.join(ROOT, "assets", "scenes", "cornell_mesh.json"))
    frames, _ = pkg.viewer.replay(scene, SCRIPT, max_bounces=6)
    want = oracle_replay(pkg, orc, scene, SCRIPT, 6)
    assert len(frames) == len(want) == 12
    denoised_frames = 0
    for i, (got, (rgba, exact, denoised)) in enumerate(zip(frames, want)):
        assert got.shape == rgba.shape, i
        if denoised:
            denoised_frames += 1
            assert exact.mean() > 0.25, i            # enough pixels left to mean something
            diff = np.abs(got.astype(np.int32) - rgba.astype(np.int32))[exact]
            assert int(diff.max()) <= 1, (i, int(diff.max()))
            assert float((diff > 0).mean()) < 0.02, i
            assert_denoised_frame(got, rgba, i)
        else:
            assert np.array_equal(got, rgba), (i, int(np.sum(got != rgba)))
    assert denoised_frames == 4                      # three turns with max_iterations reached + the megakernel frame
    # a second script: depth view, a filter of one pass, budget-free turns of one iteration at the scene's own spp
    script2 = {"window": [56, 40], "iterations_per_frame": 1, "events": [
        {"max_iterations": 4}, {"frames": 2}, {"display": "depth"}, {"frames": 1}, {"display": "final"}, {"mouse": [-35, 12]},
        {"frames": 1}, {"method": "megakernel"}, {"frames": 2}, {"key": "S", "count": 4}, {"method": "streaming"}, {"frames": 5}]}
    frames, _ = pkg.viewer.replay(scene, script2, max_bounces=5)
    want = oracle_replay(pkg, orc, scene, script2, 5)
    assert len(frames) == len(want) == 11
    for i, (got, (rgba, exact, denoised)) in enumerate(zip(frames, want)):
        assert not denoised and np.array_equal(got, rgba), (i, int(np.sum(got != rgba)))
    assert np.all(frames[2][..., 3] == 1)            # the depth view's alpha (path_tracer.cu:345-354)
    assert np.array_equal(frames[-1], frames[-2])    # max_iterations 4 reached after four of the five turns


@pytest.mark.gpu
def test_replay_frames_cpp_equals_python(pkg, tmp_path):
    """the viewer loop on the GPU: C++ (`hip_pt --replay`, PNG sequence) and Python (`viewer.replay`) show the same
    frames -- camera moves and Space restart the accumulation, max_iterations stops it (path_trace is a no-op past it,
    path_tracer.cu:391), the denoised buffer is what `final` shows after a denoise, a resize reallocates"""
    from PIL import Image
    _ensure_cli()
    script = tmp_path / "replay.json"
    script.write_text(json.dumps(SCRIPT))
    prefix = tmp_path / "view"
    r = subprocess.run([HIP_PT, "scenes/cornell_mesh.json", "--replay", str(script), "-o", str(prefix), "--max-bounces", "6"], cwd=ROOT,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    scene = pkg.json_parser.scene_from_json(os.path.join(ROOT, "assets", "scenes", "cornell_mesh.json"))
    frames, controller = pkg.viewer.replay(scene, SCRIPT, max_bounces=6)
    shown = sum(ev.get("frames", 0) for ev in SCRIPT["events"])
    assert len(frames) == shown == 12 and f"{shown} frames shown" in r.stdout
    for i, want in enumerate(frames):
        got = np.array(Image.open(f"{prefix}_{i:04d}.png"))
        assert got.shape == want.shape and np.array_equal(got, want), i
    assert frames[0].shape == (48, 64, 4) and frames[-1].shape == (40, 40, 4)
    # frames 0 and 1 accumulate (2 + 2 iterations of one image); a camera move restarts: frame 2 is another image
    assert not np.array_equal(frames[0], frames[1]) and not np.array_equal(frames[1], frames[2])
    # max_iterations = 3: frame 5 (normal view) had used iterations 0 and 1; the first of the next three turns traces
    # iteration 2 and then path_trace is a no-op -- the three turns show the same finished, denoised image
    assert np.array_equal(frames[6], frames[7]) and np.array_equal(frames[7], frames[8])
    # Space + megakernel: another image (another RNG stream per pixel, path_tracer.cu:239-243)
    assert not np.array_equal(frames[9], frames[8])
    assert np.all(frames[5][..., 3] == 255)   # the normal view is opaque


@pytest.mark.gpu
def test_replay_filter_size_changes(pkg, orc, tmp_path):
    """SCRIPT3 (the `filter_size` event, mid-run): the C++ replay's PNG sequence equals the Python replay's frames, and
    every frame equals the oracle's driven through the same script -- exact when undenoised, within 1 LSB on every pixel
    when denoised"""
    from PIL import Image
    _ensure_cli()
    script = tmp_path / "replay3.json"
    script.write_text(json.dumps(SCRIPT3))
    prefix = tmp_path / "view3"
    r = subprocess.run([HIP_PT, "scenes/cornell_mesh.json", "--replay", str(script), "-o", str(prefix), "--max-bounces", "5"], cwd=ROOT,
                       capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout + r.stderr
    scene = pkg.json_parser.scene_from_json(os.path.join(ROOT, "assets", "scenes", "cornell_mesh.json"))
    frames, _ = pkg.viewer.replay(scene, SCRIPT3, max_bounces=5)
    want = oracle_replay(pkg, orc, scene, SCRIPT3, 5)
    shown = sum(ev.get("frames", 0) for ev in SCRIPT3["events"])
    assert len(frames) == len(want) == shown == 8 and f"{shown} frames shown" in r.stdout
    for i, got in enumerate(frames):
        png = np.array(Image.open(f"{prefix}_{i:04d}.png"))
        assert png.shape == got.shape and np.array_equal(png, got), i
    assert [d for _, _, d in want] == [True] * 7 + [False]
    for i, (got, (rgba, exact, denoised)) in enumerate(zip(frames, want)):
        if denoised:
            assert_denoised_frame(got, rgba, i)
        else:
            assert np.array_equal(got, rgba), (i, int(np.sum(got != rgba)))
