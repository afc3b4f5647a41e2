"""The scenes that the CPU and GPU tests of direct lighting in the megakernel and of Russian roulette
(section 5h) share -- TEST INFRASTRUCTURE.  The loops they are rendered by stand in lit_ref.py."""
import numpy as np


def glass_lamp_scene(pkg):
    """A sphere lamp inside a glass sphere, over a floor with a diffuse ball: every segment from a diffuse surface to a point of
    the lamp crosses the glass, so every shadow ray is blocked and the lamp's light arrives only by paths that end on it after a
    dielectric vertex (or straight from the camera) -- the emission the gate must keep."""
    glm = pkg.glmlite
    s = pkg.SceneDescription()
    s.add_material("floor", pkg.DiffuseMateral((0.7, 0.7, 0.7)))
    s.add_material("ball", pkg.DiffuseMateral((0.2, 0.5, 0.3)))
    s.add_material("glass", pkg.DielectricMaterial(1.5))
    s.add_material("lamp", pkg.EmissiveMaterial((5.0, 4.0, 3.0)))
    s.add_object(pkg.Sphere((0, 0, 0), 1000.0), glm.translate((0.0, -1001.0, 0.0)), "floor")
    s.add_object(pkg.Sphere((0, 0, 0), 0.4), glm.translate((-1.0, -0.6, -0.8)), "ball")
    s.add_object(pkg.Sphere((0, 0, 0), 0.45), glm.translate((0.2, 0.1, -1.0)), "glass")
    s.add_object(pkg.Sphere((0, 0, 0), 0.2), glm.translate((0.2, 0.1, -1.0)), "lamp")
    s.camera = pkg.scenes._camera_from_look_at((0.0, 0.4, 3.0), (0.0, -0.1, -1.0), vfov_deg=45.0)
    return s


def metal_glass_scene(pkg):
    """A panel lamp (a mesh) over a floor, with a metal and a glass ball hanging between the two: shadow rays blocked by either,
    lamp hits after a metal and after a dielectric vertex (counted) and after a diffuse one (not counted)."""
    glm = pkg.glmlite
    s = pkg.SceneDescription()
    s.add_material("floor", pkg.DiffuseMateral((0.7, 0.7, 0.7)))
    s.add_material("mirror", pkg.MetalMaterial((0.9, 0.8, 0.7), 0.05))
    s.add_material("glass", pkg.DielectricMaterial(1.5))
    s.add_material("panel", pkg.EmissiveMaterial((6.0, 6.0, 5.5)))
    s.add_object(pkg.Sphere((0, 0, 0), 1000.0), glm.translate((0.0, -1001.0, 0.0)), "floor")
    s.add_object(pkg.Sphere((0, 0, 0), 0.35), glm.translate((-0.35, 0.3, -0.9)), "mirror")
    s.add_object(pkg.Sphere((0, 0, 0), 0.35), glm.translate((0.45, 0.3, -0.7)), "glass")
    s.add_object(s.add_mesh("models/light_panel.obj", pkg.scenes.light_panel_mesh()), glm.identity(), "panel")
    s.camera = pkg.scenes._camera_from_look_at((0.0, 0.6, 3.2), (0.0, 0.1, -0.8), vfov_deg=45.0)
    return s


# The statistical test's room is CLOSED (no path leaves: a plain path ends on the lamp or at the cap), its walls have albedo 0.5, and
# one small sphere lamp hangs under the ceiling.  With direct lighting the diffuse hit at the LAST bounce still draws a light sample,
# a term the plain render (capped there) does not have: its share is below albedo^bounces = 0.5^24 = 6e-8 of the image at
# STAT_BOUNCES bounces, far below what the test resolves.
STAT_BOUNCES = 24


def small_lamp_room(pkg):
    """The closed room as ONE MESH (a box of 12 triangles).  The walls are triangles on purpose: the rule's shadow ray starts AT the
    hit point with t_min 1e-4 (section 5f's epsilons), and a triangle's own test gives t = 0 to within a few ulp of the coordinates
    (~1e-6 here) for a ray that starts in its plane, so no shadow ray is blocked by the wall it starts on.  The stock scenes' walls --
    spheres of radius 1000 -- do not have that property in binary32: c = |o - centre|^2 - R^2 is known to ~0.1 there, the near root
    of the quadratic to ~1e-4 / cos, and 7 % of the shadow rays of small_lamp_sphere_room hit their own wall (measured on the CPU
    oracle: tools/direct_loop_ab.py prints that room's figures).  That is a property of the shadow epsilon on such geometry, not of
    the estimator this test is about."""
    glm = pkg.glmlite
    s = pkg.SceneDescription()
    x0, x1, y0, y1, z0, z1 = -2.0, 2.0, -1.0, 1.5, -2.0, 4.5
    positions = np.array([[x, y, z] for x in (x0, x1) for y in (y0, y1) for z in (z0, z1)], dtype=np.float32)  # index = 4 ix + 2 iy + iz
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    indices = np.array([i for a, b, c, d in quads for i in (a, b, c, a, c, d)], dtype=np.uint32)
    s.add_material("walls", pkg.DiffuseMateral((0.5, 0.5, 0.5)))
    s.add_object(s.add_mesh("models/closed_room.obj", pkg.Mesh(positions, indices)), glm.identity(), "walls")
    s.add_material("lamp", pkg.EmissiveMaterial((12.0, 11.0, 9.0)))
    s.add_object(pkg.Sphere((0, 0, 0), 0.25), glm.translate((0.6, 1.0, -0.8)), "lamp")
    s.camera = pkg.scenes._camera_from_look_at((0.0, 0.0, 4.0), (0.0, -0.1, 0.0), vfov_deg=45.0)
    return s


def small_lamp_sphere_room(pkg):
    """The same room from six wall spheres of radius 1000 (the stock scenes' walls): NOT the statistical test's scene, see
    small_lamp_room; kept so that the self-shadowing it shows stays measurable."""
    glm = pkg.glmlite
    s = pkg.SceneDescription()
    big = 1000.0
    for name, rgb, at in (("floor", (0.5, 0.5, 0.5), (0.0, -big - 1.0, 0.0)), ("ceiling", (0.5, 0.5, 0.5), (0.0, big + 1.5, 0.0)),
                          ("back", (0.5, 0.5, 0.5), (0.0, 0.0, -big - 2.0)), ("front", (0.5, 0.5, 0.5), (0.0, 0.0, big + 4.5)),
                          ("left", (0.5, 0.1, 0.1), (-big - 2.0, 0.0, 0.0)), ("right", (0.1, 0.4, 0.15), (big + 2.0, 0.0, 0.0))):
        s.add_material(name, pkg.DiffuseMateral(rgb))
        s.add_object(pkg.Sphere((0, 0, 0), big), glm.translate(at), name)
    s.add_material("lamp", pkg.EmissiveMaterial((12.0, 11.0, 9.0)))
    s.add_object(pkg.Sphere((0, 0, 0), 0.25), glm.translate((0.6, 1.0, -0.8)), "lamp")
    s.camera = pkg.scenes._camera_from_look_at((0.0, 0.0, 4.0), (0.0, -0.1, 0.0), vfov_deg=45.0)
    return s
