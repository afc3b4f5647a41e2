"""Occlusion queries (ptc_occluded_rays), the part that needs no GPU: the binding, the argument checks, and
the property the any-hit kernels rest on -- hit(scene) == OR over groups of hit(group), every group tested with the caller's
t_max -- on the CPU oracle."""
import ctypes as C

import numpy as np

import occlusion_rays as R


def test_symbols_and_struct_through_the_binding(pkg):
    capi = pkg._capi
    lib = pkg.lib()
    for name in ("ptc_occluded_rays", "ptc_get_occlusion_stats"):
        assert name in capi.SIGNATURES and hasattr(lib, name)
    # { uint64 rays, occluded, redone; double kernel_ms; uint32 launches; } + tail padding to 8
    assert C.sizeof(capi.ptc_occlusion_stats) == 40
    assert [f[0] for f in capi.ptc_occlusion_stats._fields_] == ["rays", "occluded", "redone", "kernel_ms", "launches"]
    assert lib.ptc_abi_version() == 3   # new entry points, no new version


def test_null_arguments_are_invalid_without_a_device(pkg):
    capi = pkg._capi
    lib = pkg.lib()
    rays = np.zeros((1, 8), dtype=np.float32)
    out = np.zeros(1, dtype=np.uint8)
    fp, bp = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    fake = C.c_void_p(8)   # never dereferenced: the NULL checks come first
    assert lib.ptc_occluded_rays(None, rays.ctypes.data_as(fp), 1, out.ctypes.data_as(bp)) == capi.PTC_ERR_INVALID
    assert lib.ptc_occluded_rays(fake, None, 1, out.ctypes.data_as(bp)) == capi.PTC_ERR_INVALID
    assert lib.ptc_occluded_rays(fake, rays.ctypes.data_as(fp), 1, None) == capi.PTC_ERR_INVALID
    st = capi.ptc_occlusion_stats()
    assert lib.ptc_get_occlusion_stats(None, C.byref(st)) == capi.PTC_ERR_INVALID
    assert lib.ptc_get_occlusion_stats(fake, None) == capi.PTC_ERR_INVALID


def test_hit_of_the_scene_is_the_or_over_its_objects(pkg, orc):
    """The reference's loop carries a shrinking t_max from object to object (path_tracer.cu:118-125); whether it reports a
    hit at all does not depend on that: the first object it accepts is tested with the caller's t_max.  60,000 shadow-style
    rays, the full scene's flag against the OR over one scene per object."""
    scene = R.occlusion_scene(pkg)
    rays = R.shadow_rays()
    assert len(rays) == 60000 and set(np.unique(rays[:, 3])) == {np.float32(1e-4), np.float32(1e-5)}
    _, hit = orc.intersect_rays(scene.build_scene(), rays)
    hit = hit.astype(bool)
    assert 0.2 < hit.mean() < 0.8, hit.mean()   # a condition on the inputs: neither answer dominates
    ones = R.one_object_scenes(pkg, scene)
    assert len(ones) == 8
    any_group = np.zeros(len(rays), dtype=bool)
    shares = []
    for one in ones:
        _, h = orc.intersect_rays(one.build_scene(), rays)
        any_group |= h.astype(bool)
        shares.append(float(h.mean()))
    assert int(np.sum(any_group != hit)) == 0
    assert shares[4] > 0.05 and min(shares) > 0.0   # the mesh instances and every other object do occlude some of the rays
