"""MI355X (gfx950) path-tracing core behind the render API of LesleyLai/cuda-path-tracer.

The directory name contains a hyphen, so it is imported through ``__graft_entry__.load_package()``
under the module name ``cuda_path_tracer_amd``.  All rendering happens in ``libptcore.so``
(``csrc/``, C ABI in ``include/ptcore.h``); the Python files are the host-side mirror of the reference's
``PathTracer`` / ``SceneDescription`` interface used by the tests and by bench.py."""
from . import _capi, bands, camera_controller, glmlite, hdr, json_parser, png, scenes, viewer
from ._capi import LIB_PATH, PtcError, lib
from .path_tracer import LIGHT_DTYPE, Display, DisplayBufferType, EdgeAvoidingATrousDenoiser, GPUMethod, PathTracer, ToneCurve, Texture, check_light_sample, check_megakernel_instance, check_texture_lookup, check_megakernel_instance2, check_normal_map, check_demodulate, check_denoise_variance, normal_map_decode_table, compute_vertex_normals, light_material_pdf, light_table, texture_decode_table
from .scene_description import (Camera, DielectricMaterial, DiffuseMateral, EmissiveMaterial, FlatScene, Mesh, MetalMaterial,
                                SceneDescription, Sphere, TextureSource, bvh_from_mesh)

__all__ = ["PathTracer", "GPUMethod", "DisplayBufferType", "Display", "ToneCurve", "EdgeAvoidingATrousDenoiser", "SceneDescription", "Camera",
           "Sphere", "Mesh", "DiffuseMateral", "MetalMaterial", "DielectricMaterial", "EmissiveMaterial", "FlatScene", "bvh_from_mesh",
           "light_table", "light_material_pdf", "check_light_sample", "check_megakernel_instance", "compute_vertex_normals", "Texture", "texture_decode_table", "check_texture_lookup", "check_megakernel_instance2", "check_normal_map", "check_demodulate", "check_denoise_variance", "normal_map_decode_table", "LIGHT_DTYPE", "scenes", "bands", "glmlite", "hdr", "png", "TextureSource", "json_parser", "lib", "LIB_PATH", "PtcError"]
