"""visionaray_amd -- MI355X-native (gfx950) backend for Visionaray's ray-traversal hot path.

BVH traversal + ray/triangle and ray/sphere intersection as hand-written HIP kernels behind the
C-ABI in include/vrh.h (libvrh.so), with a host API that mirrors the reference's
scheduler / render_target / BVH interface (hip_sched, hip_buffer_rt, hip_index_bvh) and the
multi-GPU render groups (render_group, render_sharded: image-tile shards gathered over RCCL).
"""
from . import _capi
from ._capi import VrhError
from .api import (BVH_NODE_DTYPE, DEGREES_TO_RADIANS, GENERIC_DTYPE, GENERIC_TYPE_SPHERE, GENERIC_TYPE_TRIANGLE, GROUP_ID_BYTES, MATERIAL_DTYPE, MATERIAL_EMISSIVE, MATERIAL_MATTE,
                  MATERIAL_MIRROR, MATERIAL_PLASTIC, PLASTIC_DTYPE, POINT_LIGHT_DTYPE,
                  SPHERE_DTYPE, TRIANGLE_DTYPE, Context, ao_kernel, broadcast_scene, build_index_bvh, camera, closest_hit_kernel, color_format, depth_format,
                  device_count, emissive, face_normals, generic_materials, generic_shading, hip_buffer_rt, hip_index_bvh, hip_sched,
                  hit_mask, index_bvh, load_obj, load_pnm, make_generic, make_sched_params, make_spheres, make_triangles, matrix_inverse, matte, mirror, model,
                  multi_hit_kernel, multi_volume_entries, multi_volume_kernel, multi_volume_kernel_desc, multi_volume_render_host,
                  normals_per_face_binding, normals_per_vertex_binding, pathtracing_kernel, pixel_sampler,
                  plastic,
                  point_light, render, render_batch, render_group, render_sampled, render_sharded, render_view, resolve_desc, rt_resolve_host, sah_cost, shading,
                  shard_bands, simple_kernel, tex3d_host, tex_address, tex_filter, texture, transfunc, unshard, view_camera, volume,
                  volume_desc, volume_kernel, volume_kernel_desc, volume_render_host, whitted_kernel, with_hit_mask)

__all__ = [
    "BVH_NODE_DTYPE", "DEGREES_TO_RADIANS", "GENERIC_DTYPE", "GENERIC_TYPE_SPHERE", "GENERIC_TYPE_TRIANGLE", "GROUP_ID_BYTES", "MATERIAL_DTYPE", "MATERIAL_EMISSIVE", "MATERIAL_MATTE",
    "MATERIAL_MIRROR", "MATERIAL_PLASTIC", "PLASTIC_DTYPE", "POINT_LIGHT_DTYPE", "SPHERE_DTYPE",
    "TRIANGLE_DTYPE", "Context", "VrhError", "_capi", "ao_kernel", "broadcast_scene", "build_index_bvh", "camera", "closest_hit_kernel", "color_format", "depth_format",
    "device_count", "emissive", "face_normals", "generic_materials", "generic_shading", "hip_buffer_rt", "hip_index_bvh", "hip_sched",
    "hit_mask", "index_bvh", "load_obj", "load_pnm", "make_generic", "make_sched_params", "make_spheres", "make_triangles", "matrix_inverse", "matte", "mirror", "model",
    "multi_hit_kernel", "multi_volume_entries", "multi_volume_kernel", "multi_volume_kernel_desc", "multi_volume_render_host",
    "normals_per_face_binding", "normals_per_vertex_binding", "pathtracing_kernel", "pixel_sampler",
    "plastic",
    "point_light", "render", "render_batch", "render_group", "render_sampled", "render_sharded", "render_view", "resolve_desc", "rt_resolve_host", "sah_cost",
    "shading", "shard_bands", "simple_kernel", "tex3d_host", "tex_address", "tex_filter", "texture", "transfunc", "unshard", "view_camera",
    "volume", "volume_desc", "volume_kernel", "volume_kernel_desc", "volume_render_host", "whitted_kernel", "with_hit_mask",
]
