"""GPU: randomized parity sweep of the generic-primitive instances (VRH_PRIM_GENERIC80) against the oracle's
VO_GENERIC mode (the C restatement of the reference over generic_primitive<triangle, sphere>).

Every case (tests/gp_cases.py sweep_case, a function of its seed alone) draws a mixed scene -- up to 3000 triangles
whose sizes span 1e-3 .. 0.3, some of them slivers, and up to 2000 spheres of radius 1e-3 .. 0.2 that overlap, interleaved
in prim order; some cases hold one kind only, a handful of primitives or a single one --, a camera outside or inside
the cloud, an image of 1 .. 140 x 1 .. 90 pixels (some narrower than a tile, one of 1 x 1), the kernel (primary, AO with
1 .. 32 samples, simple, whitted with 1 .. 5 bounces), plastics, one to three lights and a frame number, and renders
one frame through hip_sched.frame; a third of the cases under one launch option at a non-default value the launch
plan accepts for a generic scene.  tests/test_oracle_generic.py checks on the CPU what these cases cover.

Bars: prim id, the bits of t, the AO mask (with more than 8 samples the kernel writes none: the buffer must stay as it
was, and the colour, 1 - k / samples, carries the count) and the AO / primary colour are the oracle's on every pixel; simple / whitted
radiance is the oracle's bit for bit on a miss and within 1e-5 relative (the device powf; floor 1e-7, as
tests/test_gpu_fuzz_shading.py) on a hit.
"""
import numpy as np
import pytest

import gp_cases as G
import visionaray_amd as va

pytestmark = pytest.mark.gpu
@pytest.mark.parametrize("seed", G.SWEEP_SEEDS)
def test_random_generic_scenes_vs_oracle(ctx, oracle_mod, seed):
    c = G.sweep_case(seed)
    sc, ref = G.sweep_reference(seed)
    host = va.index_bvh(c["prims"], sc.nodes.view(va.BVH_NODE_DTYPE), sc.indices, sc.max_depth)     # the oracle's own tree
    dev = va.hip_index_bvh(ctx, host, c["normals"])
    assert dev.info["prim_kind"] == va._capi.VRH_PRIM_GENERIC80
    sh = G.shading_of(ctx, c)
    kern = G.kernel(c["kind"], dev, sh, c["spec"])
    rt = va.hip_buffer_rt(ctx, c["W"], c["H"])
    wide_mask = c["kind"] == "ao" and c["spec"]["ao_samples"] > 8         # a byte holds 8 sample bits: the buffer is left alone
    if wide_mask:
        rt.upload(occ=np.full(c["W"] * c["H"], 0xA5, np.uint8))
    opt = c["option"]
    if opt:
        ctx.set_option(*opt)
    try:
        va.hip_sched(ctx).frame(kern, va.make_sched_params(c["cam"], rt), frame_num=c["spec"]["frame_num"])
        out = rt.download()
    finally:
        if opt:
            ctx.set_option(opt[0], 0)
        rt.close()
    G.assert_frame(out, ref, c["kind"], c["spec"]["ao_samples"], "seed %d" % seed)
    if wide_mask:
        assert (out["occ"] == 0xA5).all()
