"""GPU: the multi-volume kernel (vrh_render_multi_volume, visionaray_amd/csrc/vrh_multi_volume.hip) against the
reference's own frames tests/golden/mv_*.npz (tests/golden/multi_volume_ref.cpp, run by make_multi_volume_golden.py):
alpha, hit, tmin and the step total bit for bit, rgb to rtol 1e-5 -- the project's bar for plastic::shade on the
device -- and mv_unshaded bit for bit in all four channels.  Where a test has no fixture the device is compared
at the same bars with vrh_multi_volume_render_host, the host build of the same header, which
tests/test_multi_volume_fixtures.py holds to the reference on the CPU.
"""
import functools
import os
import sys
from ctypes import c_void_p as C_void_p

import numpy as np
import pytest

import visionaray_amd as va
from visionaray_amd import _capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mv_cases as MC  # noqa: E402
import vol_cases as VC  # noqa: E402

pytestmark = pytest.mark.gpu
UNIT_BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def fixture(name):
    F = MC.load_frame(name)
    for a in F.values():
        a.setflags(write=False)
    return F


def render(ctx, kern, cam, scissor=None, prefill=None, flags=_capi.VRH_RT_ALL):
    """one frame through hip_sched.frame into a fresh target: (download, stats)"""
    rt = va.hip_buffer_rt(ctx, cam.width, cam.height, flags)
    if prefill is not None:
        rt.upload(**prefill)
    sp = va.make_sched_params(va.pixel_sampler.uniform_type, VC.fixed_camera(cam), rt)
    sp.scissor_box = scissor
    va.hip_sched(ctx, async_frames=False).frame(kern, sp)
    got = rt.download()
    st = ctx.volume_last_stats()
    rt.close()
    return got, st


def device_kernel(ctx, vox, tfs, filters, addresses, entries, k):
    vols = [va.volume(ctx, vox[i], filters[i], addresses[i], tfs[i]) for i in range(len(vox))]
    return va.api._multi_volume_kernel(vols, entries, k), vols


def as_fixture(want):
    return {"color": want["color"], "hit": want["prim_id"] == 0, "tmin": want["t"]}


@pytest.mark.parametrize("name", MC.FRAMES)
def test_fixture_frames(ctx, name):
    F = fixture(name)
    vox, tfs, filters, addresses, entries, k, cam = MC.frame_objects(F)
    kern, vols = device_kernel(ctx, vox, tfs, filters, addresses, entries, k)
    occ = np.full(cam.width * cam.height, 0xA5, np.uint8)
    got, st = render(ctx, kern, cam, prefill={"occ": occ})
    MC.check_frame(got, F, name, exact_rgb=name == "mv_unshaded")
    assert np.array_equal(got["occ"], occ), "VRH_RT_OCC is untouched"
    assert st == {"rays": cam.width * cam.height, "steps": int(F["total_steps"][0]), "capped": 0}
    for v in vols:
        v.close()


@pytest.mark.parametrize("name", ["vol_r8_wrap", "vol_r16_mirror", "vol_r32f_16"])
def test_single_volume_identity_equals_the_volume_kernel(ctx, name):
    """one volume under the identity transform with shade_alpha above every alpha: the frame of vrh_render_volume,
    bit for bit, with equal steps -- for R8, R16 and R32F voxels"""
    F = VC.load_frame(name)
    tf, k1, cam, filt, addr = VC.frame_objects(F)
    vol = va.volume(ctx, F["voxels"], filt, addr, tf)
    rt = va.hip_buffer_rt(ctx, cam.width, cam.height)
    sp = va.make_sched_params(va.pixel_sampler.uniform_type, VC.fixed_camera(cam), rt)
    va.hip_sched(ctx, async_frames=False).frame(va.api._volume_kernel(vol, k1), sp)
    want, want_st = rt.download(), ctx.volume_last_stats()
    rt.close()
    entries = va.multi_volume_entries([(k1.box_min[:], k1.box_max[:])], [np.eye(4, dtype=np.float32)], [va.plastic()])
    entries[0].coord_sign[:], entries[0].coord_offset[:], entries[0].coord_extent[:] = k1.coord_sign[:], k1.coord_offset[:], k1.coord_extent[:]
    k = va.multi_volume_kernel_desc(va.point_light((0.0, 0.0, 0.0)), dt=k1.dt, shade_alpha=2.0)
    k.opacity_cutoff = k1.opacity_cutoff
    got, st = render(ctx, va.api._multi_volume_kernel([vol], entries, k), cam)
    for key in ("color", "prim_id", "t"):
        assert np.array_equal(bits(got[key]), bits(want[key])), key
    assert np.array_equal(bits(got["color"]), bits(F["color"])) and st == want_st and st["steps"] == int(F["total_steps"][0])
    vol.close()


@functools.lru_cache(maxsize=None)
def formats_case(size):
    """mv_formats seen in a width x height image: objects and the host build's frame"""
    F = fixture("mv_formats")
    objs = MC.frame_objects(F, *size)
    vox, tfs, filters, addresses, entries, k, cam = objs
    return objs, va.multi_volume_render_host(vox, tfs, entries, cam, k, filters, addresses)


@pytest.mark.parametrize("size", [(1, 1), (8, 8), (61, 45)], ids=lambda s: "%dx%d" % s)
def test_image_sizes_against_the_host_build(ctx, size):
    (vox, tfs, filters, addresses, entries, k, cam), want = formats_case(size)
    kern, vols = device_kernel(ctx, vox, tfs, filters, addresses, entries, k)
    got, st = render(ctx, kern, cam)
    MC.check_frame(got, as_fixture(want), "%dx%d" % size)
    assert st == want["stats"]
    for v in vols:
        v.close()


def test_scissor_box_leaves_outside_pixels_untouched(ctx):
    (vox, tfs, filters, addresses, entries, k, cam), want = formats_case((MC.FRAME_W, MC.FRAME_H))
    kern, vols = device_kernel(ctx, vox, tfs, filters, addresses, entries, k)
    n = cam.width * cam.height
    pre = {"color": np.full((n, 4), 7.5, np.float32), "prim_id": np.full(n, 123456, np.uint32), "t": np.full(n, 42.0, np.float32),
           "occ": np.full(n, 0x5A, np.uint8)}
    box = (5, 3, 43, 29)                      # x, y and the exclusive right / bottom edges: no edge on a tile boundary
    got, st = render(ctx, kern, cam, scissor=box, prefill=pre)
    y, x = np.divmod(np.arange(n), cam.width)
    inside = (x >= box[0]) & (x < box[2]) & (y >= box[1]) & (y < box[3])
    for key in ("color", "prim_id", "t", "occ"):
        assert np.array_equal(got[key][~inside], pre[key][~inside]), key
    assert np.array_equal(got["occ"], pre["occ"])
    part = {key: got[key][inside] for key in ("color", "prim_id", "t")}
    MC.check_frame(part, {"color": want["color"][inside], "hit": (want["prim_id"] == 0)[inside], "tmin": want["t"][inside]}, "scissor")
    assert st["rays"] == int(inside.sum()) and st["steps"] == int(want["steps_px"].astype(np.int64)[inside].sum())
    for v in vols:
        v.close()


def test_colour_only_target(ctx):
    F = fixture("mv_unshaded")
    vox, tfs, filters, addresses, entries, k, cam = MC.frame_objects(F)
    kern, vols = device_kernel(ctx, vox, tfs, filters, addresses, entries, k)
    got, _ = render(ctx, kern, cam, flags=_capi.VRH_RT_COLOR)
    assert sorted(got) == ["color"] and np.array_equal(bits(got["color"]), bits(F["color"]))
    for v in vols:
        v.close()


def model_transform(rng, spread):
    """a forward model transform t * r * s as a 4x4 float32 [row, col]"""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = float(rng.uniform(-np.pi, np.pi))
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    m = np.eye(4)
    m[:3, :3] = (np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K) @ np.diag(rng.uniform(0.6, 1.6, 3))
    m[:3, 3] = rng.uniform(-spread, spread, 3)
    return m.astype(np.float32)


def random_scene(rng, n, seed, dims_max=10, alpha=(0.02, 0.5)):
    vox, tfs, filters, addresses, transforms, materials = [], [], [], [], [], []
    for i in range(n):
        w, h, d = (int(v) for v in rng.integers(1, dims_max + 1, 3))
        vox.append(VC.voxels(w, h, d, int(rng.integers(0, 3)), seed + i))
        tfs.append(va.transfunc(VC.transfunc(int(rng.choice([1, 2, 5, 17, 256])), seed + 50 + i, float(rng.uniform(*alpha))),
                                int(rng.integers(0, 2)), int(rng.integers(0, 3))))
        filters.append(int(rng.integers(0, 2)))
        addresses.append(tuple(int(v) for v in rng.integers(0, 3, 3)))
        transforms.append(model_transform(rng, 1.2))
        materials.append(va.plastic(ca=(0.1, 0.1, 0.1), cd=tuple(rng.uniform(0.2, 1.0, 3)), kd=float(rng.uniform(0.5, 1.0)),
                                    cs=tuple(rng.uniform(0.0, 1.0, 3)), ks=float(rng.uniform(0.0, 1.0)), exp=float(rng.choice([2.0, 16.0, 128.0]))))
    return vox, tfs, filters, addresses, transforms, materials


def random_camera(rng, W, H, distance):
    direction = rng.normal(size=3)
    direction /= np.linalg.norm(direction)
    cam = va.camera()
    cam.perspective(float(rng.uniform(25.0, 60.0)) * va.DEGREES_TO_RADIANS, W / H, 0.001, 1000.0)
    eye = direction * distance
    cam.look_at(eye, rng.uniform(-0.3, 0.3, 3))
    return cam.basis(W, H), eye


def test_32_volumes(ctx):
    """the example's MAX_VOLS in a 16 x 16 image: 64 KB of per-lane ranges in LDS"""
    rng = np.random.default_rng(32)
    vox, tfs, filters, addresses, transforms, materials = random_scene(rng, 32, 7000, dims_max=5, alpha=(0.01, 0.15))
    cam, eye = random_camera(rng, 16, 16, 7.0)
    vols = [va.volume(ctx, vox[i], filters[i], addresses[i], tfs[i]) for i in range(32)]
    kern = va.multi_volume_kernel(vols, [UNIT_BOX] * 32, transforms, materials, va.point_light(eye), dt=0.05)
    want = va.multi_volume_render_host(vox, tfs, kern.entries, cam, kern.desc, filters, addresses)
    got, st = render(ctx, kern, cam)
    MC.check_frame(got, as_fixture(want), "32 volumes")
    assert st == want["stats"] and st["steps"] > 0
    for v in vols:
        v.close()


@pytest.mark.parametrize("i", range(16))
def test_seeded_sweep_against_the_host_build(ctx, i):
    """random configurations of 1 to 6 volumes: rotations, translations, non-uniform scales, formats, filters,
    address modes, transfer functions, materials, thresholds, steps, image sizes"""
    rng = np.random.default_rng(20250000 + i)
    n = int(rng.integers(1, 7))
    vox, tfs, filters, addresses, transforms, materials = random_scene(rng, n, 9000 + 100 * i)
    W, H = int(rng.integers(1, 40)), int(rng.integers(1, 40))
    cam, eye = random_camera(rng, W, H, float(rng.uniform(0.0, 8.0)) if i % 4 == 3 else float(rng.uniform(5.0, 8.0)))
    light = va.point_light(eye + rng.uniform(-1.0, 1.0, 3), cl=tuple(rng.uniform(0.5, 1.0, 3)), linear_att=float(rng.uniform(0.0, 0.1)))
    vols = [va.volume(ctx, vox[j], filters[j], addresses[j], tfs[j]) for j in range(n)]
    kern = va.multi_volume_kernel(vols, [UNIT_BOX] * n, transforms, materials, light, dt=float(rng.uniform(0.02, 0.08)),
                                  opacity_cutoff=float(rng.uniform(0.5, 1.0)), shade_alpha=float(rng.choice([0.0, 0.05, 0.1, 0.3])),
                                  gradient_delta=float(rng.choice([0.01, 0.05, 0.3])),
                                  flip=tuple(bool(b) for b in rng.integers(0, 2, 3)))
    want = va.multi_volume_render_host(vox, tfs, kern.entries, cam, kern.desc, filters, addresses)
    got, st = render(ctx, kern, cam)
    MC.check_frame(got, as_fixture(want), "sweep %d" % i)
    assert st == want["stats"], i
    for v in vols:
        v.close()


def test_refusals_on_the_device(ctx):
    """a target of another size, and a volume of another context"""
    F = fixture("mv_unshaded")
    vox, tfs, filters, addresses, entries, k, cam = MC.frame_objects(F)
    kern, vols = device_kernel(ctx, vox, tfs, filters, addresses, entries, k)
    handles = (C_void_p * 2)(*[v.handle.value for v in vols])
    rt = va.hip_buffer_rt(ctx, 32, 32)
    with pytest.raises(va.VrhError) as e:
        _capi.check("vrh_render_multi_volume", ctx.handle, handles, entries, 2, rt.handle, cam, k)
    assert e.value.code == _capi.VRH_ERR_INVALID and "size" in str(e.value)
    other = va.Context(0)
    foreign = va.volume(other, vox[1], filters[1], addresses[1], tfs[1])
    mixed = (C_void_p * 2)(vols[0].handle.value, foreign.handle.value)
    rt2 = va.hip_buffer_rt(ctx, cam.width, cam.height)
    with pytest.raises(va.VrhError) as e:
        _capi.check("vrh_render_multi_volume", ctx.handle, mixed, entries, 2, rt2.handle, cam, k)
    assert e.value.code == _capi.VRH_ERR_INVALID and "volume 1 belongs to another context" in str(e.value)
    ctx.sync()
    foreign.close(), rt.close(), rt2.close()
    for v in vols:
        v.close()
    other.close()

