"""GPU: the volume kernel (vrh_render_volume, visionaray_amd/csrc/vrh_volume.hip) and the device samplers
(vrh_volume_sample) against the reference's own frames and samples, bit for bit.

tests/golden/vol_*.npz are frames of the reference's volume loop and tests/golden/tex3d_samples.npz direct
tex3D / tex1D calls (tests/golden/volume_ref.cpp, run by make_volume_golden.py).  Where a test has no
fixture -- other image sizes, the seeded sweep -- the device is compared with vrh_volume_render_host, the host
build of the same header, which tests/test_volume_fixtures.py and tests/test_volume_sampling.py hold to the
reference on the CPU.
"""
import functools
import os
import sys

import numpy as np
import pytest

import visionaray_amd as va
from visionaray_amd import _capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vol_cases as VC  # noqa: E402

pytestmark = pytest.mark.gpu
MISS = 0xFFFFFFFF
TF_LDS = 1024           # visionaray_amd/csrc/vrh_volume.hip VOLUME_TF_LDS: larger transfer functions stay in global memory


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def fixture(name):
    F = VC.load_frame(name)
    for a in F.values():
        a.setflags(write=False)
    return F


def render(ctx, vol, k, cam, scissor=None, prefill=None, flags=_capi.VRH_RT_ALL):
    """one frame through hip_sched.frame into a fresh target: (download, stats)"""
    rt = va.hip_buffer_rt(ctx, cam.width, cam.height, flags)
    if prefill is not None:
        rt.upload(**prefill)
    sp = va.make_sched_params(va.pixel_sampler.uniform_type, VC.fixed_camera(cam), rt)
    sp.scissor_box = scissor
    kern = va.api._volume_kernel(vol, k)
    va.hip_sched(ctx, async_frames=False).frame(kern, sp)
    got = rt.download()
    st = ctx.volume_last_stats()
    rt.close()
    return got, st


def check_against(got, want_color, want_hit, want_tnear, name):
    hit = np.asarray(want_hit).astype(bool)
    assert np.array_equal(got["prim_id"] == 0, hit) and np.all(got["prim_id"][~hit] == MISS), name
    assert np.array_equal(bits(got["t"][hit]), bits(np.asarray(want_tnear)[hit])) and np.all(got["t"][~hit] == -1.0), name
    bad = np.flatnonzero(np.any(bits(got["color"]) != bits(want_color), axis=1))
    assert bad.size == 0, f"{name}: {bad.size} pixels differ, first {bad[0]}: {got['color'][bad[0]]} != {want_color[bad[0]]}"


@pytest.mark.parametrize("name", VC.FRAMES)
def test_fixture_frames(ctx, name):
    F = fixture(name)
    tf, k, cam, filt, addr = VC.frame_objects(F)
    vol = va.volume(ctx, F["voxels"], filt, addr, tf)
    occ = np.full(cam.width * cam.height, 0xA5, np.uint8)
    got, st = render(ctx, vol, k, cam, prefill={"occ": occ})
    check_against(got, F["color"], F["hit"], F["tnear"], name)
    assert np.array_equal(got["occ"], occ), "VRH_RT_OCC is untouched"
    assert st == {"rays": cam.width * cam.height, "steps": int(F["total_steps"][0]), "capped": 0}
    vol.close()


def test_colour_only_target(ctx):
    F = fixture("vol_example")
    tf, k, cam, filt, addr = VC.frame_objects(F)
    vol = va.volume(ctx, F["voxels"], filt, addr, tf)
    got, _ = render(ctx, vol, k, cam, flags=_capi.VRH_RT_COLOR)
    assert sorted(got) == ["color"] and np.array_equal(bits(got["color"]), bits(F["color"]))
    vol.close()


@functools.lru_cache(maxsize=None)
def samples():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tex3d_samples.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("size", VC.SIZES, ids=lambda s: "%dx%dx%d" % s)
def test_device_samplers_equal_the_reference(ctx, size):
    """vrh_volume_sample: tex3D on the device over every format, filter and address triple of the fixture,
    and tex1D of the sampled value against the host build of the transfer function"""
    w, h, d = size
    coords = VC.coords(w, h, d)
    tf = va.transfunc(VC.transfunc(256), va.tex_filter.linear, va.tex_address.wrap)
    for fmt in VC.FORMATS:
        for f in VC.FILTERS:
            for a in VC.ADDRESS:
                key = VC.config_key(w, h, d, fmt, f, a)
                kept = np.unpackbits(samples()[key + "_kept"])[:len(coords)].astype(bool)
                vol = va.volume(ctx, VC.voxels(w, h, d, fmt), f, a, tf)
                vox, rgba = vol.sample(coords)
                vol.close()
                bad = np.flatnonzero(kept & (bits(vox) != samples()[key]))
                assert bad.size == 0, f"{key}: {bad.size} samples differ, first at {coords[bad[0]]}"
                assert np.array_equal(bits(rgba), bits(tf.tex1d(vox))), key


@pytest.mark.parametrize("cfg", VC.tf_configs(), ids=lambda c: VC.tf_key(*c))
def test_device_tex1d_equals_the_reference(ctx, cfg):
    """tex1D on the device at the fixture's coordinates: a 1 x 1 x n float volume sampled nearest hands
    each coordinate to the transfer function as its voxel"""
    n, f, a = cfg
    coords = VC.tf_coords(n)
    key = VC.tf_key(*cfg)
    kept = np.unpackbits(samples()[key + "_kept"])[:len(coords)].astype(bool)
    vol = va.volume(ctx, coords.reshape(1, 1, -1), va.tex_filter.nearest, va.tex_address.clamp, va.transfunc(VC.transfunc(n), f, a))
    at = np.zeros((len(coords), 3), np.float32)
    at[:, 0] = (np.arange(len(coords)) + 0.5) / len(coords)
    vox, rgba = vol.sample(at)
    vol.close()
    assert np.array_equal(bits(vox), bits(coords)), "the nearest sample returns the voxel itself"
    bad = np.flatnonzero(kept & np.any(bits(rgba) != samples()[key], axis=1))
    assert bad.size == 0, f"{key}: {bad.size} samples differ, first at {coords[bad[0]]}"


def test_scissor_box_leaves_outside_pixels_untouched(ctx):
    F = fixture("vol_r8_wrap")
    tf, k, cam, filt, addr = VC.frame_objects(F)
    vol = va.volume(ctx, F["voxels"], filt, addr, tf)
    n = cam.width * cam.height
    pre = {"color": np.full((n, 4), 7.5, np.float32), "prim_id": np.full(n, 123456, np.uint32), "t": np.full(n, 42.0, np.float32),
           "occ": np.full(n, 0x5A, np.uint8)}
    box = (5, 3, 43, 29)                      # x, y and the exclusive right / bottom edges: no edge on a tile boundary
    got, st = render(ctx, vol, k, cam, scissor=box, prefill=pre)
    y, x = np.divmod(np.arange(n), cam.width)
    inside = (x >= box[0]) & (x < box[2]) & (y >= box[1]) & (y < box[3])
    for key in ("color", "prim_id", "t", "occ"):
        assert np.array_equal(got[key][~inside], pre[key][~inside]), key
    assert np.array_equal(got["occ"], pre["occ"])
    assert np.array_equal(bits(got["color"][inside]), bits(F["color"][inside]))
    hit = F["hit"].astype(bool)
    assert np.array_equal(got["prim_id"][inside] == 0, hit[inside])
    assert st["rays"] == int(inside.sum()) and st["steps"] == int(F["steps_px"].astype(np.int64)[inside].sum())
    vol.close()


@pytest.mark.parametrize("size", [(1, 1), (8, 8), (65, 9), (60, 44)], ids=lambda s: "%dx%d" % s)
def test_image_sizes_against_the_host_build(ctx, size):
    F = fixture("vol_r32f_16")
    tf, k, cam, filt, addr = VC.frame_objects(F, *size)
    vol = va.volume(ctx, F["voxels"], filt, addr, tf)
    want = va.volume_render_host(F["voxels"], tf, cam, k, filt, addr)
    got, st = render(ctx, vol, k, cam)
    check_against(got, want["color"], want["prim_id"] == 0, want["t"], "%dx%d" % size)
    assert st == want["stats"]
    vol.close()


def test_set_transfunc_between_two_frames(ctx):
    """a replaced transfer function renders the host build's frame, and the fixture's one its bits again"""
    A = B = fixture("vol_r32f_16")
    tf, k, cam, filt, addr = VC.frame_objects(A)
    vol = va.volume(ctx, A["voxels"], filt, addr, tf)
    got, _ = render(ctx, vol, k, cam)
    check_against(got, A["color"], A["hit"], A["tnear"], "first")
    # another transfer function: the host build gives the frame; then back to the fixture's
    other = va.transfunc(VC.transfunc(300, 5, 0.1), va.tex_filter.nearest, va.tex_address.mirror)
    vol.set_transfunc(other)
    got, st = render(ctx, vol, k, cam)
    want = va.volume_render_host(A["voxels"], other, cam, k, filt, addr)
    check_against(got, want["color"], want["prim_id"] == 0, want["t"], "replaced")
    assert st == want["stats"] and not np.array_equal(bits(got["color"]), bits(A["color"]))
    vol.set_transfunc(tf)
    got, st = render(ctx, vol, k, cam)
    check_against(got, B["color"], B["hit"], B["tnear"], "restored")
    assert st["steps"] == int(B["total_steps"][0])
    vol.close()


def test_two_fixtures_share_a_volume_through_set_transfunc(ctx):
    """vol_r8_wrap's voxels rendered with vol_behind's transfer function and view equal the host build, and
    after set_transfunc back the first fixture's bits return"""
    A, B = fixture("vol_r8_wrap"), fixture("vol_behind")
    tfa, ka, cama, filt, addr = VC.frame_objects(A)
    tfb, kb, camb, _f, _a = VC.frame_objects(B)
    vol = va.volume(ctx, A["voxels"], filt, addr, tfb)
    got, st = render(ctx, vol, kb, camb)
    want = va.volume_render_host(A["voxels"], tfb, camb, kb, filt, addr)
    check_against(got, want["color"], want["prim_id"] == 0, want["t"], "b on a")
    vol.set_transfunc(tfa)
    got, st = render(ctx, vol, ka, cama)
    check_against(got, A["color"], A["hit"], A["tnear"], "a")
    assert st["steps"] == int(A["total_steps"][0])
    vol.close()


@pytest.mark.parametrize("n", [TF_LDS - 1, TF_LDS, TF_LDS + 1, 2 * TF_LDS + 3])
def test_transfer_function_sizes_around_the_lds_limit(ctx, n):
    F = fixture("vol_tf4096")
    _tf, k, cam, filt, addr = VC.frame_objects(F)
    tf = va.transfunc(VC.transfunc(n, 3, 0.06), va.tex_filter.linear, va.tex_address.clamp)
    vol = va.volume(ctx, F["voxels"], filt, addr, tf)
    want = va.volume_render_host(F["voxels"], tf, cam, k, filt, addr)
    got, st = render(ctx, vol, k, cam)
    check_against(got, want["color"], want["prim_id"] == 0, want["t"], "tf %d" % n)
    assert st == want["stats"] and st["steps"] > 0
    vol.close()


def test_seeded_sweep_against_the_host_build(ctx):
    """About 20 random volumes (<= 12^3), formats, filters, address modes, transfer functions, boxes, flips,
    cameras and steps against vrh_volume_render_host -- the host build of the same header, which the CPU
    tests (tests/test_volume_fixtures.py, tests/test_volume_sampling.py) hold to the reference bit for bit."""
    rng = np.random.default_rng(20240607)
    some_hit = 0
    for i in range(20):
        w, h, d = (int(v) for v in rng.integers(1, 13, 3))
        fmt = int(rng.integers(0, 3))
        filt = int(rng.integers(0, 2))
        addr = tuple(int(v) for v in rng.integers(0, 3, 3))
        vox = VC.voxels(w, h, d, fmt, 1000 + i)
        n = int(rng.choice([1, 2, 3, 17, 256, 1500]))
        tf = va.transfunc(VC.transfunc(n, 2000 + i, float(rng.uniform(0.02, 0.5))), int(rng.integers(0, 2)), int(rng.integers(0, 3)))
        lo = rng.uniform(-3.0, 2.0, 3)
        hi = lo + rng.uniform(0.3, 3.0, 3)
        extent = float(np.linalg.norm(hi - lo))
        k = va.volume_kernel_desc((lo, hi), dt=extent / float(rng.uniform(20.0, 300.0)), opacity_cutoff=float(rng.uniform(0.5, 1.0)),
                                  flip=tuple(bool(b) for b in rng.integers(0, 2, 3)))
        centre = (lo + hi) / 2
        direction = rng.normal(size=3)
        direction /= np.linalg.norm(direction)
        cam = va.camera()
        W, H = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        cam.perspective(float(rng.uniform(20.0, 70.0)) * va.DEGREES_TO_RADIANS, W / H, 0.001, 1000.0)
        if i % 5 == 4:
            cam.look_at(centre + (hi - lo) * rng.uniform(-0.3, 0.3, 3), centre + direction)        # the eye inside
        else:
            cam.look_at(centre + direction * extent * float(rng.uniform(0.8, 2.0)), centre + rng.uniform(-0.2, 0.2, 3) * extent)
        basis = cam.basis(W, H)
        want = va.volume_render_host(vox, tf, basis, k, filt, addr)
        vol = va.volume(ctx, vox, filt, addr, tf)
        got, st = render(ctx, vol, k, basis)
        vol.close()
        check_against(got, want["color"], want["prim_id"] == 0, want["t"], "sweep %d" % i)
        assert st == want["stats"], i
        some_hit += int(want["stats"]["steps"] > 0)
    assert some_hit >= 15


def test_refusals_on_the_device(ctx):
    F = fixture("vol_example")
    tf, k, cam, filt, addr = VC.frame_objects(F)
    vol = va.volume(ctx, F["voxels"], filt, addr, tf)
    rt = va.hip_buffer_rt(ctx, 32, 32)                    # not the camera's size
    with pytest.raises(va.VrhError) as e:
        _capi.check("vrh_render_volume", ctx.handle, vol.handle, rt.handle, cam, k)
    assert e.value.code == _capi.VRH_ERR_INVALID
    k.dt = 0.0
    rt2 = va.hip_buffer_rt(ctx, cam.width, cam.height)
    with pytest.raises(va.VrhError) as e:
        _capi.check("vrh_render_volume", ctx.handle, vol.handle, rt2.handle, cam, k)
    assert e.value.code == _capi.VRH_ERR_INVALID and "dt" in str(e.value)
    ctx.sync()
    rt.close(), rt2.close(), vol.close()
