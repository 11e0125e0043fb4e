"""CPU: the shared texture sampler (include/visionaray_hip/detail/vrh_texture.h) through vrh_tex2d_host
against the reference's own tex2D, the binary PNM reader, and model.load_textures().

tests/golden/tex2d_samples.npz holds direct tex2D calls of the reference (tests/golden/textured_ref.cpp, run
by make_textured_golden.py) over the textures, filters, address-mode pairs and coordinates of
tests/tex_cases.py.  Coordinates at which the reference read outside the texel array (found there with guard
texels of two colours) are marked dropped: on those the sampler must still return a value, from inside the
array.  Everything else is compared bit for bit.
"""
import functools
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import visionaray_amd as va
from visionaray_amd import _capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tex_cases as TC  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@functools.lru_cache(maxsize=None)
def samples():
    with np.load(os.path.join(HERE, "golden", "tex2d_samples.npz")) as z:
        return {k: z[k] for k in z.files}


def host_sample(w, h, f, ax, ay, coords, texels=None):
    tex = va.texture(TC.texels(w, h) if texels is None else texels, f, (ax, ay))
    return tex.tex2d(coords)


@pytest.mark.parametrize("cfg", TC.configs(), ids=lambda c: TC.config_key(*c))
def test_tex2d_host_equals_the_reference(cfg):
    w, h, f, ax, ay = cfg
    key = TC.config_key(*cfg)
    S = samples()
    coords = TC.coords(w, h)
    kept = np.unpackbits(S[key + "_kept"])[:len(coords)].astype(bool)
    assert kept[:TC.NUM_RANDOM].all(), "the fixture kept every random coordinate"
    assert int((~kept).sum()) == int(S["dropped"][TC.configs().index(cfg)])
    got = np.ascontiguousarray(host_sample(w, h, f, ax, ay, coords)).view(np.uint32).ravel()
    want = S[key]
    bad = np.flatnonzero(kept & (got != want))
    assert bad.size == 0, f"{key}: {bad.size} samples differ, first at {coords[bad[0]]}: {got[bad[0]]:08x} != {want[bad[0]]:08x}"


@pytest.mark.parametrize("cfg", [c for c in TC.configs()], ids=lambda c: TC.config_key(*c))
def test_dropped_samples_read_inside_the_array(cfg):
    """On the coordinates the fixture dropped, the sample must come from the array: texels of zeros between
    guard texels of 255 sample to zero -- nearest, or any interpolation of zeros -- unless a guard is read."""
    w, h, f, ax, ay = cfg
    S = samples()
    coords = TC.coords(w, h)
    kept = np.unpackbits(S[TC.config_key(*cfg) + "_kept"])[:len(coords)].astype(bool)
    if kept.all():
        return
    guard = 4 * (2 * w + 8)
    store = np.full(guard + w * h * 4 + guard, 255, np.uint8)
    inner = store[guard:guard + w * h * 4].reshape(h, w, 4)
    inner[...] = 0
    tex = va.texture(inner, f, (ax, ay))
    assert np.shares_memory(tex.pixels, store)
    assert np.all(tex.tex2d(coords[~kept]) == 0)


def test_formats_expand_like_the_loader():
    rgb = TC.texels(5, 3)[:, :, :3].copy()
    c = TC.coords(5, 3)[:300]
    rgba = np.concatenate([rgb, np.full((3, 5, 1), 255, np.uint8)], axis=2)
    assert np.array_equal(va.texture(rgb).tex2d(c), va.texture(rgba).tex2d(c))
    r = rgb[:, :, 0].copy()
    rrr = np.stack([r, r, r, np.full_like(r, 255)], axis=2)
    assert np.array_equal(va.texture(r).tex2d(c), va.texture(rrr).tex2d(c))


def test_dummy_and_errors():
    d = _capi.vrh_texture_desc()
    c = np.zeros((3, 2), np.float32)
    out = np.zeros((3, 4), np.uint8)
    p = lambda a: a.ctypes.data_as(_capi.C.c_void_p)
    L = _capi.lib()
    assert L.vrh_tex2d_host(_capi.C.byref(d), p(c), 3, p(out)) == _capi.VRH_OK and np.all(out == 255)
    tex = va.texture(TC.texels(2, 2))
    for field, value in (("format", 3), ("filter", 2)):
        d = tex.desc()
        setattr(d, field, value)
        assert L.vrh_tex2d_host(_capi.C.byref(d), p(c), 3, p(out)) == _capi.VRH_ERR_INVALID
    d = tex.desc()
    d.address[1] = 3
    assert L.vrh_tex2d_host(_capi.C.byref(d), p(c), 3, p(out)) == _capi.VRH_ERR_INVALID
    d = tex.desc()
    d.width = 32769
    assert L.vrh_tex2d_host(_capi.C.byref(d), p(c), 3, p(out)) == _capi.VRH_ERR_INVALID
    d = tex.desc()
    d.width, d.height = 32768, 16384        # 2^29 texels (the pixels are not read)
    assert L.vrh_tex2d_host(_capi.C.byref(d), p(c), 3, p(out)) == _capi.VRH_ERR_INVALID
    for bad in (np.inf, np.nan, 2.0 ** 20 + 1.0, -(2.0 ** 20) - 1.0):
        c2 = c.copy()
        c2[1, 1] = bad
        with pytest.raises(va.VrhError) as e:
            tex.tex2d(c2)
        assert e.value.code == _capi.VRH_ERR_INVALID
    tex.tex2d(np.float32([[2.0 ** 20, -(2.0 ** 20)]]))


# ---- PNM -------------------------------------------------------------------------------------------

def write_pnm(path, magic, w, h, maxv, data, comments=True):
    head = magic + b"\n"
    if comments:
        head += b"# a comment line\n"
    head += b"%d %d\n" % (w, h)
    if comments:
        head += b"#another\n# and one more\n"
    head += b"%d\n" % maxv
    with open(path, "wb") as f:
        f.write(head + bytes(data))


def test_pnm_reader(tmp_path):
    px = TC.texels(7, 5)[:, :, :3].copy()
    write_pnm(tmp_path / "a.ppm", b"P6", 7, 5, 255, px.tobytes())
    assert np.array_equal(va.load_pnm(tmp_path / "a.ppm"), px)
    write_pnm(tmp_path / "b.ppm", b"P6", 7, 5, 255, px.tobytes(), comments=False)
    assert np.array_equal(va.load_pnm(tmp_path / "b.ppm"), px)
    g = px[:, :, 0].copy()
    write_pnm(tmp_path / "g.pgm", b"P5", 7, 5, 255, g.tobytes())
    got = va.load_pnm(tmp_path / "g.pgm")
    assert got.shape == (5, 7, 1) and np.array_equal(got[:, :, 0], g)
    # max value 100: uint8(v * ((1.0 / max) * 255)), pnm_image.cpp:88-97
    low = (px % 101).astype(np.uint8)
    write_pnm(tmp_path / "c.ppm", b"P6", 7, 5, 100, low.tobytes())
    want = (low.astype(np.float64) * ((1.0 / 100) * 255)).astype(np.uint8)
    assert np.array_equal(va.load_pnm(tmp_path / "c.ppm"), want)
    write_pnm(tmp_path / "h.pgm", b"P5", 7, 5, 100, low[:, :, 1].tobytes())
    assert np.array_equal(va.load_pnm(tmp_path / "h.pgm")[:, :, 0], want[:, :, 1])
    # errors
    write_pnm(tmp_path / "t.ppm", b"P6", 7, 5, 255, px.tobytes()[:-1])
    write_pnm(tmp_path / "p3.ppm", b"P3", 1, 1, 255, b"1 2 3\n")
    (tmp_path / "x.png").write_bytes(b"\x89PNG\r\n\x1a\n" + b"\0" * 32)
    for name, code in (("t.ppm", _capi.VRH_ERR_INVALID), ("p3.ppm", _capi.VRH_ERR_UNSUPPORTED),
                       ("x.png", _capi.VRH_ERR_UNSUPPORTED), ("missing.ppm", _capi.VRH_ERR_INVALID)):
        with pytest.raises(va.VrhError) as e:
            va.load_pnm(tmp_path / name)
        assert e.value.code == code, name


OBJ = """mtllib scene.mtl
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
vt 0 0
vt 2 0
vt 2 2
vt 0 2
usemtl checker
f 1/1 2/2 3/3
usemtl gone
f 1/1 3/3 4/4
usemtl png
f 2/2 3/3 4/4
usemtl plain
f 1/1 2/2 4/4
usemtl again
f 1/1 2/2 3/3
"""
MTL = """newmtl checker
Kd 0.8 0.8 0.8
map_Kd maps\\checker.ppm
newmtl gone
Kd 0.5 0.5 0.5
map_Kd maps/not_there.ppm
newmtl png
Kd 0.5 0.5 0.5
map_Kd maps/image.png
newmtl plain
Kd 0.2 0.9 0.2
newmtl again
Kd 0.8 0.8 0.8
map_Kd maps\\checker.ppm
"""


def write_textured_obj(d):
    """a small OBJ + MTL + P6 set under directory d; returns the OBJ path and the map's pixels"""
    os.makedirs(os.path.join(d, "maps"), exist_ok=True)
    with open(os.path.join(d, "scene.obj"), "w") as f:
        f.write(OBJ)
    with open(os.path.join(d, "scene.mtl"), "w") as f:
        f.write(MTL)
    px = TC.texels(5, 3)[:, :, :3].copy()
    write_pnm(os.path.join(d, "maps", "checker.ppm"), b"P6", 5, 3, 255, px.tobytes())
    with open(os.path.join(d, "maps", "image.png"), "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + b"\0" * 32)
    return os.path.join(d, "scene.obj"), px


def test_model_load_textures(tmp_path):
    path, px = write_textured_obj(str(tmp_path))
    m = va.load_obj(path)
    by_name = dict(zip(m.material_names, range(len(m.material_names))))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        texs = m.load_textures()
    assert len(texs) == len(m.materials)
    t = texs[by_name["checker"]]
    assert t is not None and np.array_equal(t.pixels, px)
    assert t.filter == va.tex_filter.linear and t.address == (va.tex_address.wrap, va.tex_address.wrap)
    assert texs[by_name["again"]] is t, "a map shared by two materials is loaded once"
    assert texs[by_name["gone"]] is None and texs[by_name["png"]] is None and texs[by_name["plain"]] is None
    msgs = [str(w.message) for w in caught]
    assert len(msgs) == 2 and any("not_there.ppm" in s for s in msgs) and any("image.png" in s for s in msgs)


# ---- the sampler under the sanitizers, as a stand-alone host program ----------------------------------

def test_sampler_edge_list_under_sanitizers(tmp_path):
    exe = tmp_path / "tex2d_edge_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "tex2d_edge_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stdout.strip().splitlines()[-1].startswith("tex2d_edge_check ok"), r.stdout[-500:]
