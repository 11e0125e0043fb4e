"""CPU: the oracle's generic-primitive mode (VO_GENERIC: triangles and spheres as 80-byte records in one BVH,
oracle/vrh_oracle.c) against the reference's own outputs, and the inputs of the randomized GPU sweep.

Pins, the bar tests/test_oracle.py holds the other kinds to: over each fixture tests/golden/gp_<case>.npz
(tests/golden/make_generic_primitive_golden.py: the reference's builder and kernels over
generic_primitive<triangle, sphere>) vo_build gives the reference's nodes and indices byte for byte, and the
primary, AO, simple and whitted frames over that tree equal the reference's bit for bit -- the denormal channels of
gp_example included.  gp_sweep is drawn by the generator of the GPU sweep (slivers, tiny and overlapping spheres,
the camera inside the cloud).  A generic list of one kind gives the bits of that kind's own mode.

Coverage of tests/test_gpu_fuzz_generic.py's inputs (tests/gp_cases.py sweep_case), on the oracle's frames alone: see
test_sweep_* below.  A seed base that misses a condition is refused (gp_cases.SWEEP_BASE records them).
"""
import ctypes as C

import numpy as np
import pytest

import gp_cases as G

f32 = np.float32


def fixture_scene(O, case):
    a = G.fixture(case)
    return G.oracle_scene(O, case, a["records"], a["nodes"], a["indices"], a["normals"], G.tree_depth(G.host_bvh(case).nodes))


@pytest.mark.parametrize("case", G.CASES)
def test_oracle_builds_the_reference_tree(oracle_mod, case):
    a = G.fixture(case)
    nodes, idx, depth = oracle_mod.build_bvh(a["records"], oracle_mod.VO_GENERIC)
    assert G.same_bits(nodes.view(np.uint32).reshape(-1, 8), a["nodes"])
    assert G.same_bits(idx, a["indices"])
    assert depth == G.tree_depth(G.host_bvh(case).nodes)


@pytest.mark.parametrize("case", G.CASES)
def test_oracle_frames_equal_the_reference_bit_for_bit(oracle_mod, case):
    O = oracle_mod
    a, s = G.fixture(case), G.spec()[case]
    sc = fixture_scene(O, case)
    cam = G.oracle_camera(a["camera"], s["W"], s["H"])
    out = {k: G.oracle_frame(O, sc, cam, k, s, a["materials"], a["lights"]) for k in G.KERNELS}
    hit = a["prim_id"] != G.MISS
    for k in G.KERNELS:
        assert np.array_equal(out[k]["prim_id"], a["prim_id"]), k
        assert G.same_bits(out[k]["t"], a["t"]), k
    bg = f32(s["bg"])
    assert G.same_bits(out["primary"]["color"], np.where(hit[:, None], f32(1.0), bg[None, :]).astype(f32))
    assert np.array_equal(out["ao"]["occ"], a["occ"])
    assert G.same_bits(out["ao"]["color"], a["ao_color"])
    assert G.same_bits(out["simple"]["color"], a["simple_color"])
    assert G.same_bits(out["whitted"]["color"], a["whitted_color"])
    # both kinds are in every frame compared, and so are the example's denormal channels
    sph = G.sphere_ids(a["records"])[np.where(hit, a["prim_id"], 0)] & hit
    assert sph.any() and (hit & ~sph).any() and not hit.all()
    for k in ("simple_color", "whitted_color"):
        n = int(((np.abs(a[k]) < np.finfo(f32).tiny) & (a[k] != 0.0)).sum())
        assert n == s["denormal_channels"][k]
    assert case != "gp_example" or s["denormal_channels"]["simple_color"] > 0


def test_gp_sweep_is_what_its_name_says():
    """slivers, tiny and overlapping spheres, the camera inside the cloud"""
    a = G.fixture("gp_sweep")
    r = a["records"]
    tri = np.ascontiguousarray(r["data"][r["type"] == 1]).view(f32).reshape(-1, 16)
    sph = np.ascontiguousarray(r["data"][r["type"] == 2]).view(f32).reshape(-1, 16)
    e1, e2 = tri[:, 8:11].astype(np.float64), tri[:, 12:15].astype(np.float64)
    sin = np.linalg.norm(np.cross(e1, e2), axis=1) / (np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1))
    assert (sin < 1e-3).any()
    c, rad = sph[:, 4:7].astype(np.float64), sph[:, 8].astype(np.float64)
    assert (rad < 3e-3).any()
    d = np.linalg.norm(c[:, None] - c[None], axis=2) - rad[:, None] - rad[None]
    assert (d[np.triu_indices(len(c), 1)] < 0.0).any()
    assert np.abs(a["camera"][0]).max() <= 0.5


def small_scene(seed, nt, ns):
    tris, sph = G.random_mixed(seed, nt, ns)
    cam = G.outside_camera(40, 30)
    return tris, sph, G.oracle_camera(cam, 40, 30)


def test_triangles_only_equal_the_triangle_mode(oracle_mod):
    O = oracle_mod
    tris, _, cam = small_scene(31, 200, 0)
    tris["geom_id"] = tris["prim_id"] % 3                     # the oracle's shade / whitted specs hold three materials
    gen = G.va.make_generic(tris, None)
    nodes, idx, depth = O.build_bvh(tris, O.VO_TRI)
    gn, gi, gd = O.build_bvh(gen, O.VO_GENERIC)
    assert G.same_bits(nodes.view(np.uint8), gn.view(np.uint8)) and G.same_bits(idx, gi) and depth == gd
    fn = O.face_normals(tris)
    plain = O.Scene("tri", O.VO_TRI, tris, nodes, idx, fn, depth)
    g = O.Scene("gen", O.VO_GENERIC, gen, nodes, idx, fn, depth)
    rng = np.random.default_rng(5)
    mask = (rng.uniform(0.0, 1.0, (3 * len(tris), 2)).astype(f32), (rng.random((8, 8)) < 0.5).astype(np.uint8))
    for hm in (None, mask):
        frames = [lambda s: O.render(s, cam, mode=O.VO_MODE_PRIMARY, hit_mask=hm),
                  lambda s: O.render(s, cam, mode=O.VO_MODE_AO, radius=0.3, hit_mask=hm),
                  lambda s: O.render_simple(s, cam, O.VO_NORMALS_PER_FACE, hit_mask=hm),
                  lambda s: O.render_whitted(s, cam, O.VO_NORMALS_PER_FACE, hit_mask=hm),
                  lambda s: O.render_multi(s, cam, O.VO_NORMALS_PER_FACE, max_hits=5, hit_mask=hm)]
        for f in frames:
            a, b = f(plain), f(g)
            assert set(a) == set(b)
            for k in a:
                assert (G.same_bits(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k]), k
            assert ((a["prim_id"] if "prim_id" in a else a["mh_prim_id"]) != G.MISS).any()
        if hm is not None:
            assert not np.array_equal(O.render(plain, cam, mode=O.VO_MODE_PRIMARY)["prim_id"], frames[0](plain)["prim_id"])


def primary_rays(cam):
    """origin and directions of the oracle's primary rays (sched_common.h:130-150), in its float operations"""
    eye, cu, cv, cw, W, H = cam
    x, y = np.meshgrid(np.arange(W, dtype=f32), np.arange(H, dtype=f32))
    u = (f32(2.0) * (x.reshape(-1) + f32(0.5)) / f32(W) - f32(1.0))[:, None]
    v = (f32(2.0) * (y.reshape(-1) + f32(0.5)) / f32(H) - f32(1.0))[:, None]
    return eye[None, :].astype(f32), normalize((cu[None, :] * u + cv[None, :] * v) + cw[None, :])


def dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def normalize(v):
    return v * (f32(1.0) / np.sqrt(dot(v, v)))[:, None]


def cross(u, v):
    return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)


def hit_normals(prims, normals, ref, ori, dirs):
    """(hit position, per-face normal) of every pixel's closest hit as the oracle's generic mode takes them: a
    triangle's from the table, a sphere's (isect_pos - center) / radius"""
    pid = np.where(ref["prim_id"] == G.MISS, 0, ref["prim_id"])
    pos = ori + dirs * ref["t"][:, None]
    words = np.ascontiguousarray(prims["data"]).view(f32).reshape(len(prims), 16)
    ids = np.ascontiguousarray(prims["data"]).view(np.uint32).reshape(len(prims), 16)[:, 1]
    row = np.zeros(len(prims), np.int64)
    row[ids] = np.arange(len(prims))                           # record of a prim id
    rec = words[row[pid]]
    n_sph = (pos - rec[:, 4:7]) / rec[:, 8:9]
    is_sphere = (prims["type"] == 2)[row[pid]]
    return pos, np.where(is_sphere[:, None], n_sph, normals[pid, :3]).astype(f32)


def test_spheres_only_equal_the_sphere_mode(oracle_mod):
    """primary visibility on every pixel.  AO: the sphere mode takes its normal from a table by prim id, the generic
    mode from the hit position, so the sphere mode renders pixel by pixel (vo_render_pixels), each with the analytic
    normal of that pixel's hit in its sphere's row."""
    O = oracle_mod
    _, sph, cam = small_scene(32, 0, 120)
    sph["radius"] *= f32(2.0)
    gen = G.va.make_generic(None, sph)
    nodes, idx, depth = O.build_bvh(sph, O.VO_SPHERE)
    gn, gi, gd = O.build_bvh(gen, O.VO_GENERIC)
    assert G.same_bits(nodes.view(np.uint8), gn.view(np.uint8)) and G.same_bits(idx, gi) and depth == gd
    table = np.zeros((len(sph), 4), f32)
    plain = O.Scene("sph", O.VO_SPHERE, sph, nodes, idx, table, depth)
    g = O.Scene("gen", O.VO_GENERIC, gen, nodes, idx, np.zeros((len(sph), 4), f32), depth)
    a, b = O.render(plain, cam, mode=O.VO_MODE_PRIMARY), O.render(g, cam, mode=O.VO_MODE_PRIMARY)
    for k in ("prim_id", "t", "color", "list_index"):
        assert G.same_bits(a[k], b[k]), k
    hit = a["prim_id"] != G.MISS
    assert hit.any() and not hit.all()
    ao = O.render(g, cam, mode=O.VO_MODE_AO, radius=0.4, samples=8, frame_num=3)
    ori, dirs = primary_rays(cam)
    _, n = hit_normals(gen, np.zeros((len(sph), 4), f32), ao, ori, dirs)
    for p in np.flatnonzero(hit):
        table[:] = 0.0
        table[ao["prim_id"][p], :3] = n[p]
        one = O.render_pixels(plain, cam, [p], mode=O.VO_MODE_AO, radius=0.4, samples=8, frame_num=3)
        assert one["prim_id"][0] == ao["prim_id"][p] and one["occ"][0] == ao["occ"][p], p
        assert G.same_bits(one["color"][0], ao["color"][p]) and G.same_bits(one["t"][:1], ao["t"][p:p + 1]), p
    assert ao["occ"].any() and (ao["occ"][hit] != 255).any()


def test_what_the_generic_mode_has_no_restatement_of_is_refused(oracle_mod):
    """the per-vertex binding and the path tracer: a stated return, nothing written (the product refuses both)"""
    O = oracle_mod
    sc = fixture_scene(O, "gp_soup")
    a, s = G.fixture("gp_soup"), G.spec()["gp_soup"]
    cam = G.oracle_camera(a["camera"], s["W"], s["H"])
    sc.vertex_normals = np.zeros((3 * len(a["records"]), 4), f32)
    for render in (O.render_simple, O.render_whitted):
        out = render(sc, cam, O.VO_NORMALS_PER_VERTEX)
        assert out["rays"] == 0 and (out["prim_id"] == G.MISS).all() and not out["color"].any()
    assert not O.render_multi(sc, cam, O.VO_NORMALS_PER_VERTEX, max_hits=4)["color"].any()
    m = np.ascontiguousarray(a["materials"]).view(f32).reshape(-1).view(O.PLASTIC_DTYPE)
    with pytest.raises(ValueError):
        O.render_pathtracing(sc, cam, O.VO_NORMALS_PER_FACE, m, (1.0, 1.0, 1.0, 1.0), (0.0, 0.0, 0.0, 1.0), 3, 1e-3)
    assert O.render(sc, cam, mode=O.VO_MODE_PATHTRACING, materials=m, num_bounces=3)["rays"] == 0


# ---- the inputs of the GPU sweep ----------------------------------------------------------------------------

def test_sweep_cases_are_what_the_sweep_promises():
    cases = [G.sweep_case(i) for i in G.SWEEP_SEEDS]
    assert len(cases) == 32
    nt = np.array([len(c["tris"]) for c in cases])
    ns = np.array([int(c["is_sphere"].sum()) for c in cases])
    assert (nt <= 3000).all() and (ns <= 2000).all() and nt.max() > 2000 and ns.max() > 1500
    assert ((ns == 0) & (nt > 1)).sum() >= 2 and ((nt == 0) & (ns > 1)).sum() >= 2
    assert ((nt + ns < 8) & (nt + ns > 1)).sum() >= 2
    assert ((nt == 1) & (ns == 0)).any() and ((nt == 0) & (ns == 1)).any()
    for c in cases:
        ids = np.ascontiguousarray(c["prims"]["data"]).view(np.uint32).reshape(-1, 16)
        assert np.array_equal(ids[:, 1], np.arange(len(ids))) and np.array_equal(ids[:, 0], np.arange(len(ids)) % 4)
    wh = np.array([(c["W"], c["H"]) for c in cases])
    assert (wh >= 1).all() and (wh[:, 0] <= 140).all() and (wh[:, 1] <= 90).all()
    assert (wh.min(axis=1) < 8).sum() >= 3 and (wh == 1).all(axis=1).any() and (wh % 8 != 0).any(axis=1).sum() >= 16
    assert [c["kind"] for c in cases] == G.KERNELS * 8
    opts = [c["option"] for c in cases if c["option"]]
    assert 3 * len(opts) >= len(cases)
    assert {o[0] for o in opts} == {"block_threads", "wide_anyhit", "ao_cut", "ao_gate", "exact_minmax", "xcd_queues", "descent_cap",
                                     "pop_on_miss", "scalar_fetch", "refill_min"}
    assert {o[1] for o in opts if o[0] == "block_threads"} == {128, 256}
    for kind in ("ao", "whitted"):
        assert any(c["kind"] == kind and c["option"] == ("block_threads", 256) for c in cases)
    assert {c["spec"]["ao_samples"] for c in cases if c["kind"] == "ao"} <= {1, 2, 3, 5, 8, 32}
    assert len({c["spec"]["frame_num"] for c in cases}) > 8 and all(0 <= c["spec"]["frame_num"] < 50 for c in cases)
    for c in cases:
        m = np.ascontiguousarray(c["materials"]).view(f32).reshape(-1, 13)
        assert (m[:, 4:7] * m[:, 7:8] > 0.0).all() and 1 <= len(c["lights"]) <= 3      # a diffuse part in every channel


def degenerate(c):
    """a case that cannot be asked for hits and misses: fewer than 8 primitives, or fewer pixels than one 8 x 8 tile"""
    return len(c["prims"]) < 8 or c["W"] * c["H"] < 64


def test_sweep_frames_hold_hits_misses_and_both_kinds(oracle_mod):
    closest = {k: set() for k in G.KERNELS}
    mixed = 0
    for i in G.SWEEP_SEEDS:
        c = G.sweep_case(i)
        sc, ref = G.sweep_reference(i)
        hit = ref["prim_id"] != G.MISS
        closest[c["kind"]] |= set(np.unique(c["is_sphere"][ref["prim_id"][hit]]).tolist())
        if not degenerate(c):
            assert hit.any() and not hit.all(), i
        if c["kind"] == "ao" and not degenerate(c):
            bits = np.unpackbits(ref["occ"][hit][:, None], axis=1, bitorder="little")[:, :min(c["spec"]["ao_samples"], 8)]
            assert bits.any() and not bits.all(), i
        mixed += G.mixed_leaves(sc.nodes, sc.indices, c["prims"]) > 0
        assert np.isfinite(ref["color"]).all(), i
    assert all(v == {False, True} for v in closest.values()), closest
    assert 2 * mixed >= len(G.SWEEP_SEEDS)


class vo_hit(C.Structure):
    _fields_ = [("hit", C.c_int), ("prim_id", C.c_uint32), ("geom_id", C.c_uint32), ("list_index", C.c_uint32),
                ("t", C.c_float), ("u", C.c_float), ("v", C.c_float)]


def tracer(O, sc):
    """trace(origin, direction, any_hit, max_t) -> (hit, prim id): vo_intersect over the scene's tree"""
    fn = O.lib().vo_intersect
    fn.restype = vo_hit
    fn.argtypes = [C.POINTER(C.c_float)] * 2 + [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_float, C.c_void_p]
    f3 = C.c_float * 3
    nodes, idx, prims = (a.ctypes.data_as(C.c_void_p) for a in (sc.nodes, sc.indices, sc.prims))

    def trace(o, d, any_hit, max_t):
        h = fn(f3(*map(float, o)), f3(*map(float, d)), nodes, idx, prims, sc.kind, any_hit, max_t, None)
        return bool(h.hit), int(h.prim_id)
    return trace


FLT_MAX = float(np.finfo(f32).max)
PROBES = 400        # rays looked at per seed


def ao_rays(c, ref, pos, n, pixels, smp):
    """the oracle's AO ray `smp` of the hit pixels `pixels` (shade_pixel_at, in its float operations)"""
    n, pos = n[pixels], pos[pixels]
    wide = np.abs(n[:, 0]) > np.abs(n[:, 1])
    z = np.zeros(len(n), f32)
    bv = normalize(np.where(wide[:, None], np.stack([-n[:, 2], z, n[:, 0]], 1), np.stack([z, n[:, 2], -n[:, 1]], 1)))
    bu = cross(bv, n)
    sx, sy = np.zeros(len(n), f32), np.zeros(len(n), f32)
    frame = c["spec"]["frame_num"]
    for j, p in enumerate(pixels):
        for kk in range(16):
            ctr = (((int(p) * 8 + int(smp[j])) * 16 + kk) * 2 + frame * 0x9E3779B1) & 0xFFFFFFFF
            xa, ya = f32(2.0) * uniform(ctr) - f32(1.0), f32(2.0) * uniform((ctr + 1) & 0xFFFFFFFF) - f32(1.0)
            if xa * xa + ya * ya < f32(1.0):
                sx[j], sy[j] = xa, ya
                break
    sz = np.sqrt(np.maximum(f32(0.0), f32(1.0) - sx * sx - sy * sy))
    d = normalize((bu * sx[:, None] + bv * sy[:, None]) + n * sz[:, None])
    return pos + d * f32(c["spec"]["ao_eps"]), d


def wang(a):
    a = (a ^ 61) ^ (a >> 16)
    a = (a + (a << 3)) & 0xFFFFFFFF
    a = a ^ (a >> 4)
    a = (a * 0x27d4eb2d) & 0xFFFFFFFF
    return a ^ (a >> 15)


def uniform(k):
    return f32(wang(k) >> 8) * f32(1.0 / 16777216.0)


def test_sweep_ao_rays_and_reflections_cross_kinds(oracle_mod):
    """at least two AO seeds have a sphere occluding a ray from a triangle's surface and two the reverse; at least two
    whitted seeds reflect from one kind onto the other.  The rays are the oracle's, formed again here in its float
    operations for up to PROBES pixels per seed and traced with vo_intersect; every AO ray formed for a set mask bit
    must be occluded, or the rays here are not the oracle's."""
    O = oracle_mod
    sphere_from_tri, tri_from_sphere, reflect = set(), set(), set()
    for i in G.SWEEP_SEEDS:
        c = G.sweep_case(i)
        if c["kind"] not in ("ao", "whitted"):
            continue
        sc, ref = G.sweep_reference(i)
        ori, dirs = primary_rays(G.oracle_camera(c["camera"], c["W"], c["H"]))
        pos, n = hit_normals(c["prims"], c["normals"], ref, ori, dirs)
        trace = tracer(O, sc)
        hit = ref["prim_id"] != G.MISS
        if c["kind"] == "ao":
            samples = min(c["spec"]["ao_samples"], 8)          # the mask holds the first 8 samples
            bits = np.unpackbits(ref["occ"][:, None], axis=1, bitorder="little")[:, :samples]
            px, smp = np.nonzero(bits & hit[:, None])
            px, smp = px[:PROBES], smp[:PROBES]
            o, d = ao_rays(c, ref, pos, n, px, smp)
            for j in range(len(px)):
                h, pid = trace(o[j], d[j], 1, c["spec"]["ao_radius"])
                assert h, (i, int(px[j]), int(smp[j]))
                a, b = c["is_sphere"][ref["prim_id"][px[j]]], c["is_sphere"][pid]
                if b and not a:
                    sphere_from_tri.add(i)
                if a and not b:
                    tri_from_sphere.add(i)
        elif c["spec"]["bounces"] >= 2:
            # whitted.inl:64-77: reflect(view, shading normal) from the first hit, origin pos + dir * eps
            px = np.flatnonzero(hit)[:PROBES]
            view = -dirs[px]
            rd = n[px] * (f32(2.0) * dot(n[px], view))[:, None] - view
            o = pos[px] + rd * f32(c["spec"]["eps"])
            for j in range(len(px)):
                h, pid = trace(o[j], rd[j], 0, FLT_MAX)
                if h and c["is_sphere"][pid] != c["is_sphere"][ref["prim_id"][px[j]]]:
                    reflect.add(i)
    assert len(sphere_from_tri) >= 2 and len(tri_from_sphere) >= 2, (sphere_from_tri, tri_from_sphere)
    assert len(reflect) >= 2, reflect
