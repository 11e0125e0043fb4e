"""The randomized cases of the path tracer's sweep, shared by tests/test_oracle_pathtracing.py (CPU: the
oracle against the reference generator, the usability caps) and tests/test_gpu_fuzz_pathtracing.py (GPU
against the oracle).  Everything here is a function of the seed alone.

A case: a triangle scene (the soup of test_gpu_fuzz, or a closed room with the camera inside), 3 to 5
plastics by geom_id = i % n, ambient / background, normal binding, bounce count, epsilon, a frame
number from the whole u32 range, an image size and three cameras.  The frames compared are those of
FRAMES: one frame, three frames in flight (three cameras, consecutive frame numbers), one through the
jittered sampler and two jittered_blend frames onto a random target.

Tolerance of a case that can reach powf (derived from the oracle alone, the method of
tests/golden/make_pathtrace_golden.py): every frame is rendered with the C library's powf (A), every
powf result one float up (B) and one float down (C).  A pixel is stable when its path signature is the
same in A, B and C; sens = the largest relative colour difference A-B / A-C over the stable hit
pixels; rtol = 2 * sens.  A case is usable when on every frame at most MAX_UNSTABLE of the hit pixels
are unstable and rtol <= MAX_RTOL.

Measured (the frame with the largest value of each case; GPU: an MI355X, largest relative difference
over all frames, every frame's share of hit pixels within its rtol):

    seed  family  bounces  unstable  sens      rtol      GPU max rel  GPU share
       3  room    4        0.00062   1.09e-03  2.19e-03  3.49e-04     1.0000
      10  soup    4        0.00054   2.46e-03  4.91e-03  4.89e-04     0.9995
      14  soup    2        0         1.96e-04  3.92e-04  1.91e-04     1.0000
      19  room    4        0         3.41e-03  6.82e-03  4.87e-04     1.0000
      22  soup    2        0         1.38e-04  2.76e-04  1.43e-05     1.0000
      30  soup    3        0         2.47e-03  4.93e-03  1.02e-04     1.0000
      35  room    3        0         9.64e-04  1.93e-03  7.70e-05     1.0000
    2, 6, 7, 11, 23 (0 or 1 bounce: the colour does not depend on powf): all 0, GPU bit-identical
    0, 1, 4, 5, 8, 9, 12, 13, 16, 17, 20, 21 cannot reach powf: GPU bit-identical, ray totals equal

The one pixel of seed 10 outside its tolerance (a channel that is 0 in the oracle is -3.7e-9 on the GPU)
takes another path there: the oracle gives the GPU's colour when the first powf(x, 0.5) of that path
alone is one float lower.  The uniform shift does not find every such pixel, so they count against the
99 % share, as in tests/test_gpu_pathtracing.py.
"""
import functools

import numpy as np

import visionaray_amd as va
from test_gpu_fuzz import _camera, _ocam, _scene

MISS = 0xFFFFFFFF
MAX_UNSTABLE = 0.0025     # make_pathtrace_golden.MAX_UNSTABLE
MAX_RTOL = 1e-2           # the committed fixtures have 1.5e-3 and 4.3e-3
MAX_TRIS = 3000
EXPS = (0.0, 1.0, 8.5, 64.0, 500.0)
BOUNCES = (0, 1, 2, 3, 5, 10, 17)
EPSILONS = (1e-4, 1e-3, 1e-2)
FRAMES = ("single", "flight0", "flight1", "flight2", "jittered", "blend")

# Seeds of the sweep.  A seed whose powf case breaks a cap above is replaced by another seed, never
# relaxed (tests/test_oracle_pathtracing.py test_sweep_cases_are_usable prints the table).
# Replaced so far: 15 (rtol 7.6e-2) by 35, 18 (rtol 1.35e-2) by 30.
SEEDS = [s for s in range(24) if s not in (15, 18)] + [30, 35]


def _room(rng):
    """12 triangles of the box [-1, 1]^3 with randomly flipped winding around a few hundred random ones"""
    q = np.float32([[[-1, -1, -1], [1, -1, -1], [1, -1, 1], [-1, -1, 1]], [[-1, 1, -1], [-1, 1, 1], [1, 1, 1], [1, 1, -1]],
                    [[-1, -1, -1], [-1, 1, -1], [1, 1, -1], [1, -1, -1]], [[-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]],
                    [[-1, -1, -1], [-1, -1, 1], [-1, 1, 1], [-1, 1, -1]], [[1, -1, -1], [1, 1, -1], [1, 1, 1], [1, -1, 1]]])
    v1 = np.concatenate([q[:, 0], q[:, 0]])
    e1 = np.concatenate([q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]])
    e2 = np.concatenate([q[:, 2] - q[:, 0], q[:, 3] - q[:, 0]])
    flip = rng.random(12) < 0.5
    e1[flip], e2[flip] = e2[flip].copy(), e1[flip].copy()
    n = int(rng.integers(100, 500))
    c = rng.uniform(-0.9, 0.9, (n, 3))
    size = 10.0 ** rng.uniform(-2.0, -0.7, (n, 1))
    f1, f2 = rng.standard_normal((n, 3)) * size, rng.standard_normal((n, 3)) * size
    return va.make_triangles(np.concatenate([v1, c - 0.5 * (f1 + f2)]), np.concatenate([e1, f1]), np.concatenate([e2, f2]))


def _room_camera(rng, W, H):
    cam = va.camera()
    cam.perspective(float(rng.uniform(0.5, 1.6)), np.float32(W) / np.float32(H), 0.001, 1000.0)
    cam.look_at(tuple(float(x) for x in rng.uniform(-0.7, 0.7, 3)), tuple(float(x) for x in rng.uniform(-1.0, 1.0, 3)),
                (0.0, 1.0, 0.0))
    return cam


def _material(rng, family):
    m = np.zeros(1, va.PLASTIC_DTYPE)
    m["ca"], m["ka"] = rng.uniform(0.0, 1.0, 3), rng.uniform(0.0, 1.0)      # unused by the path tracer
    m["cd"], m["kd"] = rng.uniform(0.1, 1.0, 3), rng.uniform(0.3, 1.0)
    m["cs"], m["ks"] = rng.uniform(0.1, 1.0, 3), rng.uniform(0.2, 1.0)
    m["exp"] = EXPS[int(rng.integers(len(EXPS)))]
    if family == "diffuse":
        m["ks"] = 0.0
    elif family == "specular":
        m["kd"] = 0.0
    elif family == "zero":
        m["cd"], m["cs"] = 0.0, 0.0
    return m


def powf_free(materials):
    """no path of the case reaches powf: prob_spec is 0 and prob_diff is not (plastic.inl:203-216)"""
    cd = (materials["cd"][:, 0] + materials["cd"][:, 1] + materials["cd"][:, 2]) / np.float32(3.0) * materials["kd"]
    cs = (materials["cs"][:, 0] + materials["cs"][:, 1] + materials["cs"][:, 2]) / np.float32(3.0) * materials["ks"]
    return bool(np.all(cs == 0.0) and np.all(cd > 0.0))


@functools.lru_cache(maxsize=None)
def draw_case(seed):
    rng = np.random.default_rng(5000 + seed)
    family = "room" if seed % 2 else "soup"
    prims = _room(rng) if family == "room" else _scene(rng, "tri")[:MAX_TRIS].copy()
    W, H = int(rng.integers(9, 121)), int(rng.integers(7, 81))
    cams = [(_room_camera if family == "room" else _camera)(rng, W, H) for _ in range(3)]
    nmat = int(rng.integers(3, 6))
    if seed % 4 < 2:                                    # half of the cases cannot reach powf
        fams = ["diffuse"] * nmat
    else:
        fams = [("diffuse", "specular", "mixed", "zero")[int(rng.integers(4))] for _ in range(nmat)]
        fams[int(rng.integers(nmat))] = ("specular", "mixed", "zero")[int(rng.integers(3))]
    materials = np.concatenate([_material(rng, f) for f in fams])
    prims["geom_id"] = np.arange(len(prims), dtype=np.uint32) % nmat
    free = powf_free(materials)
    bounces = BOUNCES[int(rng.integers(len(BOUNCES)))]
    case = {
        "seed": seed, "family": family, "prims": prims, "W": W, "H": H, "cams": cams, "materials": materials,
        "families": fams, "powf_free": free, "num_bounces": bounces if free else min(bounces, 4),
        "ambient": tuple(float(np.float32(x)) for x in list(rng.uniform(0.0, 2.0, 3)) + [rng.uniform(0.0, 1.0)]),
        "bg": tuple(float(np.float32(x)) for x in rng.uniform(0.0, 1.0, 4)),
        "per_vertex": bool(rng.random() < 0.5),
        "eps": EPSILONS[int(rng.integers(len(EPSILONS)))],
        "frame_num": int(rng.integers(0, 1 << 32)),
        "blend_first": int(rng.integers(1, 9)),            # jittered_blend weighs a frame with 1 / frame_num
        "init": rng.uniform(0.05, 1.0, (W * H, 4)).astype(np.float32),
    }
    prims.setflags(write=False)
    materials.setflags(write=False)
    case["init"].setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def _oracle_scene(O, seed):
    prims = draw_case(seed)["prims"]
    fn = va.face_normals(prims)
    nodes, indices, depth = O.build_bvh(prims.view(O.TRI_DTYPE), O.VO_TRI)
    return O.Scene("pt%d" % seed, O.VO_TRI, prims, nodes, indices, fn, depth, O.vertex_normals(fn))


def oracle_scene(O, case):
    """the oracle's scene of a case over the oracle's own build (tree-identical to the product's: test_capi)"""
    return _oracle_scene(O, case["seed"])


def ocams(case):
    return [_ocam(c.basis(case["W"], case["H"]), case["W"], case["H"]) for c in case["cams"]]


def oracle_frame(O, sc, case, which, pow_shift=0):
    """the oracle's frame `which` (one of FRAMES) of a case"""
    cams = ocams(case)
    binding = O.VO_NORMALS_PER_VERTEX if case["per_vertex"] else O.VO_NORMALS_PER_FACE
    kw = dict(binding=binding, materials=case["materials"], ambient=case["ambient"], bg=case["bg"],
              num_bounces=case["num_bounces"], eps=case["eps"], pow_shift=pow_shift)
    fn = case["frame_num"]
    if which == "single":
        return O.render_pathtracing(sc, cams[0], frame_num=fn, **kw)
    if which.startswith("flight"):
        f = int(which[6:])
        return O.render_pathtracing(sc, cams[f], frame_num=(fn + f) & 0xFFFFFFFF, **kw)
    if which == "jittered":
        return O.render_pathtracing(sc, cams[0], frame_num=fn, sampler="jittered", init=case["init"], **kw)
    first = O.render_pathtracing(sc, cams[0], frame_num=case["blend_first"], sampler="jittered_blend", init=case["init"], **kw)
    last = O.render_pathtracing(sc, cams[0], frame_num=case["blend_first"] + 1, sampler="jittered_blend",
                                init=first["color"], **kw)
    # a pixel's path of the blend: both frames' signatures
    last["sig"] = last["sig"] ^ (first["sig"] * np.uint64(0x9E3779B97F4A7C15))
    last["rays_first"] = first["rays"]
    # prim_id / t are the last frame's; a pixel's colour holds a path when either frame hit
    last["lit"] = (first["prim_id"] != MISS) | (last["prim_id"] != MISS)
    return last


def rel_diff(a, b):
    """|a - b| / |a| per rgb channel; a channel that is 0 in a and not in b counts as infinite"""
    a, b = a[:, :3].astype(np.float64), b[:, :3].astype(np.float64)
    rel = np.abs(a - b) / np.where(a == 0.0, 1.0, np.abs(a))
    rel[(a == 0.0) & (b != 0.0)] = np.inf
    return rel


@functools.lru_cache(maxsize=None)
def reference(O, seed, which):
    """(the oracle's frame A, {unstable, sens, rtol, hits}) of frame `which` of a case; computed once"""
    case = draw_case(seed)
    sc = oracle_scene(O, case)
    if case["powf_free"]:
        A = B = C = oracle_frame(O, sc, case, which, 0)
    else:
        A, B, C = (oracle_frame(O, sc, case, which, s) for s in (0, +1, -1))
    hit = A.get("lit", A["prim_id"] != MISS)
    stable = (A["sig"] == B["sig"]) & (A["sig"] == C["sig"])
    sel = hit & stable
    sens = 0.0
    for other in (B, C):
        rel = rel_diff(A["color"][sel], other["color"][sel])
        assert np.isfinite(rel).all(), "a channel that is 0 with the C library's powf is not 0 with the moved powf"
        sens = max(sens, float(rel.max()) if rel.size else 0.0)
    for a in A.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return A, {"unstable": float(np.sum(hit & ~stable)) / max(1, int(hit.sum())), "sens": sens, "rtol": 2.0 * sens,
               "hits": int(hit.sum())}


def check_frame(got, ref, tol, free, label):
    """The sweep's bar for one frame.  prim_id / t bit-identical; a powf-free case: colour
    bit-identical; any other: misses bit-identical and at least 99 % of the hit pixels within rtol with
    their zero channels exactly zero (the bar of the fixtures in tests/test_gpu_pathtracing.py).
    Returns the largest finite relative difference (0 when bit-identical)."""
    assert np.array_equal(got["prim_id"], ref["prim_id"]), f"{label}: prim_id"
    assert np.array_equal(got["t"].view(np.uint32), ref["t"].view(np.uint32)), f"{label}: t"
    gb, rb = got["color"].view(np.uint32), ref["color"].view(np.uint32)
    hit = ref.get("lit", ref["prim_id"] != MISS)
    if free:
        bad = np.any(gb != rb, axis=1)
        assert not bad.any(), f"{label}: {int(bad.sum())} of {bad.size} pixels differ (first {int(np.argmax(bad))})"
        return 0.0
    assert np.array_equal(gb[~hit], rb[~hit]), f"{label}: miss pixels"
    if not hit.any():
        return 0.0
    # as tests/test_gpu_pathtracing.py applies it to the fixtures: a channel that is 0 in the reference and not
    # in the frame makes its pixel miss the tolerance (infinite difference), whatever rtol is
    rel = rel_diff(ref["color"][hit], got["color"][hit])
    assert np.array_equal(gb[hit][:, 3], rb[hit][:, 3]), f"{label}: alpha"
    ok = np.all(rel <= tol["rtol"], axis=1)
    finite = rel[np.isfinite(rel)]
    worst = float(finite.max()) if finite.size else 0.0
    print(f"{label}: {ok.mean():.5f} of {ok.size} hit pixels within rtol {tol['rtol']:.3e}, max rel {worst:.3e}, "
          f"pixels with a zero channel that is not zero {int((~np.isfinite(rel)).any(axis=1).sum())}, "
          f"bit-identical {np.mean(np.all(gb[hit] == rb[hit], axis=1)):.4f}")
    assert ok.mean() >= 0.99, f"{label}: only {ok.mean():.4f} of the hit pixels are within rtol {tol['rtol']:.3e}"
    return worst
