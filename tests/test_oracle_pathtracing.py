"""CPU: the oracle's path-tracing mode (VO_MODE_PATHTRACING, oracle/vrh_oracle.c) pinned to the reference.

The committed fixtures (tests/golden/pt_*.npz: frames of the reference's own pathtracing::kernel) and,
where oracle/_ref/pathtrace_ref is built, the generator itself on the cases of the GPU sweep
(tests/pt_cases.py) at pow_shift 0, +1 and -1: colours, per-pixel ray counts, path signatures and
totals bit-identical.  Then the usability caps of the sweep's powf cases, and properties of the mode.
"""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import pt_cases as P  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
GEN = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "pathtrace_ref")
MISS = 0xFFFFFFFF
with open(os.path.join(GOLDEN, "pathtrace.json")) as _f:
    PT = json.load(_f)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def fixture_frame(O, g, frame_num, **kw):
    sc = O.make_shade_scene(g["scene"])
    m, _, _, bg = O.whitted_spec()
    m = m.copy()
    if g["materials"] == "diffuse":
        m["ks"] = 0.0
    binding = O.VO_NORMALS_PER_VERTEX if g["binding"] == "vertex" else O.VO_NORMALS_PER_FACE
    return O.render_pathtracing(sc, O.scene_camera(g["scene"], g["W"], g["H"]), binding, m, g["ambient"], bg,
                                g["bounces"], g["eps"], frame_num=frame_num, **kw)


@pytest.mark.parametrize("case,fr", [(c, f) for c in ("pt_cornell12_diffuse", "pt_hfstack_diffuse", "pt_hf64_vertex_diffuse")
                                     for f in PT[c]["frames"]])
def test_diffuse_fixtures_are_bit_identical(oracle_mod, case, fr):
    g = PT[case]
    out = fixture_frame(oracle_mod, g, fr)
    ref = np.load(os.path.join(GOLDEN, case + ".npz"))["color_f%d" % fr]
    assert np.array_equal(bits(out["color"]), bits(ref))
    assert out["rays"] == g["rays"][str(fr)] == int(out["nrays"].sum())


def test_blend_fixture_is_bit_identical(oracle_mod):
    g = PT["pt_cornell12_blend"]
    ref = np.load(os.path.join(GOLDEN, "pt_cornell12_blend.npz"))
    target, total = np.zeros((g["W"] * g["H"], 4), np.float32), 0
    for n in range(g["first_frame"], g["first_frame"] + g["num_frames"]):
        out = fixture_frame(oracle_mod, g, n, sampler="jittered_blend", init=target)
        target, total = out["color"], total + out["rays"]
        if n == g["first_frame"]:
            assert np.array_equal(bits(target), bits(ref["color_first"]))
    assert np.array_equal(bits(target), bits(ref["color_last"]))
    assert total == g["rays_total"]


@pytest.mark.parametrize("case", ["pt_cornell12_plastic2", "pt_cornell12_plastic"])
def test_plastic_fixtures_within_their_tolerance(oracle_mod, case):
    """the bar tests/test_gpu_pathtracing.py applies to the GPU (same host libm here: expect 1.0)"""
    g = PT[case]
    fr = g["frames"][0]
    out = fixture_frame(oracle_mod, g, fr)
    ref = np.load(os.path.join(GOLDEN, case + ".npz"))["color_f%d" % fr]
    hit = out["prim_id"] != MISS
    assert hit.any() and np.array_equal(bits(out["color"][~hit]), bits(ref[~hit]))
    got, want = out["color"][hit].astype(np.float64), ref[hit].astype(np.float64)
    rel = np.abs(got - want) / np.where(want == 0.0, 1.0, np.abs(want))
    rel[(want == 0.0) & (got != 0.0)] = np.inf          # a zero channel must stay exactly zero
    assert np.isfinite(rel).all()
    ok = np.all(rel <= g["rtol_spec"], axis=1)
    print(f"{case}: {ok.mean():.5f} of {ok.size} hit pixels within rtol_spec {g['rtol_spec']:.3e}; bit-identical "
          f"{np.mean(np.all(bits(out['color'][hit]) == bits(ref[hit]), axis=1)):.4f}; rays {out['rays']} / {g['rays'][str(fr)]}")
    assert ok.mean() >= 0.99


# ---- the generator itself on the sweep cases ---------------------------------------------------------

def generator_frame(O, case, cam, frame_num, accum, pow_shift):
    import make_pathtrace_golden as G
    prims = case["prims"]
    fn = P.va.face_normals(prims)
    normals = O.vertex_normals(fn) if case["per_vertex"] else fn
    return G.run_ref_arrays(prims, normals, case["per_vertex"], case["materials"], cam[:4], case["W"], case["H"],
                            case["ambient"], case["bg"], case["eps"], case["num_bounces"], frame_num, accum, pow_shift)


@pytest.mark.skipif(not os.path.exists(GEN), reason="oracle/_ref/pathtrace_ref is not built (no reference tree here)")
@pytest.mark.parametrize("seed", P.SEEDS)
def test_sweep_cases_equal_the_reference_generator(oracle_mod, seed):
    """oracle and generator on the same host (same powf), same tree (both builders are tree-identical)"""
    O = oracle_mod
    case = P.draw_case(seed)
    sc = P.oracle_scene(O, case)
    cams = P.ocams(case)
    for shift in (0, +1, -1):
        out = P.oracle_frame(O, sc, case, "single", shift)
        colors, sig, rays, total = generator_frame(O, case, cams[0], case["frame_num"], 0, shift)
        assert np.array_equal(bits(out["color"]), bits(colors[0])), shift
        assert np.array_equal(out["nrays"], rays) and np.array_equal(out["sig"], sig), shift
        assert out["rays"] == total, shift
    # the sampler path: two jittered_blend frames (the generator's target starts at 0)
    binding = O.VO_NORMALS_PER_VERTEX if case["per_vertex"] else O.VO_NORMALS_PER_FACE
    kw = dict(binding=binding, materials=case["materials"], ambient=case["ambient"], bg=case["bg"],
              num_bounces=case["num_bounces"], eps=case["eps"], sampler="jittered_blend")
    first = O.render_pathtracing(sc, cams[0], frame_num=case["blend_first"], **kw)
    last = O.render_pathtracing(sc, cams[0], frame_num=case["blend_first"] + 1, init=first["color"], **kw)
    colors, sig, rays, total = generator_frame(O, case, cams[0], case["blend_first"], 2, 0)
    assert np.array_equal(bits(first["color"]), bits(colors[0])) and np.array_equal(bits(last["color"]), bits(colors[1]))
    assert np.array_equal(last["nrays"], rays) and np.array_equal(last["sig"], sig)
    assert first["rays"] + last["rays"] == total


# ---- the sweep's cases are usable --------------------------------------------------------------------

def test_sweep_covers_what_it_is_for():
    cases = [P.draw_case(s) for s in P.SEEDS]
    fams = {f for c in cases for f in c["families"]}
    assert fams == {"diffuse", "specular", "mixed", "zero"}
    assert {c["family"] for c in cases} == {"soup", "room"}
    assert {float(m["exp"]) for c in cases for m in c["materials"]} == set(P.EXPS)
    assert any(c["powf_free"] and c["num_bounces"] >= 10 and c["family"] == "room" for c in cases)
    assert any(not c["powf_free"] and c["num_bounces"] >= 3 for c in cases)
    assert any(c["per_vertex"] for c in cases) and any(not c["per_vertex"] for c in cases)
    assert any(c["frame_num"] * c["W"] * c["H"] >= 1 << 32 for c in cases)
    assert all(len(c["prims"]) <= P.MAX_TRIS and 9 <= c["W"] <= 120 and 7 <= c["H"] <= 80 for c in cases)
    assert any(c["W"] % 8 and c["H"] % 8 for c in cases)
    for c in cases:
        assert c["powf_free"] == all(f == "diffuse" for f in c["families"])
        assert c["powf_free"] or c["num_bounces"] <= 4


def test_sweep_cases_are_usable(oracle_mod):
    """every case that can reach powf, every frame the GPU sweep compares: unstable share <= 0.25 %
    and rtol <= 1e-2, from the oracle alone"""
    O = oracle_mod
    print("\nseed family  WxH     tris bounces  frame       unstable   sens       rtol")
    broken = []
    for seed in P.SEEDS:
        case = P.draw_case(seed)
        if case["powf_free"]:
            continue
        for which in P.FRAMES:
            _, tol = P.reference(O, seed, which)
            print(f"{seed:4d} {case['family']:5s} {case['W']:3d}x{case['H']:<3d} {len(case['prims']):5d} {case['num_bounces']:4d}    "
                  f"{which:9s}  {tol['unstable']:.5f}   {tol['sens']:.3e}  {tol['rtol']:.3e}")
            if tol["unstable"] > P.MAX_UNSTABLE or tol["rtol"] > P.MAX_RTOL:
                broken.append((seed, which, tol))
    assert not broken, broken


def test_powf_free_cases_do_not_depend_on_powf(oracle_mod):
    O = oracle_mod
    for seed in P.SEEDS:
        case = P.draw_case(seed)
        if not case["powf_free"]:
            continue
        sc = P.oracle_scene(O, case)
        a, b = P.oracle_frame(O, sc, case, "single", 0), P.oracle_frame(O, sc, case, "single", +1)
        assert np.array_equal(bits(a["color"]), bits(b["color"])) and np.array_equal(a["sig"], b["sig"])


# ---- properties ---------------------------------------------------------------------------------------

def room_case(O, W=40, H=30, specular_exp=None):
    """the Cornell box from inside; specular_exp: one purely specular material of that exponent"""
    sc = O.make_shade_scene("cornell12")
    m, _, _, bg = O.whitted_spec()
    m = m.copy()
    if specular_exp is None:
        m["ks"] = 0.0
    else:
        m["kd"], m["exp"] = 0.0, specular_exp
    return sc, O.scene_camera("cornell12", W, H), m, bg


def test_zero_bounces_is_background_and_traces_no_ray(oracle_mod):
    O = oracle_mod
    sc, cam, m, bg = room_case(O)
    out = O.render_pathtracing(sc, cam, O.VO_NORMALS_PER_FACE, m, (0.7, 1.3, 0.2, 0.9), bg, 0, 1e-3)
    assert np.array_equal(out["color"], np.tile(np.float32(bg), (len(out["color"]), 1)))
    assert out["rays"] == 0 and not out["nrays"].any()
    prim = O.render(sc, cam, mode=O.VO_MODE_PRIMARY)
    assert np.array_equal(out["prim_id"], prim["prim_id"]) and np.array_equal(bits(out["t"]), bits(prim["t"]))
    assert (out["prim_id"] != MISS).any()


def test_one_bounce_is_black_on_hits(oracle_mod):
    O = oracle_mod
    sc, cam, m, bg = room_case(O)
    out = O.render_pathtracing(sc, cam, O.VO_NORMALS_PER_FACE, m, (0.7, 1.3, 0.2, 0.9), bg, 1, 1e-3)
    hit = out["prim_id"] != MISS
    assert hit.any() and (~hit).any()
    assert np.array_equal(out["color"][hit], np.tile(np.float32([0, 0, 0, 1]), (int(hit.sum()), 1)))
    assert np.array_equal(out["color"][~hit], np.tile(np.float32(bg), (int((~hit).sum()), 1)))
    assert out["rays"] == out["color"].shape[0]


def test_a_path_dies_by_a_non_positive_pdf(oracle_mod):
    """a purely specular material of exponent 0 samples half vectors over the whole hemisphere: for some
    dot(wo, h) <= 0, so pdf <= 0 (brdf.h:151-152) and the path ends after its first ray although that ray hit"""
    O = oracle_mod
    sc, cam, m, bg = room_case(O, specular_exp=0.0)
    out = O.render_pathtracing(sc, cam, O.VO_NORMALS_PER_FACE, m, (1.0, 1.0, 1.0, 1.0), bg, 4, 1e-3)
    died = (out["prim_id"] != MISS) & (out["nrays"] == 1)
    assert died.any()
    assert np.array_equal(out["color"][died], np.tile(np.float32([0, 0, 0, 1]), (int(died.sum()), 1)))
    assert ((out["prim_id"] != MISS) & (out["nrays"] == 4)).any()


def seed_hash(a):
    """cuda_sched.inl:27-36"""
    M = 0xFFFFFFFF
    a = ((a + 0x7ed55d16) + (a << 12)) & M
    a = ((a ^ 0xc761c23c) ^ (a >> 19)) & M
    a = ((a + 0x165667b1) + (a << 5)) & M
    a = (((a + 0xd3a2646c) & M) ^ (a << 9)) & M
    a = ((a + 0xfd7046c5) + (a << 3)) & M
    a = ((a ^ 0xb55a4f09) ^ (a >> 16)) & M
    return a


def seed_hash_inverse(h):
    """the hash is a bijection of u32 (every step is): the a with seed_hash(a) == h"""
    M = 0xFFFFFFFF

    def unxorshift(v, c, s):            # v = (a ^ c) ^ (a >> s)
        v ^= c
        a = v
        for _ in range(32 // s + 1):
            a = v ^ (a >> s)
        return a & M

    def unaddshift(v, c, s):            # v = (a + c) + (a << s) = a * (1 + 2^s) + c
        return ((v - c) * pow(1 + (1 << s), -1, 1 << 32)) & M

    def unaddxor(v, c, s):              # v = (a + c) ^ (a << s): bit by bit from the low end
        a = 0
        for i in range(32):
            for b in (0, 1):
                cand = a | (b << i)
                if (((cand + c) & M) ^ ((cand << s) & M)) & ((2 << i) - 1) == v & ((2 << i) - 1):
                    a = cand
                    break
        return a

    a = unxorshift(h, 0xb55a4f09, 16)
    a = unaddshift(a, 0xfd7046c5, 3)
    a = unaddxor(a, 0xd3a2646c, 9)
    a = unaddshift(a, 0x165667b1, 5)
    a = unxorshift(a, 0xc761c23c, 19)
    a = unaddshift(a, 0x7ed55d16, 12)
    assert seed_hash(a) == h
    return a


def wrapping_frames(W, H, p):
    """(n0, n1): frame numbers of a W x H image (W * H odd) that give pixel p the seeds 2^31 - 1 (0 mod
    2^31 - 1: the engine state becomes 1) and 1 (state 1 too); n * W * H wraps in 32 bits for both"""
    inv = pow(W * H, -1, 1 << 32)
    n0 = ((seed_hash_inverse(0x7FFFFFFF) - p) * inv) & 0xFFFFFFFF
    n1 = ((seed_hash_inverse(1) - p) * inv) & 0xFFFFFFFF
    for n, want in ((n0, 0x7FFFFFFF), (n1, 1)):
        assert n * W * H >= 1 << 32 and seed_hash((n * W * H + p) & 0xFFFFFFFF) == want
    return n0, n1


def test_a_seed_that_is_zero_mod_the_modulus_and_a_wrapping_frame_number(oracle_mod):
    """minstd_rand0 seeded with 0 mod 2^31 - 1 starts from state 1, like one seeded with 1: the two
    frames give pixel p the same random numbers, so the same colour and path; the other pixels differ"""
    O = oracle_mod
    W, H = 9, 7
    sc, cam, m, bg = room_case(O, W, H)
    p = 3 * W + 4
    n0, n1 = wrapping_frames(W, H, p)
    a = O.render_pathtracing(sc, cam, O.VO_NORMALS_PER_FACE, m, (0.7, 1.3, 0.2, 0.9), bg, 6, 1e-3, frame_num=n0)
    b = O.render_pathtracing(sc, cam, O.VO_NORMALS_PER_FACE, m, (0.7, 1.3, 0.2, 0.9), bg, 6, 1e-3, frame_num=n1)
    assert a["prim_id"][p] != MISS and a["nrays"][p] >= 2 and a["color"][p, :3].any()
    assert np.array_equal(bits(a["color"][p]), bits(b["color"][p])) and a["sig"][p] == b["sig"][p]
    hit = a["prim_id"] != MISS
    assert np.any(bits(a["color"][hit]) != bits(b["color"][hit]))
    assert np.isfinite(a["color"]).all()


def test_rows_scissor_and_ssaa(oracle_mod):
    O = oracle_mod
    sc, cam, m, bg = room_case(O)
    W, H = cam[4], cam[5]
    args = (sc, cam, O.VO_NORMALS_PER_FACE, m, (0.7, 1.3, 0.2, 0.9), bg, 5, 1e-3)
    whole = O.render_pathtracing(*args, frame_num=7)
    rows = O.render_pathtracing(*args, frame_num=7, rows=(8, 19))
    box = O.render_pathtracing(*args, frame_num=7, scissor=(5, 3, 33, 21))
    y, x = np.arange(W * H) // W, np.arange(W * H) % W
    for got, sel in ((rows, (y >= 8) & (y < 19)), (box, (x >= 5) & (x < 33) & (y >= 3) & (y < 21))):
        assert np.array_equal(bits(got["color"][sel]), bits(whole["color"][sel]))
        assert np.array_equal(got["sig"][sel], whole["sig"][sel])
        assert not got["color"][~sel].any() and np.all(got["prim_id"][~sel] == MISS)
        assert got["rays"] == int(whole["nrays"][sel].sum())
    jit = O.render_pathtracing(*args, frame_num=7, sampler="jittered")
    jbox = O.render_pathtracing(*args, frame_num=7, sampler="jittered", scissor=(5, 3, 33, 21), init=(0.5, 0.25, 0.125, 1.0))
    sel = (x >= 5) & (x < 33) & (y >= 3) & (y < 21)
    assert np.array_equal(bits(jbox["color"][sel]), bits(jit["color"][sel]))
    assert np.array_equal(jbox["color"][~sel], np.tile(np.float32([0.5, 0.25, 0.125, 1.0]), (int((~sel).sum()), 1)))
    assert np.any(bits(jit["color"]) != bits(whole["color"]))
    with pytest.raises(ValueError):
        O.render_pathtracing(*args, sampler="ssaa4")


def test_powf_shift_moves_one_float_and_keeps_exact_results(oracle_mod):
    L = oracle_mod.lib()
    r = np.float32(L.vo_powf(0.3, 8.5, 0))
    assert np.float32(L.vo_powf(0.3, 8.5, +1)) == np.nextafter(r, np.float32(np.inf))
    assert np.float32(L.vo_powf(0.3, 8.5, -1)) == np.nextafter(r, np.float32(-np.inf))
    for x, y in ((0.3, 0.0), (1.0, 8.5), (0.0, 8.5), (1e-30, 64.0), (1e30, 64.0)):
        assert L.vo_powf(x, y, +1) == L.vo_powf(x, y, 0) == L.vo_powf(x, y, -1), (x, y)


def test_sincos_are_the_restated_ones(oracle_mod):
    """vrh_libm.h's host build (equal to glibc's on all inputs: tests/test_libm_sincosf.py): spot values"""
    import math
    L = oracle_mod.lib()
    for x in (0.0, 1e-5, 0.5, 1.0, 3.0, 6.2831855, 100.0, 1e6):
        x = float(np.float32(x))
        assert abs(L.vo_libm_sinf(x) - math.sin(x)) <= 1.2e-7 and abs(L.vo_libm_cosf(x) - math.cos(x)) <= 1.2e-7
