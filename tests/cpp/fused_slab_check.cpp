// tests/cpp/fused_slab_check.cpp -- the fused slab test of detail/vrh_fused_slab.h against the exact one, and
// the upload side of the fused records (vrh_quad.cpp build_quads), on the host.
//
//   1. seeded ray / box cases: rays aimed at corners, edges and faces of boxes that are full or flat on one or
//      two axes, origins inside, on and outside the box out to O_max, one or two direction components scaled to
//      1e-6 or to the smallest value whose reciprocal is finite, coordinates from 1e-3 to 1e4, radius 0.1 and
//      FLT_MAX.  For every ray the kernel would let onto the fused records (ray_ok): if the exact test passes
//      on the exact box, the fused test passes on the widened box.  Non-vacuity: of those exact passes, the
//      share that FAILS the fused test on the unwidened box is printed (the wrapper demands >= 1 %).
//   2. a widened box contains its exact box; a point box at +inf passes for no ray of part 1.
//   3. build_quads: a nested tree gets fused records (same links, widened boxes, +inf unused entries, every
//      primitive's leaf slot naming its leaf's exact box); with one child bound one ulp outside its parent it
//      keeps its exact records and gets no fused ones.
// Prints one line per part; exit status 0 iff all hold.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "visionaray_hip/detail/vrh_fused_slab.h"
#include "../../visionaray_amd/csrc/vrh_internal.h"

namespace {

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rng()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}
float uni() { return (float)(rng() >> 8) * (1.0f / 16777216.0f); }           // [0, 1)
float sym() { return 2.0f * uni() - 1.0f; }                                  // [-1, 1)
float log_uniform(float lo, float hi) { return lo * std::pow(hi / lo, uni()); }

// the smallest positive float whose reciprocal is finite
float tiniest_invertible()
{
    float d = 0x1p-128f;
    while (!std::isfinite(1.0f / d)) d = std::nextafter(d, 1.0f);
    return d;
}

struct box { float lo[3], hi[3]; };

template <bool FIN>
bool exact_on(const box& b, const float o[3], const float inv[3], float max_t)
{
    float tn;
    return vrh::fused::exact_entry<FIN>(b.lo[0], b.lo[1], b.lo[2], b.hi[0], b.hi[1], b.hi[2], o[0], o[1], o[2],
                                        inv[0], inv[1], inv[2], max_t, tn);
}
template <bool FIN>
bool fused_on(const box& b, const float o[3], const float inv[3], float max_t)
{
    float tn;
    return vrh::fused::entry<FIN>(b.lo[0], b.lo[1], b.lo[2], b.hi[0], b.hi[1], b.hi[2], inv[0], inv[1], inv[2],
                                  -(o[0] * inv[0]), -(o[1] * inv[1]), -(o[2] * inv[2]), max_t, tn);
}

int part_cases()
{
    const float tiny = tiniest_invertible();
    const uint64_t N = 6000000;
    uint64_t eligible = 0, exact_pass = 0, plain_fused_fail = 0, bad = 0, contained_bad = 0, inf_pass = 0;
    uint64_t by_target[3] = {}, by_flat[3] = {}, by_origin[3] = {}, by_dir[4] = {}, by_radius[2] = {};
    for (uint64_t n = 0; n < N; ++n)
    {
        // coordinates of magnitude S, 1e-3 .. 1e4; the "scene" spans [-2 S, 2 S], origins within O_max = 4 S
        const float S = log_uniform(1e-3f, 1e4f);
        const float omax = 4.0f * S;
        box b;
        const uint32_t flat = rng() % 4u == 0u ? 1u + rng() % 2u : 0u;       // axes of zero extent
        const uint32_t flat_axis = rng() % 3u;
        for (uint32_t a = 0; a < 3; ++a)
        {
            const float c = S * sym();
            const bool is_flat = flat == 1u ? a == flat_axis : flat == 2u ? a != flat_axis : false;
            const float h = is_flat ? 0.0f : log_uniform(1e-3f, 1.0f) * S;
            b.lo[a] = c - h; b.hi[a] = c + h;
        }
        // the target: a corner, a point of an edge, a point of a face
        const uint32_t target = rng() % 3u;
        float tg[3];
        const uint32_t free_axis = rng() % 3u;
        for (uint32_t a = 0; a < 3; ++a)
        {
            const bool on_bound = target == 0u || (target == 1u ? a != free_axis : a == free_axis);
            tg[a] = on_bound ? ((rng() & 1u) ? b.lo[a] : b.hi[a]) : b.lo[a] + (b.hi[a] - b.lo[a]) * uni();
        }
        // the origin: inside the box, on it, or outside out to O_max
        const uint32_t where = rng() % 3u;
        float o[3];
        for (uint32_t a = 0; a < 3; ++a)
        {
            if (where == 0u) o[a] = b.lo[a] + (b.hi[a] - b.lo[a]) * uni();
            else if (where == 1u) o[a] = (rng() & 1u) ? ((rng() & 1u) ? b.lo[a] : b.hi[a]) : b.lo[a] + (b.hi[a] - b.lo[a]) * uni();
            else o[a] = (rng() % 8u == 0u) ? ((rng() & 1u) ? omax : -omax) : omax * sym() * ((rng() & 1u) ? 1.0f : 0.1f);
        }
        float d[3] = { tg[0] - o[0], tg[1] - o[1], tg[2] - o[2] };
        const float len = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        if (!(len > 0.0f)) { d[0] = sym(); d[1] = sym(); d[2] = sym(); }
        else for (float& x : d) x /= len;
        // one or two components scaled down to 1e-6, or to the smallest value that keeps inv finite
        const uint32_t dirmod = rng() % 4u;
        if (dirmod != 0u)
        {
            const uint32_t count = 1u + rng() % 2u, first = rng() % 3u;
            for (uint32_t k = 0; k < count; ++k)
            {
                float& x = d[(first + k) % 3u];
                if (dirmod == 1u) x *= 1e-6f;
                else if (dirmod == 2u) x = std::copysign(tiny, x);
                else x = std::copysign(1e-6f, x);
            }
        }
        float inv[3] = { 1.0f / d[0], 1.0f / d[1], 1.0f / d[2] };
        const uint32_t rsel = rng() & 1u;
        const float max_t = rsel ? FLT_MAX : 0.1f;

        box w;
        for (uint32_t a = 0; a < 3; ++a)
        {
            w.lo[a] = vrh::fused::widen_lo(b.lo[a], omax);
            w.hi[a] = vrh::fused::widen_hi(b.hi[a], omax);
            if (!(w.lo[a] <= b.lo[a] && w.hi[a] >= b.hi[a])) ++contained_bad;
        }
        if (!vrh::fused::ray_ok(o[0], o[1], o[2], inv[0], inv[1], inv[2], omax)) continue;
        ++eligible;
        box inf_box;
        for (uint32_t a = 0; a < 3; ++a) inf_box.lo[a] = inf_box.hi[a] = INFINITY;
        if (fused_on<true>(inf_box, o, inv, max_t) || fused_on<false>(inf_box, o, inv, max_t)) ++inf_pass;
        const bool fin = (n & 1u) != 0u;          // both forms of the test (with and without tn < FLT_MAX)
        const bool ex = fin ? exact_on<true>(b, o, inv, max_t) : exact_on<false>(b, o, inv, max_t);
        if (!ex) continue;
        ++exact_pass;
        ++by_target[target]; ++by_flat[flat]; ++by_origin[where]; ++by_dir[dirmod]; ++by_radius[rsel];
        if (!(fin ? fused_on<true>(b, o, inv, max_t) : fused_on<false>(b, o, inv, max_t))) ++plain_fused_fail;
        if (!(fin ? fused_on<true>(w, o, inv, max_t) : fused_on<false>(w, o, inv, max_t)))
        {
            if (++bad <= 5)
                std::printf("MISS S %g omax %g o %a %a %a d %a %a %a box %a %a %a .. %a %a %a max_t %g\n", S, omax, o[0], o[1], o[2],
                            d[0], d[1], d[2], b.lo[0], b.lo[1], b.lo[2], b.hi[0], b.hi[1], b.hi[2], max_t);
        }
    }
    std::printf("cases: %llu generated, %llu eligible, %llu exact passes, %llu of them fail the fused test on the exact box "
                "(%.2f %%), %llu fail it on the widened box\n",
                (unsigned long long)N, (unsigned long long)eligible, (unsigned long long)exact_pass,
                (unsigned long long)plain_fused_fail, 100.0 * double(plain_fused_fail) / double(exact_pass ? exact_pass : 1),
                (unsigned long long)bad);
    std::printf("kinds: corner %llu edge %llu face %llu | full %llu flat1 %llu flat2 %llu | inside %llu on %llu outside %llu | "
                "dir plain %llu x1e-6 %llu tiniest %llu 1e-6 %llu | radius 0.1 %llu FLT_MAX %llu\n",
                (unsigned long long)by_target[0], (unsigned long long)by_target[1], (unsigned long long)by_target[2],
                (unsigned long long)by_flat[0], (unsigned long long)by_flat[1], (unsigned long long)by_flat[2],
                (unsigned long long)by_origin[0], (unsigned long long)by_origin[1], (unsigned long long)by_origin[2],
                (unsigned long long)by_dir[0], (unsigned long long)by_dir[1], (unsigned long long)by_dir[2],
                (unsigned long long)by_dir[3], (unsigned long long)by_radius[0], (unsigned long long)by_radius[1]);
    std::printf("widened boxes: %llu not containing their exact box; +inf entry: %llu passes\n",
                (unsigned long long)contained_bad, (unsigned long long)inf_pass);
    bool kinds = true;
    for (uint64_t c : by_target) kinds = kinds && c > 0;
    for (uint64_t c : by_flat) kinds = kinds && c > 0;
    for (uint64_t c : by_origin) kinds = kinds && c > 0;
    for (uint64_t c : by_dir) kinds = kinds && c > 0;
    for (uint64_t c : by_radius) kinds = kinds && c > 0;
    return (bad == 0 && contained_bad == 0 && inf_pass == 0 && kinds && exact_pass >= 1000000) ? 0 : 1;
}

vrh::node32 inner(const float lo[3], const float hi[3], uint32_t first)
{
    vrh::node32 n{};
    for (int a = 0; a < 3; ++a) { n.bmin[a] = lo[a]; n.bmax[a] = hi[a]; }
    n.first = first; n.num_prims = 0;
    return n;
}
vrh::node32 leaf(const float lo[3], const float hi[3], uint32_t first, uint32_t count)
{
    vrh::node32 n = inner(lo, hi, first);
    n.num_prims = count;
    return n;
}

int part_upload()
{
    // root 0 -> (1 inner, 2 leaf); 1 -> (3 leaf, 4 leaf); leaves hold primitives [0,2) [2,3) [3,6)
    const float r_lo[3] = { -1, -1, -1 }, r_hi[3] = { 1, 1, 1 };
    const float a_lo[3] = { -1, -1, -1 }, a_hi[3] = { 0.25f, 1, 1 };
    const float b_lo[3] = { 0, -0.5f, -1 }, b_hi[3] = { 1, 1, 0.5f };
    const float c_lo[3] = { -1, -1, -1 }, c_hi[3] = { -0.5f, 0, 1 };
    const float d_lo[3] = { -0.75f, -1, 0 }, d_hi[3] = { 0.25f, 1, 1 };
    std::vector<vrh::node32> nodes = { inner(r_lo, r_hi, 1), inner(a_lo, a_hi, 3), leaf(b_lo, b_hi, 3, 3),
                                       leaf(c_lo, c_hi, 0, 2), leaf(d_lo, d_hi, 2, 1) };
    std::vector<float> quads;
    uint32_t root = 0, depth = 0;
    vrh::fused_records fz;
    fz.omax = 2.0f; fz.num_indices = 6;
    bool ok = vrh::build_quads(nodes.data(), 5, quads, root, depth, &fz) && fz.built;
    ok = ok && quads.size() == 32 && fz.recs.size() == 32 && fz.leaf_slot.size() == 6;
    if (ok)
    {
        // entries: 0 = node 3, 1 = node 4, 2 = node 2, 3 unused
        const uint32_t want_slot[6] = { 0, 0, 1, 2, 2, 2 };
        for (int i = 0; i < 6; ++i) ok = ok && fz.leaf_slot[i] == want_slot[i];
        ok = ok && std::memcmp(&quads[24], &fz.recs[24], 16) == 0;
        for (uint32_t e = 0; e < 3 && ok; ++e)
            for (int a = 0; a < 3; ++a)
            {
                const float lo = quads[a * 4 + e], hi = quads[12 + a * 4 + e];
                ok = ok && fz.recs[a * 4 + e] == vrh::fused::widen_lo(lo, 2.0f) && fz.recs[a * 4 + e] < lo;
                ok = ok && fz.recs[12 + a * 4 + e] == vrh::fused::widen_hi(hi, 2.0f) && fz.recs[12 + a * 4 + e] > hi;
            }
        for (int a = 0; a < 6; ++a) ok = ok && fz.recs[a * 4 + 3] == INFINITY;
        ok = ok && quads[3] == nodes[3].bmin[0];      // the exact records' unused entry repeats entry 0
    }
    std::printf("upload: nested tree %s\n", ok ? "gets fused records" : "FAILED");

    // the same records with an exaggerated widening
    vrh::fused_records fw;
    fw.omax = 2.0f; fw.num_indices = 6; fw.extra = 0.25f;
    std::vector<float> quads_w;
    bool okw = vrh::build_quads(nodes.data(), 5, quads_w, root, depth, &fw) && fw.built;
    okw = okw && quads_w.size() == quads.size() && std::memcmp(quads_w.data(), quads.data(), quads.size() * 4) == 0;
    okw = okw && fw.recs[0] == quads[0] - 0.25f && fw.recs[12] == quads[12] + 0.25f;
    std::printf("upload: widening option %s\n", okw ? "applies" : "FAILED");

    // node 1's upper x bound one ulp outside the root's: the 4-wide records stand (the skipped level still
    // nests), the fused ones are refused
    std::vector<vrh::node32> out = nodes;
    out[0].bmax[0] = 0.25f;                      // the root now ends where node 1 does ...
    out[2].bmax[0] = 0.25f; out[2].bmin[0] = 0.0f;
    out[1].bmax[0] = std::nextafter(0.25f, 1.0f);   // ... and node 1 one ulp beyond it
    out[4].bmax[0] = 0.25f;
    std::vector<float> quads2;
    vrh::fused_records f2;
    f2.omax = 2.0f; f2.num_indices = 6;
    const bool have = vrh::build_quads(out.data(), 5, quads2, root, depth, &f2);
    const bool ok2 = have && quads2.size() == 32 && !f2.built && f2.recs.empty() && f2.leaf_slot.empty();
    std::printf("upload: one ulp outside the parent %s\n", ok2 ? "keeps the exact records only" : "FAILED");
    return (ok && okw && ok2) ? 0 : 1;
}

} // namespace

namespace vrh { void set_error(const std::string&) {} }

int main()
{
    int rc = part_cases();
    rc |= part_upload();
    std::printf(rc == 0 ? "ok\n" : "FAILED\n");
    return rc;
}
