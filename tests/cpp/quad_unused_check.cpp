// tests/cpp/quad_unused_check.cpp -- the never-hit boxes of unused 4-wide entries (vrh_quad.cpp build_quads with
// never_hit_unused, what the default build uploads; vrh_device.h NEVER_HIT_UNUSED), on the host.
//
//   1. records: hand-made binary trees of 3, 5, 6 and 7 leaves (split in halves) and a comb of 6 leaves, whose
//      4-wide records have 2, 3 and 4 children.  Every unused entry holds lo = hi = +inf on the three axes and the
//      link QUAD_NONE; every used entry and every link equals the build without never_hit_unused, whose unused
//      entries repeat entry 0's box.
//   2. rays: over every record of those trees, both forms of the entry test -- hardware min / max (vrh_device.h
//      quad_entry, here its host mirror fused::exact_entry) and the literal x < y ? x : y of the reference
//      (vrh_device.h tmin / tmax) -- each with and without the tn < FLT_MAX compare.  Direction components
//      positive, negative, tiny (1e-30 and minus the smallest value whose reciprocal is finite), huge (FLT_MAX) and
//      +-inf, whose reciprocal +-0 finite_ray admits; +-0, whose reciprocal is +-inf, finite_ray does NOT admit:
//      such rays are counted and left out, as the kernel leaves them to the binary records.  Origins inside the
//      boxes, on a bound, outside and at +-1e30; max_t from 1e-6 to FLT_MAX, and +inf for the forms that keep the
//      tn < FLT_MAX compare.  For every admitted ray: no unused entry passes the test WITHOUT the link compare,
//      and every entry gives what the old records gave WITH it (the same pass / fail, the same tn where it passes).
//   3. an inverted box (lo = +inf, hi = -inf) is NOT a never-hit box: it passes for some admitted ray.
// Prints one line per part; exit status 0 iff all hold.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "visionaray_hip/detail/vrh_fused_slab.h"
#include "../../visionaray_amd/csrc/vrh_internal.h"

namespace vrh { void set_error(const std::string&) {} }

namespace {

using vrh::node32;
using vrh::QUAD_NONE;

// vrh_device.h tmin / tmax (math/detail/math.h:48-60)
float tmin(float x, float y) { return x < y ? x : y; }
float tmax(float x, float y) { return x < y ? y : x; }

struct ray { float o[3], inv[3]; };

// vrh_device.h finite_ray
bool finite_ray(const ray& r)
{
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(r.inv[a]) || !std::isfinite(r.o[a])) return false;
    return true;
}

// form 0 / 1: hardware min / max with / without FINITE_MAX_T; 2 / 3: literal min / max, the same
bool entry_test(int form, const float* rec, uint32_t e, const ray& r, float max_t, float& tn)
{
    const float xl = rec[e], yl = rec[4 + e], zl = rec[8 + e], xh = rec[12 + e], yh = rec[16 + e], zh = rec[20 + e];
    if (form == 0)
        return vrh::fused::exact_entry<true>(xl, yl, zl, xh, yh, zh, r.o[0], r.o[1], r.o[2], r.inv[0], r.inv[1], r.inv[2], max_t, tn);
    if (form == 1)
        return vrh::fused::exact_entry<false>(xl, yl, zl, xh, yh, zh, r.o[0], r.o[1], r.o[2], r.inv[0], r.inv[1], r.inv[2], max_t, tn);
    const float t1x = (xl - r.o[0]) * r.inv[0], t1y = (yl - r.o[1]) * r.inv[1], t1z = (zl - r.o[2]) * r.inv[2];
    const float t2x = (xh - r.o[0]) * r.inv[0], t2y = (yh - r.o[1]) * r.inv[1], t2z = (zh - r.o[2]) * r.inv[2];
    tn = tmax(tmax(tmin(t1x, t2x), tmin(t1y, t2y)), tmin(t1z, t2z));
    const float tf = tmin(tmin(tmax(t1x, t2x), tmax(t1y, t2y)), tmax(t1z, t2z));
    if (form == 2) return (tf >= tn) & (tf >= 0.0f) & (tn < max_t);
    return (tf >= tn) & (tn < FLT_MAX) & (tf >= 0.0f) & (tn < max_t);
}

// A binary tree over `leaves` unit-ish boxes in a row along x (leaf i holds primitive i); the two children of a
// node are adjacent (bvh.h).  comb: every inner node's first child is a leaf.
struct tree
{
    std::vector<node32> nodes;
    void fill(uint32_t n, uint32_t lo, uint32_t hi, bool comb)       // node n covers leaves [lo, hi)
    {
        node32& me = nodes[n];
        me.bmin[0] = -2.0f + 0.75f * float(lo); me.bmax[0] = -2.0f + 0.75f * float(hi - 1) + 0.5f;
        me.bmin[1] = -1.0f; me.bmax[1] = 0.5f;
        me.bmin[2] = -0.25f; me.bmax[2] = 1.0f;
        if (hi - lo == 1)
        {
            // leaves differ on y and z too, inside the common bounds
            me.bmin[1] = -1.0f + 0.125f * float(lo % 3u); me.bmax[2] = 1.0f - 0.125f * float(lo % 2u);
            me.first = lo; me.num_prims = 1;
            return;
        }
        const uint32_t mid = comb ? lo + 1 : lo + (hi - lo) / 2;
        const uint32_t fc = uint32_t(nodes.size());
        nodes.resize(nodes.size() + 2);
        nodes[n].first = fc; nodes[n].num_prims = 0;
        fill(fc, lo, mid, comb);
        fill(fc + 1, mid, hi, comb);
    }
    tree(uint32_t leaves, bool comb) { nodes.resize(1); fill(0, 0, leaves, comb); }
};

struct built { std::vector<float> fresh, old; };        // with / without never_hit_unused

bool build(const tree& t, built& b)
{
    uint32_t root = 0, depth = 0;
    const uint32_t n = uint32_t(t.nodes.size());
    return vrh::build_quads(t.nodes.data(), n, b.fresh, root, depth, nullptr, true)
        && vrh::build_quads(t.nodes.data(), n, b.old, root, depth, nullptr, false)
        && b.fresh.size() == b.old.size() && !b.fresh.empty() && b.fresh.size() % 32 == 0;
}

uint32_t link_of(const float* rec, uint32_t e) { uint32_t l; std::memcpy(&l, &rec[24 + e], 4); return l; }

int part_records(const std::vector<built>& all, uint64_t (&by_children)[5])
{
    uint64_t bad = 0, unused = 0;
    for (const built& b : all)
        for (size_t q = 0; q < b.fresh.size() / 32; ++q)
        {
            const float* rn = &b.fresh[q * 32];
            const float* ro = &b.old[q * 32];
            uint32_t children = 0;
            for (uint32_t e = 0; e < 4; ++e)
            {
                bad += link_of(rn, e) != link_of(ro, e);
                if (link_of(rn, e) == QUAD_NONE)
                {
                    ++unused;
                    for (int a = 0; a < 6; ++a)
                    {
                        bad += !(rn[a * 4 + e] == INFINITY);
                        bad += !(ro[a * 4 + e] == ro[a * 4]);        // the old records repeat entry 0
                    }
                }
                else
                {
                    bad += children != e;                            // used entries are a prefix
                    ++children;
                    for (int a = 0; a < 6; ++a)
                        bad += std::memcmp(&rn[a * 4 + e], &ro[a * 4 + e], 4) != 0 || !std::isfinite(rn[a * 4 + e]);
                }
            }
            by_children[children] += 1;
        }
    std::printf("records: %llu with 2, %llu with 3, %llu with 4 children, %llu unused entries, %llu wrong\n",
                (unsigned long long)by_children[2], (unsigned long long)by_children[3], (unsigned long long)by_children[4],
                (unsigned long long)unused, (unsigned long long)bad);
    return (bad == 0 && by_children[0] == 0 && by_children[1] == 0 && by_children[2] > 0 && by_children[3] > 0
            && by_children[4] > 0) ? 0 : 1;
}

float tiniest_invertible()
{
    float d = 0x1p-128f;
    while (!std::isfinite(1.0f / d)) d = std::nextafter(d, 1.0f);
    return d;
}

int part_rays(const std::vector<built>& all, bool& inverted_passes)
{
    const float tiny = tiniest_invertible();
    const float dirs[] = { 1.0f, -1.0f, -0.7f, 1e-30f, -tiny, FLT_MAX, INFINITY, -INFINITY, 0.0f, -0.0f };
    // inside the row of boxes, on a lower / an upper bound, outside, far outside on either side
    const float oxs[] = { -1.75f, -2.0f, -3.0f, 1e30f, -1e30f };
    const float oys[] = { 0.0f, 2.0f, 1e30f };
    const float ozs[] = { 0.5f, -5.0f, -1e30f };
    const float max_ts[] = { 1e-6f, 8.0f, FLT_MAX, INFINITY };
    uint64_t rays = 0, not_admitted = 0, zero_inv = 0, unused_tests = 0, unused_pass = 0, used_tests = 0, used_pass = 0, differ = 0;
    uint64_t inv_pass = 0;
    float inverted[32];
    for (int a = 0; a < 3; ++a) { inverted[a * 4] = INFINITY; inverted[12 + a * 4] = -INFINITY; }
    for (float dx : dirs) for (float dy : dirs) for (float dz : dirs)
    for (float ox : oxs) for (float oy : oys) for (float oz : ozs)
    {
        ray r;
        r.o[0] = ox; r.o[1] = oy; r.o[2] = oz;
        r.inv[0] = 1.0f / dx; r.inv[1] = 1.0f / dy; r.inv[2] = 1.0f / dz;      // make_ray (intersect.inl:63)
        ++rays;
        if (!finite_ray(r)) { ++not_admitted; continue; }
        zero_inv += (r.inv[0] == 0.0f) | (r.inv[1] == 0.0f) | (r.inv[2] == 0.0f);
        for (float max_t : max_ts)
            for (int form = 0; form < 4; ++form)
            {
                if ((form == 0 || form == 2) && !(max_t <= FLT_MAX)) continue;   // FINITE_MAX_T: the host checked the radius
                for (const built& b : all)
                    for (size_t q = 0; q < b.fresh.size() / 32; ++q)
                        for (uint32_t e = 0; e < 4; ++e)
                        {
                            const float* rn = &b.fresh[q * 32];
                            const float* ro = &b.old[q * 32];
                            float tn_new, tn_old;
                            const bool h_new = entry_test(form, rn, e, r, max_t, tn_new);
                            const bool h_old = entry_test(form, ro, e, r, max_t, tn_old) & (link_of(ro, e) != QUAD_NONE);
                            if (link_of(rn, e) == QUAD_NONE) { ++unused_tests; unused_pass += h_new; }
                            else { ++used_tests; used_pass += h_new; }
                            differ += h_new != h_old;
                            if (h_new && h_old) differ += std::memcmp(&tn_new, &tn_old, 4) != 0;
                        }
                float tn;
                inv_pass += entry_test(form, inverted, 0, r, max_t, tn);
            }
    }
    inverted_passes = inv_pass > 0;
    std::printf("rays: %llu generated, %llu not admitted by finite_ray, %llu admitted with a zero reciprocal; unused entries: "
                "%llu tests, %llu pass; used entries: %llu tests, %llu pass; %llu differ from the compared records\n",
                (unsigned long long)rays, (unsigned long long)not_admitted, (unsigned long long)zero_inv,
                (unsigned long long)unused_tests, (unsigned long long)unused_pass, (unsigned long long)used_tests,
                (unsigned long long)used_pass, (unsigned long long)differ);
    std::printf("inverted box: %llu passes\n", (unsigned long long)inv_pass);
    return (unused_pass == 0 && differ == 0 && unused_tests > 0 && used_pass > 0 && used_pass < used_tests
            && not_admitted > 0 && zero_inv > 0) ? 0 : 1;
}

} // namespace

int main()
{
    std::vector<built> all;
    bool ok = true;
    for (uint32_t leaves : { 3u, 5u, 6u, 7u })
    {
        all.emplace_back();
        ok = ok && build(tree(leaves, false), all.back());
    }
    all.emplace_back();
    ok = ok && build(tree(6u, true), all.back());
    if (!ok) { std::printf("build_quads FAILED\nFAILED\n"); return 1; }
    uint64_t by_children[5] = {};
    int rc = part_records(all, by_children);
    bool inverted_passes = false;
    rc |= part_rays(all, inverted_passes);
    rc |= inverted_passes ? 0 : 1;
    std::printf(rc == 0 ? "ok\n" : "FAILED\n");
    return rc;
}
