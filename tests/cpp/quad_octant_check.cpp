// tests/cpp/quad_octant_check.cpp -- the octant form of the 4-wide entry test (vrh_octant.h octant::entry, what the AO
// kernel's step runs) against the sorting form (vrh_device.h quad_entry<true>, here its host mirror
// fused::exact_entry<true> and a restatement that also returns tf), on the host.
//
// Every case is one entry of a 128-byte record as vrh_quad.cpp lays it out, read the way the kernel reads it: the near
// piece of an axis at byte near_piece(inv), the far piece at far_piece(inv).  Compared per case: pass / fail, tn as a
// value and tf as a value (+0 and -0 are equal; NaN equals NaN -- only the never-hit box under a zero reciprocal
// gives one, on both sides).
//
//   1. random: boxes with lo <= hi and rays with a finite origin and a finite inverse direction, the same number in
//      each of the eight octants; magnitudes from 2^-20 to 2^20, a share of the boxes flat on one axis, a share of
//      the origins on a plane of the box.
//   2. edges, all combinations of: box planes (ordinary, flat on 1, 2 and 3 axes, subnormal extents, +-FLT_MAX), origins
//      (inside, exactly on the lower / upper plane, next to a plane so that the difference underflows, far away),
//      inv (+-1, +-FLT_MAX, +-FLT_MIN, +-0) per axis, radius (0, 1e-6, 1, FLT_MAX); and the never-hit box lo = hi = +inf.
// Prints one line per part; exit status 0 iff all hold; the last line is then "ok".
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "visionaray_hip/detail/vrh_fused_slab.h"
#include "visionaray_hip/detail/vrh_octant.h"

namespace {

struct ray { float o[3], inv[3]; };

// vrh_device.h quad_entry<true>, tf returned too
bool sorted_entry(const float* lo, const float* hi, const ray& r, float max_t, float& tn, float& tf)
{
    const float t1x = (lo[0] - r.o[0]) * r.inv[0], t1y = (lo[1] - r.o[1]) * r.inv[1], t1z = (lo[2] - r.o[2]) * r.inv[2];
    const float t2x = (hi[0] - r.o[0]) * r.inv[0], t2y = (hi[1] - r.o[1]) * r.inv[1], t2z = (hi[2] - r.o[2]) * r.inv[2];
    tn = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(t1x, t2x), __builtin_fminf(t1y, t2y)), __builtin_fminf(t1z, t2z));
    tf = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(t1x, t2x), __builtin_fmaxf(t1y, t2y)), __builtin_fmaxf(t1z, t2z));
    return (tf >= tn) & (tf >= 0.0f) & (tn < max_t);
}

bool same_value(float a, float b) { return a == b || (std::isnan(a) && std::isnan(b)); }

struct tally { uint64_t cases = 0, pass = 0, differ = 0, mirror_differ = 0, nan_cases = 0, zero_sign = 0; uint64_t octant[8] = {}; };

// entry e of a record holding the box [lo, hi]; the other entries hold a box no case uses
void one_case(const float* lo, const float* hi, uint32_t e, const ray& r, float max_t, tally& t)
{
    alignas(16) float rec[32];
    for (int i = 0; i < 32; ++i) rec[i] = 12345.0f;
    for (int a = 0; a < 3; ++a) { rec[4 * a + e] = lo[a]; rec[12 + 4 * a + e] = hi[a]; }
    const unsigned char* b = reinterpret_cast<const unsigned char*>(rec);
    float nf[2][3];
    for (int a = 0; a < 3; ++a)
    {
        std::memcpy(&nf[0][a], b + 16u * a + vrh::octant::near_piece(r.inv[a]) + 4u * e, 4);
        std::memcpy(&nf[1][a], b + 16u * a + vrh::octant::far_piece(r.inv[a]) + 4u * e, 4);
    }
    float tn_o, tf_o, tn_s, tf_s, tn_m;
    const bool h_o = vrh::octant::entry<true>(nf[0][0], nf[0][1], nf[0][2], nf[1][0], nf[1][1], nf[1][2], r.o[0], r.o[1], r.o[2],
                                              r.inv[0], r.inv[1], r.inv[2], max_t, tn_o, tf_o);
    const bool h_s = sorted_entry(lo, hi, r, max_t, tn_s, tf_s);
    const bool h_m = vrh::fused::exact_entry<true>(lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], r.o[0], r.o[1], r.o[2],
                                                   r.inv[0], r.inv[1], r.inv[2], max_t, tn_m);
    t.cases += 1;
    t.pass += h_o;
    t.differ += (h_o != h_s) || !same_value(tn_o, tn_s) || !same_value(tf_o, tf_s);
    t.mirror_differ += (h_m != h_s) || std::memcmp(&tn_m, &tn_s, 4) != 0;
    t.nan_cases += std::isnan(tn_s) || std::isnan(tf_s);
    t.zero_sign += (tn_o == tn_s && std::signbit(tn_o) != std::signbit(tn_s)) || (tf_o == tf_s && std::signbit(tf_o) != std::signbit(tf_s));
    t.octant[(r.inv[0] < 0.0f) | ((r.inv[1] < 0.0f) << 1) | ((r.inv[2] < 0.0f) << 2)] += 1;
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;      // xorshift64
    return uint32_t(rng_state >> 32);
}
float unit() { return float(rnd() >> 8) * 0x1p-24f; }                                   // [0, 1)
float signed_mag(int emin, int emax)                                                     // +-(1 + u) 2^e
{
    const float m = std::ldexp(1.0f + unit(), emin + int(rnd() % uint32_t(emax - emin + 1)));
    return (rnd() & 1u) ? -m : m;
}

int part_random(uint64_t per_octant)
{
    tally t;
    for (uint32_t oct = 0; oct < 8; ++oct)
        for (uint64_t i = 0; i < per_octant; ++i)
        {
            float lo[3], hi[3];
            ray r;
            const uint32_t kind = rnd() % 16u;
            for (int a = 0; a < 3; ++a)
            {
                const float c = signed_mag(-20, 20), w = std::fabs(signed_mag(-20, 20));
                lo[a] = c; hi[a] = c + w;                                   // c + w >= c under round to nearest
                if (kind == uint32_t(a)) hi[a] = lo[a];                     // flat on one axis
                r.o[a] = kind == 4u + uint32_t(a) ? lo[a] : kind == 7u + uint32_t(a) ? hi[a]       // on a plane
                       : (rnd() & 1u) ? lo[a] + (hi[a] - lo[a]) * unit() : signed_mag(-20, 20);     // inside / anywhere
                const float d = std::fabs(signed_mag(-20, 20));
                r.inv[a] = ((oct >> a) & 1u) ? -(1.0f / d) : 1.0f / d;
            }
            const float radii[] = { 0.1f, 8.0f, 1e6f, FLT_MAX };
            one_case(lo, hi, rnd() % 4u, r, radii[rnd() % 4u], t);
        }
    bool even = true;
    for (int o = 0; o < 8; ++o) even = even && t.octant[o] == per_octant;
    std::printf("random: %llu cases, %llu per octant, %llu pass, %llu differ, %llu differ from the mirror\n",
                (unsigned long long)t.cases, (unsigned long long)per_octant, (unsigned long long)t.pass,
                (unsigned long long)t.differ, (unsigned long long)t.mirror_differ);
    return (even && t.differ == 0 && t.mirror_differ == 0 && t.pass > 0 && t.pass < t.cases) ? 0 : 1;
}

int part_edges()
{
    tally t, never;
    uint64_t skipped = 0;
    const float sub = 0x1p-149f;                                     // the smallest subnormal
    // (lo, hi) per axis: ordinary, flat, a subnormal extent at 0 and at 1 (the latter rounds to flat), huge
    const float planes[][2] = { { -1.0f, 2.0f }, { 0.5f, 0.5f }, { 0.0f, sub }, { -sub, sub }, { 0.0f, 0.0f }, { -0.0f, 0.0f },
                                { 1.0f, 1.0f + FLT_EPSILON }, { -FLT_MAX, FLT_MAX }, { FLT_MAX, FLT_MAX } };
    const float invs[] = { 1.0f, -1.0f, FLT_MAX, -FLT_MAX, FLT_MIN, -FLT_MIN, 0.0f, -0.0f, 3.0f, -0x1p-140f };
    const float radii[] = { 0.0f, 1e-6f, 1.0f, FLT_MAX };
    const int NP = int(sizeof planes / sizeof planes[0]), NI = int(sizeof invs / sizeof invs[0]);
    for (int px = 0; px < NP; ++px) for (int py = 0; py < NP; ++py) for (int pz = 0; pz < NP; pz += 2)
    for (int ix = 0; ix < NI; ++ix) for (int iy = 0; iy < NI; ++iy) for (int iz = (ix + iy) % 3; iz < NI; iz += 3)
    for (int ok = 0; ok < 6; ++ok)
    {
        const float lo[3] = { planes[px][0], planes[py][0], planes[pz][0] }, hi[3] = { planes[px][1], planes[py][1], planes[pz][1] };
        ray r;
        r.inv[0] = invs[ix]; r.inv[1] = invs[iy]; r.inv[2] = invs[iz];
        for (int a = 0; a < 3; ++a)
        {
            // on the lower plane, on the upper plane, one step below the lower plane (lo - o underflows or is one
            // unit in the last place), one step above the upper, the middle, far outside
            r.o[a] = ok == 0 ? lo[a] : ok == 1 ? hi[a] : ok == 2 ? std::nextafter(lo[a], -INFINITY)
                   : ok == 3 ? std::nextafter(hi[a], INFINITY) : ok == 4 ? 0.5f * lo[a] + 0.5f * hi[a] : -1e30f;
            if (!std::isfinite(r.o[a])) r.o[a] = ok == 2 ? -FLT_MAX : FLT_MAX;
        }
        // a zero reciprocal (a direction component of +-inf, which no normalised AO direction has) is compared where
        // both differences of its axis are finite: an overflowed one times zero is a NaN on one plane only, which the
        // two forms drop at different places
        bool skip = false;
        for (int a = 0; a < 3; ++a)
            skip = skip || (r.inv[a] == 0.0f && !(std::isfinite(lo[a] - r.o[a]) && std::isfinite(hi[a] - r.o[a])));
        skipped += skip;
        if (skip) continue;
        for (float max_t : radii) one_case(lo, hi, uint32_t(px + ix) % 4u, r, max_t, t);
    }
    // the never-hit box of an unused entry: fails for every finite ray under both forms
    const float inf3[3] = { INFINITY, INFINITY, INFINITY };
    for (int ix = 0; ix < NI; ++ix) for (int iy = 0; iy < NI; ++iy) for (int iz = 0; iz < NI; ++iz)
        for (float o : { 0.0f, -3.0f, 1e30f, FLT_MAX, -FLT_MAX })
            for (float max_t : radii)
            {
                ray r;
                r.inv[0] = invs[ix]; r.inv[1] = invs[iy]; r.inv[2] = invs[iz];
                r.o[0] = o; r.o[1] = -o; r.o[2] = 0.25f * o;
                one_case(inf3, inf3, uint32_t(ix) % 4u, r, max_t, never);
            }
    std::printf("edges: %llu cases, %llu pass, %llu differ, %llu differ from the mirror, %llu zeros of the other sign, "
                "%llu rays left out; never-hit box: %llu cases, %llu pass, %llu differ, %llu with a NaN distance\n",
                (unsigned long long)t.cases, (unsigned long long)t.pass, (unsigned long long)t.differ,
                (unsigned long long)t.mirror_differ, (unsigned long long)t.zero_sign, (unsigned long long)skipped,
                (unsigned long long)never.cases,
                (unsigned long long)never.pass, (unsigned long long)never.differ, (unsigned long long)never.nan_cases);
    return (t.differ == 0 && t.mirror_differ == 0 && t.pass > 0 && t.pass < t.cases && t.zero_sign > 0
            && never.cases > 0 && never.pass == 0 && never.differ == 0 && never.mirror_differ == 0 && never.nan_cases > 0) ? 0 : 1;
}

} // namespace

int main()
{
    int rc = part_random(160000);                 // 1.28 million cases
    rc |= part_edges();
    std::printf(rc == 0 ? "ok\n" : "FAILED\n");
    return rc;
}
