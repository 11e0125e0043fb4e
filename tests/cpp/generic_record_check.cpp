// The 80-byte generic primitive record and the host re-layout of vrh_scene_upload as a stand-alone host program,
// built with -fsanitize=address,undefined (tests/test_generic_build.py).  It reads a fixture's records from a file
// (80 bytes each, as the reference wrote them); builds visionaray_hip/standalone.h's
// generic_primitive<basic_triangle<3, float>, basic_sphere<float>> for both alternatives from the fields of each
// record and checks that it is the file's bytes (the alternative at 0, the type index at 64); and runs the re-layout
// (vrh_internal.h generic_leaf_record) over every record as a leaf would hold them -- the last one with the END
// flag -- and over a record with a bad type index.
//
//     generic_record_check <records.bin>
#include "../../include/visionaray_hip/standalone.h"
#include "../../visionaray_amd/csrc/vrh_internal.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace vrh;
using tri_t = visionaray::basic_triangle<3, float>;
using sphere_t = visionaray::basic_sphere<float>;
using public_t = visionaray::generic_primitive<tri_t, sphere_t>;
static_assert(sizeof(public_t) == sizeof(generic80) && offsetof(public_t, type_index) == offsetof(generic80, type), "one record");

// the bytes of the public record that carry data: ids, the vectors' three floats, the radius, the type index
static bool same_record(const public_t& p, const unsigned char* b, bool sphere)
{
    const unsigned char* m = reinterpret_cast<const unsigned char*>(&p);
    bool ok = std::memcmp(m, b, 8) == 0 && std::memcmp(m + 16, b + 16, 12) == 0 && std::memcmp(m + 64, b + 64, 4) == 0;
    if (sphere) return ok && std::memcmp(m + 32, b + 32, 4) == 0;
    return ok && std::memcmp(m + 32, b + 32, 12) == 0 && std::memcmp(m + 48, b + 48, 12) == 0;
}

#define REQUIRE(cond)                                                                             \
    do { if (!(cond)) { std::printf("FAILED: %s (record %zu)\n", #cond, i); return 1; } } while (0)

int main(int argc, char** argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s <records.bin>\n", argv[0]); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<unsigned char> raw;
    unsigned char buf[80];
    while (std::fread(buf, 80, 1, f) == 1) raw.insert(raw.end(), buf, buf + 80);
    std::fclose(f);
    const size_t n = raw.size() / 80;
    if (n == 0) return 2;
    std::vector<generic80> recs(n);                     // exactly n records: a read past the end is the sanitizer's
    std::memcpy(recs.data(), raw.data(), raw.size());
    size_t tris = 0, spheres = 0;
    std::vector<uint32_t> leaf(12 * n);
    for (size_t i = 0; i < n; ++i)
    {
        const generic80& g = recs[i];
        const unsigned char* b = &raw[80 * i];
        uint32_t type, ids[2];
        std::memcpy(&type, b + VRH_GENERIC_TYPE_OFFSET, 4);
        std::memcpy(ids, b, 8);
        REQUIRE(g.type == type && (type == VRH_GENERIC_TYPE_TRI || type == VRH_GENERIC_TYPE_SPHERE));
        uint32_t* w = &leaf[12 * i];
        const bool end = i + 1 == n;
        REQUIRE(generic_leaf_record(g, end, w));
        REQUIRE(w[9] == ids[1] && w[10] == ids[0]);                       // prim_id@4, geom_id@0 of either alternative
        REQUIRE((w[11] & PRIM_FLAG_END) == (end ? PRIM_FLAG_END : 0u));
        if (type == VRH_GENERIC_TYPE_TRI)
        {
            ++tris;
            REQUIRE(g.tri.geom_id == ids[0] && g.tri.prim_id == ids[1]);
            REQUIRE(std::memcmp(w, b + 16, 12) == 0 && std::memcmp(w + 3, b + 32, 12) == 0 && std::memcmp(w + 6, b + 48, 12) == 0);
            REQUIRE((w[11] & PRIM_FLAG_SPHERE) == 0u);
            tri_t t(visionaray::vec3(g.tri.v1[0], g.tri.v1[1], g.tri.v1[2]), visionaray::vec3(g.tri.e1[0], g.tri.e1[1], g.tri.e1[2]),
                    visionaray::vec3(g.tri.e2[0], g.tri.e2[1], g.tri.e2[2]));
            t.geom_id = g.tri.geom_id; t.prim_id = g.tri.prim_id;
            const public_t p(t);
            REQUIRE(p.is_triangle() && !p.is_sphere() && same_record(p, b, false));
            REQUIRE(p.triangle().prim_id == ids[1] && p.triangle().e2.z == g.tri.e2[2]);
        }
        else
        {
            ++spheres;
            REQUIRE(g.sphere.geom_id == ids[0] && g.sphere.prim_id == ids[1]);
            REQUIRE(std::memcmp(w, b + 16, 12) == 0 && std::memcmp(w + 3, b + 32, 4) == 0);     // centre@16, radius@32
            REQUIRE((w[11] & PRIM_FLAG_SPHERE) != 0u);
            for (int k = 4; k < 9; ++k) REQUIRE(w[k] == 0u);
            sphere_t sp(visionaray::vec3(g.sphere.center[0], g.sphere.center[1], g.sphere.center[2]), g.sphere.radius);
            sp.geom_id = g.sphere.geom_id; sp.prim_id = g.sphere.prim_id;
            const public_t p(sp);
            REQUIRE(p.is_sphere() && !p.is_triangle() && same_record(p, b, true));
            REQUIRE(p.sphere().prim_id == ids[1] && p.sphere().radius == g.sphere.radius);
        }
    }
    {
        const size_t i = 0;
        generic80 bad = recs[0];
        uint32_t w[12];
        bad.type = 0u;
        REQUIRE(!generic_leaf_record(bad, false, w));
        bad.type = 3u;
        REQUIRE(!generic_leaf_record(bad, true, w));
        REQUIRE(tris > 0 && spheres > 0);
        REQUIRE(prim_record_bytes(VRH_PRIM_GENERIC80) == sizeof(generic80) && prim_record_bytes(7u) == 0u);
    }
    std::printf("generic record ok: %zu triangles, %zu spheres\n", tris, spheres);
    return 0;
}
