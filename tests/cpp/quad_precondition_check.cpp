// tests/cpp/quad_precondition_check.cpp -- what the AO kernel's octant step (vrh_octant.h) needs of the 4-wide records,
// decided on the host by build_quads (vrh_quad.cpp): every used entry's box has lo <= hi on the three axes.
//
//   1. the fixture scenes' trees (cornell12, heightfields of 16, 64 and 200 cells a side, 1000 spheres; built by
//      build_bvh) all get records; every used entry of them has lo <= hi, every unused one the never-hit box.
//   2. the hf16 tree with ONE box inverted on one axis -- a child of the root, a grandchild, the last leaf, each on
//      x, y and z -- gets none; nor with one bound a NaN (a lower one, an upper one).
// Prints one line per part; exit status 0 iff all hold; the last line is then "ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <utility>
#include <vector>

#include "../../visionaray_amd/csrc/vrh_internal.h"

extern "C" int vrh_gen_heightfield(uint32_t grid, void* out);
extern "C" int vrh_gen_cornell(void* out);
extern "C" int vrh_gen_spheres(uint32_t n, void* out);

namespace vrh { void set_error(const std::string&) {} }

namespace {

using vrh::node32;

std::vector<node32> tree_of(const void* prims, uint32_t n, uint32_t kind)
{
    std::vector<node32> nodes(2 * size_t(n));
    std::vector<uint32_t> indices(n);
    uint32_t count = 0;
    if (vrh::build_bvh(prims, n, kind, nodes.data(), &count, indices.data(), nullptr) != 0) count = 0;
    nodes.resize(count);
    return nodes;
}

std::vector<node32> heightfield(uint32_t grid)
{
    std::vector<vrh::tri64> t(2 * size_t(grid) * grid);
    vrh_gen_heightfield(grid, t.data());
    return tree_of(t.data(), uint32_t(t.size()), VRH_PRIM_TRI64);
}

bool quads_of(const std::vector<node32>& nodes, std::vector<float>& out)
{
    uint32_t root = 0, depth = 0;
    return vrh::build_quads(nodes.data(), uint32_t(nodes.size()), out, root, depth, nullptr, true);
}

} // namespace

int main()
{
    std::vector<std::pair<std::string, std::vector<node32>>> scenes;
    {
        std::vector<vrh::tri64> t(12);
        vrh_gen_cornell(t.data());
        scenes.push_back({ "cornell12", tree_of(t.data(), 12, VRH_PRIM_TRI64) });
    }
    for (uint32_t g : { 16u, 64u, 200u }) scenes.push_back({ "hf" + std::to_string(g), heightfield(g) });
    {
        std::vector<vrh::sphere48> s(1000);
        vrh_gen_spheres(1000, s.data());
        scenes.push_back({ "sph1000", tree_of(s.data(), 1000, VRH_PRIM_SPHERE48) });
    }
    uint64_t accepted = 0, used = 0, unused = 0, flat = 0, bad = 0;
    for (const auto& sc : scenes)
    {
        std::vector<float> q;
        if (sc.second.size() < 3 || !quads_of(sc.second, q) || q.empty()) { std::printf("%s: no records\n", sc.first.c_str()); continue; }
        ++accepted;
        for (size_t r = 0; r < q.size() / 32; ++r)
            for (uint32_t e = 0; e < 4; ++e)
            {
                uint32_t l;
                std::memcpy(&l, &q[r * 32 + 24 + e], 4);
                for (int a = 0; a < 3; ++a)
                {
                    const float lo = q[r * 32 + 4 * a + e], hi = q[r * 32 + 12 + 4 * a + e];
                    if (l == vrh::QUAD_NONE) bad += !(lo == INFINITY && hi == INFINITY);
                    else { bad += !(lo <= hi); flat += lo == hi; }
                }
                (l == vrh::QUAD_NONE ? unused : used) += 1;
            }
    }
    std::printf("fixture scenes: %llu of %llu accepted, %llu used entries (%llu flat axes), %llu unused, %llu wrong\n",
                (unsigned long long)accepted, (unsigned long long)scenes.size(), (unsigned long long)used,
                (unsigned long long)flat, (unsigned long long)unused, (unsigned long long)bad);
    int rc = (accepted == scenes.size() && used > 0 && unused > 0 && flat > 0 && bad == 0) ? 0 : 1;

    const std::vector<node32>& base = scenes[1].second;                 // hf16
    uint64_t tried = 0, refused = 0;
    if (base.size() >= 7 && base[0].num_prims == 0 && base[base[0].first].num_prims == 0)
    {
        const uint32_t child = base[0].first + 1, grandchild = base[base[0].first].first, last = uint32_t(base.size()) - 1;
        std::vector<float> q;
        for (uint32_t n : { child, grandchild, last })
            for (int a = 0; a < 3; ++a)
            {
                // a flat axis cannot be inverted by a swap: widen it first (the widened tree is still accepted)
                std::vector<node32> t = base;
                if (t[n].bmin[a] == t[n].bmax[a]) t[n].bmax[a] = std::nextafter(t[n].bmax[a], INFINITY);
                std::swap(t[n].bmin[a], t[n].bmax[a]);
                ++tried; refused += !quads_of(t, q);
                for (int which = 0; which < 2; ++which)
                {
                    t = base;
                    (which ? t[n].bmax[a] : t[n].bmin[a]) = std::numeric_limits<float>::quiet_NaN();
                    ++tried; refused += !quads_of(t, q);
                }
            }
    }
    std::printf("one inverted box or one NaN bound: %llu trees, %llu refused\n", (unsigned long long)tried, (unsigned long long)refused);
    rc |= (tried == 27 && refused == tried) ? 0 : 1;
    std::printf(rc == 0 ? "ok\n" : "FAILED\n");
    return rc;
}
