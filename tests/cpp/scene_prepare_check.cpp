// tests/cpp/scene_prepare_check.cpp -- the host half of vrh_scene_upload (vrh_upload.cpp prepare_scene) as a
// program of its own, for AddressSanitizer and UBSan (tests/test_scene_prepare.py).
//
//   1. identity: small trees of every primitive kind (built by build_bvh: triangles, spheres, generic primitives
//      with both alternatives in one leaf; the triangle tree again with its primitives in leaf order and no index
//      array; a one-node tree; a hand-made comb with a reversed index array; a tree with one non-finite bound),
//      each under pair layout 1 and 2, never-hit unused entries on and off, and fused records off / on with
//      widening 0 and 24.  One line per run: the scalar fields and an FNV-1a-64 hash of every output array.  The
//      test compares the lines with tests/golden/scene_prepare.txt, recorded from vrh_scene_upload as it was
//      before prepare_scene was split from it.
//   2. refusals: every malformed input is refused with VRH_ERR_INVALID; one line each with the message (compared
//      with the same file).
//   3. properties of the outputs of part 1, counted on the way (the test asserts the counts are not zero): END
//      flags exactly on each leaf's last primitive; under layout 1 the inner links are a permutation and child 0's
//      pair follows its parent; the comb's depth; no 4-wide or fused records over a non-finite bound; the sphere
//      flag in word 11 of generic sphere records only.
// Exit status 0 iff all hold; the last line is then "ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../visionaray_amd/csrc/vrh_internal.h"

extern "C" int vrh_gen_heightfield(uint32_t grid, void* out);
extern "C" int vrh_gen_spheres(uint32_t n, void* out);

namespace vrh { void set_error(const std::string&) {} }

namespace check {

using namespace vrh;

// one input of prepare_scene; the primitive records are kept as bytes (the allocation is aligned for any record)
struct input
{
    std::string name;
    std::vector<node32> nodes;
    std::vector<unsigned char> prims;
    uint32_t num_prims = 0, kind = 0;
    std::vector<uint32_t> indices;
    bool have_indices = true;
    uint32_t num_nodes() const { return uint32_t(nodes.size()); }
    const uint32_t* idx() const { return have_indices ? indices.data() : nullptr; }
    template <class P> P* as(uint32_t i = 0) { return reinterpret_cast<P*>(prims.data()) + i; }
    template <class P> const P* as(uint32_t i = 0) const { return reinterpret_cast<const P*>(prims.data()) + i; }
};

struct config { upload_options opt; std::string name; };

inline std::vector<config> configs()
{
    std::vector<config> out;
    for (int layout : { 1, 2 })
        for (int never : { 0, 1 })
            for (int fused : { 0, 1 })
                for (int widen : { 0, 24 })
                {
                    config c;
                    c.opt.pair_layout = layout; c.opt.never_hit_unused = never != 0;
                    c.opt.want_fused = fused != 0; c.opt.fused_widen = widen;
                    c.name = "layout" + std::to_string(layout) + " never_hit" + std::to_string(never) + " fused"
                             + std::to_string(fused) + " widen" + std::to_string(widen);
                    out.push_back(c);
                }
    return out;
}

inline void build(input& in)
{
    in.nodes.resize(2 * size_t(in.num_prims));
    in.indices.resize(in.num_prims);
    uint32_t n = 0;
    build_bvh(in.prims.data(), in.num_prims, in.kind, in.nodes.data(), &n, in.indices.data(), nullptr);
    in.nodes.resize(n);
}

inline input heightfield(uint32_t grid)
{
    input in;
    in.name = "tri_hf" + std::to_string(grid);
    in.kind = VRH_PRIM_TRI64;
    in.num_prims = 2 * grid * grid;
    in.prims.resize(sizeof(tri64) * in.num_prims);
    vrh_gen_heightfield(grid, in.prims.data());
    for (uint32_t i = 0; i < in.num_prims; ++i) in.as<tri64>(i)->geom_id = i % 5;
    build(in);
    return in;
}

inline input spheres(uint32_t n)
{
    input in;
    in.name = "sphere" + std::to_string(n);
    in.kind = VRH_PRIM_SPHERE48;
    in.num_prims = n;
    in.prims.resize(sizeof(sphere48) * n);
    vrh_gen_spheres(n, in.prims.data());
    for (uint32_t i = 0; i < n; ++i) { in.as<sphere48>(i)->radius *= 8.0f; in.as<sphere48>(i)->geom_id = i % 3; }
    build(in);
    return in;
}

// every third primitive a sphere at the triangle's first vertex, so that leaves hold both alternatives
inline input generic(uint32_t grid)
{
    const input hf = heightfield(grid);
    input in;
    in.name = "generic_hf" + std::to_string(grid);
    in.kind = VRH_PRIM_GENERIC80;
    in.num_prims = hf.num_prims;
    in.prims.assign(sizeof(generic80) * in.num_prims, 0);
    for (uint32_t i = 0; i < in.num_prims; ++i)
    {
        generic80& g = *in.as<generic80>(i);
        const tri64& t = *hf.as<tri64>(i);
        if (i % 3 == 1)
        {
            g.sphere.geom_id = 7; g.sphere.prim_id = i;
            for (int a = 0; a < 3; ++a) g.sphere.center[a] = t.v1[a];
            g.sphere.radius = 0.05f;
            g.type = VRH_GENERIC_TYPE_SPHERE;
        }
        else { g.tri = t; g.type = VRH_GENERIC_TYPE_TRI; }
    }
    build(in);
    return in;
}

// the same tree over the primitives in leaf order, without an index array
inline input leaf_ordered(const input& src)
{
    input in = src;
    in.name = src.name + "_noindex";
    const size_t bytes = prim_record_bytes(src.kind);
    for (uint32_t i = 0; i < src.num_prims; ++i)
        std::memcpy(&in.prims[bytes * i], &src.prims[bytes * src.indices[i]], bytes);
    in.have_indices = false;
    return in;
}

// `leaves` one-triangle leaves in a row along x: every inner node's first child is a leaf (depth leaves - 1); the
// index array is reversed
inline input comb(uint32_t leaves)
{
    input in;
    in.name = "comb" + std::to_string(leaves);
    in.kind = VRH_PRIM_TRI64;
    in.num_prims = leaves;
    in.prims.assign(sizeof(tri64) * leaves, 0);
    in.nodes.resize(2 * size_t(leaves) - 1);
    for (uint32_t i = 0; i < leaves; ++i)
    {
        tri64& t = *in.as<tri64>(leaves - 1 - i);           // leaf i holds primitive leaves - 1 - i
        t.prim_id = 100 + i; t.geom_id = i;
        t.v1[0] = float(i); t.e1[0] = 0.5f; t.e2[1] = 0.5f + 0.01f * float(i);
        in.indices.push_back(leaves - 1 - i);
    }
    auto leaf = [&](node32& n, uint32_t i) {
        const tri64& t = *in.as<tri64>(leaves - 1 - i);
        n.bmin[0] = t.v1[0]; n.bmax[0] = t.v1[0] + 0.5f; n.bmin[1] = 0.0f; n.bmax[1] = t.e2[1]; n.bmin[2] = n.bmax[2] = 0.0f;
        n.first = i; n.num_prims = 1;
    };
    if (leaves == 1) { leaf(in.nodes[0], 0); return in; }
    // node 0 and every node 2 k (k >= 1, but the last) is the inner node over leaves [k, leaves); node 2 k + 1 is leaf k
    for (uint32_t k = 0; k + 1 < leaves; ++k)
    {
        node32& inner = in.nodes[2 * k];
        inner.bmin[0] = float(k); inner.bmax[0] = float(leaves - 1) + 0.5f;
        inner.bmin[1] = 0.0f; inner.bmax[1] = 0.5f + 0.01f * float(leaves - 1);
        inner.bmin[2] = inner.bmax[2] = 0.0f;
        inner.first = 2 * k + 1; inner.num_prims = 0;
        leaf(in.nodes[2 * k + 1], k);
    }
    leaf(in.nodes[2 * leaves - 2], leaves - 1);
    return in;
}

inline std::vector<input> identity_inputs()
{
    std::vector<input> v;
    v.push_back(heightfield(8));
    v.push_back(leaf_ordered(v[0]));
    v.push_back(spheres(150));
    v.push_back(leaf_ordered(v[2]));
    v.push_back(generic(7));
    v.push_back(comb(1));
    v.back().name = "one_node";
    v.push_back(comb(9));
    input bad = heightfield(5);
    bad.name = "nonfinite";
    bad.nodes[4].bmax[1] = std::numeric_limits<float>::infinity();
    v.push_back(bad);
    return v;
}

struct refusal { input in; uint32_t num_nodes, num_prims, num_indices; };

// the first leaf / inner node after the root, and the deepest-numbered inner node
inline uint32_t find_node(const input& in, bool leaf, bool last = false)
{
    uint32_t found = 0;
    for (uint32_t i = 1; i < in.num_nodes(); ++i)
        if ((in.nodes[i].num_prims != 0) == leaf) { found = i; if (!last) break; }
    return found;
}

inline std::vector<refusal> refusal_inputs()
{
    const input hf = heightfield(6), gen = generic(4);
    std::vector<refusal> v;
    auto add = [&](const input& base, const char* name) -> refusal& {
        v.push_back({ base, base.num_nodes(), base.num_prims, uint32_t(base.indices.size()) });
        v.back().in.name = name;
        return v.back();
    };
    const uint32_t leaf = find_node(hf, true), inner = find_node(hf, false), last_inner = find_node(hf, false, true);
    add(hf, "even_node_count").num_nodes -= 1;
    add(hf, "root_first_not_1").in.nodes[0].first = 3;
    add(hf, "leaf_range_past_indices").in.nodes[leaf].num_prims += hf.num_prims;
    add(hf, "leaf_first_2^31").in.nodes[leaf].first = 0x80000000u;
    add(hf, "inner_first_0").in.nodes[inner].first = 0;
    add(hf, "inner_first_even").in.nodes[inner].first += 1;
    add(hf, "inner_first_past_nodes").in.nodes[inner].first = hf.num_nodes();
    // the root's children are both inner nodes in this tree: the second one's pair gets the first one as a parent too
    // (the first one's own subtree is then unreachable, which alone is accepted)
    add(hf, "pair_with_two_parents").in.nodes[1].first = hf.nodes[2].first;
    add(hf, "cycle_to_ancestor").in.nodes[last_inner].first = 1;
    add(hf, "index_out_of_range").in.indices[3] = hf.num_prims;
    add(gen, "generic_type_0").in.as<generic80>(5)->type = 0;
    add(gen, "generic_type_3").in.as<generic80>(gen.num_prims - 1)->type = 3;
    add(hf, "unknown_kind").in.kind = 7;
    add(hf, "zero_nodes").num_nodes = 0;
    add(hf, "zero_prims").num_prims = 0;
    add(comb(1), "root_leaf_past_indices").in.nodes[0].num_prims = 2;
    // two defects each: which one is reported
    refusal& a = add(hf, "even_node_count_and_index_out_of_range");
    a.num_nodes -= 1; a.in.indices[0] = 0xFFFFFFFFu;
    refusal& b = add(hf, "cycle_and_index_out_of_range");
    b.in.nodes[last_inner].first = 1; b.in.indices[0] = 0xFFFFFFFFu;
    refusal& c = add(gen, "generic_type_and_malformed_pair");
    c.in.as<generic80>(2)->type = 9; c.in.nodes[1].first = 0; c.in.nodes[1].num_prims = 0;
    return v;
}

inline uint64_t fnv(const std::vector<float>& v)
{
    uint64_t h = 0xcbf29ce484222325ull;
    const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(float); ++i) h = (h ^ p[i]) * 0x100000001b3ull;
    return h;
}

inline void print_result(const input& in, const config& c, const prepared_scene& p)
{
    uint32_t omax;
    std::memcpy(&omax, &p.fused_omax, 4);
    std::printf("%s %s: root=%08x pairs=%u indices=%u depth=%u quad_depth=%u max_prim_id=%u max_geom_id=%u omax=%08x "
                "finite=%d quads=%d fused=%d | pairs %zu %016llx prims %zu %016llx quads %zu %016llx fused %zu %016llx "
                "leaf_boxes %zu %016llx\n", in.name.c_str(), c.name.c_str(), p.root, p.num_pairs, p.num_indices, p.max_depth,
                p.quad_depth, p.max_prim_id, p.max_geom_id, omax, int(p.finite_bounds), int(p.have_quads), int(p.fused_built),
                p.pairs.size(), (unsigned long long)fnv(p.pairs), p.prims.size(), (unsigned long long)fnv(p.prims),
                p.quads.size(), (unsigned long long)fnv(p.quads), p.fused_recs.size(), (unsigned long long)fnv(p.fused_recs),
                p.leaf_boxes.size(), (unsigned long long)fnv(p.leaf_boxes));
}

inline void print_refusal(const input& in, int rc, const std::string& err)
{
    std::printf("refused %s: %d %s\n", in.name.c_str(), rc, err.c_str());
}

} // namespace check

#ifndef SCENE_PREPARE_CHECK_NO_MAIN
namespace {

using namespace check;

struct counts { unsigned long long end_set = 0, end_clear = 0, links = 0, child0 = 0, sphere_recs = 0, tri_recs = 0, mixed_leaves = 0; };
int failures = 0;
void fail(const input& in, const config& c, const char* what) { std::printf("FAILED %s %s: %s\n", in.name.c_str(), c.name.c_str(), what); ++failures; }

uint32_t word(const std::vector<float>& v, size_t i) { uint32_t w; std::memcpy(&w, &v[i], 4); return w; }

void properties(const input& in, const config& c, const prepared_scene& p, counts& n)
{
    const size_t per = leaf_record_bytes(in.kind) / 4, flag_at = in.kind == VRH_PRIM_SPHERE48 ? 6 : 11;
    if (p.prims.size() != per * p.num_indices || p.pairs.size() != 16 * size_t(p.num_pairs ? p.num_pairs : 1)) fail(in, c, "array sizes");
    // END flags: on the last primitive of every leaf, nowhere else
    std::vector<uint8_t> want(p.num_indices, 0);
    for (const node32& nd : in.nodes)
        if (nd.num_prims)
        {
            want[nd.first + nd.num_prims - 1] = 1;
            bool tri = false, sph = false;
            if (in.kind == VRH_PRIM_GENERIC80)
                for (uint32_t i = nd.first; i < nd.first + nd.num_prims; ++i)
                    (in.as<generic80>(in.have_indices ? in.indices[i] : i)->type == VRH_GENERIC_TYPE_SPHERE ? sph : tri) = true;
            n.mixed_leaves += tri && sph;
        }
    for (uint32_t i = 0; i < p.num_indices; ++i)
    {
        const uint32_t flags = word(p.prims, per * i + flag_at);
        if ((flags & PRIM_FLAG_END) != want[i]) fail(in, c, "END flag");
        (want[i] ? n.end_set : n.end_clear) += 1;
        if (in.kind == VRH_PRIM_GENERIC80)
        {
            const bool sphere = in.as<generic80>(in.have_indices ? in.indices[i] : i)->type == VRH_GENERIC_TYPE_SPHERE;
            if (((flags & PRIM_FLAG_SPHERE) != 0) != sphere) fail(in, c, "sphere flag");
            (sphere ? n.sphere_recs : n.tri_recs) += 1;
        }
        else if (flags & PRIM_FLAG_SPHERE) fail(in, c, "sphere flag outside a generic scene");
    }
    // layout 1: every pair is reached once from the root (the links are a permutation of the pairs), and a pair's
    // child-0 pair is the next record
    if (c.opt.pair_layout == 1 && !(p.root & 0x80000000u))
    {
        std::vector<uint8_t> seen(p.num_pairs, 0);
        std::vector<uint32_t> st{ p.root };
        size_t reached = 0;
        while (!st.empty())
        {
            const uint32_t k = st.back(); st.pop_back();
            if (k >= p.num_pairs || seen[k]) { fail(in, c, "layout 1: link out of range or repeated"); break; }
            seen[k] = 1; ++reached; ++n.links;
            const uint32_t w0 = word(p.pairs, 16 * size_t(k) + 12), w1 = word(p.pairs, 16 * size_t(k) + 13);
            if (!(w0 & 0x80000000u)) { if (w0 != k + 1) fail(in, c, "layout 1: child 0 does not follow its parent"); ++n.child0; st.push_back(w0); }
            if (!(w1 & 0x80000000u)) st.push_back(w1);
        }
        if (reached != p.num_pairs || p.root != 0) fail(in, c, "layout 1: not a permutation");
    }
    if (in.name == "comb9" && p.max_depth != 8) fail(in, c, "comb depth");
    if (in.name == "one_node" && (p.num_pairs != 0 || p.root != 0x80000000u || p.max_depth != 0 || p.have_quads)) fail(in, c, "one-node tree");
    if (in.name == "nonfinite" && (p.finite_bounds || p.have_quads || p.fused_built || !p.quads.empty() || !p.fused_recs.empty() || !p.leaf_boxes.empty()))
        fail(in, c, "records over a non-finite bound");
    if (in.name != "nonfinite" && !p.finite_bounds) fail(in, c, "finite bounds reported non-finite");
    if (p.fused_built != !p.fused_recs.empty() || p.have_quads != !p.quads.empty() || (p.fused_built && !c.opt.want_fused)
        || (p.fused_built && (p.fused_recs.size() != p.quads.size() || p.leaf_boxes.size() != 8 * size_t(p.num_indices))))
        fail(in, c, "fused records");
}

} // namespace

int main()
{
    counts n;
    unsigned long long runs = 0, nonfinite = 0, fused = 0, quads = 0;
    for (const input& in : identity_inputs())
        for (const config& c : configs())
        {
            prepared_scene p;
            std::string err;
            const int rc = prepare_scene(in.nodes.data(), in.num_nodes(), in.prims.data(), in.num_prims, in.kind, in.idx(),
                                         uint32_t(in.indices.size()), c.opt, p, err);
            if (rc != VRH_OK) { fail(in, c, err.c_str()); continue; }
            print_result(in, c, p);
            properties(in, c, p, n);
            ++runs; nonfinite += !p.finite_bounds; fused += p.fused_built; quads += p.have_quads;
        }
    unsigned long long refused = 0;
    for (const refusal& r : refusal_inputs())
    {
        prepared_scene p;
        std::string err;
        const int rc = prepare_scene(r.in.nodes.data(), r.num_nodes, r.in.prims.data(), r.num_prims, r.in.kind, r.in.idx(),
                                     r.num_indices, configs()[0].opt, p, err);
        print_refusal(r.in, rc, err);
        if (rc != VRH_ERR_INVALID || err.empty()) { fail(r.in, configs()[0], "not refused with VRH_ERR_INVALID"); continue; }
        ++refused;
    }
    std::printf("checked: %llu runs, %llu refusals, %llu END flags set, %llu clear, %llu layout-1 links, %llu child-0 pairs, "
                "%llu generic sphere records, %llu generic triangle records, %llu mixed leaves, %llu non-finite runs, "
                "%llu with 4-wide records, %llu with fused records, %d failures\n", runs, refused, n.end_set, n.end_clear, n.links,
                n.child0, n.sphere_recs, n.tri_recs, n.mixed_leaves, nonfinite, quads, fused, failures);
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
#endif
