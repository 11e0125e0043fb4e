// visionaray_amd/csrc/vrh_upload.cpp -- the host half of vrh_scene_upload: validates a caller's BVH (untrusted
// bytes) and re-lays it into the arrays the device reads (node pairs, leaf-ordered primitives, 4-wide records).
// Plain C++ that knows nothing of HIP or of the library it is linked into, so that a stand-alone program can
// run it under a sanitizer (tests/test_scene_prepare.py).

#include "vrh_internal.h"
#include "../../include/visionaray_hip/detail/vrh_fused_slab.h"

#include <algorithm>
#include <cmath>
#include <utility>

namespace vrh {

bool check_generic_types(const void* prims, uint32_t num_prims, const char* who, std::string& err)
{
    for (uint32_t i = 0; i < num_prims; ++i)
    {
        const uint32_t ty = static_cast<const generic80*>(prims)[i].type;
        if (ty == VRH_GENERIC_TYPE_TRI || ty == VRH_GENERIC_TYPE_SPHERE) continue;
        err = std::string(who) + ": generic primitive " + std::to_string(i) + " has type index " + std::to_string(ty)
              + " (1 triangle, 2 sphere)";
        return false;
    }
    return true;
}

int prepare_scene(const void* nodes_v, uint32_t num_nodes, const void* prims_v, uint32_t num_prims, uint32_t prim_kind,
                  const uint32_t* indices, uint32_t num_indices, const upload_options& opt, prepared_scene& out,
                  std::string& err)
{
    auto refuse = [&](const std::string& msg) { err = msg; return VRH_ERR_INVALID; };
    if (!(num_nodes >= 1 && num_prims >= 1)) return refuse("vrh_scene_upload: empty BVH");
    if (prim_record_bytes(prim_kind) == 0u) return refuse("vrh_scene_upload: unknown prim_kind");
    if (prim_kind == VRH_PRIM_GENERIC80 && !check_generic_types(prims_v, num_prims, "vrh_scene_upload", err)) return VRH_ERR_INVALID;
    if (num_nodes % 2 != 1) return refuse("vrh_scene_upload: node count must be odd (root + child pairs)");
    if (!indices) num_indices = num_prims;
    auto nodes = static_cast<const node32*>(nodes_v);
    out = prepared_scene{};
    out.num_indices = num_indices;

    // -- node pairs + topology validation + depth
    const uint32_t npairs = out.num_pairs = (num_nodes - 1) / 2;
    std::vector<float>& pairs = out.pairs;
    pairs.assign(16 * size_t(std::max<uint32_t>(npairs, 1)), 0.0f);
    std::vector<uint8_t> end_flag(num_indices, 0);
    auto link_of = [&](const node32& c, uint32_t& link) -> bool {
        if (c.num_prims != 0)
        {
            if (uint64_t(c.first) + c.num_prims > num_indices || c.first >= 0x80000000u) return false;
            end_flag[c.first + c.num_prims - 1] = 1;
            link = 0x80000000u | c.first;
            return true;
        }
        if (c.first == 0 || c.first % 2 != 1 || uint64_t(c.first) + 1 >= num_nodes) return false;
        link = (c.first - 1) / 2;
        return true;
    };
    auto links_of = [&](size_t k, uint32_t w[2]) { std::memcpy(w, &pairs[16 * k + 12], 8); };
    uint32_t& root = out.root;
    if (!link_of(nodes[0], root)) return refuse("vrh_scene_upload: malformed root node");
    if (nodes[0].num_prims == 0 && nodes[0].first != 1) return refuse("vrh_scene_upload: root children must be nodes 1,2");
    for (uint32_t k = 0; k < npairs; ++k)
    {
        const node32 &c0 = nodes[2 * k + 1], &c1 = nodes[2 * k + 2];
        uint32_t l[2];
        if (!link_of(c0, l[0]) || !link_of(c1, l[1])) return refuse("vrh_scene_upload: malformed node pair " + std::to_string(k));
        // slab-major, child-interleaved (vrh_device.h): packed (child 0, child 1) operand pairs, then the links
        const float q[12] = { c0.bmin[0], c1.bmin[0], c0.bmin[1], c1.bmin[1], c0.bmin[2], c1.bmin[2],
                              c0.bmax[0], c1.bmax[0], c0.bmax[1], c1.bmax[1], c0.bmax[2], c1.bmax[2] };
        std::memcpy(&pairs[16 * size_t(k)], q, 48);
        std::memcpy(&pairs[16 * size_t(k) + 12], l, 8);
    }
    // depth (root depth 0) by iterative DFS over links
    {
        // every pair may be reached at most once: a pair reached twice (a DAG or a cycle) is rejected
        std::vector<std::pair<uint32_t, uint32_t>> st;
        std::vector<uint8_t> seen(npairs, 0);
        if (!(root & 0x80000000u)) st.push_back({ root, 1u });
        while (!st.empty())
        {
            auto e = st.back(); st.pop_back();
            if (seen[e.first]) return refuse("vrh_scene_upload: BVH is not a tree (a node pair is reached twice)");
            seen[e.first] = 1;
            out.max_depth = std::max(out.max_depth, e.second);
            uint32_t w[2];
            links_of(e.first, w);
            for (int c = 0; c < 2; ++c)
                if (!(w[c] & 0x80000000u))
                {
                    // cannot happen: link_of admits an inner link (first - 1) / 2 only with first + 1 < num_nodes,
                    // which is below npairs; kept as the guard of the seen[] index above
                    if (w[c] >= npairs) return refuse("vrh_scene_upload: child pair out of range");
                    st.push_back({ w[c], e.second + 1 });
                }
        }
    }

    // -- cache-line pairing (VRH_OPT_PAIR_LAYOUT = 1; auto off: measured neutral, within 1.3 %,
    // profiles/r01/ab_layout.log): re-lay the pair records in a depth-first preorder that puts each pair's child-0
    // pair right after it, so a parent and a child share a 128-B line on half of the descent steps (31 % in the
    // builder's order).  Links are renumbered; the tree, the traversal order and every result are unchanged.
    if (opt.pair_layout == 1 && npairs > 1 && !(root & 0x80000000u))
    {
        std::vector<uint32_t> perm(npairs, 0xFFFFFFFFu);
        uint32_t next = 0;
        std::vector<uint32_t> st{ root };
        while (!st.empty())
        {
            const uint32_t k = st.back(); st.pop_back();
            perm[k] = next++;
            uint32_t w[2];
            links_of(k, w);
            if (!(w[1] & 0x80000000u)) st.push_back(w[1]);
            if (!(w[0] & 0x80000000u)) st.push_back(w[0]);
        }
        for (uint32_t k = 0; k < npairs; ++k)
            if (perm[k] == 0xFFFFFFFFu) perm[k] = next++;      // unreachable records keep a slot
        if (next != npairs) return refuse("vrh_scene_upload: pair layout: not a permutation");
        std::vector<float> np(pairs.size());
        for (uint32_t k = 0; k < npairs; ++k)
        {
            float* d = &np[16 * size_t(perm[k])];
            std::memcpy(d, &pairs[16 * size_t(k)], 64);
            uint32_t w[2];
            std::memcpy(w, d + 12, 8);
            for (int c = 0; c < 2; ++c)
                if (!(w[c] & 0x80000000u)) w[c] = perm[w[c]];
            std::memcpy(d + 12, w, 8);
        }
        pairs.swap(np);
        root = perm[root];
    }

    // -- leaf-ordered primitives with END flags (a generic primitive takes the triangle's three words whichever
    // alternative it holds: vrh_internal.h generic_leaf_record)
    const size_t per = leaf_record_bytes(prim_kind) / 4;
    out.prims.resize(per * num_indices);
    for (uint32_t i = 0; i < num_indices; ++i)
    {
        uint32_t src = indices ? indices[i] : i;
        if (src >= num_prims) return refuse("vrh_scene_upload: index out of range");
        uint32_t w[12] = {};
        if (prim_kind == VRH_PRIM_TRI64)
        {
            const tri64& t = static_cast<const tri64*>(prims_v)[src];
            const float f[9] = { t.v1[0], t.v1[1], t.v1[2], t.e1[0], t.e1[1], t.e1[2], t.e2[0], t.e2[1], t.e2[2] };
            std::memcpy(w, f, sizeof f);
            w[9] = t.prim_id; w[10] = t.geom_id; w[11] = end_flag[i] ? PRIM_FLAG_END : 0u;
        }
        else if (prim_kind == VRH_PRIM_GENERIC80)
            generic_leaf_record(static_cast<const generic80*>(prims_v)[src], end_flag[i] != 0, w);   // types checked above
        else
        {
            const sphere48& s = static_cast<const sphere48*>(prims_v)[src];
            const float f[4] = { s.center[0], s.center[1], s.center[2], s.radius };
            std::memcpy(w, f, sizeof f);
            w[4] = s.prim_id; w[5] = s.geom_id; w[6] = end_flag[i] ? PRIM_FLAG_END : 0u;
        }
        if (per == 8) std::memcpy(&out.prims[per * i], w, 32);     // constant sizes: no call per primitive
        else std::memcpy(&out.prims[per * i], w, 48);
    }
    bool& finite_bounds = out.finite_bounds;
    for (uint32_t i = 0; i < num_nodes && finite_bounds; ++i)
        for (int a = 0; a < 3; ++a)
            finite_bounds = finite_bounds && std::isfinite(nodes[i].bmin[a]) && std::isfinite(nodes[i].bmax[a]);
    for (uint32_t i = 0; i < num_prims; ++i)
    {
        uint32_t ids[2];
        std::memcpy(ids, static_cast<const uint8_t*>(prims_v) + size_t(i) * prim_record_bytes(prim_kind), 8);
        out.max_geom_id = std::max(out.max_geom_id, ids[0]);
        out.max_prim_id = std::max(out.max_prim_id, ids[1]);
    }

    // the fused records (vrh_fused_slab.h) serve ray origins within twice the root box's largest coordinate: an
    // AO ray starts on a surface, inside the root box; a ray from farther out walks the binary records
    // (only in a build whose kernels walk them, VRH_FUSED_STEP -- libvrh_fused.so; VRH_OPT_FUSED_STEP 2 leaves them out)
    fused_records fz;
    if (finite_bounds)
    {
        float extent = 0.0f;
        for (int a = 0; a < 3; ++a)
        {
            fz.omax = std::max(fz.omax, 2.0f * std::max(std::fabs(nodes[0].bmin[a]), std::fabs(nodes[0].bmax[a])));
            extent = std::max(extent, nodes[0].bmax[a] - nodes[0].bmin[a]);
        }
        fz.omax = fused::omax_floor(fz.omax);
        fz.extra = opt.fused_widen ? std::ldexp(extent, -opt.fused_widen) : 0.0f;
        fz.num_indices = num_indices;
    }
    // never_hit_unused: the AO kernel's step does not compare links with QUAD_NONE, so unused entries get never-hit boxes
    uint32_t quad_root = 0;
    out.have_quads = finite_bounds && build_quads(nodes, num_nodes, out.quads, quad_root, out.quad_depth,
                                                  opt.want_fused ? &fz : nullptr, opt.never_hit_unused);
    if (!out.have_quads) { out.quads.clear(); out.quad_depth = 0; }
    else if (fz.built)
    {
        // the leaves' exact boxes, two float4 per leaf-ordered primitive (read at a leaf's first primitive)
        out.leaf_boxes.assign(size_t(8) * fz.leaf_slot.size(), 0.0f);
        for (size_t i = 0; i < fz.leaf_slot.size(); ++i)
        {
            const uint32_t s = fz.leaf_slot[i];
            if (s == QUAD_NONE) continue;
            const float* rec = &out.quads[size_t(s >> 2) * 32 + (s & 3u)];
            for (int a = 0; a < 3; ++a) { out.leaf_boxes[8 * i + a] = rec[4 * a]; out.leaf_boxes[8 * i + 4 + a] = rec[12 + 4 * a]; }
        }
        out.fused_recs = std::move(fz.recs);
        out.fused_omax = fz.omax;
        out.fused_built = true;
    }
    return VRH_OK;
}

} // namespace vrh
