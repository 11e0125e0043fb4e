// visionaray_amd/csrc/vrh_quad.cpp -- 4-wide node records for any-hit rays, derived from the
// reference's binary BVH at upload.
//
// An any-hit ray's result (exit_traversal.h:49-56: the first accepted hit ends the ray) depends
// only on WHICH leaves it reaches, not on the order: before its first hit the running best_t is
// max(), so every box test (update_if.h:60-66) compares against constants.  A leaf is reached iff
// the box test passes for every node on its root path.  If a grandchild's box lies inside its
// parent's box (and every box has min <= max), the slab distances are monotone in the bounds --
// (b - o) * inv rounds monotonically for a fixed finite o and inv -- so the grandchild's tnear is
// >= and its tfar <= the parent's, and passing the grandchild's test implies passing the parent's.
// The parent's test can then be skipped: a record holding the (up to) four grandchildren of a
// node reaches exactly the leaves the binary traversal reaches, in half the dependent steps.
// build_quads checks containment and box validity for every skipped node; if any check fails the
// scene keeps the binary path for all rays.  Only rays with finite origin and inverse direction
// over finite bounds use the records (the slab distances are then never NaN).
//
// Record (32 floats, 128 B): xmin[4] ymin[4] zmin[4] xmax[4] ymax[4] zmax[4] link[4] pad[4];
// link = quad index of an inner grandchild, LEAF_BIT | first primitive (leaf order) of a leaf,
// QUAD_NONE for an unused entry.  An unused entry's box repeats entry 0's, or with `never_hit_unused` (the
// default build's upload, vrh_device.h NEVER_HIT_UNUSED) is the point box lo = hi = +inf that no finite ray passes, so
// the AO kernel's step needs no compare of the link; every other reader of the records keeps its link test.
// That step also takes an axis' near plane from the sign of the ray's inverse direction instead of a min / max of
// the two plane distances (vrh_octant.h), which is exact only for boxes with lo <= hi: build_quads refuses a tree in
// which any node that becomes an entry has another box (valid_box; a NaN bound fails it), and a tree of 2^25 records
// or more, whose byte offsets would not fit the step's 32 bits.
#include "vrh_internal.h"
#include "../../include/visionaray_hip/detail/vrh_fused_slab.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <deque>
#include <unordered_map>

#ifndef VRH_QUAD_ORDER
#define VRH_QUAD_ORDER 0      // record order: 0 = breadth-first, 1 = depth-first (sibling groups)
#endif

namespace vrh {

namespace {

// the AO kernel's octant step (vrh_octant.h) addresses a record by a 32-bit byte offset: 2^25 records of 128 B
constexpr uint32_t MAX_RECORDS = 1u << 25;

// lo <= hi on the three axes (a NaN bound fails).  The octant step relies on it for every used entry: it takes the
// near plane of an axis from the sign of the ray's inverse direction, not from a min / max of the two distances
bool valid_box(const node32& n)
{
    for (int a = 0; a < 3; ++a)
        if (!(n.bmin[a] <= n.bmax[a])) return false;
    return true;
}

bool inside(const node32& g, const node32& p)
{
    for (int a = 0; a < 3; ++a)
        if (!(g.bmin[a] >= p.bmin[a] && g.bmax[a] <= p.bmax[a])) return false;
    return true;
}

// every box valid and every child's box inside its parent's: then a leaf's own exact box test implies the test
// of each of its ancestors, which is what lets a hit found through the fused records be verified against the
// leaf's box alone (fused_records)
bool nested(const node32* nodes, uint32_t num_nodes)
{
    for (uint32_t n = 0; n < num_nodes; ++n)
    {
        if (!valid_box(nodes[n])) return false;
        if (nodes[n].num_prims != 0) continue;
        const uint32_t fc = nodes[n].first;
        if (uint64_t(fc) + 1 >= num_nodes) return false;
        if (!inside(nodes[fc], nodes[n]) || !inside(nodes[fc + 1], nodes[n])) return false;
    }
    return true;
}

} // namespace

bool build_quads(const node32* nodes, uint32_t num_nodes, std::vector<float>& out, uint32_t& root_link,
                 uint32_t& quad_depth, fused_records* fz, bool never_hit_unused)
{
    out.clear();
    quad_depth = 0;
    if (fz) { fz->recs.clear(); fz->leaf_slot.clear(); fz->built = false; }
    if (num_nodes < 3 || nodes[0].num_prims != 0) return false;     // single leaf: nothing to widen
    bool fuse = fz != nullptr && nested(nodes, num_nodes) && fz->omax <= 0x1p100f;
    if (fuse) fz->leaf_slot.assign(fz->num_indices, QUAD_NONE);
    std::unordered_map<uint32_t, uint32_t> index;                    // binary inner node -> quad
    std::deque<std::pair<uint32_t, uint32_t>> queue;                 // (binary node, quad depth)
    index[0] = 0;
    queue.push_back({ 0u, 1u });
    out.resize(32, 0.0f);
    while (!queue.empty())
    {
#if VRH_QUAD_ORDER == 1
        // depth-first: a record's inner entries get consecutive indices (as in breadth-first), and
        // the first of them is expanded next, so a descent's records lie close together
        const uint32_t n = queue.back().first, depth = queue.back().second;
        queue.pop_back();
#else
        const uint32_t n = queue.front().first, depth = queue.front().second;
        queue.pop_front();
#endif
        quad_depth = std::max(quad_depth, depth);
        const uint32_t q = index[n];
        uint32_t entries[4];
        uint32_t links[4];
        uint32_t ne = 0;
        const uint32_t fc = nodes[n].first;
        if (uint64_t(fc) + 1 >= num_nodes) return false;
        for (uint32_t c = fc; c < fc + 2; ++c)
        {
            const node32& cn = nodes[c];
            if (!valid_box(cn)) return false;
            if (cn.num_prims != 0)
            {
                entries[ne] = c;
                links[ne++] = 0x80000000u | cn.first;
                continue;
            }
            if (uint64_t(cn.first) + 1 >= num_nodes) return false;
            for (uint32_t g = cn.first; g < cn.first + 2; ++g)
            {
                const node32& gn = nodes[g];
                if (!valid_box(gn) || !inside(gn, cn)) return false;
                entries[ne] = g;
                if (gn.num_prims != 0)
                    links[ne++] = 0x80000000u | gn.first;
                else
                {
                    auto it = index.find(g);
                    uint32_t gq;
                    if (it == index.end())
                    {
                        gq = uint32_t(out.size() / 32);
                        if (gq >= MAX_RECORDS) return false;
                        index[g] = gq;
                        out.resize(out.size() + 32, 0.0f);
                        queue.push_back({ g, depth + 1 });
                    }
                    else
                        return false;                                // not a tree
                    links[ne++] = gq;
                }
            }
        }
#if VRH_QUAD_ORDER == 1
        // the entries were queued in order; depth-first expands the first one next
        std::reverse(queue.end() - std::count_if(links, links + ne, [](uint32_t l) { return !(l & 0x80000000u); }), queue.end());
#endif
        float* rec = &out[size_t(q) * 32];
        for (uint32_t e = 0; e < 4; ++e)
        {
            const bool used = e < ne;
            const node32& b = nodes[used ? entries[e] : entries[0]];
            for (int a = 0; a < 3; ++a)
            {
                // never_hit_unused: a point box at +inf.  For a finite origin and a finite inverse direction
                // (inf - o) * inv is +inf or -inf on every axis, never NaN: tn = +inf fails tn < max_t, or all
                // axes give -inf and tf = -inf fails tf >= 0.  Not lo = +inf, hi = -inf:
                // that box gives tn = -inf, tf = +inf and passes
                rec[a * 4 + e] = (used || !never_hit_unused) ? b.bmin[a] : INFINITY;
                rec[12 + a * 4 + e] = (used || !never_hit_unused) ? b.bmax[a] : INFINITY;
            }
            const uint32_t l = used ? links[e] : QUAD_NONE;
            std::memcpy(&rec[24 + e], &l, 4);
            if (fuse && used && (l & 0x80000000u))
            {
                // the leaf's exact box is entry e of this record: every primitive of the leaf names it
                const uint64_t first = l & 0x7FFFFFFFu, count = b.num_prims;
                if (first + count > fz->num_indices) { fuse = false; continue; }
                for (uint64_t i = first; i < first + count; ++i) fz->leaf_slot[i] = q * 4u + e;
            }
        }
    }
    root_link = 0;
    if (fuse)
    {
        // the same records and links over boxes widened outward (vrh_fused_slab.h); an unused entry is a point
        // box at +inf, which no finite ray passes
        fz->recs = out;
        for (size_t q = 0; q < out.size() / 32 && fuse; ++q)
        {
            float* rec = &fz->recs[q * 32];
            for (uint32_t e = 0; e < 4; ++e)
            {
                uint32_t l;
                std::memcpy(&l, &rec[24 + e], 4);
                for (int a = 0; a < 3; ++a)
                {
                    float& lo = rec[a * 4 + e];
                    float& hi = rec[12 + a * 4 + e];
                    lo = l == QUAD_NONE ? INFINITY : fused::widen_lo(lo, fz->omax, fz->extra);
                    hi = l == QUAD_NONE ? INFINITY : fused::widen_hi(hi, fz->omax, fz->extra);
                    if (l != QUAD_NONE && !(std::isfinite(lo) && std::isfinite(hi))) fuse = false;
                }
            }
        }
    }
    if (fz)
    {
        fz->built = fuse;
        if (!fuse) { fz->recs.clear(); fz->leaf_slot.clear(); }
    }
    return true;
}

} // namespace vrh
