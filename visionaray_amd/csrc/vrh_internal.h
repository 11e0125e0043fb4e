// visionaray_amd/csrc/vrh_internal.h -- shared host-side declarations of libvrh.
#pragma once

#include "../../include/vrh.h"

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace vrh {

// Reference binary layouts
struct node32                                     // bvh_node, bvh.h:52-119
{
    float    bmin[3];
    uint32_t first;                               // first_child (inner) | first_prim (leaf)
    float    bmax[3];
    uint32_t num_prims;                           // 0 = inner
};
struct tri64                                      // basic_triangle<3,float>
{
    uint32_t geom_id, prim_id, pad[2];
    float    v1[4], e1[4], e2[4];
};
struct sphere48                                   // basic_sphere<float>
{
    uint32_t geom_id, prim_id, pad[2];
    float    center[4];
    float    radius, pad2[3];
};
static_assert(sizeof(node32) == 32, "node layout");
static_assert(sizeof(tri64) == 64, "triangle layout");
static_assert(sizeof(sphere48) == 48, "sphere layout");

void set_error(const std::string& msg);

constexpr uint32_t QUAD_NONE = 0xFFFFFFFFu;     // unused entry of a 4-wide record

// 4-wide any-hit records from the binary BVH (vrh_quad.cpp); false = the scene keeps the binary
// path (containment or box validity does not hold, or the root is a leaf)
// `fz` (optional): the fused records of the AO kernel's 4-wide step (vrh_fused_slab.h) -- the same records over
// boxes widened for ray origins within `omax` (and by at least `extra`), and per leaf-ordered primitive the
// entry (record * 4 + entry) of `out` that holds its leaf's exact box.  Built only if every node's box is valid
// and lies inside its parent's; `out` does not depend on it.
// `never_hit_unused`: the boxes of unused entries (link QUAD_NONE) in `out` are point boxes at +inf, which no ray
// with finite origin and inverse direction passes, instead of copies of entry 0's box.
struct fused_records
{
    float omax = 0.0f, extra = 0.0f;              // in
    uint32_t num_indices = 0;                     // in: leaf-ordered primitives
    std::vector<float> recs;                      // out
    std::vector<uint32_t> leaf_slot;              // out
    bool built = false;                           // out
};
bool build_quads(const node32* nodes, uint32_t num_nodes, std::vector<float>& out, uint32_t& root_link,
                 uint32_t& quad_depth, fused_records* fz = nullptr, bool never_hit_unused = false);

int build_bvh(const void* prims, uint32_t n, uint32_t kind, node32* nodes_out, uint32_t* num_nodes_out,
              uint32_t* indices_out, uint32_t* max_depth_out);

} // namespace vrh
