// visionaray_amd/csrc/vrh_internal.h -- shared host-side declarations of libvrh.
#pragma once

#include "../../include/vrh.h"

#include <cstddef>
#include <cstdint>
#include <cstring>
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
struct generic80                                  // generic_primitive<basic_triangle<3,float>, basic_sphere<float>>
{
    union { tri64 tri; sphere48 sphere; };
    uint32_t type;                                // 1 triangle, 2 sphere (the variant's type index)
    uint32_t pad[3];
};
static_assert(sizeof(sphere48) == 48, "sphere layout");
static_assert(sizeof(generic80) == 80 && offsetof(generic80, type) == VRH_GENERIC_TYPE_OFFSET, "generic primitive layout");

// bytes of one host record of a primitive kind (0: unknown kind)
constexpr uint32_t prim_record_bytes(uint32_t kind)
{
    return kind == VRH_PRIM_TRI64 ? 64u : kind == VRH_PRIM_SPHERE48 ? 48u : kind == VRH_PRIM_GENERIC80 ? 80u : 0u;
}

// bytes of one leaf-ordered device record of a primitive kind (a generic primitive takes the triangle's)
constexpr uint32_t leaf_record_bytes(uint32_t kind) { return kind == VRH_PRIM_SPHERE48 ? 32u : 48u; }

// Device flags word of a leaf-ordered primitive (vrh_device.h): bit 0 END_BIT, bit 1 the record is a sphere
// (generic scenes only).
constexpr uint32_t PRIM_FLAG_END = 1u, PRIM_FLAG_SPHERE = 2u;

// The device leaf record of one generic primitive, three 16-byte words (the triangle format; a sphere keeps
// centre and radius in the first word, both keep prim_id, geom_id and flags in the third).  Host-only and
// header-only so that a stand-alone program can run it under a sanitizer.  False: the type index is neither
// 1 nor 2.
inline bool generic_leaf_record(const generic80& g, bool end, uint32_t out[12])
{
    for (int k = 0; k < 12; ++k) out[k] = 0u;
    if (g.type == VRH_GENERIC_TYPE_TRI)
    {
        const tri64& t = g.tri;
        const float w[9] = { t.v1[0], t.v1[1], t.v1[2], t.e1[0], t.e1[1], t.e1[2], t.e2[0], t.e2[1], t.e2[2] };
        std::memcpy(out, w, sizeof w);
        out[9] = t.prim_id; out[10] = t.geom_id; out[11] = end ? PRIM_FLAG_END : 0u;
        return true;
    }
    if (g.type == VRH_GENERIC_TYPE_SPHERE)
    {
        const sphere48& s = g.sphere;
        const float w[4] = { s.center[0], s.center[1], s.center[2], s.radius };
        std::memcpy(out, w, sizeof w);
        out[9] = s.prim_id; out[10] = s.geom_id; out[11] = PRIM_FLAG_SPHERE | (end ? PRIM_FLAG_END : 0u);
        return true;
    }
    return false;
}

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

// The host half of vrh_scene_upload (vrh_upload.cpp): the caller's tree is validated and re-laid into exactly the
// bytes the device arrays receive.  The options are those of the context and of the library the runtime is built
// for: VRH_OPT_PAIR_LAYOUT, VRH_OPT_FUSED_WIDEN, whether the kernels walk fused records, and whether their 4-wide
// step needs never-hit boxes in unused entries (build_quads).
struct upload_options
{
    int pair_layout = 0, fused_widen = 0;
    bool want_fused = false, never_hit_unused = false;
};
struct prepared_scene
{
    std::vector<float> pairs;                     // 16 floats per pair record, at least one record
    std::vector<float> prims;                     // leaf-ordered records of leaf_record_bytes(kind)
    std::vector<float> quads, fused_recs, leaf_boxes;     // empty where the scene has none
    uint32_t root = 0, num_pairs = 0, num_indices = 0, max_depth = 0, quad_depth = 0, max_prim_id = 0, max_geom_id = 0;
    float fused_omax = 0.0f;
    bool finite_bounds = true, have_quads = false, fused_built = false;
};
// VRH_OK, or VRH_ERR_INVALID with the defect in `err` (`out` is then unspecified); `indices` may be null (identity)
int prepare_scene(const void* nodes, uint32_t num_nodes, const void* prims, uint32_t num_prims, uint32_t kind,
                  const uint32_t* indices, uint32_t num_indices, const upload_options& opt, prepared_scene& out,
                  std::string& err);
// every generic primitive holds a triangle or a sphere; false: the first other type index, in `err` under the name `who`
bool check_generic_types(const void* prims, uint32_t num_prims, const char* who, std::string& err);

int build_bvh(const void* prims, uint32_t n, uint32_t kind, node32* nodes_out, uint32_t* num_nodes_out,
              uint32_t* indices_out, uint32_t* max_depth_out);

} // namespace vrh
