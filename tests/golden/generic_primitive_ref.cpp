// tests/golden/generic_primitive_ref.cpp -- fixture generator for mixed triangle / sphere scenes
// (VRH_PRIM_GENERIC80: generic_primitive<basic_triangle<3, float>, basic_sphere<float>> in one BVH).
//
// Runs the reference's own builder and kernels on the CPU, from the reference's headers (never copied into
// this repository), over a scene file written by make_generic_primitive_golden.py:
//
//     generic_primitive_ref <scene.bin> <out.bin>
//
// scene.bin: the `header` below, the plastic materials (13 floats each: ca[3] ka cd[3] kd cs[3] ks exp), the
// point lights (10 floats each: position[3] cl[3] kl constant linear quadratic), the primitives as 80-byte
// records (the alternative's bytes at 0 -- basic_triangle<3, float> 64 B or basic_sphere<float> 48 B -- and the
// u32 type index at 64: 1 triangle, 2 sphere) and the normals as float4 rows, one per prim_id (a sphere's row
// is never read).
// out.bin: u32 num_nodes, the nodes (32 B each), the indices (u32 per primitive), then per pixel, W x H each:
//   primary   prim id (0xFFFFFFFF: miss), t (-1: miss)
//   AO        occlusion mask (u8), colour (float4) -- ao/main.cpp's body with the project's deterministic AO
//             sample spec (oracle/ref_harness.cpp ao_sample), the normal taken through get_surface
//   simple    colour (float4) of simple::kernel
//   whitted   colour (float4) of whitted::kernel, and a u8 that is 1 where two consecutive closest hits of the
//             pixel's path lie on primitives of different kinds (a reflection from a sphere onto a triangle or
//             the reverse)
// The program checks that the reference's record is 80 bytes with the type index at 64 and that every
// record it builds equals the file's in the alternative's bytes and the type index.
#include <visionaray/math/math.h>
#include <visionaray/bvh.h>
#include <visionaray/generic_primitive.h>
#include <visionaray/get_normal.h>
#include <visionaray/get_surface.h>
#include <visionaray/intersector.h>
#include <visionaray/kernels.h>
#include <visionaray/material.h>
#include <visionaray/point_light.h>
#include <visionaray/result_record.h>
#include <visionaray/traverse.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace visionaray;

using tri_t = basic_triangle<3, float>;
using sphere_t = basic_sphere<float>;
using prim_t = generic_primitive<tri_t, sphere_t>;

struct header
{
    uint32_t magic;          // 0x50475246
    uint32_t W, H, num_prims, num_materials, num_lights, num_bounces;
    uint32_t ao_samples;     // 8 (the sample spec's counter is p * 8 + sample)
    float eps;               // simple / whitted epsilon
    float ao_radius, ao_eps;
    float bg[4], ambient[4];
    float eye[3], cam_u[3], cam_v[3], cam_w[3];
};

// SURVEY.md Appendix A counter hash and the parity AO sampler (frame 0)
static uint32_t wang(uint32_t a)
{
    a = (a ^ 61u) ^ (a >> 16);
    a = a + (a << 3);
    a = a ^ (a >> 4);
    a = a * 0x27d4eb2du;
    a = a ^ (a >> 15);
    return a;
}
static float U(uint32_t k) { return float(wang(k) >> 8) * (1.0f / 16777216.0f); }
static vec2 ao_sample(uint32_t p, int smp)
{
    for (uint32_t k = 0; k < 16; ++k)
    {
        uint32_t ctr = ((p * 8u + uint32_t(smp)) * 16u + k) * 2u;
        float xa = 2.0f * U(ctr) - 1.0f;
        float ya = 2.0f * U(ctr + 1) - 1.0f;
        if (xa * xa + ya * ya < 1.0f) return vec2(xa, ya);
    }
    return vec2(0.0f, 0.0f);
}

// records the prim ids of a pixel's closest hits, in order
struct path_intersector : basic_intersector<path_intersector>
{
    using basic_intersector<path_intersector>::operator();

    std::vector<uint32_t> hits;

    template <typename R, typename P, typename Cond, typename = typename std::enable_if<is_any_bvh<P>::value>::type>
    auto operator()(detail::closest_hit_tag, multi_hit_max<1>, R const& ray, P const& prim, typename R::scalar_type max_t,
                    Cond update_cond = Cond())
        -> decltype(intersect<detail::ClosestHit>(ray, prim, std::declval<path_intersector&>(), max_t, update_cond))
    {
        auto hr = intersect<detail::ClosestHit>(ray, prim, *this, max_t, update_cond);
        hits.push_back(hr.hit ? uint32_t(hr.prim_id) : 0xFFFFFFFFu);
        return hr;
    }
};

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s <scene.bin> <out.bin>\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    header h;
    if (!in || fread(&h, sizeof(h), 1, in) != 1 || h.magic != 0x50475246u) { fprintf(stderr, "bad scene file\n"); return 3; }
    if (h.ao_samples != 8u) { fprintf(stderr, "the AO sample spec has 8 samples\n"); return 3; }

    aligned_vector<plastic<float>> materials;
    for (uint32_t i = 0; i < h.num_materials; ++i)
    {
        float m[13];
        if (fread(m, 4, 13, in) != 13) return 3;
        plastic<float> p;
        p.set_ca(from_rgb(vec3(m[0], m[1], m[2])));
        p.set_ka(m[3]);
        p.set_cd(from_rgb(vec3(m[4], m[5], m[6])));
        p.set_kd(m[7]);
        p.set_cs(from_rgb(vec3(m[8], m[9], m[10])));
        p.set_ks(m[11]);
        p.set_specular_exp(m[12]);
        materials.push_back(p);
    }
    aligned_vector<point_light<float>> lights;
    for (uint32_t i = 0; i < h.num_lights; ++i)
    {
        float l[10];
        if (fread(l, 4, 10, in) != 10) return 3;
        point_light<float> pl;
        pl.set_position(vec3(l[0], l[1], l[2]));
        pl.set_cl(vec3(l[3], l[4], l[5]));
        pl.set_kl(l[6]);
        pl.set_constant_attenuation(l[7]);
        pl.set_linear_attenuation(l[8]);
        pl.set_quadratic_attenuation(l[9]);
        lights.push_back(pl);
    }

    static_assert(sizeof(tri_t) == 64, "basic_triangle<3, float> is 64 bytes");
    static_assert(sizeof(sphere_t) == 48, "basic_sphere<float> is 48 bytes");
    static_assert(sizeof(prim_t) == 80 && alignof(prim_t) == 16, "the generic primitive record is 80 bytes, aligned to 16");
    aligned_vector<prim_t> prims(h.num_prims);
    std::vector<uint8_t> is_sphere(h.num_prims, 0);      // by prim_id
    for (uint32_t i = 0; i < h.num_prims; ++i)
    {
        unsigned char rec[80];
        if (fread(rec, 80, 1, in) != 1) return 3;
        uint32_t type;
        std::memcpy(&type, rec + 64, 4);
        size_t used = 0;
        if (type == 1u) { tri_t t; std::memcpy(&t, rec, sizeof(t)); prims[i] = t; used = sizeof(t); }
        else if (type == 2u)
        {
            sphere_t s; std::memcpy(&s, rec, sizeof(s)); prims[i] = s; used = sizeof(s);
            if (s.prim_id >= h.num_prims) return 3;
            is_sphere[s.prim_id] = 1;
        }
        else { fprintf(stderr, "primitive %u: type index %u\n", i, type); return 3; }
        // the layout the product takes verbatim: the alternative's bytes at 0, the type index at 64
        // (ids first: bytes 8..15 of either alternative are padding, as is the tail of a vector's 16 bytes)
        const unsigned char* mine = reinterpret_cast<const unsigned char*>(&prims[i]);
        uint32_t mytype;
        std::memcpy(&mytype, mine + 64, 4);
        bool same = mytype == type && std::memcmp(mine, rec, 8) == 0;
        for (size_t o = 16; o < used; o += 16) same = same && std::memcmp(mine + o, rec + o, o == 32 && type == 2u ? 4 : 12) == 0;
        if (!same) { fprintf(stderr, "primitive %u: the reference's record differs from the file's\n", i); return 5; }
    }
    std::vector<float> raw(size_t(h.num_prims) * 4);
    if (fread(raw.data(), 16, h.num_prims, in) != h.num_prims) return 3;
    fclose(in);
    aligned_vector<vec3> normals(h.num_prims);
    for (size_t i = 0; i < h.num_prims; ++i) normals[i] = vec3(raw[4 * i], raw[4 * i + 1], raw[4 * i + 2]);

    auto bvh = build<index_bvh<prim_t>>(prims.data(), prims.size());
    using bvh_ref = index_bvh<prim_t>::bvh_ref;
    std::vector<bvh_ref> bvhs{ bvh.ref() };
    vec4 bg(h.bg[0], h.bg[1], h.bg[2], h.bg[3]), ambient(h.ambient[0], h.ambient[1], h.ambient[2], h.ambient[3]);
    auto kp = make_kernel_params(normals_per_face_binding{}, bvhs.data(), bvhs.data() + bvhs.size(), normals.data(),
                                 materials.data(), lights.data(), lights.data() + lights.size(), h.num_bounces, h.eps, bg,
                                 ambient);
    simple::kernel<decltype(kp)> simple_k;
    simple_k.params = kp;
    whitted::kernel<decltype(kp)> whitted_k;
    whitted_k.params = kp;

    const vec3 eye(h.eye[0], h.eye[1], h.eye[2]), cam_u(h.cam_u[0], h.cam_u[1], h.cam_u[2]);
    const vec3 cam_v(h.cam_v[0], h.cam_v[1], h.cam_v[2]), cam_w(h.cam_w[0], h.cam_w[1], h.cam_w[2]);
    const size_t npx = size_t(h.W) * h.H;
    std::vector<uint32_t> pid(npx, 0xFFFFFFFFu);
    std::vector<float> tval(npx, -1.0f), ao_color(npx * 4), simple_color(npx * 4), whitted_color(npx * 4);
    std::vector<uint8_t> occ(npx, 0), cross(npx, 0);
    for (uint32_t y = 0; y < h.H; ++y)
        for (uint32_t x = 0; x < h.W; ++x)
        {
            // sched_common.h:130-150 make_primary_ray_impl
            const float u = 2.0f * (float(x) + 0.5f) / float(h.W) - 1.0f;
            const float v = 2.0f * (float(y) + 0.5f) / float(h.H) - 1.0f;
            ray r;
            r.ori = eye;
            r.dir = normalize(cam_u * u + cam_v * v + cam_w);
            const size_t p = size_t(y) * h.W + x;

            // primary visibility and AO (ao/main.cpp:183-246)
            auto hr = closest_hit(r, kp.prims.begin, kp.prims.end);
            vec4 clr = bg;
            if (hr.hit)
            {
                pid[p] = uint32_t(hr.prim_id);
                tval[p] = hr.t;
                hr.isect_pos = r.ori + r.dir * hr.t;
                auto surf = get_surface(hr, kp);
                vec3 n = surf.geometric_normal;
                vec3 uu, vv, w = n;
                make_orthonormal_basis(uu, vv, w);
                vec4 c(1.0f);
                uint8_t mask = 0;
                for (int smp = 0; smp < 8; ++smp)
                {
                    vec2 sxy = ao_sample(uint32_t(p), smp);
                    float sx = sxy.x, sy = sxy.y;
                    float sz = sqrt(std::max(0.0f, 1.0f - sx * sx - sy * sy));
                    auto dir = normalize(sx * uu + sy * vv + sz * w);
                    ray ao;
                    ao.ori = hr.isect_pos + dir * h.ao_eps;
                    ao.dir = dir;
                    auto ar = any_hit(ao, kp.prims.begin, kp.prims.end, h.ao_radius);
                    if (ar.hit) { c = c - 1.0f / 8; mask |= uint8_t(1u << smp); }
                }
                occ[p] = mask;
                clr = vec4(c.xyz(), 1.0f);
            }
            std::memcpy(&ao_color[4 * p], &clr, 16);

            {
                path_intersector isect;
                result_record<float> res = simple_k(isect, r);
                const float c4[4] = { res.color.x, res.color.y, res.color.z, res.color.w };
                std::memcpy(&simple_color[4 * p], c4, 16);
            }
            {
                path_intersector isect;
                result_record<float> res = whitted_k(isect, r);
                const float c4[4] = { res.color.x, res.color.y, res.color.z, res.color.w };
                std::memcpy(&whitted_color[4 * p], c4, 16);
                for (size_t k = 0; k + 1 < isect.hits.size(); ++k)
                {
                    const uint32_t a = isect.hits[k], b = isect.hits[k + 1];
                    if (a != 0xFFFFFFFFu && b != 0xFFFFFFFFu && is_sphere[a] != is_sphere[b]) cross[p] = 1;
                }
            }
        }

    FILE* out = fopen(argv[2], "wb");
    if (!out) return 4;
    const uint32_t nn = uint32_t(bvh.nodes().size());
    static_assert(sizeof(bvh_node) == 32, "bvh_node is 32 bytes");
    bool ok = fwrite(&nn, 4, 1, out) == 1 && fwrite(bvh.nodes().data(), 32, nn, out) == nn
           && fwrite(bvh.indices().data(), 4, bvh.indices().size(), out) == bvh.indices().size()
           && bvh.indices().size() == h.num_prims
           && fwrite(pid.data(), 4, npx, out) == npx && fwrite(tval.data(), 4, npx, out) == npx
           && fwrite(occ.data(), 1, npx, out) == npx && fwrite(ao_color.data(), 16, npx, out) == npx
           && fwrite(simple_color.data(), 16, npx, out) == npx && fwrite(whitted_color.data(), 16, npx, out) == npx
           && fwrite(cross.data(), 1, npx, out) == npx;
    fclose(out);
    return ok ? 0 : 4;
}
