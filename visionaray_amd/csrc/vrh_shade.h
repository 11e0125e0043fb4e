// visionaray_amd/csrc/vrh_shade.h -- built-in shading on top of the traversal.
//
// simple::kernel (detail/simple.inl:19-83) for triangles with plastic<float> materials indexed by
// geom_id and point lights: ambient term, two-sided shading normal, one plastic::shade per light.
// Operation order is the reference's, expression by expression, compiled like the traversal with
// -ffp-contract=off and IEEE division / sqrt; the attenuation division is in double as in
// point_light.inl:20-25.  The one libm call, powf (blinn specular, brdf.h:111-122), is the device
// library's: it can differ from the host libm in the last bit, so radiance is compared with a
// relative tolerance (north star: 1e-5) while hit ids stay bit-exact.
#pragma once

#include "visionaray_hip/detail/vrh_device.h"
#include "visionaray_hip/detail/vrh_libm.h"
#include "visionaray_hip/detail/vrh_sampler.h"
#include "visionaray_hip/detail/vrh_texture.h"

namespace vrh {
namespace dev {

// device copies of vrh_plastic / vrh_point_light (include/vrh.h), 4-byte fields
struct plastic_t { float ca[3]; float ka; float cd[3]; float kd; float cs[3]; float ks; float exp; };
struct point_light_t { float position[3]; float cl[3]; float kl; float constant_att, linear_att, quadratic_att; };

// device copy of vrh_material (include/vrh.h): the kind word and the kind's parameters, fetched as four
// 16-byte loads.  p[]: plastic ca[3] ka cd[3] kd cs[3] ks exp; matte ca[3] ka cd[3] kd (the plastic
// record's first eight words); mirror cr[3] kr ior[3] absorption[3]; emissive ce[3] ls
struct __attribute__((aligned(16))) material_t { uint32_t kind; float p[15]; };
constexpr uint32_t MAT_PLASTIC = 0, MAT_MATTE = 1, MAT_MIRROR = 2, MAT_EMISSIVE = 3;

struct shade_params
{
    union
    {
        const plastic_t* materials;
        const material_t* gmaterials;   // a generic shading (vrh_shading_create_generic): EPI 5 only
    };
    const point_light_t* lights;
    uint32_t num_lights;
    uint32_t per_vertex;          // normals_per_vertex_binding
    const float4* vnormals;       // 3 per prim_id
    float ambient[4];
    float amb[3];                 // ambient[i] * ambient[3], computed on the host (the same IEEE products)
};

__device__ __forceinline__ f3 neg(f3 a) { return mk3(-a.x, -a.y, -a.z); }

// Textures (vrh_shading_set_textures; get_surface.h:422-454).  shade_params keeps its layout -- the
// untextured instances keep their argument offsets -- so the texture table hangs off the shading's device
// block: the TEX_BLOCK_BYTES before the material records hold the texture coordinates (3 per prim_id) and
// the texture descriptors (one per material: textures[geom_id]).  Only the TEX instances read it.
struct tex_block { const float2* tc; const tex_view* tex; };
constexpr uint32_t TEX_BLOCK_BYTES = 32;
constexpr uint32_t TEX_ONE = 0xFFFFFFFFu;       // a packed sample of 255s: tex_color 1.0, the dummy texture's

// tex_color of a hit as the packed RGBA8 sample: the descriptor (two 16-byte loads) and the triangle's
// three coordinates are fetched together, then the texels
__device__ inline uint32_t surface_tex(const shade_params& S, uint32_t prim_id, uint32_t mi, float u, float v)
{
    const tex_block tb = *reinterpret_cast<const tex_block*>(reinterpret_cast<const char*>(S.materials) - TEX_BLOCK_BYTES);
    const tex_view t = tb.tex[mi];
    const float2 a = tb.tc[3u * prim_id], b = tb.tc[3u * prim_id + 1u], c = tb.tc[3u * prim_id + 2u];
    if (!t.pixels) return TEX_ONE;                                     // width or height 0: C(1.0)
    return tex2d(t, tex_coord_lerp(a.x, b.x, c.x, u, v), tex_coord_lerp(a.y, b.y, c.y, u, v));
}
__device__ __forceinline__ f3 tex_rgb(uint32_t p) { return mk3(unorm8(p), unorm8(p >> 8), unorm8(p >> 16)); }

struct surface_t { f3 gn, sn; plastic_t m; uint32_t mi; uint32_t tex; };

// get_surface (get_surface.h:336-376, 576-592) for a triangle hit: normals by binding, material by
// the primitive's geom_id
// (GENERIC: the material is left to the caller, which fetches the tagged record by sf.mi)
// (TEX: sf.tex is the packed texture sample at the hit)
template <bool GENERIC = false, bool TEX = false>
__device__ inline surface_t get_surface(const shade_params& S, const float4* __restrict__ prims,
                                        const float4* __restrict__ normals, uint32_t prim_id, uint32_t li,
                                        float u, float v)
{
    surface_t sf;
    const float4* q = prims + 3u * li;
    const float4 qb = q[1], qc = q[2];
    sf.mi = __float_as_uint(qc.z);
    if constexpr (!GENERIC) sf.m = S.materials[sf.mi];
    if constexpr (TEX && !GENERIC) sf.tex = surface_tex(S, prim_id, sf.mi, u, v);
    if (!S.per_vertex)
    {
        const float4 nn = normals[prim_id];                            // get_normal.h:26-37
        sf.gn = sf.sn = mk3(nn.x, nn.y, nn.z);
    }
    else
    {
        // geometric normal of primitive(list_index) (get_normal.h:110-116), shading normal
        // lerp(n0, n1, n2, u, v) (get_shading_normal.h:64-84, math.h:466-475)
        const float4 qa = q[0];
        const f3 e1 = mk3(qa.w, qb.x, qb.y), e2 = mk3(qb.z, qb.w, qc.x);
        sf.gn = normalize(cross(e1, e2));
        const float4 a = S.vnormals[3u * prim_id], b = S.vnormals[3u * prim_id + 1u], c = S.vnormals[3u * prim_id + 2u];
        const f3 s2 = mk3(c.x, c.y, c.z) * v;
        const f3 s3 = mk3(b.x, b.y, b.z) * u;
        const f3 s1 = mk3(a.x, a.y, a.z) * (1.0f - (u + v));
        sf.sn = normalize((s1 + s2) + s3);
    }
    return sf;
}

// get_surface for a hit in a generic_primitive<triangle, sphere> BVH (VRH_PRIM_GENERIC80; get_surface.h through
// get_normal_dispatch and detail/generic_primitive_get_normal.h), per-face normal binding: a triangle takes
// normals[prim_id], a sphere (isect_pos - center) / radius with true divisions (get_normal.h:135-138,
// vector3.inl:200-203) -- its entry of `normals` is never read.  The shading normal is the geometric normal.
__device__ inline surface_t get_surface_generic(const shade_params& S, const float4* __restrict__ prims,
                                                const float4* __restrict__ normals, uint32_t prim_id, uint32_t li, f3 pos)
{
    surface_t sf;
    const float4* q = prims + 3u * li;
    const float4 qc = q[2];
    sf.mi = __float_as_uint(qc.z);
    sf.m = S.materials[sf.mi];
    if (__float_as_uint(qc.w) & SPHERE_BIT)
    {
        const float4 qa = q[0];
        sf.gn = sf.sn = mk3((pos.x - qa.x) / qa.w, (pos.y - qa.y) / qa.w, (pos.z - qa.z) / qa.w);
    }
    else
    {
        const float4 nn = normals[prim_id];                            // get_normal.h:26-37
        sf.gn = sf.sn = mk3(nn.x, nn.y, nn.z);
    }
    return sf;
}

// The device powf is v_log_f32, a multiply, v_exp_f32, and v_exp_f32 returns 0 for a result below FLT_MIN.  The host's
// powf returns the denormal, which reaches the image where a channel has no diffuse part (the reference example's
// pure colours under exponent 128).  SUBNORMAL: a zero result is formed again as the square of x^(y/2), an IEEE
// product that rounds into the denormal range as any other (and stays 0 where x^y rounds to 0); every other result
// is the builtin's, bit for bit.  Only the generic-primitive instances ask for it: the others keep their code.
template <bool SUBNORMAL>
__device__ __forceinline__ float shade_powf(float x, float y)
{
    float r = __builtin_powf(x, y);
    if constexpr (SUBNORMAL)
        if (r == 0.0f)
        {
            const float h = __builtin_powf(x, y * 0.5f);
            r = h * h;
        }
    return r;
}

// plastic::shade (plastic.inl:21-37) for one point light: pi * (lambertian + blinn) * intensity * ndotl
// (TEX: the diffuse term is tex_color * lambertian.f, plastic.inl:180-183)
template <bool TEX = false, bool SUBNORMAL = false>
__device__ inline f3 plastic_shade(const plastic_t& m, f3 n, f3 wo, f3 pos, const point_light_t& L, uint32_t tex = TEX_ONE)
{
    constexpr float PI = 3.14159265358979323846264338328e+00f;      // math.h:240 constants::pi
    constexpr float INV_PI = 3.18309886183790691216444201928e-01f;  // math.h:242 constants::inv_pi
    const f3 lpos = mk3(L.position[0], L.position[1], L.position[2]);
    const f3 wi = normalize(lpos - pos);                                // simple.inl:59
    const float ndotl = tmax(0.0f, dot(n, wi));                        // plastic.inl:29
    f3 cd = (mk3(m.cd[0], m.cd[1], m.cd[2]) * m.kd) * INV_PI;          // lambertian::f, brdf.h:36-41
    if constexpr (TEX) cd = tex_rgb(tex) * cd;
    // blinn::f, brdf.h:111-122
    const f3 h = normalize(wo + wi);
    const float hdotn = tmax(0.0f, dot(h, n));
    const f3 spec = mk3(m.cs[0], m.cs[1], m.cs[2]) * m.ks;
    const float sat = tmax(0.0f, tmin(dot(wi, h), 1.0f));              // saturate, math.h:454-457
    const float p5 = shade_powf<SUBNORMAL>(1.0f - sat, 5.0f);
    const f3 schlick = spec + mk3(1.0f - spec.x, 1.0f - spec.y, 1.0f - spec.z) * p5;
    const float nfactor = (m.exp + 2.0f) / (8.0f * PI);
    const f3 bl = (schlick * nfactor) * shade_powf<SUBNORMAL>(hdotn, m.exp);
    // point_light::intensity, point_light.inl:12-28
    const f3 dv = lpos - pos;
    const float dist = __builtin_sqrtf(dot(dv, dv));
    const float den = L.constant_att + L.linear_att * dist + L.quadratic_att * dist * dist;
    const float att = (float)(1.0 / (double)den);
    const f3 I = (mk3(L.cl[0], L.cl[1], L.cl[2]) * L.kl) * att;
    return ((PI * (cd + bl)) * I) * ndotl;
}

// colour of a closest hit, simple.inl:32-69 (the miss colour is the caller's)
// (GEN: the scene holds generic primitives -- get_surface_generic; untextured)
template <bool TEX = false, bool GEN = false>
__device__ inline float4 shade_simple(const shade_params& S, const float4* __restrict__ prims,
                                      const float4* __restrict__ normals, const ray_t& r, float t,
                                      uint32_t prim_id, const hit_extra& hx)
{
    const f3 pos = r.ori + r.dir * t;                                  // simple.inl:37
    const surface_t sf = [&]() __attribute__((always_inline)) {
        if constexpr (GEN) return get_surface_generic(S, prims, normals, prim_id, hx.li, pos);
        else return get_surface<false, TEX>(S, prims, normals, prim_id, hx.li, hx.u, hx.v);
    }();
    // plastic.inl:13-16 ambient() = ca * ka, times from_rgba(ambient_color) (spectrum.inl:375-378)
    const f3 amb = mk3(S.amb[0], S.amb[1], S.amb[2]);
    f3 shaded = (mk3(sf.m.ca[0], sf.m.ca[1], sf.m.ca[2]) * sf.m.ka) * amb;
    const f3 view = neg(r.dir);
    const f3 n = dot(sf.gn, view) < 0.0f ? neg(sf.sn) : sf.sn;       // faceforward, vector.inl:674-681
    for (uint32_t li = 0; li < S.num_lights; ++li)
        shaded = shaded + plastic_shade<TEX, GEN>(sf.m, n, view, pos, S.lights[li], sf.tex);   // simple.inl:63
    return make_float4(shaded.x, shaded.y, shaded.z, 1.0f);           // to_rgba
}

// whitted::kernel (detail/whitted.inl:186-277) as a per-lane state machine: a closest-hit ray
// (primary or reflection) that hits sets up the surface, then one any-hit shadow ray per light
// (max_t = distance to the light), then the reflection ray of the plastic fall-through bounce
// (reflect(view, shading normal), kr = 0.1, whitted.inl:64-77).  The lane keeps what the loop body
// carries between those rays.  The bounce's surface (isect_pos, two-sided shading normal,
// view_dir, shaded_clr: 12 words) is read only when a ray of the bounce ends, so it lives in LDS
// after the traversal stack ([word][lane], conflict-free), not in registers: the kernel then fits
// 96 VGPRs without spills, 5 waves / SIMD instead of 4 at 124.
struct whitted_lane
{
    f3 color;        // accumulated radiance (`color`)
    float thr;       // throughput
    uint32_t depth;  // loop iterations entered
    uint32_t li;     // light of the shadow ray in flight
    uint32_t mi;     // material (geom_id)
    uint32_t shadow; // 1 while a shadow ray is traced
    float* sm;       // LDS base of the surface words: word k of this lane at sm[base + k * stride]
    uint32_t base, stride;
    __device__ __forceinline__ float& at(uint32_t k) const { return sm[base + k * stride]; }
    __device__ __forceinline__ f3 ld3(uint32_t k) const { return mk3(at(k), at(k + 1u), at(k + 2u)); }
    __device__ __forceinline__ void st3(uint32_t k, f3 v) const { at(k) = v.x; at(k + 1u) = v.y; at(k + 2u) = v.z; }
};
constexpr uint32_t WL_POS = 0, WL_N = 3, WL_VIEW = 6, WL_SHADED = 9, WL_WORDS = 12;   // LDS words per lane

// loop body up to the light loop (whitted.inl:225-233), for a hit at t of ray r
// (TEX: *tex receives the bounce's packed texture sample, which every light of the bounce reads while its
// shadow ray is in flight: one more register of lane state, kept outside whitted_lane so that the
// untextured instances keep their code)
template <bool TEX = false, bool GEN = false>
__device__ inline void whitted_surface(const shade_params& S, const float4* __restrict__ prims,
                                       const float4* __restrict__ normals, whitted_lane& w, const ray_t& r, float t,
                                       uint32_t prim_id, const hit_extra& hx, uint32_t* tex = nullptr)
{
    const f3 pos = r.ori + r.dir * t;
    w.st3(WL_POS, pos);
    const surface_t sf = [&]() __attribute__((always_inline)) {
        if constexpr (GEN) return get_surface_generic(S, prims, normals, prim_id, hx.li, pos);
        else return get_surface<false, TEX>(S, prims, normals, prim_id, hx.li, hx.u, hx.v);
    }();
    w.mi = sf.mi;
    if constexpr (TEX) *tex = sf.tex;
    const f3 amb = mk3(S.amb[0], S.amb[1], S.amb[2]);
    w.st3(WL_SHADED, (mk3(sf.m.ca[0], sf.m.ca[1], sf.m.ca[2]) * sf.m.ka) * amb);
    const f3 view = neg(r.dir);
    w.st3(WL_VIEW, view);
    w.st3(WL_N, dot(sf.gn, view) < 0.0f ? neg(sf.sn) : sf.sn);      // faceforward
    w.li = 0;
}

// specular_bounce(plastic) = reflect(view_dir, shading_normal): 2 * dot(n, i) * n - i
// (vector.inl:683-689, whitted.inl:262) with the un-flipped shading normal sn.  Computed from the
// stored two-sided normal n = +-sn: dot(-sn, v) = -dot(sn, v) and (-d) * (-x) = d * x exactly under
// round-to-nearest, so the result is bit-identical.
__device__ inline f3 whitted_reflect(const whitted_lane& w)
{
    const f3 n = w.ld3(WL_N), view = w.ld3(WL_VIEW);
    const float d2 = 2.0f * dot(n, view);
    return mk3(d2 * n.x, d2 * n.y, d2 * n.z) - view;
}

// shadow ray of light w.li (whitted.inl:237-252): origin pushed along the light direction, any hit
// closer than the light
__device__ inline ray_t whitted_shadow_ray(const shade_params& S, const whitted_lane& w, float eps, float& max_t)
{
    const point_light_t& L = S.lights[w.li];
    const f3 lpos = mk3(L.position[0], L.position[1], L.position[2]);
    const f3 pos = w.ld3(WL_POS);
    const f3 ldir = normalize(lpos - pos);
    const f3 dv = pos - lpos;
    max_t = __builtin_sqrtf(dot(dv, dv));                              // length(isect_pos - position)
    return make_ray(pos + ldir * eps, ldir);
}

// a shadow ray ended: add the light's plastic::shade unless occluded (select(active, clr, 0))
template <bool TEX = false, bool GEN = false>
__device__ inline void whitted_light_done(const shade_params& S, whitted_lane& w, bool occluded, uint32_t tex = TEX_ONE)
{
    const f3 c = occluded ? mk3(0.0f, 0.0f, 0.0f)
               : plastic_shade<TEX, GEN>(S.materials[w.mi], w.ld3(WL_N), w.ld3(WL_VIEW), w.ld3(WL_POS), S.lights[w.li], tex);
    w.st3(WL_SHADED, w.ld3(WL_SHADED) + c);
    w.li += 1u;
}

// pathtracing::kernel (detail/pathtracing.inl:29-121) as a per-lane state machine: a chain of
// closest-hit rays, each hit sampling the plastic material for the next direction.  Between two rays
// the lane keeps the path throughput `dst`, the state of its random_sampler<float> (seeded per pixel,
// vrh_sampler.h pixel_seed) and the number of rays traced; the surface is consumed when the ray ends,
// so nothing else survives a ray.
struct pt_lane
{
    f3 dst;          // path throughput (`dst`), starts at 1
    uint32_t x;      // sampler engine state
    uint32_t bounce; // rays of this path that have ended
};

// orthonormal basis around w as lambertian / blinn::sample_f build it (brdf.h:48-54, 139-145)
__device__ __forceinline__ void pt_basis(f3 w, f3& u, f3& v)
{
    v = fabsf(w.x) > fabsf(w.y) ? normalize(mk3(-w.z, 0.0f, w.x)) : normalize(mk3(0.0f, w.z, -w.y));
    u = cross(v, w);
}

// One bounce (pathtracing.inl:73-113) for a hit at t of ray r: get_surface, two-sided normal,
// plastic::sample_impl (plastic.inl:186-230), dst *= src * (dot(n, wi) / pdf).  Returns false when
// the path dies (pdf <= 0: dst = 0); otherwise r is the next ray, from pos + wi * eps.
// Draw order: u, then the lambertian branch's cosine_sample_hemisphere(next(), next()) takes its
// SECOND argument first (the reference fixtures are g++ builds: arguments right to left), the blinn
// branch u1 then u2 (two statements).
// TEX: plastic::sample of a textured shade record (plastic.inl:62) = tex_color * sample_impl(...).
template <bool TEX = false>
__device__ inline bool pt_bounce(const shade_params& S, const float4* __restrict__ prims,
                                 const float4* __restrict__ normals, pt_lane& w, ray_t& r, float t,
                                 uint32_t prim_id, const hit_extra& hx, float eps)
{
    constexpr float PI = 3.14159265358979323846264338328e+00f;      // math.h:240-242 constants
    constexpr float TWO_PI = 6.28318530717958647692528676656e+00f;
    constexpr float INV_PI = 3.18309886183790691216444201928e-01f;
    const surface_t sf = get_surface<false, TEX>(S, prims, normals, prim_id, hx.li, hx.u, hx.v);
    const plastic_t& m = sf.m;
    const f3 wo = neg(r.dir);
    const f3 n = dot(sf.gn, wo) < 0.0f ? neg(sf.sn) : sf.sn;         // faceforward, vector.inl:674-681
    // mean_value (spectrum.inl:268-271): hadd / 3
    float prob_diff = (((m.cd[0] + m.cd[1]) + m.cd[2]) / 3.0f) * m.kd;
    float prob_spec = (((m.cs[0] + m.cs[1]) + m.cs[2]) / 3.0f) * m.ks;
    const bool all_zero = prob_diff == 0.0f && prob_spec == 0.0f;
    prob_diff = all_zero ? 0.5f : prob_diff;
    prob_spec = all_zero ? 0.5f : prob_spec;
    prob_diff = prob_diff / (prob_diff + prob_spec);
    const float u = minstd_next(w.x);
    f3 bu, bv, wi, src;
    float pdf;
    pt_basis(n, bu, bv);
    if (u < prob_diff)
    {
        // lambertian::sample_f (brdf.h:44-62), cosine_sample_hemisphere (sampling.h:61-71)
        const float u2 = minstd_next(w.x);
        const float u1 = minstd_next(w.x);
        const float rr = __builtin_sqrtf(u1);
        const float theta = TWO_PI * u2;
        const float sx = rr * libm::cosf(theta);
        const float sy = rr * libm::sinf(theta);
        const float sz = __builtin_sqrtf(tmax(0.0f, 1.0f - u1));
        wi = normalize((sx * bu + sy * bv) + sz * n);
        pdf = dot(n, wi) * INV_PI;
        src = (mk3(m.cd[0], m.cd[1], m.cd[2]) * m.kd) * INV_PI;
    }
    else
    {
        // blinn::sample_f (brdf.h:128-155), returning blinn::f (brdf.h:114-126)
        const float u1 = minstd_next(w.x);
        const float u2 = minstd_next(w.x);
        const float costheta = __builtin_powf(u1, 1.0f / (m.exp + 1.0f));
        const float sintheta = __builtin_sqrtf(tmax(0.0f, 1.0f - costheta * costheta));
        const float phi = u2 * TWO_PI;
        const f3 h = normalize(((sintheta * libm::cosf(phi)) * bu + (sintheta * libm::sinf(phi)) * bv) + costheta * n);
        const float d2 = 2.0f * dot(h, wo);                           // reflect(wo, h), vector.inl:683-689
        wi = mk3(d2 * h.x, d2 * h.y, d2 * h.z) - wo;
        const float vdoth = dot(wo, h);
        pdf = ((m.exp + 1.0f) * __builtin_powf(costheta, m.exp)) / (((2.0f * PI) * 4.0f) * vdoth);
        const f3 h2 = normalize(wo + wi);
        const float hdotn = tmax(0.0f, dot(h2, n));
        const f3 spec = mk3(m.cs[0], m.cs[1], m.cs[2]) * m.ks;
        const float sat = tmax(0.0f, tmin(dot(wi, h2), 1.0f));
        const float p5 = __builtin_powf(1.0f - sat, 5.0f);
        const f3 schlick = spec + mk3(1.0f - spec.x, 1.0f - spec.y, 1.0f - spec.z) * p5;
        const float nfactor = (m.exp + 2.0f) / (8.0f * PI);
        src = (schlick * nfactor) * __builtin_powf(hdotn, m.exp);
    }
    if (pdf <= 0.0f)
    {
        w.dst = mk3(0.0f, 0.0f, 0.0f);
        return false;
    }
    if constexpr (TEX) src = tex_rgb(sf.tex) * src;
    src = src * (dot(n, wi) / pdf);
    w.dst = mk3(w.dst.x * src.x, w.dst.y * src.y, w.dst.z * src.z);
    const f3 pos = r.ori + r.dir * t;
    r = make_ray(pos + wi * eps, wi);
    return true;
}

// The same bounce for a generic_material<plastic, matte, mirror, emissive> (detail/generic_material.inl
// sample_visitor; pathtracing.inl:73-113): the hit's record says which material samples.  The kind is
// per lane, so the bodies diverge inside a wave; the lane state between rays is pt_lane as above.
//   plastic   the code of pt_bounce: u, then two draws (lambertian second argument first, blinn u1 u2)
//   matte     lambertian::sample_f (brdf.h:44-62) with NO selection draw: two draws, second argument first
//   mirror    specular_reflection::sample_f (brdf.h:188-209): wi = reflect(wo, n), pdf = 1, no draws,
//             src = fresnel_reflectance(conductor, ior, absorption, |dot(n, wo)|) * (cr * kr) / |dot(n, wi)|
//             (fresnel.h:18-35), then * dot(n, wi) / pdf like every sampled direction
//   emissive  emissive::sample (emissive.inl:29-40, 78-82): pdf = 1, src = ce * ls, no draws; src is NOT
//             scaled by dot / pdf, dst *= src and the path ends KEEPING dst (pathtracing.inl:94-101; the
//             final select zeroes only paths still alive)
// Returns false when the path ends (emissive: dst is the pixel's radiance; pdf <= 0: dst = 0).
// Every body loads the 16-byte quarters of the record it reads where it reads them (the kind word comes
// with the first), so no lane holds all sixteen words across the sampling code.
// The last iteration of the loop (bounce == num_bounces - 1) on a hit: its sample reaches the image only
// through an emissive surface (dst *= ce * ls, the path ended); any other path is still alive after the
// loop, or was killed by pdf <= 0, and is 0 either way
// TEX: emissive (tex_color * ce) * ls (emissive.inl:89), plastic and matte tex_color * sample_impl(...)
// (plastic.inl:62, matte.inl:64); the mirror body takes no sample
template <bool TEX = false>
__device__ inline void pt_last_generic(const shade_params& S, const float4* __restrict__ prims, pt_lane& w, uint32_t li,
                                       uint32_t prim_id = 0, float u = 0.0f, float v = 0.0f)
{
    const uint32_t mi = __float_as_uint(prims[3u * li + 2u].z);
    const float4* mp = reinterpret_cast<const float4*>(S.gmaterials + mi);
    const float4 q0 = mp[0];
    f3 src = mk3(0.0f, 0.0f, 0.0f);
    if (__float_as_uint(q0.x) == MAT_EMISSIVE)
    {
        const float ls = mp[1].x;
        if constexpr (TEX) src = (tex_rgb(surface_tex(S, prim_id, mi, u, v)) * mk3(q0.y, q0.z, q0.w)) * ls;
        else
        src = mk3(q0.y, q0.z, q0.w) * ls;
        w.dst = mk3(w.dst.x * src.x, w.dst.y * src.y, w.dst.z * src.z);
    }
    else
        w.dst = src;
}

template <bool TEX = false>
__device__ inline bool pt_bounce_generic(const shade_params& S, const float4* __restrict__ prims,
                                         const float4* __restrict__ normals, pt_lane& w, ray_t& r, float t,
                                         uint32_t prim_id, const hit_extra& hx, float eps)
{
    constexpr float PI = 3.14159265358979323846264338328e+00f;      // math.h:240-242 constants
    constexpr float TWO_PI = 6.28318530717958647692528676656e+00f;
    constexpr float INV_PI = 3.18309886183790691216444201928e-01f;
    const surface_t sf = get_surface<true>(S, prims, normals, prim_id, hx.li, hx.u, hx.v);
    // words of the record: q0 = kind p0 p1 p2, q1 = p3..p6, q2 = p7..p10, q3 = p11..p14 (material_t)
    const float4* mp = reinterpret_cast<const float4*>(S.gmaterials + sf.mi);
    const uint32_t kind = __float_as_uint(mp[0].x);
    // the texture sample of the surface, taken here once for the bodies that read it (not the mirror's)
    uint32_t tex = TEX_ONE;
    if constexpr (TEX)
        if (kind != MAT_MIRROR) tex = surface_tex(S, prim_id, sf.mi, hx.u, hx.v);
    if (kind == MAT_EMISSIVE)
    {
        const float4 q0 = mp[0];
        f3 src = mk3(q0.y, q0.z, q0.w);
        if constexpr (TEX) src = tex_rgb(tex) * src;
        src = src * mp[1].x;                                          // ce_ * ls_
        w.dst = mk3(w.dst.x * src.x, w.dst.y * src.y, w.dst.z * src.z);
        return false;
    }
    const f3 wo = neg(r.dir);
    const f3 n = dot(sf.gn, wo) < 0.0f ? neg(sf.sn) : sf.sn;         // faceforward, vector.inl:674-681
    f3 wi, src;
    float pdf;
    if (kind == MAT_MIRROR)
    {
        const float4 q0 = mp[0], q1 = mp[1], q2 = mp[2];
        const float ior[3] = { q1.y, q1.z, q1.w }, absorption[3] = { q2.x, q2.y, q2.z };
        const float d2 = 2.0f * dot(n, wo);                           // reflect(wo, n), vector.inl:683-689
        wi = mk3(d2 * n.x, d2 * n.y, d2 * n.z) - wo;
        pdf = 1.0f;
        const float cosi = fabsf(dot(n, wo));
        float fr[3];
        for (int c = 0; c < 3; ++c)
        {
            // fresnel_reflectance(conductor_tag, eta, k, cosi), fresnel.h:18-35
            const float eta = ior[c], k = absorption[c];
            const float a = eta * eta + k * k;
            const float b = (2.0f * eta) * cosi;
            const float rs2 = ((a - b) + cosi * cosi) / ((a + b) + cosi * cosi);
            const float rp2 = (((a * cosi) * cosi - b) + 1.0f) / (((a * cosi) * cosi + b) + 1.0f);
            fr[c] = (rs2 + rp2) / 2.0f;
        }
        const f3 crkr = mk3(q0.y, q0.z, q0.w) * q1.x;
        const float adot = fabsf(dot(n, wi));
        src = mk3((fr[0] * crkr.x) / adot, (fr[1] * crkr.y) / adot, (fr[2] * crkr.z) / adot);
    }
    else
    {
        bool diffuse = true;                                          // matte: lambertian, no selection draw
        if (kind == MAT_PLASTIC)
        {
            // plastic::sample_impl (plastic.inl:186-230), mean_value (spectrum.inl:268-271): hadd / 3
            const float4 q1 = mp[1], q2 = mp[2];
            float prob_diff = (((q1.y + q1.z) + q1.w) / 3.0f) * q2.x;
            float prob_spec = (((q2.y + q2.z) + q2.w) / 3.0f) * mp[3].x;
            const bool all_zero = prob_diff == 0.0f && prob_spec == 0.0f;
            prob_diff = all_zero ? 0.5f : prob_diff;
            prob_spec = all_zero ? 0.5f : prob_spec;
            prob_diff = prob_diff / (prob_diff + prob_spec);
            const float u = minstd_next(w.x);
            diffuse = u < prob_diff;
        }
        f3 bu, bv;
        pt_basis(n, bu, bv);
        if (diffuse)
        {
            // lambertian::sample_f (brdf.h:44-62), cosine_sample_hemisphere (sampling.h:61-71)
            const float u2 = minstd_next(w.x);
            const float u1 = minstd_next(w.x);
            const float rr = __builtin_sqrtf(u1);
            const float theta = TWO_PI * u2;
            const float sx = rr * libm::cosf(theta);
            const float sy = rr * libm::sinf(theta);
            const float sz = __builtin_sqrtf(tmax(0.0f, 1.0f - u1));
            wi = normalize((sx * bu + sy * bv) + sz * n);
            pdf = dot(n, wi) * INV_PI;
            const float4 q1 = mp[1];
            src = (mk3(q1.y, q1.z, q1.w) * mp[2].x) * INV_PI;
        }
        else
        {
            // blinn::sample_f (brdf.h:128-155), returning blinn::f (brdf.h:114-126)
            const float4 q2 = mp[2], q3 = mp[3];
            const float ex = q3.y;
            const float u1 = minstd_next(w.x);
            const float u2 = minstd_next(w.x);
            const float costheta = __builtin_powf(u1, 1.0f / (ex + 1.0f));
            const float sintheta = __builtin_sqrtf(tmax(0.0f, 1.0f - costheta * costheta));
            const float phi = u2 * TWO_PI;
            const f3 h = normalize(((sintheta * libm::cosf(phi)) * bu + (sintheta * libm::sinf(phi)) * bv) + costheta * n);
            const float d2 = 2.0f * dot(h, wo);                       // reflect(wo, h), vector.inl:683-689
            wi = mk3(d2 * h.x, d2 * h.y, d2 * h.z) - wo;
            const float vdoth = dot(wo, h);
            pdf = ((ex + 1.0f) * __builtin_powf(costheta, ex)) / (((2.0f * PI) * 4.0f) * vdoth);
            const f3 h2 = normalize(wo + wi);
            const float hdotn = tmax(0.0f, dot(h2, n));
            const f3 spec = mk3(q2.y, q2.z, q2.w) * q3.x;
            const float sat = tmax(0.0f, tmin(dot(wi, h2), 1.0f));
            const float p5 = __builtin_powf(1.0f - sat, 5.0f);
            const f3 schlick = spec + mk3(1.0f - spec.x, 1.0f - spec.y, 1.0f - spec.z) * p5;
            const float nfactor = (ex + 2.0f) / (8.0f * PI);
            src = (schlick * nfactor) * __builtin_powf(hdotn, ex);
        }
    }
    if (pdf <= 0.0f)
    {
        w.dst = mk3(0.0f, 0.0f, 0.0f);
        return false;
    }
    if constexpr (TEX) src = tex_rgb(tex) * src;                      // mirror: tex is TEX_ONE, x * 1.0f = x
    src = src * (dot(n, wi) / pdf);
    w.dst = mk3(w.dst.x * src.x, w.dst.y * src.y, w.dst.z * src.z);
    const f3 pos = r.ori + r.dir * t;
    r = make_ray(pos + wi * eps, wi);
    return true;
}

// per-lane sorted hit list of multi_hit<N> in LDS, column-major [field][entry][lane]
struct mh_list
{
    uint32_t* mem;
    uint32_t base;       // lane's word offset of field 0, entry 0
    uint32_t stride;     // words between consecutive entries (= threads per block)
    uint32_t n;          // N
    __device__ __forceinline__ uint32_t& at(uint32_t field, uint32_t k) const { return mem[base + (field * n + k) * stride]; }
    __device__ __forceinline__ float t(uint32_t k) const { return __uint_as_float(at(0, k)); }
    __device__ __forceinline__ void reset() const
    {
        for (uint32_t k = 0; k < n; ++k) { at(0, k) = __float_as_uint(FMAX); at(1, k) = 0xFFFFFFFFu; }
    }
    // insert_sorted (algorithm.h:46-75) with is_closer_t (update_if.h:48-56): the first entry whose
    // t is larger takes the hit, later entries shift down, the last one drops out.  Returns the
    // new N-th t (the culling distance of multi_hit, multi_hit.h:221-244).
    __device__ __forceinline__ float insert(float t_new, uint32_t pid, uint32_t li, float u, float v) const
    {
        uint32_t pos = n - 1u;
        for (uint32_t k = 0; k < n; ++k)
            if (t_new < t(k)) { pos = k; break; }
        for (uint32_t k = n - 1u; k > pos; --k)
            for (uint32_t f = 0; f < 5u; ++f) at(f, k) = at(f, k - 1u);
        at(0, pos) = __float_as_uint(t_new); at(1, pos) = pid; at(2, pos) = li;
        at(3, pos) = __float_as_uint(u); at(4, pos) = __float_as_uint(v);
        return t(n - 1u);
    }
};

// examples/multi_hit/main.cpp:178-235: every kept hit (t order) shaded with the first light,
// alpha 0.3, composited front to back; colour starts at 0
__device__ inline float4 shade_multi(const shade_params& S, const float4* __restrict__ prims,
                                     const float4* __restrict__ normals, const ray_t& r, const mh_list& L)
{
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (uint32_t k = 0; k < L.n; ++k)
    {
        const float t = L.t(k);
        if (!(t < FMAX)) break;
        const f3 pos = r.ori + r.dir * t;
        const surface_t sf = get_surface(S, prims, normals, L.at(1, k), L.at(2, k), __uint_as_float(L.at(3, k)),
                                         __uint_as_float(L.at(4, k)));
        const f3 view = neg(r.dir);
        const f3 n = dot(sf.gn, view) < 0.0f ? neg(sf.sn) : sf.sn;
        f3 c = S.num_lights ? plastic_shade(sf.m, n, view, pos, S.lights[0]) : mk3(0.0f, 0.0f, 0.0f);
        const float a = 0.3f;
        c = c * a;
        const float f = 1.0f - acc.w;
        acc = make_float4(acc.x + c.x * f, acc.y + c.y * f, acc.z + c.z * f, acc.w + a * f);
    }
    return acc;
}

} // namespace dev
} // namespace vrh
