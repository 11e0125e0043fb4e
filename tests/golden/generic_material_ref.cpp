// tests/golden/generic_material_ref.cpp -- fixture generator for the path tracer over tagged materials
// (VRH_KERNEL_PATHTRACING with a shading of vrh_shading_create_generic).
//
// Runs the reference's own pathtracing::kernel (detail/pathtracing.inl) on the CPU, from the reference's
// headers (never copied into this repository), with generic_material<plastic<float>, matte<float>,
// mirror<float>, emissive<float>> materials, over a scene file written by make_generic_material_golden.py:
//
//     generic_material_ref <scene.bin> <out.bin>
//
// scene.bin: the `header` below, then the materials as tagged records (vrh_material, include/vrh.h: the
// kind word and 15 floats -- plastic ca[3] ka cd[3] kd cs[3] ks exp, matte ca[3] ka cd[3] kd, mirror
// cr[3] kr ior[3] absorption[3], emissive ce[3] ls), the triangles (basic_triangle<3, float>, 64 B each)
// and the normals as float4 rows (one per triangle, or three with the per-vertex binding).
// out.bin: per snapshot W x H float4 colours (one snapshot, or with the accumulation mode the target
// after the first and after the last frame), then per pixel of the LAST frame a u64 path signature, a
// u32 ray count, the first ray's prim id (0xFFFFFFFF: miss) and t (-1: miss), then a u64 total of
// closest_hit calls over all frames.
//
// Seeding, the counting intersector with its path signature, the accumulation mode and the powf shift
// are those of tests/golden/pathtrace_ref.cpp (see there); built by g++ with the same line, so the two
// sampler.next() arguments of cosine_sample_hemisphere(...) are evaluated right to left.
#include <visionaray/math/math.h>
#include <visionaray/bvh.h>
#include <visionaray/generic_material.h>
#include <visionaray/get_normal.h>
#include <visionaray/intersector.h>
#include <visionaray/kernels.h>
#include <visionaray/material.h>
#include <visionaray/point_light.h>
#include <visionaray/random_sampler.h>
#include <visionaray/result_record.h>
#include <visionaray/traverse.h>

#include <dlfcn.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace visionaray;

using tri_t = basic_triangle<3, float>;
using material_t = generic_material<plastic<float>, matte<float>, mirror<float>, emissive<float>>;

static int g_pow_shift = 0;

extern "C" float powf(float x, float y)
{
    typedef float (*fn_t)(float, float);
    static fn_t real = (fn_t)dlsym(RTLD_NEXT, "powf");
    float r = real(x, y);
    if (g_pow_shift == 0 || y == 0.0f || x == 1.0f || r == 0.0f || !std::isfinite(r)) return r;
    return nextafterf(r, g_pow_shift > 0 ? INFINITY : -INFINITY);
}

struct header
{
    uint32_t magic;          // 0x4D545246
    uint32_t W, H, num_prims, per_vertex, num_materials, num_bounces;
    uint32_t first_frame;    // frame number (accumulation: of the first frame, >= 1)
    uint32_t accum;          // 0: one uniform-sampler frame; n: n jittered_blend frames
    int32_t pow_shift;
    float eps;
    float bg[4], ambient[4];
    float eye[3], cam_u[3], cam_v[3], cam_w[3];
};

static unsigned rs_hash(unsigned a)
{
    a = (a + 0x7ed55d16u) + (a << 12);
    a = (a ^ 0xc761c23cu) ^ (a >> 19);
    a = (a + 0x165667b1u) + (a << 5);
    a = (a + 0xd3a2646cu) ^ (a << 9);
    a = (a + 0xfd7046c5u) + (a << 3);
    a = (a ^ 0xb55a4f09u) ^ (a >> 16);
    return a;
}

// the Appendix-A hash of the jitter draws (include/vrh.h vrh_pixel_sampler)
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

// counts the closest_hit calls of a path and hashes their results
struct path_intersector : basic_intersector<path_intersector>
{
    using basic_intersector<path_intersector>::operator();

    uint32_t calls = 0;
    uint32_t first_prim = 0xFFFFFFFFu;      // the first ray's hit
    float first_t = -1.0f;
    uint64_t sig = 0xcbf29ce484222325ull;

    void u32(uint32_t v)
    {
        for (int i = 0; i < 4; ++i) { sig ^= (v >> (8 * i)) & 0xFFu; sig *= 0x100000001b3ull; }
    }

    template <typename R, typename P, typename Cond, typename = typename std::enable_if<is_any_bvh<P>::value>::type>
    auto operator()(detail::closest_hit_tag, multi_hit_max<1>, R const& ray, P const& prim, typename R::scalar_type max_t,
                    Cond update_cond = Cond())
        -> decltype(intersect<detail::ClosestHit>(ray, prim, std::declval<path_intersector&>(), max_t, update_cond))
    {
        auto hr = intersect<detail::ClosestHit>(ray, prim, *this, max_t, update_cond);
        if (calls == 0 && hr.hit) { first_prim = uint32_t(hr.prim_id); first_t = hr.t; }
        ++calls;
        u32(hr.hit ? uint32_t(hr.prim_id) : 0xFFFFFFFFu);
        return hr;
    }
};

template <typename Binding>
static int run(header const& h, std::vector<material_t> const& materials, aligned_vector<tri_t>& prims,
               std::vector<vec3> const& normals, FILE* out)
{
    auto bvh = build<index_bvh<tri_t>>(prims.data(), prims.size());
    using bvh_ref = index_bvh<tri_t>::bvh_ref;
    std::vector<bvh_ref> bvhs{ bvh.ref() };
    std::vector<point_light<float>> lights;   // none: the path tracer is lit by the environment
    vec4 bg(h.bg[0], h.bg[1], h.bg[2], h.bg[3]), ambient(h.ambient[0], h.ambient[1], h.ambient[2], h.ambient[3]);
    auto kp = make_kernel_params(Binding{}, bvhs.data(), bvhs.data() + bvhs.size(), normals.data(), materials.data(),
                                 lights.data(), lights.data() + lights.size(), h.num_bounces, h.eps, bg, ambient);
    pathtracing::kernel<decltype(kp)> kern;
    kern.params = kp;

    const vec3 eye(h.eye[0], h.eye[1], h.eye[2]), cam_u(h.cam_u[0], h.cam_u[1], h.cam_u[2]);
    const vec3 cam_v(h.cam_v[0], h.cam_v[1], h.cam_v[2]), cam_w(h.cam_w[0], h.cam_w[1], h.cam_w[2]);
    const size_t npx = size_t(h.W) * h.H;
    std::vector<float> target(npx * 4, 0.0f);
    std::vector<uint64_t> sig(npx);
    std::vector<uint32_t> nrays(npx), fprim(npx);
    std::vector<float> ft(npx);
    uint64_t total = 0;
    const uint32_t frames = h.accum ? h.accum : 1u;
    for (uint32_t f = 0; f < frames; ++f)
    {
        const uint32_t n = h.first_frame + f;
        for (uint32_t y = 0; y < h.H; ++y)
            for (uint32_t x = 0; x < h.W; ++x)
            {
                float fx = float(x), fy = float(y);
                if (h.accum)
                {
                    const uint32_t k = (y * h.W + x) * 2u + 0x632BE5ABu + n * 0x68E31DA4u;
                    fy = fy + (U(k) - 0.5f);
                    fx = fx + (U(k + 1u) - 0.5f);
                }
                // sched_common.h:130-150 make_primary_ray_impl
                const float u = 2.0f * (fx + 0.5f) / float(h.W) - 1.0f;
                const float v = 2.0f * (fy + 0.5f) / float(h.H) - 1.0f;
                ray r;
                r.ori = eye;
                r.dir = normalize(cam_u * u + cam_v * v + cam_w);
                random_sampler<float> samp(rs_hash(n * h.W * h.H + y * h.W + x));
                path_intersector isect;
                result_record<float> res = kern(isect, r, samp);
                const size_t p = size_t(y) * h.W + x;
                isect.u32(isect.calls);
                sig[p] = isect.sig;
                nrays[p] = isect.calls;
                fprim[p] = isect.first_prim;
                ft[p] = isect.first_t;
                total += isect.calls;
                const float c[4] = { res.color.x, res.color.y, res.color.z, res.color.w };
                if (h.accum)
                {
                    const float s = 1.0f / float(n), d = 1.0f - s;
                    for (int i = 0; i < 4; ++i) target[4 * p + i] = c[i] * s + target[4 * p + i] * d;
                }
                else
                    for (int i = 0; i < 4; ++i) target[4 * p + i] = c[i];
            }
        if (f == 0 || f + 1 == frames)
            if (fwrite(target.data(), 4, target.size(), out) != target.size()) return 4;
        if (frames == 1) break;
    }
    if (fwrite(sig.data(), 8, npx, out) != npx || fwrite(nrays.data(), 4, npx, out) != npx
        || fwrite(fprim.data(), 4, npx, out) != npx || fwrite(ft.data(), 4, npx, out) != npx || fwrite(&total, 8, 1, out) != 1)
        return 4;
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s <scene.bin> <out.bin>\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    header h;
    if (!in || fread(&h, sizeof(h), 1, in) != 1 || h.magic != 0x4D545246u) { fprintf(stderr, "bad scene file\n"); return 3; }
    g_pow_shift = h.pow_shift;
    std::vector<material_t> materials;
    for (uint32_t i = 0; i < h.num_materials; ++i)
    {
        uint32_t kind;
        float m[15];
        if (fread(&kind, 4, 1, in) != 1 || fread(m, 4, 15, in) != 15) return 3;
        if (kind == 0)
        {
            plastic<float> p;
            p.set_ca(from_rgb(vec3(m[0], m[1], m[2])));
            p.set_ka(m[3]);
            p.set_cd(from_rgb(vec3(m[4], m[5], m[6])));
            p.set_kd(m[7]);
            p.set_cs(from_rgb(vec3(m[8], m[9], m[10])));
            p.set_ks(m[11]);
            p.set_specular_exp(m[12]);
            materials.emplace_back(p);
        }
        else if (kind == 1)
        {
            matte<float> p;
            p.set_ca(from_rgb(vec3(m[0], m[1], m[2])));
            p.set_ka(m[3]);
            p.set_cd(from_rgb(vec3(m[4], m[5], m[6])));
            p.set_kd(m[7]);
            materials.emplace_back(p);
        }
        else if (kind == 2)
        {
            mirror<float> p;
            p.set_cr(from_rgb(vec3(m[0], m[1], m[2])));
            p.set_kr(m[3]);
            p.set_ior(spectrum<float>(from_rgb(vec3(m[4], m[5], m[6]))));
            p.set_absorption(spectrum<float>(from_rgb(vec3(m[7], m[8], m[9]))));
            materials.emplace_back(p);
        }
        else if (kind == 3)
        {
            emissive<float> p;
            p.set_ce(from_rgb(vec3(m[0], m[1], m[2])));
            p.set_ls(m[3]);
            materials.emplace_back(p);
        }
        else { fprintf(stderr, "unknown material kind %u\n", kind); return 3; }
    }
    static_assert(sizeof(tri_t) == 64, "basic_triangle<3, float> is 64 bytes");
    aligned_vector<tri_t> prims(h.num_prims);
    if (fread(prims.data(), sizeof(tri_t), h.num_prims, in) != h.num_prims) return 3;
    const size_t nn = size_t(h.num_prims) * (h.per_vertex ? 3 : 1);
    std::vector<float> raw(nn * 4);
    if (fread(raw.data(), 16, nn, in) != nn) return 3;
    fclose(in);
    std::vector<vec3> normals(nn);
    for (size_t i = 0; i < nn; ++i) normals[i] = vec3(raw[4 * i], raw[4 * i + 1], raw[4 * i + 2]);
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 4;
    const int rc = h.per_vertex ? run<normals_per_vertex_binding>(h, materials, prims, normals, out)
                                : run<normals_per_face_binding>(h, materials, prims, normals, out);
    fclose(out);
    return rc;
}
