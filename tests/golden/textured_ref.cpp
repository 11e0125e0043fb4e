// tests/golden/textured_ref.cpp -- fixture generator for textures (vrh_shading_set_textures, vrh_tex2d_host).
//
// Runs the reference's own tex2D and its simple / whitted / pathtracing kernels with the textured parameter
// pack (make_kernel_params(binding, prims, normals, tex_coords, materials, textures, lights, ...),
// kernels.h:396-437) on the CPU, from the reference's headers (never copied into this repository), over a
// file written by make_textured_golden.py:
//
//     textured_ref <in.bin> <out.bin>
//
// in.bin starts with a u32 magic 0x54585246 and a u32 mode.
//
// mode 0, samples: u32 W, H, filter, address x, address y, n, guard; W * H RGBA8 texels; n coordinate pairs.
// out.bin: n x 4 floats, tex2D(tex, coord).  The texels are stored with guard texels of byte `guard`
// before and after the array (the reference reads texel N of an axis for a Wrap coordinate that maps to
// exactly 1.0): the script samples twice with two guard bytes, and a coordinate whose two results differ
// read outside the array.
//
// mode 1, frame: the `frame_header` below, then the materials (16 words each: kind, then the kind's
// parameters as include/vrh.h vrh_material lays them out), the lights (10 floats each: position, cl, kl,
// constant / linear / quadratic attenuation), the triangles (basic_triangle<3, float>, 64 B each), the
// normals as float4 rows (one per triangle, three with the per-vertex binding), the texture coordinates
// (three float pairs per triangle) and the textures (u32 W, H, filter, address x, address y, then W * H
// RGBA8 texels; W or H 0 is the dummy).  Texture storage is guarded as in mode 0 (frame_header.guard).
// out.bin: per snapshot W x H float4 colours (one snapshot, or with the accumulation mode the target after
// the first and after the last frame), then per pixel of the LAST frame the prim id (0xFFFFFFFF: miss) and
// t of the first closest_hit call, a u64 path signature and a u32 count of closest_hit calls, then the
// u64 total of those calls over all frames.
//
// Seeds, jitter, blending, path signature and the powf shift are those of tests/golden/pathtrace_ref.cpp.
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
#include <visionaray/texture/texture.h>
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
using texel_t = vector<4, unorm<8>>;
using tex_ref_t = texture_ref<texel_t, 2>;
using generic_t = generic_material<plastic<float>, matte<float>, mirror<float>, emissive<float>>;

static int g_pow_shift = 0;

extern "C" float powf(float x, float y)
{
    typedef float (*fn_t)(float, float);
    static fn_t real = (fn_t)dlsym(RTLD_NEXT, "powf");
    float r = real(x, y);
    if (g_pow_shift == 0 || y == 0.0f || x == 1.0f || r == 0.0f || !std::isfinite(r)) return r;
    return nextafterf(r, g_pow_shift > 0 ? INFINITY : -INFINITY);
}

struct frame_header
{
    uint32_t W, H, num_prims, per_vertex, num_materials, generic;
    uint32_t algo;           // 0 simple::kernel, 1 whitted::kernel, 2 pathtracing::kernel
    uint32_t num_bounces;
    uint32_t first_frame;    // frame number (accumulation: of the first frame, >= 1)
    uint32_t accum;          // 0: one uniform-sampler frame; n: n jittered_blend frames
    int32_t pow_shift;
    uint32_t num_lights, num_textures, guard;
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

// a texture's texels between two runs of guard texels
struct guarded_texture
{
    std::vector<uint8_t> store;
    uint32_t w = 0, h = 0, filter = 0, ax = 0, ay = 0;
    size_t guard_texels = 0;

    bool read(FILE* in, uint32_t guard)
    {
        uint32_t d[5];
        if (fread(d, 4, 5, in) != 5) return false;
        w = d[0]; h = d[1]; filter = d[2]; ax = d[3]; ay = d[4];
        guard_texels = 2 * size_t(w) + 8;
        store.assign((2 * guard_texels + size_t(w) * h) * 4, uint8_t(guard));
        return size_t(w) * h == 0 || fread(store.data() + guard_texels * 4, 4, size_t(w) * h, in) == size_t(w) * h;
    }

    tex_ref_t ref() const
    {
        tex_ref_t t(w, h);
        t.reset(reinterpret_cast<texel_t const*>(store.data() + guard_texels * 4));
        t.set_filter_mode(filter == 0 ? Nearest : Linear);
        t.set_address_mode(0, tex_address_mode(ax));
        t.set_address_mode(1, tex_address_mode(ay));
        return t;
    }
};

static int run_samples(FILE* in, FILE* out)
{
    guarded_texture g;
    uint32_t d[7];
    if (fread(d, 4, 7, in) != 7) return 3;
    const uint32_t n = d[5], guard = d[6];
    g.w = d[0]; g.h = d[1]; g.filter = d[2]; g.ax = d[3]; g.ay = d[4];
    g.guard_texels = 2 * size_t(g.w) + 8;
    g.store.assign((2 * g.guard_texels + size_t(g.w) * g.h) * 4, uint8_t(guard));
    if (fread(g.store.data() + g.guard_texels * 4, 4, size_t(g.w) * g.h, in) != size_t(g.w) * g.h) return 3;
    std::vector<float> coords(size_t(n) * 2), res(size_t(n) * 4);
    if (fread(coords.data(), 8, n, in) != n) return 3;
    tex_ref_t t = g.ref();
    for (uint32_t i = 0; i < n; ++i)
    {
        vector<4, float> c = tex2D(t, vector<2, float>(coords[2 * i], coords[2 * i + 1]));
        res[4 * i] = c.x; res[4 * i + 1] = c.y; res[4 * i + 2] = c.z; res[4 * i + 3] = c.w;
    }
    return fwrite(res.data(), 16, n, out) == n ? 0 : 4;
}

// counts the closest_hit calls of a pixel, hashes their results and keeps the first one
struct path_intersector : basic_intersector<path_intersector>
{
    using basic_intersector<path_intersector>::operator();

    uint32_t calls = 0;
    uint64_t sig = 0xcbf29ce484222325ull;
    uint32_t first_prim = 0xFFFFFFFFu;
    float first_t = -1.0f;

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

template <template <typename> class Kernel, bool Sampled>
struct call_kernel;
template <template <typename> class Kernel>
struct call_kernel<Kernel, false>
{
    template <typename K>
    static result_record<float> go(K const& k, path_intersector& isect, ray const& r, random_sampler<float>&) { return k(isect, r); }
};
template <template <typename> class Kernel>
struct call_kernel<Kernel, true>
{
    template <typename K>
    static result_record<float> go(K const& k, path_intersector& isect, ray const& r, random_sampler<float>& s) { return k(isect, r, s); }
};

template <template <typename> class Kernel, bool Sampled, typename Binding, typename Material>
static int run(frame_header const& h, std::vector<Material> const& materials, std::vector<point_light<float>> const& lights,
               aligned_vector<tri_t>& prims, std::vector<vec3> const& normals, std::vector<vec2> const& tex_coords,
               std::vector<tex_ref_t> const& textures, FILE* out)
{
    auto bvh = build<index_bvh<tri_t>>(prims.data(), prims.size());
    using bvh_ref = index_bvh<tri_t>::bvh_ref;
    std::vector<bvh_ref> bvhs{ bvh.ref() };
    vec4 bg(h.bg[0], h.bg[1], h.bg[2], h.bg[3]), ambient(h.ambient[0], h.ambient[1], h.ambient[2], h.ambient[3]);
    auto kp = make_kernel_params(Binding{}, bvhs.data(), bvhs.data() + bvhs.size(), normals.data(), tex_coords.data(),
                                 materials.data(), textures.data(), lights.data(), lights.data() + lights.size(),
                                 h.num_bounces, h.eps, bg, ambient);
    Kernel<decltype(kp)> kern;
    kern.params = kp;

    const vec3 eye(h.eye[0], h.eye[1], h.eye[2]), cam_u(h.cam_u[0], h.cam_u[1], h.cam_u[2]);
    const vec3 cam_v(h.cam_v[0], h.cam_v[1], h.cam_v[2]), cam_w(h.cam_w[0], h.cam_w[1], h.cam_w[2]);
    const size_t npx = size_t(h.W) * h.H;
    std::vector<float> target(npx * 4, 0.0f), first_t(npx);
    std::vector<uint64_t> sig(npx);
    std::vector<uint32_t> nrays(npx), first_prim(npx);
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
                const float u = 2.0f * (fx + 0.5f) / float(h.W) - 1.0f;
                const float v = 2.0f * (fy + 0.5f) / float(h.H) - 1.0f;
                ray r;
                r.ori = eye;
                r.dir = normalize(cam_u * u + cam_v * v + cam_w);
                random_sampler<float> samp(rs_hash(n * h.W * h.H + y * h.W + x));
                path_intersector isect;
                result_record<float> res = call_kernel<Kernel, Sampled>::go(kern, isect, r, samp);
                const size_t p = size_t(y) * h.W + x;
                isect.u32(isect.calls);
                sig[p] = isect.sig;
                nrays[p] = isect.calls;
                first_prim[p] = isect.first_prim;
                first_t[p] = isect.first_t;
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
    if (fwrite(first_prim.data(), 4, npx, out) != npx || fwrite(first_t.data(), 4, npx, out) != npx
        || fwrite(sig.data(), 8, npx, out) != npx || fwrite(nrays.data(), 4, npx, out) != npx || fwrite(&total, 8, 1, out) != 1)
        return 4;
    return 0;
}

static plastic<float> make_plastic(const float* m)
{
    plastic<float> p;
    p.set_ca(from_rgb(vec3(m[0], m[1], m[2])));
    p.set_ka(m[3]);
    p.set_cd(from_rgb(vec3(m[4], m[5], m[6])));
    p.set_kd(m[7]);
    p.set_cs(from_rgb(vec3(m[8], m[9], m[10])));
    p.set_ks(m[11]);
    p.set_specular_exp(m[12]);
    return p;
}

template <typename Binding>
static int dispatch(frame_header const& h, std::vector<uint32_t> const& mats, std::vector<point_light<float>> const& lights,
                    aligned_vector<tri_t>& prims, std::vector<vec3> const& normals, std::vector<vec2> const& tc,
                    std::vector<tex_ref_t> const& textures, FILE* out)
{
    if (h.generic)
    {
        if (h.algo != 2) return 5;
        std::vector<generic_t> materials;
        for (uint32_t i = 0; i < h.num_materials; ++i)
        {
            const uint32_t kind = mats[16 * i];
            const float* m = reinterpret_cast<const float*>(&mats[16 * i + 1]);
            if (kind == 0)
                materials.push_back(generic_t(make_plastic(m)));
            else if (kind == 1)
            {
                matte<float> p;
                p.set_ca(from_rgb(vec3(m[0], m[1], m[2])));
                p.set_ka(m[3]);
                p.set_cd(from_rgb(vec3(m[4], m[5], m[6])));
                p.set_kd(m[7]);
                materials.push_back(generic_t(p));
            }
            else if (kind == 2)
            {
                mirror<float> p;
                p.set_cr(from_rgb(vec3(m[0], m[1], m[2])));
                p.set_kr(m[3]);
                p.set_ior(spectrum<float>(from_rgb(vec3(m[4], m[5], m[6]))));
                p.set_absorption(spectrum<float>(from_rgb(vec3(m[7], m[8], m[9]))));
                materials.push_back(generic_t(p));
            }
            else if (kind == 3)
            {
                emissive<float> p;
                p.set_ce(from_rgb(vec3(m[0], m[1], m[2])));
                p.set_ls(m[3]);
                materials.push_back(generic_t(p));
            }
            else
                return 5;
        }
        return run<pathtracing::kernel, true, Binding>(h, materials, lights, prims, normals, tc, textures, out);
    }
    std::vector<plastic<float>> materials;
    for (uint32_t i = 0; i < h.num_materials; ++i)
    {
        if (mats[16 * i] != 0) return 5;
        materials.push_back(make_plastic(reinterpret_cast<const float*>(&mats[16 * i + 1])));
    }
    if (h.algo == 0) return run<simple::kernel, false, Binding>(h, materials, lights, prims, normals, tc, textures, out);
    if (h.algo == 1) return run<whitted::kernel, false, Binding>(h, materials, lights, prims, normals, tc, textures, out);
    if (h.algo == 2) return run<pathtracing::kernel, true, Binding>(h, materials, lights, prims, normals, tc, textures, out);
    return 5;
}

static int run_frame(FILE* in, FILE* out)
{
    frame_header h;
    if (fread(&h, sizeof(h), 1, in) != 1) return 3;
    g_pow_shift = h.pow_shift;
    std::vector<uint32_t> mats(size_t(h.num_materials) * 16);
    if (fread(mats.data(), 64, h.num_materials, in) != h.num_materials) return 3;
    std::vector<point_light<float>> lights;
    for (uint32_t i = 0; i < h.num_lights; ++i)
    {
        float l[10];
        if (fread(l, 4, 10, in) != 10) return 3;
        point_light<float> p;
        p.set_position(vec3(l[0], l[1], l[2]));
        p.set_cl(vec3(l[3], l[4], l[5]));
        p.set_kl(l[6]);
        p.set_constant_attenuation(l[7]);
        p.set_linear_attenuation(l[8]);
        p.set_quadratic_attenuation(l[9]);
        lights.push_back(p);
    }
    static_assert(sizeof(tri_t) == 64, "basic_triangle<3, float> is 64 bytes");
    aligned_vector<tri_t> prims(h.num_prims);
    if (fread(prims.data(), sizeof(tri_t), h.num_prims, in) != h.num_prims) return 3;
    const size_t nn = size_t(h.num_prims) * (h.per_vertex ? 3 : 1);
    std::vector<float> raw(nn * 4);
    if (fread(raw.data(), 16, nn, in) != nn) return 3;
    std::vector<vec3> normals(nn);
    for (size_t i = 0; i < nn; ++i) normals[i] = vec3(raw[4 * i], raw[4 * i + 1], raw[4 * i + 2]);
    std::vector<float> rawtc(size_t(h.num_prims) * 6);
    if (fread(rawtc.data(), 24, h.num_prims, in) != h.num_prims) return 3;
    std::vector<vec2> tc(size_t(h.num_prims) * 3);
    for (size_t i = 0; i < tc.size(); ++i) tc[i] = vec2(rawtc[2 * i], rawtc[2 * i + 1]);
    std::vector<guarded_texture> store(h.num_textures);
    std::vector<tex_ref_t> textures;
    for (uint32_t i = 0; i < h.num_textures; ++i)
    {
        if (!store[i].read(in, h.guard)) return 3;
        textures.push_back(store[i].ref());
    }
    return h.per_vertex ? dispatch<normals_per_vertex_binding>(h, mats, lights, prims, normals, tc, textures, out)
                        : dispatch<normals_per_face_binding>(h, mats, lights, prims, normals, tc, textures, out);
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s <in.bin> <out.bin>\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    uint32_t head[2];
    if (!in || fread(head, 4, 2, in) != 2 || head[0] != 0x54585246u) { fprintf(stderr, "bad input file\n"); return 3; }
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 4;
    const int rc = head[1] == 0 ? run_samples(in, out) : run_frame(in, out);
    fclose(in);
    fclose(out);
    return rc;
}
