// tests/golden/render_target_ref.cpp -- fixture generator for formatted render targets (vrh_rt_alloc_formatted,
// visionaray_hip/detail/vrh_pixel.h).
//
// Our own program over the reference's headers (never copied into this repository): it runs the reference's
// detail::pixel_access::store / blend, detail::depth_transform, simple_buffer_rt<CF, DF>::clear_* and
// simple_sched<basic_ray<float>> with make_sched_params(uniform_type, view, proj, rt) on inputs written by
// make_render_target_golden.py, for PF_RGBA32F / PF_RGB32F / PF_RGBA8 / PF_RGB8 colour with PF_UNSPECIFIED /
// PF_DEPTH32F / PF_DEPTH24_STENCIL8 depth:
//
//     render_target_ref pixels <in.bin> <out.bin>
//     render_target_ref frame  <in.bin> <out.bin>
//
// pixels: in.bin = pixels_header, then per step { u32 blend, u32 frame_num, N float4 colours, N u32 hit flags,
// N float3 positions }.  A target of N x 1 pixels is cleared (colour and depth), then every step's records are
// stored (blend 0) or blended with 1 / frame_num, 1 - 1 / frame_num (blend 1) exactly as sample_pixel_impl
// does it: depth = hit ? depth_transform(isect_pos, view, ., proj, .) : 1, with identity matrices.  out.bin: for
// every colour format (in the order above) and every depth format, after the clears and after every step: the
// colour buffer's bytes, then the depth buffer's (none for PF_UNSPECIFIED).
// frame: in.bin = frame_header, then the triangles (basic_triangle<3, float>, 64 B each).  One frame of
// simple_sched over build<index_bvh>(triangles), kernel: colour = a function of prim_id, hit, isect_pos = ori +
// dir * t; into <PF_RGBA8, PF_DEPTH24_STENCIL8> and <PF_RGB8, PF_DEPTH32F>.  out.bin: each target's colour then
// depth bytes, then per pixel the prim id (0xFFFFFFFF: miss) and t (-1: miss) the kernel saw.
#include <visionaray/math/math.h>
#include <visionaray/bvh.h>
#include <visionaray/pixel_format.h>
#include <visionaray/pixel_traits.h>
#include <visionaray/render_target.h>
#include <visionaray/result_record.h>
#include <visionaray/scheduler.h>
#include <visionaray/simple_buffer_rt.h>
#include <visionaray/traverse.h>
#include <visionaray/detail/pixel_access.h>
#include <visionaray/detail/sched_common.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace visionaray;

struct pixels_header
{
    uint32_t magic;          // 0x58505452
    uint32_t N, steps;
    float clear_color[4];
    float clear_depth;
};

struct frame_header
{
    uint32_t magic;          // 0x52465452
    uint32_t W, H, num_prims;
    float view[16], proj[16];   // column-major
};

static std::vector<char> read_file(const char* path)
{
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", path); exit(1); }
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<char> buf(n);
    if (fread(buf.data(), 1, n, f) != size_t(n)) exit(1);
    fclose(f);
    return buf;
}

template <typename T>
static void put(FILE* f, const T* p, size_t n) { fwrite(p, sizeof(T), n, f); }

struct step_t
{
    uint32_t blend, frame_num;
    const float* color;
    const uint32_t* hit;
    const float* pos;
};

template <pixel_format CF>
static void dump(simple_buffer_rt<CF, PF_UNSPECIFIED>& rt, size_t n, FILE* out)
{
    put(out, rt.color(), n);
}

template <pixel_format CF, pixel_format DF>
static void dump(simple_buffer_rt<CF, DF>& rt, size_t n, FILE* out)
{
    put(out, rt.color(), n);
    put(out, rt.depth(), n);
}

template <pixel_format CF>
static void clear_depth(simple_buffer_rt<CF, PF_UNSPECIFIED>&, float) {}

template <pixel_format CF, pixel_format DF>
static void clear_depth(simple_buffer_rt<CF, DF>& rt, float d) { rt.clear_depth_buffer(d); }

// colour only: the render_target_ref<CF> overloads of sample_pixel_impl (sched_common.h:361-397, 480-520)
template <pixel_format CF>
static void apply(simple_buffer_rt<CF, PF_UNSPECIFIED>& rt, const step_t& s, int x, int n, result_record<float>& rr)
{
    if (s.blend)
    {
        float alpha = 1.0f / float(s.frame_num);
        detail::pixel_access::blend(pixel_format_constant<CF>{}, pixel_format_constant<PF_RGBA32F>{}, x, 0, n, 1, rr, rt.color(),
                                    alpha, 1.0f - alpha);
    }
    else
        detail::pixel_access::store(pixel_format_constant<CF>{}, pixel_format_constant<PF_RGBA32F>{}, x, 0, n, 1, rr, rt.color());
}

// colour and depth: the render_target_ref<CF, DF> overloads (sched_common.h:399-439, 522-575)
template <pixel_format CF, pixel_format DF>
static void apply(simple_buffer_rt<CF, DF>& rt, const step_t& s, int x, int n, result_record<float>& rr)
{
    mat4 id = mat4::identity();
    rr.depth = select(rr.hit, detail::depth_transform(rr.isect_pos, id, id, id, id), 1.0f);
    if (s.blend)
    {
        float alpha = 1.0f / float(s.frame_num);
        detail::pixel_access::blend(pixel_format_constant<CF>{}, pixel_format_constant<PF_RGBA32F>{}, pixel_format_constant<DF>{},
                                    pixel_format_constant<PF_DEPTH32F>{}, x, 0, n, 1, rr, rt.color(), rt.depth(), alpha, 1.0f - alpha);
    }
    else
        detail::pixel_access::store(pixel_format_constant<CF>{}, pixel_format_constant<PF_RGBA32F>{}, pixel_format_constant<DF>{},
                                    pixel_format_constant<PF_DEPTH32F>{}, x, 0, n, 1, rr, rt.color(), rt.depth());
}

template <pixel_format CF, pixel_format DF>
static void run_pixels(const pixels_header& h, const std::vector<step_t>& steps, FILE* out)
{
    simple_buffer_rt<CF, DF> rt;
    rt.resize(h.N, 1);
    rt.clear_color_buffer(vec4(h.clear_color[0], h.clear_color[1], h.clear_color[2], h.clear_color[3]));
    clear_depth(rt, h.clear_depth);
    dump(rt, h.N, out);
    for (const step_t& s : steps)
    {
        for (uint32_t i = 0; i < h.N; ++i)
        {
            result_record<float> rr;
            rr.hit = s.hit[i] != 0;
            rr.color = vec4(s.color[4 * i], s.color[4 * i + 1], s.color[4 * i + 2], s.color[4 * i + 3]);
            rr.isect_pos = vec3(s.pos[3 * i], s.pos[3 * i + 1], s.pos[3 * i + 2]);
            apply(rt, s, int(i), int(h.N), rr);
        }
        dump(rt, h.N, out);
    }
}

template <pixel_format CF>
static void run_pixels_cf(const pixels_header& h, const std::vector<step_t>& steps, FILE* out)
{
    run_pixels<CF, PF_UNSPECIFIED>(h, steps, out);
    run_pixels<CF, PF_DEPTH32F>(h, steps, out);
    run_pixels<CF, PF_DEPTH24_STENCIL8>(h, steps, out);
}

static int pixels_main(const char* in, const char* outp)
{
    std::vector<char> buf = read_file(in);
    pixels_header h;
    memcpy(&h, buf.data(), sizeof(h));
    if (h.magic != 0x58505452u) { fprintf(stderr, "bad magic\n"); return 1; }
    const size_t per = 8 + size_t(h.N) * (16 + 4 + 12);
    if (buf.size() != sizeof(h) + per * h.steps) { fprintf(stderr, "bad size\n"); return 1; }
    std::vector<step_t> steps;
    for (uint32_t k = 0; k < h.steps; ++k)
    {
        const char* p = buf.data() + sizeof(h) + per * k;
        step_t s;
        memcpy(&s.blend, p, 4);
        memcpy(&s.frame_num, p + 4, 4);
        s.color = reinterpret_cast<const float*>(p + 8);
        s.hit = reinterpret_cast<const uint32_t*>(p + 8 + size_t(h.N) * 16);
        s.pos = reinterpret_cast<const float*>(p + 8 + size_t(h.N) * 20);
        steps.push_back(s);
    }
    FILE* out = fopen(outp, "wb");
    if (!out) return 1;
    run_pixels_cf<PF_RGBA32F>(h, steps, out);
    run_pixels_cf<PF_RGB32F>(h, steps, out);
    run_pixels_cf<PF_RGBA8>(h, steps, out);
    run_pixels_cf<PF_RGB8>(h, steps, out);
    fclose(out);
    return 0;
}

using tri_t = basic_triangle<3, float>;

// colour of a primitive: four channels in and beyond [0, 1], a function of the prim id alone
static vec4 prim_color(unsigned id)
{
    auto ch = [](unsigned v) { return float(v % 37u) / 32.0f - 0.0625f; };
    return vec4(ch(id * 7u + 1u), ch(id * 11u + 5u), ch(id * 13u + 9u), float(id % 5u + 1u) / 4.0f);
}

template <pixel_format CF, pixel_format DF, typename BVH>
static void run_frame(const frame_header& h, BVH& bvh, std::vector<uint32_t>& pid, std::vector<float>& tt, FILE* out)
{
    simple_buffer_rt<CF, DF> rt;
    rt.resize(h.W, h.H);
    rt.clear_color_buffer(vec4(0.0f));
    rt.clear_depth_buffer(1.0f);
    mat4 view(h.view), proj(h.proj);
    auto sparams = make_sched_params(pixel_sampler::uniform_type{}, view, proj, rt);
    simple_sched<basic_ray<float>> sched;
    auto ref = bvh.ref();
    sched.frame([&](basic_ray<float> r, int x, int y) -> result_record<float>
    {
        result_record<float> rr;
        auto hr = closest_hit(r, &ref, &ref + 1);
        rr.hit = hr.hit;
        rr.color = hr.hit ? prim_color(hr.prim_id) : vec4(0.1f, 0.2f, 0.3f, 1.0f);
        rr.isect_pos = r.ori + r.dir * hr.t;
        pid[size_t(y) * h.W + x] = hr.hit ? unsigned(hr.prim_id) : 0xFFFFFFFFu;
        tt[size_t(y) * h.W + x] = hr.hit ? hr.t : -1.0f;
        return rr;
    }, sparams);
    dump(rt, size_t(h.W) * h.H, out);
}

static int frame_main(const char* in, const char* outp)
{
    std::vector<char> buf = read_file(in);
    frame_header h;
    memcpy(&h, buf.data(), sizeof(h));
    if (h.magic != 0x52465452u) { fprintf(stderr, "bad magic\n"); return 1; }
    if (buf.size() != sizeof(h) + size_t(h.num_prims) * sizeof(tri_t)) { fprintf(stderr, "bad size\n"); return 1; }
    std::vector<tri_t> prims(h.num_prims);
    memcpy(prims.data(), buf.data() + sizeof(h), size_t(h.num_prims) * sizeof(tri_t));
    auto bvh = build<index_bvh<tri_t>>(prims.data(), prims.size());
    const size_t n = size_t(h.W) * h.H;
    std::vector<uint32_t> pid(n), pid2(n);
    std::vector<float> tt(n), tt2(n);
    FILE* out = fopen(outp, "wb");
    if (!out) return 1;
    run_frame<PF_RGBA8, PF_DEPTH24_STENCIL8>(h, bvh, pid, tt, out);
    run_frame<PF_RGB8, PF_DEPTH32F>(h, bvh, pid2, tt2, out);
    if (pid != pid2 || memcmp(tt.data(), tt2.data(), n * 4) != 0) { fprintf(stderr, "the two frames differ\n"); return 1; }
    put(out, pid.data(), n);
    put(out, tt.data(), n);
    fclose(out);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc == 4 && !strcmp(argv[1], "pixels")) return pixels_main(argv[2], argv[3]);
    if (argc == 4 && !strcmp(argv[1], "frame")) return frame_main(argv[2], argv[3]);
    fprintf(stderr, "usage: render_target_ref pixels|frame <in.bin> <out.bin>\n");
    return 2;
}
