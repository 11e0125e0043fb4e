// tests/cpp/render_target_user.hip -- formatted render targets through the C++ header layer
// (tests/test_gpu_cpp_render_target.py): hip_buffer_rt<PF_RGBA8, PF_UNSPECIFIED> and <PF_RGBA32F, PF_DEPTH32F>
// through hip_sched::frame, each with a built-in kernel and with a hipcc user lambda.
//
//     render_target_user <out dir> <matrices.bin>
//
// matrices.bin: view and projection matrix (column-major, 32 floats) for the depth target's frames.  Every frame
// leaves <case>.staging (RGBA32F colour, then prim ids, then t) and <case>.formatted (the colour buffer, then the
// depth words if any) in the directory; the test holds them to vrh_rt_resolve_host.  The user lambda also renders
// three jittered_blend frames into the RGBA8 target (the formatted buffer accumulates) and, through camera matrices,
// into the depth target (its result's isect_pos becomes the depth).  Refused before any launch, and reported: a user
// kernel through hip_sched::frames() into a formatted target, and into a depth target through a pinhole camera.
// Prints one JSON line.
#include <visionaray_hip/hip_kernels.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace visionaray;

static const unsigned W = 61, H = 45;

static auto shade_kernel(hip_bvh_ref ref)
{
    return [=] __device__ (ray r) mutable -> result_record<float>
    {
        result_record<float> result;
        auto hr = closest_hit(r, &ref, &ref + 1);
        result.hit = hr.hit;
        // colours in and beyond [0, 1], alpha below 1: the unorm clamp and the RGB formats' alpha multiply see them
        result.color = hr.hit ? vec4(hr.t * 0.25f, hr.u * 1.5f - 0.25f, hr.v, 0.75f) : vec4(0.1f, 0.2f, 0.3f, 1.0f);
        result.isect_pos = r.ori + r.dir * hr.t;
        return result;
    };
}

template <typename RT>
static void dump(RT& rt, std::string const& dir, const char* name)
{
    const size_t n = size_t(W) * H;
    std::vector<float> color(4 * n), t(n);
    std::vector<uint32_t> pid(n);
    rt.download(color.data(), pid.data(), t.data());
    FILE* f = fopen((dir + "/" + name + ".staging").c_str(), "wb");
    if (!f) throw std::runtime_error("cannot write to " + dir);
    fwrite(color.data(), 16, n, f); fwrite(pid.data(), 4, n, f); fwrite(t.data(), 4, n, f);
    fclose(f);
    std::vector<unsigned char> fc(n * RT::color_bytes), fd(n * 4);
    rt.download_formatted(fc.data(), RT::depth_format != VRH_DF_NONE ? fd.data() : nullptr);
    f = fopen((dir + "/" + name + ".formatted").c_str(), "wb");
    fwrite(fc.data(), 1, fc.size(), f);
    if (RT::depth_format != VRH_DF_NONE) fwrite(fd.data(), 1, fd.size(), f);
    fclose(f);
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: render_target_user <out dir> <matrices.bin>\n"); return 2; }
    const std::string dir = argv[1];
    try
    {
        float mats[32];
        FILE* mf = fopen(argv[2], "rb");
        if (!mf || fread(mats, 4, 32, mf) != 32) throw std::runtime_error("cannot read the matrices");
        fclose(mf);

        using tri_t = basic_triangle<3, float>;
        std::vector<tri_t> prims;
        for (unsigned i = 0; i < 60; ++i)
        {
            const float a = float(i) * 0.7f, x = 0.9f * std::cos(a) * float(i % 7) / 7.0f, y = 0.9f * std::sin(a) * float(i % 5) / 5.0f;
            tri_t t(vec3(x, y, -0.5f + float(i % 11) * 0.1f), vec3(0.35f, 0.05f, 0.02f), vec3(-0.04f, 0.3f, 0.03f));
            t.prim_id = i; t.geom_id = 0;
            prims.push_back(t);
        }
        auto host = build<index_bvh<tri_t>>(prims.data(), prims.size());
        std::vector<vec4> normals(prims.size(), vec4(0.0f, 0.0f, 1.0f, 0.0f));
        hip_index_bvh<tri_t> dev(host, normals.data());
        camera cam;
        cam.perspective(45.0f * constants::degrees_to_radians<float>(), W / static_cast<float>(H), 0.001f, 1000.0f);
        cam.look_at(vec3(0.0f, 0.0f, 3.0f), vec3(0.0f, 0.0f, 0.0f), vec3(0.0f, 1.0f, 0.0f));
        hip_sched<ray> sched(hip_context::default_context(), false);

        hip_buffer_rt<PF_RGBA8, PF_UNSPECIFIED> rt8;
        rt8.resize(W, H);
        auto sp8 = make_sched_params(pixel_sampler::uniform_type{}, cam, rt8);
        sched.frame(make_hip_ao_kernel(dev, vec4(0.1f, 0.2f, 0.3f, 1.0f), 4, 0.5f), sp8, 2);
        dump(rt8, dir, "rgba8_builtin");
        sched.frame(shade_kernel(dev.ref()), sp8);
        dump(rt8, dir, "rgba8_user");
        sp8.scissor_box = recti(5, 3, 50, 40);
        rt8.clear_color_buffer(vec4(1.0f, 0.5f, 0.25f, 1.0f));
        sched.frame(shade_kernel(dev.ref()), sp8);
        dump(rt8, dir, "rgba8_user_box");

        hip_buffer_rt<PF_RGBA32F, PF_DEPTH32F> rtd;
        rtd.resize(W, H);
        rtd.clear_depth_buffer();
        auto spd = make_sched_params(pixel_sampler::uniform_type{}, mat4(mats), mat4(mats + 16), rtd);
        sched.frame(make_hip_closest_hit_kernel(dev, vec4(0.1f, 0.2f, 0.3f, 1.0f)), spd);
        dump(rtd, dir, "depth32f_builtin");
        auto r = rtd.ref();
        sched.frame(shade_kernel(dev.ref()), spd);
        dump(rtd, dir, "depth32f_user");
        auto spdb = make_sched_params(pixel_sampler::jittered_blend_type{}, mat4(mats), mat4(mats + 16), rtd);
        sched.frame(shade_kernel(dev.ref()), spdb, 2);
        dump(rtd, dir, "depth32f_user_blend2");

        // jittered_blend of a user kernel: the formatted buffer accumulates
        rt8.clear_color_buffer(vec4(0.0f, 0.0f, 0.0f, 0.0f));
        auto sp8b = make_sched_params(pixel_sampler::jittered_blend_type{}, cam, rt8);
        for (unsigned f = 1; f <= 3; ++f)
        {
            sched.frame(shade_kernel(dev.ref()), sp8b, f);
            dump(rt8, dir, f == 1 ? "rgba8_user_blend1" : f == 2 ? "rgba8_user_blend2" : "rgba8_user_blend3");
        }

        // refused before anything is launched: the targets stay as they are
        int pinhole_refused = 0, names_depth = 0, frames_refused = 0, names_batch = 0;
        auto spdp = make_sched_params(pixel_sampler::uniform_type{}, cam, rtd);
        try { sched.frame(shade_kernel(dev.ref()), spdp); }
        catch (std::runtime_error const& e) { pinhole_refused = 1; names_depth = std::string(e.what()).find("depth") != std::string::npos ? 1 : 0; }
        std::vector<camera> cams(1, cam);
        try { sched.frames(shade_kernel(dev.ref()), cams, rt8); }
        catch (std::runtime_error const& e) { frames_refused = 1; names_batch = std::string(e.what()).find("batch") != std::string::npos ? 1 : 0; }
        dump(rtd, dir, "depth32f_after_refusal");
        dump(rt8, dir, "rgba8_after_refusal");
        printf("{\"width\":%u,\"height\":%u,\"pinhole_depth_refused\":%d,\"names_depth\":%d,\"frames_refused\":%d,\"names_batch\":%d,"
               "\"has_depth_ptr\":%d,\"formatted_differs\":%d}\n", W, H, pinhole_refused, names_depth, frames_refused, names_batch,
               r.depth != nullptr ? 1 : 0, r.formatted_color != static_cast<void*>(r.color) ? 1 : 0);
    }
    catch (std::exception const& e)
    {
        fprintf(stderr, "render_target_user: %s\n", e.what());
        return 1;
    }
    return 0;
}
