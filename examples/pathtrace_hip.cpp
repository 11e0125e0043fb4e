// examples/pathtrace_hip.cpp -- progressive path tracing on the HIP backend through the C++ drop-in
// API, headless: the viewer's `pathtracing` algorithm (src/viewer/viewer.cpp) as
// make_hip_pathtracing_kernel + pixel_sampler::jittered_blend_type.  N frames with frame numbers
// 1 .. N are blended into one render target (frame n weighs 1 / n), and the image is written as a
// PFM file (RGB float, bottom row first -- the target's row order).
//
//     pathtrace_hip [grid] [width] [height] [frames] [bounces] [out.pfm]
#include <visionaray_hip/standalone.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace visionaray;

int main(int argc, char** argv)
{
    unsigned grid = argc > 1 ? unsigned(atoi(argv[1])) : 64;
    unsigned W = argc > 2 ? unsigned(atoi(argv[2])) : 320;
    unsigned H = argc > 3 ? unsigned(atoi(argv[3])) : 180;
    unsigned frames = argc > 4 ? unsigned(atoi(argv[4])) : 16;
    unsigned bounces = argc > 5 ? unsigned(atoi(argv[5])) : 10;
    const char* out = argc > 6 ? argv[6] : nullptr;
    try
    {
        using tri = basic_triangle<3, float>;
        std::vector<tri> tris(size_t(2) * grid * grid);
        hip_detail::check(vrh_gen_heightfield(grid, tris.data()), "vrh_gen_heightfield");
        for (size_t i = 0; i < tris.size(); ++i) tris[i].geom_id = unsigned(i % 3);   // material by geom_id
        auto host_bvh = build<index_bvh<tri>>(tris.data(), tris.size());
        std::vector<vec4> normals(tris.size());
        hip_detail::check(vrh_face_normals(tris.data(), uint32_t(tris.size()), &normals[0].x), "vrh_face_normals");
        hip_index_bvh<tri> device_bvh(host_bvh, normals.data());

        // plastic materials (ca ka cd kd cs ks exp); the path tracer ignores the lights
        std::vector<vrh_plastic> materials = {
            { { 0.0f, 0.0f, 0.0f }, 1.0f, { 0.8f, 0.3f, 0.2f }, 1.0f, { 1.0f, 1.0f, 1.0f }, 0.4f, 32.0f },
            { { 0.0f, 0.0f, 0.0f }, 1.0f, { 0.2f, 0.7f, 0.3f }, 0.9f, { 0.9f, 0.9f, 0.9f }, 0.2f, 8.0f },
            { { 0.0f, 0.0f, 0.0f }, 1.0f, { 0.3f, 0.3f, 0.9f }, 0.7f, { 1.0f, 0.8f, 0.6f }, 0.6f, 64.5f } };
        std::vector<vrh_point_light> lights = { { { 0.0f, 2.0f, 0.0f }, { 1.0f, 1.0f, 1.0f }, 1.0f, 1.0f, 0.0f, 0.0f } };
        hip_shading shading(materials, lights);

        hip_buffer_rt<PF_RGBA32F, PF_UNSPECIFIED> rt;
        rt.resize(W, H);
        rt.clear_color_buffer();

        camera cam;
        cam.perspective(45.0f * constants::degrees_to_radians<float>(), W / static_cast<float>(H), 0.001f, 1000.0f);
        cam.look_at(vec3(0.0f, 0.9f, 1.4f), vec3(0.0f, 0.0f, 0.0f), vec3(0.0f, 1.0f, 0.0f));

        hip_sched<ray> sched;
        auto kernel = make_hip_pathtracing_kernel(normals_per_face_binding{}, device_bvh, shading,
                                                  vec4(0.1f, 0.2f, 0.3f, 1.0f), vec4(1.0f, 1.0f, 1.0f, 1.0f), bounces, 1e-3f);
        auto sparams = make_sched_params(pixel_sampler::jittered_blend_type{}, cam, rt);
        unsigned long long rays = 0;
        for (unsigned n = 1; n <= frames; ++n)
        {
            sched.frame(kernel, sparams, n);          // frame n: its own random numbers, weight 1 / n
            sched.context().sync();
            rays += sched.context().last_frame_stats().rays;
        }

        size_t npx = size_t(W) * H;
        std::vector<float> color(4 * npx);
        rt.download(color.data());
        double mean[3] = { 0.0, 0.0, 0.0 };
        for (size_t p = 0; p < npx; ++p)
            for (int c = 0; c < 3; ++c) mean[c] += color[4 * p + c];
        if (out)
        {
            FILE* f = fopen(out, "wb");
            if (!f) throw std::runtime_error("cannot write the image");
            fprintf(f, "PF\n%u %u\n-1.0\n", W, H);
            for (size_t p = 0; p < npx; ++p) fwrite(&color[4 * p], 4, 3, f);
            fclose(f);
        }
        printf("{\"grid\":%u,\"W\":%u,\"H\":%u,\"frames\":%u,\"bounces\":%u,\"rays\":%llu,\"mean_rgb\":[%.6f,%.6f,%.6f]}\n",
               grid, W, H, frames, bounces, rays, mean[0] / npx, mean[1] / npx, mean[2] / npx);
    }
    catch (std::exception const& e)
    {
        fprintf(stderr, "pathtrace_hip: %s\n", e.what());
        return 1;
    }
    return 0;
}
