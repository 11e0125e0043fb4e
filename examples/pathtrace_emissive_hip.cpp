// examples/pathtrace_emissive_hip.cpp -- a closed box lit by an emissive ceiling quad, path traced on the
// HIP backend through the C++ drop-in API, headless.  The materials are tagged records (vrh_material:
// matte walls, one mirror wall, the emissive quad) in a hip_shading, which make_hip_pathtracing_kernel
// takes unchanged; the environment is black (ambient = 0), so every bit of light comes from the quad.
// N frames with frame numbers 1 .. N are blended into one render target (pixel_sampler::jittered_blend_type,
// frame n weighs 1 / n), and the image is written as a PFM file (RGB float, bottom row first).
//
//     pathtrace_emissive_hip [width] [height] [frames] [bounces] [out.pfm]
#include <visionaray_hip/standalone.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace visionaray;

using tri = basic_triangle<3, float>;

// the quad a b c d as the triangles (a, b, c) and (a, c, d)
static void quad(std::vector<tri>& tris, vec3 a, vec3 b, vec3 c, vec3 d, unsigned geom_id)
{
    for (int k = 0; k < 2; ++k)
    {
        tri t;
        t.v1 = a;
        t.e1 = (k == 0 ? b : c) - a;
        t.e2 = (k == 0 ? c : d) - a;
        t.prim_id = unsigned(tris.size());
        t.geom_id = geom_id;
        tris.push_back(t);
    }
}

int main(int argc, char** argv)
{
    unsigned W = argc > 1 ? unsigned(atoi(argv[1])) : 320;
    unsigned H = argc > 2 ? unsigned(atoi(argv[2])) : 240;
    unsigned frames = argc > 3 ? unsigned(atoi(argv[3])) : 64;
    unsigned bounces = argc > 4 ? unsigned(atoi(argv[4])) : 5;
    const char* out = argc > 5 ? argv[5] : nullptr;
    try
    {
        // the box [-1, 1]^3: geom 0 matte white, 1 matte red, 2 mirror, 3 emissive
        std::vector<tri> tris;
        quad(tris, vec3(-1, -1, -1), vec3(1, -1, -1), vec3(1, -1, 1), vec3(-1, -1, 1), 0);     // floor
        quad(tris, vec3(-1, 1, -1), vec3(-1, 1, 1), vec3(1, 1, 1), vec3(1, 1, -1), 0);         // ceiling
        quad(tris, vec3(-1, -1, -1), vec3(-1, 1, -1), vec3(1, 1, -1), vec3(1, -1, -1), 0);     // back
        quad(tris, vec3(-1, -1, 1), vec3(1, -1, 1), vec3(1, 1, 1), vec3(-1, 1, 1), 0);         // front
        quad(tris, vec3(-1, -1, -1), vec3(-1, -1, 1), vec3(-1, 1, 1), vec3(-1, 1, -1), 1);     // left
        quad(tris, vec3(1, -1, -1), vec3(1, 1, -1), vec3(1, 1, 1), vec3(1, -1, 1), 2);         // right
        quad(tris, vec3(-0.8f, 0.99f, -0.8f), vec3(-0.8f, 0.99f, 0.8f), vec3(0.8f, 0.99f, 0.8f), vec3(0.8f, 0.99f, -0.8f), 3);   // light
        auto host_bvh = build<index_bvh<tri>>(tris.data(), tris.size());
        std::vector<vec4> normals(tris.size());
        hip_detail::check(vrh_face_normals(tris.data(), uint32_t(tris.size()), &normals[0].x), "vrh_face_normals");
        hip_index_bvh<tri> device_bvh(host_bvh, normals.data());

        std::vector<vrh_material> materials(4);
        materials[0].kind = VRH_MATERIAL_MATTE;
        materials[0].u.matte = { { 0.0f, 0.0f, 0.0f }, 1.0f, { 0.8f, 0.8f, 0.8f }, 1.0f };
        materials[1].kind = VRH_MATERIAL_MATTE;
        materials[1].u.matte = { { 0.0f, 0.0f, 0.0f }, 1.0f, { 0.8f, 0.2f, 0.2f }, 1.0f };
        materials[2].kind = VRH_MATERIAL_MIRROR;
        materials[2].u.mirror = { { 1.0f, 1.0f, 1.0f }, 0.9f, { 0.2f, 0.9f, 1.1f }, { 3.9f, 2.4f, 2.2f } };
        materials[3].kind = VRH_MATERIAL_EMISSIVE;
        materials[3].u.emissive = { { 1.0f, 0.9f, 0.8f }, 8.0f };
        std::vector<vrh_point_light> lights;                       // the path tracer ignores point lights
        hip_shading shading(materials, lights);

        hip_buffer_rt<PF_RGBA32F, PF_UNSPECIFIED> rt;
        rt.resize(W, H);
        rt.clear_color_buffer();

        camera cam;
        cam.perspective(60.0f * constants::degrees_to_radians<float>(), W / static_cast<float>(H), 0.001f, 1000.0f);
        cam.look_at(vec3(0.0f, 0.0f, 0.9f), vec3(0.0f, -0.1f, -1.0f), vec3(0.0f, 1.0f, 0.0f));

        hip_sched<ray> sched;
        auto kernel = make_hip_pathtracing_kernel(normals_per_face_binding{}, device_bvh, shading,
                                                  vec4(0.1f, 0.2f, 0.3f, 1.0f), vec4(0.0f, 0.0f, 0.0f, 0.0f), bounces, 1e-3f);
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
        size_t lit = 0;
        for (size_t p = 0; p < npx; ++p)
        {
            for (int c = 0; c < 3; ++c) mean[c] += color[4 * p + c];
            lit += (color[4 * p] != 0.0f || color[4 * p + 1] != 0.0f || color[4 * p + 2] != 0.0f) ? 1 : 0;
        }
        if (out)
        {
            FILE* f = fopen(out, "wb");
            if (!f) throw std::runtime_error("cannot write the image");
            fprintf(f, "PF\n%u %u\n-1.0\n", W, H);
            for (size_t p = 0; p < npx; ++p) fwrite(&color[4 * p], 4, 3, f);
            fclose(f);
        }
        printf("{\"W\":%u,\"H\":%u,\"frames\":%u,\"bounces\":%u,\"rays\":%llu,\"lit_pixels\":%zu,\"mean_rgb\":[%.6f,%.6f,%.6f]}\n",
               W, H, frames, bounces, rays, lit, mean[0] / npx, mean[1] / npx, mean[2] / npx);
    }
    catch (std::exception const& e)
    {
        fprintf(stderr, "pathtrace_emissive_hip: %s\n", e.what());
        return 1;
    }
    return 0;
}
