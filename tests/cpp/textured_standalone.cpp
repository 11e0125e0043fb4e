// tests/cpp/textured_standalone.cpp -- hip_shading::set_textures through the C++ header API, in two builds
// of one source (tests/test_cpp_textures.py compiles both, syntax only):
//   * against visionaray_hip/standalone.h: its minimal texture_ref<vector<4, unorm<8>>, 2> and enums;
//   * with -DVRH_TEST_REFERENCE_HEADERS against the reference's own headers: the reference's texture_ref
//     objects, as a model's textures are (src/common/model.h:29), go in unchanged.
// What stood as make_kernel_params(binding, prims, normals, tex_coords, materials, textures, lights, ...)
// + simple::kernel (kernels.h:396-437) is hip_shading + set_textures + make_hip_simple_kernel.
#ifdef VRH_TEST_REFERENCE_HEADERS
#include <visionaray/math/math.h>
#include <visionaray/bvh.h>
#include <visionaray/camera.h>
#include <visionaray/material.h>
#include <visionaray/pixel_format.h>
#include <visionaray/point_light.h>
#include <visionaray/scheduler.h>
#include <visionaray/tags.h>
#include <visionaray/texture/texture.h>

#include <visionaray_hip/hip_backend.h>
#else
#include <visionaray_hip/standalone.h>
#endif

#include <cstdio>
#include <vector>

using namespace visionaray;

int main()
{
    using tri = basic_triangle<3, float>;
    using texel = vector<4, unorm<8>>;
    const unsigned grid = 16, W = 60, H = 44;
    try
    {
        std::vector<tri> tris(size_t(2) * grid * grid);
        hip_detail::check(vrh_gen_heightfield(grid, tris.data()), "vrh_gen_heightfield");
        for (size_t i = 0; i < tris.size(); ++i) tris[i].geom_id = unsigned(i % 3);
        auto host_bvh = build<index_bvh<tri>>(tris.data(), tris.size());
        std::vector<vec4> normals(tris.size());
        hip_detail::check(vrh_face_normals(tris.data(), uint32_t(tris.size()), &normals[0].x), "vrh_face_normals");
        hip_index_bvh<tri> device_bvh(host_bvh, normals.data());

        std::vector<vrh_plastic> materials = {
            { { 0.2f, 0.2f, 0.2f }, 1.0f, { 0.8f, 0.3f, 0.2f }, 1.0f, { 1.0f, 1.0f, 1.0f }, 0.4f, 32.0f },
            { { 0.1f, 0.1f, 0.1f }, 0.5f, { 0.2f, 0.7f, 0.3f }, 0.9f, { 0.9f, 0.9f, 0.9f }, 0.2f, 8.0f },
            { { 0.05f, 0.05f, 0.1f }, 1.0f, { 0.3f, 0.3f, 0.9f }, 0.7f, { 1.0f, 0.8f, 0.6f }, 0.6f, 64.5f } };
        std::vector<vrh_point_light> lights = { { { 0.0f, 2.0f, 0.0f }, { 1.0f, 1.0f, 1.0f }, 1.0f, 1.0f, 0.0f, 0.0f } };
        hip_shading shading(materials, lights);

        // a 4 x 4 checker (Wrap / Linear, as the OBJ loader sets a model's textures), a 2 x 2 Mirror / Clamp
        // Nearest one, and the dummy; planar texture coordinates from the vertices' x and z
        std::vector<uint8_t> checker(4 * 4 * 4), small(2 * 2 * 4);
        for (size_t i = 0; i < 16; ++i)
            for (size_t c = 0; c < 4; ++c) checker[4 * i + c] = uint8_t(((i + i / 4) & 1) ? 255 : 40 + 60 * c);
        for (size_t i = 0; i < small.size(); ++i) small[i] = uint8_t(17 * i + 30);
        std::vector<texture_ref<texel, 2>> textures;
        texture_ref<texel, 2> t0(4, 4), t1(2, 2), t2(0, 0);
        t0.reset(reinterpret_cast<texel const*>(checker.data()));
        t0.set_address_mode(Wrap);
        t0.set_filter_mode(Linear);
        t1.reset(reinterpret_cast<texel const*>(small.data()));
        t1.set_address_mode(0, Mirror);
        t1.set_address_mode(1, Clamp);
        t1.set_filter_mode(Nearest);
        t2.set_address_mode(Wrap);
        t2.set_filter_mode(Nearest);
        textures.push_back(t0);
        textures.push_back(t1);
        textures.push_back(t2);
        std::vector<vec2> tex_coords;
        for (auto const& t : tris)
        {
            const vec3 v[3] = { t.v1, t.v1 + t.e1, t.v1 + t.e2 };
            for (auto const& p : v) tex_coords.push_back(vec2(p.x * 3.0f, p.z * 3.0f));
        }
        shading.set_textures(tex_coords, textures);

        hip_buffer_rt<PF_RGBA32F, PF_UNSPECIFIED> rt;
        rt.resize(W, H);
        camera cam;
        cam.perspective(45.0f * constants::degrees_to_radians<float>(), W / static_cast<float>(H), 0.001f, 1000.0f);
        cam.look_at(vec3(0.0f, 0.9f, 1.4f), vec3(0.0f, 0.0f, 0.0f), vec3(0.0f, 1.0f, 0.0f));
        hip_sched<ray> sched;
        sched.frame(make_hip_simple_kernel(normals_per_face_binding{}, device_bvh, shading, vec4(0.1f, 0.2f, 0.3f, 1.0f),
                                           vec4(1.0f, 1.0f, 1.0f, 0.3f)),
                    make_sched_params(pixel_sampler::uniform_type{}, cam, rt));
        std::vector<float> color(size_t(4) * W * H);
        rt.download(color.data());
        unsigned long long h = 1469598103934665603ull;
        const unsigned char* b = reinterpret_cast<const unsigned char*>(color.data());
        for (size_t i = 0; i < color.size() * 4; ++i) h = (h ^ b[i]) * 1099511628211ull;
        printf("{\"W\":%u,\"H\":%u,\"color_hash\":\"%016llx\"}\n", W, H, h);
    }
    catch (std::exception const& e)
    {
        fprintf(stderr, "textured_standalone: %s\n", e.what());
        return 1;
    }
    return 0;
}
