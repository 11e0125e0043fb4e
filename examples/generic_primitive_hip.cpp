// examples/generic_primitive_hip.cpp -- the reference's generic_primitive example (src/examples/generic_primitive:
// two pyramids of six triangles and two spheres in ONE primitive list and one BVH, four plastics, one point light,
// whitted::kernel with 4 bounces and epsilon 1e-4) on the HIP backend, headless.  Two builds of one source:
//   * against visionaray_hip/standalone.h (no Visionaray headers needed): the Makefile's `examples` target;
//   * with -DVRH_TEST_REFERENCE_HEADERS against the reference's own headers: its generic_primitive, index_bvh,
//     plastic and point_light objects go in unchanged (tests/test_cpp_api.py-style drop-in compile).
// What stood as
//     make_kernel_params(normals_per_face_binding{}, primitives.data(), primitives.data() + N, normals.data(), ...)
//     whitted::kernel<decltype(kparams)> kernel;  host_sched.frame(kernel, sparams);
// is build<index_bvh<primitive_type>> + hip_index_bvh + hip_shading + make_hip_whitted_kernel + hip_sched::frame
// (the primitives go into a BVH here; the example hands the bare list to the kernel).
//
//     generic_primitive_hip [camera.bin]
// camera.bin (optional, 8 floats): the moving sphere's y, eye xyz, center xyz, fovy.  Default: y after 40 of the
// example's animation steps, the example's own camera (view_all of its box at 45 degrees).  Renders 60 x 44
// primary visibility, AO (8 samples, radius 0.5), simple and whitted frames and prints one JSON line of FNV-1a
// hashes of their buffers (tests/test_gpu_cpp_generic.py compares them with tests/golden/gp_example.npz).
#ifdef VRH_TEST_REFERENCE_HEADERS
#include <visionaray/math/math.h>
#include <visionaray/bvh.h>
#include <visionaray/camera.h>
#include <visionaray/generic_primitive.h>
#include <visionaray/material.h>
#include <visionaray/pixel_format.h>
#include <visionaray/point_light.h>
#include <visionaray/scheduler.h>
#include <visionaray/tags.h>

#include <visionaray_hip/hip_backend.h>
#else
#include <visionaray_hip/standalone.h>
#endif

#include <cmath>
#include <cstdio>
#include <string>
#include <vector>

using namespace visionaray;

static std::string fnv(const void* p, size_t n)
{
    unsigned long long h = 1469598103934665603ull;
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    char buf[20];
    snprintf(buf, sizeof(buf), "%016llx", h);
    return buf;
}

int main(int argc, char** argv)
{
    using triangle_type = basic_triangle<3, float>;
    using sphere_type = basic_sphere<float>;
    using primitive_type = generic_primitive<triangle_type, sphere_type>;
    const unsigned W = 60, H = 44, N = 14;
    try
    {
        // the moving sphere after 40 animation steps (y = -0.5, y += 0.2f * 0.1f per frame), the example's camera
        float y = -0.5f;
        for (int i = 0; i < 40; ++i) y += 0.2f * 0.1f;
        const float fovy_default = 45.0f * constants::degrees_to_radians<float>();
        const float r = length(vec3(2.0f, 2.0f, 2.0f)) * 0.5f;                  // camera::view_all, camera.inl:79-87
        float c[8] = { y, 0.0f, 0.0f, 1.0f + (r + r / std::atan(fovy_default)), 0.0f, 0.0f, 1.0f, fovy_default };
        if (argc > 1)
        {
            FILE* f = fopen(argv[1], "rb");
            if (!f || fread(c, 4, 8, f) != 8) { fprintf(stderr, "generic_primitive_hip: cannot read %s\n", argv[1]); return 2; }
            fclose(f);
        }

        // generate_frame(): the two pyramids ...
        const vec3 a(0.3f, 0.3f, 0.7f), b(0.7f, 0.3f, 0.7f), cc(0.7f, 0.3f, 0.3f), d(0.3f, 0.3f, 0.3f), top(0.5f, 0.7f, 0.5f);
        const vec3 corners[12][3] = {
            { vec3(-1, -1, 1), vec3(1, -1, 1), vec3(0, 1, 0) },   { vec3(1, -1, 1), vec3(1, -1, -1), vec3(0, 1, 0) },
            { vec3(1, -1, -1), vec3(-1, -1, -1), vec3(0, 1, 0) }, { vec3(-1, -1, -1), vec3(-1, -1, 1), vec3(0, 1, 0) },
            { vec3(1, -1, 1), vec3(-1, -1, 1), vec3(1, -1, -1) }, { vec3(-1, -1, 1), vec3(-1, -1, -1), vec3(1, -1, -1) },
            { a, b, top }, { b, cc, top }, { cc, d, top }, { d, a, top }, { b, a, cc }, { a, d, cc } };
        std::vector<primitive_type> primitives(N);
        std::vector<vec4> normals(N);                           // 16-byte rows by prim_id; a sphere's row is never read
        for (unsigned i = 0; i < N - 2; ++i)
        {
            triangle_type t;
            t.v1 = corners[i][0];
            t.e1 = corners[i][1] - t.v1;
            t.e2 = corners[i][2] - t.v1;
            t.prim_id = i;
            t.geom_id = i < 6 ? 0 : 1;
            const vec3 n = normalize(cross(t.e1, t.e2));
            normals[i] = vec4(n.x, n.y, n.z, 0.0f);
            primitives[i] = t;
        }
        // ... and the two spheres, in the same list
        sphere_type s1;
        s1.prim_id = N - 2; s1.geom_id = 2; s1.center = vec3(-0.7f, c[0], 0.8f); s1.radius = 0.5f;
        primitives[N - 2] = s1;
        sphere_type s2;
        s2.prim_id = N - 1; s2.geom_id = 3; s2.center = vec3(1.0f, 0.8f, -0.0f); s2.radius = 0.3f;
        primitives[N - 1] = s2;

        auto host_bvh = build<index_bvh<primitive_type>>(primitives.data(), primitives.size());
        hip_index_bvh<primitive_type> device_bvh(host_bvh, normals.data());

        std::vector<vrh_plastic> materials = {
            { { 0.0f, 0.0f, 0.0f }, 1.0f, { 0.0f, 1.0f, 1.0f }, 1.0f, { 0.2f, 0.4f, 0.4f }, 1.0f, 16.0f },
            { { 0.0f, 0.0f, 0.0f }, 1.0f, { 1.0f, 0.0f, 0.0f }, 1.0f, { 0.5f, 0.2f, 0.2f }, 1.0f, 128.0f },
            { { 0.0f, 0.0f, 0.0f }, 1.0f, { 0.0f, 0.0f, 1.0f }, 1.0f, { 1.0f, 1.0f, 1.0f }, 1.0f, 128.0f },
            { { 0.0f, 0.0f, 0.0f }, 1.0f, { 1.0f, 1.0f, 1.0f }, 1.0f, { 1.0f, 1.0f, 1.0f }, 1.0f, 32.0f } };
        std::vector<vrh_point_light> lights = { { { 0.0f, 10.0f, 10.0f }, { 1.0f, 1.0f, 1.0f }, 1.0f, 1.0f, 0.0f, 0.0f } };
        hip_shading shading(materials, lights);

        hip_buffer_rt<PF_RGBA32F, PF_UNSPECIFIED> rt;
        rt.resize(W, H);
        camera cam;
        cam.perspective(c[7], W / static_cast<float>(H), 0.001f, 1000.0f);
        cam.look_at(vec3(c[1], c[2], c[3]), vec3(c[4], c[5], c[6]), vec3(0.0f, 1.0f, 0.0f));
        hip_sched<ray> sched;
        auto sparams = make_sched_params(pixel_sampler::uniform_type{}, cam, rt);
        const vec4 bg(0.1f, 0.2f, 0.3f, 1.0f), ambient(1.0f, 1.0f, 1.0f, 1.0f);

        const char* names[4] = { "primary", "ao", "simple", "whitted" };
        const hip_builtin_kernel kernels[4] = {
            make_hip_closest_hit_kernel(device_bvh, bg), make_hip_ao_kernel(device_bvh, bg, 8, 0.5f, 1e-3f),
            make_hip_simple_kernel(normals_per_face_binding{}, device_bvh, shading, bg, ambient),
            make_hip_whitted_kernel(normals_per_face_binding{}, device_bvh, shading, 4, 1e-4f, bg, ambient) };
        std::vector<float> color(size_t(4) * W * H), t(size_t(W) * H);
        std::vector<uint32_t> prim_id(size_t(W) * H);
        std::vector<uint8_t> occ(size_t(W) * H);
        std::string out = "{\"W\":60,\"H\":44";
        for (int k = 0; k < 4; ++k)
        {
            sched.frame(kernels[k], sparams);
            rt.download(color.data(), prim_id.data(), t.data(), occ.data());
            out += std::string(",\"") + names[k] + "\":{\"color\":\"" + fnv(color.data(), color.size() * 4) + "\",\"prim_id\":\""
                 + fnv(prim_id.data(), prim_id.size() * 4) + "\",\"t\":\"" + fnv(t.data(), t.size() * 4) + "\",\"occ\":\""
                 + fnv(occ.data(), occ.size()) + "\"}";
        }
        size_t hits = 0;
        for (uint32_t p : prim_id) hits += p != 0xFFFFFFFFu ? 1 : 0;
        printf("%s,\"hits\":%zu}\n", out.c_str(), hits);
    }
    catch (std::exception const& e)
    {
        fprintf(stderr, "generic_primitive_hip: %s\n", e.what());
        return 1;
    }
    return 0;
}
