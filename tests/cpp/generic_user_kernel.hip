// tests/cpp/generic_user_kernel.hip -- a generic-primitive scene (VRH_PRIM_GENERIC80) and user kernels
// (tests/test_gpu_cpp_generic.py).  User kernels decide "triangle, else sphere" from a view's kind, so a generic
// view is never walked:
//   * hip_index_bvh<generic_primitive<...>>::ref() does not compile (tests/test_cpp_generic.py);
//   * checked_ref on a view taken with vrh_scene_get_view throws VRH_ERR_UNSUPPORTED;
//   * a view handed to a kernel unchecked has its closest_hit / any_hit calls declined on the device -- they
//     return misses, never a hit of a record read as the wrong kind -- and the wait for the frame throws
//     VRH_ERR_UNSUPPORTED once; the context stays usable, and the built-in kernel then renders the scene.
// Prints one JSON line: the two statuses, the prim ids the declined frame wrote that were not misses (0), and the
// hits of the built-in frame that follows.
#include <visionaray_hip/hip_kernels.h>

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace visionaray;

static auto primary_kernel(hip_bvh_ref ref)
{
    return [=] __device__ (ray r) mutable -> result_record<float>
    {
        result_record<float> result;
        result.color = vec4(__uint_as_float(0xFFFFFFFFu), -1.0f, 0.0f, 1.0f);
        auto hr = closest_hit(r, &ref, &ref + 1);
        if (hr.hit) result.color = vec4(__uint_as_float(unsigned(hr.prim_id)), hr.t, 0.0f, 1.0f);
        auto ah = any_hit(r, &ref, &ref + 1, 100.0f);
        if (ah.hit) result.color.z = 1.0f;
        result.hit = hr.hit;
        return result;
    };
}

int main()
{
    using tri_t = basic_triangle<3, float>;
    using sphere_t = basic_sphere<float>;
    using prim_t = generic_primitive<tri_t, sphere_t>;
    const unsigned W = 60, H = 44;
    try
    {
        // a wall of two triangles behind a sphere, seen from +z: every pixel near the centre has a hit
        std::vector<prim_t> prims;
        tri_t t0(vec3(-2.0f, -2.0f, -1.0f), vec3(4.0f, 0.0f, 0.0f), vec3(0.0f, 4.0f, 0.0f));
        tri_t t1(vec3(2.0f, 2.0f, -1.0f), vec3(-4.0f, 0.0f, 0.0f), vec3(0.0f, -4.0f, 0.0f));
        t0.prim_id = 0; t1.prim_id = 1;
        sphere_t s(vec3(0.0f, 0.0f, 0.0f), 0.5f);
        s.prim_id = 2;
        prims.push_back(t0); prims.push_back(s); prims.push_back(t1);
        auto host = build<index_bvh<prim_t>>(prims.data(), prims.size());
        std::vector<vec4> normals(prims.size(), vec4(0.0f, 0.0f, 1.0f, 0.0f));
        hip_index_bvh<prim_t> dev(host, normals.data());

        hip_bvh_ref view{};
        hip_detail::check(vrh_scene_get_view(dev.handle(), 0, &view.view), "vrh_scene_get_view");
        if (view.view.prim_kind != VRH_PRIM_GENERIC80) { fprintf(stderr, "the view does not carry the kind\n"); return 1; }
        int checked_status = 0;
        try { (void)checked_ref(view); }
        catch (hip_error const& e) { checked_status = e.status; }

        hip_buffer_rt<PF_RGBA32F, PF_UNSPECIFIED> rt;
        rt.resize(W, H);
        camera cam;
        cam.perspective(45.0f * constants::degrees_to_radians<float>(), W / static_cast<float>(H), 0.001f, 1000.0f);
        cam.look_at(vec3(0.0f, 0.0f, 3.0f), vec3(0.0f, 0.0f, 0.0f), vec3(0.0f, 1.0f, 0.0f));
        hip_sched<ray> sched;
        auto sp = make_sched_params(pixel_sampler::uniform_type{}, cam, rt);
        std::vector<float> out(4 * size_t(W) * H);
        int declined_status = 0;
        std::string declined_text;
        try
        {
            sched.frame(primary_kernel(view), sp);
            rt.download(out.data());
        }
        catch (hip_error const& e) { declined_status = e.status; declined_text = e.what(); }
        hip_context::default_context()->sync();                  // reported once: nothing left to throw
        rt.download(out.data());
        size_t wrong = 0;
        for (size_t p = 0; p < size_t(W) * H; ++p)
        {
            uint32_t bits;
            memcpy(&bits, &out[4 * p], 4);
            wrong += (bits != 0xFFFFFFFFu || out[4 * p + 2] != 0.0f) ? 1 : 0;
        }
        // the built-in kernel renders the same scene on the same context and target
        sched.frame(make_hip_closest_hit_kernel(dev, vec4(0.1f, 0.2f, 0.3f, 1.0f)), sp);
        std::vector<uint32_t> pid(size_t(W) * H);
        rt.download(out.data(), pid.data());
        size_t hits = 0;
        for (uint32_t p : pid) hits += p != 0xFFFFFFFFu ? 1 : 0;
        const uint32_t centre = pid[size_t(H / 2) * W + W / 2];
        printf("{\"checked_ref_status\":%d,\"declined_status\":%d,\"names_generic\":%d,\"wrong_pixels\":%zu,\"builtin_hits\":%zu,"
               "\"centre_prim\":%u}\n", checked_status, declined_status, declined_text.find("generic") != std::string::npos ? 1 : 0,
               wrong, hits, centre);
    }
    catch (std::exception const& e)
    {
        fprintf(stderr, "generic_user_kernel: %s\n", e.what());
        return 1;
    }
    return 0;
}
