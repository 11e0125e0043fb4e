// tests/cpp/volume_user_kernel.hip -- the volume example's kernel (src/examples/volume/main.cpp:123-167) as a
// USER kernel: the reference's lambda, nearly verbatim, compiled by hipcc over visionaray_hip/hip_kernels.h
// (intersect(ray, aabb), tex3D and tex1D on device refs of a hip_volume) and run by hip_sched::frame.  Two
// changes from the reference's text: the ray type is scalar, so the any() / all() / select() of the packet
// version fall away, and `color.xyz() *= color.w` is written out (the stand-alone vector has no xyz()
// reference).
//
//     volume_user_kernel [n] [width] [height]
//         the scene of examples/volume_hip.cpp through the lambda AND through the built-in kernel: one JSON
//         line with both colour hashes (tests/test_gpu_cpp_volume.py: they are equal, and equal to the
//         example's and to the Python API's)
//     volume_user_kernel bench <r8|r32f> [n] [width] [height] [reps]
//         the measurement of tools/volume_bench.py: a procedural n^3 volume (linear / clamp), a 256-entry
//         linear transfer function, the view_all camera, dt = box extent / 512; after a warm-up of both, `reps`
//         alternated frames of A (the built-in kernel) and B (the lambda), each timed from issue to
//         completion: one JSON line with the medians
#include <visionaray_hip/hip_kernels.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace visionaray;

using rt_type = hip_buffer_rt<PF_RGBA32F, PF_UNSPECIFIED>;

static unsigned long long color_hash(rt_type& rt)
{
    std::vector<float> color(4 * rt.width() * rt.height());
    rt.download(color.data());
    unsigned long long hash = 0;
    for (size_t i = 0; i < color.size(); ++i)
    {
        uint32_t b;
        std::memcpy(&b, &color[i], 4);
        hash += (unsigned long long)b * (2ull * i + 1ull);
    }
    return hash;
}

// the example's lambda over device refs; dt and the cutoff as the example writes them unless given
template <typename SP>
static void lambda_frame(hip_sched<ray>& sched, hip_volume const& vol, aabb bbox, float dt, SP sparams)
{
    using R = ray;
    using S = float;
    using C = vector<4, S>;
    const hip_volume_ref volume = volume_ref(vol);
    const hip_transfunc_ref transfunc = transfunc_ref(vol);
    sched.frame([=] __device__ (R ray) -> result_record<S>
    {
        result_record<S> result;

        auto hit_rec = intersect(ray, bbox);
        auto t = hit_rec.tnear;

        result.color = C(0.0);

        while (t < hit_rec.tfar)
        {
            auto pos = ray.ori + ray.dir * t;
            auto tex_coord = vector<3, S>(
                    ( pos.x + 1.0f ) / 2.0f,
                    (-pos.y + 1.0f ) / 2.0f,
                    (-pos.z + 1.0f ) / 2.0f
                    );

            // sample volume and do post-classification
            auto voxel = tex3D(volume, tex_coord);
            C color = tex1D(transfunc, voxel);

            // premultiplied alpha
            color = C(color.xyz() * color.w, color.w);

            // front-to-back alpha compositing
            result.color += color * (1.0f - result.color.w);

            // early-ray termination - don't traverse w/o a contribution
            if (result.color.w >= 0.999)
            {
                break;
            }

            // step on
            t += dt;
        }

        result.hit = hit_rec.hit;
        return result;
    }, sparams);
}

static int scene(unsigned n, unsigned W, unsigned H)
{
    std::vector<float> voxels(size_t(n) * n * n);
    for (unsigned z = 0; z < n; ++z)
        for (unsigned y = 0; y < n; ++y)
            for (unsigned x = 0; x < n; ++x)
                voxels[(size_t(z) * n + y) * n + x] = float(((x * 73856093u) ^ (y * 19349663u) ^ (z * 83492791u)) & 1023u) / 1023.0f;
    const float transfunc[4][4] = { { 0.0f, 0.0f, 0.0f, 0.0f }, { 0.9f, 0.2f, 0.1f, 0.01f }, { 0.1f, 0.8f, 0.3f, 0.04f },
                                    { 0.2f, 0.3f, 1.0f, 0.12f } };
    hip_volume volume(voxels.data(), n, n, n, 1, 2, &transfunc[0][0], 4, 1, 2);
    rt_type rt;
    rt.resize(W, H);
    camera cam;
    cam.perspective(45.0f * constants::degrees_to_radians<float>(), W / static_cast<float>(H), 0.001f, 1000.0f);
    cam.look_at(vec3(1.5f, 1.2f, 3.0f), vec3(0.0f, 0.0f, 0.0f), vec3(0.0f, 1.0f, 0.0f));
    hip_sched<ray> sched(hip_context::default_context(), false);
    const aabb bbox(vec3(-1.0f, -1.0f, -1.0f), vec3(1.0f, 1.0f, 1.0f));
    auto sparams = make_sched_params(pixel_sampler::uniform_type{}, cam, rt);

    rt.clear_color_buffer(vec4(9.0f, 9.0f, 9.0f, 9.0f));
    lambda_frame(sched, volume, bbox, 0.01f, sparams);
    const unsigned long long lambda = color_hash(rt);
    rt.clear_color_buffer(vec4(9.0f, 9.0f, 9.0f, 9.0f));
    sched.frame(make_hip_volume_kernel(volume, bbox), sparams);
    const vrh_volume_stats st = sched.context().volume_last_stats();
    const unsigned long long builtin = color_hash(rt);
    printf("{\"n\":%u,\"W\":%u,\"H\":%u,\"steps\":%llu,\"lambda_hash\":\"%016llx\",\"builtin_hash\":\"%016llx\"}\n", n, W, H,
           (unsigned long long)st.steps, lambda, builtin);
    return lambda == builtin ? 0 : 1;
}

static double median(std::vector<double> v)
{
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

template <typename T>
static int bench(const char* name, unsigned n, unsigned W, unsigned H, unsigned reps)
{
    // smooth blobs: voxel = a product of three sines of the position, scaled into the format's range
    std::vector<T> voxels(size_t(n) * n * n);
    const float top = std::is_same<T, float>::value ? 1.0f : 255.0f;
    for (unsigned z = 0; z < n; ++z)
        for (unsigned y = 0; y < n; ++y)
            for (unsigned x = 0; x < n; ++x)
            {
                const float s = std::sin(9.0f * x / n) * std::sin(7.0f * y / n + 1.0f) * std::sin(5.0f * z / n + 2.0f);
                voxels[(size_t(z) * n + y) * n + x] = T((0.5f + 0.5f * s) * top);
            }
    std::vector<float> tf(256 * 4);
    for (int i = 0; i < 256; ++i)
    {
        const float u = i / 255.0f;
        tf[4 * i] = u; tf[4 * i + 1] = 1.0f - u; tf[4 * i + 2] = 0.5f + 0.5f * std::sin(20.0f * u);
        tf[4 * i + 3] = 0.02f * u * u;
    }
    hip_volume volume(voxels.data(), n, n, n, 1, 2, tf.data(), 256, 1, 2);
    rt_type rt;
    rt.resize(W, H);
    const aabb bbox(vec3(-1.0f, -1.0f, -1.0f), vec3(1.0f, 1.0f, 1.0f));
    camera cam;
    const float fovy = 45.0f * constants::degrees_to_radians<float>();
    cam.perspective(fovy, W / static_cast<float>(H), 0.001f, 1000.0f);
    // camera::view_all (detail/camera.inl:79-87)
    const float r = std::sqrt(12.0f) * 0.5f;
    cam.look_at(vec3(0.0f, 0.0f, r + r / std::atan(fovy)), vec3(0.0f, 0.0f, 0.0f), vec3(0.0f, 1.0f, 0.0f));
    hip_sched<ray> sched(hip_context::default_context(), false);      // frame() returns when the frame is done
    auto sparams = make_sched_params(pixel_sampler::uniform_type{}, cam, rt);
    const float dt = 2.0f / 512.0f;
    const auto kernel = make_hip_volume_kernel(volume, bbox, dt);

    auto timed = [&](bool builtin) {
        const auto t0 = std::chrono::steady_clock::now();
        if (builtin) sched.frame(kernel, sparams);
        else lambda_frame(sched, volume, bbox, dt, sparams);
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    };
    for (int w = 0; w < 2; ++w) { timed(true); timed(false); }        // warm-up of both
    std::vector<double> a, b;
    for (unsigned i = 0; i < reps; ++i) { a.push_back(timed(true)); b.push_back(timed(false)); }
    const unsigned long long hb = color_hash(rt);                      // the last frame: the lambda's
    sched.frame(kernel, sparams);
    const vrh_volume_stats st = sched.context().volume_last_stats();
    const unsigned long long ha = color_hash(rt);
    const double ma = median(a), mb = median(b);
    printf("{\"format\":\"%s\",\"n\":%u,\"W\":%u,\"H\":%u,\"reps\":%u,\"rays\":%llu,\"steps\":%llu,\"builtin_ms\":%.4f,\"lambda_ms\":%.4f,"
           "\"builtin_gsteps_per_s\":%.3f,\"lambda_gsteps_per_s\":%.3f,\"same_bits\":%s}\n", name, n, W, H, reps,
           (unsigned long long)st.rays, (unsigned long long)st.steps, ma, mb, st.steps / ma * 1e-6, st.steps / mb * 1e-6,
           ha == hb ? "true" : "false");
    return 0;
}

int main(int argc, char** argv)
{
    try
    {
        if (argc > 2 && std::string(argv[1]) == "bench")
        {
            const unsigned n = argc > 3 ? unsigned(atoi(argv[3])) : 256, W = argc > 4 ? unsigned(atoi(argv[4])) : 1920;
            const unsigned H = argc > 5 ? unsigned(atoi(argv[5])) : 1080, reps = argc > 6 ? unsigned(atoi(argv[6])) : 5;
            if (std::string(argv[2]) == "r8") return bench<uint8_t>("r8", n, W, H, reps);
            return bench<float>("r32f", n, W, H, reps);
        }
        const unsigned n = argc > 1 ? unsigned(atoi(argv[1])) : 32, W = argc > 2 ? unsigned(atoi(argv[2])) : 320;
        const unsigned H = argc > 3 ? unsigned(atoi(argv[3])) : 180;
        return scene(n, W, H);
    }
    catch (std::exception const& e)
    {
        fprintf(stderr, "volume_user_kernel: %s\n", e.what());
        return 2;
    }
}
