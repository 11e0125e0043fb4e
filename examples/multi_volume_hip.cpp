// examples/multi_volume_hip.cpp -- the multi-volume rendering example (src/examples/multi_volume/main.cpp) on the
// HIP backend through the C++ drop-in API, headless.  Three procedural volumes -- the Marschner-Lobb signal
// (201^3), a heart surface (256^3) and a mandelbulb (256^3), linear / clamp -- each with its 5-entry nearest /
// clamp transfer function, rotated by pi / 4 about x, y and z and translated by 2.5 i along x, with the example's
// plastic material and a point light at the eye, are marched together by make_hip_multi_volume_kernel (dt
// 0.007, gradient shading where alpha >= 0.1, early ray termination at opacity 0.999).  The image is written
// as a binary PPM (PNM P6, top row first).  The three volumes are this program's own statements of the example's
// formulas: the same fields, not promised to be the example's voxels to the last bit (the C library's cos, sin,
// atan2 and pow decide that).
//
//     multi_volume_hip [width] [height] [out.ppm] [scale]
//
// `scale` (default 1.0) multiplies the volumes' side lengths.  Prints one JSON line: the frame's rays and steps
// and a hash of the colour buffer's bits (the sum of bits[i] * (2 i + 1) over its 32-bit words, modulo 2^64).
//
//     multi_volume_hip --volumes in.bin out.bin
//
// renders three given float volumes in place of the procedural ones: in.bin holds u32 width, height; 11 floats
// eye, center, up, fovy, aspect; then per volume u32 w, h, d and its w * h * d floats.  out.bin gets the colour
// buffer (RGBA float, bottom row first), the prim_id buffer (u32) and the t buffer (float), then u64 rays, u64 steps.
//
// Compiles two ways: against visionaray_hip/standalone.h alone (vrh_plastic / vrh_point_light records), and with
// -DVRH_TEST_REFERENCE_HEADERS against the reference's own headers, whose aabb, mat4, plastic<float> and
// point_light<float> objects go into make_hip_multi_volume_kernel unchanged.
#ifdef VRH_TEST_REFERENCE_HEADERS
#include <visionaray/math/math.h>
#include <visionaray/camera.h>
#include <visionaray/material.h>
#include <visionaray/pixel_format.h>
#include <visionaray/point_light.h>
#include <visionaray/scheduler.h>

#include <visionaray_hip/hip_backend.h>
#else
#include <visionaray_hip/standalone.h>
#endif

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace visionaray;

namespace {

// the post-classification transfer functions of the example
const float tfdata[3][5][4] = {
    { { 0.0f, 0.2f, 0.8f, 0.005f }, { 1.0f, 0.8f, 0.0f, 0.01f }, { 0.0f, 1.0f, 0.0f, 0.50f }, { 1.0f, 0.8f, 0.0f, 0.01f }, { 1.0f, 1.0f, 1.0f, 0.005f } },
    { { 1.0f, 0.0f, 0.0f, 1.0f }, { 1.0f, 0.0f, 0.0f, 0.2f }, { 1.0f, 0.0f, 0.0f, 0.2f }, { 1.0f, 0.0f, 0.0f, 0.2f }, { 1.0f, 1.0f, 1.0f, 0.002f } },
    { { 1.0f, 1.0f, 1.0f, 1.0f }, { 1.0f, 1.0f, 1.0f, 0.50f }, { 1.0f, 1.0f, 1.0f, 0.50f }, { 1.0f, 1.0f, 1.0f, 0.50f }, { 0.0f, 0.0f, 1.0f, 0.002f } } };

struct voxels { unsigned w, h, d; std::vector<float> data; };

const float PI = constants::pi<float>();

voxels marschner_lobb(unsigned n)
{
    voxels v{ n, n, n, std::vector<float>(size_t(n) * n * n) };
    const float fM = 6.0f, a = 0.25f;
    for (unsigned z = 0; z < n; ++z)
        for (unsigned y = 0; y < n; ++y)
            for (unsigned x = 0; x < n; ++x)
            {
                const float xx = float(x) / n * 2.0f - 1.0f, yy = float(y) / n * 2.0f - 1.0f, zz = float(z) / n * 2.0f - 1.0f;
                const float rho = std::cos(2 * PI * fM * std::cos(PI * std::sqrt(xx * xx + yy * yy) / 2));
                v.data[(size_t(z) * n + y) * n + x] = (1 - std::sin(PI * zz / 2) + a * (1 + rho)) / (2 * (1 + a));
            }
    return v;
}

voxels heart(unsigned n)
{
    voxels v{ n, n, n, std::vector<float>(size_t(n) * n * n) };
    for (unsigned z = 0; z < n; ++z)
        for (unsigned y = 0; y < n; ++y)
            for (unsigned x = 0; x < n; ++x)
            {
                const float xx = float(x) / n * 4.0f - 2.0f, yy = float(y) / n * 4.0f - 2.0f, zz = float(z) / n * 4.0f - 2.0f;
                // the cube through pow in double and the differences in double, rounded to float on the store, as in the example
                const float s = xx * xx + (9.0f / 4.0f) * (yy * yy) + zz * zz - 1;
                v.data[(size_t(z) * n + y) * n + x] = float(std::pow(double(s), 3.0) - double((xx * xx) * (zz * zz * zz))
                                                            - double((9.0f / 80.0f) * (yy * yy) * (zz * zz * zz)));
            }
    return v;
}

voxels mandelbulb(unsigned n)
{
    voxels v{ n, n, n, std::vector<float>(size_t(n) * n * n) };
    const float power = 8.0f;
    for (unsigned z = 0; z < n; ++z)
        for (unsigned y = 0; y < n; ++y)
            for (unsigned x = 0; x < n; ++x)
            {
                const float v0[3] = { 3.0f * (float(x) - n / 2.0f) / n, 3.0f * (float(y) - n / 2.0f) / n, 3.0f * (float(z) - n / 2.0f) / n };
                float p[3] = { v0[0], v0[1], v0[2] };
                int i = 0;
                for (; i < 8; ++i)
                {
                    const float r = std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
                    const float theta = std::atan2(std::sqrt(p[0] * p[0] + p[1] * p[1]), p[2]), phi = std::atan2(p[1], p[0]);
                    const float rn = std::pow(r, power);
                    p[0] = rn * std::sin(theta * power) * std::cos(phi * power) + v0[0];
                    p[1] = rn * std::sin(theta * power) * std::sin(phi * power) + v0[1];
                    p[2] = rn * std::cos(theta * power);
                    if (p[0] * p[0] + p[1] * p[1] + p[2] * p[2] > 2.0f) break;
                }
                v.data[(size_t(z) * n + y) * n + x] = i < 8 ? 1.0f : 0.0f;
            }
    return v;
}

struct frame_result { std::vector<float> color, t; std::vector<uint32_t> prim_id; vrh_volume_stats stats; };

// the example's scene around three volumes
frame_result render(std::vector<voxels> const& vols, camera const& cam, unsigned W, unsigned H)
{
    std::vector<hip_volume> volumes;
    std::vector<aabb> bboxes;
    std::vector<mat4> transforms;
#ifdef VRH_TEST_REFERENCE_HEADERS
    std::vector<plastic<float>> materials;
#else
    std::vector<vrh_plastic> materials;
#endif
    for (size_t i = 0; i < vols.size(); ++i)
    {
        volumes.emplace_back(vols[i].data.data(), vols[i].w, vols[i].h, vols[i].d, /* Linear */ 1, /* Clamp */ 2, &tfdata[i % 3][0][0], 5,
                             /* Nearest */ 0, /* Clamp */ 2);
        bboxes.emplace_back(vec3(-1.0f, -1.0f, -1.0f), vec3(1.0f, 1.0f, 1.0f));
        vec3 axis(i % 3 == 0 ? 1.0f : 0.0f, i % 3 == 1 ? 1.0f : 0.0f, i % 3 == 2 ? 1.0f : 0.0f);
        mat4 r = rotate(mat4::identity(), axis, PI / 4.0f);
        mat4 s = scale(mat4::identity(), vec3(1.0f, 1.0f, 1.0f));
        mat4 t = translate(mat4::identity(), vec3(i * 2.5f, 0.0f, 0.0f));
        transforms.push_back(t * r * s);
#ifdef VRH_TEST_REFERENCE_HEADERS
        plastic<float> m;
        m.set_ca(from_rgb(vec3(0.2f, 0.2f, 0.2f)));
        m.set_cd(from_rgb(vec3(0.8f, 0.8f, 0.8f)));
        m.set_cs(from_rgb(vec3(0.8f, 0.8f, 0.8f)));
        m.set_ka(1.0f);
        m.set_kd(1.0f);
        m.set_ks(1.0f);
        m.set_specular_exp(128.0f);
#else
        vrh_plastic m{};
        for (int c = 0; c < 3; ++c) { m.ca[c] = 0.2f; m.cd[c] = 0.8f; m.cs[c] = 0.8f; }
        m.ka = m.kd = m.ks = 1.0f;
        m.exp = 128.0f;
#endif
        materials.push_back(m);
    }
#ifdef VRH_TEST_REFERENCE_HEADERS
    point_light<float> light;
    light.set_cl(vec3(1.0f, 1.0f, 1.0f));
    light.set_kl(1.0f);
    light.set_position(cam.eye());
#else
    vrh_point_light light{};
    light.position[0] = cam.eye().x; light.position[1] = cam.eye().y; light.position[2] = cam.eye().z;
    light.cl[0] = light.cl[1] = light.cl[2] = 1.0f;
    light.kl = 1.0f;
    light.constant_att = 1.0f;
#endif

    hip_buffer_rt<PF_RGBA32F, PF_UNSPECIFIED> rt;
    rt.resize(W, H);
    rt.clear_color_buffer();
    hip_sched<ray> sched;
    auto kernel = make_hip_multi_volume_kernel(volumes, bboxes, transforms, materials, light);     // the example's constants
    sched.frame(kernel, make_sched_params(pixel_sampler::uniform_type{}, cam, rt));
    frame_result res;
    res.stats = sched.context().volume_last_stats();
    res.color.resize(size_t(4) * W * H);
    res.prim_id.resize(size_t(W) * H);
    res.t.resize(size_t(W) * H);
    rt.download(res.color.data(), res.prim_id.data(), res.t.data());     // prim_id 0 / 0xFFFFFFFF and tmin / -1 per pixel
    return res;
}

int from_file(const char* in_name, const char* out_name)
{
    FILE* in = fopen(in_name, "rb");
    if (!in) throw std::runtime_error("cannot read the volumes");
    uint32_t size[2];
    float la[11];
    if (fread(size, 4, 2, in) != 2 || fread(la, 4, 11, in) != 11) throw std::runtime_error("short header");
    std::vector<voxels> vols(3);
    for (auto& v : vols)
    {
        uint32_t d[3];
        if (fread(d, 4, 3, in) != 3) throw std::runtime_error("short volume header");
        v.w = d[0]; v.h = d[1]; v.d = d[2];
        v.data.resize(size_t(d[0]) * d[1] * d[2]);
        if (fread(v.data.data(), 4, v.data.size(), in) != v.data.size()) throw std::runtime_error("short volume");
    }
    fclose(in);
    camera cam;
    cam.perspective(la[9], la[10], 0.001f, 1000.0f);
    cam.look_at(vec3(la[0], la[1], la[2]), vec3(la[3], la[4], la[5]), vec3(la[6], la[7], la[8]));
    const frame_result res = render(vols, cam, size[0], size[1]);
    FILE* out = fopen(out_name, "wb");
    if (!out) throw std::runtime_error("cannot write the frame");
    const unsigned long long st[2] = { res.stats.rays, res.stats.steps };
    fwrite(res.color.data(), 4, res.color.size(), out);
    fwrite(res.prim_id.data(), 4, res.prim_id.size(), out);
    fwrite(res.t.data(), 4, res.t.size(), out);
    fwrite(st, 8, 2, out);
    fclose(out);
    return res.stats.capped ? 1 : 0;
}

} // namespace

int main(int argc, char** argv)
{
    try
    {
        if (argc == 4 && !strcmp(argv[1], "--volumes")) return from_file(argv[2], argv[3]);
        unsigned W = argc > 1 ? unsigned(atoi(argv[1])) : 512;
        unsigned H = argc > 2 ? unsigned(atoi(argv[2])) : 512;
        const char* out = argc > 3 && argv[3][0] ? argv[3] : nullptr;
        const float scale_by = argc > 4 ? float(atof(argv[4])) : 1.0f;
        std::vector<voxels> vols;
        vols.push_back(marschner_lobb(unsigned(201 * scale_by)));
        vols.push_back(heart(unsigned(256 * scale_by)));
        vols.push_back(mandelbulb(unsigned(256 * scale_by)));

        camera cam;
        cam.perspective(45.0f * constants::degrees_to_radians<float>(), W / static_cast<float>(H), 0.001f, 1000.0f);
        cam.look_at(vec3(2.5f, 1.0f, 11.0f), vec3(2.5f, 0.0f, 0.0f), vec3(0.0f, 1.0f, 0.0f));     // all three boxes in view
        const frame_result res = render(vols, cam, W, H);

        const size_t npx = size_t(W) * H;
        unsigned long long hash = 0;
        for (size_t i = 0; i < 4 * npx; ++i)
        {
            uint32_t b;
            std::memcpy(&b, &res.color[i], 4);
            hash += (unsigned long long)b * (2ull * i + 1ull);
        }
        if (out)
        {
            FILE* f = fopen(out, "wb");
            if (!f) throw std::runtime_error("cannot write the image");
            fprintf(f, "P6\n%u %u\n255\n", W, H);
            for (unsigned y = H; y-- > 0;)
                for (unsigned x = 0; x < W; ++x)
                    for (int c = 0; c < 3; ++c)
                    {
                        const float v = res.color[4 * (size_t(y) * W + x) + c];
                        fputc(int(v <= 0.0f ? 0.0f : v >= 1.0f ? 255.0f : v * 255.0f + 0.5f), f);
                    }
            fclose(f);
        }
        printf("{\"W\":%u,\"H\":%u,\"volumes\":3,\"rays\":%llu,\"steps\":%llu,\"capped\":%u,\"color_hash\":\"%016llx\"}\n", W, H,
               (unsigned long long)res.stats.rays, (unsigned long long)res.stats.steps, res.stats.capped, hash);
    }
    catch (std::exception const& e)
    {
        fprintf(stderr, "multi_volume_hip: %s\n", e.what());
        return 1;
    }
    return 0;
}
