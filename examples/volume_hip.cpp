// examples/volume_hip.cpp -- the volume rendering example (src/examples/volume/main.cpp) on the HIP backend
// through the C++ drop-in API, headless: a scalar volume in the box [-1, 1]^3 is ray-marched with
// make_hip_volume_kernel (tex3D, a transfer function through tex1D, front-to-back compositing, early ray
// termination at opacity 0.999) and the image is written as a PFM file (RGB float, bottom row first -- the
// target's row order).  The volume is procedural: n^3 floats from an integer hash.
//
//     volume_hip [n] [width] [height] [out.pfm]
//
// Prints one JSON line: the frame's rays and steps and a hash of the colour buffer's bits (the sum of
// bits[i] * (2 i + 1) over its 32-bit words, modulo 2^64).
#include <visionaray_hip/standalone.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace visionaray;

int main(int argc, char** argv)
{
    unsigned n = argc > 1 ? unsigned(atoi(argv[1])) : 32;
    unsigned W = argc > 2 ? unsigned(atoi(argv[2])) : 320;
    unsigned H = argc > 3 ? unsigned(atoi(argv[3])) : 180;
    const char* out = argc > 4 ? argv[4] : nullptr;
    try
    {
        std::vector<float> voxels(size_t(n) * n * n);
        for (unsigned z = 0; z < n; ++z)
            for (unsigned y = 0; y < n; ++y)
                for (unsigned x = 0; x < n; ++x)
                    voxels[(size_t(z) * n + y) * n + x] = float(((x * 73856093u) ^ (y * 19349663u) ^ (z * 83492791u)) & 1023u) / 1023.0f;
        const float transfunc[4][4] = { { 0.0f, 0.0f, 0.0f, 0.0f }, { 0.9f, 0.2f, 0.1f, 0.01f }, { 0.1f, 0.8f, 0.3f, 0.04f },
                                        { 0.2f, 0.3f, 1.0f, 0.12f } };
        hip_volume volume(voxels.data(), n, n, n, /* Linear */ 1, /* Clamp */ 2, &transfunc[0][0], 4, /* Linear */ 1, /* Clamp */ 2);

        hip_buffer_rt<PF_RGBA32F, PF_UNSPECIFIED> rt;
        rt.resize(W, H);
        rt.clear_color_buffer();

        camera cam;
        cam.perspective(45.0f * constants::degrees_to_radians<float>(), W / static_cast<float>(H), 0.001f, 1000.0f);
        cam.look_at(vec3(1.5f, 1.2f, 3.0f), vec3(0.0f, 0.0f, 0.0f), vec3(0.0f, 1.0f, 0.0f));

        hip_sched<ray> sched;
        const aabb bbox(vec3(-1.0f, -1.0f, -1.0f), vec3(1.0f, 1.0f, 1.0f));
        auto kernel = make_hip_volume_kernel(volume, bbox);          // dt 0.01, cutoff 0.999, y and z flipped: the example's
        sched.frame(kernel, make_sched_params(pixel_sampler::uniform_type{}, cam, rt));
        const vrh_volume_stats st = sched.context().volume_last_stats();

        size_t npx = size_t(W) * H;
        std::vector<float> color(4 * npx);
        rt.download(color.data());
        unsigned long long hash = 0;
        for (size_t i = 0; i < 4 * npx; ++i)
        {
            uint32_t b;
            std::memcpy(&b, &color[i], 4);
            hash += (unsigned long long)b * (2ull * i + 1ull);
        }
        if (out)
        {
            FILE* f = fopen(out, "wb");
            if (!f) throw std::runtime_error("cannot write the image");
            fprintf(f, "PF\n%u %u\n-1.0\n", W, H);
            for (size_t p = 0; p < npx; ++p) fwrite(&color[4 * p], 4, 3, f);
            fclose(f);
        }
        printf("{\"n\":%u,\"W\":%u,\"H\":%u,\"rays\":%llu,\"steps\":%llu,\"capped\":%u,\"color_hash\":\"%016llx\"}\n", n, W, H,
               (unsigned long long)st.rays, (unsigned long long)st.steps, st.capped, hash);
    }
    catch (std::exception const& e)
    {
        fprintf(stderr, "volume_hip: %s\n", e.what());
        return 1;
    }
    return 0;
}
