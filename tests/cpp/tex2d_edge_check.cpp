// The shared texture sampler (include/visionaray_hip/detail/vrh_texture.h) on the CPU under AddressSanitizer
// and UndefinedBehaviorSanitizer (tests/test_textures.py builds it with g++ -fsanitize=address,undefined):
// a stand-alone host program.  Over textures of 1x1, 2x2, 5x3, 16x16 and 64x37 texels held in exact-size
// heap blocks, both filters and all nine address-mode pairs, it samples the whole edge list of
// tests/tex_cases.py crossed with itself -- 0, -0.0, +-1, 2, k/N, the floats next to k/N, (k + 1/2)/N,
// +-1e-8, -1e-30, the float below 1, +-(2^20 - 0.7) -- for EVERY k in 0..N.  A read outside a block or an
// undefined float -> int conversion ends the program with the sanitizer's report.  It also checks that a
// texture of zeros samples to zero everywhere (any interpolation of zeros is zero).
#include "visionaray_hip/detail/vrh_texture.h"

#include <cmath>
#include <cstdio>
#include <memory>
#include <vector>

using namespace vrh::dev;

static std::vector<float> edge_values(int n)
{
    std::vector<float> v = { 0.0f, -0.0f, 1.0f, -1.0f, 2.0f, 1e-8f, -1e-8f, -1e-30f, std::nextafterf(1.0f, 0.0f),
                             TEX_MAX_COORD - 0.7f, -(TEX_MAX_COORD - 0.7f), TEX_MAX_COORD, -TEX_MAX_COORD };
    for (int k = 0; k <= n; ++k)
    {
        const float q = float(k) / float(n);
        v.push_back(q);
        v.push_back(std::nextafterf(q, -4.0f));
        v.push_back(std::nextafterf(q, 4.0f));
        v.push_back((float(k) + 0.5f) / float(n));
    }
    return v;
}

int main()
{
    const int sizes[5][2] = { { 1, 1 }, { 2, 2 }, { 5, 3 }, { 16, 16 }, { 64, 37 } };
    unsigned long long samples = 0, sum = 0;
    for (const auto& sz : sizes)
    {
        const int w = sz[0], h = sz[1];
        // exact-size heap blocks: one of hashed texels, one of zeros
        std::unique_ptr<uint32_t[]> texels(new uint32_t[size_t(w) * h]), flat(new uint32_t[size_t(w) * h]);
        for (int i = 0; i < w * h; ++i)
        {
            texels[i] = uint32_t(i) * 2654435761u ^ 0x9E3779B9u;
            flat[i] = 0u;
        }
        const std::vector<float> ex = edge_values(w), ey = edge_values(h);
        for (uint32_t filter = 0; filter < 2; ++filter)
            for (uint32_t ax = 0; ax < 3; ++ax)
                for (uint32_t ay = 0; ay < 3; ++ay)
                {
                    const tex_view t = make_tex_view(texels.get(), uint32_t(w), uint32_t(h), filter, ax, ay);
                    const tex_view f = make_tex_view(flat.get(), uint32_t(w), uint32_t(h), filter, ax, ay);
                    for (float x : ex)
                        for (float y : ey)
                        {
                            sum += tex2d(t, x, y);
                            if (tex2d(f, x, y) != 0u)
                            {
                                std::printf("FAILED: %dx%d filter %u address %u %u at (%.9g, %.9g): a texture of zeros sampled to %08x\n",
                                            w, h, filter, ax, ay, x, y, tex2d(f, x, y));
                                return 1;
                            }
                            ++samples;
                        }
                }
    }
    for (uint32_t k = 0; k < 256; ++k)
        if (unorm8(k) != float(double(float(k)) / 255.0) || !(unorm8(k) >= 0.0f && unorm8(k) <= 1.0f))
        {
            std::printf("FAILED: unorm8(%u)\n", k);
            return 1;
        }
    std::printf("tex2d_edge_check ok: %llu samples (checksum %llx)\n", samples, sum);
    return 0;
}
