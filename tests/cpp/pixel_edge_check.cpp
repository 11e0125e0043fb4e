// tests/cpp/pixel_edge_check.cpp -- edge cases of include/visionaray_hip/detail/vrh_pixel.h as a stand-alone
// host program (tests/test_render_target_fixtures.py builds it plain and with -fsanitize=address,undefined):
// no float -> integer conversion may be undefined and nothing may be read or written outside the arrays for NaN /
// infinite / huge colours and depths, a depth transform whose w is 0, 1 x 1 images and empty scissor boxes.
#include "visionaray_hip/detail/vrh_pixel.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

using namespace vrh::dev;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

static resolve_params params(uint32_t w, uint32_t h, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, bool blend)
{
    resolve_params P{};
    P.width = w; P.height = h;
    P.clip[0] = x0; P.clip[1] = y0; P.clip[2] = x1; P.clip[3] = y1;
    P.blend = blend ? 1u : 0u; P.s = 0.25f; P.d = 0.75f;
    P.matrix_cam = 1u;
    P.width_f = float(w); P.height_f = float(h);
    for (int i = 0; i < 4; ++i) P.view[i * 5] = P.proj[i * 5] = P.inv_view[i * 5] = P.inv_proj[i * 5] = 1.0f;
    return P;
}

int main()
{
    const float inf = std::numeric_limits<float>::infinity();
    const float nan = std::numeric_limits<float>::quiet_NaN();
    const float odd[] = { nan, -nan, inf, -inf, 3.0e38f, -3.0e38f, 1.0e10f, -1.0e10f, 0.0f, -0.0f, 1.0f, 1.0e-45f, 0.5f };
    const int n_odd = int(sizeof(odd) / sizeof(odd[0]));

    // the conversions themselves
    CHECK(float_to_unorm8(nan) == 0u && float_to_unorm8(-inf) == 0u && float_to_unorm8(inf) == 255u && float_to_unorm8(3.0e38f) == 255u);
    CHECK(float_to_unorm8(1.0f) == 255u && float_to_unorm8(0.0f) == 0u && float_to_unorm8(0.3f) == 0x4cu);
    CHECK(cvt(nan) == 0 && cvt(inf) == 2147483647 && cvt(-inf) == -2147483647 - 1 && cvt(3.0e38f) == 2147483647);
    CHECK(cvt(2147483648.0f) == 2147483647 && cvt(-2147483648.0f) == -2147483647 - 1 && cvt(2147483520.0f) == 2147483520);
    CHECK(cvt(-1.5f) == -1 && cvt(16777215.0f) == 16777215);
    CHECK(depth24_pack(1.0f) == 0xFFFFFF00u && depth24_pack(0.0f) == 0u && depth24_pack(nan) == 0u);
    const uint32_t w = 0x3f77b6e2u;
    float f;
    std::memcpy(&f, &w, 4);
    CHECK(depth24_pack(f) == 0xf7b6e100u);
    for (uint32_t u = 0; u < 256u; ++u) CHECK(float_to_unorm8(unorm8_to_float(u)) == u);

    // every odd value as colour and as t, every format, store and blend, over odd earlier contents
    for (uint32_t cf = 0; cf < 4; ++cf)
        for (uint32_t df = 0; df < 3; ++df)
            for (int blend = 0; blend < 2; ++blend)
            {
                const uint32_t W = uint32_t(n_odd), H = uint32_t(n_odd);
                std::vector<float> color(size_t(W) * H * 4), t(size_t(W) * H);
                std::vector<uint32_t> pid(size_t(W) * H);
                for (uint32_t y = 0; y < H; ++y)
                    for (uint32_t x = 0; x < W; ++x)
                    {
                        const size_t i = size_t(y) * W + x;
                        color[4 * i] = odd[x]; color[4 * i + 1] = odd[y]; color[4 * i + 2] = odd[(x + y) % n_odd]; color[4 * i + 3] = odd[(x * 3 + y) % n_odd];
                        t[i] = odd[(x + 2 * y) % n_odd];
                        pid[i] = (x + y) % 5 == 0 ? PIXEL_MISS : uint32_t(i);
                    }
                std::vector<unsigned char> cout_(size_t(W) * H * color_bytes(cf), 0xFF), dout(size_t(W) * H * 4 + 4, 0xFF);
                resolve_params P = params(W, H, 0, 0, W, H, blend != 0);
                resolve_host(cf, df, P, color.data(), pid.data(), t.data(), cout_.data(), dout.data());
                // a projection whose w is 0 everywhere: z / 0
                for (int i = 0; i < 16; ++i) P.proj[i] = 0.0f;
                P.proj[10] = 1.0f;
                resolve_host(cf, df, P, color.data(), pid.data(), t.data(), cout_.data(), dout.data());
                // singular inverses: the ray itself is NaN
                for (int i = 0; i < 16; ++i) P.inv_proj[i] = 0.0f;
                P.jitter = 1u; P.frame_num = 0xFFFFFFFFu;
                resolve_host(cf, df, P, color.data(), pid.data(), t.data(), cout_.data(), dout.data());
                // the staging t as the depth itself (a user kernel's launch): no prim ids are read
                P.matrix_cam = 0u;
                resolve_host(cf, df, P, color.data(), nullptr, t.data(), cout_.data(), dout.data());
            }

    // 1 x 1 images: exactly one element is written
    for (uint32_t cf = 0; cf < 4; ++cf)
        for (uint32_t df = 0; df < 3; ++df)
        {
            const float c[4] = { 0.3f, 1.7f, -0.2f, 0.5f };
            const uint32_t pid = 3u;
            const float t = 1.5f;
            std::vector<unsigned char> co(color_bytes(cf)), dz(4);
            const resolve_params P = params(1, 1, 0, 0, 1, 1, false);
            resolve_host(cf, df, P, c, &pid, &t, co.data(), dz.data());
            if (cf == CF_RGBA8) CHECK(co[0] == 0x4c && co[1] == 0xff && co[2] == 0x00 && co[3] == 0x7f);
            if (cf == CF_RGB8) CHECK(co[0] == 0x26 && co[1] == 0xd8 && co[2] == 0x00);
            if (df == DF_DEPTH32F) { float z; std::memcpy(&z, dz.data(), 4); CHECK(z == 0.75f); }
        }

    // empty boxes: nothing is read or written (the arrays are empty)
    for (uint32_t cf = 0; cf < 4; ++cf)
        for (uint32_t df = 0; df < 3; ++df)
            for (int blend = 0; blend < 2; ++blend)
            {
                resolve_host(cf, df, params(5, 4, 2, 2, 2, 2, blend != 0), nullptr, nullptr, nullptr, nullptr, nullptr);
                resolve_host(cf, df, params(5, 4, 3, 1, 1, 4, blend != 0), nullptr, nullptr, nullptr, nullptr, nullptr);
                resolve_host(cf, df, params(5, 4, 0, 4, 5, 4, blend != 0), nullptr, nullptr, nullptr, nullptr, nullptr);
            }

    if (failures) { std::printf("pixel_edge_check: %d failures\n", failures); return 1; }
    std::printf("pixel_edge_check ok\n");
    return 0;
}
