// tests/cpp/volume_edge_check.cpp -- stand-alone check of the shared volume header
// (include/visionaray_hip/detail/vrh_volume.h) on its edge cases, meant to run plain and under
// -fsanitize=address,undefined (tests/test_volume_sampling.py):
//   * coordinates that map to exactly 1.0 under Wrap (index N of an axis), the largest coordinates, every
//     address mode, both filters, the three voxel formats -- on heap arrays of exactly the volume's size, so
//     a read outside the array is an error of the sanitizer;
//   * the same for the transfer function;
//   * box clips with zero direction components and an origin on a slab plane (NaN slab distances);
//   * the step limit: a march stopped by it reports so and takes exactly `cap` steps.
#include "visionaray_hip/detail/vrh_volume.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace vrh::dev;

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

static const float edge_coords[] = { 0.0f, -0.0f, 1.0f, -1.0f, 2.0f, 1e-8f, -1e-8f, -1e-30f, 0.99999994f, 0.5f, 0.25f, -0.75f,
                                     3.5f, -2.5f, 1048575.3f, -1048575.3f, 1048576.0f, -1048576.0f };
static const int num_edges = int(sizeof(edge_coords) / sizeof(edge_coords[0]));

template <typename S>
static void check_volume(uint32_t fmt, uint32_t w, uint32_t h, uint32_t d, float lo, float hi)
{
    std::vector<S> vox(size_t(w) * h * d);
    for (size_t i = 0; i < vox.size(); ++i) vox[i] = S((i * 2654435761u >> 8) % 251u) ;
    for (uint32_t filter = 0; filter < 2; ++filter)
        for (uint32_t a = 0; a < 27; ++a)
        {
            const uint32_t address[3] = { a % 3, (a / 3) % 3, a / 9 };
            const vol_view v = make_vol_view(vox.data(), w, h, d, fmt, filter, address);
            for (int i = 0; i < num_edges; ++i)
                for (int j = 0; j < num_edges; ++j)
                    for (int k = 0; k < num_edges; ++k)
                    {
                        const float s = tex3d(v, edge_coords[i], edge_coords[j], edge_coords[k]);
                        EXPECT(s >= lo && s <= hi);
                    }
        }
}

static void check_transfunc(uint32_t n)
{
    std::vector<rgba_t> e(n);
    for (uint32_t i = 0; i < n; ++i) e[i] = rgba_t{ float(i), 0.5f, 1.0f, 0.25f };
    for (uint32_t filter = 0; filter < 2; ++filter)
        for (uint32_t a = 0; a < 3; ++a)
        {
            const tf_view t = make_tf_view(e.data(), n, filter, a);
            for (int i = 0; i < num_edges; ++i)
            {
                const rgba_t c = tex1d(t, t.entries, edge_coords[i]);
                // (1 - u) * a + u * a may round an ulp off a
                EXPECT(c.x >= 0.0f && c.x <= float(n - 1) * 1.000001f && std::fabs(c.y - 0.5f) < 1e-6f && std::fabs(c.z - 1.0f) < 1e-6f
                       && std::fabs(c.w - 0.25f) < 1e-6f);
            }
        }
}

static void check_clip_and_cap()
{
    const float bmin[3] = { -1.0f, -1.0f, -1.0f }, bmax[3] = { 1.0f, 1.0f, 1.0f };
    float tn, tf;
    // through the centre along x
    {
        const float o[3] = { -3.0f, 0.0f, 0.0f }, d[3] = { 1.0f, 0.0f, 0.0f };
        EXPECT(box_clip(o, d, bmin, bmax, tn, tf) && tn == 2.0f && tf == 4.0f);
    }
    // zero components with the origin ON two slab planes: 0 * inf = NaN distances; whatever the reference's
    // min / max make of them, the clip returns and the march below ends
    {
        const float o[3] = { -3.0f, 1.0f, -1.0f }, d[3] = { 1.0f, 0.0f, 0.0f };
        (void)box_clip(o, d, bmin, bmax, tn, tf);
    }
    // parallel to a slab and outside it: a miss
    {
        const float o[3] = { -3.0f, 2.0f, 0.0f }, d[3] = { 1.0f, 0.0f, 0.0f };
        EXPECT(!box_clip(o, d, bmin, bmax, tn, tf));
    }
    // the box behind the eye is still clipped to a (negative) interval, as the reference does
    {
        const float o[3] = { 3.0f, 0.0f, 0.0f }, d[3] = { 1.0f, 0.0f, 0.0f };
        EXPECT(box_clip(o, d, bmin, bmax, tn, tf) && tn == -4.0f && tf == -2.0f);
    }

    std::vector<float> vox(8, 0.5f);
    std::vector<rgba_t> e(2, rgba_t{ 1.0f, 1.0f, 1.0f, 0.0f });      // transparent: never ends by the cutoff
    const uint32_t address[3] = { TEX_CLAMP, TEX_CLAMP, TEX_CLAMP };
    const vol_view v = make_vol_view(vox.data(), 2, 2, 2, VOL_R32F, TEX_LINEAR, address);
    const tf_view t = make_tf_view(e.data(), 2, TEX_LINEAR, TEX_CLAMP);
    march_params K{};
    for (int a = 0; a < 3; ++a) { K.bmin[a] = -1.0f; K.bmax[a] = 1.0f; K.sign[a] = 1.0f; K.offset[a] = 1.0f; K.extent[a] = 2.0f; }
    K.dt = 0.01f; K.cutoff = 0.999f;
    const float o[3] = { -3.0f, 0.0f, 0.0f }, d[3] = { 1.0f, 0.0f, 0.0f };
    rgba_t c;
    bool capped = true;
    K.cap = 2u * uint32_t(std::ceil(std::sqrt(12.0) / 0.01)) + 8u;
    uint32_t steps = march(v, t, t.entries, K, o, d, 2.0f, 4.0f, c, capped);
    EXPECT(!capped && steps >= 199 && steps <= 201 && c.w == 0.0f);
    K.cap = 17;
    steps = march(v, t, t.entries, K, o, d, 2.0f, 4.0f, c, capped);
    EXPECT(capped && steps == 17);
    // a step that does not advance t (never accepted by the host) ends at the limit instead of hanging
    K.dt = 0.0f;
    K.cap = 1000;
    steps = march(v, t, t.entries, K, o, d, 2.0f, 4.0f, c, capped);
    EXPECT(capped && steps == 1000);
    // NaN interval: no step at all
    steps = march(v, t, t.entries, K, o, d, NAN, 4.0f, c, capped);
    EXPECT(!capped && steps == 0 && c.x == 0.0f && c.w == 0.0f);
}

int main()
{
    const uint32_t sizes[][3] = { { 1, 1, 1 }, { 2, 2, 2 }, { 5, 7, 3 }, { 6, 4, 9 } };
    for (const auto& s : sizes)
    {
        check_volume<uint8_t>(VOL_R8, s[0], s[1], s[2], 0.0f, 1.0f);
        check_volume<uint16_t>(VOL_R16, s[0], s[1], s[2], 0.0f, 1.0f);
        check_volume<float>(VOL_R32F, s[0], s[1], s[2], 0.0f, 250.001f);
    }
    for (uint32_t n : { 1u, 2u, 4u, 37u }) check_transfunc(n);
    check_clip_and_cap();
    if (failures) { std::printf("volume_edge_check: %d failures\n", failures); return 1; }
    std::printf("volume_edge_check ok\n");
    return 0;
}
