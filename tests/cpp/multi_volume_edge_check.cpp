// tests/cpp/multi_volume_edge_check.cpp -- a stand-alone program over include/visionaray_hip/detail/vrh_multi_volume.h,
// built plain and with -fsanitize=address,undefined by tests/test_capi_multi_volume.py:
//   - the split samplers (mv_tex3d, mv_tex1d, mv_gradient) against tex3d / tex1d of vrh_volume.h, bit for bit,
//     over every format, filter and address mode, gradient coordinates outside [0, 1] included
//   - a direction component of 0 in volume space (infinite inverse, NaN through the reference's min / max)
//   - tmax == tmin, a ray that enters no box, 32 volumes, and the step limit
// The voxel arrays are exact-size heap blocks: a read outside them is an AddressSanitizer report.
#include "visionaray_hip/detail/vrh_multi_volume.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

using namespace vrh::dev;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static uint32_t rng_state = 12345u;
static float rnd() { rng_state = rng_state * 1664525u + 1013904223u; return float(rng_state >> 8) / 16777216.0f; }

struct volume_data
{
    std::unique_ptr<unsigned char[]> bytes;
    vol_view view;
    volume_data(uint32_t w, uint32_t h, uint32_t d, uint32_t fmt, uint32_t filter, const uint32_t address[3])
    {
        const size_t b = fmt == VOL_R8 ? 1 : fmt == VOL_R16 ? 2 : 4, n = size_t(w) * h * d;
        bytes.reset(new unsigned char[n * b]);
        for (size_t i = 0; i < n; ++i)
        {
            if (fmt == VOL_R8) bytes[i] = (unsigned char)(rnd() * 256.0f);
            else if (fmt == VOL_R16) { const uint16_t v = uint16_t(rnd() * 65536.0f); memcpy(&bytes[2 * i], &v, 2); }
            else { const float v = rnd(); memcpy(&bytes[4 * i], &v, 4); }
        }
        view = make_vol_view(bytes.get(), w, h, d, fmt, filter, address);
    }
};

template <uint32_t FMT>
static void check_samplers(const vol_view& v)
{
    const float special[] = { -1.5f, -0.01f, -0.0f, 0.0f, 0.005f, 0.5f, 0.995f, 1.0f, 1.01f, 2.5f };
    for (int k = 0; k < 400; ++k)
    {
        float tc[3];
        for (int a = 0; a < 3; ++a) tc[a] = k < 100 ? special[(k / (a == 0 ? 1 : a == 1 ? 10 : 3)) % 10] : rnd() * 3.0f - 1.0f;
        const float c1[1][3] = { { tc[0], tc[1], tc[2] } };
        float one;
        mv_tex3d<FMT, 1>(v, c1, &one);
        CHECK(bits(one) == bits(tex3d<FMT>(v, tc[0], tc[1], tc[2])));
        // the gradient against six calls of tex3d at the example's coordinates
        const float D = 0.01f;
        float g[3];
        mv_gradient<FMT>(v, tc, D, g);
        const float s1x = tex3d<FMT>(v, tc[0] - D, tc[1] - 0.0f, tc[2] - 0.0f), s2x = tex3d<FMT>(v, tc[0] + D, tc[1] + 0.0f, tc[2] + 0.0f);
        const float s1y = tex3d<FMT>(v, tc[0] + 0.0f, tc[1] + D, tc[2] + 0.0f), s2y = tex3d<FMT>(v, tc[0] - 0.0f, tc[1] - D, tc[2] - 0.0f);
        const float s1z = tex3d<FMT>(v, tc[0] + 0.0f, tc[1] + 0.0f, tc[2] + D), s2z = tex3d<FMT>(v, tc[0] - 0.0f, tc[1] - 0.0f, tc[2] - D);
        CHECK(bits(g[0]) == bits(s2x - s1x) && bits(g[1]) == bits(s2y - s1y) && bits(g[2]) == bits(s2z - s1z));
    }
}

static void samplers()
{
    const uint32_t dims[3][3] = { { 1, 1, 1 }, { 5, 7, 3 }, { 8, 8, 8 } };
    for (const auto& d : dims)
        for (uint32_t fmt = 0; fmt < 3; ++fmt)
            for (uint32_t filter = 0; filter < 2; ++filter)
                for (uint32_t mode = 0; mode < 3; ++mode)
                {
                    const uint32_t address[3] = { mode, (mode + 1) % 3, (mode + 2) % 3 };
                    const uint32_t same[3] = { mode, mode, mode };
                    for (const uint32_t* a : { address, same })
                    {
                        volume_data vol(d[0], d[1], d[2], fmt, filter, a);
                        if (fmt == VOL_R8) check_samplers<VOL_R8>(vol.view);
                        else if (fmt == VOL_R16) check_samplers<VOL_R16>(vol.view);
                        else check_samplers<VOL_R32F>(vol.view);
                    }
                }
    for (uint32_t n : { 1u, 2u, 5u, 64u })
        for (uint32_t filter = 0; filter < 2; ++filter)
            for (uint32_t mode = 0; mode < 3; ++mode)
            {
                std::unique_ptr<rgba_t[]> e(new rgba_t[n]);
                for (uint32_t i = 0; i < n; ++i) { e[i].x = rnd(); e[i].y = rnd(); e[i].z = rnd(); e[i].w = rnd(); }
                const tf_view t = make_tf_view(e.get(), n, filter, mode);
                for (int k = 0; k < 300; ++k)
                {
                    const float c = k == 0 ? 0.0f : k == 1 ? 1.0f : k == 2 ? -0.0f : rnd() * 3.0f - 1.0f;
                    const rgba_t a = mv_tex1d(t, c), b = tex1d(t, t.entries, c);
                    CHECK(bits(a.x) == bits(b.x) && bits(a.y) == bits(b.y) && bits(a.z) == bits(b.z) && bits(a.w) == bits(b.w));
                }
            }
}

// a frame's worth of records over one shared 4^3 float volume
struct scene
{
    std::unique_ptr<volume_data> vol;
    std::unique_ptr<rgba_t[]> tf;
    std::vector<mv_record> recs;
    mv_params K{};
    scene(uint32_t n, float alpha)
    {
        const uint32_t clamp[3] = { TEX_CLAMP, TEX_CLAMP, TEX_CLAMP };
        vol.reset(new volume_data(4, 4, 4, VOL_R32F, TEX_LINEAR, clamp));
        tf.reset(new rgba_t[4]);
        for (int i = 0; i < 4; ++i) { tf[i].x = 0.2f * float(i + 1); tf[i].y = 0.5f; tf[i].z = 0.7f; tf[i].w = alpha; }
        K.dt = 0.05f; K.cutoff = 0.999f; K.shade_alpha = 0.1f; K.delta = 0.01f;
        K.light_pos[0] = 1.0f; K.light_pos[1] = 2.0f; K.light_pos[2] = 9.0f;
        K.light_cl[0] = K.light_cl[1] = K.light_cl[2] = 1.0f; K.light_kl = 1.0f;
        K.light_att[0] = 1.0f; K.light_att[1] = 0.0f; K.light_att[2] = 0.0f;
        K.num = n; K.cap = 100000u;
        recs.assign(n, mv_record{});
        for (uint32_t i = 0; i < n; ++i)
        {
            mv_record& r = recs[i];
            r.vol = vol->view;
            r.tf = make_tf_view(tf.get(), 4, TEX_LINEAR, TEX_CLAMP);
            for (int a = 0; a < 4; ++a) r.minv[5 * a] = 1.0f;
            r.minv[12] = -0.01f * float(i);                          // volume i sits 0.01 i along x
            for (int a = 0; a < 3; ++a)
            {
                r.bmin[a] = -1.0f; r.bmax[a] = 1.0f;
                r.sign[a] = a == 0 ? 1.0f : -1.0f; r.offset[a] = 1.0f; r.extent[a] = 2.0f;
                r.ca[a] = 0.2f; r.cd[a] = 0.8f; r.cs[a] = 0.8f;
            }
            r.ka = r.kd = r.ks = 1.0f; r.exp = 32.0f;
            mv_light_dir(r.minv, K.light_pos, r.light_dir);
        }
    }
    mv_result march(const float ori[3], const float dir[3], bool active = true)
    {
        mv_array_ranges R;
        return multi_march<mv_single_ray>(recs.data(), K, ori, dir, active, R);
    }
};

static bool finite4(const rgba_t& c) { return std::isfinite(c.x) && std::isfinite(c.y) && std::isfinite(c.z) && std::isfinite(c.w); }

static void marches()
{
    {
        // axis-parallel rays: two direction components are 0 (the inverse infinite); with the origin on a slab
        // plane 0 * inf = NaN goes through the reference's min / max
        scene s(3, 0.3f);
        const float dirs[3][3] = { { 0.0f, 0.0f, -1.0f }, { 1.0f, 0.0f, 0.0f }, { 0.0f, -1.0f, -0.0f } };
        const float oris[5][3] = { { 0.1f, 0.2f, 5.0f }, { 1.0f, -1.0f, 5.0f }, { -5.0f, 1.0f, 1.0f }, { 1.0f, 5.0f, -1.0f },
                                   { 0.3f, 0.2f, 0.1f } };                 // the last one inside every box: a hit in every direction
        int hits = 0;
        for (const auto& d : dirs)
            for (const auto& o : oris)
            {
                const mv_result r = s.march(o, d);
                CHECK(finite4(r.color) && !r.capped && r.steps < 1000u);
                CHECK(r.hit ? r.steps > 0u : (r.steps == 0u && r.color.w == 0.0f));
                hits += r.hit ? 1 : 0;
            }
        CHECK(hits >= 4);
        // the shaded path ran and left a colour
        const float o[3] = { 0.1f, 0.2f, 5.0f }, d[3] = { 0.0f, 0.0f, -1.0f };
        const mv_result r = s.march(o, d);
        CHECK(r.hit && r.shaded > 0u && r.samples >= r.steps && r.color.w > 0.0f && r.tmin == 4.0f);
        // an inactive lane takes no step
        const mv_result off = s.march(o, d, false);
        CHECK(!off.hit && off.steps == 0u && off.color.w == 0.0f);
    }
    {
        // a ray that enters no box
        scene s(2, 0.3f);
        const float o[3] = { 0.0f, 5.0f, 5.0f }, d[3] = { 0.0f, 0.0f, -1.0f };
        const mv_result miss = s.march(o, d);
        CHECK(!miss.hit && miss.steps == 0u && miss.color.x == 0.0f && miss.color.w == 0.0f);
        const float n = 1.0f / std::sqrt(2.0f);
        const float o2[3] = { -3.0f, 0.0f, 1.0f }, d2[3] = { n, 0.0f, n };     // reaches x = -1 where z = 3 > 1
        CHECK(!s.march(o2, d2).hit);
        // tmax == tmin: a box of no thickness is hit (tfar >= tnear) at tnear == tfar == 5; no step, and hit = tmax > tmin is false
        scene flat(1, 0.3f);
        flat.recs[0].bmin[2] = flat.recs[0].bmax[2] = 0.0f;
        const float o3[3] = { 0.0f, 0.0f, 5.0f };
        const mv_result edge = flat.march(o3, d);
        CHECK(edge.steps == 0u && !edge.hit && edge.tmin == 5.0f && edge.color.w == 0.0f);
    }
    {
        // 32 volumes, every one sampled in a step
        scene s(MULTI_VOLUME_MAX, 0.01f);
        const float o[3] = { 0.5f, 0.1f, 5.0f }, d[3] = { 0.0f, 0.0f, -1.0f };
        const mv_result r = s.march(o, d);
        CHECK(r.hit && finite4(r.color) && r.samples == r.steps * MULTI_VOLUME_MAX && r.shaded == 0u);
    }
    {
        // the step limit stops a ray and says so
        scene s(1, 0.001f);
        s.K.cap = 7u;
        const float o[3] = { 0.0f, 0.0f, 5.0f }, d[3] = { 0.0f, 0.0f, -1.0f };
        const mv_result r = s.march(o, d);
        CHECK(r.capped && r.steps == 7u);
    }
}

int main()
{
    samplers();
    marches();
    if (failures) { printf("multi_volume_edge_check: %d checks failed\n", failures); return 1; }
    printf("multi_volume_edge_check ok\n");
    return 0;
}
