// include/visionaray_hip/detail/vrh_texture.h -- the reference's tex2D for texture<vector<4, unorm<8>>, 2>
// (the model's diffuse maps, src/common/model.h:29), restated once for host AND device code.  Used by the
// built-in shading kernels (vrh_shade.h), by vrh_tex2d_host (include/vrh.h) and callable from user kernels
// (hip_kernels.h) on a tex_view.  Compile with -ffp-contract=off, as everything that restates the reference.
//
// tex2D (texture/detail/sampler2d.h:88-127): the texels enter the filter as integers 0..255, the filter
// interpolates in float, its result goes back to int by truncation, and only then is it normalised with
// unorm_to_float<8> (math/detail/unorm.inl:28-31).  A sample is therefore one of 256 values per channel:
// tex2d() returns it packed as one RGBA8 dword (r in the low byte), unorm8() is the normalisation.
//   nearest (filter/nearest.h:51-73):  c = map(coord); lo = int(c * float(size)); texel lo.y * W + lo.x
//   linear  (filter/linear.h:72-118):  c1 = map(coord - 0.5f / float(size)), c2 = map(coord + 0.5f / float(size));
//       lo = int(c1 * size), hi = int(c2 * size); texels (lo.x, lo.y) (hi.x, lo.y) (lo.x, hi.y) (hi.x, hi.y);
//       uv = c1 * size - float(lo); lerp(a, b, x) = (1 - x) * a + x * b along x for both rows, then along y
//   map, per axis (filter/common.h:27-50): Wrap c - floor(c); Mirror float(N - 1) / float(N) - (c - floor(c))
//       where int(floor(c)) is odd, else c - floor(c); Clamp max(0, min(c, 1 - 1 / float(N)))
// A Wrap coordinate just below an integer maps to exactly 1.0, and the reference then reads texel N of
// that axis: in x the next row's first texel (reproduced: the same linear index), in y -- or past the last
// row -- outside the array (undefined there).  Here the final linear index is clamped into [0, W * H - 1],
// so nothing outside the array is ever read.
// Coordinates must be finite and at most 2^20 in magnitude, sizes at most 32768: every float -> int
// conversion is then defined (vrh_shading_set_textures and vrh_tex2d_host refuse anything else).
#pragma once

#include <cstdint>

#if defined(__HIP__)
#define VRH_TEX_FN __host__ __device__ inline
#else
#define VRH_TEX_FN inline
#endif

namespace vrh {
namespace dev {

constexpr uint32_t TEX_NEAREST = 0, TEX_LINEAR = 1;            // vrh_texture_filter
constexpr uint32_t TEX_WRAP = 0, TEX_MIRROR = 1, TEX_CLAMP = 2; // vrh_texture_address
constexpr uint32_t TEX_MAX_DIM = 32768u;
constexpr float TEX_MAX_COORD = 1048576.0f;                    // 2^20

// A texture as the sampler sees it: 32 bytes, one load.  The per-axis constants are computed once on the
// host (make_tex_view) with the IEEE operations of the reference; float(N) is the conversion of the size
// itself, exact on both sides.  pixels == nullptr or a zero size: the reference's dummy texture, whose
// colour is 1 (get_surface.h:443-445).
struct __attribute__((aligned(16))) tex_view
{
    const uint32_t* pixels;   // W x H packed RGBA8, rows in order, r in the low byte
    uint32_t dims;            // W | H << 16 (H <= 32768 fits 16 bits)
    uint32_t modes;           // filter | address[0] << 8 | address[1] << 16
    float half[2];            // 0.5f / float(N)
    float aux[2];             // Clamp: 1.0f - 1.0f / float(N); Mirror: float(N - 1) / float(N); Wrap: 0
};
static_assert(sizeof(tex_view) == 32, "a texture descriptor is one 32-byte load");

inline tex_view make_tex_view(const uint32_t* pixels, uint32_t w, uint32_t h, uint32_t filter, uint32_t ax, uint32_t ay)
{
    tex_view t{};
    t.pixels = (w && h) ? pixels : nullptr;
    t.dims = w | h << 16;
    t.modes = filter | ax << 8 | ay << 16;
    const uint32_t n[2] = { w, h }, a[2] = { ax, ay };
    for (int d = 0; d < 2; ++d)
    {
        if (!n[d]) continue;
        const float N = float(int(n[d]));
        t.half[d] = 0.5f / N;
        t.aux[d] = a[d] == TEX_CLAMP ? 1.0f - 1.0f / N : a[d] == TEX_MIRROR ? float(int(n[d]) - 1) / N : 0.0f;
    }
    return t;
}

// map_tex_coord (filter/common.h:27-50) of one axis
VRH_TEX_FN float tex_map(float c, uint32_t mode, float aux)
{
    if (mode == TEX_CLAMP)
    {
        const float m = c < aux ? c : aux;          // min(x, b)
        return 0.0f < m ? m : 0.0f;                 // max(a, y)
    }
    const float fl = __builtin_floorf(c);
    const float fr = c - fl;
    if (mode == TEX_MIRROR && (int(fl) & 1) == 1) return aux - fr;
    return fr;
}

// unorm_to_float<8> (math/detail/unorm.inl:28-31): float(double(float(k)) / 255.0), as a table
struct unorm8_table
{
    float v[256];
    constexpr unorm8_table() : v{}
    {
        for (int k = 0; k < 256; ++k) v[k] = float(double(float(k)) / 255.0);
    }
};
VRH_TEX_FN float unorm8(uint32_t k)
{
    static constexpr unorm8_table T{};
    return T.v[k & 255u];
}

VRH_TEX_FN int tex_index(int x, int y, int w, int last)
{
    const int i = y * w + x;                        // index(x, y, texsize), filter/common.h:72-75
    return i < 0 ? 0 : i > last ? last : i;         // never outside the array
}

// (1 - x) * a + x * b over the four channels of two packed texels, as floats
VRH_TEX_FN void tex_lerp4(float out[4], const float a[4], const float b[4], float x)
{
    for (int c = 0; c < 4; ++c) out[c] = (1.0f - x) * a[c] + x * b[c];
}
VRH_TEX_FN void tex_unpack(float out[4], uint32_t p)
{
    for (int c = 0; c < 4; ++c) out[c] = float(int((p >> (8 * c)) & 255u));
}

// tex2D(tex, coord) before its normalisation: the packed RGBA8 sample.  The view must not be a dummy.
VRH_TEX_FN uint32_t tex2d(const tex_view& t, float cx, float cy)
{
    const int w = int(t.dims & 0xFFFFu), h = int(t.dims >> 16);
    const float wf = float(w), hf = float(h);
    const uint32_t ax = (t.modes >> 8) & 255u, ay = (t.modes >> 16) & 255u;
    const int last = w * h - 1;
    if ((t.modes & 255u) == TEX_NEAREST)
    {
        const float mx = tex_map(cx, ax, t.aux[0]), my = tex_map(cy, ay, t.aux[1]);
        const int lx = int(mx * wf), ly = int(my * hf);
        return t.pixels[tex_index(lx, ly, w, last)];
    }
    const float c1x = tex_map(cx - t.half[0], ax, t.aux[0]), c1y = tex_map(cy - t.half[1], ay, t.aux[1]);
    const float c2x = tex_map(cx + t.half[0], ax, t.aux[0]), c2y = tex_map(cy + t.half[1], ay, t.aux[1]);
    const int lx = int(c1x * wf), ly = int(c1y * hf), hx = int(c2x * wf), hy = int(c2y * hf);
    // the four texel loads are issued together, before the first use
    const uint32_t p0 = t.pixels[tex_index(lx, ly, w, last)], p1 = t.pixels[tex_index(hx, ly, w, last)];
    const uint32_t p2 = t.pixels[tex_index(lx, hy, w, last)], p3 = t.pixels[tex_index(hx, hy, w, last)];
    const float ux = c1x * wf - float(lx), uy = c1y * hf - float(ly);
    float s0[4], s1[4], s2[4], s3[4], r1[4], r2[4], r[4];
    tex_unpack(s0, p0); tex_unpack(s1, p1); tex_unpack(s2, p2); tex_unpack(s3, p3);
    tex_lerp4(r1, s0, s1, ux);
    tex_lerp4(r2, s2, s3, ux);
    tex_lerp4(r, r1, r2, uy);
    uint32_t out = 0;
    for (int c = 0; c < 4; ++c) out |= (uint32_t(int(r[c])) & 255u) << (8 * c);
    return out;
}

// get_tex_coord (get_tex_coord.h:23-39) = lerp(a, b, c, u, v) of math.h:466-475, one component
VRH_TEX_FN float tex_coord_lerp(float a, float b, float c, float u, float v)
{
    const float s2 = c * v;
    const float s3 = b * u;
    const float s1 = a * (1.0f - (u + v));
    return (s1 + s2) + s3;
}

} // namespace dev
} // namespace vrh
