// include/visionaray_hip/detail/vrh_pixel.h -- the reference's pixel formats (pixel_format.h), its colour and
// depth conversions (detail/color_conversion.h:180-265, math/detail/unorm.inl:18-31), pixel_access::store / get /
// blend (detail/pixel_access.h) and depth_transform (detail/sched_common.h:339-354), restated once for host AND
// device code.  Used by the resolve kernel of formatted render targets (visionaray_amd/csrc/vrh_resolve.hip) and
// by vrh_rt_resolve_host (include/vrh.h).  Compile with -ffp-contract=off (and IEEE fp32 division / sqrt on
// the device), as everything that restates the reference.
//
// A formatted target's frame is rendered into RGBA32F staging colour, prim_id and t buffers; what is restated
// here takes one pixel of those to the formatted colour and depth buffers:
//   colour store from RGBA32F
//     RGBA8   per channel uint8(uint32(double(saturate(c)) * 255.0)) (truncation), 4 bytes r g b a
//     RGB8    rgb * a first, then the same conversion, 3 bytes, no padding
//     RGB32F  rgb * a, no clamp; 16-byte elements (the reference's vector<3, float> is 16 bytes: the fourth
//             word is unspecified there and written as 0 here)
//     RGBA32F copy
//   colour get (for blending): unorm -> float(double(float(u)) / 255.0); the RGB formats read alpha 1
//   depth   (z + 1) * 0.5 with p = proj * (view * (pos, 1)), z = p.z / p.w; 1.0 for a miss;
//           pos = ori + dir * t of the frame's own ray (the matrix camera's, restated below from vrh.h
//           vrh_view_camera as visionaray_amd/csrc/vrh_kernels.hip primary_ray has it)
//     DEPTH32F           the float
//     DEPTH24_STENCIL8   uint32(cvt(depth * 16777215.0f)) << 8, read as float((v & 0xFFFFFF00) >> 8) / 16777215.0f
//   blend   get, dst = src * s + dst * d per float channel (respectively in float depth), store: the
//           quantised intermediate is what the reference accumulates
// No float -> integer conversion here is undefined: saturate() maps NaN to 0, so the unorm conversion sees
// [0, 1]; cvt() is the saturating conversion the GPU's v_cvt_i32_f32 performs (NaN -> 0, below / above the
// int range -> INT_MIN / INT_MAX), written as compares, where the reference's plain cast is undefined.
#pragma once

#include "vrh_sampler.h"

#include <cstddef>
#include <cstdint>

#if defined(__HIP__)
#define VRH_PIXEL_FN __host__ __device__ inline
#else
#define VRH_PIXEL_FN inline
#endif

namespace vrh {
namespace dev {

constexpr uint32_t CF_RGBA32F = 0, CF_RGB32F = 1, CF_RGBA8 = 2, CF_RGB8 = 3;   // vrh_color_format
constexpr uint32_t DF_NONE = 0, DF_DEPTH32F = 1, DF_DEPTH24_STENCIL8 = 2;     // vrh_depth_format
constexpr uint32_t PIXEL_MISS = 0xFFFFFFFFu;                                   // prim_id of a miss

struct px4 { float x, y, z, w; };

// element i of an array of 16-byte pixels: one 16-byte access on the device (the arrays are 16-byte aligned
// there), a copy of any alignment on the host
VRH_PIXEL_FN px4 load4(const void* buf, size_t i)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const float4 v = static_cast<const float4*>(buf)[i];
    return px4{ v.x, v.y, v.z, v.w };
#else
    px4 v;
    __builtin_memcpy(&v, static_cast<const char*>(buf) + i * 16, 16);
    return v;
#endif
}
VRH_PIXEL_FN void store4(void* buf, size_t i, px4 v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    static_cast<float4*>(buf)[i] = make_float4(v.x, v.y, v.z, v.w);
#else
    __builtin_memcpy(static_cast<char*>(buf) + i * 16, &v, 16);
#endif
}

// bytes of one element of a colour / depth buffer
VRH_PIXEL_FN uint32_t color_bytes(uint32_t cf) { return cf == CF_RGBA8 ? 4u : cf == CF_RGB8 ? 3u : 16u; }
VRH_PIXEL_FN uint32_t depth_bytes(uint32_t df) { return df == DF_NONE ? 0u : 4u; }

// what a frame's resolve needs besides the buffers (vrh_resolve_desc with the box clipped and the inverses taken)
struct resolve_params
{
    uint32_t width, height;
    uint32_t clip[4];             // x0, y0, x1, y1: pixels x0 <= x < x1, y0 <= y < y1
    uint32_t blend;               // 0 store, 1 blend
    float s, d;
    uint32_t matrix_cam;          // 1: the depth is that of the matrix camera's ray at t; 0: the staging t holds the depth
    uint32_t jitter, frame_num;
    float px_off[2];
    float width_f, height_f;
    float view[16], proj[16];     // column-major
    float inv_view[16], inv_proj[16];
};

// ---- colour ----------------------------------------------------------------------------------------

// clamp(c, 0, 1); NaN -> 0
VRH_PIXEL_FN float saturate(float c) { return c > 0.0f ? (c < 1.0f ? c : 1.0f) : 0.0f; }

// unorm<8>(float) (unorm.inl:18-24) of an already clamped value, and back (:26-31)
VRH_PIXEL_FN uint32_t float_to_unorm8(float c) { return uint32_t(double(saturate(c)) * 255.0) & 0xFFu; }
VRH_PIXEL_FN float unorm8_to_float(uint32_t u) { return float(double(float(u)) / 255.0); }

VRH_PIXEL_FN uint32_t rgba8_pack(px4 c)
{
    return float_to_unorm8(c.x) | float_to_unorm8(c.y) << 8 | float_to_unorm8(c.z) << 16 | float_to_unorm8(c.w) << 24;
}
VRH_PIXEL_FN px4 rgba8_unpack(uint32_t v)
{
    return px4{ unorm8_to_float(v & 0xFFu), unorm8_to_float((v >> 8) & 0xFFu), unorm8_to_float((v >> 16) & 0xFFu),
                unorm8_to_float(v >> 24) };
}

// RGBA -> RGB: multiply by alpha (color_conversion.h:231-247)
VRH_PIXEL_FN px4 premultiply(px4 c) { return px4{ c.x * c.w, c.y * c.w, c.z * c.w, 0.0f }; }

// pixel_access::blend (pixel_access.h:1155-1175): dst = color * sfactor + dst * dfactor
VRH_PIXEL_FN px4 blend_color(px4 c, px4 dst, float s, float d)
{
    return px4{ c.x * s + dst.x * d, c.y * s + dst.y * d, c.z * s + dst.z * d, c.w * s + dst.w * d };
}

template <uint32_t CF>
VRH_PIXEL_FN px4 color_get(const void* buf, size_t i)
{
    if constexpr (CF == CF_RGBA32F) return load4(buf, i);
    else if constexpr (CF == CF_RGB32F)
    {
        const px4 v = load4(buf, i);
        return px4{ v.x, v.y, v.z, 1.0f };
    }
    else if constexpr (CF == CF_RGBA8) return rgba8_unpack(static_cast<const uint32_t*>(buf)[i]);
    else
    {
        const uint8_t* b = static_cast<const uint8_t*>(buf) + i * 3;
        return px4{ unorm8_to_float(b[0]), unorm8_to_float(b[1]), unorm8_to_float(b[2]), 1.0f };
    }
}

template <uint32_t CF>
VRH_PIXEL_FN void color_store(void* buf, size_t i, px4 c)
{
    if constexpr (CF == CF_RGBA32F) store4(buf, i, c);
    else if constexpr (CF == CF_RGB32F) store4(buf, i, premultiply(c));
    else if constexpr (CF == CF_RGBA8) static_cast<uint32_t*>(buf)[i] = rgba8_pack(c);
    else
    {
        const px4 m = premultiply(c);
        uint8_t* b = static_cast<uint8_t*>(buf) + i * 3;
        b[0] = uint8_t(float_to_unorm8(m.x));
        b[1] = uint8_t(float_to_unorm8(m.y));
        b[2] = uint8_t(float_to_unorm8(m.z));
    }
}

// ---- depth -----------------------------------------------------------------------------------------

// float -> int as the GPU converts: NaN -> 0, saturating at the ends of the int range
VRH_PIXEL_FN int32_t cvt(float f)
{
    if (!(f == f)) return 0;
    if (f >= 2147483648.0f) return 2147483647;
    if (f <= -2147483648.0f) return -2147483647 - 1;
    return int32_t(f);
}

VRH_PIXEL_FN uint32_t depth24_pack(float depth) { return uint32_t(cvt(depth * 16777215.0f)) << 8; }
VRH_PIXEL_FN float depth24_unpack(uint32_t v) { return float((v & 0xFFFFFF00u) >> 8) / 16777215.0f; }

template <uint32_t DF>
VRH_PIXEL_FN float depth_get(const void* buf, size_t i)
{
    if constexpr (DF == DF_DEPTH32F) return static_cast<const float*>(buf)[i];
    else return depth24_unpack(static_cast<const uint32_t*>(buf)[i]);
}

template <uint32_t DF>
VRH_PIXEL_FN void depth_store(void* buf, size_t i, float depth)
{
    if constexpr (DF == DF_DEPTH32F) static_cast<float*>(buf)[i] = depth;
    else static_cast<uint32_t*>(buf)[i] = depth24_pack(depth);
}

// m * v, column-major m, row by row, left to right (matrix4.inl:171-181)
VRH_PIXEL_FN void mat_vec(const float* m, const float* v, float* out)
{
    for (int r = 0; r < 4; ++r) out[r] = m[r] * v[0] + m[4 + r] * v[1] + m[8 + r] * v[2] + m[12 + r] * v[3];
}

// depth_transform (sched_common.h:339-354)
VRH_PIXEL_FN float depth_transform(const float pos[3], const float* view, const float* proj)
{
    const float p[4] = { pos[0], pos[1], pos[2], 1.0f };
    float e[4], c[4];
    mat_vec(view, p, e);
    mat_vec(proj, e, c);
    const float z = c[2] / c[3];
    return (z + 1.0f) * 0.5f;
}

// the matrix camera's ray of pixel (x, y) with the sampler's jitter / offset (vrh.h vrh_view_camera,
// vrh_pixel_sampler; sched_common.h:152-216)
VRH_PIXEL_FN void matrix_ray(const resolve_params& P, uint32_t x, uint32_t y, float ori[3], float dir[3])
{
    float fx = float(x), fy = float(y);
    if (P.jitter)
    {
        const uint32_t k = (y * P.width + x) * 2u + 0x632BE5ABu + P.frame_num * 0x68E31DA4u;
        fy = fy + (uniform01(k) - 0.5f);
        fx = fx + (uniform01(k + 1u) - 0.5f);
    }
    else
    {
        fx = fx + P.px_off[0];
        fy = fy + P.px_off[1];
    }
    const float u = 2.0f * (fx + 0.5f) / P.width_f - 1.0f;
    const float v = 2.0f * (fy + 0.5f) / P.height_f - 1.0f;
    const float* iv = P.inv_view;
    const float* ip = P.inv_proj;
    float a[4], b[4], o[4], d[4];
    for (int r = 0; r < 4; ++r)
    {
        a[r] = ip[r] * u + ip[4 + r] * v + ip[8 + r] * -1.0f + ip[12 + r] * 1.0f;
        b[r] = ip[r] * u + ip[4 + r] * v + ip[8 + r] * 1.0f + ip[12 + r] * 1.0f;
    }
    mat_vec(iv, a, o);
    mat_vec(iv, b, d);
    float far[3];
    for (int i = 0; i < 3; ++i)
    {
        ori[i] = o[i] / o[3];
        far[i] = d[i] / d[3] - ori[i];
    }
    // normalize (vector3.inl:331-336): v * (1 / sqrt(dot(v, v)))
    const float inv = 1.0f / __builtin_sqrtf(far[0] * far[0] + far[1] * far[1] + far[2] * far[2]);
    for (int i = 0; i < 3; ++i) dir[i] = far[i] * inv;
}

// the depth a frame of the matrix camera stores at pixel (x, y): result.depth = hit ? depth_transform(isect_pos) : 1
// (sched_common.h:425) with isect_pos = ori + dir * t
VRH_PIXEL_FN float pixel_depth(const resolve_params& P, uint32_t x, uint32_t y, uint32_t prim_id, float t)
{
    if (prim_id == PIXEL_MISS) return 1.0f;
    float ori[3], dir[3];
    matrix_ray(P, x, y, ori, dir);
    const float pos[3] = { ori[0] + dir[0] * t, ori[1] + dir[1] * t, ori[2] + dir[2] * t };
    return depth_transform(pos, P.view, P.proj);
}

// the depth of pixel (x, y), linear index i, of the staged frame: a built-in kernel's frame leaves prim_id and t, and
// the depth is the matrix camera's; a user kernel's launch (visionaray_hip/hip_kernels.h) leaves result.depth itself
// in the t buffer (matrix_cam 0), prim_id is then not read
VRH_PIXEL_FN float staged_depth(const resolve_params& P, uint32_t x, uint32_t y, size_t i, const uint32_t* prim_id, const float* t)
{
    return P.matrix_cam ? pixel_depth(P, x, y, prim_id[i], t[i]) : t[i];
}

// ---- one pixel -------------------------------------------------------------------------------------

// pixel_access::store / blend of pixel (x, y), linear index i, into the formatted buffers
template <uint32_t CF, uint32_t DF, bool BLEND>
VRH_PIXEL_FN void resolve_pixel(const resolve_params& P, uint32_t x, uint32_t y, size_t i, px4 c, const uint32_t* prim_id,
                                const float* t, void* color_out, void* depth_out)
{
    if constexpr (BLEND) c = blend_color(c, color_get<CF>(color_out, i), P.s, P.d);
    color_store<CF>(color_out, i, c);
    if constexpr (DF != DF_NONE)
    {
        float depth = staged_depth(P, x, y, i, prim_id, t);
        if constexpr (BLEND) depth = depth * P.s + depth_get<DF>(depth_out, i) * P.d;
        depth_store<DF>(depth_out, i, depth);
    }
}

// ---- the host twin ---------------------------------------------------------------------------------

// the resolve pass on the host: the same per-pixel text over the box P.clip (which must lie inside the image);
// color: width * height RGBA32F, prim_id / t: read with a depth format only
template <uint32_t CF, uint32_t DF, bool BLEND>
inline void resolve_host_loop(const resolve_params& P, const float* color, const uint32_t* prim_id, const float* t,
                              void* color_out, void* depth_out)
{
    for (uint32_t y = P.clip[1]; y < P.clip[3]; ++y)
        for (uint32_t x = P.clip[0]; x < P.clip[2]; ++x)
        {
            const size_t i = size_t(y) * P.width + x;
            resolve_pixel<CF, DF, BLEND>(P, x, y, i, load4(color, i), prim_id, t, color_out, depth_out);
        }
}

template <uint32_t CF>
inline void resolve_host_cf(uint32_t df, const resolve_params& P, const float* color, const uint32_t* prim_id, const float* t,
                            void* color_out, void* depth_out)
{
    if (df == DF_NONE)
    {
        if (P.blend) resolve_host_loop<CF, DF_NONE, true>(P, color, prim_id, t, color_out, depth_out);
        else resolve_host_loop<CF, DF_NONE, false>(P, color, prim_id, t, color_out, depth_out);
    }
    else if (df == DF_DEPTH32F)
    {
        if (P.blend) resolve_host_loop<CF, DF_DEPTH32F, true>(P, color, prim_id, t, color_out, depth_out);
        else resolve_host_loop<CF, DF_DEPTH32F, false>(P, color, prim_id, t, color_out, depth_out);
    }
    else
    {
        if (P.blend) resolve_host_loop<CF, DF_DEPTH24_STENCIL8, true>(P, color, prim_id, t, color_out, depth_out);
        else resolve_host_loop<CF, DF_DEPTH24_STENCIL8, false>(P, color, prim_id, t, color_out, depth_out);
    }
}

inline void resolve_host(uint32_t cf, uint32_t df, const resolve_params& P, const float* color, const uint32_t* prim_id,
                         const float* t, void* color_out, void* depth_out)
{
    if (cf == CF_RGBA32F) resolve_host_cf<CF_RGBA32F>(df, P, color, prim_id, t, color_out, depth_out);
    else if (cf == CF_RGB32F) resolve_host_cf<CF_RGB32F>(df, P, color, prim_id, t, color_out, depth_out);
    else if (cf == CF_RGBA8) resolve_host_cf<CF_RGBA8>(df, P, color, prim_id, t, color_out, depth_out);
    else resolve_host_cf<CF_RGB8>(df, P, color, prim_id, t, color_out, depth_out);
}

} // namespace dev
} // namespace vrh
