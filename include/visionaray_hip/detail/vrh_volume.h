// include/visionaray_hip/detail/vrh_volume.h -- the reference's volume rendering example
// (src/examples/volume/main.cpp:123-167), restated once for host AND device code: tex3D of a scalar volume,
// tex1D of an RGBA transfer function, the ray / box clip and the front-to-back march.  Used by the volume
// kernel (visionaray_amd/csrc/vrh_volume.hip) and by vrh_tex3d_host / vrh_tex1d_host / vrh_volume_render_host
// (include/vrh.h).  Compile with -ffp-contract=off (and IEEE fp32 division on the device), as everything
// that restates the reference.  The whole algorithm calls neither powf nor sinf / cosf: every result is
// the reference's bit for bit.
//
// tex3D (texture/detail/sampler3d.h, filter/nearest.h:80-102, filter/linear.h:125-180, filter/common.h):
//   per axis the map_tex_coord of vrh_texture.h (tex_map); texel index z * W * H + y * W + x
//   nearest: c = map(coord); lo = int(c * float(size)); texel index(lo)
//   linear:  c1 = map(coord - 0.5f / float(size)), c2 = map(coord + 0.5f / float(size)); lo = int(c1 * size),
//            hi = int(c2 * size); the eight texels (lo.x lo.y lo.z) (hi.x lo.y lo.z) (lo.x hi.y lo.z)
//            (hi.x hi.y lo.z) (lo.x lo.y hi.z) (hi.x lo.y hi.z) (lo.x hi.y hi.z) (hi.x hi.y hi.z);
//            uvw = c1 * size - float(lo); lerp(a, b, x) = (1 - x) * a + x * b along x four times, along y
//            twice, along z once
//   float texels are filtered in float and returned as they are.  unorm<8> / unorm<16> texels enter as
//   integers, are filtered in float, truncated to int, and only then normalised with unorm_to_float<Bits>
//   = float(double(float(k)) / double(2^Bits - 1)) (math/detail/unorm.inl:26-31).
// tex1D (texture/detail/sampler1d.h, filter/nearest.h:31-44, filter/linear.h:24-65) on vector<4, float>
//   texels: the same with one axis, two texels and one lerp per channel.
// As in vrh_texture.h a Wrap coordinate that maps to exactly 1.0 gives index N of its axis: the reference's
// linear index is computed as it stands and then clamped into [0, count - 1], so nothing outside the
// arrays is ever read.
#pragma once

#include "vrh_texture.h"

namespace vrh {
namespace dev {

constexpr uint32_t VOL_R8 = 0, VOL_R16 = 1, VOL_R32F = 2;   // vrh_volume_format
constexpr uint32_t VOLUME_MAX_STEPS = 65536u;               // VRH_VOLUME_MAX_STEPS

struct __attribute__((aligned(16))) rgba_t { float x, y, z, w; };

// A volume as the sampler sees it.  The per-axis constants are computed once on the host (make_vol_view)
// with the IEEE operations of the reference.
struct __attribute__((aligned(16))) vol_view
{
    const void* voxels;       // W x H x D voxels of `format`, x fastest
    uint32_t format;          // VOL_R8 / VOL_R16 / VOL_R32F
    uint32_t modes;           // filter | address[0] << 8 | address[1] << 16 | address[2] << 24
    int32_t dims[3];          // W, H, D
    int32_t last;             // W * H * D - 1
    float size[3];            // float(N)
    float half[3];            // 0.5f / float(N)
    float aux[3];             // Clamp: 1.0f - 1.0f / float(N); Mirror: float(N - 1) / float(N); Wrap: 0
};

// A transfer function: `size` RGBA32F entries
struct __attribute__((aligned(16))) tf_view
{
    const rgba_t* entries;
    int32_t size;
    uint32_t modes;           // filter | address << 8
    float sizef, half, aux;
    uint32_t pad;
};

inline void tex_axis_constants(uint32_t n, uint32_t address, float& sizef, float& half, float& aux)
{
    const float N = float(int(n));
    sizef = N;
    half = 0.5f / N;
    aux = address == TEX_CLAMP ? 1.0f - 1.0f / N : address == TEX_MIRROR ? float(int(n) - 1) / N : 0.0f;
}

inline vol_view make_vol_view(const void* voxels, uint32_t w, uint32_t h, uint32_t d, uint32_t format, uint32_t filter,
                              const uint32_t address[3])
{
    vol_view v{};
    v.voxels = voxels;
    v.format = format;
    v.modes = filter | address[0] << 8 | address[1] << 16 | address[2] << 24;
    const uint32_t n[3] = { w, h, d };
    for (int a = 0; a < 3; ++a)
    {
        v.dims[a] = int32_t(n[a]);
        tex_axis_constants(n[a], address[a], v.size[a], v.half[a], v.aux[a]);
    }
    v.last = int32_t(w * h * d) - 1;
    return v;
}

inline tf_view make_tf_view(const rgba_t* entries, uint32_t size, uint32_t filter, uint32_t address)
{
    tf_view t{};
    t.entries = entries;
    t.size = int32_t(size);
    t.modes = filter | address << 8;
    tex_axis_constants(size, address, t.sizef, t.half, t.aux);
    return t;
}

// unorm_to_float<Bits> (math/detail/unorm.inl:26-31) for Bits = 8 (maxv 255.0) and 16 (65535.0): the
// reference's own expression, a double division that IEEE hardware rounds the same way everywhere
VRH_TEX_FN float unorm_to_float(int k, double maxv)
{
    return float(double(float(uint32_t(k))) / maxv);
}

template <uint32_t FMT>
VRH_TEX_FN float vol_texel(const vol_view& v, int i)
{
    if (FMT == VOL_R8) return float(int(static_cast<const uint8_t*>(v.voxels)[i]));
    if (FMT == VOL_R16) return float(int(static_cast<const uint16_t*>(v.voxels)[i]));
    return static_cast<const float*>(v.voxels)[i];
}

VRH_TEX_FN int vol_index(const vol_view& v, int x, int y, int z)
{
    const int i = z * v.dims[0] * v.dims[1] + y * v.dims[0] + x;   // index(x, y, z, texsize), filter/common.h
    return i < 0 ? 0 : i > v.last ? v.last : i;                     // never outside the array
}

template <uint32_t FMT>
VRH_TEX_FN float vol_finish(float s)
{
    if (FMT == VOL_R8) return unorm_to_float(int(s), 255.0);
    if (FMT == VOL_R16) return unorm_to_float(int(s), 65535.0);
    return s;
}

VRH_TEX_FN float tex_lerp(float a, float b, float x) { return (1.0f - x) * a + x * b; }

// tex3D(volume, coord) for voxels of format FMT
template <uint32_t FMT>
VRH_TEX_FN float tex3d(const vol_view& v, float cx, float cy, float cz)
{
    const uint32_t ax = (v.modes >> 8) & 255u, ay = (v.modes >> 16) & 255u, az = v.modes >> 24;
    if ((v.modes & 255u) == TEX_NEAREST)
    {
        const float mx = tex_map(cx, ax, v.aux[0]), my = tex_map(cy, ay, v.aux[1]), mz = tex_map(cz, az, v.aux[2]);
        const int lx = int(mx * v.size[0]), ly = int(my * v.size[1]), lz = int(mz * v.size[2]);
        // nearest returns the texel itself: an integer for the unorm formats
        return vol_finish<FMT>(vol_texel<FMT>(v, vol_index(v, lx, ly, lz)));
    }
    const float c1x = tex_map(cx - v.half[0], ax, v.aux[0]), c2x = tex_map(cx + v.half[0], ax, v.aux[0]);
    const float c1y = tex_map(cy - v.half[1], ay, v.aux[1]), c2y = tex_map(cy + v.half[1], ay, v.aux[1]);
    const float c1z = tex_map(cz - v.half[2], az, v.aux[2]), c2z = tex_map(cz + v.half[2], az, v.aux[2]);
    const int lx = int(c1x * v.size[0]), ly = int(c1y * v.size[1]), lz = int(c1z * v.size[2]);
    const int hx = int(c2x * v.size[0]), hy = int(c2y * v.size[1]), hz = int(c2z * v.size[2]);
    // the eight voxel loads are issued together, before the first use
    const float s0 = vol_texel<FMT>(v, vol_index(v, lx, ly, lz)), s1 = vol_texel<FMT>(v, vol_index(v, hx, ly, lz));
    const float s2 = vol_texel<FMT>(v, vol_index(v, lx, hy, lz)), s3 = vol_texel<FMT>(v, vol_index(v, hx, hy, lz));
    const float s4 = vol_texel<FMT>(v, vol_index(v, lx, ly, hz)), s5 = vol_texel<FMT>(v, vol_index(v, hx, ly, hz));
    const float s6 = vol_texel<FMT>(v, vol_index(v, lx, hy, hz)), s7 = vol_texel<FMT>(v, vol_index(v, hx, hy, hz));
    const float ux = c1x * v.size[0] - float(lx), uy = c1y * v.size[1] - float(ly), uz = c1z * v.size[2] - float(lz);
    const float p1 = tex_lerp(s0, s1, ux), p2 = tex_lerp(s2, s3, ux), p3 = tex_lerp(s4, s5, ux), p4 = tex_lerp(s6, s7, ux);
    const float p12 = tex_lerp(p1, p2, uy), p34 = tex_lerp(p3, p4, uy);
    return vol_finish<FMT>(tex_lerp(p12, p34, uz));
}

// the format as a run-time value (host entry points, user kernels)
VRH_TEX_FN float tex3d(const vol_view& v, float cx, float cy, float cz)
{
    return v.format == VOL_R8 ? tex3d<VOL_R8>(v, cx, cy, cz)
         : v.format == VOL_R16 ? tex3d<VOL_R16>(v, cx, cy, cz) : tex3d<VOL_R32F>(v, cx, cy, cz);
}

VRH_TEX_FN int tf_index(const tf_view& t, int i) { return i < 0 ? 0 : i >= t.size ? t.size - 1 : i; }

// tex1D(transfunc, coord); `entries` are the view's entries or a copy of them (the kernel's LDS stage)
VRH_TEX_FN rgba_t tex1d(const tf_view& t, const rgba_t* entries, float c)
{
    const uint32_t a = (t.modes >> 8) & 255u;
    if ((t.modes & 255u) == TEX_NEAREST)
    {
        const float m = tex_map(c, a, t.aux);
        return entries[tf_index(t, int(m * t.sizef))];
    }
    const float c1 = tex_map(c - t.half, a, t.aux), c2 = tex_map(c + t.half, a, t.aux);
    const int lo = int(c1 * t.sizef), hi = int(c2 * t.sizef);
    const rgba_t e0 = entries[tf_index(t, lo)], e1 = entries[tf_index(t, hi)];
    const float u = c1 * t.sizef - float(lo);
    rgba_t r;
    r.x = tex_lerp(e0.x, e1.x, u); r.y = tex_lerp(e0.y, e1.y, u);
    r.z = tex_lerp(e0.z, e1.z, u); r.w = tex_lerp(e0.w, e1.w, u);
    return r;
}

// the reference's scalar min / max (math/detail/math.h:50-60) with their own NaN behaviour
VRH_TEX_FN float ref_min(float x, float y) { return x < y ? x : y; }
VRH_TEX_FN float ref_max(float x, float y) { return x < y ? y : x; }

// intersect(ray, aabb) (math/intersect.h:54-81): hit = tfar >= tnear
VRH_TEX_FN bool box_clip(const float ori[3], const float dir[3], const float bmin[3], const float bmax[3],
                         float& tnear, float& tfar)
{
    float t1[3], t2[3];
    for (int d = 0; d < 3; ++d)
    {
        const float inv = 1.0f / dir[d];
        t1[d] = (bmin[d] - ori[d]) * inv;
        t2[d] = (bmax[d] - ori[d]) * inv;
    }
    // min_max(x, y, z) = max(min(x, y), z), max_min(x, y, z) = min(max(x, y), z)
    tnear = ref_max(ref_min(t1[0], t2[0]), ref_max(ref_min(t1[1], t2[1]), ref_min(t1[2], t2[2])));
    tfar = ref_min(ref_max(t1[0], t2[0]), ref_min(ref_max(t1[1], t2[1]), ref_max(t1[2], t2[2])));
    return tfar >= tnear;
}

// the parameters of the march: tc[d] = (sign[d] * pos[d] + offset[d]) / extent[d], sign +-1
struct march_params
{
    float bmin[3], bmax[3];
    float sign[3], offset[3], extent[3];
    float dt, cutoff;
    uint32_t cap;             // hard step limit, 2 * ceil(diagonal / dt) + 8
};

// The example's loop (volume/main.cpp:127-165): from tnear in steps of dt while t < tfar; each step samples
// the volume, classifies the voxel through the transfer function, premultiplies and composites front to
// back; it ends early once the opacity reaches the cutoff.  Returns the steps taken; `capped` is set
// if the loop was stopped by the step limit.
template <uint32_t FMT>
VRH_TEX_FN uint32_t march(const vol_view& vol, const tf_view& tf, const rgba_t* entries, const march_params& K,
                          const float ori[3], const float dir[3], float tnear, float tfar, rgba_t& color, bool& capped)
{
    color.x = color.y = color.z = color.w = 0.0f;
    capped = false;
    uint32_t steps = 0;
    float t = tnear;
    while (t < tfar)
    {
        if (steps >= K.cap) { capped = true; break; }
        ++steps;
        float tc[3];
        for (int d = 0; d < 3; ++d) tc[d] = (K.sign[d] * (ori[d] + dir[d] * t) + K.offset[d]) / K.extent[d];
        const float voxel = tex3d<FMT>(vol, tc[0], tc[1], tc[2]);
        rgba_t c = tex1d(tf, entries, voxel);
        c.x *= c.w; c.y *= c.w; c.z *= c.w;
        const float s = 1.0f - color.w;
        color.x += c.x * s; color.y += c.y * s; color.z += c.z * s; color.w += c.w * s;
        if (color.w >= K.cutoff) break;
        t += K.dt;
    }
    return steps;
}

VRH_TEX_FN uint32_t march(const vol_view& vol, const tf_view& tf, const rgba_t* entries, const march_params& K,
                          const float ori[3], const float dir[3], float tnear, float tfar, rgba_t& color, bool& capped)
{
    return vol.format == VOL_R8 ? march<VOL_R8>(vol, tf, entries, K, ori, dir, tnear, tfar, color, capped)
         : vol.format == VOL_R16 ? march<VOL_R16>(vol, tf, entries, K, ori, dir, tnear, tfar, color, capped)
                                 : march<VOL_R32F>(vol, tf, entries, K, ori, dir, tnear, tfar, color, capped);
}

// the primary ray of pixel (x, y) as vrh_render generates it for the uniform sampler
// (sched_common.h:130-150): u = 2 (x + 0.5) / W - 1, dir = normalize((cam_u u + cam_v v) + cam_w)
VRH_TEX_FN void pinhole_dir(float dir[3], const float cu[3], const float cv[3], const float cw[3], uint32_t x, uint32_t y,
                            float wf, float hf)
{
    const float u = 2.0f * (float(x) + 0.5f) / wf - 1.0f;
    const float v = 2.0f * (float(y) + 0.5f) / hf - 1.0f;
    float d[3];
    for (int a = 0; a < 3; ++a) d[a] = (cu[a] * u + cv[a] * v) + cw[a];
    const float n = 1.0f / __builtin_sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    for (int a = 0; a < 3; ++a) dir[a] = d[a] * n;
}

} // namespace dev
} // namespace vrh
