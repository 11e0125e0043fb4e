// include/visionaray_hip/detail/vrh_multi_volume.h -- the reference's multi-volume example
// (src/examples/multi_volume/main.cpp:410-567), restated once for host AND device code over the samplers,
// the box clip and tex_lerp of vrh_volume.h.  Used by the multi-volume kernel
// (visionaray_amd/csrc/vrh_multi_volume.hip) and by vrh_multi_volume_render_host (include/vrh.h).  Compile with
// -ffp-contract=off (and IEEE fp32 division / sqrt on the device), as everything that restates the reference.
//
// Up to 32 volumes, each with its own box, inverse model transform, transfer function and plastic material,
// are marched along one ray in lock-step: t runs from the smallest tnear to the largest tfar of the boxes
// that were hit; a step samples every volume whose own [tnear, tfar) holds t, adds the premultiplied samples
// and composites the sum front to back.  A sample whose alpha reaches shade_alpha is shaded: six more tex3D
// fetches give a central-difference gradient, and where that is not 0 the sample's rgb is multiplied by
// plastic::shade for one point light (normal = normalize(gradient), isect_pos = the volume-space position,
// view_dir = -ray.dir in world space, light_dir = normalize(Minv * light position): the example's own mix of
// spaces, kept).  Shading multiplies rgb only: alpha, the number of steps, hit and tmin never depend on powf
// and are the reference's bit for bit; rgb is the reference's up to the last-bit freedom of powf.
//
//   matrix<4, 4> * vector<4> (math/detail/matrix4.inl:171-181): row r = ((m(r,0) x + m(r,1) y) + m(r,2) z) + m(r,3) w,
//     w = 1 for positions, 0 for directions (the product by w is formed: it decides the sign of a zero)
//   gradient (multi_volume/main.cpp:91-108): s1.x at -delta, s2.x at +delta, s1.y at +delta, s2.y at -delta,
//     s1.z at +delta, s2.z at -delta, every other component of the coordinate -+ 0.0f; grad = s2 - s1
//   plastic::shade (detail/material/plastic.inl:21-37) with the shade record's light_dir, lambertian::f and
//     blinn::f (brdf.h:36-41, 111-126), point_light::intensity (detail/point_light.inl:12-28)
//
// The loop is written once over two policies.  `Wave` says whether any lane of the wave holds a condition (the
// host: the ray itself): the loop runs while any lane has t < tmax, and a volume is skipped where no lane is
// inside it, so the index of the volume records stays uniform over the wave; a lane applies the reference's
// own per-lane tests, so this changes no bits.  `Ranges` keeps the 2 * num_volumes floats tnear / tfar of a ray
// (the host: an array; the kernel: a column of LDS).
#pragma once

#include "vrh_volume.h"

#if !defined(__HIP_DEVICE_COMPILE__)
#include <cmath>
#endif

namespace vrh {
namespace dev {

constexpr uint32_t MULTI_VOLUME_MAX = 32u;                 // VRH_MULTI_VOLUME_MAX, the example's MAX_VOLS

// One volume of the frame.  minv is column-major (matrix::data()); light_dir is constant per volume and computed
// once on the host by mv_light_dir, the kernel's own expression.
struct __attribute__((aligned(16))) mv_record
{
    vol_view vol;
    tf_view tf;
    float minv[16];
    float bmin[3], bmax[3];
    float sign[3], offset[3], extent[3];
    float light_dir[3];
    float ca[3], ka, cd[3], kd, cs[3], ks, exp;            // plastic<float>
    float pad;
};
static_assert(sizeof(mv_record) % 16 == 0, "records are read as an array");

struct mv_params
{
    float dt, cutoff, shade_alpha, delta;
    float light_pos[3], light_cl[3], light_kl, light_att[3];   // point_light<float>: constant, linear, quadratic
    uint32_t num;             // volumes, 1 .. MULTI_VOLUME_MAX
    uint32_t cap;             // hard step limit, 2 * ceil(2 D / dt) + 8
};

VRH_TEX_FN float mv_powf(float x, float y)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_powf(x, y);
#else
    return powf(x, y);
#endif
}

// (Minv * (v, w)).xyz
VRH_TEX_FN void mv_transform(const float m[16], const float v[3], float w, float out[3])
{
    for (int r = 0; r < 3; ++r) out[r] = ((m[r] * v[0] + m[4 + r] * v[1]) + m[8 + r] * v[2]) + m[12 + r] * w;
}

VRH_TEX_FN float mv_dot(const float a[3], const float b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// normalize (vector3.inl:331-336): v * rsqrt(dot(v, v)), rsqrt = 1 / sqrt
VRH_TEX_FN void mv_normalize(const float v[3], float out[3])
{
    const float s = 1.0f / __builtin_sqrtf(mv_dot(v, v));
    for (int a = 0; a < 3; ++a) out[a] = v[a] * s;
}

// sr.light_dir of volume `minv`: normalize((Minv * (light.position, 1)).xyz)
VRH_TEX_FN void mv_light_dir(const float minv[16], const float light_pos[3], float out[3])
{
    float p[3];
    mv_transform(minv, light_pos, 1.0f, p);
    mv_normalize(p, out);
}

// A pointer read from a volume record is a generic one to the compiler, and loads through it would be FLAT
// loads.  On the device the voxels and the transfer functions lie in global memory: the kernel's samplers say
// so at every load.  They restate tex3d / tex1d of vrh_volume.h expression by expression (the host build is
// checked against those, tests/cpp/multi_volume_edge_check.cpp), the linear arm in two halves so that the
// loads of several fetches can be issued together.
#if defined(__HIP_DEVICE_COMPILE__)
#define VRH_MV_GLOBAL __attribute__((address_space(1)))
#else
#define VRH_MV_GLOBAL
#endif

template <uint32_t FMT>
VRH_TEX_FN float mv_texel(const vol_view& v, int i)
{
    if (FMT == VOL_R8) return float(int(((const VRH_MV_GLOBAL uint8_t*)v.voxels)[i]));
    if (FMT == VOL_R16) return float(int(((const VRH_MV_GLOBAL uint16_t*)v.voxels)[i]));
    return ((const VRH_MV_GLOBAL float*)v.voxels)[i];
}

VRH_TEX_FN rgba_t mv_entry(const tf_view& t, int i)
{
    const VRH_MV_GLOBAL float* e = (const VRH_MV_GLOBAL float*)t.entries + 4 * tf_index(t, i);
    rgba_t r;
    r.x = e[0]; r.y = e[1]; r.z = e[2]; r.w = e[3];
    return r;
}

// the eight voxel indices and the three weights of a linear fetch ...
VRH_TEX_FN void tex3d_linear_taps(const vol_view& v, float cx, float cy, float cz, int idx[8], float u[3])
{
    const uint32_t ax = (v.modes >> 8) & 255u, ay = (v.modes >> 16) & 255u, az = v.modes >> 24;
    const float c1x = tex_map(cx - v.half[0], ax, v.aux[0]), c2x = tex_map(cx + v.half[0], ax, v.aux[0]);
    const float c1y = tex_map(cy - v.half[1], ay, v.aux[1]), c2y = tex_map(cy + v.half[1], ay, v.aux[1]);
    const float c1z = tex_map(cz - v.half[2], az, v.aux[2]), c2z = tex_map(cz + v.half[2], az, v.aux[2]);
    const int lx = int(c1x * v.size[0]), ly = int(c1y * v.size[1]), lz = int(c1z * v.size[2]);
    const int hx = int(c2x * v.size[0]), hy = int(c2y * v.size[1]), hz = int(c2z * v.size[2]);
    idx[0] = vol_index(v, lx, ly, lz); idx[1] = vol_index(v, hx, ly, lz);
    idx[2] = vol_index(v, lx, hy, lz); idx[3] = vol_index(v, hx, hy, lz);
    idx[4] = vol_index(v, lx, ly, hz); idx[5] = vol_index(v, hx, ly, hz);
    idx[6] = vol_index(v, lx, hy, hz); idx[7] = vol_index(v, hx, hy, hz);
    u[0] = c1x * v.size[0] - float(lx); u[1] = c1y * v.size[1] - float(ly); u[2] = c1z * v.size[2] - float(lz);
}

// ... and the filter over the eight voxels
template <uint32_t FMT>
VRH_TEX_FN float tex3d_linear_filter(const float s[8], const float u[3])
{
    const float p1 = tex_lerp(s[0], s[1], u[0]), p2 = tex_lerp(s[2], s[3], u[0]);
    const float p3 = tex_lerp(s[4], s[5], u[0]), p4 = tex_lerp(s[6], s[7], u[0]);
    const float p12 = tex_lerp(p1, p2, u[1]), p34 = tex_lerp(p3, p4, u[1]);
    return vol_finish<FMT>(tex_lerp(p12, p34, u[2]));
}

VRH_TEX_FN int tex3d_nearest_tap(const vol_view& v, float cx, float cy, float cz)
{
    const uint32_t ax = (v.modes >> 8) & 255u, ay = (v.modes >> 16) & 255u, az = v.modes >> 24;
    const float mx = tex_map(cx, ax, v.aux[0]), my = tex_map(cy, ay, v.aux[1]), mz = tex_map(cz, az, v.aux[2]);
    return vol_index(v, int(mx * v.size[0]), int(my * v.size[1]), int(mz * v.size[2]));
}

// tex3D of K coordinates at once: the voxel loads of all of them (8 K for a linear volume) are issued before
// the first use
template <uint32_t FMT, int K>
VRH_TEX_FN void mv_tex3d(const vol_view& v, const float c[][3], float f[])
{
    if ((v.modes & 255u) == TEX_NEAREST)
    {
        int idx[K];
        for (int k = 0; k < K; ++k) idx[k] = tex3d_nearest_tap(v, c[k][0], c[k][1], c[k][2]);
        for (int k = 0; k < K; ++k) f[k] = vol_finish<FMT>(mv_texel<FMT>(v, idx[k]));
        return;
    }
    int idx[K][8];
    float u[K][3], s[K][8];
    for (int k = 0; k < K; ++k) tex3d_linear_taps(v, c[k][0], c[k][1], c[k][2], idx[k], u[k]);
    for (int k = 0; k < K; ++k)
        for (int j = 0; j < 8; ++j) s[k][j] = mv_texel<FMT>(v, idx[k][j]);
    for (int k = 0; k < K; ++k) f[k] = tex3d_linear_filter<FMT>(s[k], u[k]);
}

// tex1D(transfunc, coord), the expressions of tex1d
VRH_TEX_FN rgba_t mv_tex1d(const tf_view& t, float c)
{
    const uint32_t a = (t.modes >> 8) & 255u;
    if ((t.modes & 255u) == TEX_NEAREST) return mv_entry(t, int(tex_map(c, a, t.aux) * t.sizef));
    const float c1 = tex_map(c - t.half, a, t.aux), c2 = tex_map(c + t.half, a, t.aux);
    const int lo = int(c1 * t.sizef), hi = int(c2 * t.sizef);
    const rgba_t e0 = mv_entry(t, lo), e1 = mv_entry(t, hi);
    const float u = c1 * t.sizef - float(lo);
    rgba_t r;
    r.x = tex_lerp(e0.x, e1.x, u); r.y = tex_lerp(e0.y, e1.y, u);
    r.z = tex_lerp(e0.z, e1.z, u); r.w = tex_lerp(e0.w, e1.w, u);
    return r;
}

// gradient(volume, tc) with its six fetches
template <uint32_t FMT>
VRH_TEX_FN void mv_gradient(const vol_view& v, const float tc[3], float delta, float grad[3])
{
    // s1.x s2.x s1.y s2.y s1.z s2.z
    const float c[6][3] = {
        { tc[0] - delta, tc[1] - 0.0f, tc[2] - 0.0f }, { tc[0] + delta, tc[1] + 0.0f, tc[2] + 0.0f },
        { tc[0] + 0.0f, tc[1] + delta, tc[2] + 0.0f }, { tc[0] - 0.0f, tc[1] - delta, tc[2] - 0.0f },
        { tc[0] + 0.0f, tc[1] + 0.0f, tc[2] + delta }, { tc[0] - 0.0f, tc[1] - 0.0f, tc[2] - delta } };
    float f[6];
    mv_tex3d<FMT, 6>(v, c, f);
    grad[0] = f[1] - f[0]; grad[1] = f[3] - f[2]; grad[2] = f[5] - f[4];
}

// materials[i].shade(sr): pi * (lambertian + blinn) * light.intensity(isect_pos) * ndotl
VRH_TEX_FN void mv_plastic_shade(const mv_record& r, const mv_params& K, const float n[3], const float wo[3],
                                 const float pos[3], float out[3])
{
    constexpr float PI = 3.14159265358979323846264338328e+00f;      // math.h:240 constants::pi
    constexpr float INV_PI = 3.18309886183790691216444201928e-01f;  // math.h:242 constants::inv_pi
    const float* wi = r.light_dir;
    const float ndotl = ref_max(0.0f, mv_dot(n, wi));
    // blinn::f
    const float hs[3] = { wo[0] + wi[0], wo[1] + wi[1], wo[2] + wi[2] };
    float h[3];
    mv_normalize(hs, h);
    const float hdotn = ref_max(0.0f, mv_dot(h, n));
    const float sat = ref_max(0.0f, ref_min(mv_dot(wi, h), 1.0f));   // saturate, math.h:454-457
    const float p5 = mv_powf(1.0f - sat, 5.0f);
    const float nfactor = (r.exp + 2.0f) / (8.0f * PI);
    const float pe = mv_powf(hdotn, r.exp);
    // point_light::intensity: the light's world position against the volume-space position
    const float dv[3] = { K.light_pos[0] - pos[0], K.light_pos[1] - pos[1], K.light_pos[2] - pos[2] };
    const float dist = __builtin_sqrtf(mv_dot(dv, dv));
    const float den = K.light_att[0] + K.light_att[1] * dist + K.light_att[2] * dist * dist;
    const float att = float(1.0 / double(den));
    for (int a = 0; a < 3; ++a)
    {
        const float cd = (r.cd[a] * r.kd) * INV_PI;
        const float spec = r.cs[a] * r.ks;
        const float schlick = spec + (1.0f - spec) * p5;
        const float bl = (schlick * nfactor) * pe;
        const float I = (K.light_cl[a] * K.light_kl) * att;
        out[a] = ((PI * (cd + bl)) * I) * ndotl;
    }
}

// One volume's sample at the world-space position pw of a ray with direction dir: colori, premultiplied
template <uint32_t FMT>
VRH_TEX_FN rgba_t mv_sample(const mv_record& r, const mv_params& K, const float pw[3], const float dir[3], bool& shaded)
{
    float pos[3], tc[3];
    mv_transform(r.minv, pw, 1.0f, pos);
    for (int d = 0; d < 3; ++d) tc[d] = (r.sign[d] * pos[d] + r.offset[d]) / r.extent[d];
    const float c1[1][3] = { { tc[0], tc[1], tc[2] } };
    float voxel;
    mv_tex3d<FMT, 1>(r.vol, c1, &voxel);
    rgba_t c = mv_tex1d(r.tf, voxel);
    shaded = false;
    if (c.w >= K.shade_alpha)
    {
        float grad[3];
        mv_gradient<FMT>(r.vol, tc, K.delta, grad);
        const float len = __builtin_sqrtf(mv_dot(grad, grad));
        if (len != 0.0f)
        {
            const float s = 1.0f / len;
            const float n[3] = { grad[0] * s, grad[1] * s, grad[2] * s };
            const float wo[3] = { -dir[0], -dir[1], -dir[2] };
            float sh[3];
            mv_plastic_shade(r, K, n, wo, pos, sh);
            c.x *= sh[0]; c.y *= sh[1]; c.z *= sh[2];
            shaded = true;
        }
    }
    c.x *= c.w; c.y *= c.w; c.z *= c.w;
    return c;
}

// the host's policies: the wave is the ray, the ranges an array
struct mv_single_ray { static VRH_TEX_FN bool any(bool b) { return b; } };
struct mv_array_ranges
{
    float v[2 * MULTI_VOLUME_MAX];
    VRH_TEX_FN void set(uint32_t i, float tn, float tf) { v[2 * i] = tn; v[2 * i + 1] = tf; }
    VRH_TEX_FN float tnear(uint32_t i) const { return v[2 * i]; }
    VRH_TEX_FN float tfar(uint32_t i) const { return v[2 * i + 1]; }
};

struct mv_result
{
    rgba_t color;
    float tmin;
    uint32_t steps;           // iterations of the loop
    uint32_t samples;         // volume samples taken, and those of them that were shaded
    uint32_t shaded;
    bool hit, capped;
};

// The kernel of the example for one ray.  Every lane of a wave calls it, `active` or not: an inactive lane
// takes no step and leaves hit = false.
// `recs[i]` is record i (the host: a pointer; the kernel: an accessor that tells the compiler i is uniform).
template <class Wave, class Records, class Ranges>
VRH_TEX_FN mv_result multi_march(const Records& recs, const mv_params& K, const float ori[3], const float dir[3],
                                 bool active, Ranges& R)
{
    float tmin = 3.402823466e+38f, tmax = -3.402823466e+38f;         // numeric_limits<float>::max()
    uint32_t mask = 0;                                                // volumes some lane's range is not empty for
    for (uint32_t i = 0; i < K.num; ++i)
    {
        const mv_record& r = recs[i];
        float o[3], d[3], tn, tf;
        mv_transform(r.minv, ori, 1.0f, o);
        mv_transform(r.minv, dir, 0.0f, d);                           // not renormalised
        const bool h = box_clip(o, d, r.bmin, r.bmax, tn, tf);
        if (h && tn < tmin) tmin = tn;
        if (h && tf > tmax) tmax = tf;
        R.set(i, tn, tf);
        if (Wave::any(active && tn < tf)) mask |= 1u << i;
    }
    mv_result res;
    res.color.x = res.color.y = res.color.z = res.color.w = 0.0f;
    res.steps = res.samples = res.shaded = 0;
    res.capped = false;
    bool done = !active;
    float t = tmin;
    for (;;)
    {
        const bool live = !done && t < tmax;
        if (!Wave::any(live)) break;
        const bool over = live && res.steps >= K.cap;
        if (over) { res.capped = true; done = true; }
        const bool go = live && !over;
        if (go) ++res.steps;
        const float pw[3] = { ori[0] + dir[0] * t, ori[1] + dir[1] * t, ori[2] + dir[2] * t };
        rgba_t sum;
        sum.x = sum.y = sum.z = sum.w = 0.0f;
        for (uint32_t m = mask; m; m &= m - 1u)
        {
            const uint32_t i = uint32_t(__builtin_ctz(m));
            const bool inside = go && t >= R.tnear(i) && t < R.tfar(i);
            if (!Wave::any(inside)) continue;
            if (inside)
            {
                const mv_record& r = recs[i];
                bool sh;
                const rgba_t c = r.vol.format == VOL_R8 ? mv_sample<VOL_R8>(r, K, pw, dir, sh)
                               : r.vol.format == VOL_R16 ? mv_sample<VOL_R16>(r, K, pw, dir, sh)
                                                         : mv_sample<VOL_R32F>(r, K, pw, dir, sh);
                sum.x += c.x; sum.y += c.y; sum.z += c.z; sum.w += c.w;
                ++res.samples;
                res.shaded += sh ? 1u : 0u;
            }
        }
        if (go)
        {
            const float s = 1.0f - res.color.w;
            res.color.x += sum.x * s; res.color.y += sum.y * s; res.color.z += sum.z * s; res.color.w += sum.w * s;
            if (res.color.w >= K.cutoff) done = true;
            else t += K.dt;
        }
    }
    res.hit = active && tmax > tmin;
    res.tmin = tmin;
    return res;
}

} // namespace dev
} // namespace vrh
