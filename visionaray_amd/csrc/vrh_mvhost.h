// visionaray_amd/csrc/vrh_mvhost.h -- host-side checks of the multi-volume descriptors (include/vrh.h) and the
// volume records built from them, shared by vrh_multi_volume_render_host (vrh_volume_host.cpp) and
// vrh_render_multi_volume (vrh_multi_volume.hip).
#pragma once

#include "vrh_volhost.h"
#include "visionaray_hip/detail/vrh_multi_volume.h"

#include <vector>

namespace vrh {

static_assert(VRH_MULTI_VOLUME_MAX == dev::MULTI_VOLUME_MAX, "the example's MAX_VOLS");
static_assert(sizeof(vrh_plastic) == 13 * 4 && sizeof(vrh_point_light) == 10 * 4, "material and light records");

// The entries, the kernel parameters and the camera.  Fills K (the step limit included) and one record per
// volume, all but its two views.  empty: valid
inline std::string check_multi_volume(const vrh_multi_volume_entry* entries, uint32_t n, const vrh_multi_volume_kernel_desc& k,
                                      const vrh_camera& cam, dev::mv_params& K, std::vector<dev::mv_record>& recs)
{
    if (n < 1 || n > VRH_MULTI_VOLUME_MAX) return std::to_string(n) + " volumes: 1 to 32 can be rendered";
    if (!entries) return "null entries";
    if (cam.width == 0 || cam.height == 0) return "an image of size 0";
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(cam.eye[a]) || !std::isfinite(cam.cam_u[a]) || !std::isfinite(cam.cam_v[a]) || !std::isfinite(cam.cam_w[a]))
            return "a camera that is not finite";
    const float* lf = reinterpret_cast<const float*>(&k.light);
    for (int i = 0; i < 10; ++i)
        if (!std::isfinite(lf[i])) return "a light that is not finite";
    if (std::isnan(k.shade_alpha)) return "shade_alpha is not a number";
    if (!std::isfinite(k.gradient_delta) || !(std::fabs(k.gradient_delta) <= VRH_TEX_MAX_COORD / 2))
        return "gradient_delta is not finite or exceeds 2^19 in magnitude";
    if (std::isnan(k.opacity_cutoff)) return "opacity_cutoff is not a number";
    double D = 0.0;
    for (uint32_t v = 0; v < n; ++v)
    {
        const vrh_multi_volume_entry& e = entries[v];
        const std::string at = "volume " + std::to_string(v) + ": ";
        for (int a = 0; a < 3; ++a)
        {
            if (!std::isfinite(e.box_min[a]) || !std::isfinite(e.box_max[a]) || !(e.box_min[a] <= e.box_max[a]))
                return at + "a box that is not finite or has min > max";
            if (e.coord_sign[a] != 1.0f && e.coord_sign[a] != -1.0f) return at + "a coordinate sign that is neither +1 nor -1";
            if (!std::isfinite(e.coord_offset[a])) return at + "a coordinate offset that is not finite";
            if (!std::isfinite(e.coord_extent[a]) || e.coord_extent[a] == 0.0f) return at + "a coordinate extent that is 0 or not finite";
            for (const float c : { e.box_min[a], e.box_max[a] })
                if (!(std::fabs((double(e.coord_sign[a]) * c + e.coord_offset[a]) / e.coord_extent[a]) <= VRH_TEX_MAX_COORD / 2))
                    return at + "a texture coordinate of the box exceeds 2^19 in magnitude";
        }
        const float* mf = reinterpret_cast<const float*>(&e.material);
        for (int i = 0; i < 13; ++i)
            if (!std::isfinite(mf[i])) return at + "a material that is not finite";
        for (int i = 0; i < 16; ++i)
            if (!std::isfinite(e.transform_inv[i])) return at + "a transform that is not finite";
        // world = A^-1 (volume - b) with A the 3 x 3 part and b the translation of transform_inv, in double
        const float* m = e.transform_inv;
        const double a00 = m[0], a01 = m[4], a02 = m[8], a10 = m[1], a11 = m[5], a12 = m[9], a20 = m[2], a21 = m[6], a22 = m[10];
        const double c00 = a11 * a22 - a12 * a21, c01 = a12 * a20 - a10 * a22, c02 = a10 * a21 - a11 * a20;
        const double det = a00 * c00 + a01 * c01 + a02 * c02;
        const double scale = (std::fabs(a00) + std::fabs(a01) + std::fabs(a02)) * (std::fabs(a10) + std::fabs(a11) + std::fabs(a12))
                           * (std::fabs(a20) + std::fabs(a21) + std::fabs(a22));
        if (!(std::fabs(det) > 1e-12 * scale)) return at + "a transform whose 3 x 3 part is singular";
        const double inv[3][3] = {
            { c00 / det, (a02 * a21 - a01 * a22) / det, (a01 * a12 - a02 * a11) / det },
            { c01 / det, (a00 * a22 - a02 * a20) / det, (a02 * a10 - a00 * a12) / det },
            { c02 / det, (a01 * a20 - a00 * a21) / det, (a00 * a11 - a01 * a10) / det } };
        for (int corner = 0; corner < 8; ++corner)
        {
            double p[3], d2 = 0.0;
            for (int a = 0; a < 3; ++a) p[a] = double((corner >> a) & 1 ? e.box_max[a] : e.box_min[a]) - double(m[12 + a]);
            for (int r = 0; r < 3; ++r)
            {
                const double w = inv[r][0] * p[0] + inv[r][1] * p[1] + inv[r][2] * p[2];
                d2 += (w - double(cam.eye[r])) * (w - double(cam.eye[r]));
            }
            if (!std::isfinite(d2)) return at + "a box corner that is not finite in world space";
            if (std::sqrt(d2) > D) D = std::sqrt(d2);
        }
    }
    if (!std::isfinite(k.dt)) return "dt is not finite";
    if (!(k.dt > 0.0f)) return "dt <= 0";
    if (double(k.dt) < D * (1.0 / 1048576.0)) return "dt is below 2^-20 of the distance from the eye to the farthest box corner";
    if (2.0 * D / double(k.dt) > double(VRH_VOLUME_MAX_STEPS)) return "more than 65536 steps from the nearest to the farthest box corner";
    K.dt = k.dt; K.cutoff = k.opacity_cutoff; K.shade_alpha = k.shade_alpha; K.delta = k.gradient_delta;
    for (int a = 0; a < 3; ++a) { K.light_pos[a] = k.light.position[a]; K.light_cl[a] = k.light.cl[a]; }
    K.light_kl = k.light.kl;
    K.light_att[0] = k.light.constant_att; K.light_att[1] = k.light.linear_att; K.light_att[2] = k.light.quadratic_att;
    K.num = n;
    K.cap = 2u * uint32_t(std::ceil(2.0 * D / double(k.dt))) + 8u;
    recs.assign(n, dev::mv_record{});
    for (uint32_t v = 0; v < n; ++v)
    {
        const vrh_multi_volume_entry& e = entries[v];
        dev::mv_record& r = recs[v];
        std::memcpy(r.minv, e.transform_inv, sizeof(r.minv));
        for (int a = 0; a < 3; ++a)
        {
            r.bmin[a] = e.box_min[a]; r.bmax[a] = e.box_max[a];
            r.sign[a] = e.coord_sign[a]; r.offset[a] = e.coord_offset[a]; r.extent[a] = e.coord_extent[a];
            r.ca[a] = e.material.ca[a]; r.cd[a] = e.material.cd[a]; r.cs[a] = e.material.cs[a];
        }
        r.ka = e.material.ka; r.kd = e.material.kd; r.ks = e.material.ks; r.exp = e.material.exp;
        dev::mv_light_dir(r.minv, K.light_pos, r.light_dir);
    }
    return "";
}

} // namespace vrh
