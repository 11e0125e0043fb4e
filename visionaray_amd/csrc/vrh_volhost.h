// visionaray_amd/csrc/vrh_volhost.h -- host-side checks of the volume descriptors (include/vrh.h), shared by
// the host entry points (vrh_volume_host.cpp) and the device ones (vrh_volume.hip).
#pragma once

#include "vrh_texhost.h"
#include "visionaray_hip/detail/vrh_volume.h"

#include <cmath>
#include <cstring>
#include <string>

namespace vrh {

static_assert(int(VRH_VOL_R8) == int(dev::VOL_R8) && int(VRH_VOL_R16) == int(dev::VOL_R16)
              && int(VRH_VOL_R32F) == int(dev::VOL_R32F), "volume formats");
static_assert(VRH_VOLUME_MAX_STEPS == dev::VOLUME_MAX_STEPS, "volume step limit");
static_assert(sizeof(dev::rgba_t) == 16, "a transfer-function entry is four floats");

inline size_t voxel_bytes(uint32_t format) { return format == VRH_VOL_R8 ? 1 : format == VRH_VOL_R16 ? 2 : 4; }

// empty: the descriptor is valid
inline std::string check_volume_desc(const vrh_volume_desc& d)
{
    if (d.format > VRH_VOL_R32F) return "unknown volume format " + std::to_string(d.format);
    if (d.filter > VRH_TEX_LINEAR) return "unknown texture filter " + std::to_string(d.filter);
    for (int a = 0; a < 3; ++a)
        if (d.address[a] > VRH_TEX_CLAMP) return "unknown texture address mode " + std::to_string(d.address[a]);
    if (d.width == 0 || d.height == 0 || d.depth == 0) return "a volume dimension of 0";
    if (d.width > VRH_TEX_MAX_DIM || d.height > VRH_TEX_MAX_DIM || d.depth > VRH_TEX_MAX_DIM) return "a volume dimension above 32768";
    const uint64_t n = uint64_t(d.width) * d.height * d.depth;
    if (n > VRH_TEX_MAX_TEXELS) return "a volume of more than 2^28 voxels";
    if (!d.voxels) return "a volume without voxels";
    if (d.format == VRH_VOL_R32F)
    {
        // unaligned pointers are legal in the ABI: the floats are read through memcpy
        const unsigned char* p = static_cast<const unsigned char*>(d.voxels);
        for (uint64_t i = 0; i < n; ++i)
        {
            float v;
            std::memcpy(&v, p + 4 * i, 4);
            if (!std::isfinite(v)) return "voxel " + std::to_string(i) + " is not finite";
            if (!(std::fabs(v) <= VRH_TEX_MAX_COORD)) return "voxel " + std::to_string(i) + " exceeds 2^20 in magnitude";
        }
    }
    return "";
}

inline std::string check_transfunc_desc(const vrh_transfunc_desc& d)
{
    if (d.filter > VRH_TEX_LINEAR) return "unknown texture filter " + std::to_string(d.filter);
    if (d.address > VRH_TEX_CLAMP) return "unknown texture address mode " + std::to_string(d.address);
    if (d.size == 0) return "a transfer function of size 0";
    if (d.size > VRH_TEX_MAX_DIM) return "a transfer function size above 32768";
    if (!d.rgba) return "a transfer function without entries";
    for (uint64_t i = 0; i < uint64_t(d.size) * 4; ++i)
        if (!std::isfinite(d.rgba[i])) return "transfer-function entry " + std::to_string(i / 4) + " is not finite";
    return "";
}

// The kernel parameters and the camera; fills K (the step limit included).  empty: valid
inline std::string check_volume_kernel(const vrh_volume_kernel_desc& k, const vrh_camera& cam, dev::march_params& K)
{
    if (cam.width == 0 || cam.height == 0) return "an image of size 0";
    for (int a = 0; a < 3; ++a)
    {
        if (!std::isfinite(cam.eye[a]) || !std::isfinite(cam.cam_u[a]) || !std::isfinite(cam.cam_v[a]) || !std::isfinite(cam.cam_w[a]))
            return "a camera that is not finite";
        if (!std::isfinite(k.box_min[a]) || !std::isfinite(k.box_max[a]) || !(k.box_min[a] <= k.box_max[a]))
            return "a box that is not finite or has min > max";
        if (k.coord_sign[a] != 1.0f && k.coord_sign[a] != -1.0f) return "a coordinate sign that is neither +1 nor -1";
        if (!std::isfinite(k.coord_offset[a])) return "a coordinate offset that is not finite";
        if (!std::isfinite(k.coord_extent[a]) || k.coord_extent[a] == 0.0f) return "a coordinate extent that is 0 or not finite";
    }
    if (!std::isfinite(k.dt)) return "dt is not finite";
    if (!(k.dt > 0.0f)) return "dt <= 0";
    double far2 = 0.0, diag2 = 0.0;
    for (int a = 0; a < 3; ++a)
    {
        const double lo = std::fabs(double(cam.eye[a]) - double(k.box_min[a])), hi = std::fabs(double(cam.eye[a]) - double(k.box_max[a]));
        const double m = lo > hi ? lo : hi, e = double(k.box_max[a]) - double(k.box_min[a]);
        far2 += m * m;
        diag2 += e * e;
        // every position the march samples lies in the box (up to rounding): its texture coordinates stay
        // where every float -> int conversion of the sampler is defined
        for (const float c : { k.box_min[a], k.box_max[a] })
            if (!(std::fabs((double(k.coord_sign[a]) * c + k.coord_offset[a]) / k.coord_extent[a]) <= VRH_TEX_MAX_COORD / 2))
                return "a texture coordinate of the box exceeds 2^19 in magnitude";
    }
    const double D = std::sqrt(far2), diagonal = std::sqrt(diag2);
    if (double(k.dt) < D * (1.0 / 1048576.0)) return "dt is below 2^-20 of the distance from the eye to the farthest box corner";
    if (diagonal / double(k.dt) > double(VRH_VOLUME_MAX_STEPS)) return "more than 65536 steps across the box diagonal";
    for (int a = 0; a < 3; ++a)
    {
        K.bmin[a] = k.box_min[a]; K.bmax[a] = k.box_max[a];
        K.sign[a] = k.coord_sign[a]; K.offset[a] = k.coord_offset[a]; K.extent[a] = k.coord_extent[a];
    }
    K.dt = k.dt;
    K.cutoff = k.opacity_cutoff;
    K.cap = 2u * uint32_t(std::ceil(diagonal / double(k.dt))) + 8u;
    return "";
}

// The entry points vrh_render_volume / vrh_render_multi_volume are compiled from vrh_volume.hip / vrh_multi_volume.hip
// under the names vrh_render_volume_frame / vrh_render_multi_volume_frame (the Makefile passes -Dvrh_render_volume=...
// to those two files, which also renames the declaration of vrh.h they see, and nothing else: no other identifier of
// those names may be added to them).  vrh_resolve.hip defines the public entry points around them (a formatted
// target's refusals, then the frame, then the resolve pass); csrc/vrh_exports.map keeps the inner names out of the
// library's dynamic symbols.  Their own error texts keep the public names.

// the scissor box of a camera clipped to the image: x0, y0, x1, y1
inline void volume_clip(const vrh_camera& cam, uint32_t clip[4])
{
    const uint32_t* sb = cam.scissor;
    const bool whole = sb[0] == 0 && sb[1] == 0 && sb[2] == 0 && sb[3] == 0;
    clip[0] = whole ? 0u : (sb[0] < cam.width ? sb[0] : cam.width);
    clip[1] = whole ? 0u : (sb[1] < cam.height ? sb[1] : cam.height);
    clip[2] = whole ? cam.width : (sb[2] < cam.width ? sb[2] : cam.width);
    clip[3] = whole ? cam.height : (sb[3] < cam.height ? sb[3] : cam.height);
}

} // namespace vrh
