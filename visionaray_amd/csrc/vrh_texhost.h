// visionaray_amd/csrc/vrh_texhost.h -- host-side checks and pixel expansion of vrh_texture_desc, shared by
// vrh_tex2d_host / vrh_pnm_load (vrh_texture.cpp) and vrh_shading_set_textures (vrh_runtime.hip).
#pragma once

#include "vrh_internal.h"
#include "visionaray_hip/detail/vrh_texture.h"

#include <cmath>
#include <string>
#include <vector>

namespace vrh {

static_assert(int(VRH_TEX_NEAREST) == int(dev::TEX_NEAREST) && int(VRH_TEX_LINEAR) == int(dev::TEX_LINEAR), "texture filters");
static_assert(int(VRH_TEX_WRAP) == int(dev::TEX_WRAP) && int(VRH_TEX_MIRROR) == int(dev::TEX_MIRROR)
              && int(VRH_TEX_CLAMP) == int(dev::TEX_CLAMP), "texture address modes");
static_assert(VRH_TEX_MAX_DIM == dev::TEX_MAX_DIM && VRH_TEX_MAX_COORD == dev::TEX_MAX_COORD, "texture limits");

inline bool tex_is_dummy(const vrh_texture_desc& d) { return d.width == 0 || d.height == 0; }

// empty: the descriptor is valid
inline std::string check_texture_desc(const vrh_texture_desc& d)
{
    if (d.format > VRH_TEX_R8) return "unknown texture format " + std::to_string(d.format);
    if (d.filter > VRH_TEX_LINEAR) return "unknown texture filter " + std::to_string(d.filter);
    for (int a = 0; a < 2; ++a)
        if (d.address[a] > VRH_TEX_CLAMP) return "unknown texture address mode " + std::to_string(d.address[a]);
    if (tex_is_dummy(d)) return "";
    if (d.width > VRH_TEX_MAX_DIM || d.height > VRH_TEX_MAX_DIM) return "a texture dimension above 32768";
    if (uint64_t(d.width) * d.height > VRH_TEX_MAX_TEXELS) return "a texture of more than 2^28 texels";
    if (!d.pixels) return "a texture without pixels";
    return "";
}

// the index of the first coordinate value that is not finite or exceeds 2^20 in magnitude, else n
inline size_t first_bad_coord(const float* c, size_t n)
{
    for (size_t i = 0; i < n; ++i)
        if (!(std::fabs(c[i]) <= VRH_TEX_MAX_COORD)) return i;
    return n;
}

// the texels as packed RGBA8 (swizzle.h:196-224 with AlphaIsOne for RGB8 / R8)
inline void expand_rgba8(const vrh_texture_desc& d, std::vector<uint32_t>& out)
{
    const size_t n = size_t(d.width) * d.height;
    out.resize(n);
    const uint8_t* p = static_cast<const uint8_t*>(d.pixels);
    for (size_t i = 0; i < n; ++i)
    {
        uint32_t r, g, b, a = 255u;
        if (d.format == VRH_TEX_RGBA8) { r = p[4 * i]; g = p[4 * i + 1]; b = p[4 * i + 2]; a = p[4 * i + 3]; }
        else if (d.format == VRH_TEX_RGB8) { r = p[3 * i]; g = p[3 * i + 1]; b = p[3 * i + 2]; }
        else { r = g = b = p[i]; }
        out[i] = r | g << 8 | b << 16 | a << 24;
    }
}

} // namespace vrh
