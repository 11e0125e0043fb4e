// visionaray_amd/csrc/vrh_texture.cpp -- host entry points of the texture support (include/vrh.h):
// vrh_tex2d_host, the host build of the shared sampler (visionaray_hip/detail/vrh_texture.h), and the
// binary PNM reader vrh_pnm_load / vrh_pnm_free (<- src/common/pnm_image.cpp).
#include "vrh_texhost.h"

#include <cstdio>
#include <cstdlib>
#include <new>

using namespace vrh;

extern "C" {

VRH_API int vrh_tex2d_host(const vrh_texture_desc* desc, const float* coords, uint32_t n, uint8_t* rgba_out)
{
    if (!desc || (n && (!coords || !rgba_out))) { set_error("vrh_tex2d_host: null argument"); return VRH_ERR_INVALID; }
    const std::string bad = check_texture_desc(*desc);
    if (!bad.empty()) { set_error("vrh_tex2d_host: " + bad); return VRH_ERR_INVALID; }
    const size_t bc = first_bad_coord(coords, size_t(n) * 2);
    if (bc != size_t(n) * 2)
    {
        set_error("vrh_tex2d_host: coordinate " + std::to_string(bc / 2) + " is not finite or exceeds 2^20 in magnitude");
        return VRH_ERR_INVALID;
    }
    if (tex_is_dummy(*desc))
    {
        for (size_t i = 0; i < size_t(n) * 4; ++i) rgba_out[i] = 255u;
        return VRH_OK;
    }
    std::vector<uint32_t> expanded;
    const uint32_t* pixels = static_cast<const uint32_t*>(desc->pixels);
    try
    {
        // RGBA8 texels are sampled where they are (the bytes are read through a packed copy only when the
        // pointer is not 4-byte aligned)
        if (desc->format != VRH_TEX_RGBA8 || (reinterpret_cast<uintptr_t>(desc->pixels) & 3u))
        {
            expand_rgba8(*desc, expanded);
            pixels = expanded.data();
        }
    }
    catch (const std::bad_alloc&) { set_error("host allocation failed"); return VRH_ERR_OOM; }
    const dev::tex_view t = dev::make_tex_view(pixels, desc->width, desc->height, desc->filter, desc->address[0], desc->address[1]);
    for (uint32_t i = 0; i < n; ++i)
    {
        const uint32_t s = dev::tex2d(t, coords[2 * size_t(i)], coords[2 * size_t(i) + 1]);
        for (int c = 0; c < 4; ++c) rgba_out[4 * size_t(i) + c] = uint8_t(s >> (8 * c));
    }
    return VRH_OK;
}

// one header token of a PNM file: white space and `#` comment lines skipped; false at the end of the file
static bool pnm_token(FILE* f, std::string& tok)
{
    tok.clear();
    int c = fgetc(f);
    for (;;)
    {
        while (c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f') c = fgetc(f);
        if (c != '#') break;
        while (c != '\n' && c != EOF) c = fgetc(f);
    }
    while (c != EOF && c != ' ' && c != '\t' && c != '\n' && c != '\r' && c != '\v' && c != '\f' && tok.size() < 16)
    {
        tok.push_back(char(c));
        c = fgetc(f);
    }
    // the single white-space character after the token is consumed: after the max value the samples begin
    return !tok.empty();
}

static bool pnm_number(FILE* f, uint32_t& v)
{
    std::string tok;
    if (!pnm_token(f, tok)) return false;
    uint64_t x = 0;
    for (char ch : tok)
    {
        if (ch < '0' || ch > '9') return false;
        x = x * 10 + uint64_t(ch - '0');
        if (x > 0xFFFFFFFFull) return false;
    }
    v = uint32_t(x);
    return true;
}

VRH_API int vrh_pnm_load(const char* filename, vrh_pnm_image* out)
{
    if (!filename || !out) { set_error("vrh_pnm_load: null argument"); return VRH_ERR_INVALID; }
    *out = vrh_pnm_image{};
    FILE* f = std::fopen(filename, "rb");
    if (!f) { set_error(std::string("vrh_pnm_load: cannot open ") + filename); return VRH_ERR_INVALID; }
    struct closer { FILE* f; ~closer() { std::fclose(f); } } guard{ f };
    std::string magic;
    if (!pnm_token(f, magic) || magic.size() != 2 || magic[0] != 'P' || magic[1] < '1' || magic[1] > '7')
    {
        set_error(std::string("vrh_pnm_load: ") + filename + " is not a binary PNM file (P5 / P6)");
        return VRH_ERR_UNSUPPORTED;
    }
    if (magic != "P5" && magic != "P6")
    {
        set_error(std::string("vrh_pnm_load: ") + filename + ": PNM type " + magic + " is not supported (binary P5 / P6 are)");
        return VRH_ERR_UNSUPPORTED;
    }
    uint32_t w = 0, h = 0, maxv = 0;
    if (!pnm_number(f, w) || !pnm_number(f, h) || !pnm_number(f, maxv) || w == 0 || h == 0 || maxv == 0)
    {
        set_error(std::string("vrh_pnm_load: ") + filename + ": malformed header");
        return VRH_ERR_INVALID;
    }
    if (maxv > 255u)
    {
        set_error(std::string("vrh_pnm_load: ") + filename + ": 16-bit samples are not supported");
        return VRH_ERR_UNSUPPORTED;
    }
    if (w > VRH_TEX_MAX_DIM || h > VRH_TEX_MAX_DIM || uint64_t(w) * h > VRH_TEX_MAX_TEXELS)
    {
        set_error(std::string("vrh_pnm_load: ") + filename + ": image too large");
        return VRH_ERR_INVALID;
    }
    const uint32_t ch = magic == "P6" ? 3u : 1u;
    const size_t bytes = size_t(w) * h * ch;
    uint8_t* px = static_cast<uint8_t*>(std::malloc(bytes));
    if (!px) { set_error("host allocation failed"); return VRH_ERR_OOM; }
    if (std::fread(px, 1, bytes, f) != bytes)
    {
        std::free(px);
        set_error(std::string("vrh_pnm_load: ") + filename + ": truncated");
        return VRH_ERR_INVALID;
    }
    if (maxv != 255u)
    {
        const double scale = (1.0 / double(int(maxv))) * 255;            // pnm_image.cpp:88-97
        for (size_t i = 0; i < bytes; ++i) px[i] = static_cast<uint8_t>(px[i] * scale);
    }
    out->pixels = px; out->width = w; out->height = h; out->channels = ch; out->max_value = maxv;
    return VRH_OK;
}

VRH_API int vrh_pnm_free(vrh_pnm_image* image)
{
    if (!image) return VRH_OK;
    std::free(image->pixels);
    *image = vrh_pnm_image{};
    return VRH_OK;
}

} // extern "C"
