// visionaray_amd/csrc/vrh_resolve.hip -- formatted render targets (include/vrh.h vrh_rt_alloc_formatted): the
// resolve pass that converts a frame from the target's RGBA32F staging colour (and prim_id / t, for depth) into
// its RGBA8 / RGB8 / RGB32F / RGBA32F colour and DEPTH32F / DEPTH24_STENCIL8 depth buffers, as the reference's
// pixel_access::store / blend write them (visionaray_hip/detail/vrh_pixel.h has the per-pixel text, shared with
// vrh_rt_resolve_host below), and the entry points of such targets.
//
// The pass is a stream of pixels: 16 B (20-24 B with depth) read and 3-16 B (+ 4 B depth) written per pixel,
// no reuse, so it is written for the memory system.  Rows of the scissor box go to threadIdx.y, consecutive
// lanes take consecutive pixels of a row:
//   RGBA32F / RGB32F  one pixel per lane: a 16-byte load and a 16-byte store
//   RGBA8             four pixels per lane where the row segment allows: the lanes' quads are aligned in the
//                     linear pixel index (so 16-byte aligned in the byte buffer whatever the image width), a
//                     full quad is four 16-byte loads and one 16-byte store (and one for depth), the partial
//                     quads at the two ends of a row segment go pixel by pixel
//   RGB8              one pixel per lane, three byte stores (a wave's stores cover 192 consecutive bytes; the
//                     3-byte pixels share no dword across rows or lanes that a wider store could own)
// No LDS, no atomics.  The x 255.0 of the unorm conversion is a double multiply per channel
// (v_cvt_f64_f32, v_mul_f64, v_cvt_u32_f64), a few full-rate fp64 operations per pixel beside the 20 bytes moved.

#include "vrh_resolve.h"
#include "vrh_volhost.h"

#include <cstring>
#include <string>

using namespace vrh;
using namespace vrh::dev;

// the volume entry points of vrh_volume.hip / vrh_multi_volume.hip, compiled under these names (Makefile): the
// public ones below add a formatted target's refusals and resolve pass around them
extern "C" {
int vrh_render_volume_frame(vrh_ctx* ctx, const vrh_volume* v, vrh_rt* rt, const vrh_camera* cam,
                            const vrh_volume_kernel_desc* kd);
int vrh_render_multi_volume_frame(vrh_ctx* ctx, const vrh_volume* const* volumes, const vrh_multi_volume_entry* entries,
                                  uint32_t n, vrh_rt* rt, const vrh_camera* cam, const vrh_multi_volume_kernel_desc* kd);
}

namespace {

constexpr int RESOLVE_BX = 64, RESOLVE_BY = 4;

struct resolve_args
{
    resolve_params P;
    const void* color;            // staging RGBA32F
    const uint32_t* prim_id;
    const float* t;
    void* color_out;
    void* depth_out;
};

template <uint32_t CF, uint32_t DF, bool BLEND>
__global__ __launch_bounds__(RESOLVE_BX * RESOLVE_BY) void resolve_kernel(const resolve_args A)
{
    const resolve_params& P = A.P;
    const uint32_t y = P.clip[1] + blockIdx.y * RESOLVE_BY + threadIdx.y;
    if (y >= P.clip[3]) return;
    const uint32_t j = blockIdx.x * RESOLVE_BX + threadIdx.x;
    const size_t row = size_t(y) * P.width;
    if constexpr (CF == CF_RGBA8)
    {
        // quad j of this row's segment [a, b) of the linear pixel index, quads aligned to 4 pixels
        const size_t a = row + P.clip[0], b = row + P.clip[2];
        const size_t q = a / 4 + j;
        const size_t lo = q * 4 > a ? q * 4 : a;
        const size_t hi = q * 4 + 4 < b ? q * 4 + 4 : b;
        if (lo >= hi) return;
        if (hi - lo == 4)
        {
            uint32_t c4[4] = {}, d4[4] = {};
            if constexpr (BLEND)
            {
                const uint4 cw = static_cast<const uint4*>(A.color_out)[q];
                c4[0] = cw.x; c4[1] = cw.y; c4[2] = cw.z; c4[3] = cw.w;
                if constexpr (DF != DF_NONE)
                {
                    const uint4 dw = static_cast<const uint4*>(A.depth_out)[q];
                    d4[0] = dw.x; d4[1] = dw.y; d4[2] = dw.z; d4[3] = dw.w;
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
            {
                const size_t i = lo + k;
                px4 c = load4(A.color, i);
                if constexpr (BLEND) c = blend_color(c, rgba8_unpack(c4[k]), P.s, P.d);
                c4[k] = rgba8_pack(c);
                if constexpr (DF != DF_NONE)
                {
                    // depth_get / depth_store of vrh_pixel.h on the quad's words
                    float depth = staged_depth(P, uint32_t(i - row), y, i, A.prim_id, A.t);
                    if constexpr (BLEND)
                        depth = depth * P.s + (DF == DF_DEPTH32F ? __uint_as_float(d4[k]) : depth24_unpack(d4[k])) * P.d;
                    d4[k] = DF == DF_DEPTH32F ? __float_as_uint(depth) : depth24_pack(depth);
                }
            }
            static_cast<uint4*>(A.color_out)[q] = make_uint4(c4[0], c4[1], c4[2], c4[3]);
            if constexpr (DF != DF_NONE) static_cast<uint4*>(A.depth_out)[q] = make_uint4(d4[0], d4[1], d4[2], d4[3]);
        }
        else
            for (size_t i = lo; i < hi; ++i)
                resolve_pixel<CF, DF, BLEND>(P, uint32_t(i - row), y, i, load4(A.color, i), A.prim_id, A.t, A.color_out, A.depth_out);
    }
    else
    {
        const uint32_t x = P.clip[0] + j;
        if (x >= P.clip[2]) return;
        const size_t i = row + x;
        resolve_pixel<CF, DF, BLEND>(P, x, y, i, load4(A.color, i), A.prim_id, A.t, A.color_out, A.depth_out);
    }
}

template <uint32_t CF, uint32_t DF>
void launch_resolve_df(const resolve_args& a, dim3 grid, hipStream_t s)
{
    const dim3 blk(RESOLVE_BX, RESOLVE_BY);
    if (a.P.blend) hipLaunchKernelGGL((resolve_kernel<CF, DF, true>), grid, blk, 0, s, a);
    else hipLaunchKernelGGL((resolve_kernel<CF, DF, false>), grid, blk, 0, s, a);
}

template <uint32_t CF>
void launch_resolve_cf(uint32_t df, const resolve_args& a, dim3 grid, hipStream_t s)
{
    if (df == DF_NONE) launch_resolve_df<CF, DF_NONE>(a, grid, s);
    else if (df == DF_DEPTH32F) launch_resolve_df<CF, DF_DEPTH32F>(a, grid, s);
    else launch_resolve_df<CF, DF_DEPTH24_STENCIL8>(a, grid, s);
}

// clear_color_buffer / clear_depth_buffer: the converted value into every pixel
template <uint32_t CF>
__global__ void clear_color_kernel(void* buf, size_t n, px4 c)
{
    const size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n) color_store<CF>(buf, i, c);
}

template <uint32_t DF>
__global__ void clear_depth_kernel(void* buf, size_t n, float depth)
{
    const size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i < n) depth_store<DF>(buf, i, depth);
}

bool format_ok(const vrh_rt_format* f, const char* who)
{
    if (!f) { set_error(std::string(who) + ": null format"); return false; }
    if (f->color_format > VRH_CF_RGB8) { set_error(std::string(who) + ": unknown colour format " + std::to_string(f->color_format)); return false; }
    if (f->depth_format > VRH_DF_DEPTH24_STENCIL8) { set_error(std::string(who) + ": unknown depth format " + std::to_string(f->depth_format)); return false; }
    return true;
}

// the box of a descriptor's scissor (all zero: the whole image), clipped to the image
void clip_box(const uint32_t sb[4], uint32_t w, uint32_t h, uint32_t clip[4])
{
    const bool whole = sb[0] == 0 && sb[1] == 0 && sb[2] == 0 && sb[3] == 0;
    clip[0] = whole ? 0u : (sb[0] < w ? sb[0] : w);
    clip[1] = whole ? 0u : (sb[1] < h ? sb[1] : h);
    clip[2] = whole ? w : (sb[2] < w ? sb[2] : w);
    clip[3] = whole ? h : (sb[3] < h ? sb[3] : h);
}

void fill_resolve_params(resolve_params& P, uint32_t w, uint32_t h, const resolve_frame& f)
{
    P = resolve_params{};
    P.width = w; P.height = h;
    for (int i = 0; i < 4; ++i) P.clip[i] = f.clip[i];
    P.blend = f.blend ? 1u : 0u; P.s = f.s; P.d = f.d;
    P.jitter = f.jitter; P.frame_num = f.frame_num;
    P.px_off[0] = f.px_off[0]; P.px_off[1] = f.px_off[1];
    P.width_f = float(w); P.height_f = float(h);
    if (f.mats)
    {
        P.matrix_cam = 1u;
        std::memcpy(P.view, f.mats, sizeof(P.view));
        std::memcpy(P.proj, f.mats + 16, sizeof(P.proj));
        std::memcpy(P.inv_view, f.inv_mats, sizeof(P.inv_view));
        std::memcpy(P.inv_proj, f.inv_mats + 16, sizeof(P.inv_proj));
    }
}

// a descriptor as a frame; inv: 32 floats for the inverses
int desc_frame(const vrh_resolve_desc* d, uint32_t w, uint32_t h, uint32_t depth_format, const char* who, float mats[32],
               float inv[32], resolve_frame& f)
{
    if (!d) { set_error(std::string(who) + ": null descriptor"); return VRH_ERR_INVALID; }
    if (d->blend > 1u) { set_error(std::string(who) + ": blend must be 0 (store) or 1 (blend)"); return VRH_ERR_INVALID; }
    if (d->jitter > 1u) { set_error(std::string(who) + ": jitter must be 0 or 1"); return VRH_ERR_INVALID; }
    f = resolve_frame{};
    clip_box(d->scissor, w, h, f.clip);
    f.blend = d->blend; f.s = d->s; f.d = d->d;
    f.jitter = d->jitter; f.frame_num = d->frame_num;
    f.px_off[0] = d->px_off[0]; f.px_off[1] = d->px_off[1];
    if (d->matrix_cam)
    {
        std::memcpy(mats, d->view, 64);
        std::memcpy(mats + 16, d->proj, 64);
        vrh_matrix_inverse(d->view, inv);
        vrh_matrix_inverse(d->proj, inv + 16);
        f.mats = mats; f.inv_mats = inv;
    }
    return VRH_OK;
}

// the context stream after the asynchronous frames and a render group's writes (vrh_runtime.hip rt_wait)
int wait_target(vrh_ctx* ctx, vrh_rt* rt)
{
    VRH_HIP(ctx_join(ctx));
    if (rt->written_pending) VRH_HIP(hipStreamWaitEvent(ctx->stream, rt->written, 0));
    return VRH_OK;
}

} // namespace

namespace vrh {

int resolve_refuse(const vrh_rt* rt, bool depth_ok, const char* who)
{
    if (!rt || !rt->formatted) return VRH_OK;
    if (rt->depth_format != VRH_DF_NONE && !depth_ok)
    {
        set_error(std::string(who) + ": a render target with a depth format is rendered by vrh_render_view only "
                  "(the depth is that of the matrix camera)");
        return VRH_ERR_UNSUPPORTED;
    }
    return VRH_OK;
}

int resolve_enqueue(vrh_rt* rt, const resolve_frame& f, hipStream_t stream)
{
    if (f.clip[2] <= f.clip[0] || f.clip[3] <= f.clip[1]) return VRH_OK;
    if (f.clip[2] > rt->width || f.clip[3] > rt->height) { set_error("resolve: box outside the target"); return VRH_ERR_INVALID; }
    resolve_args a{};
    fill_resolve_params(a.P, rt->width, rt->height, f);
    a.color = rt->color; a.prim_id = rt->prim_id; a.t = rt->t;
    a.color_out = rt->fcolor; a.depth_out = rt->fdepth;
    const uint32_t bw = f.clip[2] - f.clip[0], bh = f.clip[3] - f.clip[1];
    // RGBA8: the quads a row segment of bw pixels can touch (one more than it fills when it starts inside one)
    const uint32_t per_row = rt->color_format == VRH_CF_RGBA8 ? (bw + 3u) / 4u + 1u : bw;
    const dim3 grid((per_row + RESOLVE_BX - 1) / RESOLVE_BX, (bh + RESOLVE_BY - 1) / RESOLVE_BY);
    switch (rt->color_format)
    {
    case VRH_CF_RGBA32F: launch_resolve_cf<CF_RGBA32F>(rt->depth_format, a, grid, stream); break;
    case VRH_CF_RGB32F: launch_resolve_cf<CF_RGB32F>(rt->depth_format, a, grid, stream); break;
    case VRH_CF_RGBA8: launch_resolve_cf<CF_RGBA8>(rt->depth_format, a, grid, stream); break;
    default: launch_resolve_cf<CF_RGB8>(rt->depth_format, a, grid, stream); break;
    }
    VRH_HIP(hipGetLastError());
    return VRH_OK;
}

int resolve_clear_color(vrh_rt* rt, const float color[4], hipStream_t stream)
{
    const size_t n = size_t(rt->width) * rt->height;
    const px4 c = color ? px4{ color[0], color[1], color[2], color[3] } : px4{ 0.0f, 0.0f, 0.0f, 0.0f };
    const dim3 grid(unsigned((n + 255) / 256)), blk(256);
    switch (rt->color_format)
    {
    case VRH_CF_RGBA32F: hipLaunchKernelGGL(clear_color_kernel<CF_RGBA32F>, grid, blk, 0, stream, rt->fcolor, n, c); break;
    case VRH_CF_RGB32F: hipLaunchKernelGGL(clear_color_kernel<CF_RGB32F>, grid, blk, 0, stream, rt->fcolor, n, c); break;
    case VRH_CF_RGBA8: hipLaunchKernelGGL(clear_color_kernel<CF_RGBA8>, grid, blk, 0, stream, rt->fcolor, n, c); break;
    default: hipLaunchKernelGGL(clear_color_kernel<CF_RGB8>, grid, blk, 0, stream, rt->fcolor, n, c); break;
    }
    VRH_HIP(hipGetLastError());
    return VRH_OK;
}

} // namespace vrh

extern "C" {

VRH_API int vrh_rt_alloc_formatted(vrh_ctx* ctx, uint32_t w, uint32_t h, uint32_t flags, const vrh_rt_format* format,
                                   vrh_rt** out)
{
    static_assert(int(VRH_CF_RGBA32F) == int(CF_RGBA32F) && int(VRH_CF_RGB32F) == int(CF_RGB32F) && int(VRH_CF_RGBA8) == int(CF_RGBA8)
                  && int(VRH_CF_RGB8) == int(CF_RGB8), "colour formats");
    static_assert(int(VRH_DF_NONE) == int(DF_NONE) && int(VRH_DF_DEPTH32F) == int(DF_DEPTH32F)
                  && int(VRH_DF_DEPTH24_STENCIL8) == int(DF_DEPTH24_STENCIL8), "depth formats");
    if (!format_ok(format, "vrh_rt_alloc_formatted")) return VRH_ERR_INVALID;
    VRH_CHECK(ctx && out && w > 0 && h > 0, "vrh_rt_alloc_formatted: bad argument");
    *out = nullptr;
    vrh_rt* rt = nullptr;
    // the staging buffers every frame renders into: colour, prim_id and t whatever the flags say
    const int rc = vrh_rt_alloc(ctx, w, h, flags | VRH_RT_COLOR | VRH_RT_PRIM_ID | VRH_RT_T, &rt);
    if (rc) return rc;
    rt->formatted = true;
    rt->color_format = format->color_format;
    rt->depth_format = format->depth_format;
    const size_t n = size_t(w) * h;
    const size_t cb = n * color_bytes(rt->color_format), db = n * depth_bytes(rt->depth_format);
    hipError_t e = hipMalloc(&rt->fcolor, cb);
    if (e == hipSuccess) e = hipMemset(rt->fcolor, 0, cb);
    if (e == hipSuccess && db) e = hipMalloc(&rt->fdepth, db);
    if (e == hipSuccess && db) e = hipMemset(rt->fdepth, 0, db);
    if (e != hipSuccess)
    {
        set_error(std::string("vrh_rt_alloc_formatted: ") + hipGetErrorString(e));
        vrh_rt_free(rt);
        return VRH_ERR_OOM;
    }
    *out = rt;
    return VRH_OK;
}

VRH_API int vrh_rt_get_formatted(const vrh_rt* rt, void** color, void** depth, vrh_rt_format* format)
{
    VRH_CHECK(rt, "vrh_rt_get_formatted: null");
    if (color) *color = rt->formatted ? rt->fcolor : static_cast<void*>(rt->color);
    if (depth) *depth = rt->formatted ? rt->fdepth : nullptr;
    if (format) *format = vrh_rt_format{ rt->formatted ? rt->color_format : uint32_t(VRH_CF_RGBA32F),
                                         rt->formatted ? rt->depth_format : uint32_t(VRH_DF_NONE) };
    return VRH_OK;
}

VRH_API int vrh_rt_download_formatted(vrh_ctx* ctx, vrh_rt* rt, void* color, void* depth)
{
    VRH_CHECK(ctx && rt, "vrh_rt_download_formatted: null");
    VRH_CHECK(rt->ctx == ctx, "vrh_rt_download_formatted: render target of another context");
    VRH_CHECK(rt->formatted, "vrh_rt_download_formatted: not a formatted target (vrh_rt_alloc_formatted)");
    VRH_CHECK(!depth || rt->fdepth, "vrh_rt_download_formatted: the target has no depth buffer");
    VRH_HIP(hipSetDevice(ctx->device));
    int rc = wait_target(ctx, rt);
    if (rc) return rc;
    VRH_HIP(hipStreamSynchronize(ctx->stream));
    if ((rc = volume_collect(ctx))) return rc;
    const size_t n = size_t(rt->width) * rt->height;
    if (color) VRH_HIP(hipMemcpy(color, rt->fcolor, n * color_bytes(rt->color_format), hipMemcpyDeviceToHost));
    if (depth) VRH_HIP(hipMemcpy(depth, rt->fdepth, n * 4, hipMemcpyDeviceToHost));
    return VRH_OK;
}

VRH_API int vrh_rt_upload_formatted(vrh_ctx* ctx, vrh_rt* rt, const void* color, const void* depth)
{
    VRH_CHECK(ctx && rt, "vrh_rt_upload_formatted: null");
    VRH_CHECK(rt->ctx == ctx, "vrh_rt_upload_formatted: render target of another context");
    VRH_CHECK(rt->formatted, "vrh_rt_upload_formatted: not a formatted target (vrh_rt_alloc_formatted)");
    VRH_CHECK(!depth || rt->fdepth, "vrh_rt_upload_formatted: the target has no depth buffer");
    VRH_HIP(hipSetDevice(ctx->device));
    const int rc = wait_target(ctx, rt);
    if (rc) return rc;
    VRH_HIP(hipStreamSynchronize(ctx->stream));
    const size_t n = size_t(rt->width) * rt->height;
    if (color) VRH_HIP(hipMemcpy(rt->fcolor, color, n * color_bytes(rt->color_format), hipMemcpyHostToDevice));
    if (depth) VRH_HIP(hipMemcpy(rt->fdepth, depth, n * 4, hipMemcpyHostToDevice));
    return VRH_OK;
}

VRH_API int vrh_rt_clear_depth(vrh_ctx* ctx, vrh_rt* rt, float depth)
{
    VRH_CHECK(ctx && rt, "vrh_rt_clear_depth: null");
    VRH_CHECK(rt->ctx == ctx, "vrh_rt_clear_depth: render target of another context");
    VRH_CHECK(rt->formatted && rt->fdepth, "vrh_rt_clear_depth: the target has no depth buffer");
    VRH_HIP(hipSetDevice(ctx->device));
    const int rc = wait_target(ctx, rt);
    if (rc) return rc;
    const size_t n = size_t(rt->width) * rt->height;
    const dim3 grid(unsigned((n + 255) / 256)), blk(256);
    if (rt->depth_format == VRH_DF_DEPTH32F) hipLaunchKernelGGL(clear_depth_kernel<DF_DEPTH32F>, grid, blk, 0, ctx->stream, rt->fdepth, n, depth);
    else hipLaunchKernelGGL(clear_depth_kernel<DF_DEPTH24_STENCIL8>, grid, blk, 0, ctx->stream, rt->fdepth, n, depth);
    VRH_HIP(hipGetLastError());
    return VRH_OK;
}

VRH_API int vrh_rt_resolve(vrh_ctx* ctx, vrh_rt* rt, const vrh_resolve_desc* desc)
{
    VRH_CHECK(ctx && rt, "vrh_rt_resolve: null");
    VRH_CHECK(rt->ctx == ctx, "vrh_rt_resolve: render target of another context");
    VRH_CHECK(rt->formatted, "vrh_rt_resolve: not a formatted target (vrh_rt_alloc_formatted)");
    float mats[32], inv[32];
    resolve_frame f;
    int rc = desc_frame(desc, rt->width, rt->height, rt->depth_format, "vrh_rt_resolve", mats, inv, f);
    if (rc) return rc;
    VRH_HIP(hipSetDevice(ctx->device));
    if ((rc = wait_target(ctx, rt))) return rc;
    rc = resolve_enqueue(rt, f, ctx->stream);
    if (rc == VRH_OK) rt->lane = -1;
    return rc;
}

VRH_API int vrh_rt_resolve_host(const vrh_rt_format* format, uint32_t w, uint32_t h, const float* color,
                                const uint32_t* prim_id, const float* t, const vrh_resolve_desc* desc,
                                void* color_out, void* depth_out)
{
    if (!format_ok(format, "vrh_rt_resolve_host")) return VRH_ERR_INVALID;
    VRH_CHECK(w > 0 && h > 0 && uint64_t(w) * h < (1ull << 32), "vrh_rt_resolve_host: bad image size");
    VRH_CHECK(color && color_out, "vrh_rt_resolve_host: null colour array");
    VRH_CHECK(format->depth_format == VRH_DF_NONE || (t && depth_out && desc && (prim_id || !desc->matrix_cam)),
              "vrh_rt_resolve_host: a depth format needs t and the depth array, and prim_id with the matrix camera");
    float mats[32], inv[32];
    resolve_frame f;
    const int rc = desc_frame(desc, w, h, format->depth_format, "vrh_rt_resolve_host", mats, inv, f);
    if (rc) return rc;
    resolve_params P;
    fill_resolve_params(P, w, h, f);
    resolve_host(format->color_format, format->depth_format, P, color, prim_id, t, color_out, depth_out);
    return VRH_OK;
}

// ---- the volume kernels into a formatted target ------------------------------------------------------

VRH_API int vrh_render_volume(vrh_ctx* ctx, const vrh_volume* v, vrh_rt* rt, const vrh_camera* cam,
                              const vrh_volume_kernel_desc* kd)
{
    int rc = resolve_refuse(rt, false, "vrh_render_volume");
    if (rc) return rc;
    rc = vrh_render_volume_frame(ctx, v, rt, cam, kd);
    if (rc || !rt->formatted) return rc;
    resolve_frame f{};
    volume_clip(*cam, f.clip);
    f.s = 1.0f;
    return resolve_enqueue(rt, f, ctx->stream);
}

VRH_API int vrh_render_multi_volume(vrh_ctx* ctx, const vrh_volume* const* volumes, const vrh_multi_volume_entry* entries,
                                    uint32_t n, vrh_rt* rt, const vrh_camera* cam, const vrh_multi_volume_kernel_desc* kd)
{
    int rc = resolve_refuse(rt, false, "vrh_render_multi_volume");
    if (rc) return rc;
    rc = vrh_render_multi_volume_frame(ctx, volumes, entries, n, rt, cam, kd);
    if (rc || !rt->formatted) return rc;
    resolve_frame f{};
    volume_clip(*cam, f.clip);
    f.s = 1.0f;
    return resolve_enqueue(rt, f, ctx->stream);
}

} // extern "C"
