// visionaray_amd/csrc/vrh_volume.hip -- the volume kernel (include/vrh.h vrh_render_volume) and the device
// objects around it: the ray marcher of src/examples/volume/main.cpp:123-167 as a stand-alone kernel -- not
// an instance of render_unified_kernel, no launch plan: its hot path is the sampler's scattered voxel
// loads, a dependent transfer-function load and a loop whose length differs per lane.
//
// One ray per lane, one 8 x 8 pixel tile per wave (neighbouring lanes sample neighbouring voxels), four
// tiles (16 x 16 pixels) per block.  The loop body is visionaray_hip/detail/vrh_volume.h march(): the eight
// voxel loads of a step are issued before the first use.  A transfer function of at most VOLUME_TF_LDS
// entries (1024: 16 KB) is staged in LDS once per block; a larger one is read from global memory.  Each
// wave adds its step count to the context's volume counters with one vector atomic at exit.
// VRH_VOLUME_BLOCK_WAVES (4 or 1) and VRH_VOLUME_TF_LDS are build-time choices for A/B builds: one wave per
// block and a transfer function left in global memory both measured the same frame time.
#include "vrh_volobj.h"

#include <new>

using namespace vrh;

namespace vrh {

// waves (8 x 8 tiles) per block, and the largest transfer function staged in LDS: 16 bytes per entry and block
#ifndef VRH_VOLUME_BLOCK_WAVES
#define VRH_VOLUME_BLOCK_WAVES 4
#endif
constexpr uint32_t VOLUME_WAVES = VRH_VOLUME_BLOCK_WAVES;
static_assert(VOLUME_WAVES == 1 || VOLUME_WAVES == 4, "one tile, or 2 x 2 tiles per block");
constexpr uint32_t VOLUME_THREADS = 64u * VOLUME_WAVES;
constexpr uint32_t VOLUME_TILES_SIDE = VOLUME_WAVES == 4 ? 2u : 1u;
#ifndef VRH_VOLUME_TF_LDS
#define VRH_VOLUME_TF_LDS (256u * VRH_VOLUME_BLOCK_WAVES)
#endif
constexpr uint32_t VOLUME_TF_LDS = VRH_VOLUME_TF_LDS;

struct volume_params
{
    dev::vol_view vol;
    dev::tf_view tf;
    dev::march_params K;
    float eye[3], cu[3], cv[3], cw[3];
    float wf, hf;
    uint32_t width;                               // row pitch of the target in pixels
    uint32_t clip[4];                             // x0, y0, x1, y1
    uint32_t blocks_x;
    float4* color;
    uint32_t* prim_id;
    float* t;
    unsigned long long* counters;                 // running totals: [0] steps, [1] waves with a capped ray
};

template <uint32_t FMT, bool TF_LDS>
__global__ __launch_bounds__(VOLUME_THREADS) void volume_kernel(const volume_params P)
{
    __shared__ dev::rgba_t s_tf[TF_LDS ? VOLUME_TF_LDS : 1];
    if (TF_LDS)
    {
        for (uint32_t i = threadIdx.x; i < uint32_t(P.tf.size); i += VOLUME_THREADS) s_tf[i] = P.tf.entries[i];
        __syncthreads();
    }
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t bx = blockIdx.x % P.blocks_x, by = blockIdx.x / P.blocks_x;
    const uint32_t x = P.clip[0] + (bx * VOLUME_TILES_SIDE + (wave & 1u)) * 8u + (lane & 7u);
    const uint32_t y = P.clip[1] + (by * VOLUME_TILES_SIDE + (wave >> 1)) * 8u + (lane >> 3);
    const bool active = x < P.clip[2] && y < P.clip[3];
    uint32_t steps = 0;
    bool capped = false;
    if (active)
    {
        float dir[3], tnear, tfar;
        dev::pinhole_dir(dir, P.cu, P.cv, P.cw, x, y, P.wf, P.hf);
        const bool hit = dev::box_clip(P.eye, dir, P.K.bmin, P.K.bmax, tnear, tfar);
        dev::rgba_t c;
        if (TF_LDS) steps = dev::march<FMT>(P.vol, P.tf, s_tf, P.K, P.eye, dir, tnear, tfar, c, capped);
        else steps = dev::march<FMT>(P.vol, P.tf, P.tf.entries, P.K, P.eye, dir, tnear, tfar, c, capped);
        const size_t o = size_t(y) * P.width + x;
        P.color[o] = make_float4(c.x, c.y, c.z, c.w);
        if (P.prim_id) P.prim_id[o] = hit ? 0u : 0xFFFFFFFFu;
        if (P.t) P.t[o] = hit ? tnear : -1.0f;
    }
    // the wave's steps: every lane of the wave is here
    uint32_t sum = steps;
    for (int m = 32; m > 0; m >>= 1) sum += __shfl_xor(sum, m, 64);
    const bool any_capped = __any(capped);
    if (lane == 0)
    {
        if (sum) atomicAdd(&P.counters[0], (unsigned long long)sum);
        if (any_capped) atomicAdd(&P.counters[1], 1ull);
    }
}

__global__ void volume_sample_kernel(const dev::vol_view vol, const dev::tf_view tf, const float* coords, uint32_t n,
                                     float* voxel_out, dev::rgba_t* rgba_out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = dev::tex3d(vol, coords[3 * size_t(i)], coords[3 * size_t(i) + 1], coords[3 * size_t(i) + 2]);
    if (voxel_out) voxel_out[i] = v;
    if (rgba_out) rgba_out[i] = dev::tex1d(tf, tf.entries, v);
}

template <uint32_t FMT>
void launch_volume(const volume_params& p, uint32_t blocks, hipStream_t s)
{
    if (uint32_t(p.tf.size) <= VOLUME_TF_LDS) hipLaunchKernelGGL((volume_kernel<FMT, true>), dim3(blocks), dim3(VOLUME_THREADS), 0, s, p);
    else hipLaunchKernelGGL((volume_kernel<FMT, false>), dim3(blocks), dim3(VOLUME_THREADS), 0, s, p);
}

// after the context stream was waited for: the counters of a volume frame not yet looked at -- the copy
// of the running totals that the frame left in pinned host memory, less the totals before it; a frame
// that was stopped by its step limit is reported once
int volume_collect(vrh_ctx* ctx)
{
    if (!ctx->vol_pending) return VRH_OK;
    const unsigned long long c[2] = { ctx->vol_host[0], ctx->vol_host[1] };
    ctx->vol_pending = false;
    ctx->vol_steps = c[0] - ctx->vol_base[0];
    ctx->vol_capped = c[1] != ctx->vol_base[1];
    ctx->vol_base[0] = c[0]; ctx->vol_base[1] = c[1];
    if (ctx->vol_capped)
    {
        set_error("a volume frame was stopped by the device's step limit: its pixels are not complete");
        return VRH_ERR_INVALID;
    }
    return VRH_OK;
}

int volume_frame_begin(vrh_ctx* ctx, vrh_rt* rt)
{
    if (!ctx->vol_counters)
    {
        // running totals on the device, and the pinned host words every frame's copy of them lands in
        unsigned long long* c = nullptr;
        VRH_HIP(hipMalloc(&c, 2 * sizeof(unsigned long long)));
        hipError_t e = hipMemset(c, 0, 2 * sizeof(unsigned long long));
        if (e == hipSuccess) e = hipHostMalloc(reinterpret_cast<void**>(&ctx->vol_host), 2 * sizeof(unsigned long long), hipHostMallocDefault);
        if (e != hipSuccess) { (void)hipFree(c); set_error(hipGetErrorString(e)); return VRH_ERR_HIP; }
        ctx->vol_host[0] = ctx->vol_host[1] = 0;
        ctx->vol_counters = c;
    }
    // ordered after every frame issued so far and after a render group's writes into the target
    VRH_HIP(ctx_join(ctx));
    if (rt->written_pending) VRH_HIP(hipStreamWaitEvent(ctx->stream, rt->written, 0));
    if (ctx->vol_pending)
    {
        // the previous volume frame's flag must not be lost: look at it before the counters are reset
        VRH_HIP(hipStreamSynchronize(ctx->stream));
        const int rc = volume_collect(ctx);
        if (rc) return rc;
    }
    return VRH_OK;
}

int volume_frame_end(vrh_ctx* ctx)
{
    VRH_HIP(hipMemcpyAsync(ctx->vol_host, ctx->vol_counters, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    ctx->vol_pending = true;
    return VRH_OK;
}

} // namespace vrh

namespace {

int upload_transfunc(vrh_volume* v, const vrh_transfunc_desc& td)
{
    dev::rgba_t* e = nullptr;
    VRH_HIP(hipMalloc(&e, size_t(td.size) * 16));
    const hipError_t c = hipMemcpy(e, td.rgba, size_t(td.size) * 16, hipMemcpyHostToDevice);
    if (c != hipSuccess) { (void)hipFree(e); set_error(hipGetErrorString(c)); return VRH_ERR_HIP; }
    if (v->entries) (void)hipFree(v->entries);
    v->entries = e;
    v->tf = dev::make_tf_view(e, td.size, td.filter, td.address);
    return VRH_OK;
}

} // namespace

extern "C" {

VRH_API int vrh_volume_create(vrh_ctx* ctx, const vrh_volume_desc* vd, const vrh_transfunc_desc* td, vrh_volume** out)
{
    VRH_CHECK(out, "vrh_volume_create: null out");
    *out = nullptr;
    VRH_CHECK(vd && td, "vrh_volume_create: null descriptor");
    std::string bad = check_volume_desc(*vd);
    if (bad.empty()) bad = check_transfunc_desc(*td);
    VRH_CHECK(bad.empty(), "vrh_volume_create: " + bad);
    VRH_CHECK(ctx, "vrh_volume_create: null context");
    VRH_HIP(hipSetDevice(ctx->device));
    auto* v = new (std::nothrow) vrh_volume;
    if (!v) { set_error("host allocation failed"); return VRH_ERR_OOM; }
    v->ctx = ctx;
    const size_t bytes = size_t(vd->width) * vd->height * vd->depth * voxel_bytes(vd->format);
    int rc = VRH_OK;
    do {
        hipError_t e = hipMalloc(&v->voxels, bytes);
        if (e != hipSuccess) { set_error(hipGetErrorString(e)); rc = e == hipErrorOutOfMemory ? VRH_ERR_OOM : VRH_ERR_HIP; break; }
        e = hipMemcpy(v->voxels, vd->voxels, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) { set_error(hipGetErrorString(e)); rc = VRH_ERR_HIP; break; }
        v->vol = dev::make_vol_view(v->voxels, vd->width, vd->height, vd->depth, vd->format, vd->filter, vd->address);
        rc = upload_transfunc(v, *td);
    } while (0);
    if (rc != VRH_OK) { vrh_volume_free(v); return rc; }
    *out = v;
    return VRH_OK;
}

VRH_API int vrh_volume_set_transfunc(vrh_volume* v, const vrh_transfunc_desc* td)
{
    VRH_CHECK(td, "vrh_volume_set_transfunc: null descriptor");
    const std::string bad = check_transfunc_desc(*td);
    VRH_CHECK(bad.empty(), "vrh_volume_set_transfunc: " + bad);
    VRH_CHECK(v && v->ctx, "vrh_volume_set_transfunc: null volume");
    VRH_HIP(hipSetDevice(v->ctx->device));
    // frames issued so far still read the old entries
    VRH_HIP(ctx_join(v->ctx));
    VRH_HIP(hipStreamSynchronize(v->ctx->stream));
    return upload_transfunc(v, *td);
}

VRH_API int vrh_volume_get_view(const vrh_volume* v, vrh_volume_view* out)
{
    VRH_CHECK(v && out, "vrh_volume_get_view: null");
    static_assert(sizeof(dev::vol_view) == sizeof(out->volume) && sizeof(dev::tf_view) == sizeof(out->transfunc), "view sizes");
    std::memcpy(out->volume, &v->vol, sizeof(out->volume));
    std::memcpy(out->transfunc, &v->tf, sizeof(out->transfunc));
    return VRH_OK;
}

VRH_API int vrh_volume_free(vrh_volume* v)
{
    if (!v) return VRH_OK;
    if (v->ctx)
    {
        (void)hipSetDevice(v->ctx->device);
        if (v->ctx->stream) (void)hipStreamSynchronize(v->ctx->stream);
    }
    if (v->voxels) (void)hipFree(v->voxels);
    if (v->entries) (void)hipFree(v->entries);
    delete v;
    return VRH_OK;
}

VRH_API int vrh_render_volume(vrh_ctx* ctx, const vrh_volume* v, vrh_rt* rt, const vrh_camera* cam,
                              const vrh_volume_kernel_desc* kd)
{
    // the hang guard comes first, before any object is looked at
    VRH_CHECK(cam && kd, "vrh_render_volume: null camera or kernel descriptor");
    volume_params p{};
    const std::string bad = check_volume_kernel(*kd, *cam, p.K);
    VRH_CHECK(bad.empty(), "vrh_render_volume: " + bad);
    VRH_CHECK(ctx && v && rt, "vrh_render_volume: null context, volume or target");
    VRH_CHECK(v->ctx == ctx && rt->ctx == ctx, "vrh_render_volume: the volume and the target belong to another context");
    VRH_CHECK(rt->color, "vrh_render_volume: the target has no colour buffer");
    VRH_CHECK(cam->width == rt->width && cam->height == rt->height,
              "vrh_render_volume: the camera's image size is not the target's (no shards)");
    VRH_HIP(hipSetDevice(ctx->device));
    const int rc = volume_frame_begin(ctx, rt);
    if (rc) return rc;
    p.vol = v->vol;
    p.tf = v->tf;
    for (int a = 0; a < 3; ++a) { p.eye[a] = cam->eye[a]; p.cu[a] = cam->cam_u[a]; p.cv[a] = cam->cam_v[a]; p.cw[a] = cam->cam_w[a]; }
    p.wf = float(cam->width); p.hf = float(cam->height);
    p.width = rt->width;
    volume_clip(*cam, p.clip);
    p.color = rt->color; p.prim_id = rt->prim_id; p.t = rt->t;
    p.counters = ctx->vol_counters;
    ctx->vol_rays = 0;
    if (p.clip[2] > p.clip[0] && p.clip[3] > p.clip[1])
    {
        const uint32_t w = p.clip[2] - p.clip[0], h = p.clip[3] - p.clip[1];
        const uint32_t side = 8u * VOLUME_TILES_SIDE;
        p.blocks_x = (w + side - 1u) / side;
        const uint32_t blocks = p.blocks_x * ((h + side - 1u) / side);
        ctx->vol_rays = uint64_t(w) * h;
        if (v->vol.format == VRH_VOL_R8) launch_volume<dev::VOL_R8>(p, blocks, ctx->stream);
        else if (v->vol.format == VRH_VOL_R16) launch_volume<dev::VOL_R16>(p, blocks, ctx->stream);
        else launch_volume<dev::VOL_R32F>(p, blocks, ctx->stream);
        VRH_HIP(hipGetLastError());
    }
    return volume_frame_end(ctx);
}

VRH_API int vrh_volume_last_stats(vrh_ctx* ctx, vrh_volume_stats* stats)
{
    VRH_CHECK(ctx && stats, "vrh_volume_last_stats: null");
    VRH_HIP(hipSetDevice(ctx->device));
    VRH_HIP(ctx_join(ctx));
    VRH_HIP(hipStreamSynchronize(ctx->stream));
    const int rc = volume_collect(ctx);
    stats->rays = ctx->vol_rays;
    stats->steps = ctx->vol_steps;
    stats->capped = ctx->vol_capped ? 1u : 0u;
    stats->reserved = 0;
    return rc;
}

VRH_API int vrh_volume_sample(vrh_ctx* ctx, const vrh_volume* v, const float* coords, uint32_t n, float* voxel_out,
                              float* rgba_out)
{
    VRH_CHECK(ctx && v && v->ctx == ctx, "vrh_volume_sample: null or foreign argument");
    if (n == 0) return VRH_OK;
    VRH_CHECK(coords, "vrh_volume_sample: null coordinates");
    const size_t bc = first_bad_coord(coords, size_t(n) * 3);
    VRH_CHECK(bc == size_t(n) * 3, "vrh_volume_sample: coordinate " + std::to_string(bc / 3) + " is not finite or exceeds 2^20 in magnitude");
    VRH_HIP(hipSetDevice(ctx->device));
    VRH_HIP(ctx_join(ctx));
    float* d = nullptr;                           // n x (3 coordinates, 1 voxel, 4 rgba)
    VRH_HIP(hipMalloc(&d, size_t(n) * 32));
    float* d_voxel = d + size_t(n) * 4;           // the rgba block first: 16-byte aligned
    dev::rgba_t* d_rgba = reinterpret_cast<dev::rgba_t*>(d);
    float* d_coords = d + size_t(n) * 5;
    int rc = VRH_OK;
    do {
        hipError_t e = hipMemcpyAsync(d_coords, coords, size_t(n) * 12, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) { set_error(hipGetErrorString(e)); rc = VRH_ERR_HIP; break; }
        hipLaunchKernelGGL(volume_sample_kernel, dim3((n + 255u) / 256u), dim3(256), 0, ctx->stream, v->vol, v->tf,
                           (const float*)d_coords, n, d_voxel, d_rgba);
        if ((e = hipGetLastError()) != hipSuccess) { set_error(hipGetErrorString(e)); rc = VRH_ERR_HIP; break; }
        if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) { set_error(hipGetErrorString(e)); rc = VRH_ERR_HIP; break; }
        if (voxel_out && (e = hipMemcpy(voxel_out, d_voxel, size_t(n) * 4, hipMemcpyDeviceToHost)) != hipSuccess)
        { set_error(hipGetErrorString(e)); rc = VRH_ERR_HIP; break; }
        if (rgba_out && (e = hipMemcpy(rgba_out, d_rgba, size_t(n) * 16, hipMemcpyDeviceToHost)) != hipSuccess)
        { set_error(hipGetErrorString(e)); rc = VRH_ERR_HIP; break; }
    } while (0);
    (void)hipFree(d);
    return rc;
}

} // extern "C"
