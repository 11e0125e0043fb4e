// visionaray_amd/csrc/vrh_multi_volume.hip -- the multi-volume kernel (include/vrh.h vrh_render_multi_volume): the
// functor of src/examples/multi_volume/main.cpp:410-567 as a stand-alone kernel of the shape of volume_kernel
// (vrh_volume.hip): one ray per lane, one 8 x 8 pixel tile per wave, four tiles per 256-thread block, a
// plain grid.  The loop is visionaray_hip/detail/vrh_multi_volume.h multi_march() with the wave's policies:
//
//   records   the per-volume records (views, matrix, box, material, light_dir) lie in a device array; the
//             loop indexes it with the lowest set bit of a mask built from wave-wide votes, made uniform for
//             the compiler with readfirstlane: a record is read with scalar loads, once per wave
//   ranges    a lane's tnear / tfar per volume live in dynamic LDS, [2 * volume + k][thread]: 2 KB per volume
//             and block (64 KB at 32 volumes), no bank conflicts, no scratch
//   culling   a volume no lane of the wave has a non-empty range for never enters the loop; within a step a
//             volume no lane is inside of is skipped
//
// The transfer functions stay in global memory.  Each wave adds its step count to the context's volume
// counters with one vector atomic at exit, as volume_kernel does.
#include "vrh_volobj.h"
#include "vrh_mvhost.h"

using namespace vrh;

namespace vrh {

constexpr uint32_t MV_THREADS = 256u;

struct mv_kernel_params
{
    const dev::mv_record* recs;
    dev::mv_params K;
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

struct mv_wave
{
    static __device__ __forceinline__ bool any(bool b) { return __any(b); }
};

// a lane's column of the block's dynamic LDS
struct mv_lds_ranges
{
    float* col;                                   // &lds[threadIdx.x]
    __device__ __forceinline__ void set(uint32_t i, float tn, float tf) { col[(2u * i) * MV_THREADS] = tn; col[(2u * i + 1u) * MV_THREADS] = tf; }
    __device__ __forceinline__ float tnear(uint32_t i) const { return col[(2u * i) * MV_THREADS]; }
    __device__ __forceinline__ float tfar(uint32_t i) const { return col[(2u * i + 1u) * MV_THREADS]; }
};

// the records through an index the compiler knows to be the same in every lane
struct mv_uniform_records
{
    const dev::mv_record* p;
    __device__ __forceinline__ const dev::mv_record& operator[](uint32_t i) const { return p[__builtin_amdgcn_readfirstlane(i)]; }
};

__global__ __launch_bounds__(MV_THREADS) void multi_volume_kernel(const mv_kernel_params P)
{
    extern __shared__ float s_ranges[];           // 2 * P.K.num * MV_THREADS floats
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t bx = blockIdx.x % P.blocks_x, by = blockIdx.x / P.blocks_x;
    const uint32_t x = P.clip[0] + (bx * 2u + (wave & 1u)) * 8u + (lane & 7u);
    const uint32_t y = P.clip[1] + (by * 2u + (wave >> 1)) * 8u + (lane >> 3);
    const bool active = x < P.clip[2] && y < P.clip[3];
    float dir[3];
    dev::pinhole_dir(dir, P.cu, P.cv, P.cw, x, y, P.wf, P.hf);
    mv_lds_ranges R{ s_ranges + threadIdx.x };
    const mv_uniform_records recs{ P.recs };
    const dev::mv_result r = dev::multi_march<mv_wave>(recs, P.K, P.eye, dir, active, R);
    if (active)
    {
        const size_t o = size_t(y) * P.width + x;
        P.color[o] = make_float4(r.color.x, r.color.y, r.color.z, r.color.w);
        if (P.prim_id) P.prim_id[o] = r.hit ? 0u : 0xFFFFFFFFu;
        if (P.t) P.t[o] = r.hit ? r.tmin : -1.0f;
    }
    // the wave's steps: every lane of the wave is here
    uint32_t sum = r.steps;
    for (int m = 32; m > 0; m >>= 1) sum += __shfl_xor(sum, m, 64);
    const bool any_capped = __any(r.capped);
    if (lane == 0)
    {
        if (sum) atomicAdd(&P.counters[0], (unsigned long long)sum);
        if (any_capped) atomicAdd(&P.counters[1], 1ull);
    }
}

} // namespace vrh

extern "C" {

VRH_API int vrh_render_multi_volume(vrh_ctx* ctx, const vrh_volume* const* volumes, const vrh_multi_volume_entry* entries,
                                    uint32_t n, vrh_rt* rt, const vrh_camera* cam, const vrh_multi_volume_kernel_desc* kd)
{
    // the descriptor checks and the hang guard come first, before any object is looked at
    VRH_CHECK(cam && kd, "vrh_render_multi_volume: null camera or kernel descriptor");
    mv_kernel_params p{};
    std::vector<dev::mv_record> recs;
    const std::string bad = check_multi_volume(entries, n, *kd, *cam, p.K, recs);
    VRH_CHECK(bad.empty(), "vrh_render_multi_volume: " + bad);
    VRH_CHECK(ctx && volumes && rt, "vrh_render_multi_volume: null context, volumes or target");
    for (uint32_t i = 0; i < n; ++i)
    {
        VRH_CHECK(volumes[i], "vrh_render_multi_volume: null volume " + std::to_string(i));
        VRH_CHECK(volumes[i]->ctx == ctx, "vrh_render_multi_volume: volume " + std::to_string(i) + " belongs to another context");
        recs[i].vol = volumes[i]->vol;
        recs[i].tf = volumes[i]->tf;
    }
    VRH_CHECK(rt->ctx == ctx, "vrh_render_multi_volume: the target belongs to another context");
    VRH_CHECK(rt->color, "vrh_render_multi_volume: the target has no colour buffer");
    VRH_CHECK(cam->width == rt->width && cam->height == rt->height,
              "vrh_render_multi_volume: the camera's image size is not the target's (no shards)");
    VRH_HIP(hipSetDevice(ctx->device));
    constexpr size_t block = sizeof(dev::mv_record) * dev::MULTI_VOLUME_MAX;
    if (!ctx->mv_records)
    {
        void* d = nullptr;
        VRH_HIP(hipMalloc(&d, block));
        const hipError_t e = hipHostMalloc(&ctx->mv_host, block, hipHostMallocDefault);
        if (e != hipSuccess) { (void)hipFree(d); ctx->mv_host = nullptr; set_error(hipGetErrorString(e)); return VRH_ERR_HIP; }
        ctx->mv_records = d;
    }
    const int rc = volume_frame_begin(ctx, rt);
    if (rc) return rc;
    // no volume frame is pending here, so nothing reads the pinned block any more
    std::memcpy(ctx->mv_host, recs.data(), sizeof(dev::mv_record) * n);
    VRH_HIP(hipMemcpyAsync(ctx->mv_records, ctx->mv_host, sizeof(dev::mv_record) * n, hipMemcpyHostToDevice, ctx->stream));
    // from here on the copy may be reading the pinned block: the frame counts as pending whatever follows, so the
    // next volume frame waits for the stream before it writes the block again (an error return below included)
    ctx->vol_pending = true;
    p.recs = static_cast<const dev::mv_record*>(ctx->mv_records);
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
        p.blocks_x = (w + 15u) / 16u;
        const uint32_t blocks = p.blocks_x * ((h + 15u) / 16u);
        ctx->vol_rays = uint64_t(w) * h;
        const size_t lds = size_t(2u * n) * MV_THREADS * sizeof(float);
        hipLaunchKernelGGL(multi_volume_kernel, dim3(blocks), dim3(MV_THREADS), lds, ctx->stream, p);
        VRH_HIP(hipGetLastError());
    }
    return volume_frame_end(ctx);
}

} // extern "C"
