// visionaray_amd/csrc/vrh_runtime.cpp -- the C-ABI of libvrh (include/vrh.h).
//
// Host-side runtime: contexts (device + stream + events + counters), scene upload with the
// MI355X layout transform (node pairs, leaf-ordered primitives), render targets, the frame launch
// (cuda_sched<R>::frame replacement, cuda_sched.inl:238-320), multi-GPU shard helpers and the
// host builder entry point.  Every HIP call is checked; nothing throws across the ABI.

#include "vrh_internal.h"
#include "vrh_kernels.h"
#include "vrh_plan.h"
#include "vrh_lbvh.h"
#include "vrh_texhost.h"
#include "vrh_resolve.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <new>
#include <string>
#include <vector>

namespace vrh {

static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }

} // namespace vrh

using namespace vrh;

#include "vrh_objects.h"

namespace {

int select_device(vrh_ctx* ctx)
{
    VRH_HIP(hipSetDevice(ctx->device));
    return VRH_OK;
}

// a scene under construction (vrh_scene_upload, vrh_scene_list_create, vrh_scene_build)
vrh_scene* new_scene(vrh_ctx* ctx)
{
    auto* sc = new (std::nothrow) vrh_scene;
    if (sc) sc->ctx = ctx;
    else set_error("host allocation failed");
    return sc;
}

// a HIP failure of entry point `who` at `what`: the scene and what it owns are freed
int scene_fail(vrh_scene* sc, hipError_t e, const char* who, const char* what)
{
    set_error(std::string(who) + ": " + what + ": " + hipGetErrorString(e));
    vrh_scene_free(sc);
    return e == hipErrorOutOfMemory ? VRH_ERR_OOM : VRH_ERR_HIP;
}

// one host block into a device array of the scene, counted in `total`
int scene_block(vrh_scene* sc, float4*& dst, const void* src, size_t bytes, uint64_t& total, const char* who, const char* what)
{
    hipError_t e = hipMalloc(&dst, bytes);
    if (e == hipSuccess) e = hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) return scene_fail(sc, e, who, what);
    total += bytes;
    return VRH_OK;
}

// the fields of vrh_scene_info that every kind of scene has
void scene_info(vrh_scene* sc, uint32_t bvhs, uint32_t nodes, uint32_t prims, uint32_t indices, uint32_t kind,
                uint32_t depth, uint32_t max_prim_id, uint32_t max_geom_id, uint64_t device_bytes)
{
    sc->info.num_bvhs = bvhs; sc->info.num_nodes = nodes; sc->info.num_prims = prims; sc->info.num_indices = indices;
    sc->info.prim_kind = kind; sc->info.max_depth = depth;
    sc->info.max_prim_id = max_prim_id; sc->info.max_geom_id = max_geom_id; sc->info.device_bytes = device_bytes;
}

// a render group's root writes its target on the group's stream (vrh_render_sharded): work on the
// target's context stream waits for that (an event wait, no host synchronisation)
int rt_wait(vrh_ctx* ctx, vrh_rt* rt)
{
    VRH_HIP(ctx_join(ctx));
    if (rt && rt->written_pending) VRH_HIP(hipStreamWaitEvent(ctx->stream, rt->written, 0));
    return VRH_OK;
}

// the context stream after every asynchronous frame, then the host after the stream
int ctx_drain(vrh_ctx* ctx)
{
    VRH_HIP(ctx_join(ctx));
    VRH_HIP(hipStreamSynchronize(ctx->stream));
    return VRH_OK;
}

} // namespace

extern "C" {

VRH_API const char* vrh_version(void) { return "visionaray-amd 0.1.0 (gfx950)"; }
VRH_API const char* vrh_last_error(void) { return g_last_error.c_str(); }

VRH_API int vrh_device_count(int* count)
{
    VRH_CHECK(count, "vrh_device_count: null");
    *count = 0;
    hipError_t e = hipGetDeviceCount(count);
    if (e != hipSuccess) { *count = 0; set_error(hipGetErrorString(e)); return VRH_ERR_NO_DEVICE; }
    return VRH_OK;
}

VRH_API int vrh_ctx_create_on_stream(int hip_device, void* hip_stream, vrh_ctx** out)
{
    VRH_CHECK(out, "vrh_ctx_create: null out");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { set_error("no HIP device visible"); return VRH_ERR_NO_DEVICE; }
    VRH_CHECK(hip_device >= 0 && hip_device < n, "vrh_ctx_create: device index out of range");
    auto* ctx = new (std::nothrow) vrh_ctx;
    if (!ctx) { set_error("host allocation failed"); return VRH_ERR_OOM; }
    ctx->device = hip_device;
    int rc = VRH_OK;
    do {
        if ((rc = select_device(ctx)) != VRH_OK) break;
        hipDeviceProp_t prop;
        hipError_t e = hipGetDeviceProperties(&prop, hip_device);
        if (e != hipSuccess) { set_error(hipGetErrorString(e)); rc = VRH_ERR_HIP; break; }
        ctx->num_cus = prop.multiProcessorCount;
        if (hip_stream) ctx->stream = static_cast<hipStream_t>(hip_stream);
        else
        {
            // a blocking stream (round 6): like the default stream cuda_sched launches on
            // (cuda_sched.inl:306-320), it is ordered against work on the NULL stream -- a program that
            // reads a target with a plain hipMemcpy after an asynchronous frame() sees the frame
            e = hipStreamCreateWithFlags(&ctx->stream, hipStreamDefault);
            if (e != hipSuccess) { set_error(hipGetErrorString(e)); rc = VRH_ERR_HIP; break; }
            ctx->own_stream = true;
        }
        // one counter block for frames on the context stream, one per frame lane (asynchronous frames)
        e = hipMalloc(&ctx->counters, COUNTER_BLOCKS * COUNTERS_WORDS * sizeof(unsigned long long));
        if (e != hipSuccess) { set_error(hipGetErrorString(e)); rc = VRH_ERR_OOM; break; }
        e = hipMemset(ctx->counters, 0, COUNTER_BLOCKS * COUNTERS_WORDS * sizeof(unsigned long long));
        if (e != hipSuccess) { set_error(hipGetErrorString(e)); rc = VRH_ERR_HIP; break; }
        ctx->last_counters = ctx->counters;
        for (int i = 0; i < VRH_MAX_FRAME_LANES; ++i) ctx->lane[i].counters = ctx->counters + size_t(i + 1) * COUNTERS_WORDS;
    } while (0);
    if (rc != VRH_OK) { vrh_ctx_destroy(ctx); return rc; }
    *out = ctx;
    return VRH_OK;
}

VRH_API int vrh_ctx_create(int hip_device, vrh_ctx** out) { return vrh_ctx_create_on_stream(hip_device, nullptr, out); }

VRH_API int vrh_ctx_get_stream(const vrh_ctx* ctx, int* hip_device, void** hip_stream)
{
    VRH_CHECK(ctx, "vrh_ctx_get_stream: null context");
    // work the caller issues on the stream comes after every frame issued so far (asynchronous frames)
    bool lanes_used = false;
    for (const auto& l : ctx->lane) lanes_used |= l.used;
    if (hip_stream && lanes_used)
    {
        VRH_HIP(hipSetDevice(ctx->device));
        VRH_HIP(ctx_join(ctx));
    }
    if (hip_device) *hip_device = ctx->device;
    if (hip_stream) *hip_stream = ctx->stream;
    return VRH_OK;
}

VRH_API int vrh_ctx_destroy(vrh_ctx* ctx)
{
    if (!ctx) return VRH_OK;
    (void)hipSetDevice(ctx->device);
    for (auto& l : ctx->lane)
        if (l.stream) (void)hipStreamSynchronize(l.stream);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (auto& l : ctx->lane)
    {
        if (l.spill) (void)hipFree(l.spill);
        for (void* q : { (void*)l.color, (void*)l.prim_id, (void*)l.t, (void*)l.occ })
            if (q) (void)hipFree(q);
        if (l.done) (void)hipEventDestroy(l.done);
        if (l.stream) (void)hipStreamDestroy(l.stream);
    }
    if (ctx->main_mark) (void)hipEventDestroy(ctx->main_mark);
    if (ctx->counters) (void)hipFree(ctx->counters);
    if (ctx->vol_counters) (void)hipFree(ctx->vol_counters);
    if (ctx->vol_host) (void)hipHostFree(ctx->vol_host);
    if (ctx->mv_records) (void)hipFree(ctx->mv_records);
    if (ctx->mv_host) (void)hipHostFree(ctx->mv_host);
    if (ctx->wave_times) (void)hipFree(ctx->wave_times);
    if (ctx->user_queues) (void)hipFree(ctx->user_queues);
    if (ctx->user_declined) (void)hipHostFree(ctx->user_declined);
    if (ctx->tile_times) (void)hipFree(ctx->tile_times);
    if (ctx->spill) (void)hipFree(ctx->spill);
    for (auto e : ctx->ev_start) (void)hipEventDestroy(e);
    for (auto e : ctx->ev_stop) (void)hipEventDestroy(e);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return VRH_OK;
}

// the accepted range of every option (0 = automatic wherever a range starts at 0); checked on the
// int64 value before it is narrowed, so a negative or huge value is refused, never wrapped
struct option_range { uint32_t option; int64_t lo, hi; const char* what; };
constexpr option_range k_option_ranges[] = {
    { VRH_OPT_BLOCK_THREADS, 0, 256, "block threads is 0 (auto) or a multiple of 64 up to 256" },
    { VRH_OPT_STACK_CAP, 0, 640, "stack cap is 0 (auto) or 1..640 LDS entries per lane" },
    { VRH_OPT_AO_SCHEDULE, 0, 4, "schedule is 0 (auto) or 3 (step loop)" },
    { VRH_OPT_BLOCKS_PER_CU, 0, 32, "blocks per CU is 0 (auto) or 1..32" },
    { VRH_OPT_WAVES_PER_SIMD, 0, 8, "waves per SIMD is 0 (auto), 1, 5, 6 or 8" },
    { VRH_OPT_EXACT_MINMAX, 0, 1, "exact min/max is 0 (auto) or 1 (on)" },
    { VRH_OPT_XCD_QUEUES, 0, 4, "xcd queues is 0 (auto), 1 (strips), 2 (off), 3 (band-interleaved) or 4 (cluster order)" },
    { VRH_OPT_REFILL_MIN, 0, 64, "refill threshold is 0 (auto) or 1..64" },
    { VRH_OPT_WIDE_ANYHIT, 0, 2, "wide any-hit is 0 (auto), 1 (on) or 2 (off)" },
    { VRH_OPT_DESCENT_CAP, 0, 1024, "descent cap is 0 (auto) or 1..1024" },
    { VRH_OPT_POP_ON_MISS, 0, 2, "pop on miss is 0 (auto), 1 (on) or 2 (off)" },
    { VRH_OPT_COOP_FETCH, 0, 2, "cooperative fetch was removed (0 / 2 = off is accepted)" },
    { VRH_OPT_SCALAR_FETCH, 0, 2, "scalar fetch is 0 (auto), 1 (on) or 2 (off)" },
    { VRH_OPT_PAIR_LAYOUT, 0, 2, "pair layout is 0 (auto), 1 (line pairing) or 2 (builder order)" },
    { VRH_OPT_AO_GATE, 0, 2, "AO gate is 0 (auto), 1 (on) or 2 (off)" },
    { VRH_OPT_WAVE_TIMES, 0, 2, "wave times is 0 (off), 1 (on) or 2 (on + tile times of counting one-frame AO launches)" },
    { VRH_OPT_AO_CUT, 0, 3, "AO cut is 0 (auto), 1 (on, entries nearest-first), 2 (off) or 3 (on, entries in cut order)" },
    { VRH_OPT_AO_STEAL, 0, 2, "AO tail stash was removed (0 / 2 = off is accepted)" },
    { VRH_OPT_AO_SHARE, 0, 2, "AO tail sharing is 0 (auto), 1 (on) or 2 (off)" },
    { VRH_OPT_CLUSTER_TILES, 0, 1024, "cluster tiles is 0 (auto) or 1..1024" },
    { VRH_OPT_QUAD_REFILL, 0, 1, "the quad-coherent hand-out was removed (0 is accepted)" },
    { VRH_OPT_GROUP_UNITS, 0, 1, "the block-shared hand-out was removed (0 is accepted)" },
    { VRH_OPT_FUSED_STEP, 0, 2, "fused step is 0 (auto), 1 (on) or 2 (off)" },
    { VRH_OPT_FUSED_WIDEN, 0, 30, "fused widening is 0 (the derived widening) or 1..30 (at least the scene extent x 2^-value)" },
    { VRH_OPT_ASYNC_FRAMES, 0, VRH_MAX_FRAME_LANES, "asynchronous frames is 0 (off), 1 (on, the default number of frame lanes) or 2..4 (on, that many frame lanes)" },
};

VRH_API int vrh_ctx_set_option(vrh_ctx* ctx, uint32_t option, int64_t value)
{
    VRH_CHECK(ctx, "vrh_ctx_set_option: null");
    const option_range* range = nullptr;
    for (const option_range& r : k_option_ranges)
        if (r.option == option) range = &r;
    if (!range) { set_error("vrh_ctx_set_option: unknown option"); return VRH_ERR_INVALID; }
    VRH_CHECK(value >= range->lo && value <= range->hi,
              std::string("vrh_ctx_set_option: value ") + std::to_string(value) + " out of range: " + range->what);
    const int v = int(value);
    switch (option)
    {
    case VRH_OPT_BLOCK_THREADS:
        // the traversal kernels are compiled for at most 256 threads per block (__launch_bounds__(256, ...)):
        // a larger block would break the register allocation's assumptions (a launch failure)
        VRH_CHECK(v % 64 == 0, std::string("vrh_ctx_set_option: ") + range->what);
        ctx->opt.block = v; break;
    case VRH_OPT_STACK_CAP: ctx->opt.stack = v; break;
    case VRH_OPT_AO_SCHEDULE:
        // the item loop (4) was removed in round 2: the step loop measured faster for every kernel
        if (v == 4) { set_error("vrh_ctx_set_option: the item-loop schedule was removed (the step loop is faster, profiles/r02_ab/ab18_sphere_schedule.log)"); return VRH_ERR_UNSUPPORTED; }
        VRH_CHECK(v == 0 || v == 3, std::string("vrh_ctx_set_option: ") + range->what); break;     // accepted; every kernel runs the step loop
    case VRH_OPT_WIDE_ANYHIT: ctx->opt.wide = v; break;
    case VRH_OPT_DESCENT_CAP: ctx->opt.dcap = v; break;
    case VRH_OPT_COOP_FETCH:
        // the cooperative quad fetch was removed in round 2 (measured slower, profiles/r01/ab_nocoop.log)
        if (v == 1) { set_error("vrh_ctx_set_option: the cooperative fetch was removed (it measured slower)"); return VRH_ERR_UNSUPPORTED; }
        break;
    case VRH_OPT_WAVE_TIMES: ctx->opt_wave_times = v; break;
    case VRH_OPT_AO_CUT: ctx->opt.cut = v; break;
    case VRH_OPT_AO_STEAL:
        // the AO tail stash was removed in round 3 (measured slower)
        if (v == 1) { set_error("vrh_ctx_set_option: the AO tail stash was removed (it measured slower)"); return VRH_ERR_UNSUPPORTED; }
        break;
    case VRH_OPT_AO_SHARE: ctx->opt.share = v; break;
    case VRH_OPT_AO_GATE: ctx->opt.gate = v; break;
    case VRH_OPT_POP_ON_MISS: ctx->opt.pop = v; break;
    case VRH_OPT_PAIR_LAYOUT: ctx->opt.layout = v; break;
    case VRH_OPT_FUSED_WIDEN: ctx->opt_fused_widen = v; break;
    case VRH_OPT_FUSED_STEP: ctx->opt_fused_step = v; break;
    case VRH_OPT_SCALAR_FETCH: ctx->opt.scalar = v; break;
    case VRH_OPT_REFILL_MIN: ctx->opt.refill = v; break;
    case VRH_OPT_BLOCKS_PER_CU: ctx->opt.bpc = v; break;
    case VRH_OPT_WAVES_PER_SIMD:
        VRH_CHECK(v == 0 || v == 1 || v == 5 || v == 6 || v == 8, std::string("vrh_ctx_set_option: ") + range->what);
        ctx->opt.occ = v; break;
    case VRH_OPT_EXACT_MINMAX: ctx->opt.exact_minmax = v; break;
    case VRH_OPT_XCD_QUEUES: ctx->opt.xcd_queues = v; break;
    case VRH_OPT_GROUP_UNITS:
    case VRH_OPT_QUAD_REFILL:
        // measured in round 4 and removed (slower: profiles/r04/ab/lane_layout/); 0 is accepted
        if (v != 0) { set_error("vrh_ctx_set_option: the quad-coherent and block-shared hand-outs were removed (they measured slower)"); return VRH_ERR_UNSUPPORTED; }
        break;
    case VRH_OPT_ASYNC_FRAMES:
    {
        // a different lane count: every frame issued so far is joined into the context stream first
        const uint32_t lanes = v == 1 ? uint32_t(VRH_DEFAULT_FRAME_LANES) : v > 1 ? uint32_t(v) : ctx->num_lanes;
        if (lanes != ctx->num_lanes)
        {
            VRH_HIP(hipSetDevice(ctx->device));
            VRH_HIP(ctx_join(ctx));
            ctx->num_lanes = lanes;
            ctx->next_lane = 0;
        }
        ctx->opt_async = v ? 1 : 0;
        break;
    }
    case VRH_OPT_CLUSTER_TILES: ctx->opt.cluster = v; break;
    default: set_error("vrh_ctx_set_option: unknown option"); return VRH_ERR_INVALID;
    }
    return VRH_OK;
}

// ---- scene upload -------------------------------------------------------------------------------

VRH_API int vrh_scene_upload(vrh_ctx* ctx, const void* nodes_v, uint32_t num_nodes, const void* prims_v,
                             uint32_t num_prims, uint32_t prim_kind, const uint32_t* indices, uint32_t num_indices,
                             const void* face_normals, vrh_scene** out)
{
    VRH_CHECK(ctx && out && nodes_v && prims_v, "vrh_scene_upload: null argument");
    VRH_CHECK(num_nodes >= 1 && num_prims >= 1, "vrh_scene_upload: empty BVH");
    *out = nullptr;
    // validation and the device layouts are host work (vrh_upload.cpp); what differs between the libraries built from
    // this file goes in as options: fused records for a VRH_FUSED_STEP build, never-hit unused entries for the default
    const upload_options opt{ ctx->opt.layout, ctx->opt_fused_widen, VRH_FUSED_STEP != 0 && ctx->opt_fused_step != 2,
                              vrh::dev::NEVER_HIT_UNUSED };
    prepared_scene p;
    std::string err;
    int rc = prepare_scene(nodes_v, num_nodes, prims_v, num_prims, prim_kind, indices, num_indices, opt, p, err);
    if (rc) { set_error(err); return rc; }
    // the kernels read face_normals[prim_id], and num_prims rows are copied
    VRH_CHECK(!face_normals || p.max_prim_id < num_prims,
              "vrh_scene_upload: face normals are indexed by prim_id, but prim_id " + std::to_string(p.max_prim_id)
                  + " is not below num_prims " + std::to_string(num_prims));
    if ((rc = select_device(ctx))) return rc;
    vrh_scene* sc = new_scene(ctx);
    if (!sc) return VRH_ERR_OOM;
    sc->roots[0] = p.root;
    sc->num_pairs = p.num_pairs;
    sc->finite_bounds = p.finite_bounds;
    const char* who = "vrh_scene_upload";
    auto bytes_of = [](const std::vector<float>& v) { return v.size() * sizeof(float); };
    uint64_t bytes = 0, fused_bytes = 0;       // the fused arrays are not part of device_bytes, which the launch plan reads
    if ((rc = scene_block(sc, sc->pairs, p.pairs.data(), bytes_of(p.pairs), bytes, who, "pairs"))) return rc;
    if ((rc = scene_block(sc, sc->prims, p.prims.data(), bytes_of(p.prims), bytes, who, "prims"))) return rc;
    if (p.have_quads && (rc = scene_block(sc, sc->quads, p.quads.data(), bytes_of(p.quads), bytes, who, "quads"))) return rc;
    if (p.fused_built)
    {
        if ((rc = scene_block(sc, sc->fquads, p.fused_recs.data(), bytes_of(p.fused_recs), fused_bytes, who, "fused records"))) return rc;
        if ((rc = scene_block(sc, sc->leaf_boxes, p.leaf_boxes.data(), bytes_of(p.leaf_boxes), fused_bytes, who, "leaf boxes"))) return rc;
        sc->fused_omax = p.fused_omax;
        sc->info.fused_records = uint32_t(p.quads.size() / 32);
        sc->info.fused_bytes = fused_bytes;
    }
    if (face_normals && (rc = scene_block(sc, sc->normals, face_normals, size_t(num_prims) * sizeof(float4), bytes, who, "normals"))) return rc;
    sc->quad_depth = sc->info.wide_depth = p.quad_depth;
    sc->info.wide_records = uint32_t(p.quads.size() / 32);
    scene_info(sc, 1, num_nodes, num_prims, p.num_indices, prim_kind, p.max_depth, p.max_prim_id, p.max_geom_id, bytes);
    *out = sc;
    return VRH_OK;
}

VRH_API int vrh_scene_get_info(const vrh_scene* scene, vrh_scene_info* info)
{
    VRH_CHECK(scene && info, "vrh_scene_get_info: null");
    *info = scene->info;
    return VRH_OK;
}

VRH_API int vrh_scene_get_view(const vrh_scene* scene, uint32_t bvh, vrh_scene_view* out)
{
    VRH_CHECK(scene && out, "vrh_scene_get_view: null");
    VRH_CHECK(bvh < scene->num_roots, "vrh_scene_get_view: bvh index out of range");
    vrh_scene_view v{};
    v.pairs = scene->pairs;
    v.prims = scene->prims;
    v.normals = scene->normals;
    v.root = scene->roots[bvh];
    v.max_depth = scene->info.max_depth;
    v.prim_kind = scene->info.prim_kind;
    v.finite_bounds = scene->finite_bounds ? 1u : 0u;
    v.num_prims = scene->info.num_indices;
    if (scene->quads && scene->num_roots == 1 && scene->finite_bounds)
    {
        v.quads = scene->quads;
        v.quad_depth = scene->quad_depth;
    }
    *out = v;
    return VRH_OK;
}

VRH_API int vrh_scene_free(vrh_scene* sc)
{
    if (!sc) return VRH_OK;
    if (sc->ctx) (void)hipSetDevice(sc->ctx->device);
    if (sc->pairs) (void)hipFree(sc->pairs);
    if (sc->prims) (void)hipFree(sc->prims);
    if (sc->normals) (void)hipFree(sc->normals);
    if (sc->quads) (void)hipFree(sc->quads);
    if (sc->fquads) (void)hipFree(sc->fquads);
    if (sc->leaf_boxes) (void)hipFree(sc->leaf_boxes);
    if (sc->vnormals) (void)hipFree(sc->vnormals);
    if (sc->dnodes) (void)hipFree(sc->dnodes);
    if (sc->dindices) (void)hipFree(sc->dindices);
    delete sc;
    return VRH_OK;
}

namespace {
// scene lists: the pair records of one member re-based into the combined arrays (inner links by
// the member's first pair, leaf links by its first primitive)
__global__ void rebase_links_kernel(float4* pairs, uint32_t n, uint32_t pair_off, uint32_t prim_off)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t* w = reinterpret_cast<uint32_t*>(pairs + 4u * size_t(i) + 3u);
    for (int c = 0; c < 2; ++c)
        w[c] = (w[c] & 0x80000000u) ? (0x80000000u | ((w[c] & 0x7FFFFFFFu) + prim_off)) : w[c] + pair_off;
}
} // namespace

VRH_API int vrh_scene_list_create(vrh_ctx* ctx, const vrh_scene* const* scenes, uint32_t count,
                                  const void* face_normals, uint32_t num_normals, vrh_scene** out)
{
    VRH_CHECK(ctx && scenes && out, "vrh_scene_list_create: null argument");
    VRH_CHECK(count >= 1 && count <= VRH_MAX_SCENE_LIST, "vrh_scene_list_create: 1..VRH_MAX_SCENE_LIST scenes");
    *out = nullptr;
    uint64_t pairs = 0, prims = 0, nodes = 0, bytes = 0;
    uint32_t kind = scenes[0] ? scenes[0]->info.prim_kind : 0u, depth = 0, max_pid = 0, max_gid = 0;
    bool finite = true;
    for (uint32_t i = 0; i < count; ++i)
    {
        const vrh_scene* m = scenes[i];
        VRH_CHECK(m && m->ctx == ctx, "vrh_scene_list_create: scene missing or of another context");
        VRH_CHECK(m->num_roots == 1, "vrh_scene_list_create: members must be single BVHs");
        if (m->info.prim_kind == VRH_PRIM_GENERIC80)
        {
            set_error("vrh_scene_list_create: BVH lists take triangle or sphere scenes, not generic-primitive scenes");
            return VRH_ERR_UNSUPPORTED;
        }
        VRH_CHECK(m->info.prim_kind == kind, "vrh_scene_list_create: members must share one primitive type");
        pairs += m->num_pairs;
        prims += m->info.num_indices;
        nodes += m->info.num_nodes;
        depth = std::max(depth, m->info.max_depth);
        max_pid = std::max(max_pid, m->info.max_prim_id);
        max_gid = std::max(max_gid, m->info.max_geom_id);
        finite = finite && m->finite_bounds;
    }
    VRH_CHECK(pairs < 0x80000000ull && prims < 0x80000000ull && nodes < 0xFFFFFFF0ull, "vrh_scene_list_create: list too large");
    VRH_CHECK(!face_normals || uint64_t(num_normals) > max_pid, "vrh_scene_list_create: face normals must cover every prim_id");
    int rc = select_device(ctx);
    if (rc) return rc;
    vrh_scene* sc = new_scene(ctx);
    if (!sc) return VRH_ERR_OOM;
    auto fail = [&](hipError_t e, const char* what) { return scene_fail(sc, e, "vrh_scene_list_create", what); };
    const uint32_t f4_per = leaf_record_bytes(kind) / 16;
    hipError_t e;
    if ((e = hipMalloc(&sc->pairs, std::max<uint64_t>(pairs, 1) * 64)) != hipSuccess) return fail(e, "pairs");
    if ((e = hipMalloc(&sc->prims, prims * f4_per * 16)) != hipSuccess) return fail(e, "prims");
    uint32_t pair_off = 0, prim_off = 0;
    for (uint32_t i = 0; i < count; ++i)
    {
        const vrh_scene* m = scenes[i];
        if (m->num_pairs)
        {
            if ((e = hipMemcpyAsync(sc->pairs + 4u * size_t(pair_off), m->pairs, size_t(m->num_pairs) * 64,
                                    hipMemcpyDeviceToDevice, ctx->stream)) != hipSuccess) return fail(e, "copy pairs");
            hipLaunchKernelGGL(rebase_links_kernel, dim3((m->num_pairs + 255u) / 256u), dim3(256), 0, ctx->stream,
                               sc->pairs + 4u * size_t(pair_off), m->num_pairs, pair_off, prim_off);
            if ((e = hipGetLastError()) != hipSuccess) return fail(e, "rebase");
        }
        if ((e = hipMemcpyAsync(sc->prims + size_t(f4_per) * prim_off, m->prims, size_t(m->info.num_indices) * f4_per * 16,
                                hipMemcpyDeviceToDevice, ctx->stream)) != hipSuccess) return fail(e, "copy prims");
        const uint32_t r = m->roots[0];
        sc->roots[i] = (r & 0x80000000u) ? (0x80000000u | ((r & 0x7FFFFFFFu) + prim_off)) : r + pair_off;
        pair_off += m->num_pairs;
        prim_off += m->info.num_indices;
    }
    bytes = std::max<uint64_t>(pairs, 1) * 64 + prims * f4_per * 16;
    if (face_normals)
    {
        if ((e = hipMalloc(&sc->normals, size_t(num_normals) * 16)) != hipSuccess) return fail(e, "normals");
        if ((e = hipMemcpyAsync(sc->normals, face_normals, size_t(num_normals) * 16, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess)
            return fail(e, "upload normals");
        bytes += uint64_t(num_normals) * 16;
    }
    if ((e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return fail(e, "sync");
    sc->num_roots = count;
    sc->num_pairs = uint32_t(pairs);
    sc->finite_bounds = finite;
    scene_info(sc, count, uint32_t(nodes), uint32_t(prims), uint32_t(prims), kind, depth, max_pid, max_gid, bytes);
    *out = sc;
    return VRH_OK;
}

VRH_API int vrh_scene_build(vrh_ctx* ctx, const void* prims, uint32_t num_prims, uint32_t prim_kind,
                            const void* face_normals, const vrh_build_desc* desc, vrh_scene** out)
{
    VRH_CHECK(ctx && prims && out && num_prims >= 1, "vrh_scene_build: bad argument");
    if (prim_kind == VRH_PRIM_GENERIC80)
    {
        set_error("vrh_scene_build: the LBVH build takes triangles or spheres, not generic primitives (build with vrh_build_bvh and upload)");
        return VRH_ERR_UNSUPPORTED;
    }
    VRH_CHECK(prim_kind == VRH_PRIM_TRI64 || prim_kind == VRH_PRIM_SPHERE48, "vrh_scene_build: unknown prim_kind");
    VRH_CHECK(!desc || desc->method == VRH_BUILD_LBVH, "vrh_scene_build: unknown build method");
    *out = nullptr;
    if (face_normals)
    {
        // the kernels read face_normals[prim_id], and num_prims rows are copied: checked before anything is built
        const size_t stride = prim_kind == VRH_PRIM_TRI64 ? 64u : 48u;
        for (uint32_t i = 0; i < num_prims; ++i)
        {
            uint32_t pid;
            std::memcpy(&pid, static_cast<const char*>(prims) + i * stride + 4, 4);
            VRH_CHECK(pid < num_prims, "vrh_scene_build: face normals are indexed by prim_id, but prim_id " + std::to_string(pid)
                                           + " (primitive " + std::to_string(i) + ") is not below num_prims "
                                           + std::to_string(num_prims));
        }
    }
    int rc = select_device(ctx);
    if (rc) return rc;
    lbvh_out b;
    std::string err;
    rc = build_lbvh(prims, num_prims, prim_kind, desc && desc->max_leaf ? desc->max_leaf : 4u, ctx->stream, b, err);
    if (rc) { set_error(err); return rc; }
    vrh_scene* sc = new_scene(ctx);
    if (!sc)
    {
        for (void* p : { (void*)b.nodes, (void*)b.indices, (void*)b.pairs, (void*)b.prims }) (void)hipFree(p);
        return VRH_ERR_OOM;
    }
    sc->pairs = b.pairs; sc->prims = b.prims; sc->dnodes = b.nodes; sc->dindices = b.indices;
    sc->roots[0] = b.root;
    sc->num_pairs = b.num_pairs;
    sc->finite_bounds = b.finite;
    uint64_t bytes = uint64_t(std::max(b.num_pairs, 1u)) * 64 + uint64_t(num_prims) * leaf_record_bytes(prim_kind);
    if (face_normals
        && (rc = scene_block(sc, sc->normals, face_normals, size_t(num_prims) * sizeof(float4), bytes, "vrh_scene_build", "normals")))
        return rc;
    scene_info(sc, 1, b.num_nodes, num_prims, num_prims, prim_kind, b.max_depth, b.max_prim_id, b.max_geom_id, bytes);
    sc->info.gpu_built = 1;
    sc->info.build_ms = b.build_ms;
    *out = sc;
    return VRH_OK;
}

VRH_API int vrh_scene_download_bvh(vrh_ctx* ctx, const vrh_scene* sc, void* nodes_out, uint32_t* num_nodes,
                                   uint32_t* indices_out)
{
    VRH_CHECK(ctx && sc && num_nodes, "vrh_scene_download_bvh: null argument");
    if (!sc->dnodes) { set_error("vrh_scene_download_bvh: only GPU-built scenes keep their tree on the device"); return VRH_ERR_UNSUPPORTED; }
    if (!nodes_out) { *num_nodes = sc->info.num_nodes; return VRH_OK; }
    VRH_CHECK(*num_nodes >= sc->info.num_nodes, "vrh_scene_download_bvh: nodes_out too small");
    int rc = select_device(ctx);
    if (rc) return rc;
    if ((rc = ctx_drain(ctx))) return rc;
    VRH_HIP(hipMemcpy(nodes_out, sc->dnodes, size_t(sc->info.num_nodes) * sizeof(node32), hipMemcpyDeviceToHost));
    if (indices_out) VRH_HIP(hipMemcpy(indices_out, sc->dindices, size_t(sc->info.num_indices) * 4, hipMemcpyDeviceToHost));
    *num_nodes = sc->info.num_nodes;
    return VRH_OK;
}

VRH_API int vrh_bvh_sah_cost(const void* nodes_v, uint32_t num_nodes, float ci, float cl, float cp, float* cost)
{
    VRH_CHECK(nodes_v && num_nodes >= 1 && cost, "vrh_bvh_sah_cost: bad argument");
    auto nodes = static_cast<const node32*>(nodes_v);
    // aabb.inl:177-196 surface_area = 2 * (s.x * s.y + s.y * s.z + s.z * s.x), s = max - min
    auto area = [](const node32& n) {
        const float sx = n.bmax[0] - n.bmin[0], sy = n.bmax[1] - n.bmin[1], sz = n.bmax[2] - n.bmin[2];
        return 2.0f * (sx * sy + sy * sz + sz * sx);
    };
    const float A_r = area(nodes[0]);
    float A_l = 0.0f, A_i = 0.0f, A_l_x_N_n = 0.0f;
    for (uint32_t i = 0; i < num_nodes; ++i)
    {
        if (nodes[i].num_prims != 0)
        {
            A_l += area(nodes[i]);
            A_l_x_N_n += area(nodes[i]) * static_cast<float>(nodes[i].num_prims);
        }
        else
            A_i += area(nodes[i]);
    }
    *cost = ci * (A_i / A_r) + cl * (A_l / A_r) + cp * (A_l_x_N_n / A_r);
    return VRH_OK;
}

VRH_API int vrh_scene_set_vertex_normals(vrh_scene* sc, const void* normals, uint32_t num_normals)
{
    VRH_CHECK(sc && normals, "vrh_scene_set_vertex_normals: null argument");
    if (sc->info.prim_kind == VRH_PRIM_GENERIC80)
    {
        set_error("vrh_scene_set_vertex_normals: generic-primitive scenes take per-face normals only");
        return VRH_ERR_UNSUPPORTED;
    }
    VRH_CHECK(sc->info.prim_kind == VRH_PRIM_TRI64, "vrh_scene_set_vertex_normals: triangles only");
    VRH_CHECK(uint64_t(num_normals) >= 3ull * (uint64_t(sc->info.max_prim_id) + 1ull),
              "vrh_scene_set_vertex_normals: need 3 normals per prim_id (3 * (max prim_id + 1))");
    int rc = select_device(sc->ctx);
    if (rc) return rc;
    if (sc->vnormals) { (void)hipFree(sc->vnormals); sc->vnormals = nullptr; sc->info.vertex_normals = 0; }
    const size_t bytes = size_t(num_normals) * sizeof(float4);
    VRH_HIP(hipMalloc(&sc->vnormals, bytes));
    VRH_HIP(hipMemcpy(sc->vnormals, normals, bytes, hipMemcpyHostToDevice));
    sc->info.vertex_normals = 1;
    sc->info.device_bytes += bytes;
    return VRH_OK;
}

// the device block of a shading's material records: dev::TEX_BLOCK_BYTES of zeros (no textures), then
// `bytes` for the records
static hipError_t alloc_material_block(vrh_shading* sh, size_t bytes)
{
    static_assert(sizeof(dev::tex_block) <= dev::TEX_BLOCK_BYTES && dev::TEX_BLOCK_BYTES % 16 == 0, "texture block");
    hipError_t e = hipMalloc(&sh->block, dev::TEX_BLOCK_BYTES + bytes);
    if (e == hipSuccess) e = hipMemset(sh->block, 0, dev::TEX_BLOCK_BYTES);
    return e;
}

static void free_textures(vrh_shading* sh)
{
    if (sh->tex_coords) (void)hipFree(sh->tex_coords);
    if (sh->tex_views) (void)hipFree(sh->tex_views);
    for (void* p : sh->tex_pixels) (void)hipFree(p);
    sh->tex_coords = nullptr; sh->tex_views = nullptr; sh->tex_pixels.clear();
    sh->num_tex_coords = 0; sh->num_textures = 0;
}

VRH_API int vrh_shading_set_textures(vrh_ctx* ctx, vrh_shading* sh, const float* tex_coords, uint32_t num_tex_coords,
                                     const vrh_texture_desc* textures, uint32_t num_textures)
{
    VRH_CHECK(ctx && sh, "vrh_shading_set_textures: null argument");
    VRH_CHECK(sh->ctx == ctx, "vrh_shading_set_textures: shading of another context");
    if (num_textures)
    {
        VRH_CHECK(textures && tex_coords, "vrh_shading_set_textures: null argument");
        VRH_CHECK(num_textures == sh->num_materials,
                  "vrh_shading_set_textures: " + std::to_string(num_textures) + " textures for " + std::to_string(sh->num_materials)
                      + " materials (textures are indexed by geom_id)");
        VRH_CHECK(num_tex_coords >= 3 && num_tex_coords % 3 == 0, "vrh_shading_set_textures: 3 tex coords per triangle");
        for (uint32_t i = 0; i < num_textures; ++i)
        {
            const std::string bad = check_texture_desc(textures[i]);
            VRH_CHECK(bad.empty(), "vrh_shading_set_textures: texture " + std::to_string(i) + ": " + bad);
        }
        const size_t bc = first_bad_coord(tex_coords, size_t(num_tex_coords) * 2);
        VRH_CHECK(bc == size_t(num_tex_coords) * 2, "vrh_shading_set_textures: texture coordinate " + std::to_string(bc / 2)
                                                         + " is not finite or exceeds 2^20 in magnitude");
    }
    int rc = select_device(ctx);
    if (rc) return rc;
    // no frame still reads the old table
    VRH_HIP(ctx_join(ctx));
    VRH_HIP(hipStreamSynchronize(ctx->stream));
    dev::tex_block tb{ nullptr, nullptr };
    VRH_HIP(hipMemcpy(sh->block, &tb, sizeof(tb), hipMemcpyHostToDevice));
    free_textures(sh);
    if (!num_textures) return VRH_OK;
    std::vector<dev::tex_view> views(num_textures);
    std::vector<uint32_t> expanded;
    hipError_t e = hipMalloc(&sh->tex_coords, sizeof(float2) * num_tex_coords);
    if (e == hipSuccess) e = hipMemcpy(sh->tex_coords, tex_coords, sizeof(float2) * num_tex_coords, hipMemcpyHostToDevice);
    for (uint32_t i = 0; i < num_textures && e == hipSuccess; ++i)
    {
        const vrh_texture_desc& d = textures[i];
        const uint32_t* dpix = nullptr;
        if (!tex_is_dummy(d))
        {
            // descriptors that share a pixel pointer, size and format share one upload
            for (uint32_t j = 0; j < i && !dpix; ++j)
                if (!tex_is_dummy(textures[j]) && textures[j].pixels == d.pixels && textures[j].width == d.width
                    && textures[j].height == d.height && textures[j].format == d.format)
                    dpix = views[j].pixels;
            if (!dpix)
            {
                expand_rgba8(d, expanded);
                void* p = nullptr;
                e = hipMalloc(&p, expanded.size() * 4);
                if (e != hipSuccess) break;
                sh->tex_pixels.push_back(p);
                e = hipMemcpy(p, expanded.data(), expanded.size() * 4, hipMemcpyHostToDevice);
                dpix = static_cast<const uint32_t*>(p);
            }
        }
        views[i] = dev::make_tex_view(dpix, d.width, d.height, d.filter, d.address[0], d.address[1]);
    }
    if (e == hipSuccess) e = hipMalloc(&sh->tex_views, sizeof(dev::tex_view) * num_textures);
    if (e == hipSuccess) e = hipMemcpy(sh->tex_views, views.data(), sizeof(dev::tex_view) * num_textures, hipMemcpyHostToDevice);
    tb.tc = sh->tex_coords; tb.tex = sh->tex_views;
    if (e == hipSuccess) e = hipMemcpy(sh->block, &tb, sizeof(tb), hipMemcpyHostToDevice);
    if (e != hipSuccess)
    {
        set_error(std::string("vrh_shading_set_textures: ") + hipGetErrorString(e));
        free_textures(sh);
        return e == hipErrorOutOfMemory ? VRH_ERR_OOM : VRH_ERR_HIP;
    }
    sh->num_tex_coords = num_tex_coords;
    sh->num_textures = num_textures;
    return VRH_OK;
}

VRH_API int vrh_shading_create(vrh_ctx* ctx, const vrh_plastic* materials, uint32_t num_materials,
                               const vrh_point_light* lights, uint32_t num_lights, vrh_shading** out)
{
    static_assert(sizeof(vrh_plastic) == sizeof(dev::plastic_t), "plastic layout");
    static_assert(sizeof(vrh_point_light) == sizeof(dev::point_light_t), "light layout");
    VRH_CHECK(ctx && out && materials && num_materials > 0, "vrh_shading_create: need at least one material");
    VRH_CHECK(num_lights == 0 || lights, "vrh_shading_create: null lights");
    *out = nullptr;
    int rc = select_device(ctx);
    if (rc) return rc;
    auto* sh = new (std::nothrow) vrh_shading;
    if (!sh) { set_error("host allocation failed"); return VRH_ERR_OOM; }
    sh->ctx = ctx;
    sh->num_materials = num_materials;
    sh->num_lights = num_lights;
    hipError_t e = alloc_material_block(sh, sizeof(vrh_plastic) * num_materials);
    if (e == hipSuccess) sh->materials = reinterpret_cast<dev::plastic_t*>(static_cast<char*>(sh->block) + dev::TEX_BLOCK_BYTES);
    if (e == hipSuccess) e = hipMemcpy(sh->materials, materials, sizeof(vrh_plastic) * num_materials, hipMemcpyHostToDevice);
    if (e == hipSuccess && num_lights)
    {
        e = hipMalloc(&sh->lights, sizeof(vrh_point_light) * num_lights);
        if (e == hipSuccess) e = hipMemcpy(sh->lights, lights, sizeof(vrh_point_light) * num_lights, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess)
    {
        set_error(std::string("vrh_shading_create: ") + hipGetErrorString(e));
        vrh_shading_free(sh);
        return e == hipErrorOutOfMemory ? VRH_ERR_OOM : VRH_ERR_HIP;
    }
    *out = sh;
    return VRH_OK;
}

VRH_API int vrh_shading_create_generic(vrh_ctx* ctx, const vrh_material* materials, uint32_t num_materials,
                                       const vrh_point_light* lights, uint32_t num_lights, vrh_shading** out)
{
    static_assert(sizeof(vrh_material) == 64 && sizeof(vrh_material) == sizeof(dev::material_t), "material layout");
    static_assert(offsetof(vrh_material, u) == 4 && offsetof(dev::material_t, p) == 4, "material layout");
    static_assert(int(VRH_MATERIAL_PLASTIC) == int(dev::MAT_PLASTIC) && int(VRH_MATERIAL_MATTE) == int(dev::MAT_MATTE)
                  && int(VRH_MATERIAL_MIRROR) == int(dev::MAT_MIRROR) && int(VRH_MATERIAL_EMISSIVE) == int(dev::MAT_EMISSIVE),
                  "material kinds");
    VRH_CHECK(ctx && out && materials && num_materials > 0, "vrh_shading_create_generic: need at least one material");
    VRH_CHECK(num_lights == 0 || lights, "vrh_shading_create_generic: null lights");
    *out = nullptr;
    for (uint32_t i = 0; i < num_materials; ++i)
        VRH_CHECK(materials[i].kind <= VRH_MATERIAL_EMISSIVE,
                  "vrh_shading_create_generic: material " + std::to_string(i) + " has unknown kind " + std::to_string(materials[i].kind));
    int rc = select_device(ctx);
    if (rc) return rc;
    auto* sh = new (std::nothrow) vrh_shading;
    if (!sh) { set_error("host allocation failed"); return VRH_ERR_OOM; }
    sh->ctx = ctx;
    sh->num_materials = num_materials;
    sh->num_lights = num_lights;
    hipError_t e = alloc_material_block(sh, sizeof(vrh_material) * num_materials);
    if (e == hipSuccess) sh->gmaterials = reinterpret_cast<dev::material_t*>(static_cast<char*>(sh->block) + dev::TEX_BLOCK_BYTES);
    if (e == hipSuccess) e = hipMemcpy(sh->gmaterials, materials, sizeof(vrh_material) * num_materials, hipMemcpyHostToDevice);
    if (e == hipSuccess && num_lights)
    {
        e = hipMalloc(&sh->lights, sizeof(vrh_point_light) * num_lights);
        if (e == hipSuccess) e = hipMemcpy(sh->lights, lights, sizeof(vrh_point_light) * num_lights, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess)
    {
        set_error(std::string("vrh_shading_create_generic: ") + hipGetErrorString(e));
        vrh_shading_free(sh);
        return e == hipErrorOutOfMemory ? VRH_ERR_OOM : VRH_ERR_HIP;
    }
    *out = sh;
    return VRH_OK;
}

VRH_API int vrh_hit_mask_create(vrh_ctx* ctx, const float* tex_coords, uint32_t num_tex_coords,
                                const uint8_t* mask, uint32_t mask_width, uint32_t mask_height, vrh_hit_mask** out)
{
    VRH_CHECK(ctx && out && tex_coords && mask, "vrh_hit_mask_create: null argument");
    VRH_CHECK(num_tex_coords >= 3 && num_tex_coords % 3 == 0, "vrh_hit_mask_create: 3 tex coords per triangle");
    VRH_CHECK(mask_width > 0 && mask_height > 0 && uint64_t(mask_width) * mask_height < (1ull << 32),
              "vrh_hit_mask_create: bad mask size");
    *out = nullptr;
    int rc = select_device(ctx);
    if (rc) return rc;
    auto* m = new (std::nothrow) vrh_hit_mask;
    if (!m) { set_error("host allocation failed"); return VRH_ERR_OOM; }
    m->ctx = ctx;
    m->num_tc = num_tex_coords;
    m->w = mask_width;
    m->h = mask_height;
    const size_t mb = size_t(mask_width) * mask_height;
    hipError_t e = hipMalloc(&m->tc, sizeof(float2) * num_tex_coords);
    if (e == hipSuccess) e = hipMemcpy(m->tc, tex_coords, sizeof(float2) * num_tex_coords, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc(&m->mask, mb);
    if (e == hipSuccess) e = hipMemcpy(m->mask, mask, mb, hipMemcpyHostToDevice);
    if (e != hipSuccess)
    {
        set_error(std::string("vrh_hit_mask_create: ") + hipGetErrorString(e));
        vrh_hit_mask_free(m);
        return e == hipErrorOutOfMemory ? VRH_ERR_OOM : VRH_ERR_HIP;
    }
    *out = m;
    return VRH_OK;
}

VRH_API int vrh_hit_mask_free(vrh_hit_mask* m)
{
    if (!m) return VRH_OK;
    if (m->ctx) (void)hipSetDevice(m->ctx->device);
    if (m->tc) (void)hipFree(m->tc);
    if (m->mask) (void)hipFree(m->mask);
    delete m;
    return VRH_OK;
}

VRH_API int vrh_shading_free(vrh_shading* sh)
{
    if (!sh) return VRH_OK;
    if (sh->ctx) (void)hipSetDevice(sh->ctx->device);
    free_textures(sh);
    if (sh->block) (void)hipFree(sh->block);        // the material records live in it
    if (sh->lights) (void)hipFree(sh->lights);
    delete sh;
    return VRH_OK;
}

// ---- render targets ------------------------------------------------------------------------------

VRH_API int vrh_rt_alloc(vrh_ctx* ctx, uint32_t w, uint32_t h, uint32_t flags, vrh_rt** out)
{
    VRH_CHECK(ctx && out && w > 0 && h > 0, "vrh_rt_alloc: bad argument");
    *out = nullptr;
    int rc = select_device(ctx);
    if (rc) return rc;
    auto* rt = new (std::nothrow) vrh_rt;
    if (!rt) { set_error("host allocation failed"); return VRH_ERR_OOM; }
    rt->ctx = ctx; rt->width = w; rt->height = h; rt->owned = true;
    size_t n = size_t(w) * h;
    hipError_t e = hipSuccess;
    if ((flags & VRH_RT_COLOR) && e == hipSuccess) e = hipMalloc(&rt->color, n * sizeof(float4));
    if ((flags & VRH_RT_PRIM_ID) && e == hipSuccess) e = hipMalloc(&rt->prim_id, n * sizeof(uint32_t));
    if ((flags & VRH_RT_T) && e == hipSuccess) e = hipMalloc(&rt->t, n * sizeof(float));
    if ((flags & VRH_RT_OCC) && e == hipSuccess) e = hipMalloc(&rt->occ, n);
    if (e != hipSuccess)
    {
        set_error(std::string("vrh_rt_alloc: ") + hipGetErrorString(e));
        vrh_rt_free(rt);
        return VRH_ERR_OOM;
    }
    *out = rt;
    return VRH_OK;
}

VRH_API int vrh_rt_wrap(vrh_ctx* ctx, uint32_t w, uint32_t h, void* color, uint32_t* prim_id, float* t, uint8_t* occ,
                        vrh_rt** out)
{
    VRH_CHECK(ctx && out && w > 0 && h > 0, "vrh_rt_wrap: bad argument");
    auto* rt = new (std::nothrow) vrh_rt;
    if (!rt) { set_error("host allocation failed"); return VRH_ERR_OOM; }
    rt->ctx = ctx; rt->width = w; rt->height = h; rt->owned = false;
    rt->color = static_cast<float4*>(color); rt->prim_id = prim_id; rt->t = t; rt->occ = occ;
    *out = rt;
    return VRH_OK;
}

VRH_API int vrh_rt_get_buffers(const vrh_rt* rt, void** color, uint32_t** prim_id, float** t, uint8_t** occ)
{
    VRH_CHECK(rt, "vrh_rt_get_buffers: null");
    if (color) *color = rt->color;
    if (prim_id) *prim_id = rt->prim_id;
    if (t) *t = rt->t;
    if (occ) *occ = rt->occ;
    return VRH_OK;
}

VRH_API int vrh_rt_free(vrh_rt* rt)
{
    if (!rt) return VRH_OK;
    if (rt->owned)
    {
        if (rt->ctx) (void)hipSetDevice(rt->ctx->device);
        if (rt->color) (void)hipFree(rt->color);
        if (rt->prim_id) (void)hipFree(rt->prim_id);
        if (rt->t) (void)hipFree(rt->t);
        if (rt->occ) (void)hipFree(rt->occ);
    }
    if (rt->fcolor || rt->fdepth)
    {
        if (rt->ctx) (void)hipSetDevice(rt->ctx->device);
        if (rt->fcolor) (void)hipFree(rt->fcolor);
        if (rt->fdepth) (void)hipFree(rt->fdepth);
    }
    if (rt->mh_prim_id || rt->mh_t)
    {
        if (rt->ctx) (void)hipSetDevice(rt->ctx->device);
        if (rt->mh_prim_id) (void)hipFree(rt->mh_prim_id);
        if (rt->mh_t) (void)hipFree(rt->mh_t);
    }
    if (rt->ctx)
        for (auto& l : rt->ctx->lane)
            if (l.pending_rt == rt) l.pending_rt = nullptr;     // a frame nobody can read any more
    if (rt->lane_written)
    {
        if (rt->ctx) (void)hipSetDevice(rt->ctx->device);
        (void)hipEventSynchronize(rt->lane_written);
        (void)hipEventDestroy(rt->lane_written);
    }
    if (rt->written)
    {
        if (rt->ctx) (void)hipSetDevice(rt->ctx->device);
        (void)hipEventSynchronize(rt->written);
        if (rt->ctx)
        {
            auto& gw = rt->ctx->group_written;
            for (size_t i = 0; i < gw.size(); ++i)
                if (gw[i] == rt->written) { gw.erase(gw.begin() + long(i)); break; }
        }
        (void)hipEventDestroy(rt->written);
    }
    delete rt;
    return VRH_OK;
}

namespace {
__global__ void fill_rt_kernel(float4* color, uint32_t* pid, float* t, uint8_t* occ, size_t n, float4 c)
{
    size_t i = size_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (color) color[i] = c;
    if (pid) pid[i] = 0xFFFFFFFFu;
    if (t) t[i] = -1.0f;
    if (occ) occ[i] = 0;
}

// asynchronous frames: a frame rendered into a lane's scratch target lands in its target, scissor box
// only (the pixels a frame writes), once the target's previous writer is done
__global__ void copy_clip_kernel(float4* color, uint32_t* pid, float* t, uint8_t* occ, const float4* s_color,
                                 const uint32_t* s_pid, const float* s_t, const uint8_t* s_occ, uint32_t width,
                                 uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1)
{
    const uint32_t x = x0 + blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t y = y0 + blockIdx.y * blockDim.y + threadIdx.y;
    if (x >= x1 || y >= y1) return;
    const size_t i = size_t(y) * width + x;
    if (color) color[i] = s_color[i];
    if (pid) pid[i] = s_pid[i];
    if (t) t[i] = s_t[i];
    if (occ) occ[i] = s_occ[i];
}
} // namespace

} // extern "C"

// Asynchronous frames into a shared target: the scratch copy of lane l's pending frame, issued on that
// lane after the target's last writer (the other lane, unless joined since); the target's last writer
// is then this lane.  Called before anything else may read or write the target (ctx_join: every entry
// point that works on the context stream; vrh_render_batch for other frames) and before the lane's
// scratch target is reused.
hipError_t ctx_flush_pending(const vrh_ctx* cctx, int only)
{
    vrh_ctx* ctx = const_cast<vrh_ctx*>(cctx);
    for (int l = 0; l < VRH_MAX_FRAME_LANES; ++l)
    {
        if (only >= 0 && l != only) continue;
        vrh_ctx::lane_t& L = ctx->lane[l];
        vrh_rt* rt = L.pending_rt;
        if (!rt) continue;
        L.pending_rt = nullptr;
        hipError_t e;
        if (rt->lane >= 0 && rt->lane != l && rt->lane_epoch == ctx->join_epoch)
            if ((e = hipStreamWaitEvent(L.stream, rt->lane_written, 0)) != hipSuccess) return e;
        const uint32_t* cl = L.pending_clip;
        const dim3 blk(64, 4), grd((cl[2] - cl[0] + 63) / 64, (cl[3] - cl[1] + 3) / 4);
        const bool* fl = L.pending_fields;
        hipLaunchKernelGGL(copy_clip_kernel, grd, blk, 0, L.stream, fl[0] ? rt->color : nullptr, fl[1] ? rt->prim_id : nullptr,
                           fl[2] ? rt->t : nullptr, fl[3] ? rt->occ : nullptr, (const float4*)L.color,
                           (const uint32_t*)L.prim_id, (const float*)L.t, (const uint8_t*)L.occ, rt->width,
                           cl[0], cl[1], cl[2], cl[3]);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = hipEventRecord(rt->lane_written, L.stream)) != hipSuccess) return e;
        rt->lane = l;
        rt->lane_epoch = ctx->join_epoch;
        if ((e = hipEventRecord(L.done, L.stream)) != hipSuccess) return e;
    }
    return hipSuccess;
}

extern "C" {

// gpu_buffer_rt::clear_color_buffer (thrust::fill, gpu_buffer_rt.inl:49-76); side buffers reset to "miss"
VRH_API int vrh_rt_clear(vrh_ctx* ctx, vrh_rt* rt, const float color[4])
{
    VRH_CHECK(ctx && rt, "vrh_rt_clear: null");
    int rc = select_device(ctx);
    if (rc) return rc;
    size_t n = size_t(rt->width) * rt->height;
    float4 c = color ? make_float4(color[0], color[1], color[2], color[3]) : make_float4(0, 0, 0, 0);
    rc = rt_wait(ctx, rt);
    if (rc) return rc;
    hipLaunchKernelGGL(fill_rt_kernel, dim3(unsigned((n + 255) / 256)), dim3(256), 0, ctx->stream,
                       rt->color, rt->prim_id, rt->t, rt->occ, n, c);
    VRH_HIP(hipGetLastError());
    // a formatted target: clear_color_buffer stores the converted colour (simple_buffer_rt.inl:54-66)
    if (rt->formatted) return resolve_clear_color(rt, color, ctx->stream);
    return VRH_OK;
}

// ---- frame ----------------------------------------------------------------------------------------

VRH_API uint32_t vrh_shard_bands(uint32_t height, uint32_t index, uint32_t count)
{
    return plan::shard_bands(height, index, count);
}

VRH_API int vrh_render(vrh_ctx* ctx, const vrh_scene* sc, vrh_rt* rt, const vrh_camera* cam,
                       const vrh_kernel_desc* k, const vrh_shard* shard, uint32_t frame_num)
{
    return vrh_render_batch(ctx, sc, rt, cam, 1, k, shard, frame_num);
}

namespace {
// one pass of a pixel sampler (vrh_render_sampled); null = the uniform sampler, colour stored
struct sampler_pass
{
    float off[2];
    uint32_t jitter, blend;
    float s, d;
    const float* inv_mats;    // vrh_render_view: inverse view, inverse projection (32 floats), else null
    const float* mats;        // vrh_render_view: view, projection (a formatted target's depth), else null
};
int render_batch_impl(vrh_ctx* ctx, const vrh_scene* sc, vrh_rt* rt, const vrh_camera* cams, uint32_t num_frames,
                      const vrh_kernel_desc* k, const vrh_shard* shard, uint32_t frame_num, const sampler_pass* sp);
} // namespace

VRH_API int vrh_render_batch(vrh_ctx* ctx, const vrh_scene* sc, vrh_rt* rt, const vrh_camera* cams,
                             uint32_t num_frames, const vrh_kernel_desc* k, const vrh_shard* shard,
                             uint32_t frame_num)
{
    return render_batch_impl(ctx, sc, rt, cams, num_frames, k, shard, frame_num, nullptr);
}

namespace {
// the passes of a pixel sampler (vrh_render_sampled / vrh_render_view); inv_mats: camera matrices
int render_sampled_impl(vrh_ctx* ctx, const vrh_scene* sc, vrh_rt* rt, const vrh_camera* cam,
                        const vrh_kernel_desc* k, const vrh_pixel_sampler* ps, uint32_t frame_num, const float* inv_mats,
                        const float* mats)
{
    VRH_CHECK(ctx && sc && rt && cam && k && ps, "vrh_render_sampled: null argument");
    VRH_CHECK(ps->kind <= VRH_SAMPLER_SSAA, "vrh_render_sampled: unknown pixel sampler");
    if (rt->formatted && ps->kind == VRH_SAMPLER_SSAA)
    {
        // the reference begins ssaa by storing a default-constructed result_record, whose depth it never defines
        set_error(std::string(inv_mats ? "vrh_render_view" : "vrh_render_sampled") + ": the ssaa sampler does not render into a formatted render target");
        return VRH_ERR_UNSUPPORTED;
    }
    if (ps->kind == VRH_SAMPLER_UNIFORM && !inv_mats) return render_batch_impl(ctx, sc, rt, cam, 1, k, nullptr, frame_num, nullptr);
    if (k->kind == VRH_KERNEL_PATHTRACING && (inv_mats || ps->kind == VRH_SAMPLER_SSAA))
    {
        set_error(inv_mats ? "vrh_render_view: camera matrices run the primary and AO kernels, not the path tracer"
                           : "vrh_render_sampled: the path-tracing kernel takes the uniform, jittered and jittered_blend samplers, not ssaa");
        return VRH_ERR_UNSUPPORTED;
    }
    // the path tracer accumulates through the jittered samplers (the viewer's progressive mode)
    if (k->kind != VRH_KERNEL_PRIMARY && k->kind != VRH_KERNEL_AO && k->kind != VRH_KERNEL_PATHTRACING)
    {
        set_error(inv_mats ? "vrh_render_view: camera matrices run the primary and AO kernels"
                           : "vrh_render_sampled: jittered / ssaa samplers run the primary and AO kernels (jittered: the path tracer too)");
        return VRH_ERR_UNSUPPORTED;
    }
    if (ps->kind != VRH_SAMPLER_SSAA)
    {
        // uniform (camera matrices): the pixel's ray, colour stored; jittered: the pixel's jittered
        // ray, colour stored; jittered_blend: blended with a = 1 / frame_num, 1 - a (sched_common.h:480-540)
        sampler_pass p{ { 0.0f, 0.0f }, ps->kind == VRH_SAMPLER_UNIFORM ? 0u : 1u, 0u, 1.0f, 0.0f, inv_mats, mats };
        if (ps->kind == VRH_SAMPLER_JITTERED_BLEND)
        {
            p.blend = 1u;
            p.s = 1.0f / float(frame_num);
            p.d = 1.0f - p.s;
        }
        return render_batch_impl(ctx, sc, rt, cam, 1, k, nullptr, frame_num, &p);
    }
    // ssaa<N> (sched_common.h:219-300, 640-720): colour 0, then every sample blended with 1 / N, 1
    // in order -- one pass per sample on the context's stream
    static const float off2[2][2] = { { -0.25f, -0.25f }, { 0.25f, 0.25f } };
    static const float off4[4][2] = { { -0.125f, -0.375f }, { 0.375f, -0.125f }, { 0.125f, 0.375f }, { -0.375f, 0.125f } };
    static const float off8[8][2] = { { -0.125f, -0.4375f }, { 0.375f, -0.3125f }, { -0.375f, -0.1875f }, { 0.125f, -0.0625f },
                                      { -0.125f, 0.0625f }, { 0.375f, 0.1825f }, { -0.375f, 0.3125f }, { 0.125f, 0.4375f } };
    VRH_CHECK(ps->count == 2 || ps->count == 4 || ps->count == 8, "vrh_render_sampled: ssaa takes 2, 4 or 8 samples");
    const float (*tab)[2] = ps->count == 2 ? off2 : ps->count == 4 ? off4 : off8;
    for (uint32_t i = 0; i < ps->count; ++i)
    {
        sampler_pass p{ { tab[i][0], tab[i][1] }, 0u, i == 0 ? 2u : 1u, 1.0f / float(ps->count), 1.0f, inv_mats, mats };
        const int rc = render_batch_impl(ctx, sc, rt, cam, 1, k, nullptr, frame_num, &p);
        if (rc) return rc;
    }
    return VRH_OK;
}
} // namespace

VRH_API int vrh_render_sampled(vrh_ctx* ctx, const vrh_scene* sc, vrh_rt* rt, const vrh_camera* cam,
                               const vrh_kernel_desc* k, const vrh_pixel_sampler* ps, uint32_t frame_num)
{
    return render_sampled_impl(ctx, sc, rt, cam, k, ps, frame_num, nullptr, nullptr);
}

// matrix4.inl:209-244 inverse(): the 2x2 sub-determinants of rows 0-1 and 2-3
// (det2(a, b, c, d) = a * d - c * b, math.h:493-496), the cofactor expansion, every entry / det
VRH_API void vrh_matrix_inverse(const float m[16], float out[16])
{
    auto det2 = [](float a, float b, float c, float d) { return a * d - c * b; };
    auto M = [m](int r, int c) { return m[c * 4 + r]; };
    const float s0 = det2(M(0, 0), M(0, 1), M(1, 0), M(1, 1)), s1 = det2(M(0, 0), M(0, 2), M(1, 0), M(1, 2));
    const float s2 = det2(M(0, 0), M(0, 3), M(1, 0), M(1, 3)), s3 = det2(M(0, 1), M(0, 2), M(1, 1), M(1, 2));
    const float s4 = det2(M(0, 1), M(0, 3), M(1, 1), M(1, 3)), s5 = det2(M(0, 2), M(0, 3), M(1, 2), M(1, 3));
    const float c5 = det2(M(2, 2), M(2, 3), M(3, 2), M(3, 3)), c4 = det2(M(2, 1), M(2, 3), M(3, 1), M(3, 3));
    const float c3 = det2(M(2, 1), M(2, 2), M(3, 1), M(3, 2)), c2 = det2(M(2, 0), M(2, 3), M(3, 0), M(3, 3));
    const float c1 = det2(M(2, 0), M(2, 2), M(3, 0), M(3, 2)), c0 = det2(M(2, 0), M(2, 1), M(3, 0), M(3, 1));
    const float det = s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0;
    const float r[16] = {
        (M(1, 1) * c5 - M(1, 2) * c4 + M(1, 3) * c3) / det, (-M(1, 0) * c5 + M(1, 2) * c2 + M(1, 3) * c1) / det,
        (M(1, 0) * c4 - M(1, 1) * c2 + M(1, 3) * c0) / det, (-M(1, 0) * c3 + M(1, 1) * c1 + M(1, 2) * c0) / det,
        (-M(0, 1) * c5 + M(0, 2) * c4 - M(0, 3) * c3) / det, (M(0, 0) * c5 - M(0, 2) * c2 + M(0, 3) * c1) / det,
        (-M(0, 0) * c4 + M(0, 1) * c2 - M(0, 3) * c0) / det, (M(0, 0) * c3 - M(0, 1) * c1 + M(0, 2) * c0) / det,
        (M(3, 1) * s5 - M(3, 2) * s4 + M(3, 3) * s3) / det, (-M(3, 0) * s5 + M(3, 2) * s2 - M(3, 3) * s1) / det,
        (M(3, 0) * s4 - M(3, 1) * s2 + M(3, 3) * s0) / det, (-M(3, 0) * s3 + M(3, 1) * s1 - M(3, 2) * s0) / det,
        (-M(2, 1) * s5 + M(2, 2) * s4 - M(2, 3) * s3) / det, (M(2, 0) * s5 - M(2, 2) * s2 + M(2, 3) * s1) / det,
        (-M(2, 0) * s4 + M(2, 1) * s2 - M(2, 3) * s0) / det, (M(2, 0) * s3 - M(2, 1) * s1 + M(2, 2) * s0) / det };
    std::memcpy(out, r, sizeof(r));
}

VRH_API int vrh_render_view(vrh_ctx* ctx, const vrh_scene* sc, vrh_rt* rt, const vrh_view_camera* vc,
                            const vrh_kernel_desc* k, const vrh_pixel_sampler* ps, uint32_t frame_num)
{
    VRH_CHECK(ctx && vc, "vrh_render_view: null argument");
    vrh_camera cam{};
    cam.width = vc->width; cam.height = vc->height;
    std::memcpy(cam.scissor, vc->scissor, sizeof(cam.scissor));
    float inv[32];
    vrh_matrix_inverse(vc->view, inv);
    vrh_matrix_inverse(vc->proj, inv + 16);
    float mats[32];
    std::memcpy(mats, vc->view, sizeof(vc->view));
    std::memcpy(mats + 16, vc->proj, sizeof(vc->proj));
    return render_sampled_impl(ctx, sc, rt, &cam, k, ps, frame_num, inv, mats);
}

// ---- vrh_render: validate, plan (vrh_launch.h), fill render_params, choose where the launch runs,
// diagnostics buffers, launch.  Every step takes what it reads as arguments.
namespace {

// which rows of the target the launch writes
struct frame_rows_t
{
    vrh_shard sh;
    uint32_t local_bands;     // 8-row bands of one frame this shard renders
    uint32_t frame_rows;      // frame f of the batch owns rows [f * frame_rows, (f + 1) * frame_rows) of the target
};

int validate_render(vrh_ctx* ctx, const vrh_scene* sc, vrh_rt* rt, const vrh_camera* cams, uint32_t num_frames,
                    const vrh_kernel_desc* k, const vrh_shard* shard, frame_rows_t& rows)
{
    VRH_CHECK(ctx && sc && rt && cams && k, "vrh_render: null argument");
    VRH_CHECK(rt->ctx == ctx && sc->ctx == ctx, "vrh_render: scene / render target of another context");
    VRH_CHECK(num_frames >= 1 && num_frames <= VRH_MAX_BATCH, "vrh_render_batch: 1..VRH_MAX_BATCH frames");
    const vrh_camera* cam = cams;
    for (uint32_t f = 1; f < num_frames; ++f)
        VRH_CHECK(cams[f].width == cam->width && cams[f].height == cam->height, "vrh_render_batch: frames differ in size");
    VRH_CHECK(cam->width > 0 && cam->height > 0, "vrh_render: empty image");
    VRH_CHECK(k->kind <= VRH_KERNEL_PATHTRACING, "vrh_render: unknown kernel kind");
    const bool ao = k->kind == VRH_KERNEL_AO;
    const bool multi = k->kind == VRH_KERNEL_MULTI_HIT;
    const bool whitted = k->kind == VRH_KERNEL_WHITTED;
    const bool path = k->kind == VRH_KERNEL_PATHTRACING;
    const bool shade = k->kind == VRH_KERNEL_SIMPLE || multi || whitted || path;
    const bool list = sc->num_roots > 1;
    if (multi)
    {
        VRH_CHECK(k->max_hits >= 1 && k->max_hits <= VRH_MAX_HITS, "vrh_render: max_hits must be in [1, 16]");
        VRH_CHECK(rt->mh_n == k->max_hits, "vrh_render: render target needs vrh_rt_alloc_multi_hit(max_hits)");
    }
    if (shade)
    {
        VRH_CHECK(k->shading, "vrh_render: the shading kernels need a vrh_shading (materials, lights)");
        if (k->shading->gmaterials && !path)
        {
            set_error("vrh_render: a generic shading (vrh_shading_create_generic) is taken by VRH_KERNEL_PATHTRACING only");
            return VRH_ERR_UNSUPPORTED;
        }
        if (sc->info.prim_kind == VRH_PRIM_GENERIC80)
        {
            // generic primitives: simple and whitted with per-face normals (the plan names what else is asked for)
            if (k->normal_binding == VRH_NORMALS_PER_VERTEX)
            {
                set_error("vrh_render: generic-primitive scenes do not support per-vertex normals");
                return VRH_ERR_UNSUPPORTED;
            }
        }
        else
        if (sc->info.prim_kind != VRH_PRIM_TRI64) { set_error("vrh_render: the shading kernels support triangles"); return VRH_ERR_UNSUPPORTED; }
        if (list) { set_error("vrh_render: the shading kernels take a single BVH (scene lists: primary and AO kernels)"); return VRH_ERR_UNSUPPORTED; }
        VRH_CHECK(k->shading->num_materials > sc->info.max_geom_id, "vrh_render: a geom_id has no material");
        VRH_CHECK(k->normal_binding <= VRH_NORMALS_PER_VERTEX, "vrh_render: unknown normal binding");
        if (k->normal_binding == VRH_NORMALS_PER_FACE) VRH_CHECK(sc->normals, "vrh_render: per-face shading needs face normals");
        else VRH_CHECK(sc->vnormals, "vrh_render: per-vertex shading needs vrh_scene_set_vertex_normals");
        if (k->shading->num_textures)
        {
            if (multi) { set_error("vrh_render: multi_hit takes no textured shading"); return VRH_ERR_UNSUPPORTED; }
            if (k->hit_mask) { set_error("vrh_render: a textured shading together with a hit mask is not supported"); return VRH_ERR_UNSUPPORTED; }
            VRH_CHECK(uint64_t(k->shading->num_tex_coords) >= 3ull * (uint64_t(sc->info.max_prim_id) + 1),
                      "vrh_render: the shading has fewer than 3 tex coords per prim_id of the scene");
            VRH_CHECK(uint64_t(k->shading->num_tex_coords) / 3 >= sc->info.num_prims,
                      "vrh_render: the scene has more primitives than the shading has tex coord triples");
        }
    }
    if (ao)
    {
        VRH_CHECK(k->samples >= 1 && k->samples <= 32, "vrh_render: AO samples must be in [1, 32]");
        // the occlusion target holds one bit per sample in a byte
        VRH_CHECK(!rt->occ || k->samples <= 8 || (k->flags & VRH_KERNEL_NO_OCC),
                  "vrh_render: a VRH_RT_OCC target records at most 8 AO samples (VRH_KERNEL_NO_OCC leaves it out)");
        VRH_CHECK(sc->normals, "vrh_render: AO needs normals");
    }
    const vrh_hit_mask* hmask = k->hit_mask;
    if (hmask && path) { set_error("vrh_render: the path-tracing kernel takes no hit mask"); return VRH_ERR_UNSUPPORTED; }
    if (hmask)
    {
        VRH_CHECK(hmask->ctx == ctx, "vrh_render: hit mask of another context");
        VRH_CHECK(sc->info.prim_kind != VRH_PRIM_TRI64 || uint64_t(hmask->num_tc) >= 3ull * (uint64_t(sc->info.max_prim_id) + 1),
                  "vrh_render: hit mask has fewer than 3 tex coords per prim_id");
    }
    rows.sh = shard ? *shard : vrh_shard{ 0, 1, 0, 0 };
    VRH_CHECK(rows.sh.count >= 1 && rows.sh.index < rows.sh.count, "vrh_render: bad shard");
    if (sc->info.prim_kind == VRH_PRIM_GENERIC80 && (rows.sh.count > 1 || rows.sh.packed))
    {
        set_error("vrh_render: generic-primitive scenes do not support shards or render groups (whole frames only)");
        return VRH_ERR_UNSUPPORTED;
    }
    rows.local_bands = vrh_shard_bands(cam->height, rows.sh.index, rows.sh.count);
    VRH_CHECK(rt->width == cam->width, "vrh_render: render target width != camera width");
    rows.frame_rows = cam->height;
    if (rows.sh.packed)
    {
        rows.frame_rows = rt->height / num_frames;
        VRH_CHECK(rows.frame_rows >= rows.local_bands * VRH_BAND_ROWS || rows.local_bands == 0, "vrh_render: packed target too small");
    }
    else VRH_CHECK(rt->height == cam->height * num_frames, "vrh_render: render target height != camera height x frames");
    VRH_CHECK(uint64_t(rt->height) * rt->width < (1ull << 32), "vrh_render: render target too large");
    return VRH_OK;
}

// the device side of the plan: the kernels' LDS formula and the (cached) occupancy query
struct render_device final : launch_device
{
    size_t lds_bytes(const launch_config& c) const override { return render_lds_bytes(c); }
    int blocks_per_cu(const launch_config& c) const override { return render_blocks_per_cu(c); }
};

int plan_render(const vrh_ctx* ctx, const vrh_scene* sc, uint32_t num_frames, const vrh_kernel_desc* k, bool sampler_pass,
                launch_plan& plan)
{
    launch_inputs in;
    in.kernel = k->kind; in.count_tests = (k->flags & VRH_KERNEL_COUNT_TESTS) != 0; in.max_hits = k->max_hits;
    in.generic_shading = k->shading && k->shading->gmaterials;
    in.textured = k->shading && k->shading->num_textures != 0 && k->kind != VRH_KERNEL_PRIMARY && k->kind != VRH_KERNEL_AO;
    in.sampler_pass = sampler_pass; in.hit_mask = k->hit_mask != nullptr; in.num_frames = num_frames;
    in.prim_kind = sc->info.prim_kind; in.max_depth = sc->info.max_depth; in.num_roots = sc->num_roots;
    in.device_bytes = sc->info.device_bytes;
    in.finite_bounds = sc->finite_bounds; in.has_quads = sc->quads != nullptr; in.root_is_pair0 = sc->roots[0] == 0u;
    in.opt = ctx->opt;
    // the AO kernel's 4-wide step leaves out the tn < FLT_MAX compare that tn < radius implies:
    // an AO radius that is not <= FLT_MAX (inf, NaN) walks the binary records instead
    in.radius_finite = k->kind != VRH_KERNEL_AO || k->radius <= FLT_MAX;
    std::string err;
    const int rc = plan_launch(in, render_device{}, plan, err);
    if (rc) set_error(err);
    return rc;
}

int fill_params(render_params& p, const launch_plan& plan, const vrh_ctx* ctx, const vrh_scene* sc, const vrh_rt* rt,
                const vrh_camera* cams, uint32_t num_frames, const vrh_kernel_desc* k, const frame_rows_t& rows,
                uint32_t frame_num, const sampler_pass* sp)
{
    const vrh_camera* cam = cams;
    const bool ao = k->kind == VRH_KERNEL_AO;
    const bool multi = k->kind == VRH_KERNEL_MULTI_HIT;
    p.pairs = sc->pairs; p.prims = sc->prims; p.normals = sc->normals; p.root = sc->roots[0];
    p.num_roots = sc->num_roots;
    for (uint32_t i = 0; i < sc->num_roots; ++i) p.roots[i] = sc->roots[i];
    p.step_limit = sc->info.num_nodes + sc->info.num_indices + 16u;
    p.refill_min = plan.refill_min; p.refill_min_primary = plan.refill_min_primary; p.descent_cap = plan.descent_cap;
    p.ao_gate = plan.ao_gate; p.step_flags = plan.step_flags;
    p.stack_cap = uint32_t(plan.cfg.stack_cap); p.stack_total = plan.stack_total; p.quad_lds = plan.quad_lds;
    p.fast_ok = plan.fast_ok;
    p.quads = sc->quads; p.quad_ok = plan.quad_ok;
    // the AO kernel's 4-wide rays walk the fused records where the scene has them (VRH_FUSED_STEP): step_flags
    // bit 2, and the leaves' exact boxes go with them
    p.aoquads = sc->quads; p.leaf_boxes = nullptr; p.fused_omax = 0.0f;
    p.ao_reach = (k->eps + k->radius) * 1.001f;
    if (VRH_FUSED_STEP && ao && plan.quad_ok && sc->fquads && sc->num_roots == 1)
    {
        p.aoquads = sc->fquads; p.leaf_boxes = sc->leaf_boxes; p.fused_omax = sc->fused_omax;
        p.step_flags |= 4u;
    }
    p.ao_cut = plan.ao_cut; p.ao_share = plan.ao_share;
    for (uint32_t f = 0; f < num_frames; ++f)
    {
        std::memcpy(p.cam[f].eye, cams[f].eye, 12); std::memcpy(p.cam[f].cam_u, cams[f].cam_u, 12);
        std::memcpy(p.cam[f].cam_v, cams[f].cam_v, 12); std::memcpy(p.cam[f].cam_w, cams[f].cam_w, 12);
        // scissor_box (scheduler.h:25-31, default recti(0, 0, w, h) at :175): pixels x0 <= x < x1,
        // y0 <= y < y1 are rendered, the rest of the target is left as it is (cuda_sched.inl:71)
        const uint32_t* sb = cams[f].scissor;
        const bool whole_image = sb[0] == 0 && sb[1] == 0 && sb[2] == 0 && sb[3] == 0;
        p.cam[f].clip[0] = whole_image ? 0u : std::min(sb[0], cam->width);
        p.cam[f].clip[1] = whole_image ? 0u : std::min(sb[1], cam->height);
        p.cam[f].clip[2] = whole_image ? cam->width : std::min(sb[2], cam->width);
        p.cam[f].clip[3] = whole_image ? cam->height : std::min(sb[3], cam->height);
    }
    p.num_frames = num_frames;
    p.frame_num = frame_num;
    p.frame_rows = rows.frame_rows;
    p.width = cam->width; p.height = cam->height;
    p.width_f = float(cam->width); p.height_f = float(cam->height);
    p.samples = ao ? k->samples : 0; p.radius = k->radius; p.eps = k->eps;
    p.samples_recip = ao ? ((1u << 20) + p.samples - 1u) / p.samples : 0u;
    std::memcpy(p.bg, k->bg, 16);
    if (sp)
    {
        p.px_off[0] = sp->off[0]; p.px_off[1] = sp->off[1];
        p.jitter = sp->jitter; p.blend = sp->blend; p.blend_s = sp->s; p.blend_d = sp->d;
        if (sp->inv_mats)
        {
            p.matrix_cam = 1u;
            std::memcpy(p.inv_view, sp->inv_mats, sizeof(p.inv_view));
            std::memcpy(p.inv_proj, sp->inv_mats + 16, sizeof(p.inv_proj));
        }
    }
    p.shard_index = rows.sh.index; p.shard_count = rows.sh.count; p.packed = rows.sh.packed ? 1u : 0u;
    p.tiles_x = (cam->width + 7u) / 8u;
    p.num_tiles = rows.local_bands * p.tiles_x;        // a band is one row of 8x8 tiles
    VRH_CHECK(uint64_t(p.num_tiles) * 64u * num_frames < (1ull << 32) && p.num_tiles < (1u << 26), "vrh_render: image too large");
    p.color = rt->color; p.prim_id = rt->prim_id; p.t = rt->t;
    p.occ = (k->flags & VRH_KERNEL_NO_OCC) ? nullptr : rt->occ;
    p.counters = ctx->counters;
    p.xcd_queues = plan.xcd_queues; p.cluster = plan.cluster;
    if (plan.cfg.epi != EPI_PLAIN)
    {
        if (k->shading->gmaterials) p.shade.gmaterials = k->shading->gmaterials;
        else p.shade.materials = k->shading->materials;
        p.shade.lights = k->shading->lights;
        p.shade.num_lights = k->shading->num_lights;
        p.shade.per_vertex = k->normal_binding == VRH_NORMALS_PER_VERTEX ? 1u : 0u;
        p.shade.vnormals = sc->vnormals;
        std::memcpy(p.shade.ambient, k->ambient, 16);
        for (int i = 0; i < 3; ++i) p.shade.amb[i] = p.shade.ambient[i] * p.shade.ambient[3];   // plastic.inl:13-16
    }
    p.num_bounces = (k->kind == VRH_KERNEL_WHITTED || k->kind == VRH_KERNEL_PATHTRACING) ? k->num_bounces : 0u;
    if (k->hit_mask && sc->info.prim_kind == VRH_PRIM_TRI64)
        p.hmask = dev::hit_mask_params{ k->hit_mask->tc, k->hit_mask->mask, k->hit_mask->w, k->hit_mask->h };
    if (multi)
    {
        p.max_hits = k->max_hits;
        p.mh_prim_id = rt->mh_prim_id;
        p.mh_t = rt->mh_t;
    }
    return VRH_OK;
}

// device blocks grown on demand: `stream` is drained first (no launch still uses the old blocks), the
// old blocks are freed and the new ones allocated; `have` is 0 while there are none
struct grown_block { void** ptr; size_t bytes; };
int grow_blocks(hipStream_t stream, size_t& have, size_t want, std::initializer_list<grown_block> blocks)
{
    if (want <= have) return VRH_OK;
    VRH_HIP(hipStreamSynchronize(stream));
    for (const grown_block& b : blocks)
        if (*b.ptr) { (void)hipFree(*b.ptr); *b.ptr = nullptr; }
    have = 0;
    for (const grown_block& b : blocks) VRH_HIP(hipMalloc(b.ptr, b.bytes));
    have = want;
    return VRH_OK;
}

// where the launch runs: the context stream with its counter / overflow blocks, or a frame lane
struct launch_site
{
    hipStream_t stream;
    unsigned long long* counters;
    void** spill; size_t* spill_bytes;   // the overflow block of that stream
    vrh_ctx::lane_t* lane;        // null: the context stream
    bool via_scratch;             // the frame renders into the lane's scratch target
    bool fields[4];               // the target's colour, prim id, t, occlusion are written
};

// (an asynchronous frame redirects p's output pointers to the lane's scratch target where it must)
int choose_site(vrh_ctx* ctx, vrh_rt* rt, const vrh_kernel_desc* k, uint32_t num_frames, const sampler_pass* sp, bool async,
                render_params& p, launch_site& site)
{
    site = launch_site{ ctx->stream, ctx->counters, &ctx->spill, &ctx->spill_bytes, nullptr, false,
                        { p.color != nullptr, p.prim_id != nullptr, p.t != nullptr, p.occ != nullptr } };
    if (!async) return VRH_OK;
    // cuda_sched issues a frame and returns (cuda_sched.inl:306-320): frames go round robin over the
    // frame lanes, so this frame's waves fill the CUs the earlier frames' launch tails leave idle
    const uint32_t li = ctx->next_lane;
    vrh_ctx::lane_t* L = &ctx->lane[li];
    if (!L->stream)
    {
        VRH_HIP(hipStreamCreateWithFlags(&L->stream, hipStreamDefault));    // blocking: see vrh_ctx_create
        VRH_HIP(hipEventCreateWithFlags(&L->done, hipEventDisableTiming));
    }
    if (!ctx->main_mark) VRH_HIP(hipEventCreateWithFlags(&ctx->main_mark, hipEventDisableTiming));
    if (!rt->lane_written) VRH_HIP(hipEventCreateWithFlags(&rt->lane_written, hipEventDisableTiming));
    ctx->next_lane = (ctx->next_lane + 1u) % ctx->num_lanes;
    const hipStream_t S = L->stream;
    site.lane = L; site.stream = S; site.counters = L->counters;
    site.spill = &L->spill; site.spill_bytes = &L->spill_bytes;
    // after everything issued on the context stream before this call (clears, uploads, frames there)
    VRH_HIP(hipEventRecord(ctx->main_mark, ctx->stream));
    VRH_HIP(hipStreamWaitEvent(S, ctx->main_mark, 0));
    if (rt->written_pending) VRH_HIP(hipStreamWaitEvent(S, rt->written, 0));
    // a primary / AO frame of one image through a sampler that does not read the target writes every
    // field of the target at every pixel of its scissor box: it may go through the scratch target,
    // and it supersedes a pending scratch copy into this target of no larger box (that frame's pixels
    // would never be seen: they are dropped, not copied).  Any other pending copy into this target,
    // and one still in this lane's scratch target, is issued first.
    // (a formatted target's resolve pass reads the frame where its kernel wrote it: never through the scratch target)
    const bool scratch_ok = num_frames == 1 && (k->kind == VRH_KERNEL_PRIMARY || k->kind == VRH_KERNEL_AO) && (!sp || sp->blend == 0)
                            && !rt->formatted;
    const uint32_t* cl = p.cam[0].clip;
    const bool* fields = site.fields;
    for (uint32_t l = 0; l < uint32_t(VRH_MAX_FRAME_LANES); ++l)
    {
        vrh_ctx::lane_t& Q = ctx->lane[l];
        if (!Q.pending_rt) continue;
        const uint32_t* qc = Q.pending_clip;
        const bool covers = Q.pending_rt == rt && scratch_ok && cl[0] <= qc[0] && cl[1] <= qc[1] && cl[2] >= qc[2]
                            && cl[3] >= qc[3] && fields[0] == Q.pending_fields[0] && fields[1] == Q.pending_fields[1]
                            && fields[2] == Q.pending_fields[2] && fields[3] == Q.pending_fields[3];
        if (covers) Q.pending_rt = nullptr;
        else if (Q.pending_rt == rt || l == li) VRH_HIP(ctx_flush_pending(ctx, int(l)));
    }
    // the target's last writer is the other lane, not yet joined: write order must hold.  A frame that
    // may go through the scratch target renders there now, and its copy becomes the lane's pending
    // copy (issued when something else needs the target, dropped when a later frame supersedes it);
    // anything else waits for that writer
    const bool other_writer = rt->lane >= 0 && rt->lane != int(li) && rt->lane_epoch == ctx->join_epoch;
    if (other_writer && scratch_ok)
    {
        const size_t n = size_t(rt->width) * rt->height;
        const int rc = grow_blocks(S, L->pixels, n, { { (void**)&L->color, n * sizeof(float4) }, { (void**)&L->prim_id, n * sizeof(uint32_t) },
                                                      { (void**)&L->t, n * sizeof(float) }, { (void**)&L->occ, n } });
        if (rc) return rc;
        p.color = fields[0] ? L->color : nullptr;
        p.prim_id = fields[1] ? L->prim_id : nullptr;
        p.t = fields[2] ? L->t : nullptr;
        p.occ = fields[3] ? L->occ : nullptr;
        site.via_scratch = true;
    }
    else if (other_writer)
        VRH_HIP(hipStreamWaitEvent(S, rt->lane_written, 0));
    return VRH_OK;
}

// the stack overflow blocks of the persistent grid and the diagnostics buffers of this launch
int launch_buffers(vrh_ctx* ctx, const launch_config& lc, uint32_t num_frames, int grid, const launch_site& site, render_params& p)
{
    p.counters = site.counters;
    if (lc.spill)
    {
        const size_t bytes = size_t(grid) * (p.stack_total - p.stack_cap) * size_t(lc.block) * sizeof(uint32_t);
        const int rc = grow_blocks(site.stream, *site.spill_bytes, bytes, { { site.spill, bytes } });
        if (rc) return rc;
        p.stack_spill = static_cast<uint32_t*>(*site.spill);
    }

    // per-wave timeline of this launch (diagnostic, VRH_OPT_WAVE_TIMES)
    ctx->wave_times_used = 0;
    if (ctx->opt_wave_times && !lc.list && !lc.sampled)
    {
        const size_t n = size_t(grid) * (lc.block / 64);
        const int rc = grow_blocks(ctx->stream, ctx->wave_times_n, n, { { (void**)&ctx->wave_times, n * 2 * sizeof(unsigned long long) } });
        if (rc) return rc;
        p.wave_times = ctx->wave_times;
        ctx->wave_times_used = n;
    }
    ctx->tile_times_used = 0;
    if (ctx->opt_wave_times == 2 && lc.count && lc.ao && num_frames == 1 && p.num_tiles > 0)
    {
        const size_t bytes = size_t(p.num_tiles) * 3 * sizeof(unsigned long long);
        const int rc = grow_blocks(ctx->stream, ctx->tile_times_n, p.num_tiles, { { (void**)&ctx->tile_times, bytes } });
        if (rc) return rc;
        VRH_HIP(hipMemsetAsync(ctx->tile_times, 0, bytes, ctx->stream));
        p.tile_times = ctx->tile_times;
        ctx->tile_times_used = p.num_tiles;
    }
    return VRH_OK;
}

// (rf: the resolve pass of a formatted target, on the launch's stream right after the frame's kernel, before the
// target's lane_written event; null for a plain target)
int launch_and_record(vrh_ctx* ctx, vrh_rt* rt, const render_params& p, const launch_config& lc, int grid, const launch_site& site,
                      const resolve_frame* rf)
{
    const hipStream_t S = site.stream;
    const uint32_t slot = ctx->frames % VRH_MAX_TIMED_FRAMES;
    while (ctx->ev_start.size() <= slot)
    {
        hipEvent_t a, b;
        VRH_HIP(hipEventCreate(&a));
        VRH_HIP(hipEventCreate(&b));
        ctx->ev_start.push_back(a);
        ctx->ev_stop.push_back(b);
    }
    VRH_HIP(hipMemsetAsync(site.counters, 0, COUNTERS_FRAME * sizeof(unsigned long long), S));
    VRH_HIP(hipEventRecord(ctx->ev_start[slot], S));
    if (p.num_tiles > 0) VRH_HIP(launch_render(p, lc, grid, S));
    // (a resolve that could not be enqueued is reported after the frame's events and bookkeeping: the frame's
    // kernel is in flight, and later frames must still be ordered after its writes)
    const int resolve_rc = rf ? resolve_enqueue(rt, *rf, S) : VRH_OK;
    VRH_HIP(hipEventRecord(ctx->ev_stop[slot], S));
    if (vrh_ctx::lane_t* L = site.lane)
    {
        const uint32_t* cl = p.cam[0].clip;
        if (site.via_scratch)
        {
            // the scissor box of the scratch target -- every pixel a primary / AO frame writes -- is this
            // lane's pending copy into the target (ctx_flush_pending: after the target's previous writer)
            if (cl[2] > cl[0] && cl[3] > cl[1])
            {
                L->pending_rt = rt;
                for (int i = 0; i < 4; ++i) L->pending_clip[i] = cl[i];
                for (int i = 0; i < 4; ++i) L->pending_fields[i] = site.fields[i];
            }
        }
        else
        {
            VRH_HIP(hipEventRecord(rt->lane_written, S));
            rt->lane = int(L - ctx->lane);
            rt->lane_epoch = ctx->join_epoch;
        }
        VRH_HIP(hipEventRecord(L->done, S));
        L->used = true;
    }
    else
        rt->lane = -1;
    ctx->last_counters = site.counters;
    ctx->last_slot = slot;
    ctx->frames++;

    ctx->last = vrh_frame_stats{};
    ctx->last.launches = p.num_tiles > 0 ? 1u : 0u;
    ctx->last.grid_blocks = uint32_t(grid);
    ctx->last.block_threads = uint32_t(lc.block);
    ctx->last.stack_depth = p.stack_total;
    ctx->last.frames = p.num_frames;
    ctx->have_frame = true;
    return resolve_rc;
}

int render_batch_impl(vrh_ctx* ctx, const vrh_scene* sc, vrh_rt* rt, const vrh_camera* cams, uint32_t num_frames,
                      const vrh_kernel_desc* k, const vrh_shard* shard, uint32_t frame_num, const sampler_pass* sp)
{
    frame_rows_t rows;
    int rc = validate_render(ctx, sc, rt, cams, num_frames, k, shard, rows);
    if (rc) return rc;
    // a formatted target: whole single frames only, depth with the matrix camera only; the frame is rendered into
    // the staging buffers with the sampler's blend forced to "store" (same jitter, offsets and frame number, so
    // the same ray), and the resolve pass stores or blends it
    sampler_pass staged;
    resolve_frame rf{};
    const bool formatted = rt->formatted;
    if (formatted)
    {
        if (num_frames > 1) { set_error("vrh_render_batch: a formatted render target takes one frame per call, not a batch"); return VRH_ERR_UNSUPPORTED; }
        if (shard) { set_error("vrh_render: a formatted render target takes whole frames, not shards"); return VRH_ERR_UNSUPPORTED; }
        if ((rc = resolve_refuse(rt, sp && sp->inv_mats, "vrh_render"))) return rc;
        rf.blend = sp ? sp->blend : 0u;
        rf.s = sp ? sp->s : 1.0f; rf.d = sp ? sp->d : 0.0f;
        rf.jitter = sp ? sp->jitter : 0u; rf.frame_num = frame_num;
        if (sp)
        {
            rf.px_off[0] = sp->off[0]; rf.px_off[1] = sp->off[1];
            rf.mats = sp->inv_mats ? sp->mats : nullptr; rf.inv_mats = sp->inv_mats;
            staged = *sp;
            staged.blend = 0u; staged.s = 1.0f; staged.d = 0.0f;
            sp = &staged;
        }
    }
    rc = select_device(ctx);        // the plan's occupancy queries ask the context's device
    if (rc) return rc;
    launch_plan plan;
    rc = plan_render(ctx, sc, num_frames, k, sp != nullptr, plan);
    if (rc) return rc;
    // asynchronous frames (VRH_OPT_ASYNC_FRAMES): whole-image frames go to a frame lane (choose_site);
    // shard renders (render groups record events on the context stream after their renders) and the
    // timeline diagnostics stay on the context stream
    const bool async = ctx->opt_async && !shard && !ctx->opt_wave_times;
    if (!async)
    {
        rc = rt_wait(ctx, rt);
        if (rc) return rc;
    }

    render_params p{};
    rc = fill_params(p, plan, ctx, sc, rt, cams, num_frames, k, rows, frame_num, sp);
    if (rc) return rc;
    const int waves_per_block = plan.cfg.block / 64;
    const uint64_t units = uint64_t(num_frames) * p.num_tiles;
    const int grid = std::max(1, int(std::min<uint64_t>(uint64_t(ctx->num_cus) * plan.per_cu, (units + waves_per_block - 1) / waves_per_block)));

    launch_site site;
    rc = choose_site(ctx, rt, k, num_frames, sp, async, p, site);
    if (rc) return rc;
    rc = launch_buffers(ctx, plan.cfg, num_frames, grid, site, p);
    if (rc) return rc;
    if (formatted) std::memcpy(rf.clip, p.cam[0].clip, sizeof(rf.clip));
    return launch_and_record(ctx, rt, p, plan.cfg, grid, site, formatted ? &rf : nullptr);
}
} // namespace

VRH_API int vrh_sync(vrh_ctx* ctx)
{
    VRH_CHECK(ctx, "vrh_sync: null");
    VRH_HIP(hipSetDevice(ctx->device));
    for (hipEvent_t ev : ctx->group_written) VRH_HIP(hipEventSynchronize(ev));
    const int rc = ctx_drain(ctx);
    return rc ? rc : volume_collect(ctx);
}

VRH_API int vrh_get_tile_times(vrh_ctx* ctx, uint64_t* out, uint64_t capacity, uint64_t* count)
{
    VRH_CHECK(ctx && count, "vrh_get_tile_times: null");
    VRH_HIP(hipSetDevice(ctx->device));
    VRH_HIP(hipStreamSynchronize(ctx->stream));
    *count = ctx->tile_times_used;
    if (out && ctx->tile_times_used)
        VRH_HIP(hipMemcpy(out, ctx->tile_times, std::min<uint64_t>(capacity, 3 * ctx->tile_times_used) * 8, hipMemcpyDeviceToHost));
    return VRH_OK;
}

VRH_API int vrh_ctx_user_queues(vrh_ctx* ctx, uint32_t** queues)
{
    VRH_CHECK(ctx && queues, "vrh_ctx_user_queues: null");
    if (!ctx->user_queues)
    {
        int rc = select_device(ctx);
        if (rc) return rc;
        VRH_HIP(hipMalloc(&ctx->user_queues, 8u * VRH_USER_QUEUE_STRIDE * sizeof(uint32_t)));
    }
    *queues = ctx->user_queues;
    return VRH_OK;
}

VRH_API int vrh_ctx_user_declined(vrh_ctx* ctx, uint32_t** host_word, uint32_t** device_word)
{
    VRH_CHECK(ctx, "vrh_ctx_user_declined: null");
    if (!ctx->user_declined)
    {
        int rc = select_device(ctx);
        if (rc) return rc;
        // pinned, mapped, coherent host memory: a declined walk's store is the host's after the stream
        // is waited for, with no copy per launch or per wait
        void* h = nullptr;
        void* d = nullptr;
        VRH_HIP(hipHostMalloc(&h, 64, hipHostMallocMapped | hipHostMallocCoherent));
        *static_cast<volatile uint32_t*>(h) = 0u;
        hipError_t e = hipHostGetDevicePointer(&d, h, 0);
        if (e != hipSuccess) { (void)hipHostFree(h); set_error(hipGetErrorString(e)); return VRH_ERR_HIP; }
        ctx->user_declined = static_cast<uint32_t*>(h);
        ctx->user_declined_dev = static_cast<uint32_t*>(d);
    }
    if (host_word) *host_word = ctx->user_declined;
    if (device_word) *device_word = ctx->user_declined_dev;
    return VRH_OK;
}

VRH_API int vrh_get_wave_times(vrh_ctx* ctx, uint64_t* out, uint64_t capacity, uint64_t* count, double* ticks_per_ms)
{
    VRH_CHECK(ctx && count, "vrh_get_wave_times: null");
    int rc = select_device(ctx);
    if (rc) return rc;
    if ((rc = ctx_drain(ctx))) return rc;
    *count = ctx->wave_times_used;
    if (ticks_per_ms)
    {
        int khz = 0;
        VRH_HIP(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ctx->device));
        *ticks_per_ms = double(khz);
    }
    if (out && ctx->wave_times_used)
        VRH_HIP(hipMemcpy(out, ctx->wave_times,
                          std::min<uint64_t>(capacity, 2 * ctx->wave_times_used) * 8,
                          hipMemcpyDeviceToHost));
    return VRH_OK;
}

VRH_API int vrh_last_frame_stats(vrh_ctx* ctx, vrh_frame_stats* stats)
{
    VRH_CHECK(ctx && stats, "vrh_last_frame_stats: null");
    VRH_CHECK(ctx->have_frame, "vrh_last_frame_stats: no frame rendered yet");
    int rc = select_device(ctx);
    if (rc) return rc;
    VRH_HIP(hipEventSynchronize(ctx->ev_stop[ctx->last_slot]));
    float ms = 0.0f;
    VRH_HIP(hipEventElapsedTime(&ms, ctx->ev_start[ctx->last_slot], ctx->ev_stop[ctx->last_slot]));
    unsigned long long c[COUNTERS_LINES + 10];
    VRH_HIP(hipMemcpy(c, ctx->last_counters, sizeof(c), hipMemcpyDeviceToHost));
    ctx->last.kernel_ms = ms;
    ctx->last.rays = c[1];
    ctx->last.hits = c[2];
    ctx->last.box_tests = c[3];
    ctx->last.prim_tests = c[4];
    ctx->last.wave_steps = c[6];
    ctx->last.busy_lane_steps = c[7];
    ctx->last.wave_box_iters = c[9];
    ctx->last.wave_prim_iters = c[10];
    ctx->last.wave_box_uniform_iters = c[11];
    ctx->last.l1_lines = c[COUNTERS_LINES];
    ctx->last.vmem_instrs = c[COUNTERS_LINES + 1];
    ctx->last.l1_requests = c[COUNTERS_LINES + 2];
    ctx->last.l1_group_accesses = c[COUNTERS_LINES + 3];
    ctx->last.l1_ideal_accesses = c[COUNTERS_LINES + 4];
    for (int k = 0; k < 5; ++k) ctx->last.l1_group_by_kind[k] = c[COUNTERS_LINES + 5 + k];
    *stats = ctx->last;
    if (c[5] & 1ull) { set_error("traversal step guard tripped: corrupt BVH (rays were cut short)"); return VRH_ERR_HIP; }
    return VRH_OK;
}

VRH_API int vrh_last_handout_stats(vrh_ctx* ctx, vrh_handout_stats* stats)
{
    VRH_CHECK(ctx && stats, "vrh_last_handout_stats: null");
    VRH_CHECK(ctx->have_frame, "vrh_last_handout_stats: no frame rendered yet");
    int rc = select_device(ctx);
    if (rc) return rc;
    VRH_HIP(hipEventSynchronize(ctx->ev_stop[ctx->last_slot]));
    unsigned long long c[9];
    VRH_HIP(hipMemcpy(c, ctx->last_counters + COUNTERS_HANDOUT, sizeof(c), hipMemcpyDeviceToHost));
    vrh_handout_stats s{};
    s.ao_handout_ticks = c[0];
    s.primary_handout_ticks = c[1];
    s.step_ticks = c[2];
    s.loop_ticks = c[3];
    s.ao_handout_events = c[4];
    s.ao_handout_rays = c[5];
    s.ao_handout_slot_runs = c[6];
    s.fused_checks = c[7];
    s.fused_rejects = c[8];
    *stats = s;
    return VRH_OK;
}

VRH_API int vrh_stats_reset(vrh_ctx* ctx)
{
    VRH_CHECK(ctx, "vrh_stats_reset: null");
    int rc = select_device(ctx);
    if (rc) return rc;
    if ((rc = ctx_drain(ctx))) return rc;
    for (int b = 0; b < COUNTER_BLOCKS; ++b)
        VRH_HIP(hipMemset(ctx->counters + size_t(b) * COUNTERS_WORDS + COUNTERS_TOTAL, 0, 16 * sizeof(unsigned long long)));
    ctx->frames = 0;
    return VRH_OK;
}

VRH_API int vrh_get_accum_stats(vrh_ctx* ctx, vrh_accum_stats* out)
{
    VRH_CHECK(ctx && out, "vrh_get_accum_stats: null");
    int rc = select_device(ctx);
    if (rc) return rc;
    if ((rc = ctx_drain(ctx))) return rc;
    vrh_accum_stats a{};
    a.frames = ctx->frames;
    a.timed_frames = std::min<uint32_t>(ctx->frames, VRH_MAX_TIMED_FRAMES);
    a.kernel_ms_min = 1e300;
    for (uint32_t i = 0; i < a.timed_frames; ++i)
    {
        float ms = 0.0f;
        VRH_HIP(hipEventElapsedTime(&ms, ctx->ev_start[i], ctx->ev_stop[i]));
        a.kernel_ms_total += ms;
        a.kernel_ms_min = std::min<double>(a.kernel_ms_min, ms);
        a.kernel_ms_max = std::max<double>(a.kernel_ms_max, ms);
    }
    if (a.timed_frames == 0) a.kernel_ms_min = 0.0;
    // first launch's start to the last launch's end: overlapping (asynchronous) frames count once
    // (asynchronous frames go round robin over the frame lanes: one of the last frames can end after the
    // last one, and a later frame can start before the first -- the span runs from the earliest start of
    // the first VRH_MAX_FRAME_LANES frames to the latest end of the last ones, measured from the first start)
    if (a.frames >= 1 && a.frames <= VRH_MAX_TIMED_FRAMES)
    {
        float end = -1e30f, begin = 0.0f;
        const uint32_t w = std::min<uint32_t>(a.frames, uint32_t(VRH_MAX_FRAME_LANES));
        for (uint32_t i = 0; i < w; ++i)
        {
            float e = 0.0f, s = 0.0f;
            VRH_HIP(hipEventElapsedTime(&e, ctx->ev_start[0], ctx->ev_stop[a.frames - 1 - i]));
            VRH_HIP(hipEventElapsedTime(&s, ctx->ev_start[0], ctx->ev_start[i]));
            end = std::max(end, e);
            begin = std::min(begin, s);
        }
        a.span_ms = double(end) - double(begin);
    }
    for (int b = 0; b < COUNTER_BLOCKS; ++b)
    {
        unsigned long long c[2];
        VRH_HIP(hipMemcpy(c, ctx->counters + size_t(b) * COUNTERS_WORDS + COUNTERS_TOTAL, sizeof(c), hipMemcpyDeviceToHost));
        a.rays += c[0];
        a.hits += c[1];
    }
    *out = a;
    return VRH_OK;
}

VRH_API int vrh_rt_download(vrh_ctx* ctx, vrh_rt* rt, void* color, uint32_t* prim_id, float* t, uint8_t* occ)
{
    VRH_CHECK(ctx && rt, "vrh_rt_download: null");
    int rc = select_device(ctx);
    if (rc) return rc;
    size_t n = size_t(rt->width) * rt->height;
    rc = rt_wait(ctx, rt);
    if (rc) return rc;
    VRH_HIP(hipStreamSynchronize(ctx->stream));
    if ((rc = volume_collect(ctx))) return rc;      // a volume frame its step limit stopped is not delivered
    if (color) { VRH_CHECK(rt->color, "vrh_rt_download: target has no colour buffer"); VRH_HIP(hipMemcpy(color, rt->color, n * 16, hipMemcpyDeviceToHost)); }
    if (prim_id) { VRH_CHECK(rt->prim_id, "vrh_rt_download: target has no prim_id buffer"); VRH_HIP(hipMemcpy(prim_id, rt->prim_id, n * 4, hipMemcpyDeviceToHost)); }
    if (t) { VRH_CHECK(rt->t, "vrh_rt_download: target has no t buffer"); VRH_HIP(hipMemcpy(t, rt->t, n * 4, hipMemcpyDeviceToHost)); }
    if (occ) { VRH_CHECK(rt->occ, "vrh_rt_download: target has no occlusion buffer"); VRH_HIP(hipMemcpy(occ, rt->occ, n, hipMemcpyDeviceToHost)); }
    return VRH_OK;
}

VRH_API int vrh_rt_alloc_multi_hit(vrh_ctx* ctx, vrh_rt* rt, uint32_t max_hits)
{
    VRH_CHECK(ctx && rt, "vrh_rt_alloc_multi_hit: null");
    VRH_CHECK(max_hits >= 1 && max_hits <= VRH_MAX_HITS, "vrh_rt_alloc_multi_hit: max_hits must be in [1, 16]");
    int rc = select_device(ctx);
    if (rc) return rc;
    if (rt->mh_prim_id) { (void)hipFree(rt->mh_prim_id); rt->mh_prim_id = nullptr; }
    if (rt->mh_t) { (void)hipFree(rt->mh_t); rt->mh_t = nullptr; }
    rt->mh_n = 0;
    const size_t n = size_t(rt->width) * rt->height * max_hits;
    VRH_HIP(hipMalloc(&rt->mh_prim_id, n * 4));
    VRH_HIP(hipMalloc(&rt->mh_t, n * 4));
    rt->mh_n = max_hits;
    return VRH_OK;
}

VRH_API int vrh_rt_download_multi_hit(vrh_ctx* ctx, vrh_rt* rt, uint32_t* prim_ids, float* t)
{
    VRH_CHECK(ctx && rt, "vrh_rt_download_multi_hit: null");
    VRH_CHECK(rt->mh_n, "vrh_rt_download_multi_hit: no multi-hit buffers (vrh_rt_alloc_multi_hit)");
    int rc = select_device(ctx);
    if (rc) return rc;
    const size_t n = size_t(rt->width) * rt->height * rt->mh_n;
    rc = rt_wait(ctx, rt);
    if (rc) return rc;
    VRH_HIP(hipStreamSynchronize(ctx->stream));
    if (prim_ids) VRH_HIP(hipMemcpy(prim_ids, rt->mh_prim_id, n * 4, hipMemcpyDeviceToHost));
    if (t) VRH_HIP(hipMemcpy(t, rt->mh_t, n * 4, hipMemcpyDeviceToHost));
    return VRH_OK;
}

VRH_API int vrh_rt_upload(vrh_ctx* ctx, vrh_rt* rt, const void* color, const uint32_t* prim_id, const float* t,
                          const uint8_t* occ)
{
    VRH_CHECK(ctx && rt, "vrh_rt_upload: null");
    int rc = select_device(ctx);
    if (rc) return rc;
    size_t n = size_t(rt->width) * rt->height;
    rc = rt_wait(ctx, rt);
    if (rc) return rc;
    VRH_HIP(hipStreamSynchronize(ctx->stream));
    if (color) { VRH_CHECK(rt->color, "vrh_rt_upload: target has no colour buffer"); VRH_HIP(hipMemcpy(rt->color, color, n * 16, hipMemcpyHostToDevice)); }
    if (prim_id) { VRH_CHECK(rt->prim_id, "vrh_rt_upload: target has no prim_id buffer"); VRH_HIP(hipMemcpy(rt->prim_id, prim_id, n * 4, hipMemcpyHostToDevice)); }
    if (t) { VRH_CHECK(rt->t, "vrh_rt_upload: target has no t buffer"); VRH_HIP(hipMemcpy(rt->t, t, n * 4, hipMemcpyHostToDevice)); }
    if (occ) { VRH_CHECK(rt->occ, "vrh_rt_upload: target has no occlusion buffer"); VRH_HIP(hipMemcpy(rt->occ, occ, n, hipMemcpyHostToDevice)); }
    return VRH_OK;
}

VRH_API int vrh_unshard(vrh_ctx* ctx, uint32_t width, uint32_t height, uint32_t count, const void* gcolor,
                        const uint32_t* gpid, const uint8_t* gocc, uint64_t stride, const vrh_kernel_desc* k,
                        vrh_rt* dst)
{
    VRH_CHECK(ctx && dst && count >= 1, "vrh_unshard: bad argument");
    VRH_CHECK(dst->width == width && dst->height == height, "vrh_unshard: destination size mismatch");
    if (dst->formatted) { set_error("vrh_unshard: a formatted render target is no unshard destination"); return VRH_ERR_UNSUPPORTED; }
    VRH_CHECK(gcolor || !dst->color || (gpid && k), "vrh_unshard: colour needs either gathered colour or prim ids + kernel");
    VRH_CHECK(gcolor || !dst->color || k->kind < VRH_KERNEL_SIMPLE,
              "vrh_unshard: shaded colour cannot be re-derived; gather the colour buffer");
    VRH_CHECK(gcolor || !dst->color || k->kind != VRH_KERNEL_AO || (gocc && k->samples <= 8),
              "vrh_unshard: re-deriving AO colour needs the gathered masks and samples <= 8");
    int rc = select_device(ctx);
    if (rc) return rc;
    if ((rc = rt_wait(ctx, dst))) return rc;
    unshard_params u{};
    u.width = width; u.height = height; u.count = count;
    u.rows_per_shard = VRH_BAND_ROWS * vrh_shard_bands(height, 0, count);
    const uint64_t n = uint64_t(u.rows_per_shard) * width;
    u.gcolor = static_cast<const char*>(gcolor);
    u.gpid = reinterpret_cast<const char*>(gpid);
    u.gocc = reinterpret_cast<const char*>(gocc);
    u.stride_color = stride ? stride : 16 * n;
    u.stride_pid = stride ? stride : 4 * n;
    u.stride_occ = stride ? stride : n;
    u.color = dst->color; u.pid = dst->prim_id; u.occ = dst->occ;
    u.clip[0] = 0; u.clip[1] = 0; u.clip[2] = width; u.clip[3] = height;
    if (k)
    {
        u.ao = k->kind == VRH_KERNEL_AO ? 1u : 0u;
        u.samples = k->samples ? k->samples : 1u;
        std::memcpy(u.bg, k->bg, 16);
    }
    VRH_HIP(launch_unshard(u, ctx->stream));
    return VRH_OK;
}

VRH_API int vrh_build_bvh(const void* prims, uint32_t num_prims, uint32_t kind, void* nodes_out,
                          uint32_t* num_nodes_out, uint32_t* indices_out, uint32_t* max_depth_out)
{
    VRH_CHECK(prims && nodes_out && num_nodes_out && indices_out, "vrh_build_bvh: null argument");
    VRH_CHECK(num_prims >= 1, "vrh_build_bvh: no primitives");
    VRH_CHECK(prim_record_bytes(kind) != 0u, "vrh_build_bvh: unknown prim kind");
    std::string err;
    VRH_CHECK(kind != VRH_PRIM_GENERIC80 || check_generic_types(prims, num_prims, "vrh_build_bvh", err), err);
    try
    {
        return build_bvh(prims, num_prims, kind, static_cast<node32*>(nodes_out), num_nodes_out, indices_out, max_depth_out);
    }
    catch (const std::bad_alloc&) { set_error("vrh_build_bvh: out of host memory"); return VRH_ERR_OOM; }
}

} // extern "C"
