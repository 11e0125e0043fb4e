// visionaray_amd/csrc/vrh_launch.h -- the launch plan of vrh_render, host-only C++17 (no HIP header:
// tests/cpp/launch_plan_check.cpp drives it with g++).  Three things live here:
//   * instance_key / instance_exists: which render_unified_kernel instances exist.  The key names every
//     template argument of the kernel -- primitive kind, epilogue, launch form, flavour (plain, textured,
//     generic primitives), ... -- so one key is one instance and key_index identifies it.  vrh_kernels.hip
//     instantiates exactly the keys instance_exists accepts, and plan_launch produces exactly those;
//   * tuning_options: the values of vrh_ctx_set_option the launch policy reads;
//   * plan_launch: kernel description + scene info + options + one occupancy query -> the instance,
//     its block / LDS stack and every tuning value of render_params.  Pure arithmetic: no stream, no
//     allocation (vrh_runtime.hip does those around it).
#pragma once

#include "../../include/vrh.h"

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>

namespace vrh {

// primary-ray epilogue of render_unified_kernel (its EPI template argument)
enum epilogue : int
{
    EPI_PLAIN = 0,          // primary visibility / AO: colour = hit ? 1 : bg
    EPI_SIMPLE = 1,         // VRH_KERNEL_SIMPLE
    EPI_MULTI_HIT = 2,      // VRH_KERNEL_MULTI_HIT
    EPI_WHITTED = 3,        // VRH_KERNEL_WHITTED
    EPI_PATH = 4,           // VRH_KERNEL_PATHTRACING (triangles)
    EPI_PATH_GENERIC = 5,   // VRH_KERNEL_PATHTRACING with a generic shading (tagged material records)
};

// register budget (waves / SIMD) of the path-tracing instances (render_unified_kernel<..., EPI 4 / 5>)
constexpr int PATH_OCC = 5;

// what the instance does beyond its key's other fields (render_unified_kernel's TEX and GEN arguments; one field,
// not two flags: there is no textured generic-primitive instance)
enum instance_flavour : int
{
    FLAVOUR_PLAIN = 0,
    FLAVOUR_TEXTURED = 1,   // TEX: the shading samples its diffuse maps (vrh_shading_set_textures)
    FLAVOUR_GENERIC = 2,    // GEN: the leaf loop walks generic primitives (VRH_PRIM_GENERIC80); kind stays 0
};

// the twelve template arguments of render_unified_kernel, by name (flavour stands for TEX and GEN)
struct instance_key
{
    int kind;          // 0 triangles, 1 spheres
    bool ao;
    bool count;        // VRH_KERNEL_COUNT_TESTS variant
    int occ;           // register budget: min waves per SIMD (1 = uncapped, 5, 6 or 8)
    epilogue epi;
    bool list;         // the step loop over a BVH list
    bool batch;        // frames in flight (the same code under a distinct symbol for profiles)
    bool spill;        // the traversal stack continues in a global overflow block
    bool sampled;      // a pixel-sampler pass (vrh_render_sampled): jittered / offset rays, blended colour
    bool share;        // AO tail sharing: one-frame AO launches at 5 waves / SIMD
    instance_flavour flavour;
};

// The instance set.  The textured and the generic-primitive flavour narrow it first; what is left is decided
// family by family: every register budget exists for the plain, frames-in-flight and shading (simple /
// multi_hit / whitted) instances; every other family at the budgets the defaults choose from.
constexpr bool instance_exists(const instance_key& k)
{
    if (k.flavour < FLAVOUR_PLAIN || k.flavour > FLAVOUR_GENERIC) return false;
    // textured: the simple, whitted and path-tracing epilogues in the launch forms each has, without test
    // counting, and uncapped (occ 1) only: capped at their families' 5 waves / SIMD the whitted and path-tracing
    // ones spill 4-12 VGPRs (12-52 bytes of scratch per lane, -Rpass-analysis=kernel-resource-usage); uncapped
    // they take 103-112 VGPRs (4 waves / SIMD) with no VGPR spill, so a textured launch runs at that lower budget
    // whatever VRH_OPT_WAVES_PER_SIMD asks for
    if (k.flavour == FLAVOUR_TEXTURED && (k.count || k.occ != 1 || k.epi == EPI_PLAIN || k.epi == EPI_MULTI_HIT)) return false;
    // generic primitives: primary visibility, AO, simple and whitted on the one-frame step loop with the whole
    // stack in LDS, uncounted, one register budget each -- primary 6 waves / SIMD, AO and whitted 5, simple
    // uncapped (DESIGN.md section 3 has their resource usage)
    if (k.flavour == FLAVOUR_GENERIC)
    {
        const int occ = k.epi == EPI_PLAIN ? (k.ao ? 5 : 6) : k.epi == EPI_SIMPLE ? 1 : k.epi == EPI_WHITTED ? 5 : 0;
        if (k.kind != 0 || k.count || k.list || k.batch || k.sampled || k.spill || k.share || k.occ != occ) return false;
    }
    if ((k.kind != 0 && k.kind != 1) || (k.occ != 1 && k.occ != 5 && k.occ != 6 && k.occ != 8)) return false;
    const bool step = !k.list && !k.batch && !k.sampled;           // the one-frame step loop
    if (int(k.list) + int(k.batch) + int(k.sampled) > 1) return false;
    if (k.epi != EPI_PLAIN)
    {
        // shading epilogues: triangles, a single BVH, the whole stack in LDS
        if (k.kind != 0 || k.ao || k.list || k.spill || k.share || k.epi < EPI_PLAIN || k.epi > EPI_PATH_GENERIC) return false;
        if (k.epi <= EPI_WHITTED) return step;
        // pathtracing::kernel: one frame, frames in flight and a pixel-sampler pass, at the default
        // register budget and uncapped (occ 1); test counting on one-frame launches, uncapped
        return (k.occ == 1 || k.occ == PATH_OCC) && (!k.count || (k.occ == 1 && step));
    }
    const int occ_family = k.ao ? 5 : 6;
    // BVH lists and pixel-sampler passes at the default register budgets; no counted sampler pass
    if (k.list || k.sampled) return k.occ == occ_family && !k.spill && !k.share && !(k.sampled && k.count);
    // AO tail sharing: uncounted one-frame AO launches at the default 5 waves / SIMD, with and without
    // the stack overflow block
    if (k.share) return k.ao && !k.count && k.occ == 5 && step;
    // the overflow-stack instances exist at the register budgets the defaults choose from: AO 5 or 6
    // waves / SIMD (triangles), primary visibility 6 or 8
    if (k.spill) return !k.count && (k.ao ? k.kind == 0 && (k.occ == 5 || k.occ == 6) : k.occ == 6 || k.occ == 8);
    return !(k.batch && k.count);
}

// The key domain as a mixed-radix index (vrh_kernels.hip builds its table of instances over it).  The compiler
// emits the kernels in the table's order, and the register allocation of some depends on their place in the code
// object (profiles/launch_key/isa_identity.txt): the flavour is the most significant digit and runs generic
// primitives, textured, plain, the order in which the recorded resource usage and profiles were taken
constexpr int KEY_OCCS[4] = { 1, 5, 6, 8 };
constexpr size_t KEYS_PER_FLAVOUR = 2 * 2 * 2 * 4 * 6 * 32;
constexpr size_t NUM_KEYS = KEYS_PER_FLAVOUR * 3;
constexpr instance_key key_at(size_t i)
{
    instance_key k{};
    k.kind = int(i % 2); i /= 2;
    k.ao = i % 2 != 0; i /= 2;
    k.count = i % 2 != 0; i /= 2;
    k.occ = KEY_OCCS[i % 4]; i /= 4;
    k.epi = epilogue(i % 6); i /= 6;
    k.list = (i & 1) != 0; k.batch = (i & 2) != 0; k.spill = (i & 4) != 0; k.sampled = (i & 8) != 0; k.share = (i & 16) != 0; i /= 32;
    k.flavour = instance_flavour(FLAVOUR_GENERIC - int(i));
    return k;
}
// NUM_KEYS for a key outside the domain (no instance)
constexpr size_t key_index(const instance_key& k)
{
    const size_t o = k.occ == 1 ? 0 : k.occ == 5 ? 1 : k.occ == 6 ? 2 : k.occ == 8 ? 3 : 4;
    if ((k.kind != 0 && k.kind != 1) || o == 4 || k.epi < EPI_PLAIN || k.epi > EPI_PATH_GENERIC || k.flavour < FLAVOUR_PLAIN
        || k.flavour > FLAVOUR_GENERIC)
        return NUM_KEYS;
    const size_t flags = size_t(k.list) | size_t(k.batch) << 1 | size_t(k.spill) << 2 | size_t(k.sampled) << 3 | size_t(k.share) << 4;
    return size_t(k.kind) + 2 * (size_t(k.ao) + 2 * (size_t(k.count) + 2 * (o + 4 * (size_t(k.epi) + 6 * (flags
           + 32 * size_t(FLAVOUR_GENERIC - k.flavour))))));
}

// the size of the instance set, flavour by flavour, beside the rule that makes it
constexpr size_t num_instances(instance_flavour f)
{
    size_t n = 0;
    for (size_t i = 0; i < KEYS_PER_FLAVOUR; ++i) n += instance_exists(key_at(size_t(FLAVOUR_GENERIC - f) * KEYS_PER_FLAVOUR + i)) ? 1 : 0;
    return n;
}
static_assert(num_instances(FLAVOUR_PLAIN) == 114 && num_instances(FLAVOUR_TEXTURED) == 8 && num_instances(FLAVOUR_GENERIC) == 4,
              "the render_unified_kernel instances: 114 plain, 8 textured, 4 generic-primitive");

struct launch_config : instance_key
{
    int block;         // threads per block (multiple of 64)
    int stack_cap;     // LDS stack entries per lane
    int max_hits;      // MULTI_HIT: N (LDS hit lists)
};

// dynamic LDS of a launch; `ao_wave_words` (the per-wave AO area) and `whitted_lane_words` (the
// bounce surface per lane) are the kernels' constants (vrh_kernels.hip render_lds_bytes passes them)
inline size_t launch_lds_bytes(const launch_config& c, int ao_wave_words, int whitted_lane_words)
{
    size_t words = size_t(c.stack_cap) * c.block + (c.ao ? size_t(c.block / 64) * ao_wave_words : 0)
                 + (c.epi == EPI_MULTI_HIT ? size_t(5) * c.max_hits * c.block : 0)
                 + (c.epi == EPI_WHITTED ? size_t(whitted_lane_words) * c.block : 0);
    return words * 4;
}

// tuning options (0 = automatic), vrh_ctx_set_option
struct tuning_options
{
    int block = 0, stack = 0, refill = 0, dcap = 0, bpc = 0, occ = 0, exact_minmax = 0, xcd_queues = 0, wide = 0, pop = 0,
        scalar = 0, layout = 0, gate = 0, cut = 0, share = 0, cluster = 0;
};

// what the launch decision reads
struct launch_inputs
{
    uint32_t kernel = VRH_KERNEL_PRIMARY;   // vrh_kernel_desc::kind
    bool count_tests = false;               // VRH_KERNEL_COUNT_TESTS
    uint32_t max_hits = 0;                  // VRH_KERNEL_MULTI_HIT: N
    bool generic_shading = false;           // the shading holds tagged material records
    bool sampler_pass = false, hit_mask = false;     // vrh_render_sampled / vrh_render_view; vrh_kernel_desc::hit_mask
    bool textured = false;                  // the shading has textures attached (vrh_shading_set_textures)
    uint32_t num_frames = 1;
    // the scene: vrh_scene_info and what the upload found (root_is_pair0: roots[0] == 0)
    // (prim_kind VRH_PRIM_GENERIC80: generic primitives, triangles and spheres in one BVH)
    uint32_t prim_kind = VRH_PRIM_TRI64, max_depth = 1, num_roots = 1;
    uint64_t device_bytes = 0;
    bool finite_bounds = true, has_quads = false, root_is_pair0 = true;
    bool radius_finite = true;              // AO: the radius is <= FLT_MAX (the 4-wide step's test relies on it)
    tuning_options opt;
};

// the two questions the plan asks the device side
struct launch_device
{
    virtual size_t lds_bytes(const launch_config& c) const = 0;      // dynamic LDS of a launch of c
    virtual int blocks_per_cu(const launch_config& c) const = 0;     // resident blocks per CU (occupancy query)
    virtual ~launch_device() = default;
};

struct launch_plan
{
    launch_config cfg;
    uint32_t stack_total;     // stack entries per lane in all: cfg.stack_cap in LDS, the rest in the overflow block
    int per_cu;               // blocks per CU the grid is sized for
    uint32_t quad_lds;        // stack entries the AO kernel's 4-wide any-hit walk keeps to (it restarts on the binary
                              // records beyond them): cfg.stack_cap; a counting launch, whose instance holds the
                              // whole stack in LDS, takes the uncounted launch's, so that it counts that launch's tests
    // render_params fields of the same names
    uint32_t refill_min, refill_min_primary, descent_cap, step_flags, ao_gate, fast_ok, quad_ok, ao_cut, ao_share,
             xcd_queues, cluster;
};

// the register budget nearest to `want` at which the family of `k` has an instance: the largest one
// not above it, else the smallest (a family with every budget keeps `want`; 0: it has none)
constexpr int family_occ(instance_key k, int want)
{
    int below = 0, least = 0;
    for (int i = 3; i >= 0; --i)
    {
        k.occ = KEY_OCCS[i];
        if (!instance_exists(k)) continue;
        least = k.occ;
        if (below == 0 && k.occ <= want) below = k.occ;
    }
    return below ? below : least;
}

// A generic-primitive scene: what the launch asks for beyond the instances of that flavour is refused here, by name,
// before anything is planned ("" where nothing is).
inline std::string generic_refusal(const launch_inputs& in)
{
    const char* what = in.num_roots > 1 ? "BVH lists"
                     : in.sampler_pass ? "pixel-sampler passes"
                     : in.num_frames > 1 ? "frames in flight (vrh_render_batch)"
                     : in.count_tests ? "test counting"
                     : in.hit_mask ? "hit masks"
                     : in.textured ? "textures"
                     : in.kernel == VRH_KERNEL_MULTI_HIT ? "multi_hit"
                     : in.kernel == VRH_KERNEL_PATHTRACING ? "the path tracer"
                     : in.generic_shading ? "generic materials"
                     : nullptr;
    return what ? std::string("vrh_render: generic-primitive scenes do not support ") + what
                    + " (primary, AO, simple and whitted, one frame per launch, one BVH)"
                : std::string();
}

inline int plan_launch(const launch_inputs& in, const launch_device& dev, launch_plan& out, std::string& err)
{
    const bool generic = in.prim_kind == VRH_PRIM_GENERIC80;
    if (generic)
    {
        err = generic_refusal(in);
        if (!err.empty()) return VRH_ERR_UNSUPPORTED;
    }
    const tuning_options& opt = in.opt;
    const bool ao = in.kernel == VRH_KERNEL_AO;
    const bool multi = in.kernel == VRH_KERNEL_MULTI_HIT;
    const bool whitted = in.kernel == VRH_KERNEL_WHITTED;
    const bool path = in.kernel == VRH_KERNEL_PATHTRACING;
    const bool shade = in.kernel == VRH_KERNEL_SIMPLE || multi || whitted || path;
    const uint32_t num_frames = in.num_frames;

    // a depth-first traversal holds at most `max_depth` stack entries (>= 1 for the root push):
    // `total` per lane, of which `cap` in LDS (the rest in a global overflow block, chosen below)
    const uint32_t need = std::max<uint32_t>(in.max_depth, 1u);
    const uint32_t total = std::max((need + 3u) & ~3u, uint32_t(opt.stack));
    const uint32_t cap = opt.stack ? uint32_t(opt.stack) : total;
    if (cap < 1u) { err = "vrh_render: stack capacity option must be >= 1"; return VRH_ERR_INVALID; }
    launch_config lc{};
    lc.kind = (generic || in.prim_kind == VRH_PRIM_TRI64) ? 0 : 1;
    // (generic_refusal has turned a textured shading over generic primitives away)
    lc.flavour = generic ? FLAVOUR_GENERIC : in.textured ? FLAVOUR_TEXTURED : FLAVOUR_PLAIN;
    lc.ao = ao;
    lc.count = in.count_tests;
    lc.stack_cap = int(cap);
    lc.epi = path ? (in.generic_shading ? EPI_PATH_GENERIC : EPI_PATH) : whitted ? EPI_WHITTED : multi ? EPI_MULTI_HIT
           : shade ? EPI_SIMPLE : EPI_PLAIN;
    lc.max_hits = multi ? int(in.max_hits) : 0;
    // every kernel runs the step loop (the round-1 item loop for sphere primary visibility measured
    // 6-9 % slower than the step loop with its round-2 defaults, profiles/r02_ab/ab18_sphere_schedule.log,
    // and was removed)
    lc.list = in.num_roots > 1;    // BVH lists: the step loop with the list merge
    if (in.sampler_pass)
    {
        // a pixel-sampler pass runs its own instance (the plain ones keep their code and registers)
        if (lc.list || lc.count) { err = "vrh_render_sampled: pixel samplers take a single BVH and no test counting"; return VRH_ERR_UNSUPPORTED; }
        lc.sampled = true;
    }
    // frames in flight on the step loop (primary / AO without a hit mask, the path tracer; uncounted):
    // the BATCH instantiation
    lc.batch = !lc.list && !lc.sampled && num_frames > 1 && !lc.count && ((lc.epi == EPI_PLAIN && !in.hit_mask) || path);
    // shading epilogues: no VGPR cap (their lane state spills at 6 waves/SIMD; measured faster at 4,
    // profiles/r01/shade/shade_bench.jsonl), except whitted, whose bounce surface lives in LDS (vrh_shade.h):
    // 96 VGPRs without spills, 5 waves/SIMD, +0.7-2.1 % over 4 (profiles/r03_ab/whitted/).
    // pathtracing::kernel (its lane state is registers only: throughput, sampler word, bounce): uncapped
    // the instances take 99-100 VGPRs (4 waves/SIMD); capped at 5 waves/SIMD (PATH_OCC) they
    // fit 94 (one frame, frames in flight) / 96 (sampler pass) VGPRs with no VGPR spill and no scratch
    // (-Rpass-analysis=kernel-resource-usage), so 5 is the default -- not compared on the GPU against 4;
    // waves_per_simd 1 and the counting variant (163 VGPRs) run uncapped.
    // The instances over tagged materials (EPI 5, a generic shading): 96 / 96 / 96 VGPRs capped at PATH_OCC, no
    // VGPR spill and no scratch either; uncapped 110 (4 waves/SIMD), the counting variant 165.
    // AO on the step loop (round 5, the lean lane state: no VGPR spill or scratch at 80 VGPRs, also in
    // the overflow-stack instances): 6 waves/SIMD, the LDS stack shrunk (below) to 16 entries so that 24
    // waves fit a CU, the rest in the overflow block -- hf1M +4.8 %, hf10M +8.7 % over 5 waves
    // (profiles/r05/occupancy/s6_*); AO tail sharing (opt-in) has 5-wave instances only.  Primary
    // visibility: 8 waves/SIMD (64 VGPRs, no spill: hf1M +6.7-11 %, hf10M +3-9 %); spheres with frames in
    // flight too, with the LDS stack shrunk to 20 entries so that 32 waves fit a CU (sph1M +4.8 % over 7
    // waves, profiles/r05/sweepS/ -- at the whole 28-entry stack in LDS only 22 fit, -1 to -4 %,
    // profiles/r05/occupancy/), but one frame per launch at 7 (the occupancy-6 instance: 8 waves with the
    // overflow stack measured -8 %, profiles/r05/s26/); the counting variants keep 5 / 6 (at 8 they
    // spill hundreds of VGPRs).  BVH lists run at 5 / 6
    const int occ_ao = (opt.share == 1 || lc.count) ? 5 : 6;
    const int occ_primary = (!lc.count && (lc.kind == 0 || num_frames > 1)) ? 8 : 6;
    const int occ_default = path ? PATH_OCC : whitted ? 5 : lc.epi ? 1 : lc.ao ? occ_ao : occ_primary;
    // sampler passes, BVH lists, the path tracer and the textured and generic-primitive flavours have instances
    // at some budgets only: the nearest one
    lc.occ = family_occ(lc, opt.occ ? opt.occ : occ_default);
    // a flavour has instances for part of what vrh_render's argument validation lets through
    // (of the plain one, all of it: tests/cpp/launch_plan_check.cpp)
    if (lc.flavour != FLAVOUR_PLAIN && !instance_exists(lc))
    {
        err = generic ? "vrh_render: no generic-primitive instance of this kernel"
            : multi ? "vrh_render: multi_hit takes no textures"
            : lc.count ? "vrh_render: a textured shading has no test-counting instance"
                       : "vrh_render: no textured instance of this kernel";
        return VRH_ERR_UNSUPPORTED;
    }
    // AO tail sharing needs several waves per block (they share LDS): 4 unless the block is set.
    // It has instances for uncounted one-frame AO launches at 5 waves / SIMD only: where there is no
    // SHARE instance the option changes nothing, not even the block size
    lc.share = opt.share == 1;
    lc.share = lc.share && instance_exists(lc);
    lc.block = opt.block ? opt.block : lc.share ? 256 : 64;
    // auto: the LDS part of the stack shrinks (in steps of 4 entries) while LDS, not registers,
    // limits the waves per CU -- a deep BVH (hf10M: depth 26) then keeps the register-bound
    // occupancy and its few deepest entries go to the overflow block
    // (the primary / AO step loops at their default register budgets have overflow-stack instances;
    // every other kernel keeps its whole stack in LDS, as does an explicit VRH_OPT_STACK_CAP >= depth)
    lc.spill = true;
    lc.spill = instance_exists(lc) && (!opt.stack || cap < total);
    if (lc.spill && !opt.stack)
    {
        launch_config lo = lc;
        lo.stack_cap = 4;
        const int reg_bound = dev.blocks_per_cu(lo);
        while (lc.stack_cap > 4 && dev.blocks_per_cu(lc) < reg_bound) lc.stack_cap -= 4;
        // measured: hf10M AO 20 LDS entries +7 % over 24 at the same 20 waves / CU
        // (profiles/r02_ab/ab6_stack.log); no BVH of depth <= 20 spills
        if (total > 20u) lc.stack_cap = std::min(lc.stack_cap, 20);
    }
    if (!lc.spill) lc.stack_cap = int(total);                       // no overflow instance: the whole stack in LDS
    else if (uint32_t(lc.stack_cap) >= total) lc.spill = false;     // nothing overflows: the plain instance
    if (dev.lds_bytes(lc) > 160u * 1024u)
    {
        err = "vrh_render: BVH depth " + std::to_string(in.max_depth) + " needs more LDS stack than a CU has";
        return VRH_ERR_UNSUPPORTED;
    }
    out.cfg = lc;
    out.stack_total = total;
    out.quad_lds = uint32_t(lc.stack_cap);
    if (lc.ao && lc.count)
    {
        launch_inputs plain = in;
        plain.count_tests = false;
        launch_plan p{};
        std::string e;
        // (an uncounted launch that has no plan changes nothing: the counting launch keeps its own LDS entries,
        // which is what it did before; the error, if any, is this launch's own and was reported above)
        if (plan_launch(plain, dev, p, e) == VRH_OK) out.quad_lds = std::min(out.quad_lds, uint32_t(p.cfg.stack_cap));
    }

    // measured: profiles/r01/ab (AO: refill at 32 free lanes), profiles/r01/ab_primary (primary
    // visibility: pop on a miss and a cap of 8 visits per descent step, +6 % on hf1M and +36 % on
    // hf10M; both hurt AO)
    const bool primary_step = !lc.ao && lc.epi == EPI_PLAIN;
    // AO step loop: refill once 24 lanes are free for scenes the 256 MB Infinity Cache holds, 28 above
    // (profiles/r03_ab/refill/, 3 repetitions at 20 frames per launch: hf1M 24 vs 32 +0.6 %, hf10M
    // 28 vs 32 +0.3 % and 24 -0.6 %)
    out.refill_min = opt.refill ? uint32_t(opt.refill) : in.device_bytes > (256ull << 20) ? 28u : 24u;
    // primary visibility with frames in flight refills once 16 lanes are free: +3 % sph1M, +2 % hf1M,
    // +1.8 % hf10M at 20 frames per launch (profiles/r02_ab/ab20_refill.log); simple::kernel and
    // whitted once 8 are: +1-2.5 % / +1 % (profiles/r02_ab/shade_refill.jsonl); one-frame primary
    // launches and multi_hit keep 1
    const uint32_t refill_shade = (lc.epi == EPI_SIMPLE || lc.epi == EPI_WHITTED || lc.epi == EPI_PATH || lc.epi == EPI_PATH_GENERIC) ? 8u : 1u;
    out.refill_min_primary = opt.refill ? uint32_t(opt.refill)
                           : (primary_step && num_frames > 1) ? 16u : lc.epi ? refill_shade : 1u;
    // primary visibility caps a lane's descent at 8 inner visits per step; at 8 waves / SIMD (round 5,
    // profiles/r05/sweepP2/, 20 frames per launch, min over rounds) triangle scenes the Infinity Cache
    // holds run best at 10 (hf1M +3 %; hf10M, above 256 MB, best at 8: 10 is -3 %), spheres at 6
    // (sph1M +1.5 %)
    const uint32_t dcap_primary = in.prim_kind == VRH_PRIM_SPHERE48 ? 6u : in.device_bytes > (256ull << 20) ? 8u : 10u;
    out.descent_cap = opt.dcap ? uint32_t(opt.dcap) : primary_step ? dcap_primary : 0xFFFFFFFFu;
    // shading epilogues (simple / multi_hit / whitted) pop on a miss too: +4-7 % (profiles/r01/shade/)
    // AO (step loop): the tile's AO rays wait for its primaries (ao_gate), any-hit rays descend the
    // 4-wide records and primaries pop on a miss -- together +6 % on hf1M and +10 % on hf10M
    // (profiles/r02_ab/ab4_c4opts.log); each alone is within +-2 %
    // (every kernel is a primary step loop, a shading epilogue or AO: pop on a miss is on unless switched off)
    out.ao_gate = (opt.gate == 1 || (opt.gate == 0 && lc.ao)) ? 1u : 0u;
    const bool pop = opt.pop != 2;
    out.step_flags = (pop ? 1u : 0u) | (opt.scalar == 2 ? 0u : 2u);
    out.fast_ok = (in.finite_bounds && !opt.exact_minmax) ? 1u : 0u;
    // 4-wide any-hit records: auto on for the AO step loop (with ao_gate), off elsewhere
    const bool wide = opt.wide == 1 || (opt.wide == 0 && lc.ao);
    // (the AO kernel restarts a 4-wide descent that would overflow its stack at pair 0: the root)
    // (and its 4-wide box test takes tn < radius to imply tn < FLT_MAX: a non-finite AO radius keeps the binary records)
    out.quad_ok = (in.has_quads && out.fast_ok && wide && in.root_is_pair0 && (!lc.ao || in.radius_finite)) ? 1u : 0u;
    // per-tile entry cut of the 4-wide tree for AO rays (needs the gate: the tile's hits are known)
    // entries nearest-first (+3.5 % over the cut order, profiles/r02_ab/ab33_ao_cut_order*.log)
    out.ao_cut = (out.quad_ok && out.ao_gate && opt.cut != 2) ? (opt.cut == 3 ? 1u : 2u) : 0u;
    out.ao_share = (lc.share && lc.block > 64) ? 1u : 0u;
    // tile queues: per-XCD strips; with frames in flight the band-interleaved order (auto) for AO
    // and for scenes larger than the 256 MB Infinity Cache.  Measured with a camera orbiting 0.5 deg
    // per frame (profiles/r02_ab/ab31_tile_order_orbit_*.log): band order hf10M AO +3.5 %, hf10M
    // primary +10 %, hf1M AO +0.3 %, but hf1M primary -2.8 % (its scene fits the MALL, and a
    // strip's primaries then keep their XCD's L2); one-frame launches keep strips (ab30)
    // AO with frames in flight: cluster order (every XCD on its own strip, the F frames of a cluster of
    // 8 tiles handed out back to back): against the band order, round 4, same box, 20 frames per
    // launch (profiles/r04/ab/cluster_hf{1M,10M}_{static,orbit}.log): hf10M +3.3 % (static camera) / +0.3 % (orbiting 0.5 deg per
    // frame), hf1M +0.9 % / +2.3 %; clusters of 4-16 tiles alike, 240 (a whole band) no gain
    const bool band_auto = num_frames > 1 && (lc.ao || in.device_bytes > (256ull << 20));
    const bool cluster_auto = num_frames > 1 && lc.ao;
    out.xcd_queues = opt.xcd_queues == 2 ? 0u : opt.xcd_queues == 1 ? 1u
                   : opt.xcd_queues == 3 ? 2u : opt.xcd_queues == 4 ? 3u
                   : cluster_auto ? 3u : (band_auto ? 2u : 1u);
    out.cluster = opt.cluster ? uint32_t(opt.cluster) : 8u;

    out.per_cu = dev.blocks_per_cu(lc);
    if (opt.bpc) out.per_cu = std::min(out.per_cu, opt.bpc);
    return VRH_OK;
}

} // namespace vrh
