// The launch plan of vrh_render (visionaray_amd/csrc/vrh_launch.h) on the CPU, host-only.
//
// launch_device is a stated model of a CDNA CU: LDS bytes by the kernels' own formula
// (launch_lds_bytes with the two device-side constants below), blocks per CU = min(register bound,
// 160 KiB / LDS bytes), at least 1, where the register bound is occ waves on each of 4 SIMDs over
// the block's waves.
//
// One sweep skeleton, run once per instance flavour (plain, textured, generic primitives).  A sweep walks
// its part of the input space -- every kernel the flavour is asked for, every legal value of every option
// singly (the plain one also in the combinations tests/test_gpu_schedules.py uses), 1 and 20 frames, the
// launch forms and refusals of its flavour, BVH depths 1..44, a scene below and above 256 MiB -- and asserts:
// every accepted input yields a key of that flavour with an instance; every key of that flavour with an
// instance is produced by some input; stack_cap <= stack_total; spill exactly when stack_cap < stack_total;
// LDS <= 160 KiB, else the call fails with VRH_ERR_UNSUPPORTED and a message; and what its flavour adds
// (flavour_checks).  Its summary line carries a digest of every decision of the sweep.
//
// The sections, by argument (tests/test_launch_plan.py):
//   (none)    one line per named case, then the plain sweep: tests/golden/launch_plan.txt;
//   textured  named cases with no textures attached (lines of launch_plan.txt), then the textured sweep;
//   generic   named cases over triangles (lines of launch_plan.txt), then the generic-primitive sweep;
//   limits    per kernel (primary, ao, simple, whitted) at default options, the greatest BVH depth plan_launch
//             accepts for a generic-primitive scene -- every depth up to it is accepted, the next one is refused
//             for LDS -- as lines "<kernel> <depth>" (tests/gp_cases.py DEPTH_LIMIT records them);
//   flavours  the three sweeps' summary lines, then the whole key domain: key_at / key_index are inverse, an
//             instance exists for exactly the keys the three sweeps produced, nothing outside the domain has
//             one: tests/golden/launch_plan_flavours.txt.
#include "../../visionaray_amd/csrc/vrh_launch.h"

#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

using namespace vrh;

namespace {

constexpr int AO_WAVE_WORDS = 552;    // vrh_kernels.hip dev::AO_WAVE_WORDS
constexpr int WHITTED_WORDS = 12;     // vrh_shade.h dev::WL_WORDS
constexpr size_t CU_LDS = 160u * 1024u;

struct model_device final : launch_device
{
    size_t lds_bytes(const launch_config& c) const override { return launch_lds_bytes(c, AO_WAVE_WORDS, WHITTED_WORDS); }
    int blocks_per_cu(const launch_config& c) const override
    {
        const int reg = c.occ * 4 / (c.block / 64);
        const int lds = int(CU_LDS / lds_bytes(c));
        return std::max(1, std::min(reg, lds));
    }
};

using setting = std::vector<std::pair<int tuning_options::*, int>>;

struct family { const char* name; uint32_t kernel; uint32_t prim; bool tagged; };
const family FAMILIES[] = {
    { "primary_tri", VRH_KERNEL_PRIMARY, VRH_PRIM_TRI64, false }, { "primary_sph", VRH_KERNEL_PRIMARY, VRH_PRIM_SPHERE48, false },
    { "ao_tri", VRH_KERNEL_AO, VRH_PRIM_TRI64, false },           { "ao_sph", VRH_KERNEL_AO, VRH_PRIM_SPHERE48, false },
    { "simple", VRH_KERNEL_SIMPLE, VRH_PRIM_TRI64, false },       { "multi_hit4", VRH_KERNEL_MULTI_HIT, VRH_PRIM_TRI64, false },
    { "whitted", VRH_KERNEL_WHITTED, VRH_PRIM_TRI64, false },     { "path", VRH_KERNEL_PATHTRACING, VRH_PRIM_TRI64, false },
    { "path_generic", VRH_KERNEL_PATHTRACING, VRH_PRIM_TRI64, true },
};
// what a launch asks for beyond its kernel and scene
struct mode { const char* suffix; bool list, sampler, mask, textured, count; };
const mode NONE{ "", false, false, false, false, false }, LIST3{ "_list3", true, false, false, false, false },
           SAMPLER{ "_sampler", false, true, false, false, false }, HIT_MASK{ "_mask", false, false, true, false, false },
           TEXTURED{ "", false, false, false, true, false }, TEXTURED_SAMPLER{ "", false, true, false, true, false },
           COUNTED{ "", false, false, false, false, true };

bool plain_kernel(const family& f) { return f.kernel == VRH_KERNEL_PRIMARY || f.kernel == VRH_KERNEL_AO; }
// what vrh_render's argument validation lets through to the plan
bool supported(const family& f, const mode& m, uint32_t frames)
{
    if (m.list) return plain_kernel(f);
    if (m.sampler) return frames == 1 && (plain_kernel(f) || f.kernel == VRH_KERNEL_PATHTRACING);
    if (m.mask) return f.kernel != VRH_KERNEL_PATHTRACING;
    return true;
}
// the families a flavour is asked for: textures go with a shading, generic primitives take the triangles' place
bool asked_for(instance_flavour fl, const family& f)
{
    return fl == FLAVOUR_TEXTURED ? !plain_kernel(f) : fl == FLAVOUR_GENERIC ? f.prim == VRH_PRIM_TRI64 : true;
}

launch_inputs inputs(const family& f, const mode& m, uint32_t frames, bool count, uint32_t depth, bool big, const setting& s,
                     bool generic = false)
{
    launch_inputs in;
    in.kernel = f.kernel;
    in.count_tests = count || m.count;
    in.max_hits = f.kernel == VRH_KERNEL_MULTI_HIT ? 4 : 0;
    in.generic_shading = f.tagged;
    in.prim_kind = generic ? uint32_t(VRH_PRIM_GENERIC80) : f.prim;
    in.max_depth = depth;
    in.device_bytes = big ? 512ull << 20 : 64ull << 20;
    in.has_quads = true;
    in.num_roots = m.list ? 3 : 1;
    in.num_frames = frames;
    in.sampler_pass = m.sampler;
    in.hit_mask = m.mask;
    in.textured = m.textured;
    for (const auto& o : s) in.opt.*o.first = o.second;
    return in;
}

std::string describe(int rc, const launch_plan& p, const std::string& err)
{
    if (rc) return "rc=" + std::to_string(rc) + " " + err;
    const launch_config& c = p.cfg;
    char buf[512];
    std::snprintf(buf, sizeof(buf),
                  "kind=%d ao=%d count=%d occ=%d epi=%d list=%d batch=%d spill=%d sampled=%d share=%d block=%d stack_cap=%d "
                  "stack_total=%u max_hits=%d per_cu=%d refill_min=%u refill_min_primary=%u descent_cap=%u step_flags=%u ao_gate=%u "
                  "fast_ok=%u quad_ok=%u ao_cut=%u ao_share=%u xcd_queues=%u cluster=%u",
                  c.kind, int(c.ao), int(c.count), c.occ, int(c.epi), int(c.list), int(c.batch), int(c.spill), int(c.sampled),
                  int(c.share), c.block, c.stack_cap, p.stack_total, c.max_hits, p.per_cu, p.refill_min, p.refill_min_primary,
                  p.descent_cap, p.step_flags, p.ao_gate, p.fast_ok, p.quad_ok, p.ao_cut, p.ao_share, p.xcd_queues, p.cluster);
    return buf;
}

// tests/test_gpu_schedules.py VARIANTS (ao_schedule is accepted and stored nowhere)
#define O(field) &tuning_options::field
const std::pair<const char*, setting> VARIANTS[] = {
    { "step", {} },
    { "refill1", { { O(refill), 1 } } },
    { "global_queue", { { O(xcd_queues), 2 } } },
    { "band_interleaved_queues", { { O(xcd_queues), 3 } } },
    { "cluster_queues", { { O(xcd_queues), 4 }, { O(cluster), 5 } } },
    { "step_wide", { { O(wide), 1 } } },
    { "step_wide_exact", { { O(wide), 1 }, { O(exact_minmax), 1 } } },
    { "step_cap1", { { O(dcap), 1 } } },
    { "step_refill24", { { O(refill), 24 } } },
    { "step_cap3_wide", { { O(dcap), 3 }, { O(wide), 1 } } },
    { "step_pop_on_miss", { { O(pop), 1 } } },
    { "step_pop_cap2_wide", { { O(pop), 1 }, { O(dcap), 2 }, { O(wide), 1 } } },
    { "scalar_off", { { O(scalar), 2 } } },
    { "scalar_off_pop_cap2", { { O(scalar), 2 }, { O(pop), 1 }, { O(dcap), 2 } } },
    { "occ5", { { O(occ), 5 } } },
    { "occ6", { { O(occ), 6 } } },
    { "no_pop_uncapped", { { O(pop), 2 }, { O(dcap), 1024 }, { O(refill), 16 } } },
    { "pop_cap10", { { O(pop), 1 }, { O(dcap), 10 } } },
    { "ao_round1", { { O(gate), 2 }, { O(wide), 2 }, { O(pop), 2 } } },
    { "ao_gate_binary", { { O(gate), 1 }, { O(wide), 2 } } },
    { "ao_ungated_wide", { { O(gate), 2 }, { O(wide), 1 } } },
    { "ao_cut_off", { { O(cut), 2 } } },
    { "ao_cut_refill1_cap1", { { O(cut), 1 }, { O(refill), 1 }, { O(dcap), 1 } } },
    { "stack_lds4", { { O(stack), 4 } } },
    { "stack_lds8_binary", { { O(stack), 8 }, { O(wide), 2 } } },
    { "pair_layout", { { O(layout), 1 } } },
};

// every option with its legal non-zero values lo, lo + step, ..., hi (include/vrh.h; waves per SIMD: 1, 5, 6, 8)
struct option_values { int tuning_options::* field; int lo, hi, step; };
const option_values OPTIONS[] = {
    { O(block), 64, 256, 64 }, { O(stack), 1, 640, 1 }, { O(refill), 1, 64, 1 }, { O(dcap), 1, 1024, 1 }, { O(bpc), 1, 32, 1 },
    { O(occ), 1, 8, 1 }, { O(exact_minmax), 1, 1, 1 }, { O(xcd_queues), 1, 4, 1 }, { O(wide), 1, 2, 1 }, { O(pop), 1, 2, 1 },
    { O(scalar), 1, 2, 1 }, { O(layout), 1, 2, 1 }, { O(gate), 1, 2, 1 }, { O(cut), 1, 3, 1 }, { O(share), 1, 2, 1 },
    { O(cluster), 1, 1024, 1 },
};
#undef O

void named_case(const std::string& name, const launch_inputs& in)
{
    launch_plan p{};
    std::string err;
    const int rc = plan_launch(in, model_device{}, p, err);
    if (!rc && p.cfg.flavour != FLAVOUR_PLAIN) { std::printf("FAILED: a plain input gives a plan of another flavour\n"); std::exit(1); }
    std::printf("%s: %s\n", name.c_str(), describe(rc, p, err).c_str());
}

void named_cases()
{
    const uint32_t depths[] = { 12, 26, 40 };
    for (const family& f : FAMILIES)
        for (uint32_t frames : { 1u, 20u })
            for (int count = 0; count < 2; ++count)
                for (uint32_t d : depths)
                    for (int big = 0; big < 2; ++big)
                        named_case(std::string(f.name) + "_f" + std::to_string(frames) + (count ? "_count" : "") + "_d" + std::to_string(d)
                                       + (big ? "_big" : "_small"), inputs(f, NONE, frames, count, d, big, {}));
    for (const family& f : FAMILIES)
        for (const mode& m : { LIST3, SAMPLER, HIT_MASK })
            for (uint32_t frames : { 1u, 20u })
                for (int count = 0; count < 2; ++count)
                    for (int big = 0; big < 2; ++big)
                    {
                        if (!supported(f, m, frames) || (m.mask && frames == 1) || (m.sampler && count) || (!m.sampler && big)) continue;
                        named_case(std::string(f.name) + m.suffix + "_f" + std::to_string(frames) + (count ? "_count" : "") + "_d26"
                                       + (big ? "_big" : "_small"), inputs(f, m, frames, count, 26, big, {}));
                    }
    for (const family* f : { &FAMILIES[2], &FAMILIES[3] })
        for (int share : { 1, 2 })
            for (uint32_t frames : { 1u, 20u })
                for (uint32_t d : depths)
                    named_case(std::string(f->name) + "_share" + std::to_string(share) + "_f" + std::to_string(frames) + "_d" + std::to_string(d),
                               inputs(*f, NONE, frames, false, d, false, { { &tuning_options::share, share } }));
    for (const auto& v : VARIANTS)
        for (const family* f : { &FAMILIES[2], &FAMILIES[0] })
            named_case(std::string(f->name) + "_" + v.first, inputs(*f, NONE, 1, false, 26, false, v.second));
}

// the families a flavour is asked for, with nothing of the flavour set: the plans of the recorded file, in its
// format (the names are named_cases')
void recorded_cases(instance_flavour fl)
{
    for (const family& f : FAMILIES)
        for (uint32_t frames : { 1u, 20u })
            for (uint32_t d : { 12u, 40u })
                if (asked_for(fl, f)) named_case(std::string(f.name) + "_f" + std::to_string(frames) + "_d" + std::to_string(d) + "_small",
                                                 inputs(f, NONE, frames, false, d, false, {}));
}

#define REQUIRE(cond, what)                                                                       \
    do { if (!(cond)) { std::printf("FAILED %s: %s\n    %s\n", what, #cond, line().c_str()); std::exit(1); } } while (0)

const char* const FLAVOUR_NAMES[] = { "", "textured ", "generic " };

// an instance exists exactly for the produced keys among those of a flavour (-1: of the whole key domain); nothing
// outside the key domain has one; returns the number of those keys
size_t check_keys(const std::vector<bool>& produced, int flavour)
{
    size_t n_keys = 0;
    for (size_t i = 0; i < NUM_KEYS; ++i)
    {
        const instance_key k = key_at(i);
        const auto line = [&] { return "key " + std::to_string(i); };
        REQUIRE(key_index(k) == i, "key_at / key_index");
        if (flavour >= 0 && k.flavour != flavour) continue;
        REQUIRE(instance_exists(k) == bool(produced[i]), "an instance exists exactly for the keys the plan produces");
        n_keys += produced[i] ? 1 : 0;
    }
    for (int kind = -1; kind <= 2; ++kind)
        for (int occ = 0; occ <= 9; ++occ)
            for (int epi = -1; epi <= 6; ++epi)
                for (int fl = -1; fl <= 3; ++fl)
                {
                    instance_key k{};
                    k.kind = kind; k.occ = occ; k.epi = epilogue(epi); k.flavour = instance_flavour(fl);
                    const auto line = [&] { return "kind " + std::to_string(kind) + " occ " + std::to_string(occ) + " epi " + std::to_string(epi)
                                                   + " flavour " + std::to_string(fl); };
                    REQUIRE(!instance_exists(k) || key_index(k) < NUM_KEYS, "no instance outside the key domain");
                }
    return n_keys;
}

// what a flavour's sweep asserts of an input beyond the common checks
void flavour_checks(instance_flavour fl, const family& f, const mode& m, uint32_t frames, bool count, uint32_t depth, int rc,
                    const launch_plan& p, const std::string& err, uint64_t& n_lds)
{
    const auto line = [&] { return std::string(f.name) + ": " + describe(rc, p, err); };
    const launch_config& c = p.cfg;
    if (fl == FLAVOUR_TEXTURED && !rc)
    {
        REQUIRE(f.kernel != VRH_KERNEL_MULTI_HIT && !count, "multi_hit and test counting take no textures");
        REQUIRE(uint32_t(c.stack_cap) == p.stack_total && !c.spill, "the whole stack in LDS");
    }
    if (fl != FLAVOUR_GENERIC) return;
    // what the generic-primitive instances cover: primary / AO / simple / whitted, one frame, one BVH, nothing else asked for
    const bool covered = (plain_kernel(f) || f.kernel == VRH_KERNEL_SIMPLE || f.kernel == VRH_KERNEL_WHITTED) && !f.tagged && !m.list
                      && !m.sampler && !m.mask && !m.textured && !m.count && frames == 1;
    if (rc)
    {
        // it is refused only where the stack does not fit a CU's LDS
        if (covered)
        {
            REQUIRE(err.find("LDS") != std::string::npos, "a covered input is refused for LDS only");
            ++n_lds;
        }
        else
            REQUIRE(err.find("generic-primitive") != std::string::npos, "the refusal names the gap");
        return;
    }
    REQUIRE(covered, "only primary, AO, simple and whitted on one frame and one BVH are accepted");
    REQUIRE(c.kind == 0, "the triangles' records");
    REQUIRE(uint32_t(c.stack_cap) == p.stack_total && !c.spill && p.stack_total >= depth, "the whole stack in LDS");
    REQUIRE(!c.share && p.ao_share == 0u && !c.batch && !c.list && !c.sampled && !c.count, "the one-frame step loop");
}

// the sweep of one flavour: marks the keys it produces, prints its summary line
void sweep(instance_flavour fl, std::vector<bool>& produced)
{
    std::vector<setting> settings{ {} };
    for (const option_values& o : OPTIONS)
        for (int v = o.lo; v <= o.hi; v += o.step)
            if (o.field != &tuning_options::occ || v == 1 || v == 5 || v == 6 || v == 8) settings.push_back({ { o.field, v } });
    if (fl == FLAVOUR_PLAIN)
        for (const auto& v : VARIANTS) settings.push_back(v.second);
    std::vector<uint32_t> depths;
    for (uint32_t d = 1; d <= 44; ++d) depths.push_back(d);
    if (fl == FLAVOUR_GENERIC)      // deep trees, with the default options: the whole stack has to fit the LDS
        for (uint32_t d : { 100u, 400u, 636u, 640u, 644u, 700u }) depths.push_back(d);
    // test counting: of the generic flavour one of the modes refused by name, else swept against every mode
    const std::vector<mode> modes = fl == FLAVOUR_PLAIN ? std::vector<mode>{ NONE, LIST3, SAMPLER, HIT_MASK }
                                  : fl == FLAVOUR_TEXTURED ? std::vector<mode>{ TEXTURED, TEXTURED_SAMPLER }
                                  : std::vector<mode>{ NONE, LIST3, SAMPLER, HIT_MASK, TEXTURED, COUNTED };
    const int counts = fl == FLAVOUR_GENERIC ? 1 : 2;

    uint64_t digest = 1469598103934665603ull, n_inputs = 0, n_accepted = 0, n_lds = 0;
    const model_device dev;
    for (const family& f : FAMILIES)
        for (const mode& m : modes)
            for (uint32_t frames : { 1u, 20u })
                for (int count = 0; count < counts; ++count)
                    for (uint32_t depth : depths)
                        for (int big = 0; big < 2; ++big)
                            for (const setting& s : settings)
                            {
                                // (a generic-primitive scene meets the whole of what can be asked for and refuses by name)
                                if (!asked_for(fl, f) || (fl != FLAVOUR_GENERIC && !supported(f, m, frames)) || (depth > 44 && !s.empty())) continue;
                                const launch_inputs in = inputs(f, m, frames, count != 0, depth, big != 0, s, fl == FLAVOUR_GENERIC);
                                launch_plan p{};
                                std::string err;
                                const int rc = plan_launch(in, dev, p, err);
                                const auto line = [&] { return std::string(f.name) + ": " + describe(rc, p, err); };
                                const launch_config& c = p.cfg;
                                // FNV-1a over the error code and, of an accepted input, every field describe() prints (the
                                // plain sweep's digest is the recorded one of launch_plan.txt; the others take in the
                                // refusal's text too)
                                const int64_t fields[] = { rc, c.kind, c.ao, c.count, c.occ, c.epi, c.list, c.batch, c.spill, c.sampled, c.share,
                                                           c.block, c.stack_cap, p.stack_total, c.max_hits, p.per_cu, p.refill_min,
                                                           p.refill_min_primary, p.descent_cap, p.step_flags, p.ao_gate, p.fast_ok, p.quad_ok,
                                                           p.ao_cut, p.ao_share, p.xcd_queues, p.cluster };
                                for (size_t i = 0; i < (rc ? 1u : sizeof(fields) / sizeof(fields[0])); ++i)
                                    digest = (digest ^ uint64_t(fields[i])) * 1099511628211ull;
                                if (fl != FLAVOUR_PLAIN)
                                    for (char ch : err) digest = (digest ^ uint64_t((unsigned char)ch)) * 1099511628211ull;
                                ++n_inputs;
                                flavour_checks(fl, f, m, frames, in.count_tests, depth, rc, p, err, n_lds);
                                if (rc)
                                {
                                    REQUIRE(rc == VRH_ERR_UNSUPPORTED && !err.empty(), "a refused input");
                                    continue;
                                }
                                ++n_accepted;
                                REQUIRE(c.flavour == fl && instance_exists(c) && key_index(c) < NUM_KEYS, "the key has an instance of the flavour");
                                REQUIRE(uint32_t(c.stack_cap) <= p.stack_total, "the LDS part of the stack");
                                REQUIRE(c.spill == (uint32_t(c.stack_cap) < p.stack_total), "the overflow block");
                                REQUIRE(dev.lds_bytes(c) <= CU_LDS, "LDS of a CU");
                                REQUIRE(p.per_cu >= 1 && c.block >= 64 && c.block <= 256 && c.block % 64 == 0, "the launch shape");
                                produced[key_index(c)] = true;
                            }
    // no dead instance: every key of the flavour with an instance was produced
    const size_t n_keys = check_keys(produced, fl);
    const auto line = [] { return std::string("sweep"); };
    REQUIRE(fl != FLAVOUR_GENERIC || n_lds > 0, "some tree is too deep for the LDS stack");
    std::printf("%ssweep ok: inputs=%llu accepted=%llu keys=%zu digest=%016llx\n", FLAVOUR_NAMES[fl], (unsigned long long)n_inputs,
                (unsigned long long)n_accepted, n_keys, (unsigned long long)digest);
}

// the deepest generic-primitive BVH each kernel takes at default options
void limits()
{
    const std::pair<const char*, uint32_t> kernels[] = { { "primary", VRH_KERNEL_PRIMARY }, { "ao", VRH_KERNEL_AO },
                                                          { "simple", VRH_KERNEL_SIMPLE }, { "whitted", VRH_KERNEL_WHITTED } };
    for (const auto& k : kernels)
    {
        const family f{ k.first, k.second, VRH_PRIM_TRI64, false };
        uint32_t limit = 0;
        for (uint32_t depth = 1; depth <= 1024; ++depth)
        {
            launch_plan p{};
            std::string err;
            const int rc = plan_launch(inputs(f, NONE, 1, false, depth, false, {}, true), model_device{}, p, err);
            const auto line = [&] { return std::string(k.first) + " depth " + std::to_string(depth) + ": " + describe(rc, p, err); };
            if (!rc)
            {
                REQUIRE(limit + 1 == depth, "every depth up to the limit is accepted");
                REQUIRE(uint32_t(p.cfg.stack_cap) == p.stack_total && p.stack_total >= depth && !p.cfg.spill, "the whole stack in LDS");
                REQUIRE(model_device{}.lds_bytes(p.cfg) <= CU_LDS, "LDS of a CU");
                limit = depth;
            }
            else
                REQUIRE(rc == VRH_ERR_UNSUPPORTED && err.find("LDS") != std::string::npos, "a deeper tree is refused for LDS");
        }
        std::printf("%s %u\n", k.first, limit);
    }
}

} // namespace

int main(int argc, char** argv)
{
    const std::string section = argc > 1 ? argv[1] : "";
    std::vector<bool> produced(NUM_KEYS, false);
    if (section == "")
    {
        named_cases();
        sweep(FLAVOUR_PLAIN, produced);
    }
    else if (section == "textured" || section == "generic")
    {
        const instance_flavour fl = section == "textured" ? FLAVOUR_TEXTURED : FLAVOUR_GENERIC;
        recorded_cases(fl);
        sweep(fl, produced);
    }
    else if (section == "limits")
        limits();
    else if (section == "flavours")
    {
        for (instance_flavour fl : { FLAVOUR_PLAIN, FLAVOUR_TEXTURED, FLAVOUR_GENERIC }) sweep(fl, produced);
        std::printf("key domain ok: keys=%zu instances=%zu\n", size_t(NUM_KEYS), check_keys(produced, -1));
    }
    else
    {
        std::fprintf(stderr, "usage: launch_plan_check [textured | generic | limits | flavours]\n");
        return 2;
    }
    return 0;
}
