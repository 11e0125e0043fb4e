// The generic-primitive axis of the launch plan (visionaray_amd/csrc/vrh_launch.h: launch_inputs::generic,
// launch_config::generic, generic_instance_exists) on the CPU, host-only, with the device model of
// tests/cpp/launch_plan_check.cpp.
//
// Sweeps the input space of that program with `generic` set -- every kernel, every legal value of every option
// singly, 1 and 20 frames, a list of three BVHs, the sampler pass, the hit-mask mode, a textured shading, tagged
// materials, test counting, BVH depths 1..44 and some up to 700, a scene below and above 256 MiB -- and asserts:
// every accepted input names an existing generic instance (and a key with an instance) with the whole stack in
// LDS; every generic instance is produced by some input; a refused input is VRH_ERR_UNSUPPORTED with a message;
// primary / AO / simple / whitted on one frame, one BVH and nothing else asked for are refused only for LDS.
// Then spot-checks that inputs with generic = false give the plans tests/golden/launch_plan.txt records (named
// cases printed in its format; tests/test_launch_plan_generic.py looks them up there).
//
// `launch_plan_generic_check limits` prints instead, per kernel (primary, ao, simple, whitted) at default options, the
// greatest BVH depth plan_launch accepts for a generic scene -- every depth up to it is accepted, the next one is
// refused for LDS -- as lines "<kernel> <depth>" (tests/gp_cases.py DEPTH_LIMIT records them).
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

struct family { const char* name; uint32_t kernel; bool tagged; bool built; };
const family FAMILIES[] = {
    { "primary_tri", VRH_KERNEL_PRIMARY, false, true }, { "ao_tri", VRH_KERNEL_AO, false, true },
    { "simple", VRH_KERNEL_SIMPLE, false, true },       { "multi_hit4", VRH_KERNEL_MULTI_HIT, false, false },
    { "whitted", VRH_KERNEL_WHITTED, false, true },     { "path", VRH_KERNEL_PATHTRACING, false, false },
    { "path_generic", VRH_KERNEL_PATHTRACING, true, false },
};

struct mode { bool list, sampler, mask, textured, count; };

launch_inputs inputs(const family& f, const mode& m, uint32_t frames, uint32_t depth, bool big, bool generic)
{
    launch_inputs in;
    in.kernel = f.kernel;
    in.count_tests = m.count;
    in.max_hits = f.kernel == VRH_KERNEL_MULTI_HIT ? 4 : 0;
    in.generic_shading = f.tagged;
    in.prim_kind = generic ? uint32_t(VRH_PRIM_GENERIC80) : uint32_t(VRH_PRIM_TRI64);
    in.max_depth = depth;
    in.num_roots = m.list ? 3 : 1;
    in.device_bytes = big ? 512ull << 20 : 64ull << 20;
    in.has_quads = !m.list;
    in.num_frames = frames;
    in.sampler_pass = m.sampler;
    in.hit_mask = m.mask;
    in.textured = m.textured;
    in.generic = generic;
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

struct option_values { int tuning_options::* field; int lo, hi, step; };
#define O(field) &tuning_options::field
const option_values OPTIONS[] = {
    { O(block), 64, 256, 64 }, { O(stack), 1, 640, 1 }, { O(refill), 1, 64, 1 }, { O(dcap), 1, 1024, 1 }, { O(bpc), 1, 32, 1 },
    { O(occ), 1, 8, 1 }, { O(exact_minmax), 1, 1, 1 }, { O(xcd_queues), 1, 4, 1 }, { O(wide), 1, 2, 1 }, { O(pop), 1, 2, 1 },
    { O(scalar), 1, 2, 1 }, { O(layout), 1, 2, 1 }, { O(gate), 1, 2, 1 }, { O(cut), 1, 3, 1 }, { O(share), 1, 2, 1 },
    { O(cluster), 1, 1024, 1 },
};
#undef O

#define REQUIRE(cond, what)                                                                       \
    do { if (!(cond)) { std::printf("FAILED %s: %s\n    %s\n", what, #cond, line().c_str()); std::exit(1); } } while (0)

int sweep()
{
    std::vector<std::pair<int tuning_options::*, int>> settings{ { nullptr, 0 } };
    for (const option_values& o : OPTIONS)
        for (int v = o.lo; v <= o.hi; v += o.step)
            if (o.field != &tuning_options::occ || v == 1 || v == 5 || v == 6 || v == 8) settings.push_back({ o.field, v });
    std::vector<uint32_t> depths;
    for (uint32_t d = 1; d <= 44; ++d) depths.push_back(d);
    for (uint32_t d : { 100u, 400u, 636u, 640u, 644u, 700u }) depths.push_back(d);
    const mode MODES[] = { { false, false, false, false, false }, { true, false, false, false, false },
                           { false, true, false, false, false },  { false, false, true, false, false },
                           { false, false, false, true, false },  { false, false, false, false, true } };
    std::vector<bool> produced(NUM_KEYS, false);
    unsigned long long n_inputs = 0, n_accepted = 0, n_lds = 0;
    const model_device dev;
    for (const family& f : FAMILIES)
        for (const mode& m : MODES)
            for (uint32_t frames : { 1u, 20u })
                for (uint32_t depth : depths)
                    for (int big = 0; big < 2; ++big)
                        for (const auto& s : settings)
                        {
                            if (depth > 44 && s.first) continue;          // the deep trees with the default options
                            launch_inputs in = inputs(f, m, frames, depth, big != 0, true);
                            if (s.first) in.opt.*s.first = s.second;
                            launch_plan p{};
                            std::string err;
                            const int rc = plan_launch(in, dev, p, err);
                            const auto line = [&] { return std::string(f.name) + ": " + describe(rc, p, err); };
                            const bool plain = f.built && !m.list && !m.sampler && !m.mask && !m.textured && !m.count && frames == 1;
                            ++n_inputs;
                            if (rc)
                            {
                                REQUIRE(rc == VRH_ERR_UNSUPPORTED && !err.empty(), "a refused input");
                                // what the instances cover is refused only where the stack does not fit a CU's LDS
                                if (plain)
                                {
                                    REQUIRE(err.find("LDS") != std::string::npos, "a covered input is refused for LDS only");
                                    ++n_lds;
                                }
                                else
                                    REQUIRE(err.find("generic-primitive") != std::string::npos, "the refusal names the gap");
                                continue;
                            }
                            const launch_config& c = p.cfg;
                            ++n_accepted;
                            REQUIRE(plain, "only primary, AO, simple and whitted on one frame and one BVH are accepted");
                            REQUIRE(c.generic && !c.textured && generic_instance_exists(c), "the key has a generic instance");
                            REQUIRE(instance_exists(c) && key_index(c) < NUM_KEYS && c.kind == 0, "the key has an instance");
                            REQUIRE(uint32_t(c.stack_cap) == p.stack_total && !c.spill && p.stack_total >= depth, "the whole stack in LDS");
                            REQUIRE(!c.share && p.ao_share == 0u && !c.batch && !c.list && !c.sampled && !c.count, "the one-frame step loop");
                            REQUIRE(dev.lds_bytes(c) <= CU_LDS, "LDS of a CU");
                            REQUIRE(p.per_cu >= 1 && c.block >= 64 && c.block <= 256 && c.block % 64 == 0, "the launch shape");
                            produced[key_index(c)] = true;
                        }
    size_t n_keys = 0;
    for (size_t i = 0; i < NUM_KEYS; ++i)
    {
        const instance_key k = key_at(i);
        const auto line = [&] { return "key " + std::to_string(i); };
        REQUIRE(!generic_instance_exists(k) || instance_exists(k), "a generic instance is an instance of its key");
        REQUIRE(generic_instance_exists(k) == bool(produced[i]), "a generic instance exists exactly for the keys the plan produces");
        n_keys += produced[i] ? 1 : 0;
    }
    const auto line = [] { return std::string("sweep"); };
    REQUIRE(n_lds > 0, "some tree is too deep for the LDS stack");
    std::printf("generic sweep ok: inputs=%llu accepted=%llu keys=%zu\n", n_inputs, n_accepted, n_keys);
    return 0;
}

// generic = false: the plans of the recorded file, in its format (the names are launch_plan_check.cpp's)
void plain_cases()
{
    const mode none{ false, false, false, false, false };
    for (const family& f : FAMILIES)
        for (uint32_t frames : { 1u, 20u })
            for (uint32_t d : { 12u, 40u })
            {
                launch_plan p{};
                std::string err;
                const int rc = plan_launch(inputs(f, none, frames, d, false, false), model_device{}, p, err);
                if (!rc && p.cfg.generic) { std::printf("FAILED: an input without generic primitives gives a generic plan\n"); std::exit(1); }
                std::printf("%s_f%u_d%u_small: %s\n", f.name, frames, d, describe(rc, p, err).c_str());
            }
}

// the deepest generic BVH each kernel takes at default options
int limits()
{
    const mode none{ false, false, false, false, false };
    const std::pair<const char*, uint32_t> kernels[] = { { "primary", VRH_KERNEL_PRIMARY }, { "ao", VRH_KERNEL_AO },
                                                          { "simple", VRH_KERNEL_SIMPLE }, { "whitted", VRH_KERNEL_WHITTED } };
    for (const auto& k : kernels)
    {
        const family f{ k.first, k.second, false, true };
        uint32_t limit = 0;
        for (uint32_t depth = 1; depth <= 1024; ++depth)
        {
            launch_plan p{};
            std::string err;
            const int rc = plan_launch(inputs(f, none, 1, depth, false, true), model_device{}, p, err);
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
    return 0;
}

} // namespace

int main(int argc, char** argv)
{
    if (argc > 1 && std::string(argv[1]) == "limits") return limits();
    plain_cases();
    return sweep();
}
