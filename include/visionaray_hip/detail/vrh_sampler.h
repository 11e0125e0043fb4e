// include/visionaray_hip/detail/vrh_sampler.h -- the reference's random_sampler<float> and its per-pixel
// seed, restated once for host AND device code.  Used by the user-kernel layer (hip_kernels.h
// random_sampler<float>, hip_detail::pixel_seed) and by the built-in path tracer (vrh_shade.h).
// Also the built-in AO kernel's counter hash and disk sample (ao_disk_sample at
// the end), host-callable so that tests/cpp/ao_sample_check.cpp checks them with g++.
//
// random_sampler<float> (random_sampler.h:24-57): std::default_random_engine -- libstdc++'s
// minstd_rand0, x <- 16807 x mod (2^31 - 1), seeded with seed mod (2^31 - 1) (1 for 0) -- under
// std::uniform_real_distribution<float>(0, 1), i.e. generate_canonical<float, 24> (random.tcc:
// one engine call; (x - 1) as float over float(2^31 - 1 + 1) = 2^31; 1.0 clamped to the float below 1)
// times (1 - 0) plus 0.  Bit-identical to the reference's CPU sampler (tests/test_gpu_ref_kernels.py).
#pragma once

#include <cstdint>

#if defined(__HIP__)
#define VRH_SAMPLER_FN __host__ __device__ inline
#else
#define VRH_SAMPLER_FN inline
#endif

namespace vrh {
namespace dev {

// engine state of a sampler seeded with `seed`
VRH_SAMPLER_FN uint32_t minstd_seed(uint32_t seed)
{
    return seed % 2147483647u == 0u ? 1u : seed % 2147483647u;
}

// random_sampler<float>::next(): advances the engine state x, returns the draw in [0, 1)
VRH_SAMPLER_FN float minstd_next(uint32_t& x)
{
    x = uint32_t((uint64_t(x) * 16807u) % 2147483647u);
    float r = float(x - 1u) / 2147483648.0f;
    if (r >= 1.0f) r = 0.99999994f;             // std::nextafter(1.0f, 0.0f)
    return r * (1.0f - 0.0f) + 0.0f;
}

// cuda_sched.inl:27-36 (the integer hash of thrust's monte_carlo example)
VRH_SAMPLER_FN unsigned seed_hash(unsigned a)
{
    a = (a + 0x7ed55d16u) + (a << 12);
    a = (a ^ 0xc761c23cu) ^ (a >> 19);
    a = (a + 0x165667b1u) + (a << 5);
    a = (a + 0xd3a2646cu) ^ (a << 9);
    a = (a + 0xfd7046c5u) + (a << 3);
    a = (a ^ 0xb55a4f09u) ^ (a >> 16);
    return a;
}

// seed of pixel (x, y) of a w x h image in frame frame_num (32-bit unsigned arithmetic): cuda_sched's
// cuda_hash(tic() + y * w + x) with the clock replaced by frame_num * w * h
VRH_SAMPLER_FN unsigned pixel_seed(unsigned x, unsigned y, unsigned w, unsigned h, unsigned frame_num)
{
    return seed_hash(frame_num * w * h + y * w + x);
}

// SURVEY.md Appendix A counter hash
VRH_SAMPLER_FN uint32_t wang(uint32_t a)
{
    a = (a ^ 61u) ^ (a >> 16);
    a = a + (a << 3);
    a = a ^ (a >> 4);
    a = a * 0x27d4eb2du;
    return a ^ (a >> 15);
}
VRH_SAMPLER_FN float uniform01(uint32_t k) { return (float)(wang(k) >> 8) * (1.0f / 16777216.0f); }

// The first accepted of 16 candidates in index order, searched four at a time: the four candidates
// of a group are formed independently of each other (four hash chains in flight instead of one),
// then the lowest accepted index of the group is taken.  cand(k, xa, ya) forms candidate k,
// accept(k, xa, ya) tests it.  The result is the sequential search's for every input: candidate k is
// selected iff it is accepted and no candidate below k is; none accepted gives sx = sy = 0.
template <class Cand, class Accept>
VRH_SAMPLER_FN void first_accepted_of16(Cand cand, Accept accept, float& sx, float& sy)
{
    sx = 0.0f; sy = 0.0f;
    for (uint32_t g = 0; g < 16u; g += 4u)
    {
        float xa[4], ya[4];
        bool ok[4];
#if defined(__HIP__)
#pragma unroll
#endif
        for (uint32_t j = 0; j < 4u; ++j)
        {
            cand(g + j, xa[j], ya[j]);
            ok[j] = accept(g + j, xa[j], ya[j]);
        }
        // index order: a lower accepted candidate overrides a higher one
        if (ok[3]) { sx = xa[3]; sy = ya[3]; }
        if (ok[2]) { sx = xa[2]; sy = ya[2]; }
        if (ok[1]) { sx = xa[1]; sy = ya[1]; }
        if (ok[0]) { sx = xa[0]; sy = ya[0]; }
        if (ok[0] | ok[1] | ok[2] | ok[3]) break;
    }
}

// candidate k of Appendix A's Malley sample s of pixel p: a point of [-1, 1)^2 from counters
// ((p * 8 + s) * 16 + k) * 2 + salt and the next one (salt: frame_salt of the frame number)
VRH_SAMPLER_FN void ao_disk_candidate(uint32_t p, uint32_t s, uint32_t salt, uint32_t k, float& xa, float& ya)
{
    const uint32_t ctr = ((p * 8u + s) * 16u + k) * 2u + salt;
    xa = 2.0f * uniform01(ctr) - 1.0f;
    ya = 2.0f * uniform01(ctr + 1u) - 1.0f;
}

// the point on the unit disk of AO sample s of pixel p: the first of the 16 candidates inside the
// disk (rejection sampling, ao/main.cpp:218-222), (0, 0) if there is none
VRH_SAMPLER_FN void ao_disk_sample(uint32_t p, uint32_t s, uint32_t salt, float& sx, float& sy)
{
    first_accepted_of16([=](uint32_t k, float& xa, float& ya) { ao_disk_candidate(p, s, salt, k, xa, ya); },
                        [](uint32_t, float xa, float ya) { return xa * xa + ya * ya < 1.0f; }, sx, sy);
}

} // namespace dev
} // namespace vrh
