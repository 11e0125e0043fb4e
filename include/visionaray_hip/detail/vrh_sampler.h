// include/visionaray_hip/detail/vrh_sampler.h -- the reference's random_sampler<float> and its per-pixel
// seed, restated once for host AND device code.  Used by the user-kernel layer (hip_kernels.h
// random_sampler<float>, hip_detail::pixel_seed) and by the built-in path tracer (vrh_shade.h).
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

} // namespace dev
} // namespace vrh
