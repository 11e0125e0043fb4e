// tests/cpp/ao_sample_check.cpp -- the AO disk sample of detail/vrh_sampler.h (ao_disk_sample: 16
// candidates searched four at a time) against a plain sequential restatement, on the host.
//
//   1. 2^20 seeded (p, s, salt) triples: the same (sx, sy) bits as the sequential loop;
//   2. pinned samples of 1920x1080 frames whose first accepted candidate has index 4..8, i.e. lies in
//      the second or third group of four: index and value bits (frame 0 reaches index 6, frames 4
//      and 5 indices 7 and 8);
//   3. first_accepted_of16 under forced accept patterns -- all 65536 subsets of the 16 candidates,
//      among them "first accept at k" for k = 0..15 and "none" (which the real predicate meets with
//      probability 0.215^16, so no search finds it): the lowest accepted index, or (0, 0).
// Prints one line per part; exit status 0 iff all hold.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "visionaray_hip/detail/vrh_sampler.h"

namespace {

uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// the sequential search (ao/main.cpp:218-222 over the Appendix-A counters), stated on its own
uint32_t seq_wang(uint32_t a)
{
    a = (a ^ 61u) ^ (a >> 16);
    a = a + (a << 3);
    a = a ^ (a >> 4);
    a = a * 0x27d4eb2du;
    return a ^ (a >> 15);
}
float seq_uniform01(uint32_t k) { return (float)(seq_wang(k) >> 8) * (1.0f / 16777216.0f); }
int seq_disk_sample(uint32_t p, uint32_t s, uint32_t salt, float& sx, float& sy)
{
    sx = 0.0f; sy = 0.0f;
    for (uint32_t k = 0; k < 16; ++k)
    {
        uint32_t ctr = ((p * 8u + s) * 16u + k) * 2u + salt;
        float xa = 2.0f * seq_uniform01(ctr) - 1.0f;
        float ya = 2.0f * seq_uniform01(ctr + 1u) - 1.0f;
        if (xa * xa + ya * ya < 1.0f) { sx = xa; sy = ya; return (int)k; }
    }
    return -1;
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rng()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

struct pin { uint32_t p, s, frame; int index; uint32_t sx, sy; };
// found by a search over the 8 AO samples of every pixel of a 1920x1080 frame (pixel index p, frame
// numbers 0, 4 and 5) with the sequential loop
const pin PINS[] = {
    { 253u, 6u, 0u, 4, 0xbeec5ea4u, 0x3ead91d4u },
    { 1156u, 6u, 0u, 4, 0x3f00a172u, 0x3ea5fe64u },
    { 638u, 6u, 0u, 5, 0xbf08cd58u, 0x3e8850b0u },
    { 965u, 6u, 0u, 5, 0x3eae7c88u, 0xbeeb7518u },
    { 53921u, 1u, 0u, 6, 0x3f548b1au, 0xbebcff04u },
    { 218994u, 5u, 0u, 6, 0xbf577008u, 0x3eb72b2cu },
    { 908864u, 4u, 4u, 7, 0x3e963de8u, 0xbf01dcdcu },
    { 185975u, 5u, 5u, 7, 0xbe7c6508u, 0x3f197c98u },
    { 106996u, 0u, 5u, 8, 0x3dd458a0u, 0x3ed7d508u },
    { 401972u, 4u, 5u, 8, 0x3e8c37b4u, 0x3ed8c2dcu },
};

} // namespace

int main()
{
    int bad = 0;
    // 1. seeded triples
    {
        uint32_t hist[17] = {};
        for (uint32_t i = 0; i < (1u << 20); ++i)
        {
            const uint32_t p = (i & 1u) ? rng() : rng() % (1920u * 1080u);
            const uint32_t s = (i & 2u) ? rng() % 8u : rng() % 32u;
            const uint32_t salt = (i & 4u) ? rng() : (rng() % 64u) * 0x9E3779B1u;
            float ax, ay, bx, by;
            const int k = seq_disk_sample(p, s, salt, ax, ay);
            vrh::dev::ao_disk_sample(p, s, salt, bx, by);
            hist[k + 1] += 1;
            if (bits(ax) != bits(bx) || bits(ay) != bits(by))
            {
                if (bad < 10) std::printf("MISMATCH p=%u s=%u salt=%u index=%d\n", p, s, salt, k);
                bad += 1;
            }
        }
        std::printf("triples: 1048576 compared, first accepted index 0..3: %u, 4..7: %u, 8..15: %u, none: %u\n",
                    hist[1] + hist[2] + hist[3] + hist[4], hist[5] + hist[6] + hist[7] + hist[8],
                    hist[9] + hist[10] + hist[11] + hist[12] + hist[13] + hist[14] + hist[15] + hist[16], hist[0]);
    }
    // 2. pinned samples
    {
        int deep = 0;
        for (const pin& q : PINS)
        {
            float ax, ay, bx, by;
            const uint32_t salt = q.frame * 0x9E3779B1u;                       // vrh_device.h frame_salt
            const int k = seq_disk_sample(q.p, q.s, salt, ax, ay);
            vrh::dev::ao_disk_sample(q.p, q.s, salt, bx, by);
            if (k != q.index || bits(ax) != q.sx || bits(ay) != q.sy || bits(bx) != q.sx || bits(by) != q.sy)
            {
                std::printf("PIN p=%u s=%u frame=%u: index %d (want %d), sequential %08x %08x, grouped %08x %08x, want %08x %08x\n",
                            q.p, q.s, q.frame, k, q.index, bits(ax), bits(ay), bits(bx), bits(by), q.sx, q.sy);
                bad += 1;
            }
            if (q.index < 4) { std::printf("PIN p=%u s=%u: index %d is in the first group\n", q.p, q.s, q.index); bad += 1; }
            deep += q.index >= 8 ? 1 : 0;
        }
        if (deep == 0) { std::printf("PINS: none with index >= 8\n"); bad += 1; }
        std::printf("pins: %d checked, %d with index >= 8\n", (int)(sizeof(PINS) / sizeof(PINS[0])), deep);
    }
    // 3. forced accept patterns: candidate k is (k + 1, -(k + 1)), accepted iff bit k of the mask is set
    {
        auto cand = [](uint32_t k, float& xa, float& ya) { xa = (float)(k + 1u); ya = -(float)(k + 1u); };
        for (uint32_t mask = 0; mask < 65536u; ++mask)
        {
            uint32_t asked = 0;
            float sx = 7.0f, sy = 7.0f;
            vrh::dev::first_accepted_of16(cand, [&](uint32_t k, float xa, float ya) {
                if (xa != (float)(k + 1u) || ya != -(float)(k + 1u)) bad += 1;      // the candidate it was given
                asked |= 1u << k;
                return ((mask >> k) & 1u) != 0u;
            }, sx, sy);
            float wx = 0.0f, wy = 0.0f;
            for (uint32_t k = 0; k < 16u; ++k)
                if ((mask >> k) & 1u) { wx = (float)(k + 1u); wy = -(float)(k + 1u); break; }
            if (bits(sx) != bits(wx) || bits(sy) != bits(wy))
            {
                if (bad < 10) std::printf("PATTERN %04x: got (%g, %g), want (%g, %g)\n", mask, sx, sy, wx, wy);
                bad += 1;
            }
            // whole groups are asked, up to the accepted one's
            const uint32_t first = mask ? (uint32_t)__builtin_ctz(mask) : 15u;
            const uint32_t want_asked = (1u << ((first / 4u + 1u) * 4u)) - 1u;
            if (asked != want_asked) { if (bad < 10) std::printf("PATTERN %04x: asked %04x\n", mask, asked); bad += 1; }
        }
        std::printf("patterns: 65536 accept masks (first accept at 0..15, none)\n");
    }
    if (bad) std::printf("FAILED: %d\n", bad); else std::printf("ok\n");
    return bad ? 1 : 0;
}
