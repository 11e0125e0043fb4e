// include/visionaray_hip/detail/vrh_octant.h -- the entry test of the AO kernel's 4-wide any-hit step in its octant
// form ("Octant step").  Host and device: ray_step (vrh_device.h) runs it,
// tests/cpp/quad_octant_check.cpp compares it with the sorting form on the CPU.
//
// quad_entry (vrh_device.h; its host mirror is fused::exact_entry) sorts the two plane distances of every axis:
// min(t1, t2) is the near one, max(t1, t2) the far one.  For a ray with a finite inverse direction over a box with
// lo <= hi the sign of inv decides that order once per ray: round to nearest is monotone, so lo - o <= hi - o, and a
// product with inv > 0 keeps the order, with inv < 0 reverses it, with inv = +-0 makes both a zero.  The near
// distance is therefore (lo - o) * inv for inv >= 0 and (hi - o) * inv for inv < 0 -- the same float min / max
// would have returned, up to the sign of a zero, which no compare of the test sees.  (A never-hit box, lo = hi =
// +inf, has equal planes; with inv = +-0 both distances are NaN under either form, and v_max3 / v_min3 drop a NaN
// operand as the nested v_max / v_min do.)
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VRH_OCTANT_HD __host__ __device__ __forceinline__
#else
#define VRH_OCTANT_HD inline
#endif

namespace vrh {
namespace octant {

constexpr float FLT_MAX_ = 3.402823466e+38f;

// a 4-wide record (vrh_quad.cpp): xmin[4] at byte 0, ymin[4] at 16, zmin[4] at 32, xmax[4] at 48, ymax[4] at 64,
// zmax[4] at 80.  The near planes of an axis are its min piece for inv >= 0 and its max piece, HI_PIECE bytes on,
// for inv < 0; the far planes are the other piece
constexpr uint32_t RECORD_BYTES = 128u;
constexpr uint32_t HI_PIECE = 48u;
VRH_OCTANT_HD bool far_first(float inv) { return inv < 0.0f; }
VRH_OCTANT_HD uint32_t near_piece(float inv) { return far_first(inv) ? HI_PIECE : 0u; }
VRH_OCTANT_HD uint32_t far_piece(float inv) { return far_first(inv) ? 0u : HI_PIECE; }

// the entry test on plane values already picked by the ray's octant: (xn, yn, zn) the near planes, (xf, yf, zf)
// the far ones.  The three compares are quad_entry's; FINITE_MAX_T as there
template <bool FINITE_MAX_T>
VRH_OCTANT_HD bool entry(float xn, float yn, float zn, float xf, float yf, float zf, float ox, float oy, float oz,
                         float ix, float iy, float iz, float max_t, float& tn, float& tf)
{
    const float tnx = (xn - ox) * ix, tny = (yn - oy) * iy, tnz = (zn - oz) * iz;
    const float tfx = (xf - ox) * ix, tfy = (yf - oy) * iy, tfz = (zf - oz) * iz;
    tn = __builtin_fmaxf(__builtin_fmaxf(tnx, tny), tnz);
    tf = __builtin_fminf(__builtin_fminf(tfx, tfy), tfz);
    if constexpr (FINITE_MAX_T) return (tf >= tn) & (tf >= 0.0f) & (tn < max_t);
    else return (tf >= tn) & (tn < FLT_MAX_) & (tf >= 0.0f) & (tn < max_t);
}
template <bool FINITE_MAX_T>
VRH_OCTANT_HD bool entry(float xn, float yn, float zn, float xf, float yf, float zf, float ox, float oy, float oz,
                         float ix, float iy, float iz, float max_t, float& tn)
{
    float tf;
    return entry<FINITE_MAX_T>(xn, yn, zn, xf, yf, zf, ox, oy, oz, ix, iy, iz, max_t, tn, tf);
}

} // namespace octant
} // namespace vrh
