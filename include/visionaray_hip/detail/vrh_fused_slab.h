// include/visionaray_hip/detail/vrh_fused_slab.h -- the fused slab test of the AO kernel's 4-wide any-hit step
// and the box widening that makes it conservative ("Fused slab test").  Host and device:
// vrh_quad.cpp widens the boxes at upload, ray_step (vrh_device.h) runs the test, tests/cpp/fused_slab_check.cpp
// runs both on the CPU.
//
// The reference's slab distance is t = RN(RN(b - o) * inv), two VALU operations per bound.  The fused form is
// t' = RN(b' * inv + n) with n = -RN(o * inv) formed once per ray: one v_fma per bound.  It is not the same number,
// so it is applied to a box widened outward by
//     delta(b) = K (|b| + O_max),  K = 2^-22,
// and the claim is:  for every ray with |o| <= O_max, |inv| >= 1/2 and finite o * inv on all three axes (ray_ok),
// if the exact test passes on the exact box, the fused test passes on the widened box.
//
// Proof, one bound of one axis, inv > 0, the lower bound b (the other three cases mirror it).  Round-to-nearest
// is monotone, so t' <= t follows from the same inequality between the real numbers that are rounded last:
//     b' inv + n <= RN(b - o) inv.
// With RN(b - o) = (b - o)(1 + e1), RN(o inv) = o inv (1 + e3) + h3, |e| <= u = 2^-24, |h3| <= 2^-150 (a product
// in the subnormal range; a float subtraction is exact there), b' = b - d, and dividing by inv:
//     d >= -o e3 - (b - o) e1 - h3 / inv,   for which   d >= u (|b| + 2 |o|) + 2^-150 / |inv|   suffices.
// widen() computes d = RN(K RN(|b| + O_max)) and b' = RN(b - d) in float: the three roundings lose at most
// 2 u d + u (|b| + d) of it, so d keeps more than 2.9 u |b| + 3.9 u O_max.  That covers u |b| + 2 u |o| for
// |o| <= O_max, and the absolute term because O_max >= 2^-100 (omax_floor) and |inv| >= 1/2 give
// 2^-150 / |inv| <= 2^-149 < u O_max.  A lower near distance and a higher far distance on every axis keep every
// comparison of the test (tf >= tn, tf >= 0, tn < max_t) true.  An overflow to +-inf keeps the order; n is
// finite (ray_ok) and b', inv are finite, so no t' is NaN.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VRH_FUSED_HD __host__ __device__ __forceinline__
#else
#define VRH_FUSED_HD inline
#endif

namespace vrh {
namespace fused {

constexpr float K = 0x1p-22f;
constexpr float OMAX_FLOOR = 0x1p-100f;
constexpr float FLT_MAX_ = 3.402823466e+38f;

VRH_FUSED_HD float omax_floor(float omax) { return omax > OMAX_FLOOR ? omax : OMAX_FLOOR; }

// the outward shift of bound b: the derived one, or `extra` (VRH_OPT_FUSED_WIDEN: a fraction of the scene
// extent) where that is larger
VRH_FUSED_HD float delta(float b, float omax, float extra)
{
    const float d = K * (__builtin_fabsf(b) + omax_floor(omax));
    return d > extra ? d : extra;
}
VRH_FUSED_HD float widen_lo(float b, float omax, float extra = 0.0f) { return b - delta(b, omax, extra); }
VRH_FUSED_HD float widen_hi(float b, float omax, float extra = 0.0f) { return b + delta(b, omax, extra); }

// one axis of a ray may use the fused records (the kernel's per-ray check at hand-out)
VRH_FUSED_HD bool axis_ok(float o, float inv, float omax)
{
    return (__builtin_fabsf(o) <= omax) & (__builtin_fabsf(o * inv) <= FLT_MAX_) & (__builtin_fabsf(inv) >= 0.5f)
         & (__builtin_fabsf(inv) <= FLT_MAX_);
}
VRH_FUSED_HD bool ray_ok(float ox, float oy, float oz, float ix, float iy, float iz, float omax)
{
    return (int(axis_ok(ox, ix, omax)) & int(axis_ok(oy, iy, omax)) & int(axis_ok(oz, iz, omax))) != 0;
}

// the exact entry test (vrh_device.h quad_entry): t = (b - o) * inv, hardware min / max
template <bool FINITE_MAX_T>
VRH_FUSED_HD bool exact_entry(float xl, float yl, float zl, float xh, float yh, float zh, float ox, float oy, float oz,
                              float ix, float iy, float iz, float max_t, float& tn)
{
    const float t1x = (xl - ox) * ix, t1y = (yl - oy) * iy, t1z = (zl - oz) * iz;
    const float t2x = (xh - ox) * ix, t2y = (yh - oy) * iy, t2z = (zh - oz) * iz;
    tn = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(t1x, t2x), __builtin_fminf(t1y, t2y)), __builtin_fminf(t1z, t2z));
    const float tf = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(t1x, t2x), __builtin_fmaxf(t1y, t2y)), __builtin_fmaxf(t1z, t2z));
    if constexpr (FINITE_MAX_T) return (tf >= tn) & (tf >= 0.0f) & (tn < max_t);
    else return (tf >= tn) & (tn < FLT_MAX_) & (tf >= 0.0f) & (tn < max_t);
}

// the fused entry test: t = fma(b, inv, n), n = -(o * inv)
template <bool FINITE_MAX_T>
VRH_FUSED_HD bool entry(float xl, float yl, float zl, float xh, float yh, float zh, float ix, float iy, float iz,
                        float nx, float ny, float nz, float max_t, float& tn)
{
    const float t1x = __builtin_fmaf(xl, ix, nx), t1y = __builtin_fmaf(yl, iy, ny), t1z = __builtin_fmaf(zl, iz, nz);
    const float t2x = __builtin_fmaf(xh, ix, nx), t2y = __builtin_fmaf(yh, iy, ny), t2z = __builtin_fmaf(zh, iz, nz);
    tn = __builtin_fmaxf(__builtin_fmaxf(__builtin_fminf(t1x, t2x), __builtin_fminf(t1y, t2y)), __builtin_fminf(t1z, t2z));
    const float tf = __builtin_fminf(__builtin_fminf(__builtin_fmaxf(t1x, t2x), __builtin_fmaxf(t1y, t2y)), __builtin_fmaxf(t1z, t2z));
    if constexpr (FINITE_MAX_T) return (tf >= tn) & (tf >= 0.0f) & (tn < max_t);
    else return (tf >= tn) & (tn < FLT_MAX_) & (tf >= 0.0f) & (tn < max_t);
}

} // namespace fused
} // namespace vrh
