// oracle/vrh_oracle_libm.cpp -- TEST INFRASTRUCTURE ONLY (see vrh_oracle.h).
//
// sinf / cosf of the oracle's path tracer: the host build of include/visionaray_hip/detail/vrh_libm.h
// (glibc 2.35's single-precision routines restated, proven equal to them on all 2^32 inputs by
// tests/test_libm_sincosf.py), behind C linkage.  The oracle's frames then do not depend on the C
// library of the machine they are computed on.
#include "../include/visionaray_hip/detail/vrh_libm.h"

extern "C" float vo_libm_sinf(float x) { return vrh::libm::sinf(x); }
extern "C" float vo_libm_cosf(float x) { return vrh::libm::cosf(x); }
