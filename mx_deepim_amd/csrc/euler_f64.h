// Euler <-> matrix conversions of lib/pair_matching/RT_transform.py in float64, shared by csrc/se3.hip (RT_transform,
// calc_RT_delta, rot_convert) and csrc/sample.hip (the rendered-pose rule).
#pragma once
#include <hip/hip_runtime.h>

// euler2mat(ai, aj, ak, 'sxyz') (RT_transform.py:240-307, the default axes RT_transform calls it with at :131):
// math.sin/cos take Python floats, so everything is float64
static __device__ inline void euler2mat_sxyz_f64(double ai, double aj, double ak, double* M) {
  const double si = sin(ai), sj = sin(aj), sk = sin(ak);
  const double ci = cos(ai), cj = cos(aj), ck = cos(ak);
  const double cc = ci * ck, cs = ci * sk, sc = si * ck, ss = si * sk;
  M[0] = cj * ck; M[1] = sj * sc - cs; M[2] = sj * cc + ss;
  M[3] = cj * sk; M[4] = sj * ss + cc; M[5] = sj * cs - sc;
  M[6] = -sj;     M[7] = cj * si;      M[8] = cj * ci;
}

// mat2euler(M, 'sxyz') (RT_transform.py:310-373), float64
static __device__ inline void mat2euler_sxyz_f64(const double* M, double* e) {
  const double eps4 = 2.220446049250313e-16 * 4.0;
  const double cy = sqrt(M[0] * M[0] + M[3] * M[3]);
  if (cy > eps4) {
    e[0] = atan2(M[7], M[8]);
    e[1] = atan2(-M[6], cy);
    e[2] = atan2(M[3], M[0]);
  } else {
    e[0] = atan2(-M[5], M[4]);
    e[1] = atan2(-M[6], cy);
    e[2] = 0.0;
  }
}
