// Eigenvalues and eigenvectors of a symmetric 3x3 float64 matrix by cyclic Jacobi: what the PCA normals of
// svs_cloudknn.hip and the quadric solve of svs_meshsimplify.hip share.  Both units are compiled with -ffp-contract=off.
#pragma once
#include "svs_common.h"

namespace svs {

constexpr int kJacobiSweeps = 8;                            // quadratic convergence: a 3x3 matrix settles in 4-5 sweeps

// One rotation that annihilates a[P][Q] (Rutishauser's update, as in Numerical Recipes' jacobi); P < Q are compile-time, so
// that a and v stay in registers.
template <int P, int Q>
__device__ __forceinline__ void jacobi_rotate(double (&a)[3][3], double (&v)[3][3]) {
  const double apq = a[P][Q];
  if (apq == 0.0) return;
  const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
  const double t = (theta >= 0.0 ? 1.0 : -1.0) / (__builtin_fabs(theta) + __builtin_sqrt(theta * theta + 1.0));
  // |theta| so large that theta^2 overflows: t = 1 / (2 theta)
  const double tt = __builtin_fabs(theta) > 1e150 ? 0.5 / theta : t;
  const double c = 1.0 / __builtin_sqrt(tt * tt + 1.0), s = tt * c;
  constexpr int R = 3 - P - Q;                              // the third index
  const double app = a[P][P], aqq = a[Q][Q], arp = a[R][P], arq = a[R][Q];
  a[P][P] = app - tt * apq;
  a[Q][Q] = aqq + tt * apq;
  a[P][Q] = a[Q][P] = 0.0;
  a[R][P] = a[P][R] = c * arp - s * arq;
  a[R][Q] = a[Q][R] = s * arp + c * arq;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double vip = v[i][P], viq = v[i][Q];
    v[i][P] = c * vip - s * viq;
    v[i][Q] = s * vip + c * viq;
  }
}

// kJacobiSweeps sweeps, rotations in the order (0,1), (0,2), (1,2): a's diagonal becomes the eigenvalues, the columns of v
// (the identity on entry) their eigenvectors.
__device__ __forceinline__ void jacobi_sweeps(double (&a)[3][3], double (&v)[3][3]) {
#pragma unroll 1
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
    jacobi_rotate<0, 1>(a, v);
    jacobi_rotate<0, 2>(a, v);
    jacobi_rotate<1, 2>(a, v);
  }
}

}  // namespace svs
