// nni_quartet.hpp -- internal: what the quartet kernels share (k_nni_quartet of nni.hip, k_support_quartet of
// nni_support.hip): an edge's four sides as the kernels read them, one pairing of a site's four products, the 4 x 4
// matrix-vector product.  One copy of the arithmetic: a candidate's site term is the same bits in both kernels.
#pragma once
#include "batched.hpp"

// arrangement k: which of the edge's sides are X, Y (children of u') and Z, W (children of v')
static const unsigned int nni_perm[3][4] = {{0, 1, 2, 3}, {0, 2, 1, 3}, {0, 3, 2, 1}};

struct NniSide
{
  const double * clv;           // inner CLV or tip CLV; nullptr: a pattern tip
  const unsigned char * tip;    // the pattern tip's codes
  const unsigned int * scaler;  // nullptr = none
};

struct NniEdge
{
  NniSide s[4];
};

// One pairing of a site's four products, for one rate category (the lane's): u' = x (.) y, v' = z (.) w, the
// per-site scaling rule on each (every entry of the SITE below the threshold: all of them times 2^256, count + 1; the
// site's verdict is the AND over the R lanes of its group), the children's counts added.
template <int R>
__device__ __forceinline__ void nni_pair(const double (&x)[4], const double (&y)[4], const double (&z)[4],
                                         const double (&w)[4], unsigned int cx, unsigned int cy, unsigned int cz,
                                         unsigned int cw, bool scale_u, bool scale_v, unsigned int grp0,
                                         double (&u)[4], double (&v)[4], unsigned int & count)
{
  int below_u = 1, below_v = 1;
#pragma unroll
  for (int j = 0; j < 4; ++j)
  {
    u[j] = x[j] * y[j];
    v[j] = z[j] * w[j];
    below_u &= (u[j] < PLLHIP_SCALE_THRESHOLD) ? 1 : 0;
    below_v &= (v[j] < PLLHIP_SCALE_THRESHOLD) ? 1 : 0;
  }
  int all_u = 1, all_v = 1;
#pragma unroll
  for (int i = 0; i < R; ++i)
  {
    all_u &= __shfl(below_u, (int)(grp0 + i), 64);
    all_v &= __shfl(below_v, (int)(grp0 + i), 64);
  }
  count = 0;
  if (scale_u)
  {
    count += cx + cy;
    if (all_u)
    {
#pragma unroll
      for (int j = 0; j < 4; ++j) u[j] *= PLLHIP_SCALE_FACTOR;
      count += 1;
    }
  }
  if (scale_v)
  {
    count += cz + cw;
    if (all_v)
    {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] *= PLLHIP_SCALE_FACTOR;
      count += 1;
    }
  }
}

// y[j] = sum_s m[j][s] a[s], in state order
__device__ __forceinline__ void nni_matvec(const double * __restrict__ m, const double (&a)[4], double (&y)[4])
{
#pragma unroll
  for (int j = 0; j < 4; ++j)
  {
    double t = 0.0;
#pragma unroll
    for (int s = 0; s < 4; ++s) t += m[j * 4 + s] * a[s];
    y[j] = t;
  }
}
