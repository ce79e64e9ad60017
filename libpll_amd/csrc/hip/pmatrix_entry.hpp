// pmatrix_entry.hpp -- internal: the arithmetic of one branch's transition-probability matrices, shared by the
// kernels that form them (pmatrix.hip: the partition's model; model_score.hip: a candidate's model block).  One
// function, so a matrix is the same bits whichever kernel made it.
#pragma once
#include "numerics.hpp"

// The workgroup's part -- categories [e_lo, e_lo + e_n) -- of P(t) into pm [R][S][S].  The model arrays are per rate
// matrix ([..][S], [..][S*S], [..]), rates per category; params: the rate matrix of every category; s_expd: [R][S]
// doubles of LDS.  Every thread of the workgroup calls it (one barrier inside, not reached for t == 0 by anybody).
template <typename P>
__device__ __forceinline__ void pmat_branch(double * __restrict__ pm, double t, const double * __restrict__ eigenvals,
                                            const double * __restrict__ eigenvecs,
                                            const double * __restrict__ inv_eigenvecs,
                                            const double * __restrict__ prop_invar, const double * __restrict__ rates,
                                            const P & params, unsigned int S, unsigned int e_lo, unsigned int e_n,
                                            double * s_expd)
{
  if (t == 0.0)
  {
    // zero-length branch: exact identity (core_pmatrix.c:174-179)
    for (unsigned int e = e_lo * S * S + threadIdx.x; e < (e_lo + e_n) * S * S; e += blockDim.x)
    {
      const unsigned int j = (e / S) % S, k = e % S;
      pm[e] = (j == k) ? 1.0 : 0.0;
    }
    return;
  }

  for (unsigned int e = e_lo * S + threadIdx.x; e < (e_lo + e_n) * S; e += blockDim.x)
  {
    const unsigned int n = e / S, m = e % S;
    const unsigned int pi = params[n];
    const double pinv = prop_invar[pi];
    // ((lambda * rate) * t) [/ (1 - pinv)]: core_pmatrix_avx.c:117-130
    double arg = (eigenvals[pi * S + m] * rates[n]) * t;
    if (pinv > 1e-8) arg = arg / (1.0 - pinv);
    s_expd[e] = pll_expm1(arg);
  }
  __syncthreads();

  for (unsigned int e = e_lo * S * S + threadIdx.x; e < (e_lo + e_n) * S * S; e += blockDim.x)
  {
    const unsigned int n = e / (S * S), j = (e / S) % S, k = e % S;
    const unsigned int pi = params[n];
    const double * __restrict__ inv = inv_eigenvecs + (size_t)pi * S * S + j * S;
    const double * __restrict__ vec = eigenvecs + (size_t)pi * S * S + k;
    const double * __restrict__ ex = s_expd + n * S;
    double p;
    if (S == 4)
    {
      // core_pmatrix_avx.c:200-222: four products, pairwise tree, then + I
      p = pairsum4((inv[0] * ex[0]) * vec[0], (inv[1] * ex[1]) * vec[4],
                   (inv[2] * ex[2]) * vec[8], (inv[3] * ex[3]) * vec[12]);
      p = p + ((j == k) ? 1.0 : 0.0);
    }
    else if (S == 20)
    {
      // core_pmatrix_avx2.c:24-37 (ONESTEP) and :236-271: accumulators strided
      // by m mod 4, first step a product, the rest fused, pairwise tree, + 1 on
      // the diagonal
      double acc[4];
      for (unsigned int l = 0; l < 4; ++l) acc[l] = (inv[l] * ex[l]) * vec[l * S];
      for (unsigned int m = 4; m < 20; m += 4)
        for (unsigned int l = 0; l < 4; ++l)
          acc[l] = fma(inv[m + l] * ex[m + l], vec[(m + l) * S], acc[l]);
      p = pairsum4(acc[0], acc[1], acc[2], acc[3]);
      if (j == k) p += 1.0;
    }
    else
    {
      // core_pmatrix.c:226-237: start from I, accumulate left to right
      p = (j == k) ? 1.0 : 0.0;
      for (unsigned int m = 0; m < S; ++m) p += (inv[m] * ex[m]) * vec[m * S];
    }
    pm[e] = p;
  }
}
