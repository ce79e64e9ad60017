/* support_rule.h -- internal: the per-replicate rule of the branch supports (include/pll_amd.h,
 * pll_amd_nni_support), one copy for the host function (host/nni_support.c, C) and the counting kernel
 * (hip/nni_support.hip).  Plain IEEE double operations -- both sides are compiled without contraction --, so the two
 * agree bit for bit; every comparison with a NaN in it is false.
 */
#ifndef PLLHIP_SUPPORT_RULE_H
#define PLLHIP_SUPPORT_RULE_H

#ifdef __HIPCC__
#define SUPPORT_RULE_FN __host__ __device__ static inline
#else
#define SUPPORT_RULE_FN static inline
#endif

/* c_0 - max(c_1, c_2); NaN if any centre is */
SUPPORT_RULE_FN double support_delta(double c0, double c1, double c2)
{
  if (c1 != c1) return c1;
  if (c2 != c2) return c2;
  return c0 - ((c1 > c2) ? c1 : c2);
}

/* replicate values l_k against the centres c_k: *sh = delta > (m1 - m2) + epsilon for the two largest m1 >= m2 of
 * cs_k = l_k - c_k; *lbp = l_0 > l_1 and l_0 > l_2 */
SUPPORT_RULE_FN void support_replicate(double c0, double c1, double c2, double delta, double epsilon, double l0,
                                       double l1, double l2, unsigned int * sh, unsigned int * lbp)
{
  const double a = l0 - c0, b = l1 - c1, c = l2 - c2;
  const double hi = (a > b) ? a : b, lo = (a > b) ? b : a;
  double m1, m2;
  if (c > hi)
  {
    m1 = c;
    m2 = hi;
  }
  else
  {
    m1 = hi;
    m2 = (c > lo) ? c : lo;
  }
  *sh = (a == a && b == b && c == c && delta > (m1 - m2) + epsilon) ? 1u : 0u;
  *lbp = (l0 > l1 && l0 > l2) ? 1u : 0u;
}

#endif
