// nni_quartet.hpp -- internal: what the calls over NNI candidates share (nni.hip, nni_support.hip; the code is in
// nni_quartet.hip): the quartet kernel's arguments, endings and launcher, and the preparation of a batch of edges --
// the check of an edge and its sides, the route, the kernel's descriptors, and the general route's u', v' and
// candidate edges.  One copy of the arithmetic and of the loop around it: a candidate's site term is the same bits
// whichever ending takes it.
#pragma once
#include "batched.hpp"

#include <vector>

// matrices of an edge in scratch: sides A..D, then the edge's own (the scoring calls), or the central branch of
// arrangements 0, 1, 2 (the support call)
enum { NNI_MATS = 5, NNI_SUPPORT_MATS = 7 };

// what k_nni_quartet does with a candidate's site terms
enum
{
  NNI_END_LNL = 0,    // weighted and summed per tile: partial
  NNI_END_TABLES = 1, // no site term: the candidate's sumtable row and combined scaler count (tables, counts)
  NNI_END_TERMS = 2   // stored per site, unweighted, the central matrix of arrangement k its own: terms
};

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

struct NniQuartetArgs
{
  const NniEdge * __restrict__ edges;     // [edges]
  const double * __restrict__ pm;         // [edges][NNI_MATS or NNI_SUPPORT_MATS][R][4][4]
  const double * __restrict__ sum_left;   // TABLES: the sumtable's two matrix sets [R][4][4]
  const double * __restrict__ sum_right;
  BatchModel m;
  double * __restrict__ partial;          // LNL: [edges][3][tiles]
  double * __restrict__ tables;           // TABLES: [edges][3][table_stride]
  unsigned int * __restrict__ counts;     // TABLES: [edges][3][count_stride] (scaled partitions)
  size_t table_stride, count_stride;
  unsigned int sites, tiles;
  int scaled;                             // the partition has scale buffers: u' and v' take the op's scaling rule
  unsigned int spitch;
  double * __restrict__ terms;            // TERMS: [edges][3][spitch], a row 0 from its last site up to spitch
};

// k_nni_quartet<R, end> for the context's 1 or 4 rate categories: grid (a.tiles, edges) on the context's stream
int pllhip_nni_quartet_launch(pllhip_ctx * c, const NniQuartetArgs & a, int end, unsigned int edges);

// ---- a batch of edges
// every edge's length and four sides (index, scaler index, length, CLV present): -1 and the error text, or 0
int pllhip_nni_check_edges(const pllhip_ctx * c, const char * what, const pllhip_nni_edge_t * E, unsigned int ne);

struct NniRoute
{
  bool scaled;  // the partition has scale buffers
  bool quartet; // the quartet kernel covers the partition and `route` does not rule it out
  int mode;     // SCALE_* of the general route's ops
};
// route: -1 the library's choice, 0 the general route, 1 the quartet kernel where it covers the partition
NniRoute pllhip_nni_route(const pllhip_ctx * c, int route);

// quartet route: the descriptors of E[0 .. en) into hd and, on the stream, to d_desc
int pllhip_nni_descriptors(pllhip_ctx * c, const pllhip_nni_edge_t * E, unsigned int en, std::vector<NniEdge> & hd,
                           NniEdge * d_desc);
// general route: u' and v' of the 3 en candidates of E[0 .. en) by the partition's own CLV kernels -- candidate i's u'
// into slot 2 i of d_clv (and of d_scal, or nullptr), its v' behind it; side sd's matrix is d_pm[mats * edge + sd]
int pllhip_nni_run_pairs(pllhip_ctx * c, const pllhip_nni_edge_t * E, unsigned int en, unsigned int mats,
                         const double * d_pm, double * d_clv, unsigned int * d_scal, int mode,
                         std::vector<BatchOp> & ops);
// general route: hge[i], i < cn, the edge (u', v') of candidate i with the central matrix
// d_pm[mats * (i / 3) + 4 + (per_arrangement ? i % 3 : 0)]; its sums or terms go to item i
void pllhip_nni_candidate_edges(const pllhip_ctx * c, BatchEdge * hge, unsigned int cn, unsigned int mats,
                                bool per_arrangement, const double * d_pm, const double * d_clv,
                                const unsigned int * d_scal);
