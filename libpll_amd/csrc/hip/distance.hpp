// distance.hpp -- internal: the body of pllhip_pairwise_distances (distance.hip) for callers inside the device layer.
#pragma once
#include "batched.hpp"

// pllhip_pairwise_distances with one more route: d_matrix != nullptr (all-pairs mode only, h_col_tips == nullptr)
// leaves the distances on the device as the square matrix [row_count][row_count] the caller zeroed -- a chunk's pairs
// are written to [x][y] and [y][x] by a kernel on the context's stream, the diagonal stays 0 -- from the same kernels
// on the same tables, so with the bits the host outputs get.  h_dist may then be nullptr, and nothing is copied to the
// host unless an output asks for it.  The stream has been waited for when this returns.
int pllhip_distances_run(pllhip_ctx * c, const char * what, const unsigned int * row_tips, unsigned int row_count,
                         const unsigned int * col_tips, unsigned int col_count, const unsigned int * params,
                         double min_length, double max_length, double tolerance, unsigned int max_iters, size_t budget,
                         const double * h_start, double * h_dist, double * h_lnl, unsigned int * h_evals,
                         int * h_status, unsigned int * h_counts, double * d_matrix);
