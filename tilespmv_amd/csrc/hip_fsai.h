// hip_fsai.h — the FSAI object (hip_fsai.hip) as the solver that takes one sees it (hip_solver.hip).
#pragma once

#include "hip_solver_common.h"

struct tilespmv_fsai {
    long long rows = 0;
    long long gnnz = 0;                 // nonzeros of G
    int longest = 0;                    // the longest row of G, 1 .. TILESPMV_FSAI_MAX_ROW
    int truncated = 0;                  // rows of A with more than TILESPMV_FSAI_MAX_ROW entries at or left of the diagonal
    int np = 0;                         // partial sums of the r.z form of the apply: solver_parts(rows)
    size_t bytes = 0;                   // of the object's own allocations (the plans' are added by info)
    void *pattern = nullptr;            // one allocation: gp, first, the counters
    void *values = nullptr;             // one allocation: gci, gval, t
    int *gp = nullptr;                  // row pointer of G, rows + 1
    int *first = nullptr;               // first[i]: the position in A's arrays of the first pattern entry of row i (the diagonal is at first[i] + gp[i + 1] - gp[i] - 1)
    int *counters = nullptr;            // FSAI_COUNTER_*
    int *gci = nullptr;                 // column indices of G
    MAT_VAL_TYPE *gval = nullptr;       // values of G: what both plans' value maps index
    MAT_VAL_TYPE *t = nullptr;          // t = G r
    tilespmv_plan *G = nullptr, *GT = nullptr;
};

namespace tilespmv {
// z = G^T (G r) on `st`; prz != NULL: also f->np partial sums of r.z (double).  The arguments are the caller's to check.  Returns a hipError_t value.
int fsai_launch(tilespmv_fsai *f, const val_t *r, val_t *z, double *prz, hipStream_t st);
}  // namespace tilespmv
