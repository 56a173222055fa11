// hip_precond.h — the block-Jacobi object (hip_precond.hip) as the solvers that take one see it (hip_solver.hip, hip_solver_bi.hip, hip_solver_gm.hip).
#pragma once

#include "hip_solver_common.h"

struct tilespmv_block_jacobi {
    long long rows = 0;
    int bs = 0;                         // block size, 1 .. 16
    long long blocks = 0;               // ceil(rows / bs)
    long long plane = 0;                // elements from one plane to the next: rows, padded to a multiple of 256 bytes
    int np = 0;                         // workgroups of the apply = partial sums of its r.z form: solver_parts(rows)
    size_t bytes = 0;                   // of the one allocation: the bs planes, then the counter
    MAT_VAL_TYPE *inv = nullptr;        // plane j at inv + j * plane: plane_j[i] = (M^-1)[i][blockstart(i) + j]
    int *singular = nullptr;            // blocks the last update replaced by the identity
};

namespace tilespmv {
// z = M^-1 r on `st`; prz != NULL: also one partial sum of r.z per workgroup (bj->np of them).  The arguments are the caller's to check.
void block_jacobi_launch(const tilespmv_block_jacobi *bj, const val_t *r, val_t *z, double *prz, hipStream_t st);
}  // namespace tilespmv
