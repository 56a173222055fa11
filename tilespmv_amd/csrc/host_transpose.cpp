// host_transpose.cpp — A^T of a CSR on the host (tilespmv_csr_transpose), and Tile_create_ex's TILESPMV_CREATE_TRANSPOSE path.
// A stable counting sort by column: the rows are cut into P chunks of about equal nonzeros, every chunk counts its columns, the counts are turned into per-chunk starting
// offsets column by column (chunk order = CSR order, so equal columns keep their order), and every chunk places its own entries.  P is bounded so that the P x colA counts stay
// within a few bytes per nonzero.  No reference counterpart: the reference multiplies A only (src/main.cu).
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <vector>

#include "host_util.h"

using namespace tilespmv;

namespace tilespmv {

// the transpose into caller-provided arrays; 0 or -1 (bad argument)
int csr_transpose_host(int rowA, int colA, const MAT_PTR_TYPE *rp, const int *ci, const val_t *v, MAT_PTR_TYPE *rpT, int *ciT, val_t *vT, int *srcT)
{
    if (rowA < 0 || colA < 0 || !rp || !rpT) return -1;
    const long long base = rp[0], nnz = (long long)rp[rowA] - base;
    if (base < 0 || nnz < 0) return -1;
    if (nnz > 0 && (!ci || !ciT || (vT && !v))) return -1;
    long long P = std::min<long long>(host_threads(), std::max<long long>(1, nnz >> 16));
    while (P > 1 && P * (long long)colA > 4 * nnz + (1 << 20)) P--;
    // chunk p holds rows [cut[p], cut[p + 1]): the first row whose entries start at or after p * nnz / P
    std::vector<int> cut((size_t)P + 1, rowA);
    cut[0] = 0;
    for (long long p = 1; p < P; p++) {
        const long long at = base + p * nnz / P;
        cut[(size_t)p] = (int)(std::lower_bound(rp, rp + rowA + 1, (MAT_PTR_TYPE)at) - rp);
        cut[(size_t)p] = std::min(std::max(cut[(size_t)p], cut[(size_t)p - 1]), rowA);
    }
    std::vector<MAT_PTR_TYPE> cnt((size_t)P * (size_t)colA, 0);
    std::atomic<int> bad(0);
    parallel_chunks(P, 1, [&](int64_t pb, int64_t pe, int) {
        for (int64_t p = pb; p < pe; p++) {
            MAT_PTR_TYPE *c = cnt.data() + (size_t)p * (size_t)colA;
            for (int r = cut[(size_t)p]; r < cut[(size_t)p + 1]; r++) {
                if (rp[r + 1] < rp[r]) { bad = 1; return; }
                for (MAT_PTR_TYPE j = rp[r]; j < rp[r + 1]; j++) {
                    const int col = ci[j];
                    if (col < 0 || col >= colA) { bad = 1; return; }
                    c[col]++;
                }
            }
        }
    });
    if (bad) return -1;
    // per column: the chunks' counts become their offsets inside the column; the column totals are scanned into rpT, then added
    parallel_chunks(colA, 1 << 16, [&](int64_t b, int64_t e, int) {
        for (int64_t col = b; col < e; col++) {
            MAT_PTR_TYPE s = 0;
            for (long long p = 0; p < P; p++) { MAT_PTR_TYPE &c = cnt[(size_t)p * (size_t)colA + (size_t)col]; const MAT_PTR_TYPE t = c; c = s; s += t; }
            rpT[col + 1] = s;
        }
    });
    rpT[0] = 0;
    for (int col = 0; col < colA; col++) rpT[col + 1] += rpT[col];
    parallel_chunks(P, 1, [&](int64_t pb, int64_t pe, int) {
        for (int64_t p = pb; p < pe; p++) {
            MAT_PTR_TYPE *c = cnt.data() + (size_t)p * (size_t)colA;
            for (int col = 0; col < colA; col++) c[col] += rpT[col];
            for (int r = cut[(size_t)p]; r < cut[(size_t)p + 1]; r++)
                for (MAT_PTR_TYPE j = rp[r]; j < rp[r + 1]; j++) {
                    const MAT_PTR_TYPE k = c[ci[j]]++;
                    ciT[k] = r;
                    if (vT) vT[k] = v[j];
                    if (srcT) srcT[k] = j;
                }
        }
    });
    return 0;
}

}  // namespace tilespmv

extern "C" int tilespmv_csr_transpose(int rowA, int colA, const MAT_PTR_TYPE *csrRowPtr, const int *csrColIdx, const MAT_VAL_TYPE *csrVal, MAT_PTR_TYPE *rowPtrT, int *colIdxT,
                                      MAT_VAL_TYPE *valT, int *srcT)
{
    return tilespmv::csr_transpose_host(rowA, colA, csrRowPtr, csrColIdx, csrVal, rowPtrT, colIdxT, valT, srcT);
}
