// tile_fields.h — the member arrays and the scalar members of Tile_matrix, listed ONCE: whoever allocates, frees, saves, loads, downloads or sizes a pool for a Tile_matrix
// walks this table (host_tile_create.cpp, host_matrix_io.cpp, hip_tile_create.hip, hip_plan.hip).  Element counts are those of SURVEY.md Appendix A; the Python mirror is
// tilespmv_amd/tile_matrix.py (field_lengths), and tests/test_host.py holds the two against each other.
#pragma once
#include "host_util.h"

namespace tilespmv {

constexpr int N_TILE_SCALARS = 14;   // in the order the cache file stores them (host_matrix_io.cpp)
inline int &tile_scalar(Tile_matrix &T, int i)
{
    int *s[N_TILE_SCALARS] = {&T.tilem, &T.tilen, &T.tilenum, &T.csrsize, &T.csrptrlen, &T.coosize, &T.ellsize, &T.hybsize,
                              &T.hybellsize, &T.hybcoosize, &T.dnssize, &T.dnsrowsize, &T.dnscolsize, &T.coototal};
    return *s[i];
}
inline void copy_tile_scalars(Tile_matrix &dst, const Tile_matrix &src)
{
    for (int i = 0; i < N_TILE_SCALARS; i++) tile_scalar(dst, i) = tile_scalar(const_cast<Tile_matrix &>(src), i);
}

// The groups follow the phases in which a builder learns the sizes: the tile list (tile_ptr needs tilem alone, and is what tilenum is computed from), the per-tile arrays
// (tilenum), the payload (the totals of the per-tile scans) and the extracted very-sparse matrix.
enum : unsigned { TF_LIST = 1u, TF_TILE = 2u, TF_PAYLOAD = 4u, TF_EXTRACTED = 8u, TF_ALL = 15u };

// what the scalar members do not say
struct TileExtents { long long rowA = 0, n_dnsrow = 0, n_dnscol = 0, hyb_idx_bytes = 0; };   // rows of the matrix; dnsrowptr[tilenum]; dnscolptr[tilenum]; bytes of hybIdx

// Bytes of hybIdx: every HYB tile has whole bytes of its own (tile_pack.h) — its ELL part in nibbles, rounded up to a byte, then one byte per remainder entry.  A builder has
// this total from its scan of the per-tile byte counts; whoever holds a finished matrix (cache file, download) recomputes it here from the per-tile arrays.  It equals
// (hybellsize + 1) / 2 + hybcoosize unless the partial last tile-row holds HYB tiles of odd width and odd height: each of those costs half a byte more.
inline long long hyb_idx_bytes(const Tile_matrix &T, long long rowA)
{
    long long bytes = 0;
    for (int bi = 0; bi < T.tilem; bi++) {
        const int rowlen = tile_rowlen(bi, T.tilem, (int)rowA);
        for (int t = T.tile_ptr[bi]; t < T.tile_ptr[bi + 1]; t++)
            if (T.Format[t] == TILESPMV_FMT_HYB) bytes += ((int)T.tilewidth[t] * rowlen + 1) / 2 + (T.hyb_coocount[t + 1] - T.hyb_coocount[t]);
    }
    return bytes;
}

// `count` elements are the array (what is saved, loaded and compared); an allocation or a download takes count + slack, a device allocation dev_slack more on top.
struct TileField { void **ptr; size_t elem; long long count, slack, dev_slack; unsigned group; };

// fn(const TileField &) for every member array of the chosen groups, in declaration order.  That order is the cache file's layout and checksum order: it must not move.
template <class Fn>
inline void for_each_tile_field(Tile_matrix &T, const TileExtents &X, unsigned groups, Fn fn)
{
    const long long n = T.tilenum, n1 = n + 1, hyb = (long long)T.hybellsize + T.hybcoosize;
    const size_t sv = sizeof(val_t);
#define TF(member, elem, count, slack, dev_slack, group) {(void **)&T.member, elem, count, slack, dev_slack, group}
    const TileField table[] = {
        TF(tile_ptr, 4, (long long)T.tilem + 1, 0, 0, TF_LIST), TF(tile_columnidx, 4, n, 0, 0, TF_LIST), TF(tile_nnz, 4, n1, 0, 0, TF_LIST),
        TF(Format, 1, n, 0, 0, TF_TILE), TF(blknnz, 4, n1, 0, 0, TF_TILE), TF(blknnznnz, 1, n1, 0, 0, TF_TILE),
        TF(dnsrowptr, 4, n1, 0, 0, TF_TILE), TF(dnscolptr, 4, n1, 0, 0, TF_TILE), TF(tilewidth, 1, n, 0, 0, TF_TILE),
        TF(csr_offset, 4, n1, 0, 0, TF_TILE), TF(csrptr_offset, 4, n1, 0, 0, TF_TILE), TF(coo_offset, 4, n1, 0, 0, TF_TILE),
        TF(ell_offset, 4, n1, 0, 0, TF_TILE), TF(hyb_offset, 4, n1, 0, 0, TF_TILE), TF(hyb_coocount, 4, n1, 0, 0, TF_TILE),
        TF(dns_offset, 4, n1, 0, 0, TF_TILE), TF(dnsrow_offset, 4, n1, 0, 0, TF_TILE), TF(dnscol_offset, 4, n1, 0, 0, TF_TILE),
        TF(new_coocount, 4, n1, 0, 0, TF_TILE),
        TF(Blockcsr_Val, sv, T.csrsize, 0, 0, TF_PAYLOAD), TF(Blockcsr_Ptr, 1, T.csrptrlen, 0, 0, TF_PAYLOAD),
        TF(csr_compressedIdx, 1, ((long long)T.csrsize + 1) / 2, 0, 0, TF_PAYLOAD),
        TF(Blockcoo_Val, sv, T.coosize, 0, 0, TF_PAYLOAD), TF(coo_compressed_Idx, 1, T.coosize, 0, 0, TF_PAYLOAD),
        TF(Blockell_Val, sv, T.ellsize, 0, 0, TF_PAYLOAD), TF(ell_compressedIdx, 1, ((long long)T.ellsize + 1) / 2, 0, 0, TF_PAYLOAD),
        TF(Blockhyb_Val, sv, hyb, 0, 1, TF_PAYLOAD),
        TF(hybIdx, 1, X.hyb_idx_bytes, (long long)T.tilem + 8, 0, TF_PAYLOAD),   // (the slack both builders have always given it; nothing relies on it)
        TF(Blockdense_Val, sv, T.dnssize, 0, 0, TF_PAYLOAD),
        TF(Blockdenserow_Val, sv, T.dnsrowsize, 0, 0, TF_PAYLOAD), TF(denserowid, 1, X.n_dnsrow, 0, 0, TF_PAYLOAD),
        TF(Blockdensecol_Val, sv, T.dnscolsize, 0, 0, TF_PAYLOAD), TF(densecolid, 1, X.n_dnscol, 0, 0, TF_PAYLOAD),
        TF(deferredcoo_val, sv, T.coototal, 0, 0, TF_EXTRACTED), TF(deferredcoo_colidx, 4, T.coototal, 0, 0, TF_EXTRACTED),
        TF(deferredcoo_ptr, 4, X.rowA + 1, 0, 0, TF_EXTRACTED),
    };
#undef TF
    for (const TileField &f : table) if (f.group & groups) fn(f);
}

// the same member of another Tile_matrix (f comes from a walk over `of`)
inline void *same_tile_field(const Tile_matrix &other, const Tile_matrix &of, const TileField &f)
{
    return *(void *const *)((const char *)&other + ((const char *)f.ptr - (const char *)&of));
}

// a zeroed host array for f, slack included; a member that is allocated already (tile_ptr, by the time the tile list is) is left alone
inline void zalloc_tile_field(const TileField &f)
{
    if (!*f.ptr) *f.ptr = zalloc<char>((size_t)std::max<long long>(f.count + f.slack, 1) * f.elem);
}

}  // namespace tilespmv
