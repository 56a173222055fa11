// host_tile_create.cpp — CSR -> Tile_matrix on the host (the kept preprocessing API).
//
// Replaces Tile_create / convert_step1..4 of the reference (src/csr2tile.h:5-1020) with an
// O(nnz) many-core algorithm that produces the SAME bytes:
//   * the reference clears and scans tilen-sized scratch per tile-row (O(tilem*tilen),
//     src/csr2tile.h:26,67-71,89) and searches the tile list per nonzero (:406-418); here every
//     tile-row is handled with a stamp array (no clearing) and one stable bucket pass;
//   * all sizes are accumulated in 64 bits and checked against the int32 offsets that the
//     Tile_matrix API exposes (the reference overflows silently, e.g. :912);
//   * threads come from std::thread (no OpenMP runtime dependency).
// Shared with the device builder (hip_tile_create.hip): the selection rule (tile_select.h), the per-tile packer (tile_pack.h) and the table of member arrays
// (tile_fields.h).  Its own: how entries get into tile order (passes 1 and 2: stamp arrays per tile-row; the device sorts once).
// What each output field means: SURVEY.md Appendix A.  Selection rules: src/csr2tile.h:143-325.
#include <sys/time.h>
#include <cmath>

#include "host_util.h"
#include "tile_fields.h"
#include "tile_pack.h"
#include "tile_select.h"

namespace tilespmv {
namespace {

struct RowScratch {   // stamp / local: one int per column block, zeroed by calloc — a page nobody stamps is never touched (2^27 column blocks: 1 GB per thread otherwise; plain
    int *stamp, *local;   // calloc, not zalloc: with huge pages advised every stamped block of a hypersparse row would fault 2 MB in)
    std::vector<int> touched, cursor;
    explicit RowScratch(int tilen) : stamp((int *)calloc((size_t)std::max(tilen, 1), sizeof(int))), local((int *)calloc((size_t)std::max(tilen, 1), sizeof(int)))
    {
        if (!stamp || !local) { fprintf(stderr, "tilespmv: out of host memory (2 x %d ints of Tile_create scratch)\n", tilen); exit(2); }
    }
    ~RowScratch() { free(stamp); free(local); }
    RowScratch(const RowScratch &) = delete;
    RowScratch &operator=(const RowScratch &) = delete;
};

void pack_nibble_stream(const uint8_t *src, uint8_t *dst, int64_t n)
{
    parallel_chunks((n + 1) / 2, 1 << 16, [&](int64_t b, int64_t e, int) {
        for (int64_t i = b; i < e; i++) {
            uint8_t hi = src[2 * i], lo = (2 * i + 1 < n) ? src[2 * i + 1] : 0;
            dst[i] = (uint8_t)((hi << 4) + lo);
        }
    });
}

}  // namespace

// First-element-pivot partition sort of the reference (src/utils.h:103-137), restated so that
// rows holding duplicate column ids come out in the same (unstable) order.
void pivot_sort(int *key, val_t *val, int n)
{
    while (n > 1) {
        const int pivot = key[0];
        std::swap(key[0], key[n - 1]); std::swap(val[0], val[n - 1]);
        int lo = 0;
        for (int i = 0; i < n; i++)
            if (key[i] < pivot) { std::swap(key[i], key[lo]); std::swap(val[i], val[lo]); lo++; }
        std::swap(key[n - 1], key[lo]); std::swap(val[n - 1], val[lo]);
        pivot_sort(key, val, lo);
        key += lo + 1; val += lo + 1; n -= lo + 1;
    }
}

void tile_create_impl(Tile_matrix *T, int rowA, int colA, const MAT_PTR_TYPE *rowptr, const int *colidx,
                      const val_t *vals, unsigned flags)
{
    memset(T, 0, sizeof(*T));
    const bool tverbose = getenv("TILESPMV_CREATE_VERBOSE") != nullptr;   // per-phase milliseconds on stderr
    auto now_ms = [] { timeval t; gettimeofday(&t, NULL); return t.tv_sec * 1e3 + t.tv_usec * 1e-3; };
    double tprev = now_ms();
    auto lap = [&](const char *what) { if (!tverbose) return; const double now = now_ms(); fprintf(stderr, "tilespmv: Tile_create %s %.1f ms\n", what, now - tprev); tprev = now; };
    const bool allow_hyb = flags & TILESPMV_CREATE_HYB, cdna4 = flags & TILESPMV_CREATE_CDNA4;
    const int tilem = tiles_of(rowA), tilen = tiles_of(colA);
    T->tilem = tilem; T->tilen = tilen;
    T->tile_ptr = zalloc<int>((size_t)tilem + 1);
    const int nthreads = host_threads();
    std::vector<RowScratch *> scratch((size_t)nthreads, nullptr);
    auto get_scratch = [&](int tid) { if (!scratch[tid]) scratch[tid] = new RowScratch(tilen); return scratch[tid]; };

    // ---- pass 1: number of populated column blocks per tile-row
    parallel_chunks(tilem, 512, [&](int64_t b, int64_t e, int tid) {
        RowScratch *S = get_scratch(tid);
        for (int bi = (int)b; bi < (int)e; bi++) {
            const int r0 = bi * BS, r1 = r0 + tile_rowlen(bi, tilem, rowA);
            int n = 0;
            for (int j = rowptr[r0]; j < rowptr[r1]; j++) {
                int cb = colidx[j] >> 4;
                if (S->stamp[cb] != bi + 1) { S->stamp[cb] = bi + 1; n++; }   // (stamps start at 1: 0 is "never seen")
            }
            T->tile_ptr[bi] = n;
        }
    });
    exclusive_scan_checked(T->tile_ptr, (int64_t)tilem + 1, "tile count");
    const int tilenum = T->tile_ptr[tilem];
    T->tilenum = tilenum;
    if (!(flags & TILESPMV_CREATE_QUIET)) printf("\n  The number of tile = %i\n", tilenum);

    const int64_t nnz_used = rowptr[rowA];
    const size_t np1 = (size_t)tilenum + 1;
    TileExtents X; X.rowA = rowA;
    for_each_tile_field(*T, X, TF_LIST, zalloc_tile_field);
    uint8_t *cnt_row = zalloc<uint8_t>((size_t)tilenum * BS);
    int *ent = zalloc<int>((size_t)nnz_used);        // CSR position of each entry, tile order
    uint8_t *lrc = zalloc<uint8_t>((size_t)nnz_used);  // (local row << 4) | local col, tile order

    lap("pass 1 (tiles per tile-row)");
    // ---- pass 2: tile list (ascending column block), per-row counts and the tile-ordered gather.
    // Because tiles are numbered tile-row-major, the nonzeros of tile-row bi occupy the same
    // index range [rowptr[16bi], rowptr[16bi+16)) before and after the gather.
    parallel_chunks(tilem, 256, [&](int64_t b, int64_t e, int tid) {
        RowScratch *S = get_scratch(tid);
        for (int bi = (int)b; bi < (int)e; bi++) {
            const int r0 = bi * BS, r1 = r0 + tile_rowlen(bi, tilem, rowA);
            const int t0 = T->tile_ptr[bi], nt = T->tile_ptr[bi + 1] - t0;
            const int stampv = tilem + bi + 1;  // distinct from pass 1's stamps
            S->touched.clear();
            for (int j = rowptr[r0]; j < rowptr[r1]; j++) {
                int cb = colidx[j] >> 4;
                if (S->stamp[cb] != stampv) { S->stamp[cb] = stampv; S->touched.push_back(cb); }
            }
            if (!std::is_sorted(S->touched.begin(), S->touched.end())) std::sort(S->touched.begin(), S->touched.end());
            S->cursor.assign((size_t)nt + 1, 0);
            for (int k = 0; k < nt; k++) { S->local[S->touched[k]] = k; T->tile_columnidx[t0 + k] = S->touched[k]; }
            for (int r = r0; r < r1; r++)
                for (int j = rowptr[r]; j < rowptr[r + 1]; j++) {
                    int k = S->local[colidx[j] >> 4];
                    S->cursor[k + 1]++;
                    cnt_row[(size_t)(t0 + k) * BS + (r - r0)]++;
                }
            int run = rowptr[r0];
            for (int k = 0; k < nt; k++) { int c = S->cursor[k + 1]; T->tile_nnz[t0 + k] = run; S->cursor[k] = run; run += c; }
            for (int r = r0; r < r1; r++)
                for (int j = rowptr[r]; j < rowptr[r + 1]; j++) {
                    int k = S->local[colidx[j] >> 4];
                    int pos = S->cursor[k]++;
                    ent[pos] = j;
                    lrc[pos] = (uint8_t)(((r - r0) << 4) | (colidx[j] & 15));
                }
        }
    });
    T->tile_nnz[tilenum] = (int)nnz_used;
    for (auto *s : scratch) delete s;

    lap("pass 2 (tile columns, tile-ordered gather)");
    // ---- per-tile metadata + format selection
    for_each_tile_field(*T, X, TF_TILE, zalloc_tile_field);
    int *hyb_bytes = zalloc<int>(np1);   // HYB tiles: bytes of the tile in hybIdx (scanned into the tile's byte offset)
    std::atomic<int64_t> refused((int64_t)tilenum);   // the first tile that cannot be served (tile_select.h "repeated positions")

    parallel_chunks(tilem, 256, [&](int64_t b, int64_t e, int) {
        for (int bi = (int)b; bi < (int)e; bi++) {
            const int rowlen = tile_rowlen(bi, tilem, rowA);
            for (int t = T->tile_ptr[bi]; t < T->tile_ptr[bi + 1]; t++) {
                const int collen = tile_collen(T->tile_columnidx[t], tilen, colA);
                const int n = T->tile_nnz[t + 1] - T->tile_nnz[t];
                const uint8_t *cr = cnt_row + (size_t)t * BS, *lr = lrc + T->tile_nnz[t];
                const bool repeat = tile_has_repeat(n, [lr](int k) { return (int)lr[k]; });
                const Choice c = select_format(n, rowlen, collen, [cr](int r) { return (int)cr[r]; }, [lr](int k) { return (int)lr[k]; }, allow_hyb, cdna4, repeat);   // (tile_select.h: shared with the device builder)
                if (c.refused) { int64_t seen = refused.load(); while (t < seen && !refused.compare_exchange_weak(seen, (int64_t)t)) {} }
                T->Format[t] = (char)c.fmt;
                T->blknnz[t] = c.stored;
                T->blknnznnz[t] = (unsigned char)c.stored;
                T->tilewidth[t] = (char)c.width;
                T->dnsrowptr[t] = c.ndr; T->dnscolptr[t] = c.ndc;
                T->hyb_coocount[t] = c.hybcoo; T->new_coocount[t] = c.extracted;
                T->csrptr_offset[t] = c.csrptr;
                int *dst[7] = { T->csr_offset, T->coo_offset, T->ell_offset, T->hyb_offset, T->dns_offset,
                                T->dnsrow_offset, T->dnscol_offset };
                dst[c.fmt][t] = c.stored;
                if (c.fmt == TILESPMV_FMT_HYB) hyb_bytes[t] = (c.width * rowlen + 1) / 2 + c.hybcoo;   // ELL part in nibbles (rounded up to a byte), then one byte per remainder entry
            }
        }
    });
    lap("format selection");
    if (refused.load() < tilenum) {   // (void entry point: as for an int32 offset overflow)
        const int64_t t = refused.load();
        const int bi = (int)(std::upper_bound(T->tile_ptr, T->tile_ptr + tilem + 1, (int)t) - T->tile_ptr) - 1;
        fprintf(stderr, TILESPMV_TILE_REFUSAL_FMT, bi, T->tile_columnidx[t], T->tile_nnz[t + 1] - T->tile_nnz[t], TILE_REPEAT_MAX);
        exit(2);
    }
    int *scans[] = { T->csr_offset, T->csrptr_offset, T->coo_offset, T->ell_offset, T->hyb_offset, T->dns_offset,
                     T->dnsrow_offset, T->dnscol_offset, T->dnsrowptr, T->dnscolptr, T->hyb_coocount,
                     T->new_coocount, T->blknnz, hyb_bytes };
    static const char *names[] = { "csr_offset", "csrptr_offset", "coo_offset", "ell_offset", "hyb_offset", "dns_offset",
                                   "dnsrow_offset", "dnscol_offset", "dnsrowptr", "dnscolptr", "hyb_coocount",
                                   "new_coocount", "blknnz", "hybIdx bytes" };
    exclusive_scan_checked_multi(scans, names, (int)(sizeof(scans) / sizeof(*scans)), (int64_t)np1);
    T->csrsize = T->csr_offset[tilenum]; T->csrptrlen = T->csrptr_offset[tilenum];
    T->coosize = T->coo_offset[tilenum]; T->ellsize = T->ell_offset[tilenum];
    T->hybsize = T->hyb_offset[tilenum]; T->hybcoosize = T->hyb_coocount[tilenum]; T->hybellsize = T->hybsize - T->hybcoosize;   // (a HYB tile stores its ELL part + its remainder)
    T->dnssize = T->dns_offset[tilenum]; T->dnsrowsize = T->dnsrow_offset[tilenum];
    T->dnscolsize = T->dnscol_offset[tilenum]; T->coototal = T->new_coocount[tilenum];

    lap("scans");
    // ---- payload arrays
    X.n_dnsrow = T->dnsrowptr[tilenum]; X.n_dnscol = T->dnscolptr[tilenum]; X.hyb_idx_bytes = hyb_bytes[tilenum];
    for_each_tile_field(*T, X, TF_PAYLOAD | TF_EXTRACTED, zalloc_tile_field);   // (zeroed: hybIdx's nibbles are OR-ed in)

    uint8_t *csr_col = zalloc<uint8_t>(T->csrsize), *ell_col = zalloc<uint8_t>(T->ellsize);   // one byte per slot, packed into nibbles below
    int *x_row = zalloc<int>(T->coototal);  // extracted entries in tile order: local row | column | value
    int *x_col = zalloc<int>(T->coototal);
    val_t *x_val = zalloc<val_t>(T->coototal);

    lap("payload allocation");
    // ---- pass 3: pack every tile into its format's arrays (tile_pack.h) and, per
    // tile-row, turn its slice of the extracted list into CSR rows (src/csr2tile.h:899-960).
    const PackOut out = pack_out_of(*T, csr_col, ell_col);
    parallel_chunks(tilem, 128, [&](int64_t b, int64_t e, int) {
        for (int bi = (int)b; bi < (int)e; bi++) {
            const int rowlen = tile_rowlen(bi, tilem, rowA);
            for (int t = T->tile_ptr[bi]; t < T->tile_ptr[bi + 1]; t++) {
                const uint8_t *rc = lrc + T->tile_nnz[t]; const int *src = ent + T->tile_nnz[t];
                pack_tile(*T, t, rowlen, hyb_bytes[t], [rc](int k) { return (int)rc[k]; }, [src, vals](int k) { return vals[src[k]]; },
                          [&](int slot, int r, int k) { x_row[slot] = r; x_col[slot] = colidx[src[k]]; x_val[slot] = vals[src[k]]; }, out);
            }
            // extracted entries of this tile-row -> per-row counts (rows of other tile-rows never appear here)
            const int x0 = T->new_coocount[T->tile_ptr[bi]], x1 = T->new_coocount[T->tile_ptr[bi + 1]];
            for (int i = x0; i < x1; i++) T->deferredcoo_ptr[bi * BS + x_row[i]]++;
        }
    });
    { int *one[] = {T->deferredcoo_ptr}; static const char *nm[] = {"deferredcoo_ptr"}; exclusive_scan_checked_multi(one, nm, 1, (int64_t)rowA + 1); }
    parallel_chunks(tilem, 256, [&](int64_t b, int64_t e, int) {
        for (int bi = (int)b; bi < (int)e; bi++) {
            const int rowlen = tile_rowlen(bi, tilem, rowA);
            const int x0 = T->new_coocount[T->tile_ptr[bi]], x1 = T->new_coocount[T->tile_ptr[bi + 1]];
            if (x0 == x1) continue;
            int fill[BS] = {0};
            for (int i = x0; i < x1; i++) {  // stable scatter in order of appearance (:943-950)
                int r = x_row[i], p = T->deferredcoo_ptr[bi * BS + r] + fill[r]++;
                T->deferredcoo_colidx[p] = x_col[i]; T->deferredcoo_val[p] = x_val[i];
            }
            for (int r = 0; r < rowlen; r++) {
                int p = T->deferredcoo_ptr[bi * BS + r], len = T->deferredcoo_ptr[bi * BS + r + 1] - p;
                int *k = T->deferredcoo_colidx + p;
                bool increasing = true;  // tiles arrive in ascending column order: usually nothing to do
                for (int i = 1; i < len && increasing; i++) increasing = k[i - 1] < k[i];
                if (!increasing) pivot_sort(k, T->deferredcoo_val + p, len);
            }
        }
    });

    // ---- index compression (src/csr2tile.h:973-1008; nibble layout src/encode.h:29-50)
    pack_nibble_stream(csr_col, T->csr_compressedIdx, T->csrsize);
    pack_nibble_stream(ell_col, T->ell_compressedIdx, T->ellsize);
    lap("pass 3 (packing, extraction, nibble streams)");
    free_later({csr_col, ell_col, hyb_bytes, x_row, x_col, x_val, cnt_row, ent, lrc});   // (0.5 GB for config 4: given back on a detached thread)
    lap("frees");
}

}  // namespace tilespmv

extern "C" {

void Tile_create_ex(Tile_matrix *matrix, int rowA, int colA, MAT_PTR_TYPE nnzA, const MAT_PTR_TYPE *csrRowPtrA,
                    const int *csrColIdxA, const MAT_VAL_TYPE *csrValA, unsigned flags)
{
    (void)nnzA;  // like the reference, the row pointer decides how many nonzeros are used
    if (flags & TILESPMV_CREATE_TRANSPOSE) {   // the Tile_matrix of A^T: the host transposer (host_transpose.cpp), then the same builder
        const long long nnz = rowA >= 0 && csrRowPtrA ? (long long)csrRowPtrA[rowA] - csrRowPtrA[0] : 0;
        std::vector<MAT_PTR_TYPE> rpT((size_t)std::max(colA, 0) + 1);
        std::vector<int> ciT((size_t)std::max<long long>(nnz, 1));
        std::vector<MAT_VAL_TYPE> vT((size_t)std::max<long long>(nnz, 1));
        if (tilespmv::csr_transpose_host(rowA, colA, csrRowPtrA, csrColIdxA, csrValA, rpT.data(), ciT.data(), vT.data(), nullptr) != 0) {
            fprintf(stderr, "tilespmv: Tile_create_ex(TILESPMV_CREATE_TRANSPOSE): not a valid %d x %d CSR\n", rowA, colA);
            exit(2);
        }
        tilespmv::tile_create_impl(matrix, colA, rowA, rpT.data(), ciT.data(), vT.data(), flags & ~TILESPMV_CREATE_TRANSPOSE);
        return;
    }
    tilespmv::tile_create_impl(matrix, rowA, colA, csrRowPtrA, csrColIdxA, csrValA, flags);
}

void Tile_create(Tile_matrix *matrix, int rowA, int colA, MAT_PTR_TYPE nnzA, MAT_PTR_TYPE *csrRowPtrA,
                 int *csrColIdxA, MAT_VAL_TYPE *csrValA)
{
    Tile_create_ex(matrix, rowA, colA, nnzA, csrRowPtrA, csrColIdxA, csrValA, 0u);
}

void Tile_destroy(Tile_matrix *T)
{
    tilespmv::for_each_tile_field(*T, tilespmv::TileExtents(), tilespmv::TF_ALL, [](const tilespmv::TileField &f) { free(*f.ptr); });
    memset(T, 0, sizeof(*T));
}

}  // extern "C"
