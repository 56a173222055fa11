/*
 * tilespmv.h — C ABI of the MI355X-native TileSpMV engine (libtilespmv_f64.so / libtilespmv_f32.so).
 *
 * Drop-in boundary for the y = A*x hot path of SuperScientificSoftwareLaboratory/TileSpMV.
 * The reference has no FFI layer: "the API" is the set of C functions its driver calls
 * (reference src/main.cu:63,87,142,165) plus the CLI.  Every entry point below names the
 * reference interface it replaces.  Plain pointers and sizes only; no C++/torch types.
 *
 * Value type is a build-time choice exactly like the reference (src/common.h:12-14,
 * src/Makefile:5,23):  libtilespmv_f64.so  <=>  -D MAT_VAL_TYPE=double
 *                      libtilespmv_f32.so  <=>  -D MAT_VAL_TYPE=float
 * Both libraries export the same symbol names.
 */
#ifndef TILESPMV_H_
#define TILESPMV_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef MAT_VAL_TYPE
#define MAT_VAL_TYPE double /* reference src/common.h:12-14 */
#endif
#ifndef MAT_PTR_TYPE
#define MAT_PTR_TYPE int /* reference src/common.h:25-27 */
#endif

/* Compile-time constants the tile format is defined by (reference src/common.h:37-63). */
#define TILESPMV_BLOCK_SIZE 16       /* BLOCK_SIZE */
#define TILESPMV_COO_NNZ_TH 12       /* COO_NNZ_TH */
#define TILESPMV_PREFETCH_SMEM_TH 4  /* PREFETCH_SMEM_TH: tiles per row-block chunk */

/* Per-tile format tags stored in Tile_matrix.Format (reference src/csr2tile.h:154-319). */
enum {
    TILESPMV_FMT_CSR = 0,
    TILESPMV_FMT_COO = 1,
    TILESPMV_FMT_ELL = 2,
    TILESPMV_FMT_HYB = 3,
    TILESPMV_FMT_DNS = 4,
    TILESPMV_FMT_DNSROW = 5,
    TILESPMV_FMT_DNSCOL = 6
};

/*
 * Tile_matrix — field names, order and types are those of reference src/format.h:3-56
 * (tests and callers read the fields by name).  Semantics after Tile_create are listed in
 * arrays of length tilenum+1 are exclusive prefixes.
 */
typedef struct {
    int tilem;
    int tilen;
    int tilenum;
    MAT_PTR_TYPE *tile_ptr;
    int *tile_columnidx;
    int *tile_nnz;
    char *Format;
    int *blknnz;
    unsigned char *blknnznnz;
    int *dnsrowptr;
    int *dnscolptr;
    char *tilewidth;
    int *csr_offset;
    int *csrptr_offset;
    int *coo_offset;
    int *ell_offset;
    int *hyb_offset;
    int *hyb_coocount;
    int *dns_offset;
    int *dnsrow_offset;
    int *dnscol_offset;
    int *new_coocount;
    MAT_VAL_TYPE *Blockcsr_Val;
    unsigned char *Blockcsr_Ptr;
    unsigned char *csr_compressedIdx;
    int csrsize;
    int csrptrlen;
    MAT_VAL_TYPE *Blockcoo_Val;
    unsigned char *coo_compressed_Idx;
    int coosize;
    MAT_VAL_TYPE *Blockell_Val;
    unsigned char *ell_compressedIdx;
    int ellsize;
    MAT_VAL_TYPE *Blockhyb_Val;
    unsigned char *hybIdx;
    int hybsize;
    int hybellsize;
    int hybcoosize;
    MAT_VAL_TYPE *Blockdense_Val;
    int dnssize;
    MAT_VAL_TYPE *Blockdenserow_Val;
    char *denserowid;
    int dnsrowsize;
    MAT_VAL_TYPE *Blockdensecol_Val;
    char *densecolid;
    int dnscolsize;
    int coototal;
    MAT_VAL_TYPE *deferredcoo_val;
    int *deferredcoo_colidx;
    MAT_PTR_TYPE *deferredcoo_ptr;
} Tile_matrix;

/* ------------------------------------------------------------------------------------------
 * Host preprocessing (kept API).
 * ---------------------------------------------------------------------------------------- */

/* Replaces reference src/csr2tile.h:629-635.  Caller owns the struct, callee mallocs every
 * member array; inputs are borrowed and not modified.  Prints "\n  The number of tile = %i\n"
 * (reference src/csr2tile.h:661).  Output is byte-identical to the reference's. */
void Tile_create(Tile_matrix *matrix, int rowA, int colA, MAT_PTR_TYPE nnzA,
                 MAT_PTR_TYPE *csrRowPtrA, int *csrColIdxA, MAT_VAL_TYPE *csrValA);

/* Same as Tile_create with option bits.  TILESPMV_CREATE_HYB enables the HYB selection rule
 * that is commented out in the shipped reference (src/csr2tile.h:308-316);
 * TILESPMV_CREATE_QUIET suppresses the stdout line. */
#define TILESPMV_CREATE_HYB 1u
#define TILESPMV_CREATE_QUIET 2u
/* TILESPMV_CREATE_CDNA4 (opt-in; default off = the reference's selection, byte-identical Tile_matrix): per-tile format chosen by
 * the bytes THIS engine moves for it (16-value units + entries) instead of the reference's thresholds (dense at 75 % fill, COO up
 * to 12 entries, ELL at row-length variation <= 0.2: src/csr2tile.h:150,159,267-270; COO_NNZ_TH src/common.h:45-47).  The result is
 * still a valid Tile_matrix for tilespmv_cpu and every plan; profiles/r03_selection_cdna4.txt has what it changes. */
#define TILESPMV_CREATE_CDNA4 4u
/* TILESPMV_CREATE_VALUE_MAP (opt-in; tilespmv_plan_create_from_csr / _from_device_csr only, Tile_create_device ignores it): the plan also keeps a device-resident VALUE MAP — for every
 * value slot of its streams the position of the source nonzero in the CSR arrays — so that tilespmv_plan_update_values (below) can rewrite every value the plan holds from a new value
 * array of the same pattern.  See tilespmv_plan_update_values for the contract. */
#define TILESPMV_CREATE_VALUE_MAP 8u
/* TILESPMV_CREATE_TRANSPOSE (opt-in; Tile_create_ex, Tile_create_device, tilespmv_plan_create_from_csr / _from_device_csr): build the tiled matrix or plan of A^T instead of A.
 * rowA, colA, nnzA and the CSR arrays still describe A; the result is that of tilespmv_csr_transpose's output (below) — a colA x rowA matrix — and a plan of it computes
 * y[0 .. colA) = A^T x with x of rowA elements.  tilerow_begin / tilerow_end count tile-rows of A^T (column blocks of A), and the refusals (-4) apply to the transposed shape.
 * The transposition runs on the device for the device entry points (tilespmv_csr_transpose_device) and on the host for Tile_create_ex; either way the result is byte for byte
 * what the unflagged entry point builds from the transposed CSR.  With TILESPMV_CREATE_VALUE_MAP as well, the plan's value map names positions of A's value array:
 * tilespmv_plan_update_values(plan_of_AT, d_csrVal_of_A, stream) refreshes it from the same array that refreshes the plan of A.  Without the flag nothing changes. */
#define TILESPMV_CREATE_TRANSPOSE 16u
void Tile_create_ex(Tile_matrix *matrix, int rowA, int colA, MAT_PTR_TYPE nnzA,
                    const MAT_PTR_TYPE *csrRowPtrA, const int *csrColIdxA,
                    const MAT_VAL_TYPE *csrValA, unsigned flags);

/* Replaces reference src/format.h:58-94: frees the member arrays (all of them, including the
 * four the reference leaks), not the struct. */
void Tile_destroy(Tile_matrix *matrix);

/* Replaces reference src/tilespmv_cpu.h:3-18: builds the row-block schedule
 * (ptroffset1/2[tilenum] caller-allocated; rowblkblock and the three chunk arrays are
 * malloc'd here and owned by the caller), computes y = A*x serially on the host in tile
 * order, compares with y_golden (exact) and prints " Run CPU TileSpMV, errcount = %i\n".
 * Host-side schedule builder + host check only — the GPU path never calls it. */
void tilespmv_cpu(Tile_matrix *matrix, int *ptroffset1, int *ptroffset2, int *rowblkblock,
                  unsigned int **blkcoostylerowidx, int **blkcoostylerowidx_colstart,
                  int **blkcoostylerowidx_colstop, int rowA, int colA, MAT_PTR_TYPE nnzA,
                  MAT_PTR_TYPE *csrRowPtrA, int *csrColIdxA, MAT_VAL_TYPE *csrValA,
                  MAT_VAL_TYPE *x, MAT_VAL_TYPE *y, MAT_VAL_TYPE *y_golden);

/* Replaces reference src/mmio_highlevel.h:593-759.  Returns 0, -1 (open), -2 (banner),
 * -4 (size line).  Entries land in file order; symmetric/hermitian files are mirrored,
 * skew-symmetric are not; pattern -> 1.0; complex keeps the real part. */
int mmio_allinone(int *m, int *n, MAT_PTR_TYPE *nnz, int *isSymmetric, MAT_PTR_TYPE **csrRowPtr,
                  int **csrColIdx, MAT_VAL_TYPE **csrVal, char *filename);

/* Binary cache of a created Tile_matrix (new: the reference never serialises it; a multi-GB
 * .mtx is otherwise re-parsed and re-tiled on every run).  save: 0 on success, -1 cannot open,
 * -3 short write.  load: callee mallocs every member (free with Tile_destroy); 0 on success,
 * -1 cannot open, -2 not a cache file (or another format version), -3 read error, -5 written by the other value
 * type, -6 corrupt / truncated / stale: the header's counts, the file length, the payload checksum (FNV-1a-64) and the
 * prefix arrays are all checked before a matrix is handed back.  A cache does not record the Tile_create flags: keep
 * caches built with TILESPMV_CREATE_HYB apart from the others (the Format array tells them apart after loading). */
int tilespmv_matrix_save(const Tile_matrix *matrix, int rowA, int colA, MAT_PTR_TYPE nnzA, const char *path);
int tilespmv_matrix_load(Tile_matrix *matrix, int *rowA, int *colA, MAT_PTR_TYPE *nnzA, const char *path);

/* Parse once (new): binary cache of what mmio_allinone returns.  The reference re-tokenises the text on
 * every run (src/mmio_highlevel.h:648-682; nlpkkt160 is ~4 GB of it).  save: 0, -1 cannot open, -3 short write (the partial
 * file is removed).  load: arrays are malloc'd like mmio_allinone's (caller frees); 0, -1 cannot open, -2 not a CSR cache,
 * -3 read error, -5 other value type, -6 corrupt (length, FNV-1a-64 checksum, row pointer, column range all checked), -7
 * stale: `source_mtx` (may be NULL = do not check) no longer has the size and modification time recorded at save time. */
int tilespmv_csr_save(const char *path, int m, int n, MAT_PTR_TYPE nnz, int isSymmetric,
                      const MAT_PTR_TYPE *csrRowPtr, const int *csrColIdx, const MAT_VAL_TYPE *csrVal,
                      const char *source_mtx);
int tilespmv_csr_load(const char *path, int *m, int *n, MAT_PTR_TYPE *nnz, int *isSymmetric,
                      MAT_PTR_TYPE **csrRowPtr, int **csrColIdx, MAT_VAL_TYPE **csrVal,
                      const char *source_mtx);
/* mmio_allinone with the cache beside it: reads `cache_path` when it is fresh for `filename`, else parses the text and
 * (re)writes the cache.  *from_cache (may be NULL): 1 read from the cache, 0 parsed and saved, -1 parsed, cache not
 * writable.  Return codes of mmio_allinone.  The CLI's `--cache[=prefix]` and bench.py's `--cache DIR` go through this. */
int mmio_allinone_cached(int *m, int *n, MAT_PTR_TYPE *nnz, int *isSymmetric, MAT_PTR_TYPE **csrRowPtr,
                         int **csrColIdx, MAT_VAL_TYPE **csrVal, char *filename, const char *cache_path,
                         int *from_cache);
/* Writes a general coordinate Matrix Market file in CSR order (the reference's counterpart: mm_write_mtx_crd,
 * src/mmio.h:605-645), formatted by all host threads; csrVal == NULL writes a pattern file.  0, -1 cannot open, -3 short
 * write. */
int tilespmv_mtx_write(const char *path, int m, int n, MAT_PTR_TYPE nnz, const MAT_PTR_TYPE *csrRowPtr,
                       const int *csrColIdx, const MAT_VAL_TYPE *csrVal);

/* ------------------------------------------------------------------------------------------
 * GPU hot path.
 * ---------------------------------------------------------------------------------------- */

/* Replaces call_tilespmv_cuda, reference src/tilespmv_cuda.h:794-809 (same argument list and
 * meaning; all pointers are HOST pointers; alpha is accepted and ignored like the reference).
 * Uploads the tiled matrix to the current HIP device, runs WARMUP_NUM warm-up and
 * BENCH_REPEAT timed SpMVs (env TILESPMV_WARMUP / TILESPMV_BENCH_REPEAT override 200 / 1000),
 * prints "  CUDA SpMV runtime %4.2f ms, %4.2f GFlops\n\n" (kept verbatim for log parsers,
 * reference :1139) plus one added "  HIP ..." line, appends "file,rowA,colA,nnzA,ms,gflops"
 * to ./results.csv (reference :1142-1147) and copies y back.  Aborts with a message and a
 * non-zero exit status on any HIP error (the reference checks nothing). */
void call_tilespmv_hip(char *filename, Tile_matrix *matrix, int *ptroffset1, int *ptroffset2,
                       int rowblkblock, unsigned int *blkcoostylerowidx,
                       int *blkcoostylerowidx_colstart, int *blkcoostylerowidx_colstop, int rowA,
                       int colA, MAT_PTR_TYPE nnzA, MAT_PTR_TYPE *csrRowPtrA, int *csrColIdxA,
                       MAT_VAL_TYPE *csrValA, MAT_VAL_TYPE alpha, MAT_VAL_TYPE *x,
                       MAT_VAL_TYPE *y, MAT_VAL_TYPE *y_golden);

/* Multi-device form of the same driver (new: the reference is single-GPU, src/main.cu:74; SURVEY.md
 * S8(b) "New").  Same 18 arguments, then the devices to use and what to do with y afterwards.
 * The matrix is cut into `ngpus` nnz-balanced blocks of whole tile-rows (tilespmv_partition_tilerows),
 * one resident plan per device, x replicated; the SpMV needs no exchange.  y_combine_mode:
 *   TILESPMV_Y_SHARDED   every device keeps its own rows (the timed figure of the other modes too);
 *   TILESPMV_Y_ALLGATHER every device receives the other shards' rows by peer copies (xGMI);
 *   TILESPMV_Y_ALLREDUCE ncclAllReduce(sum) of full-length vectors that are zero outside the owner's
 *                        rows (bit-identical to the gather); librccl is dlopen'ed for this mode only.
 * Prints the reference's runtime line for the sharded SpMV plus one "  HIP ..." line that also
 * carries the SpMV+combine time, appends results.csv, returns y on the host (in the combine modes
 * taken from the last device's full-length copy).  A device id may be repeated (several shards on
 * one device) except in all-reduce mode.  Returns 0, or — after a message on stderr and after releasing every device resource it
 * had created — a non-zero status on any error (bad arguments, no such device, HIP / RCCL failure): it never exits the process. */
#define TILESPMV_Y_SHARDED 0
#define TILESPMV_Y_ALLGATHER 1
#define TILESPMV_Y_ALLREDUCE 2
int call_tilespmv_hip_multi(char *filename, Tile_matrix *matrix, int *ptroffset1, int *ptroffset2,
                             int rowblkblock, unsigned int *blkcoostylerowidx,
                             int *blkcoostylerowidx_colstart, int *blkcoostylerowidx_colstop,
                             int rowA, int colA, MAT_PTR_TYPE nnzA, MAT_PTR_TYPE *csrRowPtrA,
                             int *csrColIdxA, MAT_VAL_TYPE *csrValA, MAT_VAL_TYPE alpha,
                             MAT_VAL_TYPE *x, MAT_VAL_TYPE *y, MAT_VAL_TYPE *y_golden, int ngpus,
                             const int *device_ids, int y_combine_mode);

/*
 * Resident-plan API (new; what call_tilespmv_hip is built from).  A plan owns the device
 * copy of one Tile_matrix (or of one contiguous block of its tile-rows: the multi-GPU shard),
 * re-laid-out for CDNA4.  x / y are DEVICE pointers; stream is a hipStream_t passed as void*.
 */
typedef struct tilespmv_plan tilespmv_plan;

/* How COO tiles (and HYB remainders) are executed — reference has both paths
 * (in-kernel deferred COO: src/tilespmv_cuda.h:462-488; extracted CSR + CSR5: :1011-1029,:1080). */
#define TILESPMV_COO_AUTO 0      /* in-tile with the unit-stream kernel (the fallback is a second launch and never wins there);
                                    by modelled bytes with TILESPMV_KERNEL_DIRECT */
#define TILESPMV_COO_IN_TILE 1   /* COO entries inside the fused launch */
#define TILESPMV_COO_FALLBACK 2  /* very-sparse fallback kernel over the extracted matrix (y += A_coo x), as the reference's CSR5 call */

/* Dense-tile arithmetic. */
#define TILESPMV_DENSE_AUTO 0
#define TILESPMV_DENSE_MFMA 1  /* v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32 */
#define TILESPMV_DENSE_VALU 2

/* Fused-kernel generation. */
#define TILESPMV_KERNEL_AUTO 0
#define TILESPMV_KERNEL_DIRECT 1  /* strip-per-16-lanes, one tile at a time (first generation) */
#define TILESPMV_KERNEL_STREAM 2  /* flat, index-addressed unit stream (second generation; default) */

/* Plan options.  VERSIONED: set `size = sizeof(tilespmv_plan_options)` (tilespmv_plan_options_init does, and sets every
 * knob to TILESPMV_KNOB_DEFAULT); a library built against a longer struct gives the fields beyond `size` their defaults,
 * one built against a shorter struct ignores the tail.  opts == NULL = all defaults.
 * The tuning knobs replace what used to travel through the process environment: an unset knob (TILESPMV_KNOB_DEFAULT)
 * takes the value of the environment variable named beside it if that is set — read with getenv at plan creation,
 * never written: the library does not call setenv / unsetenv — and the built-in default otherwise.  Two host threads may
 * create differently tuned plans at the same time (scripts/tsan_host.sh). */
#define TILESPMV_KNOB_DEFAULT (-1)
typedef struct {
    unsigned size;      /* sizeof(tilespmv_plan_options) in the caller's build */
    int coo_mode;       /* TILESPMV_COO_*    (0 = AUTO; env TILESPMV_COO_MODE)   */
    int dense_mode;     /* TILESPMV_DENSE_*  (0 = AUTO; env TILESPMV_DENSE_MODE) */
    int kernel;         /* TILESPMV_KERNEL_* (0 = AUTO; env TILESPMV_KERNEL)     */
    int tilerow_begin;  /* shard: first tile-row (0 for the whole matrix) */
    int tilerow_end;    /* shard: one past the last tile-row (<=0 means tilem) */
    int autotune;       /* != 0 (or env TILESPMV_AUTOTUNE=1): decide the AUTO modes, entry mode, strip size, XCD map and stream cache policy by timing candidates
                           (one candidate plan is resident beside the best one so far: peak device memory = two plans + x + y) */
    /* ---- knobs (TILESPMV_KNOB_DEFAULT = unset) */
    int entry_mode;     /* COO entry lists per 16-lane strip (0), per wavefront (1), per workgroup (2)      TILESPMV_WAVE_COO */
    int entry_ordered;  /* workgroup entry mode: 1 = wavefronts add in turn (bit-reproducible sums), 0 = not  TILESPMV_COO_ORDERED */
    int strip_cost;     /* strip size target in cost units (<= 0: chosen from the shard)                     TILESPMV_STRIP_COST */
    int split_above;    /* tile-rows above this cost are cut into pieces                                     TILESPMV_SPLIT_ABOVE */
    int split_cap;      /* ... and the cap of that threshold in the wavefront / workgroup entry modes        TILESPMV_SPLIT_CAP */
    int xcd_remap;      /* workgroup -> XCD map: 0 round-robin, 2 windows of 8 x xcd_chunk workgroups         TILESPMV_XCD_REMAP */
    int xcd_chunk;      /*                                                                                   TILESPMV_XCD_CHUNK */
    int csr_split;      /* what the device executes for CSR-format tiles: 0 whole tiles in their own pass (first-generation routine, y +=); 1 ELL-style split — the first w
                           entries of every row as w zero-padded 16-value units, the rest as list entries; 2 POOLED units (round 5) — the nonzeros of a tile-row's CSR tiles, COO
                           tiles and HYB remainders pooled in column-major order and cut into units of up to 16 nonzeros inside a 16-column window of x (value + column-offset nibble +
                           row nibble per slot, products scattered into the strip's LDS rows): no padding beyond the last unit of a run of columns, about s_v + 1.3 bytes per nonzero
                           on block-structured / FEM-like matrices; unset: 1 or 2, whichever puts at least 5 % fewer bytes into the streams (2 on shards whose nonzeros sit
                           mostly in ragged CSR tiles, 1 on stencil-like shards whose units share a handful of column patterns); 3 WIDE pooled units — the same pooling with
                           windows of 256 columns (a byte of column offset per slot: s_v + 1.75 bytes per nonzero), taken by the builder where 16-column windows leave >= 4 % of the
                           nonzeros on the entry lists AND a unit's sixteen gathers still touch at most 3.5 lines of x on average (window-shuffled meshes)   TILESPMV_CSR_SPLIT */
    int fix_inline;     /* split tile-rows summed inside the unit kernel (1) or by k_fixup_split (0)         TILESPMV_FIX_INLINE */
    int coo_cost;       /* cost units per COO entry in the strip cutter                                      TILESPMV_COO_COST */
    int coo_heavy_min;  /* entry mode 0: strips with more entries run their list before the unit pipeline    TILESPMV_COO_HEAVY_MIN */
    int coo_piece;      /* entries per piece of a split tile-row                                             TILESPMV_COO_PIECE */
    int strip_even;     /* strips end on multiples of this many units                                        TILESPMV_STRIP_EVEN */
    int wg_strips;      /* workgroup entry mode: 16 (256-thread workgroups) or 32 (512 threads) strips per workgroup  TILESPMV_WG_STRIPS */
    int x_window;       /* stencil-like shards: -1 / unset = brick task order on large 3-D shards, 0 = off, 1 / 2 = brick order wherever grid strides are
                           found.  (Rounds 3-5: 1 also staged the workgroup's x segments in LDS; measured 25 % slower, retired in round 6 together with the
                           slab-paced entry phase and its five `pace*` knobs)                                                 TILESPMV_X_WINDOW */
    int x_stride1;      /* ... tile-rows per grid line (0 / unset: detected from the shard)                  TILESPMV_X_STRIDE1 */
    int x_stride2;      /* ... tile-rows per grid plane (0 / unset: detected; none for 2-D problems)         TILESPMV_X_STRIDE2 */
    int mv_native;      /* tilespmv_plan_spmm: 0 one vector at a time, 1 multi-vector kernel with per-strip entries, 2 multi-vector kernel +
                           entry pass over the merged lists (entry mode 2); unset: by plan and nvec                        TILESPMV_MV_NATIVE */
    int mv_xcd_chunk;   /* XCD window of the multi-vector kernel                                             TILESPMV_MV_XCD_CHUNK */
    int lds_pad;        /* bytes of unused LDS added to every unit-kernel workgroup: fewer resident workgroups per CU  TILESPMV_LDS_PAD */
    int y_store;        /* y stores: 1 streaming (nontemporal), 0 plain; unset: streaming where y is >= 5 % of the launch's bytes  TILESPMV_Y_STORE */
    int desc_dict;      /* unit descriptors: unset = 4 B per unit + a dictionary of column patterns where the shard's units use few distinct
                           patterns AND the 8 bytes per unit are >= 2 % of the streams (stencil-like shards); 1 = wherever the patterns
                           are few; 0 = always the 12-B form.  Pooled plans (csr_split 2): any value but 0 = pattern dictionary where the patterns are few, as ONE
                           4-byte word per unit where window base, pattern id and tile-row fit it (round 6), else as 8-byte pairs; 2 = always pairs;
                           0 = the 20-byte form                                                                                 TILESPMV_DESC_DICT */
    int nt_stream;      /* value / entry-record / dense-tile loads: 1 nontemporal, 0 default cache policy; unset: nontemporal where one SpMV moves more
                           than 400 MB (about 1.6 x the Infinity Cache)                                                             TILESPMV_NT_STREAM */
    int x_panel_kb;     /* column panels (round 4): the merged entry lists of the workgroup entry mode are in column order, so the entries of a column panel (this many
                           KB of x; a power of two) are a run of a list; the plan records where the panels begin.  A panelled launch gives the unit kernel the first
                           x_panel_merge panels and every further run of x_panel_merge panels one more launch that adds its entries (y +=): the kernel boundary is the
                           one cheap chip-wide synchronisation, so all gathers of a pass fall into one slice of x and more of them hit the L2s (scattered matrices
                           with a large x: uniform random 8 M rows 1.00 -> 0.80 ms).  0 = no panels; unset: 2048 on entry-dominated shards whose x is >= 12 MB
                                                                                                                             TILESPMV_X_PANEL_KB */
    int x_panel_merge;  /* ... panels per pass: 0 = whole lists in the unit kernel (unpanelled launch); unset: chosen by timing at plan creation among 0 and the merges
                           that make passes of 4, 8 and 16 MB of x (kept when >= 3 % faster than the unpanelled launch)       TILESPMV_X_PANEL_MERGE */
    int placement_tries; /* where a large plan's blocks land in the card's memory decides between two states 13 % apart on the KKT matrices:
                           at plan creation the plan is timed (5 launches), moved to freshly allocated blocks (allocated BEFORE the old ones are freed) and timed
                           again, up to this many placements (all held until the choice is made); the fastest one seen is kept, and the search ends early once a placement is >= 9 % faster
                           than a slow time two placements agree on, or five placements agree within 1.5 %.  unset: 8 for plans of >= 1 GB, else 1 (= off)
                                                                                                                    TILESPMV_PLACEMENT_TRIES */
    int x_slice_passes; /* column slices pinned to XCDs (round 4): the other use of the recorded panels.  The unit kernel leaves the entry lists alone; per pass one launch of
                           8 x groups workgroups follows in which workgroup b (dispatched to XCD b & 7) takes its group's entries of column slice pass * 8 + (b & 7), so an XCD
                           only ever gathers from its own slice of x, which stays in its L2, and adds the rows it touched to y atomically — the eight partial sums of a row
                           meet in an order that is not fixed: never chosen when entry_ordered = 1.  N > 0 = N passes (8 N slices); 0 = off; unset (and x_panel_merge unset): timed at plan creation
                           beside the panelled forms (1, 2, 4 passes where a slice would be about 1-8 MB), kept when fastest and >= 3 % faster than the plain launch.
                           NOTE: that timed choice can pick this form on large grids where the rule alone would have added in a fixed order — the default plan of a large scattered shard
                           is then NOT bit-reproducible on real-valued data (its facts say so: TILESPMV_INFO_ENTRY_ORDERED = 0, TILESPMV_INFO_X_SLICE_PASSES > 0) and which form it has can differ
                           from run to run and rank to rank; entry_ordered = 1 or deterministic = 1 pins reproducible sums (bench.py reports what that costs per workload)
                                                                                                                    TILESPMV_X_SLICE_PASSES */
    int deterministic;  /* 1: no decision of this plan is taken by a stopwatch and every sum has a plan-fixed order — placement_tries, x_panel_merge, x_slice_passes, pace and autotune
                           that the caller left unset are switched off (as if 1 / 0 / 0 / 0 / 0) and entry_ordered is 1: two plans of the same matrix then have the same layout,
                           the same launch form and give bit-identical y on any data, run after run and rank after rank (the reference's own timing loop never changes the
                           result either, src/tilespmv_cuda.h:1112-1137).  0 / unset: the defaults described above                       TILESPMV_DETERMINISTIC */
    int absorb;         /* round 6: list entries of a COO tile that sit within a few columns of a neighbouring ELL tile (the corner entries of a band / stencil) move into
                           that tile's padding slots — the unit's 16-column window of x is shifted by -3 .. 3 columns — instead of going to the strip's entry list; and a
                           unit whose columns are the previous unit's moved one to the right (consecutive diagonals of a band tile) takes that unit's x one lane up
                           instead of gathering.  unset / 1 = both, where they apply (classic unit plans); 2 = absorbed entries only; 0 = neither                                                    TILESPMV_ABSORB */
    int value_narrow;   /* fp64 build: a plan whose unit values all survive double -> float -> double unchanged (finite, and ±0 or |v| >= FLT_MIN: constant-coefficient stencils,
                           graph Laplacians, integer / pattern matrices, anything assembled in single precision) stores them as 4-byte floats, four units per 16-byte lane load;
                           the kernels widen them in registers and the arithmetic stays fp64, so y keeps every bit.  Classic (non-pooled) unit plans of the stream kernel with
                           entry mode 0 or 2 and 16 strips per workgroup, built without TILESPMV_CREATE_VALUE_MAP and without nt_stream = 0; a narrow plan always reads its
                           streams nontemporally (nt_stream 1).  Where every value is moreover +-0 or a NORMAL IEEE binary16 number (every integer up to 2048, coefficients such as 0.25) the
                           plan can store 2-byte halves instead, four units per 8-byte lane load, widened half -> float -> double (both exact): y still keeps every bit.
                           0 = never; 1 = floats wherever eligible and narrowable (never halves); 2 = the narrowest width every value allows, wherever eligible: 2, else 4, else 8 bytes;
                           unset = the narrowest width whose launch still moves more than the 400 MB above which nt_stream is 1 by rule (smaller plans live in the caches and are bound by
                           latency, not bytes).  Ignored by the fp32 build.  TILESPMV_INFO_UNIT_VALUE_BYTES tells which form a plan has             TILESPMV_VALUE_NARROW */
    int unit_lean;      /* classic unit plans with nontemporal streams, entry mode 0 or 2 and 16 strips per workgroup in which no unit is a row unit (no dense-row tiles) run lean forms of
                           the unit kernel: what only a row unit needs — and, where the plan has no derived unit either (absorb), what only a derived unit needs — is compiled out,
                           and the unit loop tests the task's end once per task instead of once per unit.  Same plan, same streams, same arithmetic in the same order: y keeps every
                           bit.  0 = always the general kernels; unset / 1 = the lean form wherever the plan's facts allow.  TILESPMV_INFO_UNIT_LEAN tells which form a plan's launch takes.
                           The environment variable is read once per process                                                                TILESPMV_UNIT_LEAN */
    int reserved[1];    /* must be TILESPMV_KNOB_DEFAULT or 0 */
} tilespmv_plan_options;
void tilespmv_plan_options_init(tilespmv_plan_options *opts);
/* "name:offset,..." of every field above as the library was built: lets a binding that mirrors the struct by hand verify
 * its field order (the Python mirror once had four knobs permuted and nothing noticed). */
const char *tilespmv_plan_options_layout(void);

/* Returns 0 on success, non-zero (message on stderr) when no HIP device / extension is
 * usable — there is no CPU fallback behind this entry point.
 * Plan creation allocates, copies and synchronises (it always did); since round 4 it may also TIME a few launches of the finished plan on the default stream with scratch
 * x / y of its own: plans of >= 1 GB try up to `placement_tries` memory placements, shards with column panels recorded choose the panels per pass, opt-in paced plans
 * calibrate their timetable.  Every such choice has a knob that fixes it (placement_tries = 1, x_panel_merge + x_slice_passes, pace_period_us) — a fixed choice times nothing;
 * `deterministic = 1` fixes them all.  Since round 5 the value stream's final layout is written by a kernel (the emitted values are uploaded to a scratch buffer first): peak device
 * memory during creation = the plan + one more copy of its unit values (freed before the call returns); TILESPMV_ENCODE_ON_HOST=1 keeps that pass on the host.
 * Dimension limits: every `int` rowA / colA is either served or refused with a status — Tile_create, tilespmv_cpu and the matrix cache serve all of them (tile counts are
 * computed without overflow up to 2^31 - 1).  The unit-stream kernel (TILESPMV_KERNEL_STREAM) keeps column blocks in 24 bits: colA <= 2^28.  Beyond that TILESPMV_KERNEL_AUTO
 * takes the first-generation kernel (with TILESPMV_COO_IN_TILE or the CSR fallback; 64-bit x offsets, served up to colA = 2^31 - 1), an explicit TILESPMV_KERNEL_STREAM
 * returns -2 with a message on stderr, and the device builders (tilespmv_plan_create_from_csr / _from_device_csr) return -4 like for every option without a device path.
 * -2 is also the status of a shard whose unit, entry or tile ids leave the int32 range.  (tests/test_gpu_dim_limits.py runs both sides of each limit.) */
int tilespmv_plan_create(tilespmv_plan **plan, const Tile_matrix *matrix, int rowA, int colA,
                         MAT_PTR_TYPE nnzA, const tilespmv_plan_options *opts);
void tilespmv_plan_destroy(tilespmv_plan *plan);

/* Preprocessing on the device (new; SURVEY.md S8 f1 "device-side"; replaces the reference's Tile_create + upload, src/csr2tile.h:629-1020 + src/tilespmv_cuda.h:828-1057, end to end).
 *
 * Tile_create_device: the host Tile_create computed by kernels — the CSR arrays go up, every member array of the Tile_matrix comes back, byte for byte what Tile_create /
 * Tile_create_ex builds (flags: TILESPMV_CREATE_QUIET, TILESPMV_CREATE_CDNA4, and since round 6 TILESPMV_CREATE_HYB — width search src/csr2tile.h:279-306, pack :505-548, index bytes
 * :984-1008 as per-tile device code).  Returns 0, -1 no HIP device (there is no CPU fallback behind this entry point: call Tile_create), -2 an offset leaves the int32 range
 * of Tile_matrix, or a tile with a repeated position holds more than 255 entries ("Repeated entries" above tilespmv_plan_spmv: decided by the selection kernel, nothing is
 * packed, *matrix is not written), -3 HIP error / out of device memory.
 *
 * tilespmv_plan_create_from_csr: CSR in, resident plan out, nothing but the CSR arrays crossing the bus — the tiled matrix is built on the device and stays there, the stages of the
 * plan builder that touch every nonzero run as kernels calling the same per-tile functions as the host builder, so the plan is the one tilespmv_plan_create makes from
 * Tile_create's output (same streams, same y).  Not every option has a device path: returns -4 (and builds nothing) for the first-generation kernel, the CSR fallback
 * mode and whole CSR tiles (csr_split = 0) — use Tile_create + tilespmv_plan_create for those (HYB tiles, TILESPMV_CREATE_HYB in `create_flags`, are served since round 6).  autotune = 1 is served: every candidate plan is built from the one device-resident tiled
 * matrix (the CSR-fallback candidate, which has no device path, is not among them).  Other return codes as above (-2 also for the refused tile: *plan stays NULL).
 * Peak device memory during the call: the CSR arrays + the tiled matrix + the sort's key buffers (about 40 bytes per nonzero in fp64) beside the plan.  With TILESPMV_CREATE_VALUE_MAP add
 * the value map (4 bytes per value slot of the plan — about 4.5 to 6 bytes per nonzero; it stays with the plan) and, for tilespmv_plan_create_from_device_csr, one more value array
 * (sizeof(MAT_VAL_TYPE) bytes per nonzero, freed before the call returns).  With TILESPMV_CREATE_TRANSPOSE add the transposed CSR (about 4 + sizeof(MAT_VAL_TYPE) bytes per
 * nonzero) and, while it is being made, the transposer's scratch (about 16 bytes per nonzero + the radix sort's temporary storage); all freed before the call returns. */
int Tile_create_device(Tile_matrix *matrix, int rowA, int colA, MAT_PTR_TYPE nnzA, const MAT_PTR_TYPE *csrRowPtrA,
                       const int *csrColIdxA, const MAT_VAL_TYPE *csrValA, unsigned flags);
int tilespmv_plan_create_from_csr(tilespmv_plan **plan, int rowA, int colA, MAT_PTR_TYPE nnzA, const MAT_PTR_TYPE *csrRowPtrA,
                                  const int *csrColIdxA, const MAT_VAL_TYPE *csrValA, unsigned create_flags,
                                  const tilespmv_plan_options *opts);
/* The same with the CSR arrays already in DEVICE memory (a solver that assembles on the GPU, a framework's CSR tensor): nothing crosses the bus but the few numbers the host decides on.
 * The row pointer starts at 0; the arrays are borrowed for the duration of the call and not modified. */
int tilespmv_plan_create_from_device_csr(tilespmv_plan **plan, int rowA, int colA, MAT_PTR_TYPE nnzA, const MAT_PTR_TYPE *d_csrRowPtrA,
                                         const int *d_csrColIdxA, const MAT_VAL_TYPE *d_csrValA, unsigned create_flags,
                                         const tilespmv_plan_options *opts);

/* New values, same pattern (a solver that reassembles its matrix: interior-point KKT systems, Newton on a nonlinear FEM problem, variable-coefficient time steps).
 * The plan must have been created with TILESPMV_CREATE_VALUE_MAP by tilespmv_plan_create_from_csr or tilespmv_plan_create_from_device_csr.  d_csrVal is DEVICE memory holding the values
 * of the CSR the plan was created from, in the same order — same row pointer, same column indices, same duplicates, indexed like the creation's value argument (a shard,
 * tilerow_begin / tilerow_end, takes the full array too and reads only its own tile-rows' values).  Every value of the plan is rewritten in one asynchronous pass on `stream`:
 * nothing is rebuilt, allocated or copied to or from the host, no synchronisation — safe to capture into a hipGraph; the single-stream rule of tilespmv_plan_spmv holds (an SpMV of
 * this plan and an update must not run at the same time on two streams).
 * Contract: a plan created with the flag from values v1 and updated to v2 holds exactly the bytes a plan created with the flag from v2 holds (tilespmv_plan_stream_digests agree,
 * the facts agree, y agrees bit for bit where TILESPMV_INFO_ENTRY_ORDERED is 1).  To make that possible a flagged plan's layout follows the PATTERN alone: an explicit zero of
 * the CSR is a stored entry like any other (an unflagged plan treats an ELL slot that holds 0 at column nibble 0 as padding, and a packed entry record of value 0, offset 0 and
 * destination 0 as null).  On data without explicit zeros a flagged and an unflagged plan of the same matrix and options have identical SpMV streams — except
 * where the unflagged plan stores its unit values as floats (value_narrow): a flagged plan never does, because its layout may not depend on the values.
 * The pattern is the caller's promise: a changed pattern cannot be detected.  Values must be finite, like every value a plan multiplies.
 * Returns a hipError_t value (0 = success, hipErrorInvalidValue for a NULL argument), or TILESPMV_ERR_NO_VALUE_MAP (-4) — plan untouched — for a plan created without the flag or
 * by tilespmv_plan_create (a host Tile_matrix has no link back to CSR order).  TILESPMV_INFO_VALUE_MAP_BYTES is the map's size. */
#define TILESPMV_ERR_NO_VALUE_MAP (-4)
int tilespmv_plan_update_values(tilespmv_plan *plan, const MAT_VAL_TYPE *d_csrVal, void *stream);

/* Values: x (and the matrix values) must be FINITE.  Zero-padded payload is multiplied by real x entries — the padding
 * slots of ELL / HYB tiles exactly as in the reference (src/tilespmv_cpu.h:173-192 walks all `width` slots), and in
 * this engine also CSR tiles re-expressed as units, dense tiles, and the clamped reads of a partial last column block —
 * so an Inf or NaN in x can reach rows that store no entry in that column (0 * Inf = NaN).  One more carrier, outside the tile: the merged entry
 * lists (wavefront / workgroup entry modes, CSR fallback) pad a 64-record chunk that had to be closed early — its columns span 2^(32 - dest_bits)
 * (2^20 ... 2^23) or more, or, in slab-paced plans, the local part of a list ends — with null records (value 0, destination = the group's first
 * row, column = the chunk's first column): they add 0 * x[that column] to that row (tests/test_gpu_configs.py::test_non_finite_x_reaches_only_what_the_header_says).
 *
 * Repeated entries: a CSR may store the same (i, j) more than once (element contributions not yet summed, an uncoalesced framework CSR, a symmetric .mtx that lists an
 * entry twice).  Nothing is summed at creation: every stored entry keeps a slot of its own, and y is the sum over ALL stored entries — tilespmv_cpu, every plan form, SpMV
 * and SpMM, transposed plans, value-mapped plans before and after tilespmv_plan_update_values.  (1) A 16 x 16 tile without a repeated position is built exactly as before,
 * byte for byte, also beside tiles that have one.  (2) A tile with a repeated position is never stored as DNS, DNSROW or DNSCOL (one value per position): it gets the
 * format the selection rule gives with those three branches skipped — COO, ELL, HYB or CSR (an ELL / HYB width beyond 127, what tilewidth holds, becomes CSR).  (3) A tile
 * with a repeated position and more than 255 entries is REFUSED: its in-tile row pointer and blknnznnz are bytes.  That covers a local row of 256 entries, where 8-bit row
 * counters wrap (16 columns: it has repeats and at least 256 entries).  Entry points with a status return -2 and build nothing; Tile_create / Tile_create_ex are void and
 * exit(2), as for an int32 offset overflow; both print "tilespmv: tile-row R, column block C: N entries with a repeated position ..." on stderr.  Sum duplicates first for
 * such a matrix.  Not part of this: dense-row / dense-column tiles still assume ascending columns inside a row, as in the reference.
 *
 * y[16*tilerow_begin .. 16*tilerow_end) = A_shard * x.  d_x has colA elements, d_y points at
 * element 0 of the FULL-length y (the shard writes only its own rows).  Asynchronous on
 * `stream`, no allocation or synchronisation inside (safe to capture into a hipGraph).  One plan
 * must not execute on two streams at the same time: split tile-rows use per-plan scratch slots
 * and counters.  Returns a hipError_t value (0 = success). */
int tilespmv_plan_spmv(tilespmv_plan *plan, const MAT_VAL_TYPE *d_x, MAT_VAL_TYPE *d_y,
                       void *stream);

/* `count` back-to-back SpMVs on `stream` (same as calling tilespmv_plan_spmv `count` times; saves the
 * caller's per-call overhead when one SpMV takes tens of microseconds).  Returns a hipError_t value. */
int tilespmv_plan_spmv_n(tilespmv_plan *plan, const MAT_VAL_TYPE *d_x, MAT_VAL_TYPE *d_y, void *stream, int count);

/* Multi-vector form (SpMM; new): Y[rows][nvec] = A_shard * X[colA][nvec], X and Y
 * row-major (the nvec values of one row are contiguous) and 16-byte aligned, nvec in {1, 2, 4, 8}.
 * The matrix is streamed once for all nvec right-hand sides.  d_Y points at row 0 of the full-length
 * Y.  Unit-stream plans with in-tile COO and split CSR tiles (the defaults) run the native multi-vector
 * kernels; plans built with TILESPMV_COO_FALLBACK, TILESPMV_KERNEL_DIRECT or TILESPMV_CSR_SPLIT=0 go one
 * right-hand side at a time through their own SpMV (column gathered / scattered by two small kernels).
 * Returns hipErrorInvalidValue (1) for other nvec / misaligned pointers. */
#define TILESPMV_MAX_NVEC 8
int tilespmv_plan_spmm(tilespmv_plan *plan, const MAT_VAL_TYPE *d_X, MAT_VAL_TYPE *d_Y, int nvec,
                       void *stream);
double tilespmv_plan_time_spmm(tilespmv_plan *plan, const MAT_VAL_TYPE *d_X, MAT_VAL_TYPE *d_Y,
                               int nvec, void *stream, int warmup, int reps);
/* Plans without a native multi-vector kernel (CSR fallback, first-generation kernel, whole CSR tiles; or mv_native = 0) run one right-hand side at a time
 * on transposed copies of X and Y that live with the plan.  tilespmv_plan_reserve_spmm allocates them for up to `nvec`
 * right-hand sides (hipMalloc: synchronises) so that tilespmv_plan_spmm itself never allocates — call it before capturing
 * tilespmv_plan_spmm into a hipGraph.  Without it the first such tilespmv_plan_spmm call allocates (and would fail under
 * stream capture).  Returns a hipError_t value. */
int tilespmv_plan_reserve_spmm(tilespmv_plan *plan, int nvec);

/* Test / diagnostic entry (new): builds the plan's device layout ON THE HOST ONLY — no HIP call, works without a GPU — with
 * exactly the code tilespmv_plan_create runs, hashes every stream it would upload (FNV-1a-64 over element counts and bytes,
 * in upload order) and checks that the packed entry lists decode back to their entries.  Returns 0 and the digest (and the
 * plan facts, `info` may be NULL), or the error tilespmv_plan_create would return.  Used by the CPU test-suite and by the
 * ThreadSanitizer driver (two threads building differently tuned layouts); it is not part of any compute path. */
int tilespmv_plan_layout_digest(const Tile_matrix *matrix, int rowA, int colA, MAT_PTR_TYPE nnzA,
                                const tilespmv_plan_options *opts, unsigned long long *digest,
                                long long *info /* [TILESPMV_INFO_COUNT] or NULL */);

/* Same host-only build, one digest per STAGE of the unit-stream layout builder (hip_plan_stream.hip), so that a test can say which
 * knob is allowed to change which stage (`stage_digests` = TILESPMV_STAGE_COUNT values; all 0 for first-generation plans). */
enum {
    TILESPMV_STAGE_COUNT_ROWS = 0,    /* per tile-row: units / entries / whole tiles / dense tiles, cost */
    TILESPMV_STAGE_CHOOSE = 1,        /* strip size, entry mode, strips per workgroup, ordered adds, brick order */
    TILESPMV_STAGE_CUT = 2,           /* strips and pieces -> task records */
    TILESPMV_STAGE_EMIT = 3,          /* unit descriptors + values, entry triples, whole-tile and dense payload (tile order) */
    TILESPMV_STAGE_ORDER = 4,         /* task order: linear / brick (+ x windows) */
    TILESPMV_STAGE_ENCODE = 5,        /* value groups per task, 12-B descriptors or 4-B words + dictionary */
    TILESPMV_STAGE_ENTRIES = 6,       /* merged, column-ordered, packed entry lists */
    TILESPMV_STAGE_FINISH = 7,        /* byte model and cache-policy flags */
    TILESPMV_STAGE_COUNT = 8
};
int tilespmv_plan_layout_stages(const Tile_matrix *matrix, int rowA, int colA, MAT_PTR_TYPE nnzA,
                                const tilespmv_plan_options *opts, unsigned long long *stage_digests,
                                long long *info /* [TILESPMV_INFO_COUNT] or NULL */);

/* Plan facts for reports: index into `out` by TILESPMV_INFO_*. */
enum {
    TILESPMV_INFO_DEVICE_BYTES = 0,   /* bytes of the resident plan */
    TILESPMV_INFO_STREAM_BYTES = 1,   /* bytes one SpMV must read/write at least (plan model) */
    TILESPMV_INFO_NNZ = 2,            /* true nonzeros covered by the shard */
    TILESPMV_INFO_ROWS = 3,
    TILESPMV_INFO_TILES = 4,
    TILESPMV_INFO_COO_MODE = 5,       /* resolved mode */
    TILESPMV_INFO_DENSE_MODE = 6,
    TILESPMV_INFO_KERNEL = 7,
    TILESPMV_INFO_NUM_TASKS = 8,
    TILESPMV_INFO_NUM_SPLIT_ROWS = 9,
    TILESPMV_INFO_FALLBACK_NNZ = 10,  /* nonzeros executed by the CSR fallback kernel */
    TILESPMV_INFO_BUILD_US = 11,      /* host time of the re-layout (plan build), microseconds */
    TILESPMV_INFO_UPLOAD_US = 12,     /* hipMalloc + hipMemcpy time of the plan's streams, microseconds */
    TILESPMV_INFO_ENTRY_MODE = 13,    /* COO entry lists run per strip (0), per wavefront (1), per workgroup (2) */
    TILESPMV_INFO_ENTRY_ORDERED = 14, /* 1: the order of the additions is fixed by the plan (bit-reproducible y: every launch of this plan, and every plan of the same facts, host- or device-built —
                                         column-panel passes and split tile-rows included; tests/test_gpu_parity.py::test_panelled_plans_with_split_rows_sum_in_a_fixed_order, scripts/reproducibility_sweep.py) */
    TILESPMV_INFO_STRIP_COST = 15,    /* strip size target the plan was cut with */
    TILESPMV_INFO_WG_STRIPS = 16,     /* strips per workgroup of the unit kernel (16 or 32) */
    TILESPMV_INFO_LIST_ENTRIES = 17,      /* nonzeros on the strips' entry lists (COO tiles, HYB / CSR-tile remainders) after the ones that fit the padding of a neighbouring ELL unit moved there
                                             (tilespmv_plan_options.absorb); unit-stream plans, 0 otherwise.  (Until round 6: a retired fact that was always 0) */
    TILESPMV_INFO_DERIVED_UNITS = 18,     /* classic unit plans: units that take their x from the previous unit, one lane up, instead of gathering (the consecutive diagonals of a band /
                                             stencil tile: csrc/plan_tile_ops.h; tilespmv_plan_options.absorb = 2 switches them off).  (Until round 6: a retired fact that was always 0) */
    TILESPMV_INFO_BRICK_ORDER = 19,       /* 1: the strips were regrouped into bricks of the grid (stencil-like shard) */
    TILESPMV_INFO_DESC_BYTES = 20,        /* bytes per unit descriptor in HBM: 12, or 4 (column-pattern dictionary); pooled plans 20, or 8 (pattern dictionary); wide pooled plans 28 */
    TILESPMV_INFO_NT_STREAM = 21,         /* 1: the unit kernel reads the value / entry-record streams with nontemporal loads */
    TILESPMV_INFO_UNIT_VALUE_BYTES = 22,  /* bytes per stored unit value: 8, or 4 (floats) / 2 (halves) in a narrow plan (value_narrow); the fp32 build always reports 4 */
    TILESPMV_INFO_UNIT_LEAN = 23,         /* form of the unit kernel the plan's launch takes: 0 = general, 1 = lean (no unit is a row unit), 2 = lean without derived units (tilespmv_plan_options.unit_lean;
                                             the same for host- and device-built plans of one matrix).  (Until this fact: a retired slot that was always 0) */
    TILESPMV_INFO_PLACEMENT_TRIES = 24,   /* arena placements timed at plan creation (large plans; 0 / 1 = the first one was kept) */
    TILESPMV_INFO_RETIRED_25 = 25,        /* always 0 */
    TILESPMV_INFO_X_PANELS = 26,          /* column panels of the entry lists = launches of the entry part (1 = not panelled) */
    TILESPMV_INFO_X_PANEL_MERGE = 27,     /* recorded panels per pass of the panelled launch (0 = whole lists in the unit kernel) */
    TILESPMV_INFO_SCATTERED_ENTRIES = 28, /* workgroup entry mode: list entries whose column lies more than 2,048 columns outside their group's own rows — the gathers that
                                             no neighbour shares (the chip resolves about 59 G of those per second from a table that misses the L2s: profiles/r04_gather_granule.txt) */
    TILESPMV_INFO_X_SLICE_PASSES = 29,    /* column slices pinned to XCDs: launches of the sliced entry part (0 = not used); 8 x this many slices of x */
    TILESPMV_INFO_CSR_FORM = 30,          /* what CSR-format tiles became: 0 whole tiles (own pass), 1 ELL-style split (units + list entries), 2 pooled units, 3 wide pooled units (256-column windows) */
    TILESPMV_INFO_TIMED_CHOICES_US = 31,  /* microseconds of plan creation spent TIMING candidates (placement retry, column panels / slices); part of build_us; 0 = nothing was timed */
    TILESPMV_INFO_DEVICE_BUILD = 32,      /* 1: built by tilespmv_plan_create_from_csr (Tile_create, COUNT / EMIT / ENCODE on the device) */
    TILESPMV_INFO_TILE_CREATE_US = 33,    /* ... microseconds of its device Tile_create, the upload of the CSR arrays included (0 otherwise) */
    TILESPMV_INFO_VALUE_MAP_BYTES = 34,   /* bytes of the value map (TILESPMV_CREATE_VALUE_MAP; 0 without it) — not part of TILESPMV_INFO_DEVICE_BYTES, which stays the SpMV plan's */
    TILESPMV_INFO_COUNT = 35
};
void tilespmv_plan_info(const tilespmv_plan *plan, long long *out /* [TILESPMV_INFO_COUNT] */);
/* Strided strips (environment knob TILESPMV_STRIP_SWEEP: unset = by rule, 0 = never, 1 = wherever the shard's structure allows): the stride S, in tile-rows, between
 * the consecutive tile-rows of one strip of the plan's unit stream; 1 = consecutive tile-rows (every plan the knob does not reach).  Stencil-like shards whose grid lines are whole
 * tile-rows long get S = one grid line: a strip then sweeps down the grid and reads the windows of x it shares with its previous tile-row while they are still in the caches.  The
 * plan holds the same units, values and task records in another order; y is the unstrided plan's bit for bit. */
int tilespmv_plan_strip_stride(const tilespmv_plan *plan);
/* The deep unit kernel (environment knob TILESPMV_UNIT_DEEP: unset = by rule, 0 = never, 1 = wherever the plan allows): 0, or the number of unit batches
 * whose x gathers a wavefront of the plan's unit launch keeps in flight.  It serves plans that take a lean form (TILESPMV_INFO_UNIT_LEAN > 0) with per-strip entries, 16 strips
 * per workgroup and nontemporal streams and hold nothing but units: no list entry, no split tile-row, no fallback launch.  The plan is the same plan byte for byte — streams,
 * facts (tilespmv_plan_info) and y — whatever this returns.  tilespmv_plan_layout_unit_deep answers for the plan a host-only layout build of the matrix would make (no GPU
 * needed; negative on error), as tilespmv_plan_layout_digest does for the streams. */
int tilespmv_plan_unit_deep(const tilespmv_plan *plan);
int tilespmv_plan_layout_unit_deep(const Tile_matrix *matrix, int rowA, int colA, MAT_PTR_TYPE nnzA, const tilespmv_plan_options *opts);
/* Test / audit aid: one (member offset in the plan object, bytes, FNV-1a-64 of the bytes read back from the device) triple per stream of the plan, at most max_streams of them
 * written; returns the number of streams (or -3 on a HIP error).  Two plans of one matrix and one option set — one built from a host Tile_matrix, one by
 * tilespmv_plan_create_from_csr — must agree triple for triple (tests/test_gpu_device_build.py). */
long long tilespmv_plan_stream_digests(const tilespmv_plan *plan, unsigned long long *out /* [3 * max_streams] */, long long max_streams);

/* Times `reps` back-to-back SpMVs on `stream` with hipEvents recorded on that stream (after
 * `warmup` untimed ones) and returns the mean milliseconds per SpMV, or a negative value on
 * error.  Used by bench.py for the live per-launch figure. */
double tilespmv_plan_time(tilespmv_plan *plan, const MAT_VAL_TYPE *d_x, MAT_VAL_TYPE *d_y,
                          void *stream, int warmup, int reps);

/* The reference's own timing protocol as a C loop (src/tilespmv_cuda.h:1112-1137): wall clock (gettimeofday) around one
 * launch + stream synchronize, averaged over `reps`; milliseconds per SpMV, negative on error.  call_tilespmv_hip prints
 * this number in the reference's "CUDA SpMV runtime" line; bench.py reports it as reference_style_timing. */
double tilespmv_plan_time_reference_style(tilespmv_plan *plan, const MAT_VAL_TYPE *d_x, MAT_VAL_TYPE *d_y,
                                          void *stream, int reps);

/* Multi-GPU helper: nnz-balanced contiguous tile-row partition (new; the reference is
 * single-GPU, src/main.cu:74).  Writes nparts+1 tile-row boundaries. */
void tilespmv_partition_tilerows(const Tile_matrix *matrix, int nparts, int *bounds);

/* Library facts. */
int tilespmv_sizeof_value(void);    /* 8 or 4 */

/* ---- Permuted-numbering plans (new, round 6; no reference counterpart: the reference multiplies in the numbering of its file, src/main.cu:59-110).
 * For callers that STAY in the permuted numbering — a solver: x is permuted once at entry, K products run on plan-ordered vectors, y is un-permuted once at exit
 * (tilespmv_amd/halo.py HaloSpMV(reorder=True) / cg).  Around ONE product the two permutations cost what the better numbering saves (profiles/r05_rcm_probe.txt).
 *   tilespmv_reorder_rcm   reverse Cuthill-McKee on the symmetrised pattern of the leading n x n block (host, deterministic; perm[new] = old)
 *   tilespmv_csr_permute   B = P A P^T; columns >= n (a rank's halo columns) stay; every row of B comes out in ascending column order (the reference's dense-row / dense-col
 *                          tiles assume that: src/csr2tile.h:586,600-605); val / out_val may be NULL
 *   tilespmv_permute_vector  device: scatter = 0: out[i] = in[perm[i]] (into plan order), scatter = 1: out[perm[i]] = in[i] (back); asynchronous on `stream`
 * The plan of B is created like any other (Tile_create + tilespmv_plan_create, or tilespmv_plan_create_from_csr). */
int tilespmv_reorder_rcm(int n, const MAT_PTR_TYPE *csrRowPtr, const int *csrColIdx, int *perm /* [n] */);
int tilespmv_csr_permute(int n, const MAT_PTR_TYPE *csrRowPtr, const int *csrColIdx, const MAT_VAL_TYPE *csrVal, const int *perm,
                         MAT_PTR_TYPE *outRowPtr /* [n + 1] */, int *outColIdx, MAT_VAL_TYPE *outVal);
long long tilespmv_csr_bandwidth(int n, const MAT_PTR_TYPE *csrRowPtr, const int *csrColIdx);   /* max |i - j| over the leading n x n block */
int tilespmv_permute_vector(const MAT_VAL_TYPE *d_in, MAT_VAL_TYPE *d_out, const int *d_perm, long long n, int scatter, void *stream);   /* hipError_t value */

/* ---- Transposed CSR (new).  The transpose of a rowA x colA CSR (rp, ci, v) is the colA x rowA CSR whose entries are A's in CSR order, STABLY sorted by column:
 *   order = stable argsort of ci[rp[0] .. rp[rowA]);  rpT = the column counts, scanned (rpT[0] = 0);  ciT[k] = the row of entry order[k];  vT[k] = v[rp[0] + order[k]];
 *   srcT[k] = rp[0] + order[k], the entry's position in the caller's arrays.
 * Every row of A^T comes out in ascending column order whatever the order inside A's rows (what the dense-row / dense-col tiles need); duplicates keep their relative order.
 * rp[0] != 0 is allowed (a row block of a larger CSR): ci and v are then read from position rp[0] on, and srcT names positions of the caller's arrays.  v / vT and srcT may be
 * NULL (no values gathered, no positions written).  Output sizes: rpT[colA + 1], ciT / vT / srcT[rp[rowA] - rp[0]].
 *   tilespmv_csr_transpose         host, threaded like the other host passes.  Returns 0, or -1 for a bad argument (NULL array, a decreasing row pointer, a column index
 *                                  outside [0, colA)) — nothing meaningful is written then.
 *   tilespmv_csr_transpose_device  the same on DEVICE arrays: a column histogram (int atomics), one exclusive scan into rpT, the row of every entry, ONE stable radix sort of
 *                                  (column, position) pairs over ceil(log2(colA)) key bits, then the gathers.  Allocates its own scratch (about 16 bytes per nonzero plus the sort's
 *                                  temporary storage) and synchronises `stream` before it returns: it cannot be captured into a hipGraph.  Returns a hipError_t value
 *                                  (hipErrorInvalidValue for a bad argument or a column index outside [0, colA)). */
int tilespmv_csr_transpose(int rowA, int colA, const MAT_PTR_TYPE *csrRowPtr, const int *csrColIdx, const MAT_VAL_TYPE *csrVal /* may be NULL */,
                           MAT_PTR_TYPE *rowPtrT /* [colA + 1] */, int *colIdxT, MAT_VAL_TYPE *valT /* may be NULL */, int *srcT /* may be NULL */);
int tilespmv_csr_transpose_device(int rowA, int colA, const MAT_PTR_TYPE *d_csrRowPtr, const int *d_csrColIdx, const MAT_VAL_TYPE *d_csrVal /* may be NULL */,
                                  MAT_PTR_TYPE *d_rowPtrT, int *d_colIdxT, MAT_VAL_TYPE *d_valT /* may be NULL */, int *d_srcT /* may be NULL */, void *stream);

/* ---- A solver in the library: conjugate gradients around a resident plan (new; no reference counterpart: the reference multiplies once,
 * src/main.cu:59-110).  A x = b for a symmetric positive definite A, optionally preconditioned by the inverse diagonal (Jacobi).  One iteration = the plan's product Ap = A p
 * (tilespmv_plan_spmv, whatever launch form the plan has) and THREE streaming kernels: p.Ap;  x += alpha p, r -= alpha Ap with r.r (and r.z, z = dinv o r);  p = z + beta p.
 * Every scalar (rho = r.z, p.Ap, alpha, beta, |r|^2, |b|^2, the iteration count, the breakdown flag) lives in device memory: a reducing kernel leaves one partial sum per workgroup
 * and the kernel that consumes the scalar adds the partials itself, every workgroup in the same order.  The number of partials and the order of every addition are fixed by the
 * number of rows alone, sums and scalars are double in both libraries (alpha, beta rounded to the value type once, where they multiply): on a plan whose y is bit-reproducible
 * (TILESPMV_INFO_ENTRY_ORDERED = 1, e.g. deterministic = 1) the iterates x_k are too, run after run and plan after plan.
 * Guards, taken on the device: rho = 0 (b = 0, or an exactly zero residual) -> alpha = beta = 0, further iterations leave x and r as they are — a captured graph of k iterations
 * may overrun convergence; rho > 0 and not p.Ap > 0 (A is not positive definite on this Krylov space), or rho < 0 (dinv is not) -> the breakdown flag is set, alpha = beta = 0 in
 * that and every later iteration, x keeps its last good value.
 * A tilespmv_cg and its plan run on ONE stream at a time (the single-stream rule of tilespmv_plan_spmv, restated: the workspace is per solver, the split-row scratch per plan).
 * d_b, d_x and d_dinv are DEVICE vectors of `rows` elements, 16-byte aligned (hipErrorInvalidValue otherwise); nothing behind element rows - 1 is read or written.
 * Cost per iteration beside the product: 11 vector elements per row read or written (13 with Jacobi) in 3 launches; measured against a loop of torch operations (14 per row, about ten
 * launches) in profiles/cg_fused_ab.txt.  Workspace: 3 vectors of rows + 16 elements and 33 KB.
 *
 *   tilespmv_cg_create      binds a workspace to `plan`, which must be square and whole (tilerow_begin = 0, tilerow_end = tilem; a transposed plan qualifies when square) and must
 *                           outlive it.  d_dinv: NULL = plain CG; else the inverse diagonal, borrowed until destroy — its VALUES may change between solves (a value map:
 *                           tilespmv_plan_update_values, then tilespmv_csr_diagonal_device into the same array).  Allocates r, p, Ap (rows + 16 elements each: every y of this project
 *                           has room behind it), the partial-sum arrays and the scalar block in one hipMalloc (synchronises).  Returns 0, hipErrorInvalidValue (NULL / non-square /
 *                           shard plan / misaligned d_dinv: nothing allocated, and for a NULL argument no HIP call made), or the hipMalloc error.
 *   tilespmv_cg_begin       r = b - A x (x is the caller's start vector; pass zeros for none), p = z, rho = r.z, |r|^2, |b|^2; iteration count and breakdown flag cleared.
 *   tilespmv_cg_iterate     `count` iterations back to back.  Like begin: asynchronous on `stream`, no allocation, no synchronisation, no host read — safe to capture into a hipGraph
 *                           (one linear chain of kernels).  It does not stop at any tolerance: only an exactly zero rho ends the changes to x.
 *   tilespmv_cg_state_read  synchronises `stream` and reads the scalar block (set out->size = sizeof(tilespmv_cg_state) first).  status: BREAKDOWN, CONVERGED when |r|^2 is exactly 0,
 *                           else RUNNING — a tolerance is the caller's (or tilespmv_cg_solve's) to apply to rr / bb.  rr is the recurrence's |r|^2, not a recomputed |b - A x|^2.
 *   tilespmv_cg_solve       begin, then iterate(check_every) + state_read until sqrt(rr / bb) <= rtol (CONVERGED), `maxiter` iterations are done (MAXITER; the last block is cut so that
 *                           no more run) or a breakdown (BREAKDOWN).  One host synchronisation per check.  bb = 0 -> x = 0, CONVERGED, 0 iterations.
 * All but destroy return a hipError_t value (0 = success). */
typedef struct tilespmv_cg tilespmv_cg;
typedef struct { unsigned size; int iterations; int status; double rr; double bb; } tilespmv_cg_state;
#define TILESPMV_CG_RUNNING 0
#define TILESPMV_CG_CONVERGED 1
#define TILESPMV_CG_MAXITER 2
#define TILESPMV_CG_BREAKDOWN 3
int tilespmv_cg_create(tilespmv_cg **cg, tilespmv_plan *plan, const MAT_VAL_TYPE *d_dinv /* may be NULL */);
void tilespmv_cg_destroy(tilespmv_cg *cg);
int tilespmv_cg_begin(tilespmv_cg *cg, const MAT_VAL_TYPE *d_b, MAT_VAL_TYPE *d_x, void *stream);
int tilespmv_cg_iterate(tilespmv_cg *cg, MAT_VAL_TYPE *d_x, int count, void *stream);
int tilespmv_cg_state_read(tilespmv_cg *cg, void *stream, tilespmv_cg_state *out);
int tilespmv_cg_solve(tilespmv_cg *cg, const MAT_VAL_TYPE *d_b, MAT_VAL_TYPE *d_x, double rtol, int maxiter, int check_every, void *stream, tilespmv_cg_state *out);
/* d_out[i] = the sum of the stored entries (i, i) of a device CSR, i < rows (duplicates added in storage order, in double; 0 where none is stored); invert != 0: 1 / that, and 1 where
 * it is 0 — the d_dinv of tilespmv_cg_create.  rows <= the CSR's column count; the row pointer is used as it stands (positions of the arrays passed).  One thread per row,
 * asynchronous on `stream`, capturable.  Returns a hipError_t value (hipErrorInvalidValue for a NULL array, hipErrorNoDevice without a device). */
int tilespmv_csr_diagonal_device(int rows, const MAT_PTR_TYPE *d_csrRowPtr, const int *d_csrColIdx, const MAT_VAL_TYPE *d_csrVal, MAT_VAL_TYPE *d_out, int invert, void *stream);

/* ---- Several right-hand sides at once: conjugate gradients on nvec systems A x_j = b_j in lock-step around tilespmv_plan_spmm (new).  The
 * matrix is streamed ONCE per iteration for all nvec systems.  This is plain CG per column — one rho, p.Ap, alpha, beta, |r|^2, |b|^2, iteration count and breakdown flag per
 * column — not block CG: no Gram matrices, no rank-deficiency breakdowns.  Per column the meaning is that of tilespmv_cg_*, word for word: the same recurrences, sums and scalars
 * in double, alpha and beta rounded to the value type once, the same guards taken on the device (rho = 0 -> alpha = beta = 0; rho < 0, or rho > 0 without p.Ap > 0 -> that column's
 * breakdown flag, the column keeps its last good x).  A column in breakdown or at rho = 0 does not disturb the others.
 * d_B and d_X are DEVICE arrays, row-major [rows][nvec] (the nvec values of one row are contiguous: the layout of tilespmv_plan_spmm) and 16-byte aligned; nvec in {1, 2, 4, 8};
 * d_dinv (may be NULL) has `rows` elements and is shared by all columns.  Nothing behind element rows * nvec - 1 of d_B / d_X or rows - 1 of d_dinv is read or written.
 * One iteration = the multi-vector product and THREE streaming kernels over the flat arrays: 11 * rows * nvec vector elements read or written beside the product (+ 2 * rows with
 * Jacobi).  One partial sum per workgroup and column; the consuming kernel folds them itself, every workgroup in the same order.  The number of partials and the order of every
 * addition are fixed by (rows, nvec) alone: on a plan whose tilespmv_plan_spmm is bit-reproducible the iterates are too, and a column's iterates do not depend on what the other
 * columns hold.  Workspace: r, p, Ap of (rows + 16) * nvec elements each, the partial sums and one scalar block per column, in one hipMalloc.  Measured against nvec successive
 * tilespmv_cg solves on the same plan in profiles/cg_multi_ab.txt (1.1 x to 2.2 x per system-iteration at nvec 8).
 *
 *   tilespmv_cg_multi_create      as tilespmv_cg_create (square, whole plan that outlives the solver; d_dinv borrowed), for nvec right-hand sides.  Also calls
 *                                 tilespmv_plan_reserve_spmm(plan, nvec), so that plans without a native multi-vector kernel never allocate inside iterate.  Returns 0,
 *                                 hipErrorInvalidValue (NULL argument or nvec outside {1, 2, 4, 8}: no HIP call made, the plan not touched; non-square / shard plan, misaligned
 *                                 d_dinv: nothing allocated), or the allocation's error.
 *   tilespmv_cg_multi_begin       R = B - A X, P = Z, the scalars of every column; iteration counts, breakdown and freeze flags cleared.
 *   tilespmv_cg_multi_iterate     `count` iterations of all columns back to back.  Like begin: asynchronous on `stream`, no allocation, no synchronisation, no host read, one linear
 *                                 chain of kernels — safe to capture into a hipGraph, for every kind of plan.  It stops at no tolerance.
 *   tilespmv_cg_multi_state_read  synchronises `stream` and fills out[0 .. nvec - 1]; set out[0].size first: it is the distance in bytes between the elements of `out`, and the size
 *                                 of each (tilespmv_cg_state_read's rule).  status per column: BREAKDOWN, CONVERGED when |r|^2 is exactly 0, else RUNNING.
 *   tilespmv_cg_multi_solve       begin, then iterate(check_every) + state_read.  A column seen at rr <= rtol^2 bb (CONVERGED), in breakdown (BREAKDOWN) or with bb = 0 (x_j = 0,
 *                                 CONVERGED, 0 iterations) is FROZEN: a flag on the device, set by a one-workgroup kernel, makes alpha = beta = 0 for it and stops its iteration
 *                                 count; its x and r do not change by a bit from then on, so relative residual <= rtol holds for every CONVERGED column at return although CG's
 *                                 residual norm is not monotone.  Frozen columns STILL RIDE THROUGH THE PRODUCT: an iteration costs the same until the last column is done.  Ends
 *                                 when every column is final or the running columns have done `maxiter` iterations (those: MAXITER; the last block is cut so that no more run).
 *                                 out[j].iterations is the count at which column j was frozen.  One host synchronisation per check.
 * nvec = 1 is served by tilespmv_cg_* itself: bit-identical x and state.  All but destroy return a hipError_t value (0 = success). */
typedef struct tilespmv_cg_multi tilespmv_cg_multi;
int tilespmv_cg_multi_create(tilespmv_cg_multi **cg, tilespmv_plan *plan, int nvec, const MAT_VAL_TYPE *d_dinv /* may be NULL; rows elements, shared by all columns */);
void tilespmv_cg_multi_destroy(tilespmv_cg_multi *cg);
int tilespmv_cg_multi_begin(tilespmv_cg_multi *cg, const MAT_VAL_TYPE *d_B, MAT_VAL_TYPE *d_X, void *stream);
int tilespmv_cg_multi_iterate(tilespmv_cg_multi *cg, MAT_VAL_TYPE *d_X, int count, void *stream);
int tilespmv_cg_multi_state_read(tilespmv_cg_multi *cg, void *stream, tilespmv_cg_state *out /* [nvec]; out[0].size set, it is the stride */);
int tilespmv_cg_multi_solve(tilespmv_cg_multi *cg, const MAT_VAL_TYPE *d_B, MAT_VAL_TYPE *d_X, double rtol, int maxiter, int check_every, void *stream,
                            tilespmv_cg_state *out /* [nvec] */);

/* ---- Least squares in the library: CGLS around the resident plans of A and A^T (new).  min |A x - b|^2 + damp^2 |x|^2 for a rows x cols
 * matrix A of any shape and rank: conjugate gradients on (A^T A + damp^2 I) x = A^T b, never forming A^T A, optionally preconditioned by a positive diagonal z = cinv o s (with
 * cinv_j = 1 / |a_j|^2 this is Jacobi on the normal equations: column scaling).  From x0 = 0 and damp = 0 an underdetermined system converges to the minimum-norm solution.
 * r, q have `rows` elements, p, s have `cols`, all in the value type; gamma = s.z, delta = q.q + damp^2 p.p, nn = s.s and rr = r.r are accumulated in double.
 *   begin     r = b - A x;  s = A^T r - damp^2 x;  p = z;  gamma, nn, rr, bb = b.b;  nn0 = |A^T b|^2 (one more A^T product);  iteration count and breakdown flag cleared
 *   iterate   q = A p;  alpha = gamma / delta;  x += alpha p;  r -= alpha q;  s = A^T r - damp^2 x;  z = cinv o s;  gamma' = s.z;  beta = gamma' / gamma;  p = z + beta p
 * alpha, beta and damp^2 are formed in double and rounded to the value type once, where they multiply (the rule of tilespmv_cg_*).
 * One iteration = the two plan products and FOUR streaming kernels (q.q (+ p.p);  the update of x and r with r.r;  the normal pass over s;  the direction).  Every scalar lives in
 * device memory with one writing kernel per field; a reducing kernel leaves one partial per workgroup and the consuming kernel folds them itself, every workgroup in the same order: no
 * atomics, no finishing launch, no host read.  The number of partials depends on `rows` for row-length sums and on `cols` for column-length sums and on nothing else: where both plans
 * give a bit-reproducible y (TILESPMV_INFO_ENTRY_ORDERED = 1, e.g. deterministic = 1) the iterates x_k are bit-reproducible too.
 * Vector elements read or written per iteration beside the two products, by count: 4 rows + 7 cols with damp = 0 and d_cinv = NULL (then nothing extra is touched: no x read in the
 * normal pass, no store of s, z never stored); damping adds 3 cols, d_cinv adds 2 cols.  The torch loop it replaces moves 7 rows + 12 cols in about a dozen launches; measured in
 * profiles/cgls_fused_ab.txt.
 * Guards, taken on the device, with the meaning of the CG guards: gamma = 0 -> alpha = beta = 0, x and r no longer change — a captured graph of k iterations may overrun
 * convergence; gamma < 0 (a cinv that is not positive), or gamma > 0 without delta > 0 -> the breakdown flag is set, alpha = beta = 0 from then on, x keeps its last good value.
 * d_b (rows), d_x (cols) and d_cinv (cols) are DEVICE vectors, 16-byte aligned (hipErrorInvalidValue otherwise); nothing behind their last element is read or written.
 *
 *   tilespmv_cgls_create      plan_A: whole (tilerow_begin = 0, tilerow_end = tilem), rows x cols; plan_AT: whole, cols x rows — a TILESPMV_CREATE_TRANSPOSE plan or any plan of the
 *                             transposed CSR.  Both are borrowed and must outlive the solver.  d_cinv: NULL, or cols elements, borrowed; its VALUES may change between solves.  One
 *                             hipMalloc holds r, q (rows + 16 elements each), p, s (cols + 16 each), the partial-sum arrays and the scalar block.  Returns 0, hipErrorInvalidValue
 *                             (a NULL argument: no HIP call made; shapes that do not match, a shard plan, a misaligned d_cinv: nothing allocated), or the allocation's error.
 *   tilespmv_cgls_begin       as above, from the caller's x (pass zeros for none).  `damp` holds for the tilespmv_cgls_iterate calls that follow (it is kept on the device).
 *   tilespmv_cgls_iterate     `count` iterations back to back.  Like begin: asynchronous on `stream`, no allocation, no synchronisation, no host read, one linear chain of kernels —
 *                             safe to capture into a hipGraph.  It stops at no tolerance.  Both plans and the solver run on ONE stream at a time.
 *   tilespmv_cgls_state_read  synchronises `stream` and fills the state (set out->size = sizeof(tilespmv_cgls_state) first; a shorter struct gets the fields it knows).  status (the
 *                             TILESPMV_CG_* values): BREAKDOWN, CONVERGED when nn is exactly 0, else RUNNING.  nn = the squared norm of the UNPRECONDITIONED normal residual
 *                             A^T r - damp^2 x; rr = the recurrence's |r|^2, not a recomputed |b - A x|^2.
 *   tilespmv_cgls_solve       begin, then iterate(check_every) + state_read until nn <= rtol^2 nn0 (CONVERGED: |A^T r| <= rtol |A^T b|), `maxiter` iterations are done (MAXITER; the
 *                             last block is cut so that no more run) or a breakdown (BREAKDOWN).  nn0 = 0 (b = 0, or b orthogonal to the range of A) -> x = 0, CONVERGED, 0
 *                             iterations.  check_every < 1 -> 1.  One host synchronisation per check.
 * All but destroy return a hipError_t value (0 = success). */
typedef struct tilespmv_cgls tilespmv_cgls;
typedef struct { unsigned size; int iterations; int status; double nn; double nn0; double rr; double bb; } tilespmv_cgls_state;
int tilespmv_cgls_create(tilespmv_cgls **ls, tilespmv_plan *plan_A, tilespmv_plan *plan_AT, const MAT_VAL_TYPE *d_cinv /* may be NULL; cols elements */);
void tilespmv_cgls_destroy(tilespmv_cgls *ls);
int tilespmv_cgls_begin(tilespmv_cgls *ls, const MAT_VAL_TYPE *d_b, MAT_VAL_TYPE *d_x, double damp, void *stream);
int tilespmv_cgls_iterate(tilespmv_cgls *ls, MAT_VAL_TYPE *d_x, int count, void *stream);
int tilespmv_cgls_state_read(tilespmv_cgls *ls, void *stream, tilespmv_cgls_state *out);
int tilespmv_cgls_solve(tilespmv_cgls *ls, const MAT_VAL_TYPE *d_b, MAT_VAL_TYPE *d_x, double damp, double rtol, int maxiter, int check_every, void *stream,
                        tilespmv_cgls_state *out);
/* d_out[i] = the sum over k in [d_rowPtr[i], d_rowPtr[i + 1]) of v(k)^2, v(k) = d_val[d_src ? d_src[k] : k], i < rows: sums in double, in storage order, one thread per row.
 * invert != 0: 1 / that, and 1 where it is 0 (an empty column of a wide matrix makes no Inf) — the d_cinv of tilespmv_cgls_create.
 * Intended use, column scaling that follows the matrix values: transpose the PATTERN once with tilespmv_csr_transpose_device and keep rpT and srcT; after every
 * tilespmv_plan_update_values call this with d_rowPtr = rpT, d_src = srcT and d_val = A's own value array: row j of A^T read through srcT is column j of A, so d_out[j] = 1 / |a_j|^2
 * without a second sort, and in an order fixed by the pattern.  Asynchronous on `stream`, capturable.  Returns a hipError_t value (hipErrorInvalidValue for a NULL array other than
 * d_src, hipErrorNoDevice without a device). */
int tilespmv_csr_row_sqnorms_device(int rows, const MAT_PTR_TYPE *d_rowPtr, const int *d_src /* may be NULL */, const MAT_VAL_TYPE *d_val, MAT_VAL_TYPE *d_out, int invert,
                                    void *stream);

/* ---- Nonsymmetric systems in the library: BiCGStab around a resident plan (new).  A x = b for a square A that need be neither symmetric nor
 * definite, right-preconditioned by M^-1 = diag(d_dinv) (Jacobi: tilespmv_csr_diagonal_device(..., invert = 1) makes it; d_dinv = NULL: phat = p, shat = s).  The contract is that
 * of tilespmv_cg_*, word for word, wherever it can be; the state is tilespmv_cg_state and the statuses are TILESPMV_CG_*.
 *   begin     r = b - A x;  rhat = r;  p = r;  rho = rhat.r;  rr = r.r;  bb = b.b;  iteration count and breakdown flag cleared
 *   iterate   phat = dinv o p;  v = A phat;  sigma = rhat.v;  alpha = rho / sigma;  s = r - alpha v;  shat = dinv o s;  t = A shat;  omega = (t.s) / (t.t);
 *             x += alpha phat + omega shat;  r = s - omega t;  rho' = rhat.r, rr = r.r;  beta = (rho' / rho)(alpha / omega);  p = r + beta (p - omega v)
 * All vectors live in the value type; every dot product and every scalar is double in both libraries; alpha, omega and beta are formed in double and rounded to the value type
 * once, where they multiply (the rule of tilespmv_cg_*).
 * One iteration = the two plan products and FIVE streaming kernels (rhat.v;  the half step s, stored over r;  t.s and t.t;  the update of x and r with r.r and rhat.r;  the
 * direction).  Every scalar lives in device memory with one writing kernel per field; a reducing kernel leaves one partial per workgroup and the consuming kernel folds them itself,
 * every workgroup in the same order: no atomics, no finishing launch, no host read.  The number of partials depends on `rows` alone: on a plan whose y is bit-reproducible
 * (TILESPMV_INFO_ENTRY_ORDERED = 1, e.g. deterministic = 1) the iterates x_k are too, run after run and plan after plan.
 * Vector elements read or written per iteration beside the two products, by count: 18 per row (2 + 3 + 2 + 7 + 4 over the five kernels), 23 per row with Jacobi (d_dinv read and
 * shat stored in the half step, shat read in the update, d_dinv read and phat stored in the direction).  The loop of torch operations it replaces
 * (tilespmv_amd.operator.bicgstab) moves 28 per row (34 with Jacobi) in about twenty launches (scripts/bicgstab_time.py measures both).  Workspace: 5 vectors of rows + 16 elements (r, rhat, p, v, t;
 * s lives in r), 7 with Jacobi (phat, shat), and 49 KB of partial sums and scalars, in one hipMalloc.
 * Guards, taken on the device, exact-zero tests only, in the style of the CG guards:
 *   rr = 0 at the start of an iteration, or the breakdown flag set   alpha = omega = beta = 0: the iteration writes no vector, x, r and p do not change by a bit — a captured
 *                                                                    graph of k iterations may overrun convergence.
 *   rr > 0, and rho = 0 or sigma = 0                                 the breakdown flag is set; alpha = omega = beta = 0 in that and every later iteration, x keeps its last good value.
 *   t.t = 0 (or t.s = 0: omega would be 0 all the same)              omega = 0:  x += alpha phat,  r = s,  p is left as it is.  If rr is then 0 this is convergence at the half step
 *                                                                    (A = 2 I ends this way after one iteration); if rr > 0 the breakdown flag is set (omega = 0 with a live residual).
 *   The iteration counter advances in every iteration whatever the guards did: a breakdown seen at the first check of solve(check_every = 8) reports 8 iterations.
 * A tilespmv_bicgstab and its plan run on ONE stream at a time.  d_b, d_x and d_dinv are DEVICE vectors of `rows` elements, 16-byte aligned (hipErrorInvalidValue otherwise);
 * nothing behind element rows - 1 is read or written.
 *
 *   tilespmv_bicgstab_create      binds a workspace to `plan`, which must be square and whole (tilerow_begin = 0, tilerow_end = tilem; a square TILESPMV_CREATE_TRANSPOSE plan
 *                                 qualifies: it solves A^T x = b) and must outlive it; the plan is borrowed.  d_dinv: NULL, or the inverse diagonal, borrowed until destroy — its VALUES
 *                                 may change between solves (tilespmv_plan_update_values, then tilespmv_csr_diagonal_device into the same array).  One hipMalloc (synchronises).
 *                                 Returns 0, hipErrorInvalidValue (a NULL argument: no HIP call made; a non-square or shard plan, a misaligned d_dinv: nothing allocated), or the
 *                                 hipMalloc error.
 *   tilespmv_bicgstab_begin       as above, from the caller's x (pass zeros for none).
 *   tilespmv_bicgstab_iterate     `count` iterations back to back.  Like begin: asynchronous on `stream`, no allocation, no synchronisation, no host read, one linear chain of
 *                                 kernels — safe to capture into a hipGraph, for every kind of plan.  It stops at no tolerance.
 *   tilespmv_bicgstab_state_read  synchronises `stream` and fills the state (set out->size = sizeof(tilespmv_cg_state) first).  status: BREAKDOWN, else CONVERGED when rr is exactly
 *                                 0, else RUNNING.  rr is the recurrence's |r|^2, not a recomputed |b - A x|^2; BiCGStab's residual norm is not monotone.
 *   tilespmv_bicgstab_solve       begin, then iterate(check_every) + state_read until sqrt(rr / bb) <= rtol (CONVERGED), `maxiter` iterations are done (MAXITER; the last block is cut
 *                                 so that no more run) or a breakdown (BREAKDOWN).  bb = 0 -> x = 0, CONVERGED, 0 iterations.  check_every < 1 -> 1.  One host synchronisation per
 *                                 check; the residual is not looked at at the half step.
 * All but destroy return a hipError_t value (0 = success). */
typedef struct tilespmv_bicgstab tilespmv_bicgstab;
int tilespmv_bicgstab_create(tilespmv_bicgstab **s, tilespmv_plan *plan, const MAT_VAL_TYPE *d_dinv /* may be NULL */);
void tilespmv_bicgstab_destroy(tilespmv_bicgstab *s);
int tilespmv_bicgstab_begin(tilespmv_bicgstab *s, const MAT_VAL_TYPE *d_b, MAT_VAL_TYPE *d_x, void *stream);
int tilespmv_bicgstab_iterate(tilespmv_bicgstab *s, MAT_VAL_TYPE *d_x, int count, void *stream);
int tilespmv_bicgstab_state_read(tilespmv_bicgstab *s, void *stream, tilespmv_cg_state *out);
int tilespmv_bicgstab_solve(tilespmv_bicgstab *s, const MAT_VAL_TYPE *d_b, MAT_VAL_TYPE *d_x, double rtol, int maxiter, int check_every, void *stream,
                            tilespmv_cg_state *out);

/* ---- Symmetric indefinite systems in the library: MINRES around a resident plan (new).  A x = b for a square SYMMETRIC A that need not be
 * definite (saddle-point and KKT systems, on which CG breaks down), preconditioned by a POSITIVE diagonal M^-1 = diag(d_minv) (tilespmv_csr_abs_diagonal_device(..., invert = 1)
 * makes one; d_minv = NULL: z = r2).  Preconditioned Paige-Saunders MINRES: one product per iteration, short recurrences, a residual norm that never increases, and no breakdown
 * but the lucky one.  The contract is that of tilespmv_bicgstab_*, word for word, wherever it can be; the state is tilespmv_cg_state and the statuses are TILESPMV_CG_*.
 *   begin     r2 = b - A x;  r1 = 0;  z = minv o r2;  beta = sqrt(r2.z);  bb = b.(minv o b);  oldb = dbar = epsln = 0;  phibar = beta;  cs = -1;  sn = 0;  w = w2 = 0;
 *             rr = r2.z (= phibar^2; the sum itself, no square root in between);  iteration count and breakdown flag cleared
 *   iterate   v = z / beta;  y = A v;  if oldb != 0: y -= (beta/oldb) r1;  alfa = v.y;  y -= (alfa/beta) r2;  z' = minv o y;  beta' = sqrt(y.z');
 *             oldeps = epsln;  delta = cs dbar + sn alfa;  gbar = sn dbar - cs alfa;  gamma = hypot(gbar, beta');
 *             r1 = r2;  r2 = y;  z = z';  oldb = beta;  beta = beta';  epsln = sn beta;  dbar = -cs beta;  cs = gbar/gamma;  sn = beta/gamma;  phi = cs phibar;  phibar = sn phibar;
 *             w1 = w2;  w2 = w;  w = (v - oldeps w1 - delta w2) / gamma;  x += phi w;  rr = phibar^2
 * All vectors live in the value type; every dot product and every scalar is double in both libraries; 1/beta, alfa/beta, beta/oldb, oldeps, delta, 1/gamma and phi are formed in
 * double and rounded to the value type once, where they multiply (the rule of tilespmv_cg_*).  The library keeps z, not v: the product is taken of z and every consumer multiplies
 * by the rounded 1/beta (y = (A z) / beta).
 * WHAT rr AND bb ARE: without d_minv, rr is the recurrence's |r|^2 and bb is |b|^2; with d_minv, rr is r.M^-1 r and bb is b.M^-1 b — the norm MINRES minimises, and the one
 * tilespmv_minres_solve's rtol applies to.  rr is never a recomputed |b - A x|^2.
 * One iteration = the plan product and THREE streaming kernels (v.y;  the Lanczos step with the partial sums of beta'^2;  the rotation with the update of w, x and z).  Every
 * scalar lives in device memory with one writing kernel per field; a reducing kernel leaves one partial per workgroup and the consuming kernel folds them itself, every workgroup in
 * the same order: no atomics, no finishing launch, no host read.  The number of partials depends on `rows` alone: on a plan whose y is bit-reproducible
 * (TILESPMV_INFO_ENTRY_ORDERED = 1, e.g. deterministic = 1) the iterates x_k are too, run after run and plan after plan.  The three-term history (r1 / r2, w / w2) is kept without
 * copies and without exchanging pointers on the host: the kernels choose the roles of two buffers from the parity of the iteration counter on the DEVICE, so a captured
 * iterate(k) may be replayed any number of times.
 * Vector elements read or written per iteration beside the product, by count: 14 per row (2 + 4 + 8 over the three kernels), 16 per row with d_minv (read in the Lanczos step and
 * in the update; z' is recomputed there, not stored and read back).  The loop of torch operations it replaces (tilespmv_amd.operator.minres, its scalars 0-d tensors on the device) moves
 * 23 per row (26 with d_minv) in about thirty-five launches.  Measured, seconds per iteration against that loop on the same plan (scripts/minres_time.py,
 * profiles/minres_fused_ab.txt): 0.631 -> 0.441 ms = 1.43 x on the 4096^2 Laplacian shifted by -I in fp64, 0.403 -> 0.254 ms = 1.59 x in fp32, 7.6 x on a launch-bound 512^2 grid.
 * Workspace: 6 vectors of rows + 16 elements (y, z, two of r, two of w), with or without d_minv, and 16.25 KB of partial sums and scalars, in one hipMalloc.
 * Guards, taken on the device, exact tests only, in the style of the CG guards:
 *   phibar = 0 at the start of an iteration, or the breakdown flag set   the iteration writes no vector, x does not change by a bit (b = 0; beta' = 0, the lucky termination) — a
 *                                                                        captured graph of k iterations may overrun convergence.
 *   r2.z < 0 (begin) or y.z' < 0                                         M is not positive definite: the breakdown flag is set; that and every later iteration leave x alone, x
 *                                                                        keeps its last good value (in begin: the caller's x0).
 *   gamma = 0                                                            A is singular on this Krylov space and the system incompatible: breakdown, handled the same way.
 *   The iteration counter advances in every iteration whatever the guards did: a breakdown seen at the first check of solve(check_every = 8) reports 8 iterations.
 * A tilespmv_minres and its plan run on ONE stream at a time.  d_b, d_x and d_minv are DEVICE vectors of `rows` elements, 16-byte aligned (hipErrorInvalidValue otherwise);
 * nothing behind element rows - 1 is read or written.
 *
 *   tilespmv_minres_create      binds a workspace to `plan`, which must be square and whole (tilerow_begin = 0, tilerow_end = tilem; a square TILESPMV_CREATE_TRANSPOSE plan
 *                               qualifies) and must outlive it; the plan is borrowed.  That A is symmetric is the caller's word: it is not checked.  d_minv: NULL, or a positive
 *                               diagonal, borrowed until destroy — its VALUES may change between solves (tilespmv_plan_update_values, then tilespmv_csr_abs_diagonal_device into the
 *                               same array).  One hipMalloc (synchronises).  Returns 0, hipErrorInvalidValue (a NULL argument: no HIP call made; a non-square or shard plan, a
 *                               misaligned d_minv: nothing allocated), or the hipMalloc error.
 *   tilespmv_minres_begin       as above, from the caller's x (pass zeros for none).
 *   tilespmv_minres_iterate     `count` iterations back to back.  Like begin: asynchronous on `stream`, no allocation, no synchronisation, no host read, one linear chain of
 *                               kernels — safe to capture into a hipGraph, for every kind of plan.  It stops at no tolerance.
 *   tilespmv_minres_state_read  synchronises `stream` and fills the state (set out->size = sizeof(tilespmv_cg_state) first).  status: BREAKDOWN, else CONVERGED when rr is exactly
 *                               0, else RUNNING.
 *   tilespmv_minres_solve       begin, then iterate(check_every) + state_read until rr <= rtol^2 bb (CONVERGED), `maxiter` iterations are done (MAXITER; the last block is cut so
 *                               that no more run) or a breakdown (BREAKDOWN).  bb = 0 -> x = 0, CONVERGED, 0 iterations.  check_every < 1 -> 1.  One host synchronisation per check.
 * All but destroy return a hipError_t value (0 = success). */
typedef struct tilespmv_minres tilespmv_minres;
int tilespmv_minres_create(tilespmv_minres **s, tilespmv_plan *plan, const MAT_VAL_TYPE *d_minv /* may be NULL */);
void tilespmv_minres_destroy(tilespmv_minres *s);
int tilespmv_minres_begin(tilespmv_minres *s, const MAT_VAL_TYPE *d_b, MAT_VAL_TYPE *d_x, void *stream);
int tilespmv_minres_iterate(tilespmv_minres *s, MAT_VAL_TYPE *d_x, int count, void *stream);
int tilespmv_minres_state_read(tilespmv_minres *s, void *stream, tilespmv_cg_state *out);
int tilespmv_minres_solve(tilespmv_minres *s, const MAT_VAL_TYPE *d_b, MAT_VAL_TYPE *d_x, double rtol, int maxiter, int check_every, void *stream,
                          tilespmv_cg_state *out);
/* tilespmv_csr_diagonal_device with one difference: d_out[i] = the ABSOLUTE VALUE of the sum of the stored entries (i, i); invert != 0: 1 / |d|, and 1 where d is 0 — a positive
 * d_minv for tilespmv_minres_create whatever the signs on the diagonal (a KKT matrix with a negative or zero (2,2) block).  One thread per row, asynchronous on `stream`,
 * capturable.  Returns a hipError_t value (hipErrorInvalidValue for a NULL array, hipErrorNoDevice without a device). */
int tilespmv_csr_abs_diagonal_device(int rows, const MAT_PTR_TYPE *d_csrRowPtr, const int *d_csrColIdx, const MAT_VAL_TYPE *d_csrVal, MAT_VAL_TYPE *d_out, int invert,
                                     void *stream);

/* ---- A block-Jacobi preconditioner for tilespmv_cg_* and tilespmv_bicgstab_* (new).  M is the block diagonal of A for CONSECUTIVE blocks of
 * block_size rows: block k covers rows and columns [k bs, min((k + 1) bs, rows)), 1 <= bs <= 16, the last block short when rows % bs != 0 — one block per node of a structural FEM
 * matrix with bs unknowns per node, where a point diagonal is the wrong tool.  The object holds M^-1 in device memory in the value type.
 *
 * Layout of M^-1, plane-major: plane j (j < bs) is a vector of `rows` elements padded to a multiple of 256 bytes; plane_j[i] = (M^-1)[i][blockstart(i) + j], 0 where the block is
 * short — every plane is walked like a solver vector, with 16-byte lane accesses.  z = M^-1 r reads r once (a workgroup stages the slab of r its rows' blocks cover in LDS), every
 * plane once, and writes z once: bs + 2 elements per row; z_i = sum_j plane_j[i] r[blockstart(i) + j] with j ascending, accumulated in double, rounded to the value type once.
 *
 *   tilespmv_block_jacobi_create   one hipMalloc (the bs planes and a device counter; synchronises).  hipErrorInvalidValue, without any HIP call, for a NULL bj, rows <= 0 or
 *                                  block_size outside 1 .. 16.  Until the first update M^-1 is 0.
 *   tilespmv_block_jacobi_update   extracts the blocks from a DEVICE CSR (the row pointer is used as it stands; duplicates are added in storage order, in double; columns may be
 *                                  unsorted) and inverts them on the device: Gauss-Jordan with partial pivoting, in double in both builds, ties broken by the lowest row, the result
 *                                  rounded to the value type once — a function of the block's values alone, so two updates from the same values give the same bytes.  A block whose
 *                                  pivot is exactly 0 or not finite at any step gets the IDENTITY as its inverse and is counted (info).  Asynchronous on `stream`; no allocation,
 *                                  no synchronisation, no host read: capturable into a hipGraph; after every tilespmv_plan_update_values it is the same call into the same object.
 *   tilespmv_block_jacobi_apply    z = M^-1 r; d_r and d_z are distinct device vectors of `rows` elements, 16-byte aligned (hipErrorInvalidValue otherwise); nothing behind element
 *                                  rows - 1 of either is touched.  Asynchronous, capturable.
 *   tilespmv_block_jacobi_apply_dot  the same, and d_partials[w] = the sum over workgroup w's rows of r_i z_i (double; info's dot_partials of them, at most
 *                                  TILESPMV_BJ_MAX_PARTIALS: their number and the order of every addition are fixed by `rows` alone) — what the CG below folds into r.z.
 *   tilespmv_block_jacobi_info     synchronises `stream`; out[TILESPMV_BJ_INFO_*].
 *
 * Solvers that take the object: tilespmv_cg_create_block and tilespmv_bicgstab_create_block return the EXISTING solver types; begin, iterate, state_read, solve and destroy are the
 * entry points above.  bj is borrowed until destroy and its values may change between solves; its rows must be the plan's (hipErrorInvalidValue otherwise, nothing allocated).
 *   CG        z becomes a stored vector (4 work vectors).  One iteration: the product, k_cg_dot, k_cg_update (r.r partials), apply_dot r -> z (r.z partials), and p = z + beta p:
 *             four launches beside the product, 13 + bs vector elements per row BY COUNT (13 with point Jacobi).
 *   BiCGStab  phat = M^-1 p and shat = M^-1 s by two applies per iteration (7 work vectors): 18 + 2 (bs + 2) elements per row by count (23 with point Jacobi).
 *   GMRES     tilespmv_gmres_create_block, below: one apply per inner iteration and one in every close.
 * Out of scope: MINRES (it needs a positive definite M, and the diagonal blocks of an indefinite matrix are not), multi-RHS CG (the apply would need the row-major [rows][nvec]
 * layout) and CGLS.  All but destroy return a hipError_t value (0 = success). */
typedef struct tilespmv_block_jacobi tilespmv_block_jacobi;
enum {
    TILESPMV_BJ_INFO_ROWS = 0, TILESPMV_BJ_INFO_BLOCK_SIZE = 1, TILESPMV_BJ_INFO_BLOCKS = 2,
    TILESPMV_BJ_INFO_SINGULAR_BLOCKS = 3,   /* blocks the last update replaced by the identity */
    TILESPMV_BJ_INFO_DEVICE_BYTES = 4, TILESPMV_BJ_INFO_DOT_PARTIALS = 5,
    TILESPMV_BJ_INFO_COUNT = 6
};
#define TILESPMV_BJ_MAX_PARTIALS 1024
int tilespmv_block_jacobi_create(tilespmv_block_jacobi **bj, int rows, int block_size);
void tilespmv_block_jacobi_destroy(tilespmv_block_jacobi *bj);
int tilespmv_block_jacobi_update(tilespmv_block_jacobi *bj, const MAT_PTR_TYPE *d_csrRowPtr, const int *d_csrColIdx, const MAT_VAL_TYPE *d_csrVal, void *stream);
int tilespmv_block_jacobi_apply(const tilespmv_block_jacobi *bj, const MAT_VAL_TYPE *d_r, MAT_VAL_TYPE *d_z, void *stream);   /* z = M^-1 r, z != r */
int tilespmv_block_jacobi_apply_dot(const tilespmv_block_jacobi *bj, const MAT_VAL_TYPE *d_r, MAT_VAL_TYPE *d_z, double *d_partials, void *stream);
int tilespmv_block_jacobi_info(const tilespmv_block_jacobi *bj, void *stream, long long *out /* [TILESPMV_BJ_INFO_COUNT] */);
int tilespmv_cg_create_block(tilespmv_cg **cg, tilespmv_plan *plan, const tilespmv_block_jacobi *bj);
int tilespmv_bicgstab_create_block(tilespmv_bicgstab **s, tilespmv_plan *plan, const tilespmv_block_jacobi *bj);

/* ---- A factorised sparse approximate inverse (FSAI) preconditioner for tilespmv_cg_* (new): for symmetric positive definite systems whose
 * difficulty is not inside a row (the inverse diagonal) or a node (block Jacobi).  G is sparse and LOWER TRIANGULAR with G A G^T ~ I (Kolotilina-Yeremin); the preconditioner is
 * M^-1 = G^T G, positive definite whatever A is, and applying it is two sparse products — a plan of G and a transposed plan of G, both held by the object.
 *
 * Input: a square CSR in DEVICE memory whose rows hold strictly ascending columns (hence no repeated entries) and every one of which stores its diagonal.  Only entries with
 * column <= row are ever read: the object is well defined for any such input and is the FSAI of the symmetric matrix whose lower triangle that is.
 * Pattern: row i of G holds the stored columns <= i of row i of A; where there are more than TILESPMV_FSAI_MAX_ROW of them, the TILESPMV_FSAI_MAX_ROW largest — those nearest the
 * diagonal, the diagonal among them (such rows are counted: truncated_rows).
 * Values: with P the m pattern columns of row i, S = A[P, P] and S y = e_m, row i of G is y / sqrt(y_m): row i of G A G^T has a unit diagonal.  S is assembled and factorised
 * (Cholesky) in double in both builds, one group of lanes per row, and the row is rounded to the value type once; every sum has a fixed order and no value is added by an atomic:
 * two runs give the same bytes.  A row whose factorisation meets a pivot that is not > 0 or not finite FALLS BACK to point Jacobi: zeros, with 1 / sqrt(a_ii) on the diagonal
 * where a_ii > 0 and 1 otherwise (counted: fallback_rows, rewritten by every update).
 *
 *   tilespmv_fsai_create     checks the input with one kernel (hipErrorInvalidValue and nothing built where it does not hold, or for a NULL argument, rows <= 0, nnz <= 0), builds
 *                            the pattern (a count, a scan, a fill), the values, and the two plans by tilespmv_plan_create_from_device_csr with TILESPMV_CREATE_VALUE_MAP (and
 *                            TILESPMV_CREATE_TRANSPOSE for the second); `opts` (may be NULL: the defaults) goes to both.  Allocates and synchronises.  Other return codes: a
 *                            hipError_t value, or the negative code of the plan builder.
 *   tilespmv_fsai_update     new values of A on the SAME pattern (the caller's promise, as for tilespmv_plan_update_values): the value kernel into the same array of G's values,
 *                            then tilespmv_plan_update_values on both plans.  Asynchronous on `stream`; no allocation, no host copy, no synchronisation: capturable into a hipGraph.
 *                            The object then holds the bytes a fresh create from those values holds.
 *   tilespmv_fsai_apply      z = G^T (G r): two tilespmv_plan_spmv calls, t = G r in a vector the object owns.  d_r and d_z are distinct device vectors of `rows` elements, 16-byte
 *                            aligned (hipErrorInvalidValue otherwise, and nothing is launched); nothing behind element rows - 1 of either is touched.  Asynchronous, capturable.
 *   tilespmv_fsai_apply_dot  the same, and d_partials[w] = partial sum w of r.z (double; info's dot_partials of them, at most TILESPMV_FSAI_MAX_PARTIALS: their number and the order
 *                            of every addition are fixed by `rows` alone) in one more streaming pass — r.z itself, not |t|^2.
 *   tilespmv_fsai_factor_csr G as a device CSR, BORROWED until destroy (row pointer of rows + 1, column indices and values of *nnz entries; the values change with every update).
 *   tilespmv_fsai_info       synchronises `stream`; out[TILESPMV_FSAI_INFO_*].
 *   tilespmv_cg_create_fsai  the EXISTING solver type; begin, iterate, state_read, solve and destroy are the entry points of tilespmv_cg_*.  f is borrowed until destroy and its values
 *                            may change between solves; hipErrorInvalidValue (nothing allocated) for a NULL f or one whose rows are not the plan's.  z is a stored vector, as with
 *                            block Jacobi.  One iteration: the product, the two products of G, and four launches (k_cg_dot, k_cg_update, the r.z partials, p = z + beta p).
 * The object and its two plans run on ONE stream at a time (the single-stream rule of tilespmv_plan_spmv).  Out of scope: larger patterns, dropping, the nonsymmetric two-factor
 * form, multi-RHS CG.  All but destroy return a hipError_t value unless said otherwise (0 = success). */
typedef struct tilespmv_fsai tilespmv_fsai;
#define TILESPMV_FSAI_MAX_ROW 64
#define TILESPMV_FSAI_MAX_PARTIALS 1024
enum {
    TILESPMV_FSAI_INFO_ROWS = 0, TILESPMV_FSAI_INFO_NNZ = 1 /* of G */, TILESPMV_FSAI_INFO_LONGEST_ROW = 2 /* of G */,
    TILESPMV_FSAI_INFO_TRUNCATED_ROWS = 3,   /* rows of A with more than TILESPMV_FSAI_MAX_ROW stored columns <= the row */
    TILESPMV_FSAI_INFO_FALLBACK_ROWS = 4,    /* rows the last create or update replaced by point Jacobi */
    TILESPMV_FSAI_INFO_DEVICE_BYTES = 5 /* both plans and their value maps included */, TILESPMV_FSAI_INFO_DOT_PARTIALS = 6,
    TILESPMV_FSAI_INFO_COUNT = 7
};
int tilespmv_fsai_create(tilespmv_fsai **f, int rows, MAT_PTR_TYPE nnz, const MAT_PTR_TYPE *d_csrRowPtr, const int *d_csrColIdx, const MAT_VAL_TYPE *d_csrVal,
                         const tilespmv_plan_options *opts /* may be NULL */, void *stream);
void tilespmv_fsai_destroy(tilespmv_fsai *f);
int tilespmv_fsai_update(tilespmv_fsai *f, const MAT_PTR_TYPE *d_csrRowPtr, const int *d_csrColIdx, const MAT_VAL_TYPE *d_csrVal, void *stream);
int tilespmv_fsai_apply(tilespmv_fsai *f, const MAT_VAL_TYPE *d_r, MAT_VAL_TYPE *d_z, void *stream);   /* z = G^T (G r), z != r */
int tilespmv_fsai_apply_dot(tilespmv_fsai *f, const MAT_VAL_TYPE *d_r, MAT_VAL_TYPE *d_z, double *d_partials, void *stream);
int tilespmv_fsai_factor_csr(const tilespmv_fsai *f, const MAT_PTR_TYPE **d_rowPtr, const int **d_colIdx, const MAT_VAL_TYPE **d_val, MAT_PTR_TYPE *nnz);   /* G, borrowed */
int tilespmv_fsai_info(const tilespmv_fsai *f, void *stream, long long *out /* [TILESPMV_FSAI_INFO_COUNT] */);
int tilespmv_cg_create_fsai(tilespmv_cg **cg, tilespmv_plan *plan, tilespmv_fsai *f);

/* ---- Nonsymmetric systems that BiCGStab does not solve: restarted GMRES around a resident plan (new).  A x = b for a square A that need be
 * neither symmetric nor definite, by GMRES(m), m = restart <= TILESPMV_GMRES_MAX_RESTART, right-preconditioned by M^-1 = diag(d_dinv) (tilespmv_csr_diagonal_device(..., invert = 1)
 * makes it; d_dinv = NULL: M = I) or by a block-Jacobi object.  One product per iteration, a residual norm that never increases inside a cycle, no breakdown but the lucky one and
 * the singular one.  The contract is that of tilespmv_bicgstab_*, word for word, wherever it can be; the state is tilespmv_cg_state and the statuses are TILESPMV_CG_*.
 *   begin     the solver's copy of b (every restart needs it: d_b is not read after begin's work is done);  bb = b.b;  iteration count and breakdown flag cleared;  open a cycle
 *   open      r = b - A x (one plan product);  rr = r.r;  beta = sqrt(rr);  V_0 = r / beta;  g = beta e_0;  j = 0.  rr = 0 exactly: nothing is formed, the cycle is dead
 *   iterate   w = A (M^-1 V_j);  h1 = V_{0..j}^T w;  w' = w - V h1;  h2 = V^T w';  w'' = w' - V h2;  h_{j+1,j} = |w''|;  column j of H = (h1 + h2, h_{j+1,j});  the j stored Givens
 *             rotations applied to it;  gamma = hypot(h_jj, h_{j+1,j}), cs = h_jj / gamma, sn = h_{j+1,j} / gamma;  g_{j+1} = -sn g_j, g_j = cs g_j;  rr = g_{j+1}^2;
 *             V_{j+1} = w'' / h_{j+1,j};  j += 1.  After `restart` iterations in a cycle: close it and open the next
 *   close     after k columns: R y = g by back substitution (k x k, in double);  x += M^-1 (V_{0..k-1} y)
 * Classical Gram-Schmidt applied twice is deliberate: a pass needs all its dot products before it subtracts, so a pass is two streaming kernels whatever j is, where modified
 * Gram-Schmidt needs j + 1 dependent reductions; the second pass keeps the float library orthogonal.
 * All vectors live in the value type; every dot product, H, the rotations, g, y and every scalar is double in both libraries; h1_i, h2_i, 1 / h_{j+1,j}, 1 / beta and y_i are
 * rounded to the value type once, where they multiply a vector (the rule of tilespmv_cg_*).
 * WHAT rr IS, AND WHEN d_x IS CURRENT: D_X HOLDS THE ITERATE ONLY AFTER A CLOSE (the end of a cycle inside iterate, or flush); between closes it is the x of the last close.  Inside
 * a cycle rr is the recurrence's g_{j+1}^2, which with right preconditioning estimates the TRUE |b - A x|^2.  After an open (begin, a full cycle, flush) rr IS A RECOMPUTED
 * |b - A x|^2 of the x in d_x — this solver is the one place in the library where that holds.  bb is |b|^2.  `iterations` counts inner iterations; an open's product is not counted.
 * One inner iteration with k = j + 1 basis vectors = the plan product and FOUR streaming kernels (the k dot products h1;  w' with the k dot products h2 from the same walk;  w''
 * with |w''|^2;  V_{j+1} with the column, the rotations, g and rr).  A close is a one-workgroup back substitution and one kernel for x; an open is the product, the residual with
 * its norm, and the fourth kernel in its open role.  Every scalar lives in device memory with one writing kernel per field; a reducing kernel leaves one partial per sum and
 * workgroup and the consuming kernel folds them itself, every workgroup in the same order: no atomics, no finishing launch, no host read.  The number of partials (at most 256 per
 * sum for vectors below 32 MiB, 512 below 128 MiB, 1024 beyond) depends on `rows` alone and the order of every addition on `rows` and j: on a plan whose y is bit-reproducible (TILESPMV_INFO_ENTRY_ORDERED = 1, e.g. deterministic = 1) the
 * iterates and the state are too, run after run and plan after plan.
 * Vector elements read or written per inner iteration beside the product, by count, each basis vector counted once per kernel: 3 k + 7 per row (k + 1, k + 2, k + 2, 2 over the
 * four kernels), 3 k + 9 with d_dinv (its read and the store of M^-1 V_{j+1}); the mean over a full cycle is 1.5 (restart + 1) + 7.  A block object adds its apply (bs + 2).  A close
 * moves k + 2 (+ 1 with d_dinv), an open 5 beside its product.  The dot products are accumulated for 8 basis vectors at a time (what a thread's registers hold), so w is read again
 * once per further group of 8, and the second kernel reads the basis a second time for h2 once w' is complete: 4 k + 2 ceil(k / 8) + 6 with those re-reads.  Folding k sums of P
 * partials in every workgroup reads 8 k P^2 bytes per kernel out of the cache: at most 1/16 of the vector traffic for vectors of 8 MiB and more.
 * Workspace: restart + 3 vectors of rows + 16 elements (the basis V_0..V_restart, w, the copy of b), one more with d_dinv or a block object, (restart + 1) 4 KB of partial sums (16 KB on the largest systems) and
 * 39 KB of R, rotations, g, y and scalars, in one hipMalloc.
 * Guards, taken on the device, exact tests only, uniform branches, in the style of the CG guards:
 *   rr = 0 at an open, or the breakdown flag set   the cycle is dead: inner iterations and closes write no vector, x does not change by a bit — a captured graph may overrun convergence.
 *   h_{j+1,j} = 0 with gamma != 0                  the lucky termination: the rotation is applied (rr = 0), V_{j+1} is not formed, the cycle is closed early: its remaining inner
 *                                                  iterations write nothing and the close uses the columns done so far.
 *   gamma = 0                                      A is singular on this Krylov space and the system incompatible: the breakdown flag is set, never cleared until begin; this iteration,
 *                                                  every later one and every close write nothing, x keeps its last good value.
 *   j = restart without a close in between         the iteration writes nothing: the device's column index never passes `restart` (a replayed graph, misused: below).
 *   The iteration counter advances in every inner iteration whatever the guards did: a breakdown seen at the first check of solve(check_every = 8) reports 8 iterations.
 * WHERE THE CYCLE POSITION LIVES: on the host, in the solver object — the close + open sequence contains a product, so the host must know when to launch it.  begin and flush reset
 * it, iterate advances it.  For graphs: a captured iterate(count) replays correctly when it was captured at a cycle boundary (after begin, flush or a whole number of cycles) and
 * count is a multiple of `restart`.
 * A tilespmv_gmres and its plan run on ONE stream at a time.  d_b, d_x and d_dinv are DEVICE vectors of `rows` elements, 16-byte aligned (hipErrorInvalidValue otherwise);
 * nothing behind element rows - 1 is read or written.
 *
 *   tilespmv_gmres_create        binds a workspace to `plan`, which must be square and whole (tilerow_begin = 0, tilerow_end = tilem; a square TILESPMV_CREATE_TRANSPOSE plan
 *                                qualifies: it solves A^T x = b) and must outlive it; the plan is borrowed.  d_dinv: NULL, or the inverse diagonal, borrowed until destroy — its VALUES
 *                                may change between solves (tilespmv_plan_update_values, then tilespmv_csr_diagonal_device into the same array).  One hipMalloc (synchronises).
 *                                Returns 0, hipErrorInvalidValue (a NULL argument, or restart outside 1 .. TILESPMV_GMRES_MAX_RESTART, which is looked at first: no HIP call made; a non-square or shard plan, a
 *                                misaligned d_dinv: nothing allocated), or the hipMalloc error.
 *   tilespmv_gmres_create_block  the same with a block-Jacobi object for M^-1 (borrowed; its values may change between solves; its rows must be the plan's: hipErrorInvalidValue
 *                                otherwise, nothing allocated): M^-1 V_{j+1} by one apply after the fourth kernel; a close forms u = V y, applies M^-1 and adds.
 *   tilespmv_gmres_begin         as above, from the caller's x (pass zeros for none).
 *   tilespmv_gmres_iterate       `count` inner iterations back to back, with a close and an open after every `restart`-th of a cycle.  Like begin: asynchronous on `stream`, no
 *                                allocation, no synchronisation, no host read, one linear chain of kernels — safe to capture into a hipGraph, for every kind of plan.  It stops at
 *                                no tolerance.
 *   tilespmv_gmres_flush         closes the cycle early (with no column done it writes nothing) and opens the next: d_x is the current iterate and rr its recomputed residual.
 *                                Asynchronous and capturable like iterate.
 *   tilespmv_gmres_state_read    synchronises `stream` and fills the state (set out->size = sizeof(tilespmv_cg_state) first).  status: BREAKDOWN, else CONVERGED when rr is exactly
 *                                0, else RUNNING.
 *   tilespmv_gmres_solve         begin, then iterate(check_every) + state_read until rr <= rtol^2 bb (CONVERGED), `maxiter` inner iterations are done (MAXITER; the last block is
 *                                cut so that no more run) or a breakdown (BREAKDOWN); then flush, so that d_x is the iterate the decision was taken on, and one more read: out->rr
 *                                is the recomputed |b - A x|^2 of the returned x, status and iterations stay those of the decision.  bb = 0 -> x = 0, CONVERGED, 0 iterations.
 *                                check_every < 1 -> 1.  One host synchronisation per check.
 * All but destroy return a hipError_t value (0 = success). */
typedef struct tilespmv_gmres tilespmv_gmres;
#define TILESPMV_GMRES_MAX_RESTART 64
int tilespmv_gmres_create(tilespmv_gmres **s, tilespmv_plan *plan, int restart, const MAT_VAL_TYPE *d_dinv /* may be NULL */);
int tilespmv_gmres_create_block(tilespmv_gmres **s, tilespmv_plan *plan, int restart, const tilespmv_block_jacobi *bj);
void tilespmv_gmres_destroy(tilespmv_gmres *s);
int tilespmv_gmres_begin(tilespmv_gmres *s, const MAT_VAL_TYPE *d_b, MAT_VAL_TYPE *d_x, void *stream);
int tilespmv_gmres_iterate(tilespmv_gmres *s, MAT_VAL_TYPE *d_x, int count, void *stream);
int tilespmv_gmres_flush(tilespmv_gmres *s, MAT_VAL_TYPE *d_x, void *stream);
int tilespmv_gmres_state_read(tilespmv_gmres *s, void *stream, tilespmv_cg_state *out);
int tilespmv_gmres_solve(tilespmv_gmres *s, const MAT_VAL_TYPE *d_b, MAT_VAL_TYPE *d_x, double rtol, int maxiter, int check_every, void *stream,
                         tilespmv_cg_state *out);

/* ---- GMRES with the Krylov basis stored as floats in the double library (new).  An inner iteration of tilespmv_gmres_* is bound by the
 * memory, and of the 4 k + 2 ceil(k / 8) + 6 vector elements it moves per row all but 2 ceil(k / 8) + 5 are reads of the stored basis V_0..V_j; the same basis is what limits the
 * size of system that fits.  tilespmv_gmres_create_basis(..., TILESPMV_GMRES_BASIS_FLOAT) keeps ALL ARITHMETIC, w, x, b, the Hessenberg column and every scalar in double and
 * stores ONLY the basis vectors as 4-byte floats (a compressed basis, as in CB-GMRES).  The solution keeps double accuracy because every open recomputes b - A x in double.
 * begin, iterate, flush, state_read, the guards, the one-writer rule of the scalars, graph capture at cycle boundaries and the single-stream rule read exactly as above; the
 * recurrence differs in these places only:
 *   the stored basis    Vhat_{j+1} = fl32(w'' / h_{j+1,j}), round to nearest;  Vhat_0 = fl32(r / beta).  h_{j+1,j} and beta come from the unrounded vector, as above.
 *   what A and M^-1 multiply   the STORED vector widened back to double, bit for bit what the next dot products read, never the unrounded one: H is then the Arnoldi matrix of the
 *                       basis the close really uses.  The fourth kernel writes Vhat and, in the same walk, its double copy: zhat = dinv o widen(Vhat) with d_dinv; without a
 *                       preconditioner a vector vcur = widen(Vhat), which the product reads; with a block object vcur is the input of its apply.
 *   dots, subtraction, close   (double) w (double) Vhat_i in the dots;  w -= (double) h_i widen(Vhat_i) and u = sum_i y_i widen(Vhat_i) in double.  The scalars are rounded once
 *                       where they multiply, as above.  The three kernels that read the whole basis take four floats with one 16-byte load against two 16-byte loads of w; the order of
 *                       every addition depends on rows and j alone (it is not the value form's order).
 * THE FLOOR INSIDE A CYCLE: the first basis vector is fl32(r / beta), not r / beta, so inside ONE cycle the true residual cannot fall below about eps32 = 6e-8 times the residual
 * the cycle began with, while the recurrence's rr keeps falling.  On a fast-converging system (the 67 x 67 skew stencil with diagonal 4, restart 64) the recurrence reports
 * sqrt(rr / bb) = 5e-16 after 40 iterations where the recomputed residual is 3e-8.  Hence
 *   tilespmv_gmres_solve   with a float basis accepts the stopping test ONLY ON A RECOMPUTED rr: when a state read passes rr <= rtol^2 bb and the host's cycle position is not
 *                       0, it flushes, reads again and tests again; if that test fails it carries on iterating from the fresh cycle.  No second flush at the end when the decision
 *                       was taken on a flushed state.  MAXITER and BREAKDOWN are as above.  A caller of begin / iterate who stops on rr must do the same: flush before believing it.
 *                       With restart <= 16 the counts equal those of the double basis on the library's test systems; at restart 64 on the fast system above 34 against 27.
 * Per row and inner iteration the float form moves 4 k + 1 basis elements of 4 bytes and 2 ceil(k / 8) + 6 doubles (the fourth kernel writes the float vector and one double copy).
 * WORKSPACE, one hipMalloc of tilespmv_gmres_workspace_bytes(s) =
 *     (restart + 1) B + v D + 2 (restart + 1) Q + 2 Q + 32768 + 4 * 768 + 256   bytes, every term a multiple of 256, where
 *     B = (rows + 16) * basis_bytes rounded up to 256     one stored basis vector
 *     D = (rows + 16) * sizeof(MAT_VAL_TYPE) rounded up to 256, and v counts the value-type vectors: w and b, and
 *         value basis: + 1 (zhat) with d_dinv or a block object;   float basis: + 1 (vcur) without a preconditioner, + 1 (zhat) with d_dinv, + 2 (both) with a block object
 *     Q = 8 P rounded up to 256, P = min(cap, max(1, min(1024, ceil((rows / L) / 512)))), L = 16 / sizeof(MAT_VAL_TYPE), rows / L rounded down,
 *         cap = 256 below rows * sizeof(MAT_VAL_TYPE) = 32 MiB, 512 below 128 MiB, 1024 beyond     the partials of one sum
 *     32768: R;  768 each: the rotations, g, y;  256: the scalars.
 *   GMRES(64) on 16.8 M rows: 9.0 GB with the value basis, 4.8 GB with the float one.
 *
 *   tilespmv_gmres_create_basis   tilespmv_gmres_create (bj = NULL) or tilespmv_gmres_create_block (d_dinv = NULL) with the bytes of a stored basis element.  basis_bytes is
 *                                 looked at first, together with restart, before any HIP call and before the plan is looked at: 0 (TILESPMV_GMRES_BASIS_VALUE) or
 *                                 sizeof(MAT_VAL_TYPE) gives exactly the solver of those two creates — so 4 is the identity in the float library and a caller may pass 4 to either;
 *                                 4 (TILESPMV_GMRES_BASIS_FLOAT) in the double library gives the float basis; anything else (2; 8 in the float library) and d_dinv together with
 *                                 bj give hipErrorInvalidValue with *s = NULL and nothing allocated.  The other refusals are those of tilespmv_gmres_create.  A 2-byte basis is
 *                                 not offered: a unit vector of 16 M rows has entries near the fp16 subnormal range and would need a scale per vector.
 *   tilespmv_gmres_basis_bytes    bytes per stored basis element: sizeof(MAT_VAL_TYPE) or 4 (0 for NULL).
 *   tilespmv_gmres_workspace_bytes   the size of the one hipMalloc, the formula above, for both forms (0 for NULL). */
#define TILESPMV_GMRES_BASIS_VALUE 0   /* the value type: exactly tilespmv_gmres_create / _create_block */
#define TILESPMV_GMRES_BASIS_FLOAT 4
int tilespmv_gmres_create_basis(tilespmv_gmres **s, tilespmv_plan *plan, int restart, const MAT_VAL_TYPE *d_dinv /* may be NULL */,
                                const tilespmv_block_jacobi *bj /* may be NULL */, int basis_bytes);
int tilespmv_gmres_basis_bytes(const tilespmv_gmres *s);
size_t tilespmv_gmres_workspace_bytes(const tilespmv_gmres *s);

const char *tilespmv_version(void);
int tilespmv_device_count(void);    /* 0 when no HIP device is visible */

#ifdef __cplusplus
}
#endif
#endif /* TILESPMV_H_ */
