// hip_tile_create.h — CSR -> Tile_matrix on the DEVICE (the device-side half; reference src/csr2tile.h:629-1020).
// A DevTile is a Tile_matrix whose member arrays live in device memory, with the uploaded CSR and the tile-ordered gather beside it.  Two consumers:
//   Tile_create_device (C ABI)            downloads it into a host Tile_matrix that is byte-identical to Tile_create's
//   tilespmv_plan_create_from_csr (C ABI) builds the plan's streams from it on the device: nothing but the CSR arrays crosses the bus
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "host_util.h"

namespace tilespmv {

struct DevTile {
    Tile_matrix T{};                       // member arrays: DEVICE pointers; counts and sizes: host values
    int rowA = 0, colA = 0;
    long long nnz = 0;                     // rowptr[rowA]
    const int *rowptr = nullptr, *colidx = nullptr;   // the uploaded CSR (device)
    const val_t *val = nullptr;
    long long val_base = 0;                // the row pointer's first entry (host CSR that is a row block of a larger matrix): position j of the arrays above is position val_base + j of the caller's
    bool val_owned = false;                // val is an array of the DevTile's own (not the caller's device array)
    const unsigned long long *key = nullptr;   // per nonzero, tile order: tile-row << (8 + cb_bits) | column block << 8 | local row << 4 | local column
    const int *ent = nullptr;              // per nonzero, tile order: its position in the CSR arrays
    const int *tile_bi = nullptr;          // per tile: its tile-row
    const long long *hyb_off = nullptr;    // the same as 64-bit offsets (nullptr: the matrix has no HYB tile): what plan_tile_ops.h's per-tile functions take
    const int *hyb_byte_off = nullptr;     // per tile (+ 1): first byte of a HYB tile in hybIdx (the running offset the reference calls ptroffset2, src/tilespmv_cpu.h:195-196)
    int cb_bits = 0;
    bool have_deferred = false;            // deferredcoo_* built (Tile_create_device) or skipped (plans never read them in the in-tile COO mode)
    int unsorted_rows = 0;                 // rows of the extracted matrix whose columns do not increase (the host sorts those after the download, like the reference)
    std::vector<void *> allocs;            // arrays with a hipMalloc of their own
    std::vector<void *> pools;             // pool blocks (several arrays carved from each): freed only by devtile_destroy
    double ms_upload = 0, ms_sort = 0, ms_tiles = 0, ms_select = 0, ms_pack = 0;
};

// Value-map builds (TILESPMV_CREATE_VALUE_MAP): the tiled matrix and the plan are built from STAND-IN values — the value of the nonzero at CSR position j is the number whose bit
// pattern is that of the smallest positive normal number plus j — instead of the caller's.  The builders only move values, so every value slot of the finished plan names its
// source (bits 0: padding), and the two layout rules that look at a value (an ELL row's length for absorbed entries, plan_tile_ops.h; null records of the packed lists, erec_is_null)
// see a nonzero wherever a nonzero is stored: they follow the pattern, never the values (hip_value_map.hip reads the map off the streams, then writes the caller's values in).
#if defined(TILESPMV_F32)
typedef unsigned vmap_bits_t;
constexpr vmap_bits_t VMAP_BIAS = 0x00800000u;                // FLT_MIN
constexpr long long VMAP_MAX_INDEX = 0x7F7FFFFFll - 0x00800000ll;   // ... + j stays finite (FLT_MAX) up to here
#else
typedef unsigned long long vmap_bits_t;
constexpr vmap_bits_t VMAP_BIAS = 0x0010000000000000ull;      // DBL_MIN
constexpr long long VMAP_MAX_INDEX = 0x7FFFFFFFll;           // (int32 CSR positions)
#endif
static_assert(sizeof(vmap_bits_t) == sizeof(val_t), "stand-in values are bit patterns of val_t");
__host__ __device__ inline val_t vmap_encode(long long j) { const vmap_bits_t b = VMAP_BIAS + (vmap_bits_t)j; val_t v; __builtin_memcpy(&v, &b, sizeof(v)); return v; }
__host__ __device__ inline long long vmap_decode(val_t v) { vmap_bits_t b; __builtin_memcpy(&b, &v, sizeof(b)); return b == 0 ? -1 : (long long)(b - VMAP_BIAS); }

// rc 0, -1 no device, -2 int32 offsets of Tile_matrix exceeded, -3 HIP error / out of device memory
// csr_on_device: the three CSR arrays are DEVICE pointers already (row pointer based at 0; borrowed, not freed): no upload at all
// stand_in_values: DevTile::val holds vmap_encode(position in the caller's value array) instead of the caller's values (a device array of its own, whichever side the CSR came from;
// nothing of the caller's values is read)
// stand_in_pos (device, with stand_in_values only; nullptr: the nonzero's own position): nonzero j's stand-in is vmap_encode(stand_in_pos[j]) — a transposed build names positions of A
int devtile_create(DevTile **out, int rowA, int colA, const MAT_PTR_TYPE *h_rowptr, const int *h_colidx, const val_t *h_val, unsigned flags, bool want_deferred, bool csr_on_device = false,
                   bool stand_in_values = false, const int *stand_in_pos = nullptr);
void devtile_destroy(DevTile *D);
// every member array into freshly malloc'd host arrays (Tile_destroy frees them)
int devtile_download(const DevTile *D, Tile_matrix *host);

// hip_transpose.hip: A^T of a CSR on the device (the definition of tilespmv_csr_transpose, include/tilespmv.h).  rp: the row pointer (device; entries from `base` on, base + nnz at
// rp[rowA]); ci0 / v0: the column indices / values of the block (the caller's position `base` first; v0 may be nullptr).  rpT[colA + 1], ciT / vT / srcT[nnz]; vT and srcT may
// be nullptr.  Allocates its scratch, synchronises `st`.  hipErrorInvalidValue: a column index outside [0, colA) or a decreasing row pointer
hipError_t csr_transpose_dev(int rowA, int colA, const int *rp, long long base, long long nnz, const int *ci0, const val_t *v0, int *rpT, int *ciT, val_t *vT, int *srcT,
                             hipStream_t st);
// A^T of the caller's CSR (host arrays, uploaded first, or device arrays) in device arrays of its own (TILESPMV_CREATE_TRANSPOSE): a colA x rowA CSR based at 0, ready for
// devtile_create(csr_on_device = true).  want_values: v gathered; want_src: src = position of every entry in A's arrays (the value map's stand-ins); keep_values_of_a (host CSR):
// A's values stay on the device in valA (valA[j] = the caller's value at position base + j)
struct DevCsrT {
    int rows = 0, cols = 0;
    long long nnz = 0, base = 0;
    int *rp = nullptr, *ci = nullptr, *src = nullptr;
    val_t *v = nullptr, *valA = nullptr;
    DevCsrT() = default;
    DevCsrT(const DevCsrT &) = delete;
    DevCsrT &operator=(const DevCsrT &) = delete;
    ~DevCsrT();
};
// 0, or -3 (HIP error, out of device memory, or not a valid CSR: message on stderr)
int devcsr_transpose(DevCsrT *T, int rowA, int colA, const MAT_PTR_TYPE *rp, const int *ci, const val_t *v, bool csr_on_device, bool want_values, bool want_src, bool keep_values_of_a);

}  // namespace tilespmv
