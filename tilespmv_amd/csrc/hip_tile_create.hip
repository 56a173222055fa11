// hip_tile_create.hip — CSR -> Tile_matrix on the device (hip_tile_create.h).
//
// Replaces Tile_create / convert_step1..4 of the reference (src/csr2tile.h:5-1020) a second time: host_tile_create.cpp is the O(nnz) many-core host version, this is the
// device version, producing the SAME bytes (tests/test_gpu_device_build.py compares every member array with the host's).  The shape of the algorithm is not the host's:
//   1. every nonzero gets a 64-bit key  tile-row | column block | local row | local column  (one wavefront per tile-row walks its slice of the CSR arrays, coalesced);
//   2. ONE stable radix sort by (tile-row, column block) puts the nonzeros into tile order — the reference searches the tile list per nonzero (src/csr2tile.h:406-418),
//      the host version buckets per tile-row with a stamp array; the key carries the local coordinates through the sort outside the sorted bit range;
//   3. run-length encoding of the sorted keys = the tile list (tile_ptr, tile_columnidx, tile_nnz);
//   4. one thread per tile: row counts from the keys, the shared selection rule (tile_select.h), sizes -> fourteen exclusive scans;
//   5. one thread per tile packs its payload with the shared packer (tile_pack.h; values gathered from the CSR array through the sorted positions); nibble streams packed by
//      a second kernel (two tiles may share a byte); the extracted very-sparse matrix (deferredcoo_*) by one more stable sort by row.
// Steps 1-3 are this builder's own; the selection rule, the packer and the table of member arrays that sizes, allocates and downloads them (tile_fields.h) are the host builder's too.
// HYB tiles (TILESPMV_CREATE_HYB, dormant in the shipped reference: SURVEY S1; width search src/csr2tile.h:279-306 = tile_select.h, pack :505-548, index bytes :984-1008) are built
// too (round 6): a tile's index bytes are tile-byte-aligned, so the thread that packs the tile writes them itself, at a byte offset that is one more scan.
#include <cstring>

#include <hip/hip_runtime.h>
#include "hip_prims.h"

#include <sys/time.h>
#include <thread>

#include "hip_tile_create.h"
#include "tile_fields.h"
#include "tile_pack.h"
#include "tile_select.h"

namespace tilespmv {
namespace {

#define TC_TRY(expr)                                                                                               \
    do {                                                                                                           \
        hipError_t e_ = (expr);                                                                                    \
        if (e_ != hipSuccess) {                                                                                    \
            fprintf(stderr, "tilespmv: device Tile_create: HIP error %d (%s) at %s:%d\n", (int)e_, hipGetErrorString(e_), __FILE__, __LINE__); \
            (void)hipGetLastError();                                                                               \
            return -3;                                                                                             \
        }                                                                                                          \
    } while (0)


// the values' upload, by a helper thread on a stream of its own
struct ValueUpload {
    std::thread th;
    hipError_t err = hipSuccess;
    void start(int dev, val_t *dst, const val_t *src, size_t bytes)
    {
        ValueUpload *self = this;
        th = std::thread([=] {
            hipError_t e = hipSetDevice(dev);
            hipStream_t cs = nullptr;
            if (e == hipSuccess) e = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking);
            if (e == hipSuccess) {
                e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, cs);
                if (e == hipSuccess) e = hipStreamSynchronize(cs);
                (void)hipStreamDestroy(cs);
            }
            self->err = e;
        });
    }
    hipError_t wait() { if (th.joinable()) th.join(); return err; }
    ~ValueUpload() { if (th.joinable()) th.join(); }
};


inline double now_ms() { timeval t; gettimeofday(&t, NULL); return t.tv_sec * 1e3 + t.tv_usec * 1e-3; }
inline int bits_for(int n) { int b = 1; while (b < 31 && (1ll << b) < (long long)n) b++; return b; }   // bits that hold 0 .. n - 1 (at least one)

typedef unsigned long long u64;

// ---- 1. keys: one wavefront per tile-row
__global__ __launch_bounds__(256) void k_tc_keys(int rowA, int tilem, const int *__restrict__ rowptr, const int *__restrict__ colidx, int bi_shift, u64 *__restrict__ key, int *__restrict__ ent)
{
    __shared__ int s_rp[4][17];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long long bi = (long long)blockIdx.x * 4 + wv;
    if (bi < tilem && lane < 17) s_rp[wv][lane] = rowptr[min(16LL * bi + lane, (long long)rowA)];
    __syncthreads();
    if (bi >= tilem) return;
    const int j0 = s_rp[wv][0], j1 = s_rp[wv][16];
    for (int j = j0 + lane; j < j1; j += 64) {
        int r = 0;
#pragma unroll
        for (int k = 1; k < 16; k++) r += s_rp[wv][k] <= j;   // local row of CSR position j
        const unsigned c = (unsigned)colidx[j];
        key[j] = ((u64)bi << bi_shift) | ((u64)(c >> 4) << 8) | (u64)((r << 4) | (int)(c & 15u));
        ent[j] = j;
    }
}

constexpr unsigned KEY_TILE_SHIFT = 8;   // key >> 8 = (tile-row, column block): what names a tile

// ---- 3. the tile list from the run-length encoded keys
__global__ void k_tc_tiles(int tilenum, int tilem, int cb_bits, const u64 *__restrict__ uniq, int *__restrict__ tile_columnidx, int *__restrict__ tile_bi, int *__restrict__ tile_ptr)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= tilenum) return;
    const u64 u = uniq[t];
    const int bi = (int)(u >> cb_bits), cb = (int)(u & ((1ull << cb_bits) - 1ull));
    tile_columnidx[t] = cb; tile_bi[t] = bi;
    const int prev = t ? (int)(uniq[t - 1] >> cb_bits) : -1;
    for (int b = prev + 1; b <= bi; b++) tile_ptr[b] = (int)t;   // tile-rows without tiles in between point at this tile too
    if (t == tilenum - 1) for (int b = bi + 1; b <= tilem; b++) tile_ptr[b] = tilenum;
}

struct TileArrays {   // the per-tile arrays of Tile_matrix (device)
    char *Format; int *blknnz; unsigned char *blknnznnz; int *dnsrowptr, *dnscolptr; char *tilewidth;
    int *csrptr_offset, *hyb_coocount, *new_coocount;
    int *fmt_offset[7];   // csr, coo, ell, hyb, dns, dnsrow, dnscol (TILESPMV_FMT_* order)
    int *hyb_bytes;       // HYB tiles: bytes of the tile in hybIdx (scanned into the tile's byte offset)
};

// ---- 4. selection: one thread per tile
__global__ __launch_bounds__(256) void k_tc_select(int tilenum, int tilem, int tilen, int rowA, int colA, bool allow_hyb, bool cdna4, const int *__restrict__ tile_nnz, const int *__restrict__ tile_bi,
                                                     const int *__restrict__ tile_columnidx, const u64 *__restrict__ key, TileArrays A, unsigned long long *__restrict__ refused)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= tilenum) return;
    const int e0 = tile_nnz[t], n = tile_nnz[t + 1] - e0;
    const int rowlen = tile_rowlen(tile_bi[t], tilem, rowA), collen = tile_collen(tile_columnidx[t], tilen, colA);
    u64 c0 = 0, c1 = 0;   // sixteen 8-bit row counters
    Occupancy occ;        // ... and, in the same walk, which positions the tile stores (tile_select.h "repeated positions")
    for (int k = 0; k < n; k++) {
        const int r = (int)(key[e0 + k] >> 4) & 15;
        occ.add((int)(key[e0 + k] & 255ull));
        const u64 one = 1ull << (8 * (r & 7)), m = 255ull << (8 * (r & 7));
        if (r < 8) c0 = (c0 & ~m) | ((c0 + one) & m); else c1 = (c1 & ~m) | ((c1 + one) & m);
    }
    const u64 *kp = key + e0;
    const Choice c = select_format(n, rowlen, collen, [c0, c1](int r) { return (int)(((r < 8 ? c0 : c1) >> (8 * (r & 7))) & 255ull); }, [kp](int k) { return (int)(kp[k] & 255ull); }, allow_hyb, cdna4, occ.repeat);
    if (c.refused) atomicMax(refused, (unsigned long long)(tilenum - t));   // the FIRST refused tile wins (0: none); read back with the scans' totals
    A.Format[t] = (char)c.fmt;
    A.blknnz[t] = c.stored;
    A.blknnznnz[t] = (unsigned char)c.stored;
    A.tilewidth[t] = (char)c.width;
    A.dnsrowptr[t] = c.ndr; A.dnscolptr[t] = c.ndc;
    A.hyb_coocount[t] = c.hybcoo; A.new_coocount[t] = c.extracted;
    A.csrptr_offset[t] = c.csrptr;
    A.fmt_offset[c.fmt][t] = c.stored;
    if (c.fmt == TILESPMV_FMT_HYB) A.hyb_bytes[t] = (c.width * rowlen + 1) / 2 + c.hybcoo;   // ELL part in nibbles (rounded up to a byte), then one byte per remainder entry
}

// totals of K int arrays of n elements each, in 64 bits (the scans below are done in int: a total that fits proves every prefix does, the counts are non-negative)
struct ScanSet { int *a[16]; };
__global__ __launch_bounds__(256) void k_tc_totals(ScanSet S, int K, long long n, unsigned long long *__restrict__ totals)
{
    for (int k = 0; k < K; k++) {
        long long acc = 0;
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) acc += S.a[k][i];
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
        if ((threadIdx.x & 63) == 0 && acc) atomicAdd(&totals[k], (unsigned long long)acc);
    }
}

struct PackArrays {
    PackOut out;               // (tile_pack.h)
    const int *hyb_byte_off;   // every tile's byte offset in hybIdx
    unsigned *x_key; int *x_col; val_t *x_val;   // extracted entries in tile order: global row, column, value (nullptr: not wanted)
    int *deferredcoo_ptr;                          // per-row counts (atomics), scanned afterwards
};

// ---- 5. packing: one thread per tile (tile_pack.h)
__global__ __launch_bounds__(256) void k_tc_pack(int tilenum, int tilem, int rowA, const Tile_matrix T, const int *__restrict__ tile_bi, const u64 *__restrict__ key, const int *__restrict__ ent,
                                                   const int *__restrict__ colidx, const val_t *__restrict__ vals, PackArrays P)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= tilenum) return;
    const int bi = tile_bi[t];
    const u64 *kp = key + T.tile_nnz[t]; const int *src = ent + T.tile_nnz[t];
    pack_tile(T, t, tile_rowlen(bi, tilem, rowA), P.hyb_byte_off[t], [kp](int k) { return (int)(kp[k] & 255ull); }, [src, vals](int k) { return vals[src[k]]; },
              [&](int slot, int r, int k) {
                  if (!P.x_key) return;
                  const unsigned row = (unsigned)bi * 16u + (unsigned)r;
                  P.x_key[slot] = row; P.x_col[slot] = colidx[src[k]]; P.x_val[slot] = vals[src[k]];
                  atomicAdd(&P.deferredcoo_ptr[row], 1);
              }, P.out);
}

// two index bytes -> one byte of a nibble stream (src/encode.h:29-50)
__global__ void k_tc_nibbles(const unsigned char *__restrict__ src, unsigned char *__restrict__ dst, long long n)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (2 * i >= n) return;
    const unsigned hi = src[2 * i], lo = (2 * i + 1 < n) ? src[2 * i + 1] : 0u;
    dst[i] = (unsigned char)((hi << 4) + lo);
}

// the extracted matrix: entries in their final (row, order of appearance) order through the sorted positions
__global__ void k_tc_deferred(int n, const int *__restrict__ pos, const int *__restrict__ x_col, const val_t *__restrict__ x_val, int *__restrict__ colidx, val_t *__restrict__ val)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    colidx[i] = x_col[pos[i]]; val[i] = x_val[pos[i]];
}
__global__ void k_tc_widen(long long n, const int *__restrict__ a, long long *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = a[i];
}
__global__ void k_tc_stand_in(long long n, long long base, val_t *__restrict__ v)   // (hip_tile_create.h vmap_encode)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = vmap_encode(base + i);
}
__global__ void k_tc_stand_in_at(long long n, const int *__restrict__ pos, val_t *__restrict__ v)   // (the stand-ins of a transposed build: positions of A)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = vmap_encode(pos[i]);
}
__global__ void k_tc_iota(int n, int *__restrict__ a)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = (int)i;
}
__global__ void k_tc_unsorted_rows(int rowA, const int *__restrict__ ptr, const int *__restrict__ colidx, int *__restrict__ count)
{
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rowA) return;
    for (int i = ptr[r] + 1; i < ptr[r + 1]; i++) if (colidx[i - 1] >= colidx[i]) { atomicAdd(count, 1); return; }
}

// Device arrays come from a few POOLS (one zeroed hipMalloc per phase of the build: the per-tile arrays, the payload arrays) instead of one hipMalloc + memset each — the build
// makes about forty arrays, and on a busy allocator their calls, not the kernels, set the time (one box: 62 ms in the packing phase against 6 ms of kernels).  An array that
// does not fit what is left of the current pool (or is asked for outside one) gets a hipMalloc of its own.
struct Pool { char *at = nullptr; size_t left = 0; };
thread_local Pool t_pool;   // (a build runs on one host thread; two builds on two threads have a pool each)
inline size_t pool_need(size_t n, size_t elem) { return (std::max<size_t>(n, 1) * elem + 16 + 255) / 256 * 256; }
int pool_begin(DevTile *D, size_t bytes)
{
    void *p = nullptr;
    t_pool = Pool();
    TC_TRY(hipMalloc(&p, bytes + 256));
    D->pools.push_back(p);   // (its own list: dfree never looks here — the first array carved from a pool has the pool's address, and freeing IT must not free the pool)
    TC_TRY(hipMemsetAsync(p, 0, bytes + 256, 0));
    t_pool.at = (char *)p; t_pool.left = bytes + 256;
    return 0;
}
inline void pool_end() { t_pool = Pool(); }
int dalloc_raw(DevTile *D, void **out, size_t n, size_t elem, bool zero)
{
    const size_t need = pool_need(n, elem);
    if (t_pool.left >= need) {   // (pool memory is zeroed already)
        *out = t_pool.at; t_pool.at += need; t_pool.left -= need;
        return 0;
    }
    void *p = nullptr;
    const size_t bytes = std::max<size_t>(n, 1) * elem + 16;
    TC_TRY(hipMalloc(&p, bytes));
    D->allocs.push_back(p);
    if (zero) TC_TRY(hipMemsetAsync(p, 0, bytes, 0));
    *out = p;
    return 0;
}
template <class V>
int dalloc(DevTile *D, V **out, size_t n, bool zero) { return dalloc_raw(D, (void **)out, n, sizeof(V), zero); }
// the member arrays of D->T (tile_fields.h) that are not allocated yet: what a pool must hold for them, and the arrays themselves (zeroed)
inline size_t dev_count(const TileField &f) { return (size_t)(f.count + f.slack + f.dev_slack); }
size_t fields_need(DevTile *D, const TileExtents &X, unsigned groups)
{
    size_t bytes = 0;
    for_each_tile_field(D->T, X, groups, [&](const TileField &f) { if (!*f.ptr) bytes += pool_need(dev_count(f), f.elem); });
    return bytes;
}
int dalloc_fields(DevTile *D, const TileExtents &X, unsigned groups)
{
    int rc = 0;
    for_each_tile_field(D->T, X, groups, [&](const TileField &f) { if (rc == 0 && !*f.ptr) rc = dalloc_raw(D, f.ptr, dev_count(f), f.elem, true); });
    return rc;
}
// hipFree waits for the whole device — also for the values' upload that runs beside the first steps of create_impl: while that is under way, memory to be released is only noted
thread_local std::vector<void *> *t_free_later = nullptr;
inline void free_now_or_later(void *p)
{
    if (!p) return;
    if (t_free_later) t_free_later->push_back(p); else (void)hipFree(p);
}
inline void dfree(DevTile *D, const void *p)   // (an array carved from a pool is not in D->allocs: it goes with its pool, at devtile_destroy)
{
    if (!p) return;
    auto it = std::find(D->allocs.begin(), D->allocs.end(), (void *)p);
    if (it == D->allocs.end()) return;
    D->allocs.erase(it);
    free_now_or_later((void *)p);
}
inline unsigned blocks_for(long long n, int per) { return (unsigned)std::max<long long>(1, (n + per - 1) / per); }

int create_impl(DevTile *D, int rowA, int colA, const MAT_PTR_TYPE *h_rowptr, const int *h_colidx, const val_t *h_val, unsigned flags, bool want_deferred, bool csr_on_device, bool stand_in,
                const int *stand_in_pos)
{
    const bool verbose = getenv("TILESPMV_CREATE_VERBOSE") != nullptr, cdna4 = flags & TILESPMV_CREATE_CDNA4, allow_hyb = flags & TILESPMV_CREATE_HYB;
    pool_end();   // (no pool left over from a build that failed on this thread)
    Tile_matrix &T = D->T;
    const int tilem = tiles_of(rowA), tilen = tiles_of(colA);
    // the row pointer may be a slice of a larger matrix's (a row block: pointers not rebased): the block's nonzeros are [base, base + nnz) of the column / value arrays
    long long base = 0, nnz = 0;
    if (csr_on_device) {   // (device CSR: based at 0 by contract; its last row pointer is the one number fetched)
        int last = 0;
        TC_TRY(hipMemcpy(&last, h_rowptr + rowA, sizeof(int), hipMemcpyDeviceToHost));
        nnz = last;
    } else { base = h_rowptr[0]; nnz = (long long)h_rowptr[rowA] - base; }
    std::vector<int> rebased;
    if (base != 0) {
        rebased.resize((size_t)rowA + 1);
        for (int r = 0; r <= rowA; r++) rebased[(size_t)r] = (int)(h_rowptr[r] - base);
        h_rowptr = rebased.data(); h_colidx += base; h_val += base;
    }
    D->rowA = rowA; D->colA = colA; D->nnz = nnz; D->val_base = base;
    if (stand_in && nnz > 0 && base + nnz - 1 > VMAP_MAX_INDEX) { fprintf(stderr, "tilespmv: value map: %lld value positions exceed what a stand-in value can name\n", base + nnz); return -2; }
    T.tilem = tilem; T.tilen = tilen;
    const int cb_bits = bits_for(tilen), bi_bits = bits_for(tilem);
    D->cb_bits = cb_bits;

    // ---- the CSR arrays cross the bus (the only large upload of the device pipeline)
    std::vector<void *> later;
    struct Later {   // released on every way out, after the upload has been joined (members are destroyed in reverse order: `values` below goes first)
        std::vector<void *> &v;
        ~Later() { t_free_later = nullptr; for (void *q : v) (void)hipFree(q); v.clear(); }
    } later_guard{later};
    ValueUpload values;   // (joined on every way out of this function, before anybody frees d_val)
    double t0 = now_ms();
    int *d_rowptr = nullptr, *d_colidx = nullptr; val_t *d_val = nullptr;
    if (csr_on_device) {   // (borrowed: never in D->allocs)
        d_rowptr = const_cast<int *>(h_rowptr); d_colidx = const_cast<int *>(h_colidx); d_val = const_cast<val_t *>(h_val);
        if (stand_in) { if (dalloc(D, &d_val, (size_t)nnz, false)) return -3; D->val_owned = true; }
    } else {
        if (dalloc(D, &d_rowptr, (size_t)rowA + 1, false) || dalloc(D, &d_colidx, (size_t)nnz, false) || dalloc(D, &d_val, (size_t)nnz, false)) return -3;
        D->val_owned = true;
        TC_TRY(hipMemcpy(d_rowptr, h_rowptr, ((size_t)rowA + 1) * sizeof(int), hipMemcpyHostToDevice));
        if (nnz) TC_TRY(hipMemcpy(d_colidx, h_colidx, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice));
        // the values follow on a stream of their own, fed by a helper thread (a copy from pageable memory holds its caller until the last chunk is staged), while this thread sorts the
        // keys, lists the tiles and selects their formats: nothing before the packing reads a value (config 4: 0.67 GB = 12.6 ms of bus time behind 7 ms of kernels)
        if (nnz && !stand_in) {
            int dev = 0;
            TC_TRY(hipGetDevice(&dev));
            bool started = false;
            try { values.start(dev, d_val, h_val, (size_t)nnz * sizeof(val_t)); started = true; } catch (...) {}   // (no thread to be had: the plain copy)
            if (started) t_free_later = &later;
            else TC_TRY(hipMemcpy(d_val, h_val, (size_t)nnz * sizeof(val_t), hipMemcpyHostToDevice));
        }
    }
    if (stand_in && nnz > 0) {   // the stand-in values instead of the caller's (hip_tile_create.h): nothing of theirs is read
        if (stand_in_pos) hipLaunchKernelGGL(k_tc_stand_in_at, dim3(blocks_for(nnz, 256)), dim3(256), 0, 0, nnz, stand_in_pos, d_val);
        else hipLaunchKernelGGL(k_tc_stand_in, dim3(blocks_for(nnz, 256)), dim3(256), 0, 0, nnz, base, d_val);
        TC_TRY(hipGetLastError());
    }
    D->rowptr = d_rowptr; D->colidx = d_colidx; D->val = d_val;
    D->ms_upload = now_ms() - t0; t0 = now_ms();

    // ---- keys + stable sort by (tile-row, column block)
    u64 *key_a = nullptr, *key_b = nullptr; int *ent_a = nullptr, *ent_b = nullptr;
    if (dalloc(D, &key_a, (size_t)nnz, false) || dalloc(D, &key_b, (size_t)nnz, false) || dalloc(D, &ent_a, (size_t)nnz, false) || dalloc(D, &ent_b, (size_t)nnz, false)) return -3;
    hipLaunchKernelGGL(k_tc_keys, dim3(blocks_for(tilem, 4)), dim3(256), 0, 0, rowA, tilem, d_rowptr, d_colidx, 8 + cb_bits, key_a, ent_a);
    TC_TRY(hipGetLastError());
    {
        u64 *k_cur = key_a, *k_alt = key_b; int *v_cur = ent_a, *v_alt = ent_b;
        size_t tmp_b = 0; void *tmp = nullptr;
        if (nnz > 0) {
            TC_TRY(prims::sort_pairs_u64_int(nullptr, tmp_b, k_cur, k_alt, v_cur, v_alt, (size_t)nnz, 8u, (unsigned)(8 + cb_bits + bi_bits), (hipStream_t)0));
            TC_TRY(hipMalloc(&tmp, std::max<size_t>(tmp_b, 16)));
            hipError_t e = prims::sort_pairs_u64_int(tmp, tmp_b, k_cur, k_alt, v_cur, v_alt, (size_t)nnz, 8u, (unsigned)(8 + cb_bits + bi_bits), (hipStream_t)0);
            if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)0)   /* (not the device: the values' upload is still under way on its own stream) */;
            free_now_or_later(tmp);
            TC_TRY(e);
        }
        D->key = k_cur; D->ent = v_cur;
        dfree(D, k_alt); dfree(D, v_alt);
    }
    D->ms_sort = now_ms() - t0; t0 = now_ms();

    // ---- tile list
    int tilenum = 0;
    if (dalloc(D, &T.tile_ptr, (size_t)tilem + 1, true)) return -3;
    u64 *d_uniq = nullptr; int *d_counts = nullptr, *d_nruns = nullptr;
    if (nnz > 0) {
        if (dalloc(D, &d_uniq, (size_t)nnz, false) || dalloc(D, &d_counts, (size_t)nnz + 1, false) || dalloc(D, &d_nruns, 1, true)) return -3;
        size_t tmp_b = 0; void *tmp = nullptr;
        TC_TRY(prims::rle_u64(nullptr, tmp_b, D->key, KEY_TILE_SHIFT, (unsigned)nnz, d_uniq, d_counts, d_nruns, (hipStream_t)0));
        TC_TRY(hipMalloc(&tmp, std::max<size_t>(tmp_b, 16)));
        hipError_t e = prims::rle_u64(tmp, tmp_b, D->key, KEY_TILE_SHIFT, (unsigned)nnz, d_uniq, d_counts, d_nruns, (hipStream_t)0);
        if (e == hipSuccess) e = hipMemcpy(&tilenum, d_nruns, sizeof(int), hipMemcpyDeviceToHost);
        free_now_or_later(tmp);
        TC_TRY(e);
    }
    T.tilenum = tilenum;
    if (!(flags & TILESPMV_CREATE_QUIET)) printf("\n  The number of tile = %i\n", tilenum);
    const size_t np1 = (size_t)tilenum + 1;
    // ---- pool of the arrays of tilenum (+ 1) elements: the table's (tile_ptr exists already), and beside them every tile's tile-row, the HYB tiles' byte counts and the scans' totals
    constexpr int NS = 14;
    TileExtents X; X.rowA = rowA;
    if (pool_begin(D, fields_need(D, X, TF_LIST | TF_TILE) + pool_need((size_t)tilenum, 4) + pool_need(np1, 4) + pool_need(NS + 1, 8))) return -3;
    int *d_tile_bi = nullptr, *d_hyb_bytes = nullptr;
    if (dalloc_fields(D, X, TF_LIST | TF_TILE) || dalloc(D, &d_tile_bi, (size_t)tilenum, true) || dalloc(D, &d_hyb_bytes, np1, true)) return -3;
    D->tile_bi = d_tile_bi;
    if (tilenum > 0) {
        hipLaunchKernelGGL(k_tc_tiles, dim3(blocks_for(tilenum, 256)), dim3(256), 0, 0, tilenum, tilem, cb_bits, d_uniq, T.tile_columnidx, d_tile_bi, T.tile_ptr);
        TC_TRY(hipGetLastError());
        // tile_nnz = exclusive scan of the run lengths (np1 elements: the last one is the total)
        TC_TRY(hipMemsetAsync(d_counts + tilenum, 0, sizeof(int), 0));
        size_t tmp_b = 0; void *tmp = nullptr;
        TC_TRY(prims::scan_int(nullptr, tmp_b, d_counts, T.tile_nnz, np1, (hipStream_t)0));
        TC_TRY(hipMalloc(&tmp, std::max<size_t>(tmp_b, 16)));
        hipError_t e = prims::scan_int(tmp, tmp_b, d_counts, T.tile_nnz, np1, (hipStream_t)0);
        if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)0);
        free_now_or_later(tmp);
        TC_TRY(e);
    }
    dfree(D, d_uniq); dfree(D, d_counts); dfree(D, d_nruns);
    D->ms_tiles = now_ms() - t0; t0 = now_ms();

    // ---- per-tile metadata + format selection + scans
    const TileArrays A{T.Format, T.blknnz, T.blknnznnz, T.dnsrowptr, T.dnscolptr, T.tilewidth, T.csrptr_offset, T.hyb_coocount, T.new_coocount,
                       {T.csr_offset, T.coo_offset, T.ell_offset, T.hyb_offset, T.dns_offset, T.dnsrow_offset, T.dnscol_offset}, d_hyb_bytes};
    unsigned long long *d_totals = nullptr, h_totals[NS + 1] = {0};   // the scans' totals, and behind them the selection kernel's refusal (tilenum - the first refused tile; 0: none)
    if (dalloc(D, &d_totals, NS + 1, true)) return -3;
    if (tilenum > 0) {
        hipLaunchKernelGGL(k_tc_select, dim3(blocks_for(tilenum, 256)), dim3(256), 0, 0, tilenum, tilem, tilen, rowA, colA, allow_hyb, cdna4, T.tile_nnz, d_tile_bi, T.tile_columnidx, D->key, A, d_totals + NS);
        TC_TRY(hipGetLastError());
    }
    ScanSet S{};
    int *scans[] = {T.csr_offset, T.csrptr_offset, T.coo_offset, T.ell_offset, T.hyb_offset, T.dns_offset, T.dnsrow_offset, T.dnscol_offset, T.dnsrowptr, T.dnscolptr, T.hyb_coocount, T.new_coocount, T.blknnz, d_hyb_bytes};
    static const char *names[] = {"csr_offset", "csrptr_offset", "coo_offset", "ell_offset", "hyb_offset", "dns_offset", "dnsrow_offset", "dnscol_offset", "dnsrowptr", "dnscolptr", "hyb_coocount", "new_coocount", "blknnz", "hybIdx bytes"};
    for (int k = 0; k < NS; k++) S.a[k] = scans[k];
    hipLaunchKernelGGL(k_tc_totals, dim3((unsigned)std::min<long long>(2048, blocks_for((long long)np1, 256))), dim3(256), 0, 0, S, NS, (long long)np1, d_totals);
    TC_TRY(hipGetLastError());
    TC_TRY(hipMemcpy(h_totals, d_totals, sizeof(h_totals), hipMemcpyDeviceToHost));
    dfree(D, d_totals);
    if (h_totals[NS] != 0) {   // a tile with a repeated position and more entries than a tile serves (tile_select.h): nothing is packed
        const long long t = (long long)tilenum - (long long)h_totals[NS];
        int bi = 0, cb = 0, e01[2] = {0, 0};
        TC_TRY(hipMemcpy(&bi, d_tile_bi + t, sizeof(int), hipMemcpyDeviceToHost));
        TC_TRY(hipMemcpy(&cb, T.tile_columnidx + t, sizeof(int), hipMemcpyDeviceToHost));
        TC_TRY(hipMemcpy(e01, T.tile_nnz + t, 2 * sizeof(int), hipMemcpyDeviceToHost));
        fprintf(stderr, TILESPMV_TILE_REFUSAL_FMT, bi, cb, e01[1] - e01[0], TILE_REPEAT_MAX);
        return -2;
    }
    for (int k = 0; k < NS; k++)
        if (h_totals[k] > (unsigned long long)INT32_MAX) { fprintf(stderr, "tilespmv: %s exceeds the int32 offsets of Tile_matrix\n", names[k]); return -2; }
    {
        size_t tmp_b = 0; void *tmp = nullptr;
        TC_TRY(prims::scan_int(nullptr, tmp_b, scans[0], scans[0], np1, (hipStream_t)0));
        TC_TRY(hipMalloc(&tmp, std::max<size_t>(tmp_b, 16)));
        hipError_t e = hipSuccess;
        for (int k = 0; k < NS && e == hipSuccess; k++)
            if (h_totals[k] > 0) e = prims::scan_int(tmp, tmp_b, scans[k], scans[k], np1, (hipStream_t)0);   // (an all-zero array is its own scan)
        if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)0);
        free_now_or_later(tmp);
        TC_TRY(e);
    }
    T.csrsize = (int)h_totals[0]; T.csrptrlen = (int)h_totals[1]; T.coosize = (int)h_totals[2]; T.ellsize = (int)h_totals[3];
    T.hybsize = (int)h_totals[4]; T.hybcoosize = (int)h_totals[10]; T.hybellsize = T.hybsize - T.hybcoosize;   // (a HYB tile stores its ELL part + its remainder)
    D->hyb_byte_off = d_hyb_bytes;   // (scanned: per tile its first byte in hybIdx)
    if (T.hybsize > 0) {             // ... and as the 64-bit offsets the plan builders' per-tile functions take (plan_tile_ops.h hyb_off)
        long long *d_off64 = nullptr;
        if (dalloc(D, &d_off64, np1, true)) return -3;
        hipLaunchKernelGGL(k_tc_widen, dim3(blocks_for((long long)np1, 256)), dim3(256), 0, 0, (long long)np1, (const int *)d_hyb_bytes, d_off64);
        TC_TRY(hipGetLastError());
        D->hyb_off = d_off64;
    }
    T.dnssize = (int)h_totals[5]; T.dnsrowsize = (int)h_totals[6]; T.dnscolsize = (int)h_totals[7]; T.coototal = (int)h_totals[11];
    X.n_dnsrow = (long long)h_totals[8]; X.n_dnscol = (long long)h_totals[9]; X.hyb_idx_bytes = (long long)h_totals[13];
    D->ms_select = now_ms() - t0; t0 = now_ms();
    pool_end();

    // ---- payload arrays: one pool for the table's, the two one-byte-per-slot index arrays and the tile-ordered list of extracted entries
    const unsigned payload = TF_PAYLOAD | (want_deferred ? TF_EXTRACTED : 0u);
    {
        size_t bytes = fields_need(D, X, payload) + pool_need((size_t)T.csrsize, 1) + pool_need((size_t)T.ellsize, 1);
        if (want_deferred) bytes += 2 * pool_need((size_t)T.coototal, 4) + pool_need((size_t)T.coototal, sizeof(val_t));
        if (pool_begin(D, bytes)) return -3;
    }
    PackArrays P{};
    unsigned char *d_csr_col = nullptr, *d_ell_col = nullptr;
    if (dalloc_fields(D, X, payload) || dalloc(D, &d_csr_col, (size_t)T.csrsize, true) || dalloc(D, &d_ell_col, (size_t)T.ellsize, true)) return -3;
    if (want_deferred && (dalloc(D, &P.x_key, (size_t)T.coototal, true) || dalloc(D, &P.x_col, (size_t)T.coototal, true) || dalloc(D, &P.x_val, (size_t)T.coototal, true))) return -3;
    P.out = pack_out_of(T, d_csr_col, d_ell_col); P.hyb_byte_off = d_hyb_bytes; P.deferredcoo_ptr = T.deferredcoo_ptr;
    pool_end();
    TC_TRY(values.wait());   // the packing reads the values
    t_free_later = nullptr;
    for (void *q : later) (void)hipFree(q);
    later.clear();
    if (tilenum > 0) {
        hipLaunchKernelGGL(k_tc_pack, dim3(blocks_for(tilenum, 256)), dim3(256), 0, 0, tilenum, tilem, rowA, T, d_tile_bi, D->key, D->ent, d_colidx, d_val, P);
        TC_TRY(hipGetLastError());
    }
    if (T.csrsize > 0) hipLaunchKernelGGL(k_tc_nibbles, dim3(blocks_for(((long long)T.csrsize + 1) / 2, 256)), dim3(256), 0, 0, d_csr_col, T.csr_compressedIdx, (long long)T.csrsize);
    if (T.ellsize > 0) hipLaunchKernelGGL(k_tc_nibbles, dim3(blocks_for(((long long)T.ellsize + 1) / 2, 256)), dim3(256), 0, 0, d_ell_col, T.ell_compressedIdx, (long long)T.ellsize);
    TC_TRY(hipGetLastError());
    if (want_deferred) {
        // rows of the extracted matrix: counts -> pointers; entries: stable sort of the tile-ordered list by row = "order of appearance" inside every row (src/csr2tile.h:943-950)
        size_t tmp_b = 0; void *tmp = nullptr;
        TC_TRY(prims::scan_int(nullptr, tmp_b, T.deferredcoo_ptr, T.deferredcoo_ptr, (size_t)rowA + 1, (hipStream_t)0));
        TC_TRY(hipMalloc(&tmp, std::max<size_t>(tmp_b, 16)));
        hipError_t e = prims::scan_int(tmp, tmp_b, T.deferredcoo_ptr, T.deferredcoo_ptr, (size_t)rowA + 1, (hipStream_t)0);
        (void)hipDeviceSynchronize();
        (void)hipFree(tmp);
        TC_TRY(e);
        if (T.coototal > 0) {
            unsigned *key_b2 = nullptr; int *pos_a = nullptr, *pos_b = nullptr;
            if (dalloc(D, &key_b2, (size_t)T.coototal, false) || dalloc(D, &pos_a, (size_t)T.coototal, false) || dalloc(D, &pos_b, (size_t)T.coototal, false)) return -3;
            hipLaunchKernelGGL(k_tc_iota, dim3(blocks_for(T.coototal, 256)), dim3(256), 0, 0, T.coototal, pos_a);
            TC_TRY(hipGetLastError());
            unsigned *k_cur = P.x_key, *k_alt = key_b2; int *v_cur = pos_a, *v_alt = pos_b;
            const unsigned row_bits = (unsigned)bits_for(std::max(rowA, 2));
            tmp_b = 0; tmp = nullptr;
            TC_TRY(prims::sort_pairs_u32_int(nullptr, tmp_b, k_cur, k_alt, v_cur, v_alt, (size_t)T.coototal, 0u, row_bits, (hipStream_t)0));
            TC_TRY(hipMalloc(&tmp, std::max<size_t>(tmp_b, 16)));
            e = prims::sort_pairs_u32_int(tmp, tmp_b, k_cur, k_alt, v_cur, v_alt, (size_t)T.coototal, 0u, row_bits, (hipStream_t)0);
            if (e == hipSuccess) {
                hipLaunchKernelGGL(k_tc_deferred, dim3(blocks_for(T.coototal, 256)), dim3(256), 0, 0, T.coototal, (const int *)v_cur, (const int *)P.x_col, (const val_t *)P.x_val, T.deferredcoo_colidx, T.deferredcoo_val);
                e = hipGetLastError();
            }
            if (e == hipSuccess) e = hipDeviceSynchronize();
            (void)hipFree(tmp);
            TC_TRY(e);
            dfree(D, key_b2); dfree(D, pos_a); dfree(D, pos_b);
            int *d_cnt = nullptr;
            if (dalloc(D, &d_cnt, 1, true)) return -3;
            hipLaunchKernelGGL(k_tc_unsorted_rows, dim3(blocks_for(rowA, 256)), dim3(256), 0, 0, rowA, (const int *)T.deferredcoo_ptr, (const int *)T.deferredcoo_colidx, d_cnt);
            TC_TRY(hipGetLastError());
            TC_TRY(hipMemcpy(&D->unsorted_rows, d_cnt, sizeof(int), hipMemcpyDeviceToHost));
            dfree(D, d_cnt);
        }
        dfree(D, P.x_key); dfree(D, P.x_col); dfree(D, P.x_val);
        D->have_deferred = true;
    }
    TC_TRY(hipDeviceSynchronize());
    dfree(D, d_csr_col); dfree(D, d_ell_col);
    D->ms_pack = now_ms() - t0;
    if (verbose)
        fprintf(stderr, "tilespmv: device Tile_create: upload of the index arrays %.1f ms (the values cross the bus behind the next three steps), keys + sort %.1f, tile list %.1f, selection + scans %.1f, packing %.1f (%d tiles, %lld nonzeros)\n", D->ms_upload, D->ms_sort, D->ms_tiles,
                D->ms_select, D->ms_pack, tilenum, nnz);
    return 0;
}

}  // namespace

int devtile_create(DevTile **out, int rowA, int colA, const MAT_PTR_TYPE *h_rowptr, const int *h_colidx, const val_t *h_val, unsigned flags, bool want_deferred, bool csr_on_device, bool stand_in_values,
                   const int *stand_in_pos)
{
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); fprintf(stderr, "tilespmv: no HIP device visible — the device Tile_create has no CPU fallback (use Tile_create)\n"); return -1; }
    DevTile *D = new DevTile();
    const int rc = create_impl(D, rowA, colA, h_rowptr, h_colidx, h_val, flags, want_deferred, csr_on_device, stand_in_values, stand_in_pos);
    pool_end();
    if (rc != 0) { devtile_destroy(D); return rc; }
    *out = D;
    return 0;
}

void devtile_destroy(DevTile *D)
{
    if (!D) return;
    for (void *p : D->allocs) (void)hipFree(p);
    for (void *p : D->pools) (void)hipFree(p);
    delete D;
}



int devtile_download(const DevTile *D, Tile_matrix *H)
{
    const Tile_matrix &T = D->T;
    memset(H, 0, sizeof(*H));
    copy_tile_scalars(*H, T);
    int rc = 0;
    auto get = [&](const TileField &f) {   // a host array for the member, slack included, filled from the device's (a member the device never built stays zero)
        zalloc_tile_field(f);
        const void *src = same_tile_field(T, *H, f);
        const size_t bytes = (size_t)(f.count + f.slack) * f.elem;
        if (bytes && src && hipMemcpy(*f.ptr, src, bytes, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); rc = -3; }
    };
    TileExtents X; X.rowA = D->rowA;
    for_each_tile_field(*H, X, TF_LIST | TF_TILE, get);   // the per-tile arrays first: two of them say how long the id arrays are
    if (T.tilenum) { X.n_dnsrow = H->dnsrowptr[T.tilenum]; X.n_dnscol = H->dnscolptr[T.tilenum]; X.hyb_idx_bytes = hyb_idx_bytes(*H, D->rowA); }
    for_each_tile_field(*H, X, TF_PAYLOAD, get);
    if (D->have_deferred) {
        for_each_tile_field(*H, X, TF_EXTRACTED, get);
        if (rc == 0 && D->unsorted_rows > 0)   // rows whose columns do not increase (unsorted CSR input): the reference's pivot sort, on the host (src/csr2tile.h:951-958, src/utils.h:103-137)
            parallel_chunks(D->rowA, 4096, [&](int64_t b, int64_t e, int) {
                for (int64_t r = b; r < e; r++) {
                    const int p = H->deferredcoo_ptr[r], len = H->deferredcoo_ptr[r + 1] - p;
                    int *k = H->deferredcoo_colidx + p;
                    bool increasing = true;
                    for (int i = 1; i < len && increasing; i++) increasing = k[i - 1] < k[i];
                    if (!increasing) pivot_sort(k, H->deferredcoo_val + p, len);
                }
            });
    } else {
        H->deferredcoo_val = zalloc<val_t>(0); H->deferredcoo_colidx = zalloc<int>(0); H->deferredcoo_ptr = zalloc<int>((size_t)D->rowA + 1);
    }
    return rc;
}

}  // namespace tilespmv

extern "C" int Tile_create_device(Tile_matrix *matrix, int rowA, int colA, MAT_PTR_TYPE nnzA, const MAT_PTR_TYPE *csrRowPtrA, const int *csrColIdxA, const MAT_VAL_TYPE *csrValA, unsigned flags)
{
    (void)nnzA;   // like Tile_create, the row pointer decides how many nonzeros are used
    tilespmv::DevTile *D = nullptr;
    tilespmv::DevCsrT Tr;   // (TILESPMV_CREATE_TRANSPOSE: A^T transposed on the device, hip_transpose.hip; the tiled matrix is built from those device arrays)
    int rc;
    if (flags & TILESPMV_CREATE_TRANSPOSE) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); fprintf(stderr, "tilespmv: no HIP device visible — the device Tile_create has no CPU fallback (use Tile_create)\n"); return -1; }
        rc = tilespmv::devcsr_transpose(&Tr, rowA, colA, csrRowPtrA, csrColIdxA, csrValA, false, true, false, false);
        if (rc == 0) rc = tilespmv::devtile_create(&D, colA, rowA, Tr.rp, Tr.ci, Tr.v, flags, true, true);
    } else
        rc = tilespmv::devtile_create(&D, rowA, colA, csrRowPtrA, csrColIdxA, csrValA, flags, true);
    if (rc != 0) return rc;
    rc = tilespmv::devtile_download(D, matrix);
    tilespmv::devtile_destroy(D);
    if (rc != 0) Tile_destroy(matrix);
    return rc;
}
