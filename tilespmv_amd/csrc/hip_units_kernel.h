// hip_units_kernel.h — the unit-stream kernel k_units (hip_plan.h "unit stream") and the device helpers it needs, shared by the translation units that
// instantiate it: hip_kernels.hip (every form whose values are val_t or floats), hip_kernels_half.hip (fp64 build: the four forms whose values are halves) and
// hip_kernels_lean.hip (the lean forms for plans without row units, every value form: UNITS_LEAN below).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "hip_plan.h"

namespace tilespmv {

// LDS scatter accumulators are fp64 in BOTH builds: on gfx950 a wavefront's ds_add_f32 takes about 170 cycles whatever the address
// pattern, its ds_add_f64 7-18 (scripts/micro/lds_atomic_rate.hip: 203 against 1860-4670 G adds/s) — the fp32 build's entry phase
// spent 0.108 ms of a 0.166 ms SpMV (power-law 8 M rows) in them.  Products are formed in the value type and widened for the add;
// sums of integer-valued data stay exact, real-valued sums get closer to the exact result than a float chain would.
typedef double lacc_t;

// ---- 16-lane all-reduce with DPP row rotations (a DPP "row" is exactly one 16-lane strip)
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, false);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
template <class T>
__device__ __forceinline__ T strip_allreduce(T v)
{
    v += dpp_mov<0x128>(v);  // row_ror:8
    v += dpp_mov<0x124>(v);  // row_ror:4
    v += dpp_mov<0x122>(v);  // row_ror:2
    v += dpp_mov<0x121>(v);  // row_ror:1
    return v;
}

__device__ __forceinline__ void wave_lds_fence()
{
    // LDS operations of one wavefront complete in issue order; this only stops the compiler
    // from moving accesses across the point where other lanes' data is consumed.
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ================================================================================================
// Second generation: unit-stream kernel (layout: hip_plan.h "unit stream").
// One 16-lane strip per task as before, but the common formats are consumed as a flat run of
// self-describing 16-value units whose addresses depend only on the unit index:
//   phase 1  COO entry list of the strip -> LDS scatter-add (ds_add) into s_y[strip row][row]
//   phase 2  units in batches of UB: descriptors come from LDS (one coalesced load per 16 units), the
//            x gathers of a batch are issued at once, the next batch's value loads go in flight before
//            the first use; a finished tile-row parks its 16 results in LDS and y is written once per
//            strip with 16-B lane stores.
// Dense tiles for the matrix cores (k_dense_mfma) and CSR tiles kept whole (k_tiles_direct<.., ACCUM>)
// run after this kernel, which keeps it at 60 VGPRs (8 waves/SIMD).
// ================================================================================================

template <bool NT, class T>
__device__ __forceinline__ T stream_load(const T *p)
{
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}

// 12-B descriptor in HBM -> the 16-B form the strip parks in LDS (both halves carry word 0)
__device__ __forceinline__ uint4 load_udesc(const UDesc *__restrict__ d, int i)
{
    const UDesc u = d[i];
    return make_uint4(u.w0, u.n0, u.w0, u.n1);
}

// ... and the same descriptor as it is held in registers while it waits for its turn (k_units): the three loaded words as they arrive, (w0, n0, n1, -).  Building the LDS form
// right behind the load needs a register move of w0, and the move needs the load's data: the wavefront then waits a full memory round trip for a prefetch it
// will not use for four batches (that is what the 12-byte-descriptor kernels did until round 5).  The LDS form is built when the chunk is parked.
__device__ __forceinline__ uint4 load_udesc_raw(const UDesc *__restrict__ d, int i)
{
    const UDesc u = d[i];
    return make_uint4(u.w0, u.n0, u.n1, 0u);
}
__device__ __forceinline__ uint4 udesc_park_form(const uint4 raw) { return make_uint4(raw.x, raw.y, raw.x, raw.z); }

// Dictionary plans (DevStream::cb_bits > 0; hip_plan.hip): 4 B per unit in HBM — column block | pattern id << cb_bits |
// flags << 27 — and the unit's column pattern (the two nibble words) in a small dictionary that stays in the vector L1.
// A lane expands its unit's descriptor to the 16-B LDS form when the chunk is parked.
__device__ __forceinline__ uint4 udict_of(const DevStream &S, unsigned w) { return S.udict[(w << 5) >> (5 + S.cb_bits)]; }   // (nibbles of rows 0-7, of rows 8-15, window shift << 29, 0)
// pooled dictionary plans: descriptor of unit i as (word 0 = window base | tile-row in strip << POOL_KR_SHIFT, pattern id) — from the 8-byte pair, or (S.cb_bits = b > 0) from the
// 4-byte word base | id << b | tile-row << 30 (hip_plan.h)
__device__ __forceinline__ uint2 pool_desc(const DevStream &S, int i)
{
    const int b = S.cb_bits;
    if (b > 0) {
        const unsigned a = reinterpret_cast<const unsigned *>(S.udesc)[i];
        return make_uint2((a & ((1u << b) - 1u)) | ((a >> POOL_WORD_KR_SHIFT) << POOL_KR_SHIFT), (a << (32 - POOL_WORD_KR_SHIFT)) >> (32 - POOL_WORD_KR_SHIFT + b));
    }
    return reinterpret_cast<const uint2 *>(S.udesc)[i];
}
__device__ __forceinline__ uint4 udesc_expand(const DevStream &S, unsigned w, uint4 pat)
{
    const unsigned w0 = (w & ((1u << S.cb_bits) - 1u)) | ((w >> 27) << UNIT_FLAG_SHIFT) | pat.z;   // (pat.z: the pattern's window shift, already at UNIT_SHIFT_SHIFT)
    return make_uint4(w0, pat.x, w0, pat.y);
}
// DERIVED units (hip_plan.h UNIT_DERIVED_CODE, plan_tile_ops.h): lanes 0-14 of the strip use the x the previous unit used one lane up (DPP row rotation: a DPP row is one strip),
// lane 15 the value it loaded itself; every other unit uses what it gathered.  `prev` = the x the previous unit of this strip used.
template <class X>
__device__ __forceinline__ X unit_x_use(X gathered, X prev, unsigned w0, int r)
{
    const X up = dpp_mov<0x12F>(prev);   // row_ror:15 = lane i reads lane i + 1
    return ((w0 >> UNIT_SHIFT_SHIFT) == UNIT_DERIVED_CODE && r != 15) ? up : gathered;
}
// first column of a classic unit's window of x: column block * 16, moved by the signed shift of a unit that took list entries (hip_plan.h UNIT_SHIFT_SHIFT)
__device__ __forceinline__ long long unit_x_base(unsigned w0) { return (long long)(w0 & 0xFFFFFFu) * 16 + ((int)w0 >> UNIT_SHIFT_SHIFT); }
// ... the same in 32 bits (24 bits of column block * 16 + a shift of -4 .. 3: below 2^28 + 3), and the clamped index of a gather: a window offset below 256 on top of a base below
// 2^28.  The plan's nibbles and offsets never point in front of column 0 (plan_tile_ops.h: a window starts at its lowest used column), so the index is an unsigned number.
__device__ __forceinline__ int unit_x_base32(unsigned w0) { return (int)((w0 & 0xFFFFFFu) << 4) + ((int)w0 >> UNIT_SHIFT_SHIFT); }
__device__ __forceinline__ unsigned x_index32(int base, unsigned off, int xlast) { return (unsigned)min(base + (int)off, xlast); }

// Descriptor word layout in LDS (16 B per unit, two identical-purpose halves so that a lane reads 8 B; HBM holds the
// 12-B form without the duplicate word, UDesc):
//   word 0 / word 2 : column block (24 bits) | flags << 24   (flag bit 0 = end of tile-row, bits 1-3 = row in strip,
//                     bit 4 = row unit, bits 5-7 = signed shift of the unit's window of x: a unit that took list entries, plan_tile_ops.h)
//   word 1          : column nibbles of rows 0-7  (row 0 in the top nibble)   [row unit: target row]
//   word 3          : column nibbles of rows 8-15
// Descriptors reach the lanes through LDS: one coalesced 16-B-per-lane load brings the descriptors of 16
// consecutive units (lane j loads unit j's), the strip parks them in LDS and every unit then costs one
// ds_read_b64 instead of one global load.  (Measured: per-unit descriptor loads, 6 % of the bytes, cost 19 %
// of the kernel — the CU's vector-memory pipeline is the bottleneck, not HBM)
constexpr int DCHUNK = 16;  // units per descriptor chunk
typedef unsigned v4u_t __attribute__((ext_vector_type(4)));
typedef unsigned v2u_t __attribute__((ext_vector_type(2)));
#ifndef NT_Y
#define NT_Y 1  // y is written once and not re-read by this kernel: streaming (nontemporal) stores keep it from displacing x in L2 (+1-2 %; per plan: DevStream::y_streaming)
#endif
#ifndef WCOO_HEAVY_CT
#define WCOO_HEAVY_CT 6  // sub-chunks (of 64 / 256 entries) per trip of the wavefront / workgroup entry phase
#endif
#ifndef MV_MIN_WAVES
#define MV_MIN_WAVES 6  // multi-vector kernel: 80 VGPRs (5 waves: 84 VGPRs, nvec 8 0.79 ms; 6: 0.74 ms; 7 spills: 1.01 ms)
#endif
#ifndef ECOO2_MIN_WAVES
#define ECOO2_MIN_WAVES 6  // workgroup entry mode: 80 VGPRs
#endif
#ifndef TILESPMV_UB
#define TILESPMV_UB 4   // units per batch of the unit loop (8 with UNITS_MIN_WAVES=6 measured below)
#endif
#ifndef UNITS_MIN_WAVES
#define UNITS_MIN_WAVES 8  // waves per SIMD asked of the register allocator (64 VGPRs)
#endif
#ifndef UNIT_X32
#define UNIT_X32 1   // x index of a unit's gather in 32 bits (column block * 16 + shift + nibble < 2^28 + 19, colA is an int): one signed min, one 64-bit scale-and-add (0: 64-bit base, add, compare and two selects).  405 -> 373 instructions per batch in the hot narrow kernel; config 4 0.1190 -> 0.1182 ms: profiles/unit_loop_pipeline_ab.txt
#endif
#ifndef UNIT_TAIL_HOT
#define UNIT_TAIL_HOT 1   // the value prefetch of a task's last iteration (there is no next batch; the load stays for the exact vmcnt) reads the plan's first 16 bytes — one word, the same for every lane of every task — instead of the task's last group once more (0), a second trip to memory for 256 B per strip of a stream that is not kept in the caches.  With UNIT_X32: config 4 0.1169 -> 0.1133 / 0.1153 ms, KKT fp32 -5.5 %: profiles/unit_loop_pipeline_ab.txt
#endif
#ifndef POOL_ECOO2_MIN_WAVES
#define POOL_ECOO2_MIN_WAVES 5   // pooled plans, workgroup entry mode: 96 VGPRs (at 6 waves = 80 VGPRs the kernel spills 12 bytes)
#endif
#ifndef POOL_MIN_WAVES
#define POOL_MIN_WAVES 7   // pooled plans, per-strip entries: 14.5 KB of LDS per workgroup; 72 VGPRs (at 8 waves = 64 VGPRs the kernel spills 20 bytes and runs slower)
#endif

// ---- packed entry records (hip_plan.h ERec): value + (column - chunk base) << dest_bits | destination
__device__ __forceinline__ val_t erec_val(const ERec &r)
{
#if defined(TILESPMV_F32)
    return __uint_as_float(r.v);
#else
    return __hiloint2double((int)r.hi, (int)r.lo);
#endif
}

// ---- wave-cooperative entry phase of k_units<.., 1>: the COO entry lists of the wavefront's four strips, merged and ordered
// by column at plan time, are walked by all 64 lanes; products go to the owning strip's slab of the wavefront's part of
// s_y with ds_add (destination = strip-in-wavefront << 7 | row byte).  A wavefront's time follows its TOTAL entry
// count, not its longest strip; every load is a full 64-lane access; neighbouring lanes of a gather read the same or
// adjacent x lines, and the four wavefronts of a workgroup sweep the columns side by side, so they find each other's lines
// in the CU's L1.  Only this wavefront adds into its slabs: the order of the additions is fixed by the plan (bit-
// reproducible).  CT x 64 entries per trip: every record load of a trip (one 12-/8-byte lane load each; the chunk's column
// base comes through the scalar cache), then its gathers, then the adds.
template <int CT>
__device__ __forceinline__ void wave_entry_trips(const DevStream &S, const val_t *__restrict__ x, lacc_t *swave, int lane, int gb, int ge, int chunk0, int cfirst)
{
    const int db = S.dest_bits;
    const unsigned dmask = (1u << db) - 1u;
    const int clast = chunk0 + ((ge - 1 - gb) >> 6);
    for (int e0 = gb + 64 * cfirst; e0 < ge; e0 += 64 * CT) {
        ERec rr[CT]; unsigned cb[CT]; val_t xx[CT];
#pragma unroll
        for (int q = 0; q < CT; q++) {
            rr[q] = S.grec[min(e0 + 64 * q + lane, ge - 1)];
            cb[q] = S.gbase[__builtin_amdgcn_readfirstlane(min(chunk0 + ((e0 - gb) >> 6) + q, clast))];
        }
#pragma unroll
        for (int q = 0; q < CT; q++) xx[q] = x[(size_t)(cb[q] + (rr[q].w >> db))];
#pragma unroll
        for (int q = 0; q < CT; q++)
            if (e0 + 64 * q + lane < ge) atomicAdd(&swave[rr[q].w & dmask], (lacc_t)(erec_val(rr[q]) * xx[q]));
    }
}

// ---- workgroup-cooperative entry phase of k_units<.., 2> (and of the fallback kernel): the entries of the workgroup's 16 or
// 32 strips, merged and ordered by column at plan time, walked by all NT lanes.  Neighbouring lanes of a gather then read
// the same or adjacent x lines: on power-law matrices the number of distinct x lines per batch drops from 0.48 per entry (one
// strip at a time) to 0.15 (64 tile-rows at a time), and the CU's L1 -> L2 request rate is what bounds those matrices.
#ifndef WG_TRIP_PIPE
#define WG_TRIP_PIPE 0   // 1: the next trip's records are requested behind the current trip's gathers.  Measured (profiles/r03_entry_ablations.txt): power-law 8 M 0.1039 -> 0.1065 ms, KKT fp64 0.427 -> 0.435, webbase 13.1 -> 12.9 us at 4 x 256 per trip; 6 x 256 spills.  Off.
#endif
// NTL: the records are read with nontemporal loads (plans whose streams do not fit the Infinity Cache: the once-read stream
// then does not displace x in the L2s; DevStream::nt_stream).

template <int CT, int NT, bool NTL>
__device__ __forceinline__ void wg_entry_trips(const ERec *__restrict__ rec, const unsigned *__restrict__ base, int chunk0, int db, bool ordered,
                                               const val_t *__restrict__ x, lacc_t *sy, int tid, int gb, int ge, int gs = -1)
{
    // [gs, ge) = the records to execute; gb = the list's begin, which chunk numbers count from (column panels execute a run that starts inside the list, even inside a chunk)
    if (gs < 0) gs = gb;
    const int e_first = gb + ((gs - gb) & ~63);
    const unsigned dmask = (1u << db) - 1u;
    const int wave = tid >> 6;
    const int clast = chunk0 + ((ge - 1 - gb) >> 6);
    ERec rr[CT]; unsigned cb[CT];
    auto load_trip = [&](int e0, ERec (&r)[CT], unsigned (&c)[CT]) {   // unconditional, clamped: exact vmcnt
#pragma unroll
        for (int q = 0; q < CT; q++) {
            if constexpr (NTL) {   // (the adjacent nontemporal dword loads become one global_load_dwordx3 / dwordx2 nt)
                const unsigned *pw = reinterpret_cast<const unsigned *>(&rec[min(e0 + NT * q + tid, ge - 1)]);
                unsigned *rw = reinterpret_cast<unsigned *>(&r[q]);
#pragma unroll
                for (int z = 0; z < (int)(sizeof(ERec) / 4); z++) rw[z] = __builtin_nontemporal_load(pw + z);
            } else r[q] = rec[min(e0 + NT * q + tid, ge - 1)];
            c[q] = base[__builtin_amdgcn_readfirstlane(min(chunk0 + ((e0 - gb) >> 6) + (NT / 64) * q + wave, clast))];   // a wavefront's 64 records are one chunk
        }
    };
    if (e_first < ge) load_trip(e_first, rr, cb);
    for (int e0 = e_first; e0 < ge; e0 += NT * CT) {
        val_t xx[CT];
        if (!WG_TRIP_PIPE && e0 > e_first) load_trip(e0, rr, cb);
#pragma unroll
        for (int q = 0; q < CT; q++) xx[q] = x[(size_t)(cb[q] + (rr[q].w >> db))];
        // the next trip's records go in flight behind this trip's gathers (loads return in issue order: the gathers are waited
        // for with the prefetch still outstanding); the last trip re-requests its own (clamped) records, which costs nothing
        ERec rn[CT]; unsigned cn[CT];
        if (WG_TRIP_PIPE) load_trip(min(e0 + NT * CT, gb + (ge - 1 - gb) / (NT * CT) * (NT * CT)), rn, cn);
        if (ordered) {
            // the wavefronts add in turn: the order of the additions into one y element is then fixed by the plan (entry
            // order inside a wavefront instruction, instruction order inside a wavefront, wavefront 0..NT/64-1 inside a trip), not
            // by timing, and two launches give the same bits (the reference's atomicAdd, src/tilespmv_cuda.h:784-790, does not)
            for (int w = 0; w < NT / 64; w++) {
                if (wave == w) {
#pragma unroll
                    for (int q = 0; q < CT; q++)
                        if (e0 + NT * q + tid < ge && e0 + NT * q + tid >= gs) atomicAdd(&sy[rr[q].w & dmask], (lacc_t)(erec_val(rr[q]) * xx[q]));
                }
                __syncthreads();
            }
        } else {
#pragma unroll
            for (int q = 0; q < CT; q++)
                if (e0 + NT * q + tid < ge && e0 + NT * q + tid >= gs) atomicAdd(&sy[rr[q].w & dmask], (lacc_t)(erec_val(rr[q]) * xx[q]));
        }
        if (WG_TRIP_PIPE) {
#pragma unroll
            for (int q = 0; q < CT; q++) { rr[q] = rn[q]; cb[q] = cn[q]; }
        }
    }
}

// ECOO: how the COO entry lists are executed — 0 per 16-lane strip (regular matrices: a handful of entries per strip),
// 1 per wavefront (the four strips' lists concatenated), 2 per workgroup (merged + column-ordered list, see above).
// GPB: strips (16-lane groups) per workgroup — 16 (256 threads) or, for the workgroup entry mode on large entry-heavy shards, 32
// (512 threads: twice as many tile-rows share one column-ordered list, so fewer distinct x lines per entry; same waves per SIMD).
// (Retired in round 6, both measured slower than what replaced them: x windows staged in LDS — DESIGN S6.9 — and the slab-paced entry phase — S6.17.  The XCD remap is a run-time
// scalar branch now (xcd_chunk > 0) instead of a template axis.)
extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
// CD: dictionary plans (4-B descriptors, above).  The descriptor words are loaded two chunks ahead, the pattern of a chunk is
// gathered from the dictionary one chunk ahead (when its word has arrived), so neither hop is waited for in the unit loop.
// NTS: value and entry-record loads are nontemporal (plans larger than the Infinity Cache, DevStream::nt_stream).
// POOL: pooled plans (hip_plan.h "pooled units", round 5): a unit is up to 16 nonzeros of a tile-row inside one 16-column window of x — slot s = value, column-offset nibble, row nibble —
// so a lane no longer owns a row: it gathers x[base + its column nibble] and adds its product to the strip's slab of s_y with ds_add (destination = tile-row in strip, its row
// nibble); there is no register accumulator, no end-of-row handling and no "rows without units": the slab is zeroed up front, entries and units add into it, y is stored from it.
// The row nibbles travel like the descriptors (8 bytes per unit, one coalesced lane load per chunk of 16 units, parked in LDS: + 2 KB per workgroup -> 7 workgroups per CU).
// WIDE (with POOL; hip_plan.h "wide pooled units", csr_form 3): windows of 256 columns — a slot's column offset is a byte (16 bytes per unit in S.ucol, parked in s_c), the descriptor's nibble words hold the ROW nibbles.
// NARROW (fp64 build; DevStream::uval_narrow): the plan's unit values are floats in groups of 4 units — one 16-byte lane load per batch instead of two —, widened in registers;
// the arithmetic is the wide kernel's.  Classic plans, entry mode 0 / 2, 16 strips per workgroup, nontemporal streams.
// Halves (DevStream::uval_narrow 2): one 8-byte lane load per batch, which waits as 2 VGPRs and is widened half -> float -> double, both exact, when the batch becomes the current
// one.  The four kernels of that form are this template under another name in a translation unit of their own (hip_kernels_half.hip), which sets the two macros below before it
// includes this header; the kernels of hip_kernels.hip do not change by a line for it.
#if defined(UNITS_LEAN) ? (!defined(UNITS_KERNEL) || defined(UNITS_NARROW_FORM)) : (defined(UNITS_KERNEL) != defined(UNITS_NARROW_FORM))
#error "hip_units_kernel.h: define UNITS_KERNEL and UNITS_NARROW_FORM together (or neither: k_units, floats); UNITS_LEAN goes with UNITS_KERNEL alone (the value form is a template argument there)"
#endif
#if !defined(UNITS_KERNEL) && !defined(UNITS_LEAN)
#define UNITS_KERNEL k_units      // the kernel's name in the including translation unit
#define UNITS_NARROW_FORM 1       // ... and what NARROW means there: DevStream::uval_narrow 1 (floats) or 2 (halves)
#endif
// (halves, workgroup entry mode: 8 waves per SIMD like the per-strip form — the unit prologue is issued behind the entry phase, see there)
// UNITS_LEAN (hip_kernels_lean.hip): the lean forms, for classic plans in which NO unit is a row unit (DevStream::unit_facts).  The template then takes the value form
// (VF = DevStream::uval_narrow) and DERIVED ("some unit is derived") as arguments in place of POOL / WIDE / NARROW, and what only a row unit needs (its identity nibbles in the
// gather, the 16-lane all-reduce in `retire`) or, with DERIVED off, only a derived unit needs (unit_x_use, xprev, the test in front of the gather) is compiled out.  Their unit
// loop is peeled (below).  Loads, waits and LDS accesses are where the general kernel has them and the arithmetic is its multiply-then-add in unit order: y is the general
// kernel's bit for bit.  Every lean form asks for 8 waves per SIMD; in the workgroup entry mode they issue the unit prologue behind the entry phase, like the halves.
#ifdef UNITS_LEAN
template <int UB, int ECOO, int GPB, bool CD, bool NTS, int VF, bool DERIVED>
__global__ __launch_bounds__(16 * GPB, UNITS_MIN_WAVES) void UNITS_KERNEL(DevStream S, int rowA, int colA, int xcd_chunk, val_t *__restrict__ partial,
                                               const val_t *__restrict__ x, val_t *__restrict__ y)
{
    constexpr bool LEAN = true, POOL = false, WIDE = false, NARROW = VF != 0, ROWUNITS = false;
    constexpr int VFORM = VF;
    static_assert(ECOO != 1 && GPB == 16 && NTS && VF >= 0 && VF <= (sizeof(val_t) == 8 ? 2 : 0), "lean forms: entry mode 0 / 2, 16 strips, nontemporal streams, a value form of this build");
#else
template <int UB, int ECOO, int GPB, bool CD, bool NTS, bool POOL = false, bool WIDE = false, bool NARROW = false>
__global__ __launch_bounds__(16 * GPB, ECOO == 1 ? 4 : ECOO == 2 ? (POOL ? POOL_ECOO2_MIN_WAVES : NARROW && UNITS_NARROW_FORM == 2 ? UNITS_MIN_WAVES : ECOO2_MIN_WAVES) : POOL ? (WIDE ? 6 : POOL_MIN_WAVES) : UNITS_MIN_WAVES) void UNITS_KERNEL(DevStream S, int rowA, int colA, int xcd_chunk, val_t *__restrict__ partial,
                                               const val_t *__restrict__ x, val_t *__restrict__ y)
{
    constexpr bool LEAN = false, ROWUNITS = true, DERIVED = true;   // the general forms serve every plan
    constexpr int VFORM = NARROW ? UNITS_NARROW_FORM : 0;   // DevStream::uval_narrow of the plans this instantiation runs
#endif
    static_assert(VFORM >= 0 && VFORM <= 2, "UNITS_NARROW_FORM: 1 or 2");
    static_assert(!NARROW || (sizeof(val_t) == 8 && !POOL && ECOO != 1 && GPB == 16 && NTS), "narrow values: fp64 classic plans, entry mode 0 / 2, 16 strips, nontemporal streams");
    constexpr int G = NARROW ? UNIT_GROUP_NARROW : UNIT_GROUP;   // units whose values share one 16-byte lane load
    static_assert(DCHUNK % UB == 0 && UB % G == 0, "a batch never straddles a descriptor chunk and is whole value groups");
    static_assert(GPB == 16 || (GPB == 32 && ECOO == 2) || (GPB == 8 && ECOO != 2 && !NTS), "512-thread workgroups exist for the workgroup entry mode only, 128-thread ones for small grids without it");
    static_assert(!(NTS && ECOO == 1), "nontemporal streams: large plans only (entry mode 1 = small grids)");
    static_assert(!POOL || GPB == 16 || GPB == 8, "pooled plans: 256-thread workgroups (128 on small grids)");
    static_assert(!WIDE || (POOL && !CD), "wide windows: pooled plans, 12-B descriptors + 16 B of column offsets");
    constexpr int GROUPS_PER_BLOCK = GPB;
    constexpr int SROWS = POOL ? POOL_STRIP_ROWS : STRIP_MAX_ROWS;   // tile-rows per strip the LDS slabs are sized for
    constexpr bool NT = NTS;  // nontemporal value loads
#ifndef TILESPMV_NT_DESC
#define TILESPMV_NT_DESC 0
#endif
#ifndef TILESPMV_NT_COO0
#define TILESPMV_NT_COO0 0
#endif
    constexpr bool NT_DESC = NTS && TILESPMV_NT_DESC, NT_COO0 = NTS && TILESPMV_NT_COO0;
    // Pooled plans of the fp32 build keep a SECOND copy of the slabs (PCOPY): the slots of a unit are in row order, so the nonzeros of one row sit in neighbouring lanes, and lanes of
    // odd / even slot add into different copies — two lanes of one LDS atomic then (almost) never hit one address.  A same-address pair costs the fp32 build a quarter of its time
    // (fem3_68: 0.119 ms, 0.088 with lane-private addresses: profiles/r05_pool_ablations.txt; the fp64 build is bound by its bytes and gains nothing).  The copy sits 16 doubles
    // off a multiple of the bank count, so that the two halves of a pair also fall into different banks; the copies are summed when the strip is done.
    constexpr bool PCOPY = POOL && sizeof(val_t) == 4;
    constexpr int SLAB = GROUPS_PER_BLOCK * SROWS * 16;
    __shared__ lacc_t s_yall[SLAB + (PCOPY ? SLAB + 16 : 0)];   // (lacc_t: fp64 in both builds, see its typedef)
    lacc_t (*s_y)[SROWS][16] = reinterpret_cast<lacc_t (*)[SROWS][16]>(&s_yall[0]);
    lacc_t *s_y1 = &s_yall[PCOPY ? SLAB + 16 : 0];
    __shared__ uint4 s_d[GROUPS_PER_BLOCK][DCHUNK];
    __shared__ uint2 s_r[POOL && !WIDE ? GROUPS_PER_BLOCK : 1][POOL && !WIDE ? DCHUNK : 1];   // pooled plans: row nibbles of the parked descriptor chunk
    __shared__ uint4 s_c[WIDE ? GROUPS_PER_BLOCK : 1][WIDE ? DCHUNK : 1];                   // wide pooled plans: column-offset bytes of the parked chunk
    const int tid = threadIdx.x, r = tid & 15, g = tid >> 4;
    // Workgroups are dealt round-robin over the 8 XCDs (blockIdx % 8 labels the XCD group), each
    // with a private L2; xcd_chunk > 0 gives every XCD runs of xcd_chunk consecutive workgroups inside
    // windows of 8 x xcd_chunk (bijective for any grid size, cdna_hip_programming.md T1).  Speed only.
    unsigned bid = blockIdx.x;
    if (xcd_chunk > 0) {   // (kernel argument: a scalar branch)
        const unsigned C = (unsigned)xcd_chunk, W = 8u * C, win = bid / W, off = bid % W, k = off & 7u;
        if ((win + 1) * W <= gridDim.x) bid = win * W + k * C + (off >> 3);
    }
    const long long task_id = (long long)bid * GROUPS_PER_BLOCK + g;
    const bool have = task_id < S.ntasks;
    constexpr bool WCOO = ECOO == 1;
    if (ECOO == 1) { if ((long long)bid * GROUPS_PER_BLOCK + (g & ~3) >= S.ntasks) return; }  // whole wavefronts leave together (wave-cooperative entry phase)
    else if (ECOO == 0 && !have) return;                                                      // ECOO == 2: every wavefront reaches the barriers
    int4 t0 = make_int4(0, 0, 0, 0), t1 = make_int4(0, -1, 0, 0);
    if (have) {
        t0 = reinterpret_cast<const int4 *>(S.task)[task_id * 2];
        t1 = reinterpret_cast<const int4 *>(S.task)[task_id * 2 + 1];
    }
    const int unit_begin = t0.x, unit_end = t0.y, coo_begin = t0.z, coo_end = t0.w;
    const int row0 = t1.x, part = t1.y, nrows = t1.w;
    const unsigned nounit = (unsigned)t1.z;
    const bool side = POOL || coo_end > coo_begin;   // the strip's slab of s_y holds sums (entries; in pooled plans everything)
    if constexpr (POOL) {   // the slab is zeroed before anything adds into it (the entry phases below sit behind a fence / barrier of their own)
        for (int k = 0; k < nrows; k++) { s_y[g][k][r] = 0; if constexpr (PCOPY) s_y1[(g * SROWS + k) * 16 + r] = 0; }
        wave_lds_fence();
    }
    // values are stored in groups of G = UNIT_GROUP units of one task (hip_plan.hip): row r of the group that starts at
    // task-relative unit j (a multiple of G) sits at uval[(unit_begin + j) * 16 + G r .. + G - 1]; a batch of UB units
    // is UB / G sixteen-byte loads per lane
    typedef std::conditional_t<VFORM == 2, _Float16, std::conditional_t<VFORM == 1, float, val_t>> sval_t;   // a value as the plan stores it
    typedef sval_t grp_t __attribute__((ext_vector_type(G)));
    const grp_t *__restrict__ ugrp = reinterpret_cast<const grp_t *>(S.uval) + r;
    const int last = unit_end - 1;
    const int last_grp = unit_begin + (unit_end - 1 - unit_begin) / G * G;  // first unit of the task's last group
    const bool have_units = unit_begin < unit_end;
    const long long xlast = (long long)colA - 1;  // row units of a partial last column block: zero payload, clamped x index
    const int xlast32 = colA - 1;
    const int ncoo = coo_end - coo_begin;
    uint4 dcur = make_uint4(0u, 0u, 0u, 0u), dnext = dcur;
    uint2 rcur = make_uint2(0u, 0u), rnext = rcur;   // POOL: row nibbles of the chunks in dcur / dnext
    const uint2 *__restrict__ urw = reinterpret_cast<const uint2 *>(S.urow);
    uint4 ccur = make_uint4(0u, 0u, 0u, 0u), cnext = ccur;   // WIDE: column-offset bytes of the chunks in dcur / dnext
    unsigned wnn = 0;   // CD: descriptor word of the chunk after `dnext`
    const unsigned *__restrict__ udw = reinterpret_cast<const unsigned *>(S.udesc);
    // POOL + CD (pooled dictionary plans, round 5): a unit's descriptor in HBM is 8 bytes — word 0 (window base | tile-row in strip) and the id of its 16-byte pattern (the 16 column
    // nibbles and the 16 row nibbles) in S.pdict, which stays in the vector L1 / L2: natural-order meshes use a few dozen patterns (fem3_68: 54).  Same staging as the classic
    // dictionary: words two chunks ahead, the pattern gathered one chunk ahead, so neither hop is waited for in the unit loop.  Round 6: 4-byte words where everything fits one (pool_desc).
    uint2 wnn2 = make_uint2(0u, 0u);
    val_t v[UB];
    auto unit_prologue = [&]() {  // descriptor chunks 0 and 1, first value batch: in flight across the entry phase
        if (have_units) {
            if constexpr (CD && POOL) {   // pooled dictionary plans: 8-byte descriptors (word 0, pattern id)
                const uint2 a = pool_desc(S, min(unit_begin + r, last)), b = pool_desc(S, min(unit_begin + DCHUNK + r, last));
                dcur.x = a.x; dcur.y = a.y; dnext.x = b.x; dnext.y = b.y;
            } else if constexpr (CD) {
                dcur.x = stream_load<NT_DESC>(udw + min(unit_begin + r, last));
                dnext.x = stream_load<NT_DESC>(udw + min(unit_begin + DCHUNK + r, last));
            } else {
                dcur = load_udesc_raw(S.udesc, min(unit_begin + r, last));
                dnext = load_udesc_raw(S.udesc, min(unit_begin + DCHUNK + r, last));
                if constexpr (WIDE) { ccur = S.ucol[min(unit_begin + r, last)]; cnext = S.ucol[min(unit_begin + DCHUNK + r, last)]; }
                else if constexpr (POOL) { rcur = urw[min(unit_begin + r, last)]; rnext = urw[min(unit_begin + DCHUNK + r, last)]; }   // (12-byte descriptors + 8 bytes of row nibbles)
            }
#pragma unroll
            for (int k = 0; k < UB; k += G) {
                const grp_t pv = stream_load<NT>(ugrp + (long long)min(unit_begin + k, last_grp) * (16 / G));
#pragma unroll
                for (int q = 0; q < G; q++) v[k + q] = pv[q];
            }
        }
    };

    // descriptors (from the chunk parked in LDS) and x gathers of one unit batch; j0 = position of the batch in the chunk
    const uint2 *sd = reinterpret_cast<const uint2 *>(&s_d[g][0]) + (r >> 3);  // this lane's 8-B half of a descriptor
    uint2 d[UB];
    unsigned rw[UB];   // POOL: this lane's half of the unit's row nibbles
    val_t xv[UB];
    const unsigned *sr = reinterpret_cast<const unsigned *>(&s_r[POOL && !WIDE ? g : 0][0]) + (r >> 3);
    const unsigned char *sc = reinterpret_cast<const unsigned char *>(&s_c[WIDE ? g : 0][0]) + r;   // this lane's byte of a unit's 16 column offsets
    auto park_first = [&]() {   // chunk 0 into LDS (CD: the patterns of chunks 0 and 1 are gathered here, the word of chunk 2 loaded)
        if constexpr (CD && POOL) {
            const uint4 p0 = S.pdict[dcur.y], p1 = S.pdict[dnext.y];
            wnn2 = pool_desc(S, min(unit_begin + 2 * DCHUNK + r, last));
            s_d[g][r] = make_uint4(dcur.x, p0.x, dcur.x, p0.y); s_r[g][r] = make_uint2(p0.z, p0.w);
            dnext = make_uint4(dnext.x, p1.x, 0u, p1.y); rnext = make_uint2(p1.z, p1.w);
        } else if constexpr (CD) {
            const uint4 p0 = udict_of(S, dcur.x), p1 = udict_of(S, dnext.x);
            wnn = stream_load<NT_DESC>(udw + min(unit_begin + 2 * DCHUNK + r, last));
            dnext.y = p1.x; dnext.z = p1.z; dnext.w = p1.y;
            s_d[g][r] = udesc_expand(S, dcur.x, p0);
        } else s_d[g][r] = udesc_park_form(dcur);
        if constexpr (WIDE) s_c[g][r] = ccur;
        else if constexpr (POOL && !CD) s_r[g][r] = rcur;
    };
    auto fetch_batch = [&](int j0) {
#pragma unroll
        for (int k = 0; k < UB; k++) d[k] = sd[2 * (j0 + k)];
        if constexpr (WIDE) {   // the descriptor's nibble half = this lane's row nibbles; the column offset is its byte of the unit's 16
#pragma unroll
            for (int k = 0; k < UB; k++) rw[k] = d[k].y;
#pragma unroll
            for (int k = 0; k < UB; k++) {
                if constexpr (UNIT_X32) xv[k] = x[x_index32((int)(d[k].x & POOL_BASE_MASK), sc[16 * (j0 + k)], xlast32)];
                else xv[k] = x[min((long long)(d[k].x & POOL_BASE_MASK) + (long long)sc[16 * (j0 + k)], xlast)];
            }
            return;
        }
        if constexpr (POOL) {
#pragma unroll
            for (int k = 0; k < UB; k++) rw[k] = sr[2 * (j0 + k)];
#pragma unroll
            for (int k = 0; k < UB; k++) {
                if constexpr (UNIT_X32) xv[k] = x[x_index32((int)(d[k].x & POOL_BASE_MASK), (d[k].y >> (28 - 4 * (r & 7))) & 15u, xlast32)];
                else xv[k] = x[min((long long)(d[k].x & POOL_BASE_MASK) + (long long)((d[k].y >> (28 - 4 * (r & 7))) & 15u), xlast)];
            }
            return;
        }
#pragma unroll
        for (int k = 0; k < UB; k++) {
            const unsigned fl = d[k].x >> 24;
            const unsigned nib = (ROWUNITS && (fl & UNIT_ROWUNIT)) ? (unsigned)r : (d[k].y >> (28 - 4 * (r & 7))) & 15u;
            if (DERIVED && (d[k].x >> UNIT_SHIFT_SHIFT) == UNIT_DERIVED_CODE && r != 15) { if constexpr (!LEAN) xv[k] = 0; }   // derived unit: only lane 15 loads (unit_x_use gives the others the previous unit's x and selects their xv[k] away: the lean forms leave it as it is)
            else if constexpr (UNIT_X32) xv[k] = x[x_index32(unit_x_base32(d[k].x), nib, xlast32)];
            else xv[k] = x[min(unit_x_base(d[k].x) + nib, xlast)];
        }
    };

    if constexpr (ECOO == 2) {
        const int4 wr = S.wg_coo[bid];
        // a strip with entries adds its slab at the end, so its slab is zeroed even when the workgroup's list is empty: in a column-panelled plan (x_panels > 1) all of a
        // strip's entries may sit in the other panels' lists
        if (wr.y > wr.x) {  // workgroup-uniform
            if (side) for (int k = 0; k < nrows; k++) s_y[g][k][r] = 0;
            __syncthreads();
        } else if ((S.panel_merge > 0 || S.slice_passes > 0) && side) {
            for (int k = 0; k < nrows; k++) s_y[g][k][r] = 0;
            wave_lds_fence();
        }
        // (issuing the unit prologue after the entry phase instead frees 16 VGPRs — 8 waves per SIMD at 6 x 256 per trip, or 8 x 256 at
        // 6 waves — and changes nothing: power-law 8 M 0.1026-0.1034 ms either way, profiles/r03_entry_ablations.txt: bytes in flight are not the limit)
        // pipelined trips on top of that (78 VGPRs at 6 x 256, no spill): 0.1050-0.1062 against 0.1031-0.1046 — slightly worse
        // (halves: behind the entry phase — the 16 VGPRs this frees keep the form at 64 VGPRs without scratch)
        constexpr bool LATE_PROLOGUE = VFORM == 2 || LEAN;
        if constexpr (!LATE_PROLOGUE) unit_prologue();
        if (wr.y > wr.x) {
            int ge = wr.y;   // column-panelled launch: this kernel takes the first panel_merge panels of the list, k_entries_acc the rest
            if (GPB == 16 && S.panel_merge > 0) ge = S.panel_off[(size_t)bid * (size_t)(S.x_panels + 1) + (size_t)min(S.x_panels, S.panel_merge)];
            if (GPB == 16 && S.slice_passes > 0) ge = wr.x;   // column slices pinned to XCDs: the whole list belongs to k_entries_xcd
            wg_entry_trips<WCOO_HEAVY_CT, 16 * GPB, NTS>(S.grec, S.gbase, wr.z, S.dest_bits, S.coo_ordered != 0, x, &s_y[0][0][0], tid, wr.x, ge);
            __syncthreads();
        }
        if constexpr (LATE_PROLOGUE) unit_prologue();
    } else if constexpr (WCOO) {
        // ---- small grids (entry mode 1 is chosen when the whole grid is resident at once): the kernel is a chain of
        // round trips, so everything that can be in flight together is: task -> {unit prologue, entry loads} -> {x gathers
        // of the first unit batch, x gathers of the entries} -> adds -> unit loop.  Registers are not a constraint here
        // (4 waves/SIMD asked of the allocator).
        constexpr int CT = 6;
        const int lane = tid & 63;
        const int4 wr = S.wg_coo[(long long)bid * (GROUPS_PER_BLOCK / 4) + (g >> 2)];  // this wavefront's merged list
        const int tot = wr.y - wr.x;
        lacc_t *swave = &s_y[g & ~3][0][0];  // the wavefront's four slabs of STRIP_MAX_ROWS x 16 values
        unit_prologue();
        ERec rr[CT]; unsigned cbase[CT]; val_t xx[CT];
        const int db = S.dest_bits;
        if (tot > 0) {
            if (side) for (int k = 0; k < nrows; k++) s_y[g][k][r] = 0;
            const int clast = wr.z + ((tot - 1) >> 6);
#pragma unroll
            for (int q = 0; q < CT; q++) {
                rr[q] = S.grec[min(wr.x + 64 * q + lane, wr.y - 1)];
                cbase[q] = S.gbase[__builtin_amdgcn_readfirstlane(min(wr.z + q, clast))];
            }
        }
        if (have_units) {  // waits for the descriptor chunk only (older than the entry loads)
            park_first();
            wave_lds_fence();
            fetch_batch(0);
        } else if (tot > 0) wave_lds_fence();
        if (tot > 0) {
            const unsigned dmask = (1u << db) - 1u;
#pragma unroll
            for (int q = 0; q < CT; q++) xx[q] = x[(size_t)(cbase[q] + (rr[q].w >> db))];
#pragma unroll
            for (int q = 0; q < CT; q++)
                if (wr.x + 64 * q + lane < wr.y) atomicAdd(&swave[rr[q].w & dmask], (lacc_t)(erec_val(rr[q]) * xx[q]));
            if (tot > 64 * CT) wave_entry_trips<CT>(S, x, swave, lane, wr.x, wr.y, wr.z, CT);
            wave_lds_fence();
        }
    } else {
    // ---- issue order: first COO chunk, descriptor chunk 0 (+1), first value batch: all in flight together.
    // Strips with many COO entries (> coo_heavy_min, default 32: irregular matrices) run their entry list first,
    // 6 x 16 entries per trip with every load of a trip in flight before its gathers, and only then start the
    // unit pipeline; the others keep the unit prologue in flight across their (short) entry list.
    constexpr int CT = 6;  // sub-chunks of 16 entries per trip
    const bool coo_heavy = ncoo > S.coo_heavy_min;
    if (side) {
        for (int k = 0; k < nrows; k++) s_y[g][k][r] = 0;
        wave_lds_fence();
    }
    if (coo_heavy) {
        for (int e0 = coo_begin; e0 < coo_end; e0 += 16 * CT) {
            unsigned rb[CT]; int cc[CT]; val_t cv[CT], xx[CT];
#pragma unroll
            for (int q = 0; q < CT; q++) {
                const int e = min(e0 + 16 * q + r, coo_end - 1);
                rb[q] = S.crow[e]; cc[q] = S.ccol[e]; cv[q] = S.cval[e];
            }
#pragma unroll
            for (int q = 0; q < CT; q++) xx[q] = x[cc[q]];
#pragma unroll
            for (int q = 0; q < CT; q++)
                if (e0 + 16 * q + r < coo_end) atomicAdd(&s_y[g][rb[q] >> 4][rb[q] & 15u], (lacc_t)(cv[q] * xx[q]));
        }
        wave_lds_fence();
    }
    unsigned rb0 = 0; int cc0 = 0; val_t cv0 = 0;
    const bool coo0 = side && !coo_heavy && (coo_begin + r < coo_end);
    if (coo0) { rb0 = stream_load<NT_COO0>(S.crow + coo_begin + r); cc0 = stream_load<NT_COO0>(S.ccol + coo_begin + r); cv0 = stream_load<NT_COO0>(S.cval + coo_begin + r); }
    unit_prologue();
    if (side && !coo_heavy) {  // up to coo_heavy_min entries: 16 with the prologue loads, the rest 4 x 16 per trip
        if (coo0) atomicAdd(&s_y[g][rb0 >> 4][rb0 & 15u], (lacc_t)(cv0 * x[cc0]));
        for (int e0 = coo_begin + 16; e0 < coo_end; e0 += 64) {
            unsigned rb[4]; int cc[4]; val_t cv[4], xx[4];
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int e = min(e0 + 16 * q + r, coo_end - 1);
                rb[q] = S.crow[e]; cc[q] = S.ccol[e]; cv[q] = S.cval[e];
            }
#pragma unroll
            for (int q = 0; q < 4; q++) xx[q] = x[cc[q]];
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (e0 + 16 * q + r < coo_end) atomicAdd(&s_y[g][rb[q] >> 4][rb[q] & 15u], (lacc_t)(cv[q] * xx[q]));
        }
        wave_lds_fence();
    }
    }

    val_t acc = 0;
    // A finished tile-row parks its 16 results in s_y; y is written once per strip at the end with 16-B
    // lane stores.  (Stores share the in-order vmcnt queue with the loads on CDNA4: a store in the middle
    // of the unit loop makes every later counted wait also wait for its write acknowledge.)
    auto retire = [&](val_t prod, unsigned flags, unsigned word1) {
        if constexpr (POOL) {   // flags = word 0 >> 24 (tile-row in strip in its top nibble), word1 = this lane's half of the row nibbles
            const unsigned dest = ((flags >> (POOL_KR_SHIFT - 24)) & 7u) * 16u + ((word1 >> (28 - 4 * (r & 7))) & 15u);
            if constexpr (PCOPY) atomicAdd(((r & 1) ? s_y1 : &s_y[0][0][0]) + g * (SROWS * 16) + dest, (lacc_t)prod);
            else atomicAdd(&s_y[g][0][0] + dest, (lacc_t)prod);
            return;
        }
        if constexpr (ROWUNITS) {
            if (flags & UNIT_ROWUNIT) {  // dense-row unit: lanes hold one row's products
                prod = strip_allreduce(prod);
                if (r != (int)(word1 & 15u)) prod = 0;
            }
        }
        acc += prod;
        if (flags & UNIT_EOR) {
            const int kr = (int)((flags >> UNIT_ROW_SHIFT) & 7u);
            if constexpr (sizeof(val_t) == sizeof(lacc_t)) {
                lacc_t out = acc;
                if (side) out += s_y[g][kr][r];
                s_y[g][kr][r] = out;
            } else {
                // fp32 build: the row's entry sums (fp64, complete: the entry phase is over) are read and the 16 FINAL results go back as floats into the head of the
                // row's 128 bytes — lane r's 4 bytes overlap the doubles of lanes r/2, which every lane of the strip has read one instruction earlier — so that
                // the y store at the end reads 16 bytes per lane as in the fp64 build instead of narrowing four doubles
                val_t out = acc;
                if (side) out = (val_t)((lacc_t)acc + s_y[g][kr][r]);
                reinterpret_cast<val_t *>(&s_y[g][kr][0])[r] = out;
            }
            acc = 0;
        }
    };
    if (have_units) {  // phase 2: units, value loads software-pipelined by one batch
        if (ECOO != 1) {  // (entry mode 1 parked the first chunk and fetched the first batch before its entry phase)
            park_first();
            wave_lds_fence();
        }
        int chunk_end = unit_begin + DCHUNK;  // first unit NOT described by the chunk in LDS
        val_t xprev = 0;   // classic plans: the x the previous unit used (derived units, unit_x_use)
        if constexpr (LEAN) {
            // The lean forms' loop.  One batch of UB units: TAIL = the task's last batch where its unit count is no multiple of UB — the only one whose units are tested
            // against unit_end, and the only one with no batch behind it to prefetch values for; every other batch runs unguarded in the loop below.  The value prefetch
            // keeps a carried pointer (the group of the batch behind the current one; it may pass the task's last group and is dereferenced only inside the task: groups
            // start at multiples of G from unit_begin, so "u + UB + k <= last_grp" is "u + UB + k < unit_end").
            const grp_t *vnext = ugrp + (long long)(unit_begin + UB) * (16 / G);
            auto batch = [&](const int u, auto tail) {
#pragma clang fp contract(off)   // the general loop's product and sum sit in different blocks (the tail guard, the row-unit test) and stay v_mul + v_add; without those branches the compiler would fuse them here, and y would differ in its last bit
                constexpr bool TAIL = decltype(tail)::value;
                if (u == chunk_end) {  // next descriptor chunk: already in registers, fetch the one after it (as in the general loop below; lean plans are classic ones)
                    wave_lds_fence();
                    if constexpr (CD) s_d[g][r] = udesc_expand(S, dnext.x, make_uint4(dnext.y, dnext.w, dnext.z, 0u));
                    else s_d[g][r] = udesc_park_form(dnext);
                    wave_lds_fence();
                    chunk_end += DCHUNK;
                    if constexpr (CD) {
                        const uint4 p = udict_of(S, wnn);   // (its word was loaded a chunk ago)
                        dnext = make_uint4(wnn, p.x, p.z, p.y);
                        wnn = stream_load<NT_DESC>(udw + (min(chunk_end + DCHUNK + r + 1, unit_end) - 1));   // (= min(.., last) from unit_end, which the loop keeps anyway: one VGPR less across the loop)
                    } else dnext = load_udesc_raw(S.udesc, min(chunk_end + r + 1, unit_end) - 1);
                }
                fetch_batch(u - (chunk_end - DCHUNK));
                sval_t vn[UB];
                if constexpr (!TAIL) {
#pragma unroll
                    for (int k = 0; k < UB; k += G) {  // unconditional: exact vmcnt
                        const grp_t *pa = vnext + k * (16 / G);
                        if constexpr (UNIT_TAIL_HOT) pa = (u + UB + k < unit_end) ? pa : reinterpret_cast<const grp_t *>(S.uval);   // behind the task's end: nobody uses what this loads (the plan's first 16 / 8 bytes)
                        else pa = ugrp + (long long)min(u + UB + k, last_grp) * (16 / G);
                        const grp_t pv = stream_load<NT>(pa);
#pragma unroll
                        for (int q = 0; q < G; q++) vn[k + q] = pv[q];
                    }
                    vnext += UB * (16 / G);
                }
                __builtin_amdgcn_sched_barrier(0);   // the batch's loads are issued before its first use, as in the general loop (whose tail guard keeps the scheduler from mixing the two)
#pragma unroll
                for (int k = 0; k < UB; k++) {
                    val_t xu = xv[k];
                    if constexpr (DERIVED) { xu = unit_x_use(xv[k], xprev, d[k].x, r); xprev = xu; }
                    if (!TAIL || u + k < unit_end) retire(v[k] * xu, d[k].x >> 24, d[k].y);
                }
                if constexpr (!TAIL) {
#pragma unroll
                    for (int k = 0; k < UB; k++) v[k] = vn[k];
                }
            };
            int u = unit_begin;
            for (; u + UB <= unit_end; u += UB) batch(u, std::false_type());
            if (u < unit_end) batch(u, std::true_type());
        } else
        for (int u = unit_begin; u < unit_end; u += UB) {
            if (u == chunk_end) {  // next descriptor chunk: already in registers, fetch the one after it
                wave_lds_fence();
                if constexpr (CD && POOL) { s_d[g][r] = make_uint4(dnext.x, dnext.y, dnext.x, dnext.w); s_r[g][r] = rnext; }
                else if constexpr (CD) s_d[g][r] = udesc_expand(S, dnext.x, make_uint4(dnext.y, dnext.w, dnext.z, 0u));
                else s_d[g][r] = udesc_park_form(dnext);
                if constexpr (WIDE) { s_c[g][r] = cnext; cnext = S.ucol[min(chunk_end + DCHUNK + r, last)]; }
                else if constexpr (POOL && !CD) { s_r[g][r] = rnext; rnext = urw[min(chunk_end + DCHUNK + r, last)]; }
                wave_lds_fence();
                chunk_end += DCHUNK;
                if constexpr (CD && POOL) {
                    const uint4 p = S.pdict[wnn2.y];   // (its words were loaded a chunk ago)
                    dnext = make_uint4(wnn2.x, p.x, 0u, p.y); rnext = make_uint2(p.z, p.w);
                    wnn2 = pool_desc(S, min(chunk_end + DCHUNK + r, last));
                } else if constexpr (CD) {
                    const uint4 p = udict_of(S, wnn);   // (its word was loaded a chunk ago)
                    dnext = make_uint4(wnn, p.x, p.z, p.y);
                    wnn = stream_load<NT_DESC>(udw + min(chunk_end + DCHUNK + r, last));
                } else dnext = load_udesc_raw(S.udesc, min(chunk_end + r, last));
            }
            if (!(ECOO == 1 && u == unit_begin)) fetch_batch(u - (chunk_end - DCHUNK));
            sval_t vn[UB];   // (narrow plans: the prefetched batch waits as floats and is widened when it becomes `v`)
#pragma unroll
            for (int k = 0; k < UB; k += G) {  // unconditional (clamped to the task's last group): exact vmcnt
                const grp_t *pa = ugrp + (long long)min(u + UB + k, last_grp) * (16 / G);
                if constexpr (UNIT_TAIL_HOT) pa = (u + UB + k <= last_grp) ? pa : reinterpret_cast<const grp_t *>(S.uval);   // behind the task's end: nobody uses what this loads (the plan's first 16 / 8 bytes)
                const grp_t pv = stream_load<NT>(pa);
#pragma unroll
                for (int q = 0; q < G; q++) vn[k + q] = pv[q];
            }
#pragma unroll
            for (int k = 0; k < UB; k++)
            {
                if constexpr (POOL) {
                    // unconditional adds (a unit past the task's end adds 0 to a row of this strip's slab: its descriptor is the clamped load of the task's last unit): with the add
                    // under a branch the compiler sinks the unit's gather into the branch and waits for it with vmcnt(0) — every unit then pays a full memory round trip
                    retire((u + k < unit_end) ? v[k] * xv[k] : (val_t)0, d[k].x >> 24, rw[k]);
                } else {
                    const val_t xu = unit_x_use(xv[k], xprev, d[k].x, r);
                    xprev = xu;
                    if (u + k < unit_end) retire(v[k] * xu, d[k].x >> 24, d[k].y);
                }
            }
#pragma unroll
            for (int k = 0; k < UB; k++) v[k] = vn[k];
        }
    }
    if constexpr (POOL) {   // every add of this wavefront into the slab is behind us
        wave_lds_fence();
        if constexpr (PCOPY) {
            for (int k = 0; k < nrows; k++) s_y[g][k][r] += s_y1[(g * SROWS + k) * 16 + r];
            wave_lds_fence();
        }
    }
    if (part >= 0) {
        val_t out = acc;
        if (side) out = (val_t)((lacc_t)acc + s_y[g][0][r]);
        if (S.ifix_count == nullptr || nounit == 0xFFFFFFFFu) {
            partial[(long long)part * 16 + r] = out;  // k_fixup_split adds the slots up after all passes
        } else {
            // All pieces of this tile-row run in this kernel: the piece that finishes last adds the slots up, in slot
            // order (same sum as k_fixup_split).  Slots and counter are agent-scope atomics (performed at the device's
            // point of coherence, past the per-XCD L2s), the counter is bumped only after this strip's 16 slot stores
            // have been acknowledged, and the slot loads are issued only after the counter value has come back.
            __hip_atomic_store(&partial[(long long)part * 16 + r], out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const FixRow f = S.ifix[nounit];
            unsigned prev = 0;
            if (r == 0) prev = __hip_atomic_fetch_add(&S.ifix_count[nounit], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            prev = (unsigned)__shfl((int)prev, tid & 48, 64);  // lane 0 of this strip
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (prev == (unsigned)f.count - 1u) {
                val_t sum = 0;
                for (int k0 = 0; k0 < f.count; k0 += 8) {  // 8 slot loads in flight, added in slot order
                    val_t sv[8];
#pragma unroll
                    for (int j = 0; j < 8; j++)
                        sv[j] = __hip_atomic_load(&partial[(long long)(f.first + min(k0 + j, f.count - 1)) * 16 + r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
                    for (int j = 0; j < 8; j++) if (k0 + j < f.count) sum += sv[j];
                }
                const long long yi = (long long)f.row * 16 + r;
                if (yi < rowA) y[yi] = sum;
                if (r == 0) __hip_atomic_store(&S.ifix_count[nounit], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next launch
            }
        }
    } else {
        if constexpr (POOL) {
            if constexpr (sizeof(val_t) != sizeof(lacc_t)) {   // fp32 build: the fp64 sums go back as floats into the head of each row's 128 bytes (the form the store below reads; lane r's 4 bytes
                for (int k = 0; k < nrows; k++) {              // overlap the doubles of lanes r / 2, which every lane of the strip has read one instruction earlier)
                    const val_t o = (val_t)s_y[g][k][r];
                    reinterpret_cast<val_t *>(&s_y[g][k][0])[r] = o;
                }
            }
        } else if constexpr (sizeof(val_t) == sizeof(lacc_t)) {
            if (!side) {  // rows without any unit and no COO contribution are zero
                unsigned m = nounit;
                while (m) { const int kr = __ffs((int)m) - 1; m &= m - 1; s_y[g][kr][r] = 0; }
            }
        } else {          // fp32 build: rows without units hold fp64 entry sums (or nothing): into the float form of the retired rows
            unsigned m = nounit;
            while (m) {
                const int kr = __ffs((int)m) - 1; m &= m - 1;
                const val_t o = side ? (val_t)s_y[g][kr][r] : (val_t)0;
                reinterpret_cast<val_t *>(&s_y[g][kr][0])[r] = o;
            }
        }
        wave_lds_fence();
        constexpr int VEC = 16 / (int)sizeof(val_t);  // values per 16-B lane store
        const lacc_t *res = &s_y[g][0][0];
        const int ystride = S.strip_stride;   // tile-row k of the strip is row0 + k * ystride (hip_plan.h DevStream::strip_stride); a 16-byte lane store never crosses a tile-row
        for (int i = r * VEC; i < 16 * nrows; i += 16 * VEC) {
            const long long yi = ((long long)row0 + (long long)(i >> 4) * ystride) * 16 + (i & 15);
            if constexpr (sizeof(val_t) == sizeof(lacc_t)) {   // fp64: the 16 bytes go out as they sit in LDS (one ds_read_b128, one store)
                if (yi + VEC <= rowA) {
                    if (NT_Y && S.y_streaming) __builtin_nontemporal_store(*reinterpret_cast<const v4u_t *>(res + i), reinterpret_cast<v4u_t *>(y + yi));
                    else *reinterpret_cast<uint4 *>(y + yi) = *reinterpret_cast<const uint4 *>(res + i);
                } else {
#pragma unroll
                    for (int q = 0; q < VEC; q++) if (yi + q < rowA) y[yi + q] = (val_t)res[i + q];
                }
            } else {                                           // fp32: the rows hold 16 floats each at the head of their 128 bytes (retire / flush above)
                const val_t *rf = reinterpret_cast<const val_t *>(res) + (i >> 4) * 32 + (i & 15);
                if (yi + VEC <= rowA) {
                    if (NT_Y && S.y_streaming) __builtin_nontemporal_store(*reinterpret_cast<const v4u_t *>(rf), reinterpret_cast<v4u_t *>(y + yi));
                    else *reinterpret_cast<uint4 *>(y + yi) = *reinterpret_cast<const uint4 *>(rf);
                } else {
#pragma unroll
                    for (int q = 0; q < VEC; q++) if (yi + q < rowA) y[yi + q] = rf[q];
                }
            }
        }
    }
}

}  // namespace tilespmv
