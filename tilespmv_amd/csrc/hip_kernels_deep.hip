// hip_kernels_deep.hip — k_units_deep, the unit-stream kernel of lean plans that hold nothing but units (hip_plan.h unit_deep_form: a lean form, entry mode 0, 16 strips per
// workgroup, nontemporal streams, no list entry, no split tile-row, no fallback launch), with the x gathers of DEPTH batches in flight per wavefront instead of one.
// Strip, lane and LDS organisation are the lean kernel's (hip_units_kernel.h): lane r owns tile row r, 4 strips per wavefront, descriptor chunks parked in LDS one chunk ahead,
// y parked per tile-row and stored once per strip.  What such a plan cannot need is not here: no entry phase, no slab sums in the retire, no piece-sum epilogue.
//   While batch b is multiplied, the gathers of batch b + 1 are in flight into a second set of registers and so is its value group, in its stored form.  Every path
//   through an iteration issues the same loads in the same order — a derived unit's lanes 0-14 load too (the descriptor of a derived unit holds lane 15's column in every
//   nibble: all 16 lanes read one word, and unit_x_use selects it away) — so the wait in front of batch b's first product is a counted vmcnt that leaves everything issued in
//   this iteration outstanding.  The loop body is one descriptor chunk (DCHUNK / UB batches) without a branch: the buffers take turns by the batch's place in the chunk, so
//   nothing a load is in flight into is ever copied, and the chunk refill is straight-line code — the next chunk is parked behind the gathers of the chunk's last batch, and
//   the loads for the chunk after it are issued BEHIND that iteration's gathers and value load, where no counted wait reaches them before the next refill.  The batches
//   behind a task's last whole chunk run the same steps once more as nested branches; only the task's last batch tests its units against the task's end.
// The arithmetic is the lean kernel's — v_mul then v_add in unit order, contraction off, halves widened half -> float -> double — so y is its y bit for bit.
// A file of its own so that hip_kernels.hip, hip_kernels_half.hip and hip_kernels_lean.hip keep their kernels, their names and their registers.
#include <hip/hip_runtime.h>

#include "hip_plan.h"
#include "hip_plan_internal.h"
#include "hip_units_kernel.h"   // the device helpers (descriptor forms, unit_x_use, x_index32, stream_load, wave_lds_fence); its kernel template is not instantiated here

namespace tilespmv {

// Waves per SIMD asked of the register allocator, by value form: the most at which no instantiation of the form uses scratch.  The second set of x and the second value group
// cost up to 14 (halves) to 28 (8-byte values) VGPRs on top of the lean kernel's 58: halves up to 72 VGPRs, floats 76, 8-byte values 86, the fp32 library 56.
constexpr int deep_min_waves(int vf) { return sizeof(val_t) == 4 ? 8 : vf == 2 ? 7 : vf == 1 ? 6 : 5; }

template <int UB, int DEPTH, bool CD, int VF, bool DERIVED>
__global__ __launch_bounds__(256, deep_min_waves(VF)) void k_units_deep(DevStream S, int rowA, int colA, int xcd_chunk, const val_t *__restrict__ x, val_t *__restrict__ y)
{
    static_assert(UB == 4 && DEPTH == 2, "the one form that was kept (DESIGN.md S8 item 15): two batches of 4 units in flight, whose buffers take turns inside a chunk of 4 batches");
    static_assert(VF >= 0 && VF <= (sizeof(val_t) == 8 ? 2 : 0), "a value form of this build");
    constexpr int G = VF != 0 ? UNIT_GROUP_NARROW : UNIT_GROUP;   // units whose values share one lane load
    constexpr int NG = UB / G;                                     // value loads per batch
    static_assert(DCHUNK % UB == 0 && UB % G == 0, "a batch never straddles a descriptor chunk and is whole value groups");
    __shared__ lacc_t s_yall[16 * STRIP_MAX_ROWS * 16];
    lacc_t (*s_y)[STRIP_MAX_ROWS][16] = reinterpret_cast<lacc_t (*)[STRIP_MAX_ROWS][16]>(&s_yall[0]);
    __shared__ uint4 s_d[16][DCHUNK];
    const int tid = threadIdx.x, r = tid & 15, g = tid >> 4;
    unsigned bid = blockIdx.x;
    if (xcd_chunk > 0) {   // runs of xcd_chunk consecutive workgroups per XCD, as in k_units
        const unsigned C = (unsigned)xcd_chunk, W = 8u * C, win = bid / W, off = bid % W, k = off & 7u;
        if ((win + 1) * W <= gridDim.x) bid = win * W + k * C + (off >> 3);
    }
    const long long task_id = (long long)bid * 16 + g;
    if (task_id >= S.ntasks) return;
    const int4 t0 = reinterpret_cast<const int4 *>(S.task)[task_id * 2], t1 = reinterpret_cast<const int4 *>(S.task)[task_id * 2 + 1];
    const int unit_begin = t0.x, unit_end = t0.y, row0 = t1.x, nrows = t1.w;
    const unsigned nounit = (unsigned)t1.z;
    typedef std::conditional_t<VF == 2, _Float16, std::conditional_t<VF == 1, float, val_t>> sval_t;   // a value as the plan stores it
    typedef sval_t grp_t __attribute__((ext_vector_type(G)));
    const grp_t *__restrict__ ugrp = reinterpret_cast<const grp_t *>(S.uval) + r;   // group of task-relative unit j (a multiple of G): ugrp[(unit_begin + j) * (16 / G)]
    const grp_t *__restrict__ vhot = reinterpret_cast<const grp_t *>(S.uval);       // UNIT_TAIL_HOT: what a value load behind the task's end reads
    const int xlast32 = colA - 1;
    const unsigned *__restrict__ udw = reinterpret_cast<const unsigned *>(S.udesc);
    const uint2 *sd = reinterpret_cast<const uint2 *>(&s_d[g][0]) + (r >> 3);       // this lane's 8-byte half of a parked descriptor

    val_t acc = 0;
    auto retire = [&](val_t prod, unsigned flags) {
#pragma clang fp contract(off)
        acc += prod;
        if (flags & UNIT_EOR) {   // the tile-row's 16 results, in the form the y store reads (fp32 build: floats at the head of the row's 128 bytes)
            const int kr = (int)((flags >> UNIT_ROW_SHIFT) & 7u);
            if constexpr (sizeof(val_t) == sizeof(lacc_t)) s_y[g][kr][r] = acc;
            else reinterpret_cast<val_t *>(&s_y[g][kr][0])[r] = acc;
            acc = 0;
        }
    };

    if (unit_begin < unit_end) {
        const int last = unit_end - 1;
        // descriptor chunks 0 and 1 and the value group of the first batch
        uint4 dcur = make_uint4(0u, 0u, 0u, 0u), dnext = dcur;
        unsigned wnn = 0;   // CD: descriptor word of the chunk after `dnext`
        if constexpr (CD) { dcur.x = udw[min(unit_begin + r, last)]; dnext.x = udw[min(unit_begin + DCHUNK + r, last)]; }
        else { dcur = load_udesc_raw(S.udesc, min(unit_begin + r, last)); dnext = load_udesc_raw(S.udesc, min(unit_begin + DCHUNK + r, last)); }
        grp_t vs[2][NG];   // value groups, as stored, of the batch that is multiplied and of the one behind it: they take turns like the x buffers
        auto load_values = [&](const int u0, const grp_t *p, grp_t (&out)[NG]) {   // unconditional: a group behind the task's end reads the plan's first word
#pragma unroll
            for (int q = 0; q < NG; q++) out[q] = stream_load<true>((u0 + q * G < unit_end) ? p + q * 16 : vhot);   // (a group is 16 lane loads)
        };
        load_values(unit_begin, ugrp + (long long)unit_begin * (16 / G), vs[0]);
        if constexpr (CD) {   // the patterns of chunks 0 and 1, the word of chunk 2
            const uint4 p0 = udict_of(S, dcur.x), p1 = udict_of(S, dnext.x);
            wnn = udw[min(unit_begin + 2 * DCHUNK + r, last)];
            dnext.y = p1.x; dnext.z = p1.z; dnext.w = p1.y;
            s_d[g][r] = udesc_expand(S, dcur.x, p0);
        } else s_d[g][r] = udesc_park_form(dcur);
        wave_lds_fence();
        constexpr int NB = DCHUNK / UB;        // batches per descriptor chunk
        int cload = unit_begin + 2 * DCHUNK + r + 1;   // this lane's unit of the chunk the next refill loads, + 1
        unsigned w0[DEPTH][UB];                // word 0 of the batches whose gathers are in flight
        val_t xv[DEPTH][UB];
        // descriptors (from the chunk in LDS) and x gathers of the batch at place j0 of its chunk
        auto gather = [&](const int j0, unsigned (&w)[UB], val_t (&xg)[UB]) {
#pragma unroll
            for (int k = 0; k < UB; k++) {
                const uint2 dk = sd[2 * (j0 + k)];
                w[k] = dk.x;
                xg[k] = x[x_index32(unit_x_base32(dk.x), (dk.y >> (28 - 4 * (r & 7))) & 15u, xlast32)];
            }
        };
        // The chunk in LDS has been read to its end: the next one, in registers since the last refill, takes its place, and the chunk after that is loaded (dictionary plans: its
        // pattern, and the word of the chunk after it).  Straight-line code of the loop body below — under a branch the compiler copies what it loads into the carried registers
        // and waits for it with vmcnt(0) on the spot.
        auto refill = [&]() {
            wave_lds_fence();
            if constexpr (CD) s_d[g][r] = udesc_expand(S, dnext.x, make_uint4(dnext.y, dnext.w, dnext.z, 0u));
            else s_d[g][r] = udesc_park_form(dnext);
            wave_lds_fence();
            if constexpr (CD) {
                const uint4 p = udict_of(S, wnn);
                dnext = make_uint4(wnn, p.x, p.z, p.y);
                wnn = udw[min(cload + DCHUNK, unit_end) - 1];
            } else dnext = load_udesc_raw(S.udesc, min(cload, unit_end) - 1);
            cload += DCHUNK;
        };
        val_t xprev = 0;   // the x the previous unit used (derived units)
        int u = unit_begin;
        auto multiply = [&](const unsigned (&w)[UB], const val_t (&xg)[UB], const grp_t (&vg)[NG], auto tail) {
#pragma clang fp contract(off)
#pragma unroll
            for (int k = 0; k < UB; k++) {
                val_t xu = xg[k];
                if constexpr (DERIVED) { xu = unit_x_use(xg[k], xprev, w[k], r); xprev = xu; }
                if (!decltype(tail)::value || u + k < unit_end) retire((val_t)vg[k / G][k % G] * xu, w[k] >> 24);
            }
        };
        const grp_t *vnext = ugrp + (long long)(unit_begin + UB) * (16 / G);
        // Batch u, at place j of its chunk: the gathers and the values of the next batch are issued, then batch u is multiplied.  Nothing
        // that a load is in flight into is ever copied (a copy waits for its data): the buffers take turns by the place in the chunk, which the unrolled loop body knows.
        // The refill's loads go behind them: no counted wait of the loop reaches them before the next refill.
        auto step = [&](auto j_) {
            constexpr int j = decltype(j_)::value, jg = (j + 1) % NB;   // (place of the next batch)
            gather(jg * UB, w0[jg % DEPTH], xv[jg % DEPTH]);
            load_values(u + UB, vnext, vs[(j + 1) % 2]);
            vnext += UB * (16 / G);
            if constexpr (jg == NB - 1) refill();
            __builtin_amdgcn_sched_barrier(0);   // every load of the iteration is issued before the first product
            multiply(w0[j % DEPTH], xv[j % DEPTH], vs[j % 2], std::false_type());
            u += UB;
        };
        const int ulast = unit_begin + (unit_end - 1 - unit_begin) / UB * UB;   // first unit of the task's last batch, which has nothing behind it to load for and is the
        gather(0, w0[0], xv[0]);                                                 // only one whose units are tested against the task's end
        // Whole chunks: NB steps in one block without a way out.  (With an exit between the steps the compiler's counted waits give way to vmcnt(0): the structured control
        // flow joins paths on which different loads are outstanding.)
        while (u + (NB - 1) * UB < ulast) {
            step(std::integral_constant<int, 0>());
            step(std::integral_constant<int, 1>());
            step(std::integral_constant<int, 2>());
            step(std::integral_constant<int, 3>());
        }
        // ... then at most NB - 1 steps and the last batch, at place j of its chunk
        auto rest = [&](auto self, auto j_) -> void {
            constexpr int j = decltype(j_)::value;
            if constexpr (j + 1 < NB) {
                if (u < ulast) { step(j_); self(self, std::integral_constant<int, j + 1>()); return; }
            }
            multiply(w0[j % DEPTH], xv[j % DEPTH], vs[j % 2], std::true_type());
        };
        rest(rest, std::integral_constant<int, 0>());
    }
    // rows without any unit are zero; then y, once per strip, 16 bytes per lane: tile-row k of the strip is row0 + k * strip_stride
    for (unsigned m = nounit; m; m &= m - 1) {
        const int kr = __ffs((int)m) - 1;
        if constexpr (sizeof(val_t) == sizeof(lacc_t)) s_y[g][kr][r] = 0;
        else reinterpret_cast<val_t *>(&s_y[g][kr][0])[r] = 0;
    }
    wave_lds_fence();
    constexpr int VEC = 16 / (int)sizeof(val_t);            // values per 16-byte lane store
    constexpr int ROWV = 128 / (int)sizeof(val_t);          // values of val_t per parked tile-row (128 bytes of LDS in both builds)
    const val_t *res = reinterpret_cast<const val_t *>(&s_y[g][0][0]);
    const int ystride = S.strip_stride;
    for (int i = r * VEC; i < 16 * nrows; i += 16 * VEC) {
        const long long yi = ((long long)row0 + (long long)(i >> 4) * ystride) * 16 + (i & 15);
        const val_t *rf = res + (i >> 4) * ROWV + (i & 15);
        if (yi + VEC <= rowA) {
            if (NT_Y && S.y_streaming) __builtin_nontemporal_store(*reinterpret_cast<const v4u_t *>(rf), reinterpret_cast<v4u_t *>(y + yi));
            else *reinterpret_cast<uint4 *>(y + yi) = *reinterpret_cast<const uint4 *>(rf);
        } else {
#pragma unroll
            for (int q = 0; q < VEC; q++) if (yi + q < rowA) y[yi + q] = rf[q];
        }
    }
}

// the unit-stream launch of a plan whose unit_deep_form is `depth` > 0, called by launch_tiles_stream in front of the lean launch; the whole-tile passes run behind it as behind any
hipError_t launch_units_deep(const DevPlan &P, const DevStream &S, int depth, int entry_mode, int wg_strips, int lds_pad_bytes, int xcd_chunk, const val_t *x, val_t *y, hipStream_t st)
{
    if (depth != unit_deep_form(S, entry_mode, wg_strips) || depth < 1) return hipErrorInvalidValue;   // (the caller asks the same function)
    const bool derived = unit_lean_form(S, entry_mode, wg_strips) == 1;
#define TSPMV_KD(CD, VF, DV) hipLaunchKernelGGL((k_units_deep<UNIT_DEEP_UB, UNIT_DEEP_DEPTH, CD, VF, DV>), dim3((unsigned)((S.ntasks + 15) / 16)), dim3(256), (size_t)lds_pad_bytes, st, S, P.rowA, P.colA, xcd_chunk, x, y)
#define TSPMV_KD_DV(CD, VF) do { if (derived) TSPMV_KD(CD, VF, true); else TSPMV_KD(CD, VF, false); } while (0)
#define TSPMV_KD_CD(VF) do { if (S.cb_bits > 0) TSPMV_KD_DV(true, VF); else TSPMV_KD_DV(false, VF); } while (0)
#if !defined(TILESPMV_F32)
    if (S.uval_narrow == 2) TSPMV_KD_CD(2);
    else if (S.uval_narrow == 1) TSPMV_KD_CD(1);
    else
#endif
    TSPMV_KD_CD(0);
#undef TSPMV_KD_CD
#undef TSPMV_KD_DV
#undef TSPMV_KD
    return hipGetLastError();
}

}  // namespace tilespmv
