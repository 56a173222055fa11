// hip_value_map.hip — new values for a plan whose pattern stays (TILESPMV_CREATE_VALUE_MAP, tilespmv_plan_update_values).
//
// A flagged plan is built from stand-in values (hip_tile_create.h vmap_encode: the value of CSR position j carries j in its bits), so when the builder is done every value slot of
// the value-carrying streams names its source nonzero.  value_map_attach reads those names into the map (int32 per slot, -1 for padding) and then writes the caller's values in
// by the same pass that tilespmv_plan_update_values runs later: slot = position < 0 ? 0 : csrVal[position].
// The value-carrying streams of a device-built plan: DevStream::uval (grouped and interleaved per row by k_pair_values), DevStream::cval, the value words of DevStream::grec, and
// DevDense::val; DevPlan::val (whole CSR tiles, csr_split = 0) has no device path and is empty in these plans, but is listed so that a slot can never be missed.
#include <hip/hip_runtime.h>

#include "hip_plan_internal.h"
#include "hip_tile_create.h"

namespace tilespmv {
namespace {

constexpr int VB = 256;                              // threads per workgroup
constexpr int VPL = 16 / (int)sizeof(val_t);         // value slots per lane of a plain stream: one 16-byte store (2 in fp64, 4 in fp32)
typedef val_t vvec_t __attribute__((ext_vector_type(VPL)));
typedef int ivec_t __attribute__((ext_vector_type(VPL)));

struct VSeg {
    val_t *dst;          // the stream (plain values, or ERec records)
    const int *map;      // its part of the map (16-byte aligned)
    long long n;         // value slots (records)
    long long blk0;      // first workgroup of this stream in the launch
    int erec;
};
struct VTable { VSeg s[tilespmv_plan::VMAP_STREAMS]; int nseg; };

// One launch over every value-carrying stream, the streams back to back: consecutive workgroups cover consecutive slots of a stream, and a stream is in task order — neighbouring
// workgroups gather from neighbouring tile-rows of csrVal (the rows of one L2's share stay in it).  Plain streams: VPL slots per lane, 16-byte map load, VPL gathers, one 16-byte store.
// Entry records: one record per lane, its value words only (the index word stays).
template <bool NT>
__global__ __launch_bounds__(VB) void k_refresh_values(const VTable T, const val_t *__restrict__ v)
{
    int k = 0;
    while (k + 1 < T.nseg && (long long)blockIdx.x >= T.s[k + 1].blk0) k++;
    const VSeg S = T.s[k];
    const long long lane = ((long long)blockIdx.x - S.blk0) * VB + threadIdx.x;
    if (S.erec) {
        if (lane >= S.n) return;
        const int j = NT ? __builtin_nontemporal_load(S.map + lane) : S.map[lane];
        const val_t x = j < 0 ? (val_t)0 : v[j];
        ERec *R = reinterpret_cast<ERec *>(S.dst) + lane;
        unsigned w[sizeof(val_t) / 4];
        __builtin_memcpy(w, &x, sizeof(val_t));
        unsigned *o = reinterpret_cast<unsigned *>(R);   // (ERec: the value words first — lo, hi in fp64, v in fp32 — then the index word)
#pragma unroll
        for (int z = 0; z < (int)(sizeof(val_t) / 4); z++) {
            if constexpr (NT) __builtin_nontemporal_store(w[z], o + z);
            else o[z] = w[z];
        }
        return;
    }
    const long long i0 = lane * VPL;
    if (i0 >= S.n) return;
    if (i0 + VPL <= S.n) {
        const ivec_t *mp = reinterpret_cast<const ivec_t *>(S.map + i0);
        const ivec_t j = NT ? __builtin_nontemporal_load(mp) : *mp;
        vvec_t x;
#pragma unroll
        for (int q = 0; q < VPL; q++) x[q] = j[q] < 0 ? (val_t)0 : v[j[q]];
        vvec_t *dp = reinterpret_cast<vvec_t *>(S.dst + i0);
        if constexpr (NT) __builtin_nontemporal_store(x, dp);
        else *dp = x;
        return;
    }
    for (long long i = i0; i < S.n; i++) { const int j = S.map[i]; S.dst[i] = j < 0 ? (val_t)0 : v[j]; }   // (the stream's last, partial vector)
}

// the map from the stand-in values the builder moved into the streams; a position outside [0, limit) sets *bad
__global__ __launch_bounds__(VB) void k_read_map(const VTable T, long long limit, int *__restrict__ map_base, int *__restrict__ bad)
{
    int k = 0;
    while (k + 1 < T.nseg && (long long)blockIdx.x >= T.s[k + 1].blk0) k++;
    const VSeg S = T.s[k];
    const long long i = ((long long)blockIdx.x - S.blk0) * VB + threadIdx.x;
    if (i >= S.n) return;
    val_t x;
    if (S.erec) {
        const unsigned *o = reinterpret_cast<const unsigned *>(reinterpret_cast<const ERec *>(S.dst) + i);
        unsigned w[sizeof(val_t) / 4];
        for (int z = 0; z < (int)(sizeof(val_t) / 4); z++) w[z] = o[z];
        __builtin_memcpy(&x, w, sizeof(val_t));
    } else x = S.dst[i];
    const long long j = vmap_decode(x);
    if (j >= limit) { atomicOr(bad, 1); return; }
    map_base[(S.map - map_base) + i] = (int)j;
}

inline long long blocks_of(long long n, bool erec) { return erec ? (n + VB - 1) / VB : (n + (long long)VB * VPL - 1) / ((long long)VB * VPL); }

// the launch table of the plan's streams; per_slot: one thread per slot (the map read) instead of VPL slots per lane
VTable table_of(const tilespmv_plan *plan, bool per_slot, long long *nblocks)
{
    VTable T{};
    long long b = 0;
    for (int k = 0; k < plan->vmap_streams; k++) {
        VSeg &S = T.s[T.nseg];
        S.dst = const_cast<val_t *>(reinterpret_cast<const val_t *>(*plan->vmap_slot[k]));
        S.map = plan->vmap + plan->vmap_off[k];
        S.n = plan->vmap_n[k];
        S.erec = plan->vmap_erec[k] ? 1 : 0;
        if (S.n <= 0 || !S.dst) continue;
        S.blk0 = b;
        b += per_slot ? (S.n + VB - 1) / VB : blocks_of(S.n, S.erec);
        T.nseg++;
    }
    *nblocks = b;
    return T;
}

hipError_t launch_refresh(const tilespmv_plan *plan, const val_t *d_val, hipStream_t st)
{
    long long nb = 0;
    const VTable T = table_of(plan, false, &nb);
    if (nb == 0) return hipSuccess;
    if (nb > INT32_MAX) return hipErrorInvalidValue;
    if (plan->st.nt_stream) hipLaunchKernelGGL(k_refresh_values<true>, dim3((unsigned)nb), dim3(VB), 0, st, T, d_val);
    else hipLaunchKernelGGL(k_refresh_values<false>, dim3((unsigned)nb), dim3(VB), 0, st, T, d_val);
    return hipGetLastError();
}

}  // namespace

int value_map_attach(tilespmv_plan *plan, long long limit, const val_t *d_val)
{
    // the value-carrying streams, as the builder recorded them (upload() / reserve(): the member it filled, its bytes)
    const void *members[tilespmv_plan::VMAP_STREAMS] = {&plan->st.uval, &plan->st.cval, &plan->dn.val, &plan->st.grec, &plan->dev.val};
    const bool erec[tilespmv_plan::VMAP_STREAMS] = {false, false, false, true, false};
    long long total = 0;
    plan->vmap_streams = 0;
    for (int m = 0; m < tilespmv_plan::VMAP_STREAMS; m++)
        for (size_t i = 0; i < plan->uploaded_slots.size(); i++) {
            if ((const void *)plan->uploaded_slots[i] != members[m]) continue;
            const int k = plan->vmap_streams++;
            plan->vmap_slot[k] = plan->uploaded_slots[i];
            plan->vmap_erec[k] = erec[m];
            plan->vmap_n[k] = (long long)(plan->uploaded_bytes[i] / (erec[m] ? sizeof(ERec) : sizeof(val_t)));
            plan->vmap_off[k] = total;
            total += (plan->vmap_n[k] + 3) / 4 * 4;   // (every stream's part starts 16-byte aligned)
            break;
        }
    const size_t bytes = (size_t)std::max<long long>(total, 4) * sizeof(int);
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); fprintf(stderr, "tilespmv: value map: device allocation of %zu MB failed\n", bytes >> 20); return -3; }
    plan->allocs.push_back(p);
    plan->vmap = (int *)p;
    plan->info[TILESPMV_INFO_VALUE_MAP_BYTES] = (long long)total * (long long)sizeof(int);
    int *d_bad = nullptr;
    hipError_t e = hipMemset(p, 0xFF, bytes);   // (-1: padding, also between the streams' parts)
    if (e == hipSuccess) e = hipMalloc((void **)&d_bad, sizeof(int));
    if (e == hipSuccess) e = hipMemset(d_bad, 0, sizeof(int));
    long long nb = 0;
    const VTable T = table_of(plan, true, &nb);
    if (e == hipSuccess && nb > INT32_MAX) e = hipErrorInvalidValue;
    if (e == hipSuccess && nb > 0) {
        hipLaunchKernelGGL(k_read_map, dim3((unsigned)nb), dim3(VB), 0, 0, T, limit, plan->vmap, d_bad);
        e = hipGetLastError();
    }
    int bad = 0;
    if (e == hipSuccess) e = hipMemcpy(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost);
    if (d_bad) (void)hipFree(d_bad);
    if (e == hipSuccess && bad) { fprintf(stderr, "tilespmv: internal error: a value slot of the plan names no nonzero of the CSR arrays\n"); return -6; }
    if (e == hipSuccess) e = launch_refresh(plan, d_val, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { fprintf(stderr, "tilespmv: value map: HIP error %d (%s)\n", (int)e, hipGetErrorString(e)); (void)hipGetLastError(); return -3; }
    return 0;
}

}  // namespace tilespmv

extern "C" int tilespmv_plan_update_values(tilespmv_plan *plan, const MAT_VAL_TYPE *d_csrVal, void *stream)
{
    if (!plan) return (int)hipErrorInvalidValue;
    if (!plan->vmap) return TILESPMV_ERR_NO_VALUE_MAP;
    if (!d_csrVal) return (int)hipErrorInvalidValue;
    return (int)tilespmv::launch_refresh(plan, d_csrVal, (hipStream_t)stream);
}
