// hip_solver_common.h — what the device-resident solvers share (hip_solver.hip, hip_solver_mv.hip, hip_solver_ls.hip, hip_solver_bi.hip, hip_solver_mr.hip, hip_solver_gm.hip): the launch shape, the number of
// partial sums, the reduction tree, the walk over a vector in its three forms (sv_walk, sv_walk_loaded, sv_dot: a kernel states its element-wise body once, for the 16-byte lane
// vectors and the scalar tail alike), and the host-side driver around the kernels: the one allocation (DeviceBlock), the versioned state structs (cg_state_of,
// state_read, put_versioned), the loop of *_solve with its convergence test (solve_loop, RrBbTest), the start of a create and the end of a solver (square_system, destroy_solver),
// and the one-thread-per-row launch of tilespmv_csr_*_device (launch_per_row).
//
// No scalar ever visits the host: a reducing kernel writes one partial per workgroup and the CONSUMING kernel folds the partials itself — every workgroup the same additions in the
// same order, so all of them hold the same bits of the scalar; no finishing launch, no atomics.  The number of partials (solver_parts) and which elements a thread adds depend on the
// vector's length alone, the wave and workgroup reductions are fixed trees: the order of every sum is fixed by the problem size.  Partial sums and scalars are double in both builds.
#pragma once

#include <algorithm>
#include <cstring>

#include "hip_plan_internal.h"

namespace tilespmv {
namespace {

constexpr int SVB = 256;                              // threads per workgroup
constexpr int SV_VPL = 16 / (int)sizeof(val_t);       // elements per 16-byte lane load (2 in fp64, 4 in fp32)
constexpr int SV_U = 2;                               // lane vectors per lane and trip: a workgroup's trip covers SV_U * SVB consecutive lane vectors
constexpr int SV_MAX_PARTS = 1024;                    // partial sums = workgroups of the streaming kernels: 4 per CU on 256 CUs
typedef val_t svec_t __attribute__((ext_vector_type(SV_VPL)));

// workgroups (= partial sums) for a stream of `elements` values: a function of that length alone
inline int solver_parts(long long elements)
{
    const long long trips = (elements / SV_VPL + (long long)SV_U * SVB - 1) / ((long long)SV_U * SVB);
    return (int)std::max<long long>(1, std::min<long long>(SV_MAX_PARTS, trips));
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
// the workgroup's sum, returned to every thread: wave trees, then the four wave sums in wave order
__device__ __forceinline__ double block_sum(double v, double *s)
{
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    const double t = ((s[0] + s[1]) + s[2]) + s[3];
    __syncthreads();
    return t;
}
// the sum of np partials, the same additions in every workgroup
__device__ __forceinline__ double fold(const double *__restrict__ part, int np, double *s)
{
    double a = 0.0;
    for (int i = threadIdx.x; i < np; i += SVB) a += part[i];
    return block_sum(a, s);
}

// a vector as its 16-byte lane vectors
__device__ __forceinline__ svec_t *lanes(val_t *p) { return reinterpret_cast<svec_t *>(p); }
__device__ __forceinline__ const svec_t *lanes(const val_t *p) { return reinterpret_cast<const svec_t *>(p); }

// Element ranges of a vector of n elements served by nwg workgroups: the full lane vectors [0, nv), nv = n / SV_VPL, are walked in trips of SV_U * SVB by workgroup blockIdx.x,
// blockIdx.x + nwg, ...; the n % SV_VPL elements behind them belong to thread 0 of workgroup 0 (scalar accesses: nothing past element n - 1 of a caller's vector is touched).
// nwg is gridDim.x, or less: then the kernel keeps the workgroups from nwg on out of the walk itself (no guard here: it would cost the kernels that need none).
#define SV_FOR_TRIPS(base, nv, nwg) for (long long base = (long long)blockIdx.x * (SV_U * SVB) + threadIdx.x; base < (nv); base += (long long)(nwg) * (SV_U * SVB))

// A kernel states its element-wise body ONCE, as a generic lambda over a position of the walk: SvLane (lane vector v, values are svec_t) in the trips, SvTail (element i, values are
// val_t) in the scalar tail.  at(p) loads from the vector p, at.put(p, x) stores; the arithmetic in between is the same expression on either value type, so the two forms round alike.
// SV_FOR_TRIPS is still written out where a trip is more than that: the loops over the basis of hip_solver_gm.hip (gm_group_dots, gm_subtract, k_gm_update), the per-column
// accumulators of hip_solver_mv.hip (k_cgm_*), the LDS slab of hip_precond.hip (k_bj_apply).
struct SvLane {
    long long v;
    __device__ __forceinline__ svec_t operator()(const val_t *p) const { return lanes(p)[v]; }
    __device__ __forceinline__ void put(val_t *p, svec_t x) const { lanes(p)[v] = x; }
};
struct SvTail {
    long long i;
    __device__ __forceinline__ val_t operator()(const val_t *p) const { return p[i]; }
    __device__ __forceinline__ void put(val_t *p, val_t x) const { p[i] = x; }
};
// acc += a . b in double: the SV_VPL products of a lane vector in element order, or the one product of a tail element
__device__ __forceinline__ void sv_mac(double &acc, svec_t a, svec_t b)
{
#pragma unroll
    for (int q = 0; q < SV_VPL; q++) acc += (double)a[q] * (double)b[q];
}
__device__ __forceinline__ void sv_mac(double &acc, val_t a, val_t b) { acc += (double)a * (double)b; }

// f(at) at every position of a vector of n elements: a lane vector is loaded, used and stored before the trip's next one is touched
template <class F> __device__ __forceinline__ void sv_walk(long long n, int nwg, F f)
{
    const long long nv = n / SV_VPL;
    SV_FOR_TRIPS(base, nv, nwg) {
#pragma unroll
        for (int u = 0; u < SV_U; u++) {
            const long long v = base + u * SVB;
            if (v < nv) f(SvLane{v});
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long long i = nv * SV_VPL; i < n; i++) f(SvTail{i});
}
// The same in two phases: load(at, t) fills the kernel's value struct Vals<svec_t or val_t> t, use(at, t) computes and stores.  All SV_U loads of a trip are issued before any
// arithmetic: more bytes in flight (and more registers) than sv_walk, for the kernels of the iteration that are bound by the memory.
template <template <class> class Vals, class Load, class Use> __device__ __forceinline__ void sv_walk_loaded(long long n, int nwg, Load load, Use use)
{
    const long long nv = n / SV_VPL;
    SV_FOR_TRIPS(base, nv, nwg) {
        Vals<svec_t> t[SV_U];
#pragma unroll
        for (int u = 0; u < SV_U; u++) {
            const long long v = base + u * SVB;
            if (v < nv) load(SvLane{v}, t[u]);
        }
#pragma unroll
        for (int u = 0; u < SV_U; u++) {
            const long long v = base + u * SVB;
            if (v < nv) use(SvLane{v}, t[u]);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long long i = nv * SV_VPL; i < n; i++) {
            Vals<val_t> t;
            load(SvTail{i}, t);
            use(SvTail{i}, t);
        }
}
// The pure dot kernels: f(a, b) with the values of the vectors a and b at every position (a == b: of the one vector).  Nothing is stored, so the lane vectors behind the end of a
// partial last trip are zeros and f runs unguarded: f adds into 1-3 accumulators with sv_mac, and a zero adds nothing.
template <class F> __device__ __forceinline__ void sv_dot(long long n, int nwg, const val_t *a, const val_t *b, F f)
{
    const long long nv = n / SV_VPL;
    SV_FOR_TRIPS(base, nv, nwg) {
        svec_t va[SV_U], vb[SV_U];
#pragma unroll
        for (int u = 0; u < SV_U; u++) {
            const long long v = base + u * SVB;
            if (v < nv) { va[u] = lanes(a)[v]; vb[u] = lanes(b)[v]; }
            else { va[u] = (val_t)0; vb[u] = (val_t)0; }
        }
#pragma unroll
        for (int u = 0; u < SV_U; u++) f(va[u], vb[u]);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long long i = nv * SV_VPL; i < n; i++) f(a[i], b[i]);
}

// the tail of the k_csr_* kernels under `invert`: 1 / d, 1 where d is 0 (a macro: as an inlined function it reaches the kernels as a select, and their code changes)
#define SV_INVERSE_OR_ONE(d) ((d) == (val_t)0 ? (val_t)1 : (val_t)1 / (d))

inline bool misaligned(const void *p) { return ((uintptr_t)p & 15u) != 0; }
// the plan of a whole rows x cols matrix (no shard)
inline bool whole_plan(const tilespmv_plan *plan, long long rows, long long cols)
{
    return plan->matrix_rows == rows && plan->dev.colA == cols && plan->dev.f_row0 == 0 && plan->dev.f_rows == rows;
}
// bytes of a work vector of rows x nvec elements inside a solver's allocation: 16 rows of slack, rounded to 256
inline size_t vec_bytes(long long rows, int nvec = 1) { return ((size_t)(rows + 16) * nvec * sizeof(val_t) + 255) / 256 * 256; }

// A solver's one allocation: zeroed, then handed out in consecutive pieces (the caller adds up their sizes; multiples of 256 keep every piece aligned).  A failed alloc leaves nothing.
struct DeviceBlock {
    char *base = nullptr, *at = nullptr;
    hipError_t alloc(size_t bytes)
    {
        hipError_t e = hipMalloc((void **)&base, bytes);
        if (e == hipSuccess) e = hipMemset(base, 0, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            if (base) (void)hipFree(base);
            base = nullptr;
        }
        at = base;
        return e;
    }
    template <class T> T *take(size_t bytes)
    {
        T *p = (T *)at;
        at += bytes;
        return p;
    }
};

// a scalar block on the host, after a synchronisation of the stream
inline hipError_t read_scalars(void *dst, const void *src, size_t bytes, hipStream_t st)
{
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) (void)hipGetLastError();
    return e;
}
// element j of a caller's array of state structs whose elements are `stride` bytes apart (a caller built against a shorter struct gets the fields it knows)
template <class State> void put_versioned(State *out, unsigned stride, int j, State s)
{
    s.size = stride;
    memcpy((char *)out + (size_t)j * stride, &s, std::min<size_t>(stride, sizeof(s)));
}

// ---- the host-side driver: what the extern "C" entry points of every solver do around their kernels (DESIGN.md §3.7 "The driver")

constexpr size_t SV_PARTS_BYTES = (size_t)SV_MAX_PARTS * sizeof(double);   // one array of partial sums inside a solver's allocation

// the status the device's scalars stand for (MAXITER is the solve loop's alone): `residual` is the squared norm whose exact zero means converged
inline int device_status(int breakdown, double residual)
{
    return breakdown ? TILESPMV_CG_BREAKDOWN : residual == 0.0 ? TILESPMV_CG_CONVERGED : TILESPMV_CG_RUNNING;
}
// a scalar block with iterations, breakdown, rr, bb as a whole tilespmv_cg_state
template <class Scal> tilespmv_cg_state cg_state_of(const Scal &h)
{
    tilespmv_cg_state s;
    s.size = sizeof(s);
    s.iterations = h.iterations;
    s.status = device_status(h.breakdown, h.rr);
    s.rr = h.rr; s.bb = h.bb;
    return s;
}
// *_state_read behind the handle's null check: the device's scalar block d_S, converted by `convert`, in the caller's struct of out->size bytes
template <class Scal, class State> int state_read(const Scal *d_S, hipStream_t st, State *out, State (*convert)(const Scal &))
{
    if (!out || out->size < 3 * sizeof(int)) return (int)hipErrorInvalidValue;
    Scal h;
    const hipError_t e = read_scalars(&h, d_S, sizeof(h), st);
    if (e != hipSuccess) return (int)e;
    put_versioned(out, out->size, 0, convert(h));
    return 0;
}

// The convergence test of a solve on tilespmv_cg_state: rr <= rtol^2 bb, and b = 0 has the solution 0.  (CGLS has its own on nn and nn0: hip_solver_ls.hip.)
struct RrBbTest {
    static double residual(const tilespmv_cg_state &s) { return s.rr; }
    static double scale(const tilespmv_cg_state &s) { return s.bb; }
    static void at_zero_scale(tilespmv_cg_state &s) { s.rr = 0.0; }
};
// *_solve of a single system behind the handle's null check.  begin(), read() (the solver's state_read into `out`) and iterate(count) are the solver's own entry points; d_x has
// x_len elements.  Refusals come before any launch; one read, hence one synchronisation, per check_every iterations; the last batch is clipped to maxiter.
// confirm(accepted) is asked when a read passes the test, before CONVERGED is declared: a solver whose recurrence may run ahead of the true residual (GMRES with a narrow basis)
// recomputes it there, fills `out` again and clears `accepted` to carry on.  The default accepts at once: the other solvers' loops are what they were.
struct AcceptAtOnce {
    int operator()(bool &) const { return 0; }
};
template <class Test, class State, class Begin, class Read, class Iterate, class Confirm = AcceptAtOnce>
int solve_loop(State *out, val_t *d_x, long long x_len, double rtol, int maxiter, int check_every, hipStream_t st, Begin begin, Read read, Iterate iterate, Confirm confirm = Confirm())
{
    if (!out || out->size < sizeof(State) || maxiter < 0) return (int)hipErrorInvalidValue;
    if (check_every < 1) check_every = 1;
    int rc = begin();
    if (rc) return rc;
    for (;;) {
        rc = read();
        if (rc) return rc;
        if (out->status == TILESPMV_CG_BREAKDOWN) return 0;
        if (Test::scale(*out) == 0.0) {   // the solution is 0
            const hipError_t e = hipMemsetAsync(d_x, 0, (size_t)x_len * sizeof(val_t), st);
            if (e != hipSuccess) return (int)e;
            Test::at_zero_scale(*out);
            out->status = TILESPMV_CG_CONVERGED;
            return (int)hipStreamSynchronize(st);
        }
        if (Test::residual(*out) <= rtol * rtol * Test::scale(*out)) {
            bool accepted = true;
            rc = confirm(accepted);
            if (rc) return rc;
            if (accepted) { out->status = TILESPMV_CG_CONVERGED; return 0; }
        }
        if (out->iterations >= maxiter) { out->status = TILESPMV_CG_MAXITER; return 0; }
        rc = iterate(std::min(check_every, maxiter - out->iterations));
        if (rc) return rc;
    }
}

// The start of a create for a square system: *out is NULL from here on unless the create succeeds; the plan is the whole of a square matrix, the borrowed diagonal (may be NULL)
// is aligned.  Returns the number of rows, or 0: refuse with hipErrorInvalidValue.
template <class Solver> long long square_system(Solver **out, const tilespmv_plan *plan, const void *d_diag)
{
    if (out) *out = nullptr;
    if (!out || !plan) return 0;
    const long long n = plan->matrix_rows;
    return (n <= 0 || !whole_plan(plan, n, n) || misaligned(d_diag)) ? 0 : n;
}
// the end of a solver whose one allocation is `block`
template <class Solver> void destroy_solver(Solver *s)
{
    if (!s) return;
    (void)hipFree(s->block);
    delete s;
}

// The tilespmv_csr_*_device entry points: kernel `k`, one thread per row of a device CSR.  idx (column indices, or positions in the value array) may be NULL where idx_optional.
template <class Kernel> int launch_per_row(Kernel k, int rows, const int *d_rowPtr, const int *d_idx, bool idx_optional, const val_t *d_val, val_t *d_out, int invert, void *stream)
{
    if (rows < 0 || (rows > 0 && (!d_rowPtr || (!d_idx && !idx_optional) || !d_val || !d_out))) return (int)hipErrorInvalidValue;
    if (tilespmv_device_count() <= 0) return (int)hipErrorNoDevice;
    if (rows > 0) hipLaunchKernelGGL(k, dim3((unsigned)((rows + SVB - 1) / SVB)), dim3(SVB), 0, (hipStream_t)stream, rows, d_rowPtr, d_idx, d_val, d_out, invert);
    return (int)hipGetLastError();
}

}  // namespace
}  // namespace tilespmv
