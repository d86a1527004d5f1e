// Scans of any density: a deterministic voxel-grid subsample in front of the eval loops and a nearest-point
// search that carries results to point sets that were never in the grid.  The host statements are
// postprocess.grid_subsample_host and postprocess.nearest_point_host; see include/geoformer_hip.h for the arguments.
//
// gf_grid_subsample (the first five steps are voxelize_idx.hip's, keyed by a cell of floats instead of integer voxels):
//   k_rs_bounds  (default origin only) per-axis minimum of the points as order-preserving 32-bit keys (post_steps.h's
//                gf_float_key): at most 512 workgroups stride over the points, reduce in registers and LDS and issue one
//                integer atomicMin per axis
//   k_rs_org     one thread: the origin of the call -- the caller's three floats or the decoded minimum -- into scratch
//   k_rs_insert  one thread per point: t = (p - origin) / cell (one subtraction, one correctly rounded division),
//                c = floor t, the cell key cx | cy << 21 | cz << 42 claimed in an open-addressing table by 64-bit CAS;
//                per slot an integer atomicMin of the point index ("first"), an integer atomicAdd of 1 (the cell's count)
//                and, in center mode, a 64-bit atomicMin of (d2 bits << 32 | index); an invalid point raises the flag
//   k_rs_sums, k_rs_top, k_rs_apply   exclusive scan, in POINT order, of "I am my cell's first": the cell's number in
//                order of first occurrence (k_rs_top carries across 256 block sums: N > 65 536)
//   k_rs_write   one thread per point: cell_of; a cell's first point also writes rep and count of its cell
// Minima and integer sums only: no result depends on the order in which the points arrive, and no float is ever added
// atomically.  Seven launches at most and six memsets, all on the caller's stream; nothing is read back here.
//
// gf_nearest_point:
//   k_rs_bounds  per-axis minimum and maximum of the points whose three coordinates are finite, as above
//   k_np_plan    one thread: the minimum corner and 1 / cell as doubles, the extent in cells, the range flag
//   k_np_bin<count>, gf_iscan, k_np_bin<fill>   counting sort of (x, y, z, index) records into hashed buckets of cells
//                of max_dist * 1.001 (geodesic.hip's point grid, with the cell coordinate floor((p - lo) / cell) in fp64)
//   k_np_query   one thread per query: the 27 cells around its own, the minimum of (d2 bits << 32 | index) over the
//                records with d2 <= r2.  A bucket may hold several cells and several of the 27 cells may share a bucket;
//                a minimum does not care.  The order inside a bucket depends on arrival, the minimum does not.
#include "common.h"
#include "post_steps.h"

namespace {

typedef unsigned long long u64;

constexpr int RS_THREADS = 256;
constexpr int RS_MAX_POINTS = 1 << 29;  // the tables (2 N slots, 2^30 at most) are never full
constexpr int RS_AXIS_BITS = 21;
constexpr u64 RS_EMPTY = 0xffffffffffffffffull;
constexpr double NP_MAX_CELLS = 1073741824.0;  // 2^30 cells per axis: the proven range of the 27-cell walk

__device__ __forceinline__ bool finite3(float x, float y, float z) {
    return isfinite(x) && isfinite(y) && isfinite(z);
}
__device__ __forceinline__ unsigned wave_min_u(unsigned v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, d, 64));
    return v;
}
__device__ __forceinline__ unsigned wave_max_u(unsigned v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, d, 64));
    return v;
}

// per-axis minimum (lo[3]) and, with hi, maximum (hi[3]) of the points as keys; `all_axes`: a point counts only when its
// three coordinates are finite (nearest point), else every non-NaN coordinate counts on its own axis (subsample: a NaN
// or infinite point makes the call invalid whatever the origin is).  At most RS_BOUNDS_BLOCKS workgroups stride over the
// points; a workgroup reduces in registers and LDS and issues one atomic per axis and bound, and only when its value
// beats the word it reads first (the word only ever moves one way, so a stale read costs an atomic, never loses one):
// with one atomic per wave, a million points spent 540 us queueing on three addresses.
constexpr int RS_BOUNDS_BLOCKS = 512;
__global__ __launch_bounds__(RS_THREADS) void k_rs_bounds(const float* __restrict__ xyz, int N, int all_axes,
                                                          unsigned* __restrict__ lo, unsigned* __restrict__ hi) {
    __shared__ unsigned s_mn[RS_THREADS / 64][3], s_mx[RS_THREADS / 64][3];
    unsigned mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
    for (int i = blockIdx.x * RS_THREADS + threadIdx.x; i < N; i += gridDim.x * RS_THREADS) {  // N <= 2^29: no overflow
        const float p[3] = {xyz[(size_t)i * 3], xyz[(size_t)i * 3 + 1], xyz[(size_t)i * 3 + 2]};
        const bool ok = !all_axes || finite3(p[0], p[1], p[2]);
#pragma unroll
        for (int a = 0; a < 3; ++a)
            if (ok && p[a] == p[a]) {
                const unsigned k = gf_float_key(p[a]);
                mn[a] = min(mn[a], k);
                mx[a] = max(mx[a], k);
            }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const unsigned m = wave_min_u(mn[a]), M = wave_max_u(mx[a]);
        if ((threadIdx.x & 63) == 0) {
            s_mn[threadIdx.x >> 6][a] = m;
            s_mx[threadIdx.x >> 6][a] = M;
        }
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int a = threadIdx.x;
        unsigned m = 0xffffffffu, M = 0u;
#pragma unroll
        for (int w = 0; w < RS_THREADS / 64; ++w) {
            m = min(m, s_mn[w][a]);
            M = max(M, s_mx[w][a]);
        }
        if (m < __hip_atomic_load(&lo[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&lo[a], m);
        if (hi && M > __hip_atomic_load(&hi[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&hi[a], M);
    }
}

// ------------------------------------------------------------------------------------------------------------------
// grid subsample
// ------------------------------------------------------------------------------------------------------------------
struct RsScratch {
    u64* keys;        // [T] cell key of the slot
    u64* best;        // [T] center mode: min of (d2 bits << 32 | index)
    int* first;       // [T] lowest point index of the slot's cell
    int* cnt;         // [T] points of the slot's cell
    int* slot_of;     // [N] (-1: invalid point)
    int* rank;        // [N] exclusive scan of the "first" flags
    int* block_sums;  // [nb]
    int* block_off;   // [nb]
    unsigned* okey;   // [4] minimum of the points, as keys
    float* org;       // [4] the origin of the call
    int* words;       // [2] {M, invalid flag}
    unsigned T;
};

unsigned rs_table_size(int N) {
    unsigned t = 1024;
    while (t < 2u * (unsigned)(N > 0 ? N : 1)) t <<= 1;  // N <= 2^29
    return t;
}
int rs_nb(int N) { return (N + SCAN_THREADS - 1) / SCAN_THREADS + 1; }

RsScratch rs_carve(void* scratch, int N) {
    RsScratch s;
    s.T = rs_table_size(N);
    const size_t n1 = (size_t)(N > 0 ? N : 0) + 1;
    u64* p = (u64*)scratch;
    s.keys = p;
    p += s.T;
    s.best = p;
    p += s.T;
    int* q = (int*)p;
    s.first = q;
    q += s.T;
    s.cnt = q;
    q += s.T;
    s.slot_of = q;
    q += n1;
    s.rank = q;
    q += n1;
    s.block_sums = q;
    q += rs_nb(N);
    s.block_off = q;
    q += rs_nb(N);
    s.okey = (unsigned*)q;
    q += 4;
    s.org = (float*)q;
    q += 4;
    s.words = q;
    return s;
}

template <class T>
__device__ __forceinline__ T rs_peek(const T* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void k_rs_org(const float* __restrict__ origin, RsScratch s) {
    if (threadIdx.x < 3) s.org[threadIdx.x] = origin ? origin[threadIdx.x] : gf_float_unkey(s.okey[threadIdx.x]);
}

__global__ __launch_bounds__(RS_THREADS) void k_rs_insert(const float* __restrict__ xyz, int N, float cell, int center,
                                                          RsScratch s) {
    const int i = blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= N) return;
    const float lim = (float)(1 << RS_AXIS_BITS);
    float p[3], c[3];
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        p[a] = xyz[(size_t)i * 3 + a];
        const float t = __fdiv_rn(p[a] - s.org[a], cell);
        c[a] = floorf(t);
        ok = ok && isfinite(t) && c[a] >= 0.0f && c[a] < lim;
    }
    if (!ok) {
        s.words[1] = 1;
        s.slot_of[i] = -1;
        return;
    }
    const u64 key = (u64)(unsigned)c[0] | ((u64)(unsigned)c[1] << RS_AXIS_BITS) | ((u64)(unsigned)c[2] << (2 * RS_AXIS_BITS));
    unsigned slot = (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 32) & (s.T - 1);
    // Every word below moves one way only (a key is written once, a minimum only falls), so each is read first and the
    // atomic issued only when it can change something: a stale read costs an atomic, never loses one.
    while (true) {  // the table has 2 N slots: a free one is always found
        u64 old = rs_peek(&s.keys[slot]);
        if (old == RS_EMPTY) old = atomicCAS(&s.keys[slot], RS_EMPTY, key);
        if (old == RS_EMPTY || old == key) break;
        slot = (slot + 1) & (s.T - 1);
    }
    if (i < rs_peek(&s.first[slot])) atomicMin(&s.first[slot], i);
    atomicAdd(&s.cnt[slot], 1);
    if (center) {
        float d[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) d[a] = p[a] - (s.org[a] + (c[a] + 0.5f) * cell);
        const float d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];  // >= +0 or +inf, never NaN: p and the centre are not both infinite
        const u64 mine = ((u64)__float_as_uint(d2) << 32) | (unsigned)i;
        if (mine < rs_peek(&s.best[slot])) atomicMin(&s.best[slot], mine);
    }
    s.slot_of[i] = (int)slot;
}

__device__ __forceinline__ int rs_flag(const RsScratch& s, int i, int N) {
    if (i >= N) return 0;
    const int slot = s.slot_of[i];
    return slot >= 0 && s.first[slot] == i ? 1 : 0;
}
__global__ __launch_bounds__(SCAN_THREADS) void k_rs_sums(RsScratch s, int N) {
    int total;
    block_excl_scan(rs_flag(s, blockIdx.x * SCAN_THREADS + threadIdx.x, N), &total);
    if (threadIdx.x == 0) s.block_sums[blockIdx.x] = total;
}
__global__ __launch_bounds__(SCAN_THREADS) void k_rs_top(RsScratch s, int nb) {
    int carry = 0;  // (every thread adds the same totals: the carry needs no LDS word of its own)
    for (int base = 0; base < nb; base += SCAN_THREADS) {
        const int i = base + threadIdx.x;
        int total;
        const int ex = block_excl_scan(i < nb ? s.block_sums[i] : 0, &total);
        if (i < nb) s.block_off[i] = carry + ex;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) s.words[0] = carry;
}
__global__ __launch_bounds__(SCAN_THREADS) void k_rs_apply(RsScratch s, int N) {
    const int i = blockIdx.x * SCAN_THREADS + threadIdx.x;
    int total;
    const int ex = block_excl_scan(rs_flag(s, i, N), &total);
    if (i < N) s.rank[i] = s.block_off[blockIdx.x] + ex;
}

__global__ __launch_bounds__(RS_THREADS) void k_rs_write(int N, int center, RsScratch s, int32_t* __restrict__ rep,
                                                         int32_t* __restrict__ cell_of, int32_t* __restrict__ count) {
    const int i = blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= N) return;
    const int slot = s.slot_of[i];
    if (slot < 0) {  // (the call is invalid: the wrapper raises; nothing is indexed through this point)
        cell_of[i] = -1;
        return;
    }
    const int f = s.first[slot];  // in [0, N): the minimum of indices that were all below N
    const int m = s.rank[f];      // in [0, M), M <= N
    cell_of[i] = m;
    if (f == i) {
        rep[m] = center ? (int)(unsigned)(s.best[slot] & 0xffffffffull) : i;
        count[m] = s.cnt[slot];
    }
}

// ------------------------------------------------------------------------------------------------------------------
// nearest point
// ------------------------------------------------------------------------------------------------------------------
struct NpPlan {
    double lo[3], inv_cell;
    double ext[3];  // the far corner, in cells
    int any, pad_;
};

struct NpScratch {
    int32_t *counts, *start, *cursor, *block_sums, *block_off;
    unsigned* bkey;  // [8]: lo keys [0..2], hi keys [4..6]
    NpPlan* plan;
    float4* sorted;  // [n]
    unsigned T;
};

unsigned np_table_size(int n) {
    unsigned t = 1024;
    while (t < 2u * (unsigned)(n > 0 ? n : 1) && t < (1u << 26)) t <<= 1;
    return t;
}

NpScratch np_carve(void* scratch, int n) {
    NpScratch s;
    s.T = np_table_size(n);
    const int nb = gf_iscan_blocks((int)s.T);
    int32_t* q = (int32_t*)scratch;
    s.counts = q;
    q += s.T;
    s.start = q;
    q += s.T + 1;
    s.cursor = q;
    q += s.T;
    s.block_sums = q;
    q += nb;
    s.block_off = q;
    q += nb;
    s.bkey = (unsigned*)q;
    q += 8;
    uintptr_t sp = ((uintptr_t)q + 63) & ~(uintptr_t)63;
    s.plan = (NpPlan*)sp;
    sp += (sizeof(NpPlan) + 63) & ~(size_t)63;
    s.sorted = (float4*)sp;
    return s;
}

__global__ void k_np_plan(NpScratch s, double cell, int32_t* __restrict__ flag) {
    if (threadIdx.x != 0) return;
    NpPlan P;
    P.any = s.bkey[0] != 0xffffffffu;  // some point has three finite coordinates
    P.pad_ = 0;
    P.inv_cell = 1.0 / cell;
    int beyond = 0;
    for (int a = 0; a < 3; ++a) {
        P.lo[a] = P.any ? (double)gf_float_unkey(s.bkey[a]) : 0.0;
        P.ext[a] = P.any ? ((double)gf_float_unkey(s.bkey[4 + a]) - P.lo[a]) * P.inv_cell : 0.0;
        if (!(P.ext[a] < NP_MAX_CELLS)) beyond = 1;
    }
    *s.plan = P;
    *flag = beyond;
}

__device__ __forceinline__ unsigned np_bucket(int cx, int cy, int cz, unsigned tmask) {
    return (((unsigned)cx * 73856093u) ^ ((unsigned)cy * 19349663u) ^ ((unsigned)cz * 83492791u)) & tmask;
}
// the cell of a valid point: every coordinate in [0, ext] -- clamped below 2^30, so that a point beyond the proven range
// (the flag is then up and the wrapper raises) still lands in a bucket of the table
__device__ __forceinline__ int np_cell(float x, double lo, double inv_cell) {
    const double u = floor(((double)x - lo) * inv_cell);
    return (int)fmin(fmax(u, -2.0), NP_MAX_CELLS);
}

template <bool FILL>
__global__ __launch_bounds__(RS_THREADS) void k_np_bin(const float* __restrict__ xyz, int n, NpScratch s) {
    const int i = blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= n) return;
    const float x = xyz[(size_t)i * 3], y = xyz[(size_t)i * 3 + 1], z = xyz[(size_t)i * 3 + 2];
    if (!finite3(x, y, z)) return;  // never a candidate
    const NpPlan& P = *s.plan;
    const unsigned b = np_bucket(np_cell(x, P.lo[0], P.inv_cell), np_cell(y, P.lo[1], P.inv_cell),
                                 np_cell(z, P.lo[2], P.inv_cell), s.T - 1);
    if (FILL)
        s.sorted[atomicAdd(&s.cursor[b], 1)] = make_float4(x, y, z, __int_as_float(i));  // cursor < start[b + 1] <= n
    else
        atomicAdd(&s.counts[b], 1);
}

__global__ __launch_bounds__(RS_THREADS) void k_np_query(const float* __restrict__ query, int Q, float r2, NpScratch s,
                                                         int32_t* __restrict__ idx, float* __restrict__ d2_out) {
    const int q = blockIdx.x * RS_THREADS + threadIdx.x;
    if (q >= Q) return;
    const float qx = query[(size_t)q * 3], qy = query[(size_t)q * 3 + 1], qz = query[(size_t)q * 3 + 2];
    const NpPlan& P = *s.plan;
    u64 best = RS_EMPTY;
    bool walk = P.any && finite3(qx, qy, qz);
    int qc[3] = {0, 0, 0};
    if (walk) {
        const float qf[3] = {qx, qy, qz};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double u = floor(((double)qf[a] - P.lo[a]) * P.inv_cell);
            // a point within max_dist lies less than one cell away, and every point's cell is in [0, ext]
            if (!(u >= -1.0 && u <= floor(P.ext[a]) + 1.0)) walk = false;
            qc[a] = (int)fmin(fmax(u, -2.0), NP_MAX_CELLS);
        }
    }
    if (walk) {
        for (int c = 0; c < 27; ++c) {
            const unsigned b = np_bucket(qc[0] + c / 9 - 1, qc[1] + (c / 3) % 3 - 1, qc[2] + c % 3 - 1, s.T - 1);
            const int end = s.start[b + 1];
            for (int t = s.start[b]; t < end; ++t) {
                const float4 p = s.sorted[t];
                const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 <= r2) best = min(best, ((u64)__float_as_uint(d2) << 32) | (unsigned)__float_as_int(p.w));
            }
        }
    }
    idx[q] = best == RS_EMPTY ? -1 : (int)(unsigned)(best & 0xffffffffull);
    d2_out[q] = best == RS_EMPTY ? __builtin_inff() : __uint_as_float((unsigned)(best >> 32));
}

}  // namespace

extern "C" int gf_resample_max_points(void) { return RS_MAX_POINTS; }
extern "C" int gf_grid_subsample_max_cells(void) { return 1 << RS_AXIS_BITS; }
extern "C" double gf_nearest_point_max_cells(void) { return NP_MAX_CELLS; }

extern "C" size_t gf_grid_subsample_scratch_bytes(int N) {
    const size_t T = rs_table_size(N), n1 = (size_t)(N > 0 ? N : 0) + 1;
    return T * (8 + 8 + 4 + 4) + (2 * n1 + 2 * rs_nb(N) + 16) * 4 + 64;
}

extern "C" int gf_grid_subsample(const float* xyz, int N, float cell, int mode, const float* origin, void* scratch,
                                 int32_t* rep, int32_t* cell_of, int32_t* count, int32_t* d_words, void* stream) {
    GF_CHECK_ARG(N >= 0 && N <= RS_MAX_POINTS, "gf_grid_subsample: N = %d points (0 to %d)", N, RS_MAX_POINTS);
    GF_CHECK_ARG(cell > 0.0f && cell <= 3.402823466e38f, "gf_grid_subsample: cell = %g (positive and finite)", (double)cell);
    GF_CHECK_ARG(mode == 0 || mode == 1, "gf_grid_subsample: mode = %d (0 first, 1 center)", mode);
    if (N == 0) return GF_OK;
    GF_CHECK_ARG(xyz && scratch && rep && cell_of && count && d_words,
                 "gf_grid_subsample: NULL xyz, scratch, rep, cell_of, count or d_words");
    hipStream_t st = (hipStream_t)stream;
    RsScratch s = rs_carve(scratch, N);
    const int nb = gf_div_up(N, SCAN_THREADS), g = gf_div_up(N, RS_THREADS);
    GF_TRY(hipMemsetAsync(s.keys, 0xff, (size_t)s.T * 8, st));
    if (mode == 1) GF_TRY(hipMemsetAsync(s.best, 0xff, (size_t)s.T * 8, st));
    GF_TRY(hipMemsetAsync(s.first, 0x7f, (size_t)s.T * 4, st));
    GF_TRY(hipMemsetAsync(s.cnt, 0, (size_t)s.T * 4, st));
    GF_TRY(hipMemsetAsync(s.okey, 0xff, 4 * 4, st));
    GF_TRY(hipMemsetAsync(s.words, 0, 2 * 4, st));
    if (!origin)
        hipLaunchKernelGGL(k_rs_bounds, dim3(g < RS_BOUNDS_BLOCKS ? g : RS_BOUNDS_BLOCKS), dim3(RS_THREADS), 0, st, xyz, N, 0, s.okey,
                           (unsigned*)nullptr);
    hipLaunchKernelGGL(k_rs_org, dim3(1), dim3(64), 0, st, origin, s);
    hipLaunchKernelGGL(k_rs_insert, dim3(g), dim3(RS_THREADS), 0, st, xyz, N, cell, mode, s);
    hipLaunchKernelGGL(k_rs_sums, dim3(nb), dim3(SCAN_THREADS), 0, st, s, N);
    hipLaunchKernelGGL(k_rs_top, dim3(1), dim3(SCAN_THREADS), 0, st, s, nb);
    hipLaunchKernelGGL(k_rs_apply, dim3(nb), dim3(SCAN_THREADS), 0, st, s, N);
    hipLaunchKernelGGL(k_rs_write, dim3(g), dim3(RS_THREADS), 0, st, N, mode, s, rep, cell_of, count);
    GF_TRY(hipMemcpyAsync(d_words, s.words, 2 * 4, hipMemcpyDeviceToDevice, st));
    GF_CHECK_LAUNCH("gf_grid_subsample");
    return GF_OK;
}

extern "C" size_t gf_nearest_point_scratch_bytes(int n) {
    const size_t T = np_table_size(n), nb = (size_t)gf_iscan_blocks((int)T);
    return (3 * T + 1 + 2 * nb + 8) * 4 + 64 + ((sizeof(NpPlan) + 63) & ~(size_t)63) +
           ((size_t)(n > 0 ? n : 0) + 1) * sizeof(float4) + 64;
}

extern "C" int gf_nearest_point(const float* query, int Q, const float* xyz, int n, float max_dist, void* scratch,
                                int32_t* idx, float* d2, int32_t* d_flag, void* stream) {
    GF_CHECK_ARG(Q >= 0 && n >= 0 && n <= RS_MAX_POINTS, "gf_nearest_point: Q = %d queries, n = %d points (n 0 to %d)", Q, n,
                 RS_MAX_POINTS);
    GF_CHECK_ARG(max_dist > 0.0f && max_dist <= 3.402823466e38f, "gf_nearest_point: max_dist = %g (positive and finite)",
                 (double)max_dist);
    if (Q == 0) return GF_OK;
    GF_CHECK_ARG(query && scratch && idx && d2 && d_flag && (xyz || n == 0),
                 "gf_nearest_point: NULL query, xyz, scratch, idx, d2 or d_flag");
    hipStream_t st = (hipStream_t)stream;
    NpScratch s = np_carve(scratch, n);
    GF_TRY(hipMemsetAsync(s.counts, 0, (size_t)s.T * 4, st));
    GF_TRY(hipMemsetAsync(s.bkey, 0xff, 4 * 4, st));
    GF_TRY(hipMemsetAsync(s.bkey + 4, 0, 4 * 4, st));
    if (n > 0)
        hipLaunchKernelGGL(k_rs_bounds, dim3(min(gf_div_up(n, RS_THREADS), RS_BOUNDS_BLOCKS)), dim3(RS_THREADS), 0, st, xyz, n, 1,
                           s.bkey, s.bkey + 4);
    hipLaunchKernelGGL(k_np_plan, dim3(1), dim3(64), 0, st, s, (double)max_dist * 1.001, d_flag);
    if (n > 0) hipLaunchKernelGGL(k_np_bin<false>, dim3(gf_div_up(n, RS_THREADS)), dim3(RS_THREADS), 0, st, xyz, n, s);
    gf_iscan(s.counts, (int)s.T, s.start, s.cursor, s.block_sums, s.block_off, st);
    if (n > 0) hipLaunchKernelGGL(k_np_bin<true>, dim3(gf_div_up(n, RS_THREADS)), dim3(RS_THREADS), 0, st, xyz, n, s);
    hipLaunchKernelGGL(k_np_query, dim3(gf_div_up(Q, RS_THREADS)), dim3(RS_THREADS), 0, st, query, Q, max_dist * max_dist, s,
                       idx, d2);
    GF_CHECK_LAUNCH("gf_nearest_point");
    return GF_OK;
}
