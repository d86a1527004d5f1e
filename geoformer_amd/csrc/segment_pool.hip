// Pooling of mask logits over a scene's over-segments (superpoints) for the S kept scenes of an eval forward:
//     out[q, p] = mean of in[q, p'] over the foreground points p' of the scene that carry p's segment id
// on logits stored [nq, N_b] row-major per scene, where a segment's members are scattered columns of a row.
//
// The caller hands in the batch's foreground points sorted (stably) by one int64 key per point -- (scene, id), or a key
// of the point's own where it has no segment -- as keys_sorted and order (sorted position -> foreground row).  A run of
// equal neighbouring keys is one segment; a scene's runs lie in its own positions fg_off .. fg_off + N_b of the order.
//
// Eight commands on the caller's stream, no host synchronisation, whatever S, nq and the runs are:
//   k_sp_heads     flag of every position that begins a run (its key differs from the one before)
//   gf_iscan       (three launches) exclusive scan of the flags -> the dense index of every position's run
//   k_sp_runs      run index per position, first position per run (one plain store per run, by its first member)
//   k_sp_pool      the only read of the logits.  A workgroup owns SP_CHUNK consecutive positions OF ONE SCENE (counted
//                  from the scene's first, so a scene is cut the same way alone and inside a batch) and SP_QT queries:
//                  one gathered load per (position, query), a segmented sum over the lanes of each wave (shuffles,
//                  fixed tree), the waves' partial sums of a run added in wave order through LDS.  A run that lies
//                  inside the chunk gets its mean here, every member the same word, written to the columns just read.
//                  A run that leaves the chunk leaves its partial sum in the chunk's head / tail slot.
//   k_sp_combine   one workgroup per chunk; the chunk in which a cut run BEGINS adds the slots of the chunks the run
//                  crosses in chunk order -> the run's sum, once per (query, run)
//   k_sp_open      the members of cut runs: that sum / length, the same word for every member.  Write only; a workgroup
//                  whose chunk begins and ends on run boundaries leaves at once.
// A long run is therefore split over as many workgroups as it has chunks: the launch is as long as a chunk, not as the
// longest run.  No floating-point atomics: every sum has one fixed order that depends only on the positions inside the
// scene.  Nothing in the table, the keys or the order can make an address leave its buffer: a scene whose row does not
// fit [0, n_fg) is skipped, a column outside [0, N_b) is neither read nor written, runs are clipped to their scene.
#include <algorithm>

#include "common.h"

namespace {

constexpr int SP_THREADS = 1024;         // one position per thread
constexpr int SP_CHUNK = SP_THREADS;     // positions per workgroup
constexpr int SP_WAVES = SP_THREADS / 64;
constexpr int SP_QT = 16;                // queries per workgroup
constexpr int SP_IDX_THREADS = 256;

struct SpScene {
    const float* in;
    float* out;
    long long N, off;  // foreground points, first position
    bool ok;
};

__device__ __forceinline__ SpScene sp_scene(const long long* __restrict__ table, int s, long long n_fg) {
    const GfSegScene* row = gf_row<GfSegScene>(table, s);
    SpScene sc;
    sc.in = (const float*)row->in;
    sc.out = (float*)row->out;
    sc.N = row->N;
    sc.off = row->off;
    sc.ok = sc.in != nullptr && sc.out != nullptr && (const float*)sc.out != sc.in && sc.N > 0 && sc.off >= 0 &&
            sc.off <= n_fg && sc.N <= n_fg - sc.off;
    return sc;
}

// first slot of scene s in the head / tail tables: at least the chunks of every scene before it
__device__ __forceinline__ long long sp_slot_base(const SpScene& sc, int s) { return sc.off / SP_CHUNK + s; }

// run [rs, re) of position j, clipped to the scene's positions [lo_s, hi_s)
__device__ __forceinline__ void sp_run_of(const int32_t* __restrict__ rid, const int32_t* __restrict__ run_start,
                                          long long j, long long lo_s, long long hi_s, long long* rs, long long* re) {
    const int r = rid[j];
    *rs = max((long long)run_start[r], lo_s);
    *re = min((long long)run_start[r + 1], hi_s);
}

__global__ __launch_bounds__(SP_IDX_THREADS) void k_sp_heads(const long long* __restrict__ keys, int n,
                                                             int32_t* __restrict__ flag) {
    const int j = blockIdx.x * SP_IDX_THREADS + threadIdx.x;
    if (j < n) flag[j] = (j == 0 || keys[j] != keys[j - 1]) ? 1 : 0;
}

__global__ __launch_bounds__(SP_IDX_THREADS) void k_sp_runs(const int32_t* __restrict__ flag,
                                                            const int32_t* __restrict__ start, int n,
                                                            int32_t* __restrict__ rid, int32_t* __restrict__ run_start) {
    const int j = blockIdx.x * SP_IDX_THREADS + threadIdx.x;
    if (j >= n) return;
    const int f = flag[j];
    const int r = start[j] + f - 1;  // flag[0] = 1: r >= 0
    rid[j] = r;
    if (f) run_start[r] = j;
    if (j == n - 1) run_start[r + 1] = n;
}

__global__ __launch_bounds__(SP_THREADS) void k_sp_pool(const long long* __restrict__ table, int nq, long long n_fg,
                                                        const int32_t* __restrict__ order,
                                                        const int32_t* __restrict__ rid,
                                                        const int32_t* __restrict__ run_start,
                                                        float* __restrict__ head_g, float* __restrict__ tail_g) {
    __shared__ float sh_head[SP_WAVES][SP_QT];  // per wave: the sum of the run of its first / last position, inside the wave
    __shared__ float sh_tail[SP_WAVES][SP_QT];
    const int s = blockIdx.y;
    const SpScene sc = sp_scene(table, s, n_fg);
    const long long c0 = (long long)blockIdx.x * SP_CHUNK;
    if (!sc.ok || c0 >= sc.N) return;  // (uniform)
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int q0 = blockIdx.z * SP_QT;
    const long long lo = sc.off + c0, hi = sc.off + min(sc.N, c0 + SP_CHUNK);  // the chunk's positions
    const long long j = lo + t;
    const bool live = j < hi;
    long long rs = j, re = j + 1, col = -1;
    if (live) {
        sp_run_of(rid, run_start, j, sc.off, sc.off + sc.N, &rs, &re);
        rs = min(rs, j);
        re = max(re, j + 1);
        col = (long long)order[j] - sc.off;
        if (col < 0 || col >= sc.N) col = -1;
    }
    float v[SP_QT];
#pragma unroll
    for (int q = 0; q < SP_QT; ++q)
        v[q] = (col >= 0 && q0 + q < nq) ? sc.in[(size_t)(q0 + q) * sc.N + col] : 0.0f;
    // segmented inclusive sum over the wave: lane l takes lane l - d while that lane is still inside l's run
    const long long wlo = lo + (long long)w * 64;
    const int first = (int)(max(rs, wlo) - wlo);                 // first and last lane of the run inside the wave
    const int last = live ? (int)(min(min(re, hi), wlo + 64) - 1 - wlo) : lane;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const bool take = lane - d >= first;
#pragma unroll
        for (int q = 0; q < SP_QT; ++q) {
            const float o = __shfl_up(v[q], d, 64);
            if (take) v[q] += o;
        }
    }
    float p[SP_QT];  // the run's sum inside this wave, the same word in every member lane
#pragma unroll
    for (int q = 0; q < SP_QT; ++q) p[q] = __shfl(v[q], last, 64);
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < SP_QT; ++q) sh_head[w][q] = p[q];
    }
    if (lane == 63) {
#pragma unroll
        for (int q = 0; q < SP_QT; ++q) sh_tail[w][q] = p[q];
    }
    __syncthreads();
    if (!live) return;
    // the run inside the chunk: the waves it crosses, in wave order
    const int wa = (int)((max(rs, lo) - lo) >> 6), wb = (int)((min(re, hi) - 1 - lo) >> 6);
    if (wa != wb) {
#pragma unroll
        for (int q = 0; q < SP_QT; ++q) p[q] = sh_tail[wa][q];
        for (int x = wa + 1; x <= wb; ++x) {
#pragma unroll
            for (int q = 0; q < SP_QT; ++q) p[q] += sh_head[x][q];
        }
    }
    if (rs >= lo && re <= hi) {  // the whole run is here: its mean, to the columns just read
        if (col < 0) return;
        const float len = (float)(re - rs);
#pragma unroll
        for (int q = 0; q < SP_QT; ++q)
            if (q0 + q < nq) sc.out[(size_t)(q0 + q) * sc.N + col] = p[q] / len;
        return;
    }
    const size_t slot = (size_t)(sp_slot_base(sc, s) + blockIdx.x) * nq;
    if (j == lo && rs < lo) {
#pragma unroll
        for (int q = 0; q < SP_QT; ++q)
            if (q0 + q < nq) head_g[slot + q0 + q] = p[q];
    }
    if (j == hi - 1 && re > hi) {
#pragma unroll
        for (int q = 0; q < SP_QT; ++q)
            if (q0 + q < nq) tail_g[slot + q0 + q] = p[q];
    }
}

__global__ __launch_bounds__(SP_IDX_THREADS) void k_sp_combine(const long long* __restrict__ table, int nq,
                                                               long long n_fg, const int32_t* __restrict__ rid,
                                                               const int32_t* __restrict__ run_start,
                                                               const float* __restrict__ head_g,
                                                               float* __restrict__ tail_g) {
    const int s = blockIdx.y;
    const SpScene sc = sp_scene(table, s, n_fg);
    const long long c0 = (long long)blockIdx.x * SP_CHUNK;
    if (!sc.ok || c0 >= sc.N) return;
    const long long lo = sc.off + c0, hi = sc.off + min(sc.N, c0 + SP_CHUNK);
    long long rs, re;
    sp_run_of(rid, run_start, hi - 1, sc.off, sc.off + sc.N, &rs, &re);
    if (re <= hi || rs < lo) return;  // the run of the last position ends here, or began in an earlier chunk (uniform)
    const int more = (int)((re - 1 - sc.off) / SP_CHUNK - blockIdx.x);  // chunks the run goes on into
    const size_t slot = (size_t)(sp_slot_base(sc, s) + blockIdx.x) * nq;
    for (int q = threadIdx.x; q < nq; q += SP_IDX_THREADS) {
        float acc = tail_g[slot + q];
#pragma unroll 8
        for (int c = 1; c <= more; ++c) acc += head_g[slot + (size_t)c * nq + q];
        tail_g[slot + q] = acc;
    }
}

__global__ __launch_bounds__(SP_THREADS) void k_sp_open(const long long* __restrict__ table, int nq, long long n_fg,
                                                        const int32_t* __restrict__ order,
                                                        const int32_t* __restrict__ rid,
                                                        const int32_t* __restrict__ run_start,
                                                        const float* __restrict__ total_g) {
    const int s = blockIdx.y;
    const SpScene sc = sp_scene(table, s, n_fg);
    const long long c0 = (long long)blockIdx.x * SP_CHUNK;
    if (!sc.ok || c0 >= sc.N) return;
    const long long lo = sc.off + c0, hi = sc.off + min(sc.N, c0 + SP_CHUNK);
    long long rs, re, rs1, re1;
    sp_run_of(rid, run_start, lo, sc.off, sc.off + sc.N, &rs, &re);
    sp_run_of(rid, run_start, hi - 1, sc.off, sc.off + sc.N, &rs1, &re1);
    if (rs >= lo && re1 <= hi) return;  // no run is cut at either end of the chunk (uniform)
    const long long j = lo + threadIdx.x;
    if (j >= hi) return;
    sp_run_of(rid, run_start, j, sc.off, sc.off + sc.N, &rs, &re);
    rs = min(rs, j);
    re = max(re, j + 1);
    if (rs >= lo && re <= hi) return;
    const long long col = (long long)order[j] - sc.off;
    if (col < 0 || col >= sc.N) return;
    const int q0 = blockIdx.z * SP_QT;
    const size_t slot = (size_t)(sp_slot_base(sc, s) + (rs - sc.off) / SP_CHUNK) * nq;  // the chunk the run begins in
    const float len = (float)(re - rs);
#pragma unroll
    for (int q = 0; q < SP_QT; ++q)
        if (q0 + q < nq) sc.out[(size_t)(q0 + q) * sc.N + col] = total_g[slot + q0 + q] / len;
}

size_t sp_align(size_t b) { return (b + 255) & ~(size_t)255; }

struct SpScratch {
    size_t flag, start, rid, run_start, block_sums, block_off, head, tail, total;
};

SpScratch sp_layout(int S, long long n_fg, int nq) {
    const size_t n = n_fg > 0 ? (size_t)n_fg : 0, s = S > 0 ? S : 0, q = nq > 0 ? nq : 0;
    const size_t nb = (size_t)gf_iscan_blocks((int)std::min<size_t>(n, 0x7fffffff));
    const size_t slots = n / SP_CHUNK + s + 1;
    SpScratch L;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += sp_align(bytes);
        return here;
    };
    L.flag = take(n * sizeof(int32_t));
    L.start = take((n + 1) * sizeof(int32_t));
    L.rid = take(n * sizeof(int32_t));
    L.run_start = take((n + 1) * sizeof(int32_t));
    L.block_sums = take(nb * sizeof(int32_t));
    L.block_off = take(nb * sizeof(int32_t));
    L.head = take(slots * q * sizeof(float));
    L.tail = take(slots * q * sizeof(float));
    L.total = at;
    return L;
}

}  // namespace

extern "C" int gf_segment_pool_scene_fields(void) { return sizeof(GfSegScene) / sizeof(long long); }

extern "C" int gf_segment_pool_chunk_points(void) { return SP_CHUNK; }

extern "C" size_t gf_segment_pool_scratch_bytes(int S, long long n_fg, int nq) { return sp_layout(S, n_fg, nq).total; }

extern "C" int gf_segment_pool_batched(const long long* table, const long long* table_host, int S, int nq,
                                       const long long* keys_sorted, const int32_t* order, long long n_fg,
                                       long long max_N, void* scratch, void* stream) {
    GF_CHECK_ARG(nq >= 1, "gf_segment_pool_batched: nq = %d queries (at least 1)", nq);
    GF_CHECK_ARG(S >= 0 && n_fg >= 0 && max_N >= 0 && n_fg <= 0x7ffffff0LL && max_N <= n_fg,
                 "gf_segment_pool_batched: S = %d scenes, n_fg = %lld foreground points, max_N = %lld", S, n_fg, max_N);
    GF_CHECK_ARG(n_fg == 0 || S == 0 || (table && keys_sorted && order && scratch),
                 "gf_segment_pool_batched: NULL table, keys, order or scratch");
    if (table_host) {
        long long at = 0;
        for (int s = 0; s < S; ++s) {
            const GfSegScene* row = gf_row<GfSegScene>(table_host, s);
            GF_CHECK_ARG(row->N >= 0 && row->N <= max_N && row->off == at,
                         "gf_segment_pool_batched: scene %d has N_b = %lld (max_N = %lld) at fg_off = %lld, expected %lld", s,
                         row->N, max_N, row->off, at);
            GF_CHECK_ARG(row->N == 0 || (row->in != 0 && row->out != 0), "gf_segment_pool_batched: scene %d: NULL logits", s);
            GF_CHECK_ARG(row->N == 0 || row->in != row->out,
                         "gf_segment_pool_batched: scene %d: out == in (the pooling is out of place)", s);
            at += row->N;
        }
        GF_CHECK_ARG(at == n_fg, "gf_segment_pool_batched: the scenes hold %lld foreground points, n_fg = %lld", at, n_fg);
    }
    if (S == 0 || n_fg == 0 || max_N == 0) return GF_OK;
    GF_CHECK_ARG(S <= 65535 && gf_div_up(nq, SP_QT) <= 65535, "gf_segment_pool_batched: S = %d, nq = %d (grid limits)", S, nq);
    hipStream_t st = (hipStream_t)stream;
    const SpScratch L = sp_layout(S, n_fg, nq);
    char* base = (char*)scratch;
    int32_t* flag = (int32_t*)(base + L.flag);
    int32_t* start = (int32_t*)(base + L.start);
    int32_t* rid = (int32_t*)(base + L.rid);
    int32_t* run_start = (int32_t*)(base + L.run_start);
    float* head_g = (float*)(base + L.head);
    float* tail_g = (float*)(base + L.tail);
    const int n = (int)n_fg;
    const dim3 idx_grid((unsigned)gf_div_up(n, SP_IDX_THREADS));
    hipLaunchKernelGGL(k_sp_heads, idx_grid, dim3(SP_IDX_THREADS), 0, st, keys_sorted, n, flag);
    gf_iscan(flag, n, start, rid, (int32_t*)(base + L.block_sums), (int32_t*)(base + L.block_off), st);
    hipLaunchKernelGGL(k_sp_runs, idx_grid, dim3(SP_IDX_THREADS), 0, st, flag, start, n, rid, run_start);
    const unsigned chunks = (unsigned)gf_div_up(max_N, SP_CHUNK), qt = (unsigned)gf_div_up(nq, SP_QT);
    hipLaunchKernelGGL(k_sp_pool, dim3(chunks, S, qt), dim3(SP_THREADS), 0, st, table, nq, n_fg, order, rid, run_start,
                       head_g, tail_g);
    hipLaunchKernelGGL(k_sp_combine, dim3(chunks, S), dim3(SP_IDX_THREADS), 0, st, table, nq, n_fg, rid, run_start,
                       head_g, tail_g);
    hipLaunchKernelGGL(k_sp_open, dim3(chunks, S, qt), dim3(SP_THREADS), 0, st, table, nq, n_fg, order, rid, run_start,
                       tail_g);
    GF_CHECK_LAUNCH("gf_segment_pool_batched");
    return GF_OK;
}
