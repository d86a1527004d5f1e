// DBSCAN of p picked instance masks over ONE radius graph (gf_knn_radius' row format): every mask restricts the graph to
// its own points and is split into spatially connected clusters (gf_mask_components); gf_mask_keep_largest then keeps
// the largest cluster of every picked row.  The host statement is postprocess.mask_components_host; see
// include/geoformer_hip.h for the arguments.
//
// The unit of work is one wave per (pick r, 64-point word w): the wave reads the pick's 8-byte member (or core) word
// and leaves when it is zero, so a mask that covers 2 % of a scene costs 2 % of the row walks.  Seven launches whatever
// N, p and k are, none of them repeated "until nothing changes":
//   k_ms_pack     one pass over the int32 rows pick[r]: the ballot-packed member bits [p, ceil(N / 64)]; zeroes the
//                 pick's table row and its largest-cluster key
//   k_ms_core     a member counts the entries of its own row whose bit is set in the pick's bit row (it stops at
//                 min_samples); the ballot of the core lanes is the pick's core word.  comp doubles as the parent
//                 array: i for a core point, -1 for every other point; count = 0 at core points.  members += popcount
//   k_ms_hook     a core lane walks its row and unions with every core entry: post_steps.h's lock-free min-index union
//                 (gf_uf_union)
//   k_ms_flatten  comp[i] = root(i) for core points, in place (gf_uf_root); count[root] += the number of the wave's
//                 lanes with that root: ONE integer atomicAdd per distinct root of the wave (gf_wave_add_per_key)
//   k_ms_border   a member that is not core takes the smallest root among the core entries of its own row (final since
//                 k_ms_flatten): reads core words of comp, writes non-core words; count[root] += 1, aggregated as above
//   k_ms_dissolve comp = -1 where count[comp] < min_points; a kept root adds itself to the pick's table (clusters,
//                 points) and offers (size << 32) | (0x7fffffff - id) to the pick's 64-bit atomicMax, both reduced over
//                 the wave first
//   k_ms_table    one thread per pick unpacks the key into {largest id, its size}
// Integer atomics only, and every value they form is a function of the inputs (sums, a maximum, the min-index root of a
// finished set), so comp and tab are bit-identical from call to call, and a pick's rows do not depend on the other
// picks: nothing of one pick is read by another.  An index outside [0, N) in a row is skipped, never followed, and only
// columns 0 .. min(deg[i], k - 1) of a row are read.  Every r * N + i is formed in 64 bits.
#include "common.h"
#include "post_steps.h"

namespace {

constexpr int MS_THREADS = 256;            // four waves: four 64-point words of one pick
constexpr int MS_WAVES = MS_THREADS / 64;
constexpr int MS_PACK_WORDS = 8;           // words per wave of k_ms_pack: 2048 points per workgroup
constexpr int MS_TAB = GF_MSP_TABLE_INTS;
static_assert(sizeof(GfMspRow) == 4 * GF_MSP_TABLE_INTS, "the row of include/geoformer_hip.h");

typedef unsigned long long u64;

__device__ __forceinline__ bool ms_bit(const u64* __restrict__ row, int j) { return (row[j >> 6] >> (j & 63)) & 1ull; }

// the wave's word of this workgroup; -1 behind the last
__device__ __forceinline__ long long ms_word(long long W) {
    const long long w = (long long)blockIdx.x * MS_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    return w < W ? w : -1;
}

__global__ __launch_bounds__(MS_THREADS) void k_ms_pack(const int32_t* __restrict__ masks, int n_rows, long long N,
                                                        const long long* __restrict__ pick, long long W,
                                                        u64* __restrict__ bits, int32_t* __restrict__ tab,
                                                        u64* __restrict__ best) {
    const long long r = blockIdx.y;
    const long long row = pick[r];
    const bool valid = row >= 0 && row < n_rows;  // (a pick outside the masks is an empty row, never an address)
    const int32_t* m = masks + (valid ? row : 0) * N;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long w0 = ((long long)blockIdx.x * MS_WAVES + wave) * MS_PACK_WORDS;
    if (blockIdx.x == 0) {
        if (threadIdx.x < MS_TAB) tab[r * MS_TAB + threadIdx.x] = 0;
        if (threadIdx.x == 64) best[r] = 0ull;
    }
    // the loads of the wave's words first, all in flight together: a point past the end reads the row's last one
    int v[MS_PACK_WORDS];
#pragma unroll
    for (int q = 0; q < MS_PACK_WORDS; q++) v[q] = 0;
    if (valid) {  // (uniform over the workgroup)
#pragma unroll
        for (int q = 0; q < MS_PACK_WORDS; q++) {
            const long long pt = (w0 + q) * 64 + lane;
            v[q] = m[pt < N ? pt : N - 1];
        }
    }
#pragma unroll
    for (int q = 0; q < MS_PACK_WORDS; q++) {
        const u64 bb = __ballot(v[q] != 0 && (w0 + q) * 64 + lane < N);
        if (lane == 0 && w0 + q < W) bits[r * W + w0 + q] = bb;
    }
}

__global__ __launch_bounds__(MS_THREADS) void k_ms_core(const int32_t* __restrict__ I, const int32_t* __restrict__ deg,
                                                        long long N, int k, int min_samples, long long W,
                                                        const u64* __restrict__ bits, u64* __restrict__ core,
                                                        int32_t* __restrict__ comp, int32_t* __restrict__ count,
                                                        int32_t* tab) {
    const long long r = blockIdx.y, w = ms_word(W);
    if (w < 0) return;
    const int lane = threadIdx.x & 63;
    const u64* brow = bits + r * W;
    const u64 word = brow[w];
    const long long i = w * 64 + lane;
    bool is_core = false;
    if (word) {  // (wave-uniform)
        if ((word >> lane) & 1ull) {
            int need = min_samples - 1;  // entries still missing
            const int last = min(deg[i], k - 1);
            const int32_t* row = I + i * k;
            for (int c = 0; c <= last && need > 0; ++c) {
                const int j = row[c];
                if ((unsigned long long)(long long)j < (unsigned long long)N && j != i && ms_bit(brow, j)) --need;
            }
            is_core = need <= 0;
        }
        if (lane == 0) atomicAdd(&((GfMspRow*)(tab + r * MS_TAB))->members, __popcll(word));  // (32-bit row index)
    }
    const u64 cw = __ballot(is_core);
    if (lane == 0) core[r * W + w] = cw;
    if (i < N) {
        comp[r * N + i] = is_core ? (int)i : -1;
        if (is_core) count[r * N + i] = 0;
    }
}

__global__ __launch_bounds__(MS_THREADS) void k_ms_hook(const int32_t* __restrict__ I, const int32_t* __restrict__ deg,
                                                        long long N, int k, long long W, const u64* __restrict__ core,
                                                        int32_t* comp) {
    const long long r = blockIdx.y, w = ms_word(W);
    if (w < 0) return;
    const int lane = threadIdx.x & 63;
    const u64* crow = core + r * W;
    if (!((crow[w] >> lane) & 1ull)) return;
    const long long i = w * 64 + lane;
    int32_t* parent = comp + r * N;  // core points only: every word followed below is a core point's
    const int last = min(deg[i], k - 1);
    const int32_t* row = I + i * k;
    for (int c = 0; c <= last; ++c) {
        const int j = row[c];
        if ((unsigned long long)(long long)j >= (unsigned long long)N || j == i || !ms_bit(crow, j)) continue;
        gf_uf_union<__HIP_MEMORY_SCOPE_AGENT>(parent, (int)i, j);
    }
}

__global__ __launch_bounds__(MS_THREADS) void k_ms_flatten(long long N, long long W, const u64* __restrict__ core,
                                                           int32_t* comp, int32_t* count) {
    const long long r = blockIdx.y, w = ms_word(W);
    if (w < 0) return;
    const int lane = threadIdx.x & 63;
    const u64 cw = core[r * W + w];
    if (!cw) return;  // (wave-uniform)
    const bool on = (cw >> lane) & 1ull;
    int32_t* parent = comp + r * N;
    int root = -1;
    if (on) root = gf_uf_root<__HIP_MEMORY_SCOPE_AGENT>(parent, (int)(w * 64 + lane));  // nothing is hooked any more
    gf_wave_add_per_key(lane, on, root, count + r * N);
}

__global__ __launch_bounds__(MS_THREADS) void k_ms_border(const int32_t* __restrict__ I, const int32_t* __restrict__ deg,
                                                          long long N, int k, long long W, const u64* __restrict__ bits,
                                                          const u64* __restrict__ core, int32_t* comp, int32_t* count) {
    const long long r = blockIdx.y, w = ms_word(W);
    if (w < 0) return;
    const int lane = threadIdx.x & 63;
    const u64* crow = core + r * W;
    const u64 bw = bits[r * W + w] & ~crow[w];  // members that are not core
    if (!bw) return;  // (wave-uniform)
    int32_t* ids = comp + r * N;
    int best = 0x7fffffff;
    if ((bw >> lane) & 1ull) {
        const long long i = w * 64 + lane;
        const int last = min(deg[i], k - 1);
        const int32_t* row = I + i * k;
        for (int c = 0; c <= last; ++c) {
            const int j = row[c];
            if ((unsigned long long)(long long)j >= (unsigned long long)N || !ms_bit(crow, j)) continue;
            best = min(best, ids[j]);  // a core point's word: its root, final since k_ms_flatten
        }
        if (best != 0x7fffffff) ids[i] = best;
    }
    gf_wave_add_per_key(lane, best != 0x7fffffff, best, count + r * N);
}

__global__ __launch_bounds__(MS_THREADS) void k_ms_dissolve(long long N, int min_points, long long W,
                                                            const u64* __restrict__ bits, const u64* __restrict__ core,
                                                            int32_t* __restrict__ comp, const int32_t* __restrict__ count,
                                                            int32_t* tab, u64* best) {
    const long long r = blockIdx.y, w = ms_word(W);
    if (w < 0) return;
    const int lane = threadIdx.x & 63;
    const u64 bw = bits[r * W + w];
    if (!bw) return;  // (wave-uniform)
    const u64 cw = core[r * W + w];
    int roots = 0, points = 0;
    u64 key = 0ull;
    if ((bw >> lane) & 1ull) {
        const long long i = w * 64 + lane;
        const int id = comp[r * N + i];  // this lane's own word: nobody else writes it here
        if (id >= 0) {
            const int size = count[r * N + id];
            if (size < min_points) {
                comp[r * N + i] = -1;
            } else if (id == i && ((cw >> lane) & 1ull)) {  // a kept cluster's root speaks for the cluster
                roots = 1;
                points = size;
                key = ((u64)(unsigned)size << 32) | (u64)(unsigned)(0x7fffffff - id);
            }
        }
    }
    if (!__ballot(roots != 0)) return;
    roots = gf_wave_sum_i(roots);
    points = gf_wave_sum_i(points);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const u64 o = (u64)__shfl_xor((long long)key, d, 64);
        key = o > key ? o : key;
    }
    if (lane == 0) {
        atomicAdd(&((GfMspRow*)tab)[r].clusters, roots);
        atomicAdd(&((GfMspRow*)tab)[r].kept_points, points);
        atomicMax(&best[r], key);
    }
}

__global__ __launch_bounds__(MS_THREADS) void k_ms_table(int p, const u64* __restrict__ best, int32_t* __restrict__ tab) {
    const int r = blockIdx.x * MS_THREADS + threadIdx.x;
    if (r >= p) return;
    const u64 key = best[r];  // 0: no kept cluster (a cluster has at least one point)
    ((GfMspRow*)tab)[r].largest = key ? 0x7fffffff - (int)(key & 0xffffffffull) : -1;
    ((GfMspRow*)tab)[r].largest_size = (int)(key >> 32);
}

// one workgroup per (row of masks, chunk of 1024 points): the first rank that picks the row decides it (every rank that
// picks a row has the same comp and tab rows); a row nobody picks is copied
__global__ __launch_bounds__(MS_THREADS) void k_ms_keep_largest(const int32_t* __restrict__ masks, long long N,
                                                                const long long* __restrict__ pick, int p,
                                                                const int32_t* __restrict__ comp,
                                                                const int32_t* __restrict__ tab, long long nchunk,
                                                                int32_t* __restrict__ out) {
    __shared__ int s_rank;
    const long long row = blockIdx.x / nchunk, c = blockIdx.x % nchunk;
    if (threadIdx.x == 0) s_rank = 0x7fffffff;
    __syncthreads();
    for (int r = threadIdx.x; r < p; r += MS_THREADS)
        if (pick[r] == row) atomicMin(&s_rank, r);  // (LDS)
    __syncthreads();
    const int r = s_rank;
    const int keep = r < p ? ((const GfMspRow*)tab)[r].largest : -1;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const long long i = c * (4 * MS_THREADS) + q * MS_THREADS + threadIdx.x;
        if (i >= N) break;
        const int v = masks[row * N + i];
        out[row * N + i] = r >= p ? v : (keep >= 0 && comp[(long long)r * N + i] == keep ? v : 0);
    }
}

size_t ms_words(long long N) { return (size_t)((N > 0 ? N : 0) + 63) / 64; }
size_t ms_align(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

// scratch: the member and the core bit rows, the pick's largest-cluster keys, then the per-root counts int32 [p, N]
extern "C" size_t gf_mask_components_scratch_bytes(int N, int p) {
    if (N <= 0 || p <= 0) return 0;
    const size_t rows = ms_align((size_t)p * ms_words(N) * sizeof(u64));
    return 2 * rows + ms_align((size_t)p * sizeof(u64)) + ms_align((size_t)p * (size_t)N * sizeof(int32_t));
}

extern "C" int gf_mask_components(const int32_t* masks, int n_rows, int N, const long long* pick, int p, const int32_t* I,
                                  const int32_t* deg, int k, int min_samples, int min_points, int32_t* comp, int32_t* tab,
                                  void* scratch, void* stream) {
    GF_CHECK_ARG(N >= 0 && p >= 0 && p <= GF_NMS_MAX_N && k >= 1, "gf_mask_components: N = %d points, p = %d picks (at most %d), k = %d columns",
                 N, p, GF_NMS_MAX_N, k);
    GF_CHECK_ARG(min_samples >= 1 && min_points >= 1, "gf_mask_components: min_samples = %d, min_points = %d (at least 1)",
                 min_samples, min_points);
    GF_CHECK_ARG(N == 0 || p == 0 || (masks && pick && I && deg && comp && tab && scratch),
                 "gf_mask_components: NULL masks, pick, I, deg, comp, tab or scratch");
    GF_CHECK_ARG(((uintptr_t)scratch & 7) == 0, "gf_mask_components: scratch must be 8-byte aligned");
    if (N == 0 || p == 0) return GF_OK;
    hipStream_t st = (hipStream_t)stream;
    const long long W = (long long)ms_words(N);
    const size_t rows = ms_align((size_t)p * W * sizeof(u64));
    u64* bits = (u64*)scratch;
    u64* core = (u64*)((char*)scratch + rows);
    u64* best = (u64*)((char*)scratch + 2 * rows);
    int32_t* count = (int32_t*)((char*)scratch + 2 * rows + ms_align((size_t)p * sizeof(u64)));
    const dim3 blk(MS_THREADS), words(gf_div_up(W, MS_WAVES), p);
    hipLaunchKernelGGL(k_ms_pack, dim3(gf_div_up(W, MS_WAVES * MS_PACK_WORDS), p), blk, 0, st, masks, n_rows, (long long)N,
                       pick, W, bits, tab, best);
    hipLaunchKernelGGL(k_ms_core, words, blk, 0, st, I, deg, (long long)N, k, min_samples, W, bits, core, comp, count, tab);
    hipLaunchKernelGGL(k_ms_hook, words, blk, 0, st, I, deg, (long long)N, k, W, core, comp);
    hipLaunchKernelGGL(k_ms_flatten, words, blk, 0, st, (long long)N, W, core, comp, count);
    hipLaunchKernelGGL(k_ms_border, words, blk, 0, st, I, deg, (long long)N, k, W, bits, core, comp, count);
    hipLaunchKernelGGL(k_ms_dissolve, words, blk, 0, st, (long long)N, min_points, W, bits, core, comp, count, tab, best);
    hipLaunchKernelGGL(k_ms_table, dim3(gf_div_up(p, MS_THREADS)), blk, 0, st, p, best, tab);
    GF_CHECK_LAUNCH("gf_mask_components");
    return GF_OK;
}

extern "C" int gf_mask_keep_largest(const int32_t* masks, int n_rows, int N, const long long* pick, int p,
                                    const int32_t* comp, const int32_t* tab, int32_t* masks_out, void* stream) {
    GF_CHECK_ARG(n_rows >= 0 && N >= 0 && p >= 0 && p <= GF_NMS_MAX_N, "gf_mask_keep_largest: n_rows = %d, N = %d points, p = %d picks (at most %d)",
                 n_rows, N, p, GF_NMS_MAX_N);
    GF_CHECK_ARG(n_rows == 0 || N == 0 || (masks && masks_out), "gf_mask_keep_largest: NULL masks or masks_out");
    GF_CHECK_ARG(n_rows == 0 || N == 0 || p == 0 || (pick && comp && tab), "gf_mask_keep_largest: NULL pick, comp or tab");
    const long long nchunk = ((long long)N + 4 * MS_THREADS - 1) / (4 * MS_THREADS);
    GF_CHECK_ARG(nchunk * n_rows <= 0x7fffffffLL, "gf_mask_keep_largest: n_rows * N = %lld", (long long)n_rows * N);
    if (n_rows == 0 || N == 0 || p == 0) return GF_OK;  // (p == 0: nothing to clean, masks_out is not written)
    hipLaunchKernelGGL(k_ms_keep_largest, dim3((unsigned)(nchunk * n_rows)), dim3(MS_THREADS), 0, (hipStream_t)stream, masks,
                       (long long)N, pick, p, comp, tab, nchunk, masks_out);
    GF_CHECK_LAUNCH("gf_mask_keep_largest");
    return GF_OK;
}
