// Instances of a scan that was run as T overlapping tiles, joined across the tiles (the host statement is
// postprocess.merge_tiles_host; the tile plan is scene.tile_plan; see include/geoformer_hip.h for the arguments).
//
// The device never sees a coordinate: the plan arrives as two integer tables over the scan's N points, tile_of and
// local_of int32 [N, 4] (the point's tiles in ascending order, -1 padded, and its index inside each), and the tiles as a
// scene table of one GfTileScene each.  Rows are the picked masks of all tiles, tile-major.
//   k_tm_pack      one thread per (tile-local point, 32-pick word): the point's memberships in the tile's picks as a
//                  bitset of ceil(p_s / 32) consecutive words, gathered from the dense int32 rows (coalesced over the
//                  points of a row)
//   k_tm_overlaps  one thread per point of the scan: one 16-byte read of its tile_of row, and a wave none of whose
//                  points lies in two tiles leaves.  For every pair (s, t) of a point's tiles the lanes of the wave that
//                  carry the SAME (s, t, bitset in s, bitset in t) form a group: the group's size is added once to
//                  shared[a, t], shared[b, s], inter[a, b] and inter[b, a] for the set bits a, b, with the pairs (a, b)
//                  dealt over the 64 lanes -- a wall of 10 000 shared points reaches a counter as 160 adds, not 10 000
//   k_tm_merge     ONE workgroup of 1024 threads: the edges of the upper triangle of inter hook a min-index union-find in
//                  LDS (post_steps.h's lock-free union at workgroup scope, gf_uf_union); then comp, the ranks of the
//                  roots (global ids), the class of the root and the maximum member score by an integer-ordered
//                  atomicMax in LDS (gf_float_key)
//   k_tm_assemble  one thread per point of the scan: for every tile of the point and every set bit, atomicOr on the
//                  instance's output word; the lanes whose word was 0 before count, one atomicAdd per distinct instance
//                  of the wave
// Integer atomics only, and every value they form is a sum, a maximum or the min-index root of a finished set: all
// outputs are bit-identical from call to call.  A tile id outside [0, T), a local index outside [0, n_s), a pick outside
// [0, n_rows) or a row outside [0, P) is skipped, never an address.  Every row * N + point is formed in 64 bits.
#include "common.h"
#include "post_steps.h"

namespace {

constexpr int TM_MAX_ROWS = 4096;  // P: the LDS tables of k_tm_merge
constexpr int TM_MAX_PICKS = 256;  // p_s: a point's bitset is at most 8 words
constexpr int TM_WORDS = TM_MAX_PICKS / 32;
static_assert(sizeof(GfTileScene) == 8 * GF_TILE_SCENE_FIELDS, "the row of include/geoformer_hip.h");
constexpr int TM_THREADS = 256;
constexpr int TM_MERGE_THREADS = 1024;
constexpr int TM_ROWS_PER_THREAD = TM_MAX_ROWS / TM_MERGE_THREADS;

typedef unsigned long long u64;

__global__ __launch_bounds__(TM_THREADS) void k_tm_pack(const long long* __restrict__ tab, uint32_t* __restrict__ bits) {
    const GfTileScene* row = gf_row<GfTileScene>(tab, blockIdx.y);
    const long long n_rows = row->n_rows, n_s = row->n_s, p_s = row->p_s;
    const int w = blockIdx.z, wpp = (int)((p_s + 31) >> 5);
    const long long j = (long long)blockIdx.x * TM_THREADS + threadIdx.x;
    if (w >= wpp || j >= n_s) return;
    const int32_t* masks = (const int32_t*)row->masks;
    const long long* pick = (const long long*)row->pick;
    const int k0 = w * 32, kn = (int)min((long long)32, p_s - k0);
    uint32_t word = 0;
    for (int k = 0; k < kn; ++k) {
        const long long r = pick[k0 + k];  // (uniform over the workgroup)
        if ((u64)r < (u64)n_rows && masks[r * n_s + j] != 0) word |= 1u << k;
    }
    bits[row->first_word + j * wpp + w] = word;
}

// One pair (s, t) of the tiles of this lane's point: see the head of the file.  Wave-uniform control flow.
__device__ __forceinline__ void tm_pair(const long long* __restrict__ tab, int T, bool on, int s, int t, int la, int lb,
                                        const uint32_t* __restrict__ bits, int P, int32_t* inter, int32_t* shared) {
    const int lane = threadIdx.x & 63;
    bool act = on && s >= 0 && t > s && t < T;
    if (!__ballot(act)) return;
    uint32_t A[TM_WORDS], B[TM_WORDS];
#pragma unroll
    for (int w = 0; w < TM_WORDS; ++w) A[w] = B[w] = 0;
    int frs = 0, frt = 0;
    if (act) {
        const GfTileScene *rs = gf_row<GfTileScene>(tab, s), *rt = gf_row<GfTileScene>(tab, t);
        const long long ps = rs->p_s, pt = rt->p_s;
        act = (u64)la < (u64)rs->n_s && (u64)lb < (u64)rt->n_s && ps <= TM_MAX_PICKS && pt <= TM_MAX_PICKS;
        if (act) {
            frs = (int)rs->first_row;
            frt = (int)rt->first_row;
            const int wa = (int)((ps + 31) >> 5), wb = (int)((pt + 31) >> 5);
            const uint32_t* pa = bits + rs->first_word + (long long)la * wa;
            const uint32_t* pb = bits + rt->first_word + (long long)lb * wb;
            uint32_t any = 0;
#pragma unroll
            for (int w = 0; w < TM_WORDS; ++w) {
                if (w < wa) A[w] = pa[w];
                if (w < wb) B[w] = pb[w];
                any |= A[w] | B[w];
            }
            act = any != 0;  // a point in no picked mask counts nowhere
        }
    }
    u64 todo = __ballot(act);
    while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const int s0 = __shfl(s, lead, 64), t0 = __shfl(t, lead, 64);
        const int frs0 = __shfl(frs, lead, 64), frt0 = __shfl(frt, lead, 64);
        bool m = ((todo >> lane) & 1ull) && s == s0 && t == t0;
        uint32_t a0[TM_WORDS], b0[TM_WORDS];
#pragma unroll
        for (int w = 0; w < TM_WORDS; ++w) {
            a0[w] = (uint32_t)__shfl((int)A[w], lead, 64);
            b0[w] = (uint32_t)__shfl((int)B[w], lead, 64);
            m = m && A[w] == a0[w] && B[w] == b0[w];
        }
        const u64 same = __ballot(m);  // (the leader is among them)
        const int cnt = __popcll(same);
        // the leader's bits dealt over the lanes: bit r of asel / bsel = pick r * 64 + lane of tile s0 / t0
        int bsel = 0;
#pragma unroll
        for (int r = 0; r < TM_WORDS / 2; ++r) {
            const uint32_t wa = lane < 32 ? a0[2 * r] : a0[2 * r + 1];
            const uint32_t wb = lane < 32 ? b0[2 * r] : b0[2 * r + 1];
            const int ra = frs0 + r * 64 + lane, rb = frt0 + r * 64 + lane;
            if (((wa >> (lane & 31)) & 1u) && ra < P) atomicAdd(&shared[(long long)ra * T + t0], cnt);
            if (((wb >> (lane & 31)) & 1u) && rb < P) {
                atomicAdd(&shared[(long long)rb * T + s0], cnt);
                bsel |= 1 << r;
            }
        }
#pragma unroll
        for (int w = 0; w < TM_WORDS; ++w) {
            uint32_t xa = (uint32_t)__builtin_amdgcn_readfirstlane((int)a0[w]);
            while (xa) {
                const int ra = frs0 + w * 32 + __ffs((int)xa) - 1;
                xa &= xa - 1;
                if (ra >= P) continue;
#pragma unroll
                for (int r = 0; r < TM_WORDS / 2; ++r) {
                    if ((bsel >> r) & 1) {
                        const int rb = frt0 + r * 64 + lane;
                        atomicAdd(&inter[(long long)ra * P + rb], cnt);
                        atomicAdd(&inter[(long long)rb * P + ra], cnt);
                    }
                }
            }
        }
        todo &= ~same;
    }
}

__global__ __launch_bounds__(TM_THREADS) void k_tm_overlaps(const long long* __restrict__ tab, int T,
                                                            const int4* __restrict__ tile_of,
                                                            const int4* __restrict__ local_of, long long N,
                                                            const uint32_t* __restrict__ bits, int P, int32_t* inter,
                                                            int32_t* shared) {
    const long long g = (long long)blockIdx.x * TM_THREADS + threadIdx.x;
    int4 tl = make_int4(-1, -1, -1, -1);
    if (g < N) tl = tile_of[g];
    const bool multi = tl.y >= 0;  // ascending and -1 padded: a second tile stands in the second column
    if (!__ballot(multi)) return;  // (the whole wave: the majority of the waves)
    const int4 lc = multi ? local_of[g] : make_int4(0, 0, 0, 0);
    tm_pair(tab, T, multi, tl.x, tl.y, lc.x, lc.y, bits, P, inter, shared);
    tm_pair(tab, T, multi, tl.x, tl.z, lc.x, lc.z, bits, P, inter, shared);
    tm_pair(tab, T, multi, tl.x, tl.w, lc.x, lc.w, bits, P, inter, shared);
    tm_pair(tab, T, multi, tl.y, tl.z, lc.y, lc.z, bits, P, inter, shared);
    tm_pair(tab, T, multi, tl.y, tl.w, lc.y, lc.w, bits, P, inter, shared);
    tm_pair(tab, T, multi, tl.z, tl.w, lc.z, lc.w, bits, P, inter, shared);
}

__global__ __launch_bounds__(TM_MERGE_THREADS) void k_tm_merge(const int32_t* __restrict__ inter,
                                                               const int32_t* __restrict__ shared,
                                                               const long long* __restrict__ cls,
                                                               const float* __restrict__ scores,
                                                               const int32_t* __restrict__ row_tile, int P, int T,
                                                               double iom, int min_shared, int32_t* __restrict__ comp,
                                                               int32_t* __restrict__ members, int32_t* __restrict__ d_G,
                                                               long long* __restrict__ inst_cls,
                                                               float* __restrict__ inst_scores) {
    __shared__ int s_parent[TM_MAX_ROWS];
    __shared__ int s_gid[TM_MAX_ROWS];
    __shared__ uint32_t s_key[TM_MAX_ROWS];
    __shared__ int s_scan[TM_MERGE_THREADS];
    const int tid = threadIdx.x;
    for (int i = tid; i < P; i += TM_MERGE_THREADS) {
        s_parent[i] = i;
        s_key[i] = 0u;
    }
    __syncthreads();
    // the upper triangle, row by row of inter (coalesced); an edge hooks the two roots
    for (int idx = tid; idx < P * P; idx += TM_MERGE_THREADS) {
        const int a = idx / P, b = idx - a * P;
        if (b <= a) continue;
        const int v = inter[idx];
        if (v < min_shared) continue;
        const int ta = row_tile[a], tb = row_tile[b];
        if (ta == tb || (unsigned)ta >= (unsigned)T || (unsigned)tb >= (unsigned)T || cls[a] != cls[b]) continue;
        const int small = min(shared[(long long)a * T + tb], shared[(long long)b * T + ta]);
        if (!((double)v >= iom * (double)small)) continue;
        gf_uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(s_parent, a, b);
    }
    __syncthreads();
    // flatten: nothing is hooked any more; the key of a score keeps its order (no NaN among the scores)
    for (int i = tid; i < P; i += TM_MERGE_THREADS) {
        const int root = gf_uf_root<__HIP_MEMORY_SCOPE_WORKGROUP>(s_parent, i);
        atomicMax(&s_key[root], gf_float_key(scores[i]));
    }
    __syncthreads();
    // global ids: the rank of every root among the roots; a thread owns TM_ROWS_PER_THREAD consecutive rows
    const int i0 = tid * TM_ROWS_PER_THREAD;
    int mine = 0;
#pragma unroll
    for (int q = 0; q < TM_ROWS_PER_THREAD; ++q) mine += (i0 + q < P && s_parent[i0 + q] == i0 + q) ? 1 : 0;
    // post_steps.h's gf_lds_incl_scan (written out: the call adds one scalar instruction to the scan's first step)
    s_scan[tid] = mine;
    __syncthreads();
    for (int d = 1; d < TM_MERGE_THREADS; d <<= 1) {
        const int v = tid >= d ? s_scan[tid - d] : 0;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
    }
    int next = s_scan[tid] - mine;
#pragma unroll
    for (int q = 0; q < TM_ROWS_PER_THREAD; ++q) {
        const int i = i0 + q;
        if (i < P && s_parent[i] == i) {
            s_gid[i] = next;
            inst_cls[next] = cls[i];
            inst_scores[next] = gf_float_unkey(s_key[i]);
            ++next;
        }
    }
    if (tid == TM_MERGE_THREADS - 1) d_G[0] = s_scan[tid];
    __syncthreads();
    for (int i = tid; i < P; i += TM_MERGE_THREADS) {
        const int root = s_parent[i];
        comp[i] = root;
        members[i] = s_gid[root];
    }
}

__global__ __launch_bounds__(TM_THREADS) void k_tm_assemble(const long long* __restrict__ tab, int T,
                                                            const int4* __restrict__ tile_of,
                                                            const int4* __restrict__ local_of, long long N,
                                                            const uint32_t* __restrict__ bits,
                                                            const int32_t* __restrict__ members, int P, int G,
                                                            int32_t* masks, int32_t* count) {
    const long long g = (long long)blockIdx.x * TM_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int tl[4] = {-1, -1, -1, -1}, lc[4] = {0, 0, 0, 0};
    if (g < N) {
        const int4 a = tile_of[g], b = local_of[g];
        tl[0] = a.x, tl[1] = a.y, tl[2] = a.z, tl[3] = a.w;
        lc[0] = b.x, lc[1] = b.y, lc[2] = b.z, lc[3] = b.w;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int s = tl[c];
        bool act = s >= 0 && s < T;
        if (!__ballot(act)) continue;
        int wpp = 0, fr = 0;
        const uint32_t* pb = bits;
        if (act) {
            const GfTileScene* row = gf_row<GfTileScene>(tab, s);
            act = (u64)lc[c] < (u64)row->n_s && row->p_s <= TM_MAX_PICKS;
            if (act) {
                wpp = (int)((row->p_s + 31) >> 5);
                fr = (int)row->first_row;
                pb = bits + row->first_word + (long long)lc[c] * wpp;
            }
        }
        // the lanes walk their set bits together, one bit per round: a round is over when no lane has a bit left
        int w = 0;
        uint32_t x = 0;
        for (;;) {
            while (x == 0 && w < wpp) x = pb[w++];
            const bool has = x != 0;
            if (!__ballot(has)) break;
            int gid = -1;
            bool fresh = false;
            if (has) {
                const int r = fr + (w - 1) * 32 + __ffs((int)x) - 1;
                x &= x - 1;
                if (r < P) gid = members[r];
                if (gid >= 0 && gid < G) fresh = atomicOr(&masks[(long long)gid * N + g], 1) == 0;
            }
            // count[gid] += the lanes with a fresh word of that instance: one atomicAdd per distinct instance
            // (written out: gf_wave_add_per_key gives the same instructions here, but a few of them in another order)
            u64 todo = __ballot(fresh);
            while (todo) {
                const int lead = __ffsll((long long)todo) - 1;
                const int g0 = __shfl(gid, lead, 64);
                const u64 same = __ballot(fresh && gid == g0);
                if (lane == lead) atomicAdd(&count[g0], __popcll(same));
                todo &= ~same;
            }
        }
    }
}

// The host copy of the scene table, checked before anything is launched: the sizes, and that the rows and the bitset
// words of the tiles follow each other.  Returns NULL or what is wrong.
const char* tm_check_table(const long long* th, int T, int P, long long* max_n, int* max_words, long long* words) {
    long long row = 0, word = 0;
    *max_n = 0;
    *max_words = 0;
    for (int s = 0; s < T; ++s) {
        const GfTileScene* r = gf_row<GfTileScene>(th, s);
        if (r->n_rows < 0 || r->n_s < 0 || r->n_s > 0x7fffffffLL || r->p_s < 0) return "a negative n_rows, n_s or p_s";
        if (r->p_s > TM_MAX_PICKS) return "more than 256 picks in a tile";
        if (r->p_s > 0 && r->n_s > 0 && (r->masks == 0 || r->pick == 0)) return "a NULL masks or pick pointer";
        if (r->first_row != row || r->first_word != word) return "first row / first word do not follow the tile before";
        const long long wpp = (r->p_s + 31) >> 5;
        row += r->p_s;
        word += r->n_s * wpp;
        if (wpp > 0 && r->n_s > *max_n) *max_n = r->n_s;
        if (r->n_s > 0 && wpp > *max_words) *max_words = (int)wpp;
    }
    if (row != P) return "the picks of the tiles do not add up to P";
    *words = word;
    return nullptr;
}

}  // namespace

extern "C" int gf_tile_merge_max_rows(void) { return TM_MAX_ROWS; }
extern "C" int gf_tile_merge_max_picks(void) { return TM_MAX_PICKS; }

#define TM_CHECK_TABLE(name)                                                                                          \
    GF_CHECK_ARG(T >= 0 && T <= 65535 && P >= 0, "%s: T = %d tiles (at most 65535), P = %d rows", name, T, P);        \
    GF_CHECK_ARG(P <= TM_MAX_ROWS, "%s: P = %d rows (at most %d)", name, P, TM_MAX_ROWS);                             \
    GF_CHECK_ARG(T == 0 || (table && table_host), "%s: NULL table or table_host", name);                              \
    long long max_n = 0, words = 0;                                                                                   \
    int max_words = 0;                                                                                                \
    {                                                                                                                 \
        const char* bad = tm_check_table(table_host, T, P, &max_n, &max_words, &words);                               \
        GF_CHECK_ARG(!bad, "%s: scene table: %s", name, bad);                                                         \
    }

extern "C" int gf_tile_pack_picks(const long long* table, const long long* table_host, int T, int P, uint32_t* bits,
                                  void* stream) {
    TM_CHECK_TABLE("gf_tile_pack_picks");
    GF_CHECK_ARG(words == 0 || bits, "gf_tile_pack_picks: NULL bits");
    if (words == 0) return GF_OK;
    hipLaunchKernelGGL(k_tm_pack, dim3(gf_div_up(max_n, TM_THREADS), T, max_words), dim3(TM_THREADS), 0,
                       (hipStream_t)stream, table, bits);
    GF_CHECK_LAUNCH("gf_tile_pack_picks");
    return GF_OK;
}

extern "C" int gf_tile_overlaps(const long long* table, const long long* table_host, int T, const int32_t* tile_of,
                                const int32_t* local_of, long long N, const uint32_t* bits, int P, int32_t* inter,
                                int32_t* shared, void* stream) {
    TM_CHECK_TABLE("gf_tile_overlaps");
    GF_CHECK_ARG(N >= 0 && N <= 0x7fffffffLL * TM_THREADS, "gf_tile_overlaps: N = %lld points", N);
    GF_CHECK_ARG(P == 0 || T == 0 || (inter && shared), "gf_tile_overlaps: NULL inter or shared");
    GF_CHECK_ARG(N == 0 || words == 0 || (tile_of && local_of && bits), "gf_tile_overlaps: NULL tile_of, local_of or bits");
    GF_CHECK_ARG((((uintptr_t)tile_of | (uintptr_t)local_of) & 15) == 0,
                 "gf_tile_overlaps: tile_of and local_of must be 16-byte aligned");
    if (P == 0 || T == 0) return GF_OK;
    hipStream_t st = (hipStream_t)stream;
    GF_TRY(hipMemsetAsync(inter, 0, (size_t)P * P * sizeof(int32_t), st));
    GF_TRY(hipMemsetAsync(shared, 0, (size_t)P * T * sizeof(int32_t), st));
    if (N == 0 || words == 0) return GF_OK;
    hipLaunchKernelGGL(k_tm_overlaps, dim3(gf_div_up(N, TM_THREADS)), dim3(TM_THREADS), 0, st, table, T,
                       (const int4*)tile_of, (const int4*)local_of, N, bits, P, inter, shared);
    GF_CHECK_LAUNCH("gf_tile_overlaps");
    return GF_OK;
}

extern "C" int gf_tile_merge(const int32_t* inter, const int32_t* shared, const long long* cls, const float* scores,
                             const int32_t* row_tile, int P, int T, double iom, int min_shared, int32_t* comp,
                             int32_t* members, int32_t* d_G, long long* inst_cls, float* inst_scores, void* stream) {
    GF_CHECK_ARG(P >= 0 && P <= TM_MAX_ROWS && T >= 0, "gf_tile_merge: P = %d rows (at most %d), T = %d tiles", P,
                 TM_MAX_ROWS, T);
    GF_CHECK_ARG(iom == iom, "gf_tile_merge: iom is NaN");
    GF_CHECK_ARG(d_G, "gf_tile_merge: NULL d_G");
    GF_CHECK_ARG(P == 0 || (inter && shared && cls && scores && row_tile && comp && members && inst_cls && inst_scores),
                 "gf_tile_merge: NULL inter, shared, cls, scores, row_tile, comp, members, inst_cls or inst_scores");
    hipLaunchKernelGGL(k_tm_merge, dim3(1), dim3(TM_MERGE_THREADS), 0, (hipStream_t)stream, inter, shared, cls, scores,
                       row_tile, P, T, iom, min_shared, comp, members, d_G, inst_cls, inst_scores);
    GF_CHECK_LAUNCH("gf_tile_merge");
    return GF_OK;
}

extern "C" int gf_tile_assemble(const long long* table, const long long* table_host, int T, const int32_t* tile_of,
                                const int32_t* local_of, long long N, const uint32_t* bits, const int32_t* members, int P,
                                int G, int32_t* masks, int32_t* count, void* stream) {
    TM_CHECK_TABLE("gf_tile_assemble");
    GF_CHECK_ARG(N >= 0 && N <= 0x7fffffffLL * TM_THREADS && G >= 0 && G <= P,
                 "gf_tile_assemble: N = %lld points, G = %d instances of P = %d rows", N, G, P);
    GF_CHECK_ARG(G == 0 || (count && (N == 0 || masks)), "gf_tile_assemble: NULL masks or count");
    GF_CHECK_ARG(G == 0 || N == 0 || words == 0 || (tile_of && local_of && bits && members),
                 "gf_tile_assemble: NULL tile_of, local_of, bits or members");
    GF_CHECK_ARG((((uintptr_t)tile_of | (uintptr_t)local_of) & 15) == 0,
                 "gf_tile_assemble: tile_of and local_of must be 16-byte aligned");
    if (G == 0) return GF_OK;
    hipStream_t st = (hipStream_t)stream;
    GF_TRY(hipMemsetAsync(count, 0, (size_t)G * sizeof(int32_t), st));
    if (N == 0) return GF_OK;
    GF_TRY(hipMemsetAsync(masks, 0, (size_t)G * (size_t)N * sizeof(int32_t), st));
    if (words == 0) return GF_OK;
    hipLaunchKernelGGL(k_tm_assemble, dim3(gf_div_up(N, TM_THREADS)), dim3(TM_THREADS), 0, st, table, T,
                       (const int4*)tile_of, (const int4*)local_of, N, bits, members, P, G, masks, count);
    GF_CHECK_LAUNCH("gf_tile_assemble");
    return GF_OK;
}
