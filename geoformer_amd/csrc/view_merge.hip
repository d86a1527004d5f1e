// Instances of a scan that was run under V views (rotations / mirrors of the same N points), joined across the views (the
// host statement is postprocess.merge_views_host; see include/geoformer_hip.h for the arguments).
//
// Every view holds all N points in the scan's own order, so the device needs no point tables: the views arrive as a
// scene table of one GfTileScene each (n_s = N, first_word unused).  Rows are the picked masks of all views, view-major.
//   k_vm_pack      one thread per (row, point): a wave's ballot over 64 consecutive points of the row is two words of the
//                  row's bitset bits[row, W] (coalesced reads of the dense int32 row); the wave's popcount is added once
//                  to cnt[row]
//   k_vm_overlaps  inter[a, b] = popcount(bits[a] & bits[b]) over the W words: a popcount "GEMM".  One workgroup of 256
//                  threads owns a 64 x 64 block of row pairs of the upper triangle of blocks; it stages 32 words of
//                  both row blocks in LDS (16-byte reads, rows padded to 36 words), every thread keeps a 4 x 4 block of
//                  sums in registers, and writes its cells and their mirror images -- every cell of inter is written.
//                  With few row blocks the words are split over workgroups too (whole stages each): the parts of a
//                  cell are then integer atomic adds to a cell the call has zeroed
//   k_vm_best      one wave per (row a, view v): the rows b of view v of a's class with inter[a, b] > 0 are dealt over the
//                  lanes; the largest IoU by the exact int64 cross-multiplied compare, the smaller row on ties, first
//                  inside a lane (ascending rows), then through a wave reduction
//   k_vm_merge     ONE workgroup of 1024 threads: mutual-best edges that pass the threshold hook a min-index union-find
//                  in LDS (post_steps.h, gf_uf_union); the views of a component are OR-ed per root in LDS; kept roots
//                  are ranked (global ids); the kept rows are sorted by (global id, row) with a bitonic sort in LDS --
//                  rows are view-major, so every instance's member rows come out sorted by view; one thread per
//                  instance then forms the score from that list: the largest member score of each view, added in view
//                  order, divided by V (no atomic touches a float)
//   k_vm_assemble  one thread per (instance, point): the member rows' bits of the point, OR-ed per view and the views
//                  counted; masks[g, p] is written directly, and the wave's popcount is added once to count[g]
//   k_vm_mean      one thread per output float: the V views' scores summed in view order and divided by V
// Integer atomics only (wave-aggregated sums, an OR of view bits, the union-find's CAS), and every value they form is a
// function of the inputs: all outputs are bit-identical from call to call.  A pick outside [0, n_rows) is an empty
// row, never an address.  Every row * N + point and row * W + word is formed in 64 bits.
#include "common.h"
#include "post_steps.h"

namespace {

constexpr int VM_MAX_ROWS = 4096;  // P: the LDS tables of k_vm_merge
constexpr int VM_MAX_VIEWS = 32;   // V: a component's views are one word
constexpr int VM_THREADS = 256;
constexpr int VM_MERGE_THREADS = 1024;
constexpr int VM_ROWS_PER_THREAD = VM_MAX_ROWS / VM_MERGE_THREADS;
constexpr int VM_TILE = 64;        // rows of a block of k_vm_overlaps
constexpr int VM_CHUNK = 32;       // words of a row staged at a time
constexpr int VM_STRIDE = VM_CHUNK + 4;  // LDS row stride in words: 16-byte aligned, rows 4 apart fall on other banks
constexpr int VM_FILL = 2048;       // workgroups k_vm_overlaps aims at: 8 per CU, two waves per SIMD
constexpr uint32_t VM_NO_KEY = 0xffffffffu;

typedef unsigned long long u64;

__global__ __launch_bounds__(VM_THREADS) void k_vm_pack(const long long* __restrict__ tab, int V, long long N, int W,
                                                        uint32_t* __restrict__ bits, int32_t* __restrict__ cnt) {
    const int a = blockIdx.y, lane = threadIdx.x & 63;
    const long long p = (long long)blockIdx.x * VM_THREADS + threadIdx.x;
    // the view of row a (uniform over the workgroup): V <= 32 rows of the table
    const int32_t* row = nullptr;
    for (int v = 0; v < V; ++v) {
        const GfTileScene* r = gf_row<GfTileScene>(tab, v);
        const long long k = a - r->first_row;
        if (k >= 0 && k < r->p_s) {
            const long long pk = ((const long long*)r->pick)[k];
            if ((u64)pk < (u64)r->n_rows) row = (const int32_t*)r->masks + pk * N;
        }
    }
    const bool on = row != nullptr && p < N && row[p] != 0;
    const u64 b = __ballot(on);
    const long long w0 = (p - lane) >> 5;  // the wave's first point is a multiple of 64
    if (w0 >= W) return;                   // (the whole wave)
    uint32_t* dst = bits + (long long)a * W;
    if (lane == 0) {
        dst[w0] = (uint32_t)b;
        if (b) atomicAdd(&cnt[a], __popcll(b));
    }
    if (lane == 32 && w0 + 1 < W) dst[w0 + 1] = (uint32_t)(b >> 32);
}

__global__ __launch_bounds__(VM_THREADS) void k_vm_overlaps(const uint32_t* __restrict__ bits, int P, int W, int nb,
                                                            int words_per_split, int32_t* __restrict__ inter) {
    __shared__ __attribute__((aligned(16))) uint32_t s_a[VM_TILE * VM_STRIDE];
    __shared__ __attribute__((aligned(16))) uint32_t s_b[VM_TILE * VM_STRIDE];
    // block (bi, bj), bi <= bj, of the upper triangle from the linear index (uniform)
    int bi = 0, left = blockIdx.x;
    while (left >= nb - bi) {
        left -= nb - bi;
        ++bi;
    }
    const int bj = bi + left;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    int acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0;
    const int lk = tid & (VM_CHUNK - 1), lr = tid >> 5;  // this thread's word and first row of a stage
    const int w_begin = blockIdx.y * words_per_split, w_end = min(W, w_begin + words_per_split);
    for (int w0 = w_begin; w0 < w_end; w0 += VM_CHUNK) {
        const int w = w0 + lk;
#pragma unroll
        for (int i = 0; i < VM_TILE / 8; ++i) {
            const int r = lr + 8 * i;
            const int ra = bi * VM_TILE + r, rb = bj * VM_TILE + r;
            s_a[r * VM_STRIDE + lk] = (ra < P && w < w_end) ? bits[(long long)ra * W + w] : 0u;
            s_b[r * VM_STRIDE + lk] = (rb < P && w < w_end) ? bits[(long long)rb * W + w] : 0u;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < VM_CHUNK; k += 4) {
            uint4 a4[4], b4[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                a4[i] = *(const uint4*)&s_a[(ty * 4 + i) * VM_STRIDE + k];
                b4[i] = *(const uint4*)&s_b[(tx * 4 + i) * VM_STRIDE + k];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[i][j] += __popc(a4[i].x & b4[j].x) + __popc(a4[i].y & b4[j].y) + __popc(a4[i].z & b4[j].z) +
                                 __popc(a4[i].w & b4[j].w);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int a = bi * VM_TILE + ty * 4 + i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int b = bj * VM_TILE + tx * 4 + j;
            if (a < P && b < P) {
                if (gridDim.y == 1) {  // the whole sum: stored
                    inter[(long long)a * P + b] = acc[i][j];
                    if (bi != bj) inter[(long long)b * P + a] = acc[i][j];
                } else if (acc[i][j] != 0) {  // a part of it: added to the zeroed cell
                    atomicAdd(&inter[(long long)a * P + b], acc[i][j]);
                    if (bi != bj) atomicAdd(&inter[(long long)b * P + a], acc[i][j]);
                }
            }
        }
    }
}

// is candidate (i2 / u2, row x2) a better partner than (i1 / u1, row x1)?  Exact: the IoUs cross-multiplied in int64
// (an intersection below 2^31 times a union below 2^32), the smaller row on ties; a row of -1 is no candidate.
__device__ __forceinline__ bool vm_better(int i1, long long u1, int x1, int i2, long long u2, int x2) {
    if (x2 < 0) return false;
    if (x1 < 0) return true;
    const long long l = (long long)i2 * u1, r = (long long)i1 * u2;
    return l > r || (l == r && x2 < x1);
}

__global__ __launch_bounds__(VM_THREADS) void k_vm_best(const int32_t* __restrict__ inter, const int32_t* __restrict__ cnt,
                                                        const long long* __restrict__ cls,
                                                        const int32_t* __restrict__ row_view,
                                                        const int32_t* __restrict__ view_first, int P, int V,
                                                        int32_t* __restrict__ best) {
    const int lane = threadIdx.x & 63;
    const long long job = (long long)blockIdx.x * (VM_THREADS / 64) + (threadIdx.x >> 6);  // (row, view) of this wave
    if (job >= (long long)P * V) return;
    const int a = (int)(job / V), v = (int)(job - (long long)a * V);
    int bi = 0, bx = -1;
    long long bu = 1;
    if (row_view[a] != v) {
        const long long ca = cls[a];
        const int na = cnt[a];
        const int lo = max(view_first[v], 0), hi = min(view_first[v + 1], P);
        for (int b = lo + lane; b < hi; b += 64) {
            const int in = inter[(long long)a * P + b];
            if (in > 0 && cls[b] == ca) {
                const long long un = (long long)na + cnt[b] - in;
                if (vm_better(bi, bu, bx, in, un, b)) bi = in, bu = un, bx = b;
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int oi = __shfl_xor(bi, d, 64), ox = __shfl_xor(bx, d, 64);
        const long long ou = __shfl_xor(bu, d, 64);
        if (vm_better(bi, bu, bx, oi, ou, ox)) bi = oi, bu = ou, bx = ox;
    }
    if (lane == 0) best[job] = bx;
}

__global__ __launch_bounds__(VM_MERGE_THREADS) void k_vm_merge(
    const int32_t* __restrict__ inter, const int32_t* __restrict__ cnt, const int32_t* __restrict__ best,
    const long long* __restrict__ cls, const float* __restrict__ scores, const int32_t* __restrict__ row_view, int P,
    int V, double iou, int min_views, int32_t* __restrict__ comp, int32_t* __restrict__ members,
    int32_t* __restrict__ d_G, long long* __restrict__ inst_cls, float* __restrict__ inst_scores,
    int32_t* __restrict__ inst_support, int32_t* __restrict__ inst_first, int32_t* __restrict__ inst_rows) {
    __shared__ int s_parent[VM_MAX_ROWS];
    __shared__ int s_gid[VM_MAX_ROWS];
    __shared__ uint32_t s_aux[VM_MAX_ROWS];  // the views of a root, then the sort's keys
    __shared__ int s_scan[VM_MERGE_THREADS];
    const int tid = threadIdx.x;
    for (int i = tid; i < P; i += VM_MERGE_THREADS) {
        s_parent[i] = i;
        s_aux[i] = 0u;
    }
    __syncthreads();
    // an edge a < b is seen from a: b = best[a, v], and a must be b's best in a's view
    for (int idx = tid; idx < P * V; idx += VM_MERGE_THREADS) {
        const int a = idx / V;
        const int b = best[idx];
        if (b <= a || b >= P) continue;
        const int va = row_view[a];
        if ((unsigned)va >= (unsigned)V || best[(long long)b * V + va] != a) continue;
        const int in = inter[(long long)a * P + b];
        const long long un = (long long)cnt[a] + cnt[b] - in;
        if (!((double)in >= iou * (double)un)) continue;
        gf_uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(s_parent, a, b);
    }
    __syncthreads();
    // flatten: nothing is hooked any more; the views of every component, one bit each, at its root
    for (int i = tid; i < P; i += VM_MERGE_THREADS) {
        const int root = gf_uf_root<__HIP_MEMORY_SCOPE_WORKGROUP>(s_parent, i);
        const int v = row_view[i];
        if ((unsigned)v < (unsigned)V) atomicOr(&s_aux[root], 1u << v);
    }
    __syncthreads();
    // global ids: the rank of every kept root among the kept roots; a thread owns VM_ROWS_PER_THREAD consecutive rows
    const int i0 = tid * VM_ROWS_PER_THREAD;
    bool keep[VM_ROWS_PER_THREAD];
    int mine = 0;
#pragma unroll
    for (int q = 0; q < VM_ROWS_PER_THREAD; ++q) {
        const int i = i0 + q;
        keep[q] = i < P && s_parent[i] == i && __popc(s_aux[i]) >= min_views && cnt[i] > 0;
        mine += keep[q] ? 1 : 0;
    }
    gf_lds_incl_scan<VM_MERGE_THREADS>(s_scan, tid, mine);
    const int G = s_scan[VM_MERGE_THREADS - 1];
    int next = s_scan[tid] - mine;
#pragma unroll
    for (int q = 0; q < VM_ROWS_PER_THREAD; ++q) {
        const int i = i0 + q;
        if (i >= P) continue;
        if (keep[q]) {
            s_gid[i] = next;
            inst_cls[next] = cls[i];
            inst_support[next] = __popc(s_aux[i]);
            ++next;
        } else {
            s_gid[i] = -1;
        }
    }
    if (tid == 0) d_G[0] = G;
    __syncthreads();  // (s_aux is read above and becomes the keys below)
    // the keys: (global id, row) of the kept rows; the rest, and the padding up to a power of two, sort to the end
    int n2 = 1;
    while (n2 < P) n2 <<= 1;
    int kept_here = 0;
    for (int i = tid; i < n2; i += VM_MERGE_THREADS) {
        uint32_t key = VM_NO_KEY;
        if (i < P) {
            const int root = s_parent[i], gid = s_gid[root];
            comp[i] = root;
            members[i] = gid;
            if (gid >= 0) {
                key = ((uint32_t)gid << 12) | (uint32_t)i;
                ++kept_here;
            }
        }
        s_aux[i] = key;
    }
    __syncthreads();
    gf_lds_incl_scan<VM_MERGE_THREADS>(s_scan, tid, kept_here);
    const int n_kept = s_scan[VM_MERGE_THREADS - 1];
    // bitonic sort of the n2 keys, ascending
    for (int size = 2; size <= n2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (n2 >> 1); t += VM_MERGE_THREADS) {
                const int lo = ((t / stride) * stride << 1) + (t % stride), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const uint32_t x = s_aux[lo], y = s_aux[hi];
                if ((x > y) == up) {
                    s_aux[lo] = y;
                    s_aux[hi] = x;
                }
            }
            __syncthreads();
        }
    }
    // the member list of every instance: rows ascending, hence views ascending; s_gid[g] becomes its first position
    __syncthreads();
    for (int k = tid; k < n_kept; k += VM_MERGE_THREADS) {
        const uint32_t key = s_aux[k];
        const int g = (int)(key >> 12);
        inst_rows[k] = (int)(key & 0xfffu);
        if (k == 0 || (int)(s_aux[k - 1] >> 12) != g) {
            s_gid[g] = k;
            inst_first[g] = k;
        }
    }
    if (tid == 0) inst_first[G] = n_kept;
    __syncthreads();
    // the score: the largest member score of every view (0 without a member), added in view order, over V
    for (int g = tid; g < G; g += VM_MERGE_THREADS) {
        int k = s_gid[g];
        float acc = 0.0f;
        for (int v = 0; v < V; ++v) {
            float m = 0.0f;
            bool any = false;
            while (k < n_kept && (int)(s_aux[k] >> 12) == g && row_view[s_aux[k] & 0xfffu] == v) {
                const float s = scores[s_aux[k] & 0xfffu];
                m = any ? fmaxf(m, s) : s;
                any = true;
                ++k;
            }
            acc = v == 0 ? m : acc + m;
        }
        inst_scores[g] = __fdiv_rn(acc, (float)V);
    }
}

__global__ __launch_bounds__(VM_THREADS) void k_vm_assemble(const uint32_t* __restrict__ bits,
                                                            const int32_t* __restrict__ inst_first,
                                                            const int32_t* __restrict__ inst_rows,
                                                            const int32_t* __restrict__ row_view,
                                                            const int32_t* __restrict__ inst_support, int P, long long N,
                                                            int W, double vote, int32_t* __restrict__ masks,
                                                            int32_t* __restrict__ count) {
    const int g = blockIdx.y, lane = threadIdx.x & 63;
    const long long p = (long long)blockIdx.x * VM_THREADS + threadIdx.x;
    const int k0 = inst_first[g], k1 = inst_first[g + 1];  // (uniform over the workgroup)
    const int w = (int)(min(p, N - 1) >> 5), bit = (int)(p & 31);
    int votes = 0, counted = -1;
    for (int k = k0; k < k1; ++k) {
        const int r = inst_rows[k];
        if ((unsigned)r >= (unsigned)P) continue;
        const int v = row_view[r];
        if (v != counted && ((bits[(long long)r * W + w] >> bit) & 1u)) {
            ++votes;
            counted = v;  // the members are sorted by view: a view counts once
        }
    }
    const bool in = p < N && votes > 0 && (double)votes >= vote * (double)inst_support[g];
    if (p < N) masks[(long long)g * N + p] = in ? 1 : 0;
    const u64 b = __ballot(in);
    if (lane == 0 && b) atomicAdd(&count[g], __popcll(b));
}

__global__ __launch_bounds__(VM_THREADS) void k_vm_mean(const long long* __restrict__ tab, int V, long long total,
                                                        float* __restrict__ out) {
    const long long k = (long long)blockIdx.x * VM_THREADS + threadIdx.x;
    if (k >= total) return;
    float acc = ((const float*)gf_row<GfTileScore>(tab, 0)->scores)[k];
    for (int v = 1; v < V; ++v) acc = acc + ((const float*)gf_row<GfTileScore>(tab, v)->scores)[k];
    out[k] = __fdiv_rn(acc, (float)V);
}

// The host copy of the view table, checked before anything is launched.  Returns NULL or what is wrong.
const char* vm_check_table(const long long* th, int V, int P, long long N) {
    long long row = 0;
    for (int v = 0; v < V; ++v) {
        const GfTileScene* r = gf_row<GfTileScene>(th, v);
        if (r->n_rows < 0 || r->p_s < 0) return "a negative n_rows or p_s";
        if (r->n_s != N) return "n_s is not N: every view holds all the points";
        if (r->p_s > 0 && N > 0 && (r->masks == 0 || r->pick == 0)) return "a NULL masks or pick pointer";
        if (r->first_row != row) return "first row does not follow the view before";
        row += r->p_s;
        if (row > VM_MAX_ROWS) return "more rows than gf_view_merge_max_rows()";
    }
    if (row != P) return "the picks of the views do not add up to P";
    return nullptr;
}

}  // namespace

extern "C" int gf_view_merge_max_rows(void) { return VM_MAX_ROWS; }
extern "C" int gf_view_merge_max_views(void) { return VM_MAX_VIEWS; }

#define VM_CHECK_SIZES(name)                                                                                           \
    GF_CHECK_ARG(P >= 0 && P <= VM_MAX_ROWS, "%s: P = %d rows (at most %d)", name, P, VM_MAX_ROWS);                    \
    GF_CHECK_ARG(V >= 1 && V <= VM_MAX_VIEWS, "%s: V = %d views (1 to %d)", name, V, VM_MAX_VIEWS)
#define VM_CHECK_POINTS(name) \
    GF_CHECK_ARG(N >= 0 && N < 0x7fffffffLL, "%s: N = %lld points (below 2^31)", name, N)

extern "C" int gf_view_pack(const long long* table, const long long* table_host, int V, int P, long long N,
                            uint32_t* bits, int32_t* cnt, void* stream) {
    VM_CHECK_SIZES("gf_view_pack");
    VM_CHECK_POINTS("gf_view_pack");
    GF_CHECK_ARG(table && table_host, "gf_view_pack: NULL table or table_host");
    const char* bad = vm_check_table(table_host, V, P, N);
    GF_CHECK_ARG(!bad, "gf_view_pack: view table: %s", bad);
    GF_CHECK_ARG(P == 0 || (cnt && (N == 0 || bits)), "gf_view_pack: NULL bits or cnt");
    if (P == 0) return GF_OK;
    hipStream_t st = (hipStream_t)stream;
    GF_TRY(hipMemsetAsync(cnt, 0, (size_t)P * sizeof(int32_t), st));
    if (N == 0) return GF_OK;
    hipLaunchKernelGGL(k_vm_pack, dim3(gf_div_up(N, VM_THREADS), P), dim3(VM_THREADS), 0, st, table, V, N,
                       (int)((N + 31) >> 5), bits, cnt);
    GF_CHECK_LAUNCH("gf_view_pack");
    return GF_OK;
}

extern "C" int gf_view_overlaps(const uint32_t* bits, int P, long long N, int32_t* inter, void* stream) {
    GF_CHECK_ARG(P >= 0 && P <= VM_MAX_ROWS, "gf_view_overlaps: P = %d rows (at most %d)", P, VM_MAX_ROWS);
    VM_CHECK_POINTS("gf_view_overlaps");
    GF_CHECK_ARG(P == 0 || (inter && (N == 0 || bits)), "gf_view_overlaps: NULL bits or inter");
    if (P == 0) return GF_OK;
    const int nb = gf_div_up(P, VM_TILE), blocks = nb * (nb + 1) / 2, W = (int)((N + 31) >> 5);
    // few blocks of row pairs leave most of the chip idle: the words are then split over workgroups as well, whole LDS
    // stages each, towards VM_FILL workgroups in all; the parts of a cell are added with integer atomics to a zeroed inter
    const int chunks = max(gf_div_up(W, VM_CHUNK), 1);
    const int per = gf_div_up(chunks, min(chunks, max(VM_FILL / blocks, 1))), splits = gf_div_up(chunks, per);
    hipStream_t st = (hipStream_t)stream;
    if (splits > 1) GF_TRY(hipMemsetAsync(inter, 0, (size_t)P * P * sizeof(int32_t), st));
    hipLaunchKernelGGL(k_vm_overlaps, dim3(blocks, splits), dim3(VM_THREADS), 0, st, bits, P, W, nb, per * VM_CHUNK, inter);
    GF_CHECK_LAUNCH("gf_view_overlaps");
    return GF_OK;
}

extern "C" int gf_view_best(const int32_t* inter, const int32_t* cnt, const long long* cls, const int32_t* row_view,
                            const int32_t* view_first, int P, int V, int32_t* best, void* stream) {
    VM_CHECK_SIZES("gf_view_best");
    GF_CHECK_ARG(P == 0 || (inter && cnt && cls && row_view && view_first && best),
                 "gf_view_best: NULL inter, cnt, cls, row_view, view_first or best");
    if (P == 0) return GF_OK;
    hipLaunchKernelGGL(k_vm_best, dim3(gf_div_up((long long)P * V, VM_THREADS / 64)), dim3(VM_THREADS), 0,
                       (hipStream_t)stream, inter, cnt, cls, row_view, view_first, P, V, best);
    GF_CHECK_LAUNCH("gf_view_best");
    return GF_OK;
}

extern "C" int gf_view_merge(const int32_t* inter, const int32_t* cnt, const int32_t* best, const long long* cls,
                             const float* scores, const int32_t* row_view, int P, int V, double iou, int min_views,
                             int32_t* comp, int32_t* members, int32_t* d_G, long long* inst_cls, float* inst_scores,
                             int32_t* inst_support, int32_t* inst_first, int32_t* inst_rows, void* stream) {
    VM_CHECK_SIZES("gf_view_merge");
    GF_CHECK_ARG(iou == iou, "gf_view_merge: iou is NaN");
    GF_CHECK_ARG(min_views >= 1 && min_views <= V, "gf_view_merge: min_views = %d (1 to V = %d)", min_views, V);
    GF_CHECK_ARG(d_G && inst_first, "gf_view_merge: NULL d_G or inst_first");
    GF_CHECK_ARG(P == 0 || (inter && cnt && best && cls && scores && row_view && comp && members && inst_cls &&
                            inst_scores && inst_support && inst_rows),
                 "gf_view_merge: NULL inter, cnt, best, cls, scores, row_view, comp, members, inst_cls, inst_scores, "
                 "inst_support or inst_rows");
    hipLaunchKernelGGL(k_vm_merge, dim3(1), dim3(VM_MERGE_THREADS), 0, (hipStream_t)stream, inter, cnt, best, cls, scores,
                       row_view, P, V, iou, min_views, comp, members, d_G, inst_cls, inst_scores, inst_support,
                       inst_first, inst_rows);
    GF_CHECK_LAUNCH("gf_view_merge");
    return GF_OK;
}

extern "C" int gf_view_assemble(const uint32_t* bits, const int32_t* inst_first, const int32_t* inst_rows,
                                const int32_t* row_view, const int32_t* inst_support, int P, int G, long long N,
                                double vote, int32_t* masks, int32_t* count, void* stream) {
    GF_CHECK_ARG(P >= 0 && P <= VM_MAX_ROWS && G >= 0 && G <= P, "gf_view_assemble: G = %d instances of P = %d rows (at most %d)",
                 G, P, VM_MAX_ROWS);
    VM_CHECK_POINTS("gf_view_assemble");
    GF_CHECK_ARG(vote > 0.0 && vote <= 1.0, "gf_view_assemble: vote = %g (in (0, 1])", vote);
    GF_CHECK_ARG(G == 0 || (count && inst_first && inst_rows && row_view && inst_support && (N == 0 || (masks && bits))),
                 "gf_view_assemble: NULL bits, inst_first, inst_rows, row_view, inst_support, masks or count");
    if (G == 0) return GF_OK;
    hipStream_t st = (hipStream_t)stream;
    GF_TRY(hipMemsetAsync(count, 0, (size_t)G * sizeof(int32_t), st));
    if (N == 0) return GF_OK;
    hipLaunchKernelGGL(k_vm_assemble, dim3(gf_div_up(N, VM_THREADS), G), dim3(VM_THREADS), 0, st, bits, inst_first,
                       inst_rows, row_view, inst_support, P, N, (int)((N + 31) >> 5), vote, masks, count);
    GF_CHECK_LAUNCH("gf_view_assemble");
    return GF_OK;
}

extern "C" int gf_view_mean_scores(const long long* table, const long long* table_host, int V, long long N, int C,
                                   float* out, void* stream) {
    const int cap = gf_tile_stitch_max_classes();
    GF_CHECK_ARG(V >= 1 && V <= VM_MAX_VIEWS, "gf_view_mean_scores: V = %d views (1 to %d)", V, VM_MAX_VIEWS);
    GF_CHECK_ARG(C >= 1 && C <= cap, "gf_view_mean_scores: C = %d classes (1 to %d)", C, cap);
    VM_CHECK_POINTS("gf_view_mean_scores");
    GF_CHECK_ARG(table && table_host, "gf_view_mean_scores: NULL table or table_host");
    for (int v = 0; v < V; ++v) {
        const GfTileScore* r = gf_row<GfTileScore>(table_host, v);
        GF_CHECK_ARG(r->n_s == N, "gf_view_mean_scores: view %d: n_s = %lld, N = %lld", v, r->n_s, N);
        GF_CHECK_ARG(N == 0 || r->scores != 0, "gf_view_mean_scores: view %d: NULL scores", v);
    }
    if (N == 0) return GF_OK;
    GF_CHECK_ARG(out, "gf_view_mean_scores: NULL out");
    const long long total = N * C;
    hipLaunchKernelGGL(k_vm_mean, dim3(gf_div_up(total, VM_THREADS)), dim3(VM_THREADS), 0, (hipStream_t)stream, table, V,
                       total, out);
    GF_CHECK_LAUNCH("gf_view_mean_scores");
    return GF_OK;
}
