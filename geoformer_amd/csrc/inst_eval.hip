// Per-scene overlap tables of the ScanNet instance evaluation (util/eval.py:290-355 assign_instances_for_scan with
// util/utils_3d.py:18-73 get_instances): for every picked mask, its intersection with every ground-truth instance of
// the evaluated class set and with the void points, and every instance's point count -- the [n_pick, N] passes the
// reference makes on the host (one np.count_nonzero(gt_ids == id & mask) per prediction x same-label instance).
//
// Four commands on the caller's stream, no host synchronisation:
//   memset   presence table, K = C * 1000 words (direct address: class rank * 1000 + id mod 1000)
//   k_ie_keys       one pass over the N gt ids: each point's key (-1 void, -2 padding up to a whole 1024-point chunk),
//                   the presence mark of its key; zero-fills the outputs (capacity, G is not known yet)
//   k_ie_slots      one workgroup: exclusive scan of the presence table -> compact slot per key in ascending id order
//                   (np.unique's order), G, the id of every slot (post_steps.h's gf_presence_to_slots)
//   k_ie_hist       grid (point chunks of 1024, groups of IE_ROWS rows): each thread keeps 4 points' slots and
//                   IE_ROWS x 4 mask bits in registers, a workgroup counts them in an LDS histogram [IE_ROWS, tile] and
//                   flushes one integer atomic per nonzero (row, slot); slots beyond one LDS tile are handled by
//                   further passes over the same registers (the masks are read once).  Row n is a virtual all-ones
//                   row: its counts are the instances' point counts.
#include "common.h"
#include "post_steps.h"

namespace {

constexpr int IE_THREADS = 256;
constexpr int IE_PER_THREAD = 4;                          // consecutive points per thread (one dwordx4)
constexpr int IE_CHUNK = IE_THREADS * IE_PER_THREAD;      // points per workgroup
constexpr int IE_ROWS = 8;                                // mask rows per workgroup
constexpr int IE_TILE = 1024;                             // LDS slots per row and pass (IE_ROWS * IE_TILE * 4 = 32 KB)
constexpr int IE_MAX_CLASSES = 64;
constexpr int IE_SCAN_THREADS = 1024;

__device__ __forceinline__ int ie_class_rank(long long cls, const int32_t* __restrict__ class_ids, int C) {
    // rank of cls among the class ids (so that keys ascend with ids), -1 when cls is not one of them
    int rank = 0;
    bool hit = false;
    for (int c = 0; c < C; ++c) {
        const long long v = class_ids[c];
        rank += v < cls;
        hit |= v == cls;
    }
    return hit ? rank : -1;
}

__global__ __launch_bounds__(IE_THREADS) void k_ie_keys(const long long* __restrict__ gt_ids, int N, int Npad,
                                                        const int32_t* __restrict__ class_ids, int C,
                                                        int32_t* __restrict__ keys, int32_t* __restrict__ present,
                                                        int32_t* __restrict__ zero_a, long long n_zero_a,
                                                        int32_t* __restrict__ zero_b, long long n_zero_b) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    const long long t0 = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (long long i = t0; i < Npad; i += stride) {
        int key = -2;
        if (i < N) {
            const long long g = gt_ids[i];
            const long long q = gf_floor_div_1000(g);
            const int rank = ie_class_rank(q, class_ids, C);
            key = -1;
            if (rank >= 0) {
                key = rank * 1000 + (int)(g - q * 1000);
                present[key] = 1;
            }
        }
        keys[i] = key;
    }
    for (long long i = t0; i < n_zero_a; i += stride) zero_a[i] = 0;
    for (long long i = t0; i < n_zero_b; i += stride) zero_b[i] = 0;
}

__global__ __launch_bounds__(IE_SCAN_THREADS) void k_ie_slots(int32_t* __restrict__ table, int K,
                                                              const int32_t* __restrict__ class_ids, int C, int max_gt,
                                                              int32_t* __restrict__ d_G, long long* __restrict__ gt_id) {
    // table: presence (0/1) in, slot (or -1) out, in place: every thread owns one contiguous run of keys
    __shared__ int32_t sums[IE_SCAN_THREADS];
    __shared__ int32_t sorted_cls[IE_MAX_CLASSES];
    const int t = threadIdx.x;
    if (t < C) sorted_cls[ie_class_rank(class_ids[t], class_ids, C)] = class_ids[t];
    const int incl = gf_presence_to_slots<IE_SCAN_THREADS>(table, K, sorted_cls, sums, t, max_gt, gt_id);
    if (t == IE_SCAN_THREADS - 1) *d_G = incl;
}

template <bool VEC>
__global__ __launch_bounds__(IE_THREADS) void k_ie_hist(const int32_t* __restrict__ masks, int n_rows, int N,
                                                        const int32_t* __restrict__ rows, int n,
                                                        const int32_t* __restrict__ keys,
                                                        const int32_t* __restrict__ slot_of_key,
                                                        const int32_t* __restrict__ d_G, int max_gt,
                                                        int32_t* __restrict__ gt_count, int32_t* __restrict__ inter) {
    __shared__ int32_t hist[IE_ROWS * IE_TILE];
    const int G = *d_G;
    if (G > max_gt) return;  // reported through d_G; nothing is written past the caller's capacity
    const int W = G + 1;     // slots 0..G-1 are instances, slot G is void
    const int t = threadIdx.x;
    const long long p0 = (long long)blockIdx.x * IE_CHUNK + t * IE_PER_THREAD;
    const int r0 = blockIdx.y * IE_ROWS;

    int slot[IE_PER_THREAD];
    {
        const int4 k4 = *reinterpret_cast<const int4*>(keys + p0);  // keys are padded to whole chunks
        const int kk[IE_PER_THREAD] = {k4.x, k4.y, k4.z, k4.w};
#pragma unroll
        for (int j = 0; j < IE_PER_THREAD; ++j) slot[j] = kk[j] >= 0 ? slot_of_key[kk[j]] : (kk[j] == -1 ? G : -1);
    }
    unsigned bits = 0;  // bit r * IE_PER_THREAD + j: point p0 + j is in row r0 + r
#pragma unroll
    for (int r = 0; r < IE_ROWS; ++r) {
        const int row = r0 + r;
        if (row > n) break;
        if (row == n) {  // the virtual all-ones row
            bits |= 0xFu << (r * IE_PER_THREAD);
            continue;
        }
        const int mr = rows ? rows[row] : row;
        if (mr < 0 || mr >= n_rows) continue;  // an index outside the masks selects nothing
        const int32_t* m = masks + (size_t)mr * N;
        if (VEC) {
            if (p0 < N) {  // N % 4 == 0: the four points are all inside or all outside
                const int4 v = *reinterpret_cast<const int4*>(m + p0);
                bits |= (unsigned)((v.x != 0) | (v.y != 0) << 1 | (v.z != 0) << 2 | (v.w != 0) << 3) << (r * IE_PER_THREAD);
            }
        } else {
#pragma unroll
            for (int j = 0; j < IE_PER_THREAD; ++j)
                if (p0 + j < N && m[p0 + j] != 0) bits |= 1u << (r * IE_PER_THREAD + j);
        }
    }

    for (int base = 0; base < W; base += IE_TILE) {  // one pass per LDS tile of slots
        const int T = min(IE_TILE, W - base);
        for (int i = t; i < IE_ROWS * T; i += IE_THREADS) hist[i] = 0;
        __syncthreads();
        if (bits) {
#pragma unroll
            for (int j = 0; j < IE_PER_THREAD; ++j) {
                const int s = slot[j] - base;
                if (s < 0 || s >= T) continue;
#pragma unroll
                for (int r = 0; r < IE_ROWS; ++r)
                    if (bits >> (r * IE_PER_THREAD + j) & 1u) atomicAdd(&hist[r * T + s], 1);
            }
        }
        __syncthreads();
        for (int i = t; i < IE_ROWS * T; i += IE_THREADS) {
            const int v = hist[i];
            if (v == 0) continue;
            const int r = i / T, s = base + i - r * T, row = r0 + r;
            if (row < n)
                atomicAdd(&inter[(size_t)row * W + s], v);
            else if (row == n && s < G)
                atomicAdd(&gt_count[s], v);
        }
        __syncthreads();
    }
}

size_t ie_align(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

extern "C" size_t gf_instance_overlaps_scratch_bytes(int N, int C) {
    const size_t Npad = (size_t)gf_div_up(N > 0 ? N : 0, IE_CHUNK) * IE_CHUNK;
    return ie_align((size_t)(C > 0 ? C : 0) * 1000 * sizeof(int32_t)) + ie_align(Npad * sizeof(int32_t));
}

extern "C" int gf_instance_overlaps(const int32_t* masks, int n_rows, int N, const int32_t* rows, int n,
                                    const long long* gt_ids, const int32_t* class_ids, int C, int max_gt,
                                    void* scratch, int32_t* d_G, long long* gt_id, int32_t* gt_count, int32_t* inter,
                                    void* stream) {
    GF_CHECK_ARG(n_rows >= 0 && N >= 0 && n >= 0 && max_gt >= 0, "gf_instance_overlaps: bad sizes");
    GF_CHECK_ARG(C >= 1 && C <= IE_MAX_CLASSES, "gf_instance_overlaps: C = %d classes (1..%d)", C, IE_MAX_CLASSES);
    GF_CHECK_ARG(rows != nullptr || n <= n_rows, "gf_instance_overlaps: n = %d rows of %d without a row list", n, n_rows);
    GF_CHECK_ARG(n == 0 || masks != nullptr, "gf_instance_overlaps: masks is NULL");
    GF_CHECK_ARG(gt_ids != nullptr || N == 0, "gf_instance_overlaps: gt_ids is NULL");
    GF_CHECK_ARG(class_ids && scratch && d_G && (max_gt == 0 || (gt_id && gt_count)) && (n == 0 || inter),
                 "gf_instance_overlaps: NULL output or scratch");
    hipStream_t st = (hipStream_t)stream;
    const int K = C * 1000;
    const int nchunk = gf_div_up(N, IE_CHUNK);
    const long long Npad = (long long)nchunk * IE_CHUNK;
    int32_t* table = (int32_t*)scratch;
    int32_t* keys = (int32_t*)((char*)scratch + ie_align((size_t)K * sizeof(int32_t)));
    // G <= min(K, N): the outputs the histogram can reach are zero-filled up to that, not to max_gt
    const long long cap = std::min<long long>(max_gt, std::min<long long>(K, N));
    GF_TRY(hipMemsetAsync(table, 0, (size_t)K * sizeof(int32_t), st));
    const long long work = std::max<long long>(Npad, (long long)n * (cap + 1));
    const int kb = (int)std::min<long long>(std::max<long long>(gf_div_up(work, IE_THREADS), 1), 2048);
    hipLaunchKernelGGL(k_ie_keys, dim3(kb), dim3(IE_THREADS), 0, st, gt_ids, N, (int)Npad, class_ids, C, keys, table,
                       inter, (long long)n * (cap + 1), gt_count, cap);
    hipLaunchKernelGGL(k_ie_slots, dim3(1), dim3(IE_SCAN_THREADS), 0, st, table, K, class_ids, C, max_gt, d_G, gt_id);
    if (nchunk > 0) {
        const dim3 grid((unsigned)nchunk, (unsigned)gf_div_up((long long)n + 1, IE_ROWS));
        const bool vec = N % 4 == 0 && ((uintptr_t)masks & 15) == 0;
        if (vec)
            hipLaunchKernelGGL(k_ie_hist<true>, grid, dim3(IE_THREADS), 0, st, masks, n_rows, N, rows, n, keys, table,
                               d_G, max_gt, gt_count, inter);
        else
            hipLaunchKernelGGL(k_ie_hist<false>, grid, dim3(IE_THREADS), 0, st, masks, n_rows, N, rows, n, keys, table,
                               d_G, max_gt, gt_count, inter);
    }
    GF_CHECK_LAUNCH("gf_instance_overlaps");
    return GF_OK;
}
