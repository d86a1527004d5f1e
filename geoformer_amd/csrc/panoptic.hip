// Panoptic labelling and the tables of panoptic quality (Kirillov et al., "Panoptic Segmentation", CVPR 2019) for a
// batch of S scenes packed one after the other: per point the panoptic id (things from the label map, stuff from the
// semantic head) and, per scene, the contingency table of predicted segments against ground-truth segments.
//     row of a point  = owner (a rank into pick)             when 0 <= owner < P
//                     = P + stuff rank of stuff_of_sem[sem]   when that names a stuff class
//                     = R - 1 (unlabelled), R = P + n_stuff + 1
//     column          = slot of the point's key among the scene's distinct keys in ascending order (np.unique's);
//                       key = class rank * 1000 + id mod 1000 for a thing (k_ie_keys' scheme), class rank * 1000 for
//                       a stuff class (its instances are ONE segment); void (class not evaluated) = the last column
//
// Four commands on the caller's stream, no host synchronisation, whatever S, N and P are:
//   memset          presence tables, S * C * 1000 words
//   k_pan_keys      one pass over the points (the only read of owner, sem, gt_ids): row and key of every point packed
//                   in one word, the presence mark of the key in its scene's table, pan; zero-fills inter and gt_id
//   k_pan_slots     one workgroup per scene: exclusive scan of the presence table -> slot per key, G_s, gt_id
//                   (post_steps.h's gf_presence_to_slots)
//   k_pan_count     a workgroup owns PAN_RUN consecutive points, cut at the scene boundaries the run contains (empty
//                   scenes are stepped over).  Per piece, one (row, column) pair per point, counted in one of two ways:
//                     R * (G_s + 1) <= lds_bins: an LDS table of that many words (LDS atomics), flushed as one global
//                                   integer atomic per non-zero bin;
//                     otherwise:    wave-aggregated global integer atomics, one per distinct pair per wave.
// Integer atomics only: the counts are exact and do not depend on the schedule.  A scene with G_s > max_gt is reported
// through d_G alone; nothing of it is counted and nothing is written past the capacities.
#include <algorithm>
#include <atomic>

#include "common.h"
#include "geoformer_hip_dev.h"
#include "post_steps.h"

namespace {

constexpr int PAN_THREADS = 256;
constexpr int PAN_PER = 4;                          // points per thread
constexpr int PAN_RUN = PAN_THREADS * PAN_PER;      // consecutive points per workgroup
constexpr int PAN_LDS_BINS = 8192;                  // LDS table of k_pan_count: 32 KB
constexpr int PAN_MAX_CLASSES = 64;
constexpr int PAN_MAX_ROWS = GF_NMS_MAX_N + PAN_MAX_CLASSES + 1;  // P <= GF_NMS_MAX_N picks, the stuff classes, unlabelled
constexpr int PAN_SCAN_THREADS = 1024;
constexpr int PAN_KEY_BITS = 17;                    // key + 1 <= 64 * 1000 < 2^17; the row sits above

std::atomic<int> g_lds_bins{-1};  // dev knob: capacity of the LDS table in bins, -1 = PAN_LDS_BINS

__global__ __launch_bounds__(PAN_THREADS) void k_pan_keys(
    const int32_t* __restrict__ owner, const int32_t* __restrict__ ids, const int32_t* __restrict__ sem,
    const long long* __restrict__ gt_ids, const int32_t* __restrict__ offsets, int S, int N,
    const int32_t* __restrict__ class_ids, const int32_t* __restrict__ is_stuff, int C,
    const int32_t* __restrict__ stuff_of_sem, int L, int n_stuff, int P, int32_t* __restrict__ packed,
    int32_t* __restrict__ present, int32_t* __restrict__ pan, int32_t* __restrict__ zero_a, long long n_zero_a,
    int32_t* __restrict__ zero_b, long long n_zero_b) {
    __shared__ int32_t s_cls[PAN_MAX_CLASSES];    // class_ids
    __shared__ int32_t s_rank[PAN_MAX_CLASSES];   // rank of the class among class_ids (keys ascend with ids)
    __shared__ int32_t s_srank[PAN_MAX_CLASSES];  // rank among the stuff classes in class_ids order, -1 for a thing
    const int t = threadIdx.x;
    if (t < C) {
        const int v = class_ids[t];
        int rank = 0, srank = 0;
        for (int c = 0; c < C; ++c) {
            rank += class_ids[c] < v;
            srank += c < t && is_stuff[c] != 0;
        }
        s_cls[t] = v;
        s_rank[t] = rank;
        s_srank[t] = is_stuff[t] != 0 ? srank : -1;
    }
    __syncthreads();
    const int K = C * 1000;
    const int R = P + n_stuff + 1;
    const long long stride = (long long)gridDim.x * PAN_RUN;
    for (long long run_lo = (long long)blockIdx.x * PAN_RUN; run_lo < N; run_lo += stride) {
        const int s0 = gf_scene_of(offsets, S, run_lo);  // (uniform over the workgroup)
#pragma unroll
        for (int i = 0; i < PAN_PER; ++i) {
            const long long p = run_lo + i * PAN_THREADS + t;
            if (p >= N) continue;
            int s = s0;
            while (s + 1 < S && offsets[s + 1] <= p) ++s;
            // predicted row
            const int o = owner[p];
            int row = R - 1, label = 0;
            if (o >= 0 && o < P) {
                row = o;
                if (pan) label = ids[p];
            } else {
                const int m = sem[p];
                const int c = (m >= 0 && m < L) ? stuff_of_sem[m] : -1;
                if (c >= 0 && c < C && s_srank[c] >= 0 && s_srank[c] < n_stuff) {
                    row = P + s_srank[c];
                    label = s_cls[c] * 1000;
                }
            }
            if (pan) pan[p] = label;
            if (!gt_ids) continue;  // (uniform: labels only)
            // ground-truth key
            const long long g = gt_ids[p];
            const long long q = gf_floor_div_1000(g);
            int key = -1;
            for (int c = 0; c < C; ++c) {
                if ((long long)s_cls[c] == q) {
                    key = s_rank[c] * 1000 + (s_srank[c] >= 0 ? 0 : (int)(g - q * 1000));
                    break;
                }
            }
            if (key >= 0) present[(size_t)s * K + key] = 1;
            packed[p] = (row << PAN_KEY_BITS) | (key + 1);
        }
    }
    const long long g0 = (long long)blockIdx.x * PAN_THREADS + t, gs = (long long)gridDim.x * PAN_THREADS;
    for (long long i = g0; i < n_zero_a; i += gs) zero_a[i] = 0;
    for (long long i = g0; i < n_zero_b; i += gs) zero_b[i] = 0;
}

__global__ __launch_bounds__(PAN_SCAN_THREADS) void k_pan_slots(int32_t* __restrict__ tables, int K,
                                                                const int32_t* __restrict__ class_ids, int C, int max_gt,
                                                                int32_t* __restrict__ d_G, long long* __restrict__ gt_id) {
    // one scene's table: presence (0/1) in, slot (or -1) out, in place: every thread owns one contiguous run of keys
    __shared__ int32_t sums[PAN_SCAN_THREADS];
    __shared__ int32_t sorted_cls[PAN_MAX_CLASSES];
    int32_t* table = tables + (size_t)blockIdx.x * K;
    long long* gid = gt_id + (size_t)blockIdx.x * max_gt;
    const int t = threadIdx.x;
    if (t < C) {
        const int v = class_ids[t];
        int rank = 0;
        for (int c = 0; c < C; ++c) rank += class_ids[c] < v;
        sorted_cls[rank] = v;
    }
    const int incl = gf_presence_to_slots<PAN_SCAN_THREADS>(table, K, sorted_cls, sums, t, max_gt, gid);
    if (t == PAN_SCAN_THREADS - 1) d_G[blockIdx.x] = incl;
}

__global__ __launch_bounds__(PAN_THREADS) void k_pan_count(const int32_t* __restrict__ packed,
                                                           const int32_t* __restrict__ offsets, int S, int N, int K, int R,
                                                           const int32_t* __restrict__ slot_of_key,
                                                           const int32_t* __restrict__ d_G, int max_gt, int lds_bins,
                                                           int32_t* __restrict__ inter) {
    __shared__ int32_t hist[PAN_LDS_BINS];
    const int t = threadIdx.x;
    const int lane = t & 63;
    const long long run_lo = (long long)blockIdx.x * PAN_RUN;
    const int run_hi = (int)min((long long)N, run_lo + PAN_RUN);
    int pk[PAN_PER];
#pragma unroll
    for (int i = 0; i < PAN_PER; ++i) {
        const long long p = run_lo + i * PAN_THREADS + t;
        pk[i] = p < N ? packed[p] : -1;
    }
    const int W = max_gt + 1;
    int s = gf_scene_of(offsets, S, run_lo);
    for (int lo = (int)run_lo; lo < run_hi && s < S; ++s) {
        const int hi = min(run_hi, offsets[s + 1]);
        if (hi <= lo) continue;  // an empty scene
        const int G = d_G[s];
        if (G >= 0 && G <= max_gt) {  // (otherwise reported through d_G; nothing of the scene is counted)
            const int32_t* slots = slot_of_key + (size_t)s * K;
            int32_t* dst = inter + (size_t)s * R * W;
            const int Wl = G + 1;  // the scene's own columns: instances 0..G-1, void at G
            const long long bins = (long long)R * Wl;
            int pair[PAN_PER];  // row * Wl + column, -1 outside the piece
#pragma unroll
            for (int i = 0; i < PAN_PER; ++i) {
                const int p = (int)run_lo + i * PAN_THREADS + t;
                pair[i] = -1;
                if (pk[i] >= 0 && p >= lo && p < hi) {
                    const int row = pk[i] >> PAN_KEY_BITS, key = (pk[i] & ((1 << PAN_KEY_BITS) - 1)) - 1;
                    const int col = key >= 0 ? slots[key] : G;
                    if (row < R && col >= 0 && col <= G) pair[i] = row * Wl + col;
                }
            }
            if (bins <= lds_bins) {  // (uniform over the workgroup)
                const int nb = (int)bins;
                for (int i = t; i < nb; i += PAN_THREADS) hist[i] = 0;
                __syncthreads();
#pragma unroll
                for (int i = 0; i < PAN_PER; ++i)
                    if (pair[i] >= 0) atomicAdd(&hist[pair[i]], 1);
                __syncthreads();
                for (int i = t; i < nb; i += PAN_THREADS) {
                    const int v = hist[i];
                    if (v == 0) continue;
                    const int row = i / Wl, col = i - row * Wl;
                    atomicAdd(&dst[(size_t)row * W + (col == G ? max_gt : col)], v);
                }
                __syncthreads();
            } else {
#pragma unroll
                for (int i = 0; i < PAN_PER; ++i) {
                    // the lanes that hold the first open lane's pair leave together: one atomic per distinct pair
                    // (post_steps.h's gf_wave_add_per_key with the pair decoded before the add; written out: the
                    // shared loop over a functor makes the kernel 12 instructions longer)
                    unsigned long long open = __ballot(pair[i] >= 0);
                    while (open) {
                        const int leader = __ffsll((long long)open) - 1;
                        const int v = __shfl(pair[i], leader, 64);
                        const unsigned long long same = __ballot(pair[i] == v) & open;
                        if (lane == leader) {
                            const int row = v / Wl, col = v - row * Wl;
                            atomicAdd(&dst[(size_t)row * W + (col == G ? max_gt : col)], __popcll(same));
                        }
                        open &= ~same;
                    }
                }
            }
        }
        lo = hi;
    }
}

size_t pan_align(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace

extern "C" int gf_panoptic_max_rows(void) { return PAN_MAX_ROWS; }

extern "C" int gf_panoptic_run_points(void) { return PAN_RUN; }

extern "C" int gf_dev_panoptic_lds_bins(int bins) {
    GF_CHECK_ARG(bins >= -1 && bins <= PAN_LDS_BINS, "gf_dev_panoptic_lds_bins: %d bins (-1 = default, 0..%d)", bins,
                 PAN_LDS_BINS);
    g_lds_bins.store(bins);
    return GF_OK;
}

extern "C" size_t gf_panoptic_overlaps_scratch_bytes(int S, int N, int C) {
    const size_t s = S > 0 ? S : 0, n = N > 0 ? N : 0, c = C > 0 ? C : 0;
    return pan_align(s * c * 1000 * sizeof(int32_t)) + pan_align(n * sizeof(int32_t));
}

extern "C" int gf_panoptic_overlaps(const int32_t* owner, const int32_t* ids, const int32_t* sem, const long long* gt_ids,
                                    const int32_t* offsets, const int32_t* offsets_host, int S, int N,
                                    const int32_t* class_ids, const int32_t* is_stuff, int C, const int32_t* stuff_of_sem,
                                    int L, int n_stuff, int P, int max_gt, void* scratch, int32_t* pan, int32_t* d_G,
                                    long long* gt_id, int32_t* inter, void* stream) {
    GF_CHECK_ARG(N >= 0 && S >= 0 && (S >= 1 || N == 0), "gf_panoptic_overlaps: N = %d points in S = %d scenes", N, S);
    GF_CHECK_ARG(C >= 1 && C <= PAN_MAX_CLASSES, "gf_panoptic_overlaps: C = %d classes (1..%d)", C, PAN_MAX_CLASSES);
    GF_CHECK_ARG(n_stuff >= 0 && n_stuff <= C && P >= 0 && P + n_stuff + 1 <= PAN_MAX_ROWS && L >= 0,
                 "gf_panoptic_overlaps: P = %d picks, %d stuff classes of %d, L = %d (at most %d rows)", P, n_stuff, C, L,
                 PAN_MAX_ROWS);
    const int R = P + n_stuff + 1;
    GF_CHECK_ARG(max_gt >= 0 && (long long)S * R * ((long long)max_gt + 1) <= 0x7fffffffLL,
                 "gf_panoptic_overlaps: max_gt = %d with %d rows in %d scenes", max_gt, R, S);
    GF_CHECK_ARG(class_ids && is_stuff && (L == 0 || stuff_of_sem), "gf_panoptic_overlaps: NULL class tables");
    GF_CHECK_ARG(N == 0 || (owner && sem), "gf_panoptic_overlaps: NULL per-point input");
    GF_CHECK_ARG(pan == nullptr || ids != nullptr || N == 0, "gf_panoptic_overlaps: pan without ids");
    GF_CHECK_ARG(gt_ids != nullptr || pan != nullptr || N == 0, "gf_panoptic_overlaps: neither gt_ids nor pan");
    const bool tables_wanted = gt_ids != nullptr || N == 0;
    GF_CHECK_ARG(S == 0 || (offsets && (!tables_wanted || (scratch && d_G && inter && (max_gt == 0 || gt_id)))),
                 "gf_panoptic_overlaps: NULL offsets, scratch or output");
    if (offsets_host) {
        GF_CHECK_ARG(offsets_host[0] == 0, "gf_panoptic_overlaps: offsets[0] = %d, not 0", offsets_host[0]);
        for (int s = 0; s < S; ++s)
            GF_CHECK_ARG(offsets_host[s + 1] >= offsets_host[s], "gf_panoptic_overlaps: offsets descend at scene %d (%d after %d)",
                         s, offsets_host[s + 1], offsets_host[s]);
        GF_CHECK_ARG(offsets_host[S] == N, "gf_panoptic_overlaps: offsets[S] = %d, N = %d", offsets_host[S], N);
    }
    if (S == 0) return GF_OK;
    hipStream_t st = (hipStream_t)stream;
    const int K = C * 1000;
    if (!tables_wanted) {  // labels only: one launch, no table is touched
        hipLaunchKernelGGL(k_pan_keys, dim3((unsigned)std::min(gf_div_up(N, PAN_RUN), 2048)), dim3(PAN_THREADS), 0, st, owner,
                           ids, sem, gt_ids, offsets, S, N, class_ids, is_stuff, C, stuff_of_sem, L, n_stuff, P,
                           (int32_t*)nullptr, (int32_t*)nullptr, pan, (int32_t*)nullptr, 0LL, (int32_t*)nullptr, 0LL);
        GF_CHECK_LAUNCH("gf_panoptic_overlaps");
        return GF_OK;
    }
    int32_t* tables = (int32_t*)scratch;
    int32_t* packed = (int32_t*)((char*)scratch + pan_align((size_t)S * K * sizeof(int32_t)));
    const long long n_inter = (long long)S * R * (max_gt + 1), n_gid = (long long)S * max_gt * 2;  // (int64 as two words)
    GF_TRY(hipMemsetAsync(tables, 0, (size_t)S * K * sizeof(int32_t), st));
    const long long work = std::max<long long>(gf_div_up(N, PAN_PER), std::max(n_inter, n_gid));
    const int kb = (int)std::min<long long>(std::max<long long>(gf_div_up(work, PAN_THREADS), 1), 2048);
    hipLaunchKernelGGL(k_pan_keys, dim3(kb), dim3(PAN_THREADS), 0, st, owner, ids, sem, gt_ids, offsets, S, N, class_ids,
                       is_stuff, C, stuff_of_sem, L, n_stuff, P, packed, tables, pan, inter, n_inter, (int32_t*)gt_id, n_gid);
    hipLaunchKernelGGL(k_pan_slots, dim3(S), dim3(PAN_SCAN_THREADS), 0, st, tables, K, class_ids, C, max_gt, d_G, gt_id);
    if (N > 0) {
        const int knob = g_lds_bins.load();
        hipLaunchKernelGGL(k_pan_count, dim3((unsigned)gf_div_up(N, PAN_RUN)), dim3(PAN_THREADS), 0, st, packed, offsets, S,
                           N, K, R, tables, d_G, max_gt, knob < 0 ? PAN_LDS_BINS : knob, inter);
    }
    GF_CHECK_LAUNCH("gf_panoptic_overlaps");
    return GF_OK;
}
