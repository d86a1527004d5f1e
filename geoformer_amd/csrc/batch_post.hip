// Post-processing of a batched eval forward: proposals and matrix NMS of B scenes in a fixed number of launches
// (GeoFormer.generate_proposal, model/geoformer/geoformer.py:193-262, once per scene; matrix NMS,
// util/utils_3d.py:95-141, once per scene in test.py:88-93).  Every kernel reads a device scene table (int64 rows,
// layouts in include/geoformer_hip.h) instead of taking one scene's pointers as arguments:
//   k_bp_stats         grid (nq, S): the statistics of gf_proposal_stats per (scene, query), same row body;
//   k_bp_select        grid S: the accepted queries of each scene in ascending order, and the scene's count;
//   k_bp_scatter       grid (x, rows): accepted rows of all scenes into ONE packed int32 buffer, scene b's block of
//                      counts[b] x num_points[b] after the blocks of the scenes before it (offsets from the counts);
//   k_bp_pack_bits /   grid (x, S): gf_mask_intersections' ballot packing and popcount pairs, one [n_b, n_b] block per
//   k_bp_intersections scene;
//   k_bp_matrix_nms    grid S: one workgroup per scene does the whole [n, n] algebra of matrix NMS in LDS;
//   k_bp_greedy_nms /  grid S / 1: greedy NMS (util/utils_3d.py:76-93), one workgroup per scene walks the proposals in
//   k_bp_greedy_ious   score order, one barrier per pick.
#include "proposal_rows.h"

#define BP_NMS_MAX_N GF_NMS_MAX_N
static_assert(sizeof(GfPropScene) == 8 * GF_PROP_SCENE_FIELDS && sizeof(GfNmsScene) == 8 * GF_NMS_SCENE_FIELDS,
              "the rows of include/geoformer_hip.h");

__global__ __launch_bounds__(PR_THREADS) void k_bp_stats(const long long* __restrict__ table, int nq,
                                                         const float* __restrict__ cls_logits,
                                                         const float* __restrict__ sem_prob, long long sem_stride,
                                                         int ncls, float logit_thresh, float score_thresh,
                                                         int npoint_thresh, int min_class, int* __restrict__ cls_pred,
                                                         int* __restrict__ npoints, float* __restrict__ scores,
                                                         int* __restrict__ final_out) {
    const int q = blockIdx.x, b = blockIdx.y;
    const GfPropScene* t = gf_row<GfPropScene>(table, b);
    const int N = (int)t->N;
    const float* row = (const float*)t->logits + (size_t)q * N;
    const size_t o = (size_t)b * nq + q;
    pr_stats_row(row, cls_logits + o * ncls, sem_prob + t->fg_off, (size_t)sem_stride, N, ncls, logit_thresh,
                 score_thresh, npoint_thresh, min_class, cls_pred + o, npoints + o, scores + o, final_out + o);
}

__global__ __launch_bounds__(1024) void k_bp_select(const int32_t* __restrict__ final_, const int32_t* __restrict__ cls_pred,
                                                    const float* __restrict__ scores, int nq, int32_t* __restrict__ sel,
                                                    long long* __restrict__ cls_out, float* __restrict__ scores_out,
                                                    int32_t* __restrict__ counts) {
    const size_t o = (size_t)blockIdx.x * nq;
    pr_select_rows(final_ + o, cls_pred + o, scores + o, nq, sel + o, cls_out + o, scores_out + o, counts + blockIdx.x);
}

__global__ __launch_bounds__(256) void k_bp_scatter(const long long* __restrict__ table, int S, int nq,
                                                    const int32_t* __restrict__ sel, const int32_t* __restrict__ counts,
                                                    const long long* __restrict__ fg_idxs, float logit_thresh,
                                                    int* __restrict__ packed) {
    // packed row r -> (scene b, i-th accepted query of b); element offset of b's block = sum over earlier scenes of
    // counts x num_points (the host slices the buffer with the same sums)
    const int r = blockIdx.y;
    int b = 0, row0 = 0;
    size_t base = 0;
    for (; b < S; b++) {
        const int c = counts[b];
        if (r < row0 + c) break;
        row0 += c;
        base += (size_t)c * (size_t)gf_row<GfPropScene>(table, b)->num_points;
    }
    if (b == S) return;
    const GfPropScene* t = gf_row<GfPropScene>(table, b);
    const int N = (int)t->N;
    const long long pt_off = t->pt_off, num_points = t->num_points;
    const int i = r - row0;
    const float* row = (const float*)t->logits + (size_t)sel[(size_t)b * nq + i] * N;
    const long long* fg = fg_idxs + t->fg_off;
    int* out = packed + base + (size_t)i * num_points;
    const int stride = gridDim.x * 256;
    for (int p0 = blockIdx.x * 256 + threadIdx.x; p0 < N; p0 += 4 * stride) {
        float x[4];
        long long dst[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int p = p0 + e * stride;
            const int pc = p < N ? p : N - 1;
            x[e] = row[pc];
            dst[e] = fg[pc] - pt_off;
        }
#pragma unroll
        for (int e = 0; e < 4; e++)
            if ((p0 + e * stride) < N && pr_sigmoid(x[e]) >= logit_thresh && dst[e] >= 0 && dst[e] < num_points)
                out[dst[e]] = 1;
    }
}

extern "C" int gf_proposal_stats_batched(const long long* table, int S, int nq, const float* cls_logits,
                                         const float* sem_prob, long long sem_stride, int ncls, float logit_thresh,
                                         float score_thresh, int npoint_thresh, int min_class, int* cls_pred,
                                         int* npoints, float* scores, int* final_mask, void* stream) {
    GF_CHECK_ARG(table && cls_logits && sem_prob && cls_pred && npoints && scores && final_mask,
                 "gf_proposal_stats_batched: null argument");
    GF_CHECK_ARG(S >= 0 && S <= 65535 && nq >= 0 && ncls >= 1 && sem_stride >= 0,
                 "gf_proposal_stats_batched: bad sizes S=%d nq=%d ncls=%d", S, nq, ncls);
    if (S == 0 || nq == 0) return GF_OK;
    hipLaunchKernelGGL(k_bp_stats, dim3(nq, S), dim3(PR_THREADS), 0, (hipStream_t)stream, table, nq, cls_logits,
                       sem_prob, sem_stride, ncls, logit_thresh, score_thresh, npoint_thresh, min_class, cls_pred,
                       npoints, scores, final_mask);
    GF_CHECK_LAUNCH("gf_proposal_stats_batched");
    return GF_OK;
}

extern "C" int gf_proposal_select_batched(const int32_t* final_, const int32_t* cls_pred, const float* scores, int S,
                                          int nq, int32_t* sel, long long* cls_out, float* scores_out, int32_t* counts,
                                          void* stream) {
    // nq == 0: empty arrays have no address; the launch only writes counts[b] = 0
    GF_CHECK_ARG(counts && S >= 0 && nq >= 0 &&
                     (nq == 0 || (final_ && cls_pred && scores && sel && cls_out && scores_out)),
                 "gf_proposal_select_batched: bad arguments");
    if (S == 0) return GF_OK;
    hipLaunchKernelGGL(k_bp_select, dim3(S), dim3(1024), 0, (hipStream_t)stream, final_, cls_pred, scores, nq, sel,
                       cls_out, scores_out, counts);
    GF_CHECK_LAUNCH("gf_proposal_select_batched");
    return GF_OK;
}

extern "C" int gf_proposal_scatter_batched(const long long* table, int S, int nq, const int32_t* sel,
                                           const int32_t* counts, int total_rows, int max_N, const long long* fg_idxs,
                                           float logit_thresh, int* packed, void* stream) {
    GF_CHECK_ARG(table && sel && counts && fg_idxs && packed, "gf_proposal_scatter_batched: null argument");
    GF_CHECK_ARG(S >= 0 && nq >= 0 && total_rows >= 0 && total_rows <= 65535 && max_N >= 0,
                 "gf_proposal_scatter_batched: bad sizes S=%d rows=%d", S, total_rows);
    if (S == 0 || total_rows == 0 || max_N == 0) return GF_OK;
    const int bx = gf_div_up(max_N, 256 * 4);
    hipLaunchKernelGGL(k_bp_scatter, dim3(bx, total_rows), dim3(256), 0, (hipStream_t)stream, table, S, nq, sel,
                       counts, fg_idxs, logit_thresh, packed);
    GF_CHECK_LAUNCH("gf_proposal_scatter_batched");
    return GF_OK;
}

// ------------------------------------------------------------------------------------
// Pairwise intersections per scene (gf_mask_intersections over a scene table)
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bp_pack_bits(const long long* __restrict__ table,
                                                      unsigned long long* __restrict__ bits) {
    const GfNmsScene* t = gf_row<GfNmsScene>(table, blockIdx.y);
    const int32_t* masks = (const int32_t*)t->masks;
    const long long N = t->N, n = t->n, W2 = (N + 63) / 64;
    unsigned long long* out = bits + t->bits_off;
    const int lane = threadIdx.x & 63;
    // one wave per (row, 64-point block), grid-stride over the scene's waves (wave-uniform trip count)
    for (long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); w < n * W2; w += (long long)gridDim.x * 4) {
        const long long row = w / W2, blk = w - row * W2;
        const long long p = blk * 64 + lane;
        const bool on = p < N && masks[row * N + p] != 0;
        const unsigned long long bb = __ballot(on);
        if (lane == 0) out[w] = bb;
    }
}

__global__ __launch_bounds__(256) void k_bp_intersections(const long long* __restrict__ table,
                                                          const unsigned long long* __restrict__ bits,
                                                          int32_t* __restrict__ inter) {
    const GfNmsScene* t = gf_row<GfNmsScene>(table, blockIdx.y);
    const long long N = t->N, n = t->n, W2 = (N + 63) / 64;
    const unsigned long long* sb = bits + t->bits_off;
    int32_t* out = inter + t->inter_off;
    const int lane = threadIdx.x & 63;
    for (long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); w < n * n; w += (long long)gridDim.x * 4) {
        const long long i = w / n, j = w - i * n;
        if (j < i) continue;
        const unsigned long long *a = sb + i * W2, *c = sb + j * W2;
        int cnt = 0;
        for (long long k = lane; k < W2; k += 64) cnt += __popcll(a[k] & c[k]);
        cnt = gf_wave_sum_i(cnt);
        if (lane == 0) {
            out[i * n + j] = cnt;
            out[j * n + i] = cnt;
        }
    }
}

extern "C" int gf_mask_intersections_batched(const long long* table, int S, long long max_waves, long long max_pairs,
                                             void* bits, int32_t* inter, void* stream) {
    GF_CHECK_ARG(table && bits && inter, "gf_mask_intersections_batched: null argument");
    GF_CHECK_ARG(S >= 0 && S <= 65535 && max_waves >= 0 && max_pairs >= 0, "gf_mask_intersections_batched: bad sizes");
    if (S == 0 || max_pairs == 0) return GF_OK;
    hipStream_t st = (hipStream_t)stream;
    const long long cap = 8192;  // workgroups per scene and launch; the waves stride over the rest
    if (max_waves > 0) {
        const long long gx = (max_waves + 3) / 4;
        hipLaunchKernelGGL(k_bp_pack_bits, dim3((unsigned)(gx < cap ? gx : cap), S), dim3(256), 0, st, table,
                           (unsigned long long*)bits);
    }
    const long long gx = (max_pairs + 3) / 4;
    hipLaunchKernelGGL(k_bp_intersections, dim3((unsigned)(gx < cap ? gx : cap), S), dim3(256), 0, st, table,
                       (const unsigned long long*)bits, inter);
    GF_CHECK_LAUNCH("gf_mask_intersections_batched");
    return GF_OK;
}

// ------------------------------------------------------------------------------------
// Matrix NMS, one workgroup per scene (util/utils_3d.py:95-141).  In sorted order (position a = rank by score):
//   iou[r,a]  = I / ((d_r + d_a) - I),  I = inter[ord r, ord a], d = the diagonal (torch's fp32 expression);
//   label     = cat_r == cat_a && r < a;  x[r,a] = label ? iou[r,a] : 0;
//   comp[a]   = max_r x[r,a];
//   coef[a]   = min_r exp(-sigma x[r,a]^2) / exp(-sigma comp[r]^2)   (gaussian)
//             = min_r (1 - x[r,a]) / (1 - comp[r])                   (linear);
//   kept      = score_a * coef[a] >= final_score_thresh, written as original indices in descending-score order.
// Ties: equal scores are ranked by ascending index (torch.argsort leaves their order unspecified).  The [n, n] IoUs are
// recomputed from the L2-resident intersection block in both passes instead of being held (1024 x 1024 fp32 would not
// fit in LDS); a column per wave, the 64 lanes over its rows.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ float bp_max_nan(float m, float v) { return (v > m || v != v) ? v : m; }
__device__ __forceinline__ float bp_min_nan(float m, float v) { return (v < m || v != v) ? v : m; }

__global__ __launch_bounds__(1024) void k_bp_matrix_nms(const long long* __restrict__ table,
                                                        const int32_t* __restrict__ inter_all, int linear, float sigma,
                                                        float final_score_thresh, int32_t* __restrict__ picks,
                                                        int32_t* __restrict__ pick_counts) {
    __shared__ float s_score[BP_NMS_MAX_N], s_diag[BP_NMS_MAX_N], s_cden[BP_NMS_MAX_N];
    __shared__ long long s_cat[BP_NMS_MAX_N];
    __shared__ int s_ord[BP_NMS_MAX_N];
    __shared__ int s_keep[BP_NMS_MAX_N];
    __shared__ int s_w[16];
    const GfNmsScene* t = gf_row<GfNmsScene>(table, blockIdx.x);
    const int n = (int)t->n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (n <= 0 || n > BP_NMS_MAX_N) {  // (the host rejects n > BP_NMS_MAX_N before the launch)
        if (tid == 0) pick_counts[blockIdx.x] = 0;
        return;
    }
    const float* scores = (const float*)t->scores;
    const long long* cats = (const long long*)t->cats;
    const int32_t* inter = inter_all + t->inter_off;
    // 1. rank = #(higher score, or equal score and lower index): a permutation for non-NaN scores; slots a NaN leaves
    //    unwritten keep index 0 (in bounds)
    for (int a = tid; a < n; a += 1024) s_ord[a] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 1024) {
        const float si = scores[i];
        int r = 0;
        for (int j = 0; j < n; j++) {
            const float sj = scores[j];
            r += (sj > si || (sj == si && j < i)) ? 1 : 0;
        }
        if (r < n) s_ord[r] = i;
    }
    __syncthreads();
    for (int a = tid; a < n; a += 1024) {
        const int o = s_ord[a];
        s_score[a] = scores[o];
        s_cat[a] = cats[o];
        s_diag[a] = (float)inter[(size_t)o * n + o];
    }
    __syncthreads();
    // 2. compensation: per column a, the largest same-class IoU with a higher-ranked proposal (0 if none), kept as the
    //    denominator of the ratio in step 3
    const float neg_sigma = -1.0f * sigma;
    for (int a = wave; a < n; a += 16) {
        const int oa = s_ord[a];
        const long long ca = s_cat[a];
        const float da = s_diag[a];
        float m = 0.f;
        for (int r = lane; r < a; r += 64) {
            if (s_cat[r] != ca) continue;
            const float I = (float)inter[(size_t)oa * n + s_ord[r]];
            m = bp_max_nan(m, I / ((s_diag[r] + da) - I));
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) m = bp_max_nan(m, __shfl_xor(m, off));
        if (lane == 0) s_cden[a] = linear ? 1.0f - m : expf(neg_sigma * (m * m));
    }
    __syncthreads();
    // 3. decay coefficient: per column a, the minimum ratio over ALL rows r (rows without a same-class higher-ranked
    //    relation contribute x = 0)
    for (int a = wave; a < n; a += 16) {
        const int oa = s_ord[a];
        const long long ca = s_cat[a];
        const float da = s_diag[a];
        float m = INFINITY;
        for (int r = lane; r < n; r += 64) {
            float x = 0.f;
            if (r < a && s_cat[r] == ca) {
                const float I = (float)inter[(size_t)oa * n + s_ord[r]];
                x = I / ((s_diag[r] + da) - I);
            }
            const float v = (linear ? 1.0f - x : expf(neg_sigma * (x * x))) / s_cden[r];
            m = bp_min_nan(m, v);
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) m = bp_min_nan(m, __shfl_xor(m, off));
        if (lane == 0) s_keep[a] = (s_score[a] * m) >= final_score_thresh;
    }
    __syncthreads();
    // 4. kept positions in order -> original indices
    int32_t* out = picks + t->pick_off;
    int run = 0;
    for (int base = 0; base < n; base += 1024) {
        const int a = base + tid;
        const bool f = a < n && s_keep[a] != 0;
        const unsigned long long bal = __ballot(f);
        if (lane == 0) s_w[wave] = __popcll(bal);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; w++) {
            const int c = s_w[w];
            if (w < wave) before += c;
            total += c;
        }
        if (f) out[run + before + __popcll(bal & ((1ull << lane) - 1ull))] = s_ord[a];
        run += total;
        __syncthreads();
    }
    if (tid == 0) pick_counts[blockIdx.x] = run;
}

extern "C" int gf_matrix_nms_batched(const long long* table, int S, const int32_t* inter, int kernel, float sigma,
                                     float final_score_thresh, int32_t* picks, int32_t* pick_counts, void* stream) {
    GF_CHECK_ARG(table && inter && picks && pick_counts, "gf_matrix_nms_batched: null argument");
    GF_CHECK_ARG(S >= 0 && (kernel == 0 || kernel == 1), "gf_matrix_nms_batched: bad arguments S=%d kernel=%d", S,
                 kernel);
    if (S == 0) return GF_OK;
    hipLaunchKernelGGL(k_bp_matrix_nms, dim3(S), dim3(1024), 0, (hipStream_t)stream, table, inter, kernel, sigma,
                       final_score_thresh, picks, pick_counts);
    GF_CHECK_LAUNCH("gf_matrix_nms_batched");
    return GF_OK;
}

// ------------------------------------------------------------------------------------
// Greedy NMS, one workgroup per scene (util/utils_3d.py:76-93).  Proposals ranked by score, descending, equal scores by
// ascending index (the rule of k_bp_matrix_nms).  Walk the ranks: a rank still alive is picked and kills every later
// rank j with iou[pick, j] > threshold (strict; the row is the pick; a NaN never kills; a dead rank kills nothing).
// Thread j is rank j and keeps its own alive flag; the workgroup's view of the flags is one uint64 word per wave in LDS
// (16 words = GF_NMS_MAX_N ranks).  Per PICK, not per rank: every thread finds the next alive rank from the words (dead
// pivots cost nothing), the waves that still hold later ranks read their element of the pick's row, ballot the kills,
// lane 0 clears them in the wave's word, one barrier.
// The scan of the next iteration may overlap another wave's clears of that iteration.  That is harmless: pick q clears
// only bits above q, bit q stays set, and the scan stops at the first set bit above the previous pick, which is q.
// ------------------------------------------------------------------------------------
template <bool FROM_INTER>
__device__ __forceinline__ void bp_greedy_walk(const void* __restrict__ mat, const float* __restrict__ scores, int n,
                                               float threshold, int32_t* __restrict__ out,
                                               int32_t* __restrict__ count) {
    __shared__ float s_score[BP_NMS_MAX_N], s_diag[BP_NMS_MAX_N];
    __shared__ int s_ord[BP_NMS_MAX_N];
    __shared__ unsigned long long s_alive[BP_NMS_MAX_N / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t* inter = (const int32_t*)mat;
    const float* ious = (const float*)mat;
    // 1. rank = #(higher score, or equal score and lower index); slots a NaN leaves unwritten keep index 0 (in bounds)
    if (tid < n) {
        s_ord[tid] = 0;
        s_score[tid] = scores[tid];
    }
    __syncthreads();
    if (tid < n) {
        const float si = s_score[tid];
        int r = 0;
        for (int j = 0; j < n; j++) {
            const float sj = s_score[j];
            r += (sj > si || (sj == si && j < tid)) ? 1 : 0;
        }
        if (r < n) s_ord[r] = tid;
    }
    __syncthreads();
    bool alive = tid < n;
    const int oj = alive ? s_ord[tid] : 0;
    float dj = 0.f;
    if (FROM_INTER) {
        if (alive) dj = (float)inter[(size_t)oj * n + oj];
        s_diag[tid] = dj;
    }
    {
        const unsigned long long bal = __ballot(alive);
        if (lane == 0) s_alive[wave] = bal;
    }
    __syncthreads();
    // 2. the walk
    int p = -1, cnt = 0;
    while (true) {
        int q = -1;
        for (int w = (p + 1) >> 6; w < BP_NMS_MAX_N / 64; w++) {
            unsigned long long m = s_alive[w];
            if (w == ((p + 1) >> 6)) m &= ~0ull << ((p + 1) & 63);
            if (m) {
                q = w * 64 + __ffsll((long long)m) - 1;
                break;
            }
        }
        if (q < 0) break;  // (uniform: every thread read the same words, see above)
        p = q;
        const int op = s_ord[p];
        if (tid == 0) out[cnt] = op;
        cnt++;
        if (wave * 64 + 63 > p) {  // wave-uniform: the wave holds ranks after the pick
            bool kill = false;
            if (alive && tid > p) {
                float v;
                if (FROM_INTER) {
                    const float I = (float)inter[(size_t)op * n + oj];
                    v = I / ((s_diag[p] + dj) - I);
                } else {
                    v = ious[(size_t)op * n + oj];
                }
                kill = v > threshold;
            }
            const unsigned long long bal = __ballot(kill);
            alive = alive && !kill;
            if (lane == 0 && bal) s_alive[wave] &= ~bal;
        }
        __syncthreads();
    }
    if (tid == 0) *count = cnt;
}

__global__ __launch_bounds__(1024) void k_bp_greedy_nms(const long long* __restrict__ table,
                                                        const int32_t* __restrict__ inter_all, float threshold,
                                                        int32_t* __restrict__ picks,
                                                        int32_t* __restrict__ pick_counts) {
    const GfNmsScene* t = gf_row<GfNmsScene>(table, blockIdx.x);
    const int n = (int)t->n;
    if (n <= 0 || n > BP_NMS_MAX_N) {  // (the host rejects n > BP_NMS_MAX_N before the launch)
        if (threadIdx.x == 0) pick_counts[blockIdx.x] = 0;
        return;
    }
    bp_greedy_walk<true>(inter_all + t->inter_off, (const float*)t->scores, n, threshold, picks + t->pick_off,
                         pick_counts + blockIdx.x);
}

__global__ __launch_bounds__(1024) void k_bp_greedy_ious(const float* __restrict__ ious,
                                                         const float* __restrict__ scores, int n, float threshold,
                                                         int32_t* __restrict__ picks, int32_t* __restrict__ pick_count) {
    bp_greedy_walk<false>(ious, scores, n, threshold, picks, pick_count);
}

extern "C" int gf_greedy_nms_batched(const long long* table, int S, const int32_t* inter, float threshold,
                                     int32_t* picks, int32_t* pick_counts, void* stream) {
    GF_CHECK_ARG(table && inter && picks && pick_counts, "gf_greedy_nms_batched: null argument");
    GF_CHECK_ARG(S >= 0, "gf_greedy_nms_batched: bad arguments S=%d", S);
    if (S == 0) return GF_OK;
    hipLaunchKernelGGL(k_bp_greedy_nms, dim3(S), dim3(1024), 0, (hipStream_t)stream, table, inter, threshold, picks,
                       pick_counts);
    GF_CHECK_LAUNCH("gf_greedy_nms_batched");
    return GF_OK;
}

extern "C" int gf_greedy_nms_ious(const float* ious, const float* scores, int n, float threshold, int32_t* picks,
                                  int32_t* pick_count, void* stream) {
    GF_CHECK_ARG(pick_count && n >= 0 && n <= BP_NMS_MAX_N, "gf_greedy_nms_ious: bad arguments n=%d (at most %d)", n,
                 BP_NMS_MAX_N);
    GF_CHECK_ARG(n == 0 || (ious && scores && picks), "gf_greedy_nms_ious: null argument");
    if (n == 0) {
        GF_TRY(hipMemsetAsync(pick_count, 0, sizeof(int32_t), (hipStream_t)stream));
        return GF_OK;
    }
    hipLaunchKernelGGL(k_bp_greedy_ious, dim3(1), dim3(1024), 0, (hipStream_t)stream, ious, scores, n, threshold, picks,
                       pick_count);
    GF_CHECK_LAUNCH("gf_greedy_nms_ious");
    return GF_OK;
}
