// Per-query bodies of the proposal kernels (GeoFormer.generate_proposal, model/geoformer/geoformer.py:193-262), shared
// by the one-scene launches (proposal.hip) and the batched ones over a scene table (batch_post.hip): both produce the
// same bits for a query because they run this code with the same workgroup shape.
#pragma once
#include "common.h"

#define PR_THREADS 1024

__device__ __forceinline__ float pr_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// One workgroup of PR_THREADS threads for query row `row` [N] with class logits `c` [ncls]; sem_prob is class-major
// with row stride `sem_stride` (the predicted class's probabilities are sem_prob[cls * sem_stride + p], p < N).
// Thread 0 writes the four outputs through the given pointers.
__device__ __forceinline__ void pr_stats_row(const float* __restrict__ row, const float* __restrict__ c,
                                             const float* __restrict__ sem_prob, size_t sem_stride, int N, int ncls,
                                             float logit_thresh, float score_thresh, int npoint_thresh, int min_class,
                                             int* cls_pred_out, int* npoints_out, float* scores_out, int* final_out) {
    __shared__ int s_cls;
    __shared__ float s_cls_score;
    __shared__ int r_cnt[PR_THREADS / 64];
    __shared__ float r_prob[PR_THREADS / 64], r_sem[PR_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) {
        // soft-max over the classes and its arg-max (first maximum), geoformer.py:215-216
        float mx = c[0];
        int arg = 0;
        for (int k = 1; k < ncls; k++)
            if (c[k] > mx) {
                mx = c[k];
                arg = k;
            }
        float den = 0.f;
        for (int k = 0; k < ncls; k++) den += expf(c[k] - mx);
        s_cls = arg;
        s_cls_score = 1.0f / den;  // exp(0) / sum
    }
    __syncthreads();
    const int cls = s_cls;
    const float* sem_row = sem_prob + (size_t)cls * sem_stride;  // class-major: the predicted class is one contiguous row
    int cnt = 0;
    float sp = 0.f, ss = 0.f;
    // four independent points per thread and trip (loads of a trip go out together; the class probability is
    // fetched for every point, from a clamped index, and selected afterwards)
    for (int p0 = tid; p0 < N; p0 += 4 * PR_THREADS) {
        float x[4], sv[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int p = p0 + e * PR_THREADS;
            const int pc = p < N ? p : N - 1;
            x[e] = row[pc];
            sv[e] = sem_row[pc];
        }
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const float pr = pr_sigmoid(x[e]);
            const bool in = (p0 + e * PR_THREADS) < N && pr >= logit_thresh;
            cnt += in ? 1 : 0;
            sp += in ? pr : 0.f;
            ss += in ? sv[e] : 0.f;
        }
    }
    cnt = gf_wave_sum_i(cnt);  // (the __shfl_xor butterflies without the LDS crossbar: common.h)
    sp = gf_wave_sum(sp);
    ss = gf_wave_sum(ss);
    if (lane == 0) {
        r_cnt[wave] = cnt;
        r_prob[wave] = sp;
        r_sem[wave] = ss;
    }
    __syncthreads();
    if (tid == 0) {
        int n = 0;
        float a = 0.f, b = 0.f;
        for (int w = 0; w < PR_THREADS / 64; w++) {
            n += r_cnt[w];
            a += r_prob[w];
            b += r_sem[w];
        }
        const float den = (float)n + 1e-6f;
        const float mask_score = a / den, sem_score = b / den;
        *cls_pred_out = cls;
        *npoints_out = n;
        *scores_out = mask_score * sqrtf(s_cls_score) * sem_score;
        *final_out = (cls >= min_class) && (n >= npoint_thresh) && (mask_score >= score_thresh);
    }
}

// Accepted queries of one scene in ascending order (one workgroup of 1024 threads): sel / cls_out / scores_out get the
// first *count entries.
__device__ __forceinline__ void pr_select_rows(const int32_t* __restrict__ final_, const int32_t* __restrict__ cls_pred,
                                               const float* __restrict__ scores, int nq, int32_t* __restrict__ sel,
                                               long long* __restrict__ cls_out, float* __restrict__ scores_out,
                                               int32_t* __restrict__ count) {
    __shared__ int s_w[16];
    __shared__ int s_run;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_run = 0;
    __syncthreads();
    for (int base = 0; base < nq; base += 1024) {
        const int q = base + threadIdx.x;
        const bool f = q < nq && final_[q] != 0;
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
        const int run = s_run;
        if (f) {
            const int pos = run + before + __popcll(bal & ((1ull << lane) - 1ull));
            sel[pos] = q;
            cls_out[pos] = cls_pred[q];
            scores_out[pos] = scores[q];
        }
        __syncthreads();
        if (threadIdx.x == 0) s_run = run + total;
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = s_run;
}
