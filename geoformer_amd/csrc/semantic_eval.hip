// Semantic-segmentation evaluation from the forward's class scores: per-point prediction and per-scene confusion
// matrices, counted on the device and accumulated there across batches (evaluation.SemanticEvaluator).
//     semantic_preds = semantic_scores.max(1)[1]                      (model/geoformer/geoformer.py:423)
//     conf[s, gt, pred] += 1 for every point of scene s               (the benchmark's evaluate_semantic_label.py)
// with the training labels of datasets/scannetv2_inst.py:314-323 restated as a lookup table, so that raw dataset
// labels need no pass of their own.
//
// One launch.  A workgroup owns SE_RUN consecutive points: every thread decides the class of SE_PER of them (the
// arg-max rule of fg_decide in foreground.hip: first maximal class, strict '>' in ascending class order, so that
// `preds >= 4` is the foreground the instance stage saw, ties and NaNs included), maps their labels and keeps the
// bin (row * C + pred) in registers.  The run is then cut at the scene boundaries it contains; per piece the
// workgroup counts its bins in an LDS table of (C + 1) * C words with LDS atomics and adds the non-zero ones to
// conf[s] with 64-bit integer atomics: exact, whatever the order.  A run inside one scene (the usual case) is one
// piece; empty scenes are stepped over.  The kernel reads the offsets defensively -- a piece never leaves the run
// and a scene index never reaches S -- so a malformed table loses counts but cannot make it write out of bounds.
#include "common.h"

namespace {

constexpr int SE_THREADS = 256;
constexpr int SE_PER = 2;                     // points per thread
constexpr int SE_RUN = SE_THREADS * SE_PER;   // consecutive points per workgroup
constexpr int SE_MAX_CLASSES = 64;            // LDS table: 65 * 64 * 4 = 16.25 KB

__global__ __launch_bounds__(SE_THREADS) void k_semantic_confusion(const float* __restrict__ scores,
                                                                   const long long* __restrict__ labels,
                                                                   const int32_t* __restrict__ offsets, int S, int N,
                                                                   int C, const int32_t* __restrict__ lut, int L,
                                                                   long long ignore_label, int map_ignore,
                                                                   int map_other, int32_t* __restrict__ preds,
                                                                   unsigned long long* __restrict__ conf) {
    extern __shared__ int32_t se_hist[];  // [(C + 1) * C]
    const int t = threadIdx.x;
    const long long run_lo = (long long)blockIdx.x * SE_RUN;
    const int run_hi = (int)min((long long)N, run_lo + SE_RUN);

    int bin[SE_PER];
#pragma unroll
    for (int i = 0; i < SE_PER; ++i) {
        const long long p = run_lo + i * SE_THREADS + t;
        bin[i] = -1;
        if (p >= N) continue;
        const float* row = scores + (size_t)p * C;
        float mx = row[0];
        int arg = 0;
        for (int k = 1; k < C; ++k) {
            const float v = row[k];
            if (v > mx) {
                mx = v;
                arg = k;
            }
        }
        if (preds) preds[p] = arg;
        if (labels) {
            const long long g = labels[p];
            int m;
            if (g == ignore_label)
                m = map_ignore;
            else if (lut)
                m = (g >= 0 && g < L) ? lut[g] : map_other;
            else
                m = (g >= 0 && g < C) ? (int)g : map_other;
            bin[i] = ((m >= 0 && m < C) ? m : C) * C + arg;
        }
    }
    if (!labels) return;

    // the scene of the run's first point: post_steps.h's gf_scene_of(offsets, S, run_lo) (written out: the call makes
    // the kernel four instructions longer)
    int s;
    {
        int lo = 0, hi = S;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (offsets[mid] > run_lo)
                hi = mid;
            else
                lo = mid + 1;
        }
        s = max(lo - 1, 0);
    }
    const int bins = (C + 1) * C;
    for (int lo = (int)run_lo; lo < run_hi && s < S; ++s) {
        const int hi = min(run_hi, offsets[s + 1]);
        if (hi <= lo) continue;  // an empty scene
        for (int i = t; i < bins; i += SE_THREADS) se_hist[i] = 0;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < SE_PER; ++i) {
            const int p = (int)run_lo + i * SE_THREADS + t;
            if (bin[i] >= 0 && p >= lo && p < hi) atomicAdd(&se_hist[bin[i]], 1);
        }
        __syncthreads();
        unsigned long long* dst = conf + (size_t)s * bins;
        for (int i = t; i < bins; i += SE_THREADS) {
            const int v = se_hist[i];
            if (v) atomicAdd(&dst[i], (unsigned long long)v);
        }
        __syncthreads();
        lo = hi;
    }
}

}  // namespace

extern "C" int gf_semantic_confusion_max_classes(void) { return SE_MAX_CLASSES; }

extern "C" int gf_semantic_confusion_run_points(void) { return SE_RUN; }

extern "C" int gf_semantic_confusion(const float* scores, const long long* labels, const int32_t* offsets,
                                     const int32_t* offsets_host, int S, int N, int C, const int32_t* lut, int L,
                                     long long ignore_label, int map_ignore, int map_other, int32_t* preds,
                                     long long* conf, void* stream) {
    GF_CHECK_ARG(N >= 0 && S >= 0, "gf_semantic_confusion: N = %d points in S = %d scenes", N, S);
    GF_CHECK_ARG(C >= 1 && C <= SE_MAX_CLASSES, "gf_semantic_confusion: C = %d classes (1..%d)", C, SE_MAX_CLASSES);
    GF_CHECK_ARG(scores != nullptr || N == 0, "gf_semantic_confusion: scores is NULL");
    GF_CHECK_ARG(lut == nullptr ? L == 0 : L >= 0, "gf_semantic_confusion: a label table of L = %d entries%s", L,
                 lut ? "" : " without the table");
    if (labels) {
        GF_CHECK_ARG(offsets != nullptr && conf != nullptr, "gf_semantic_confusion: labels without offsets or conf");
        GF_CHECK_ARG(S >= 1 || N == 0, "gf_semantic_confusion: N = %d points in no scene", N);
        if (offsets_host) {
            GF_CHECK_ARG(offsets_host[0] == 0, "gf_semantic_confusion: offsets[0] = %d, not 0", offsets_host[0]);
            for (int s = 0; s < S; ++s)
                GF_CHECK_ARG(offsets_host[s + 1] >= offsets_host[s], "gf_semantic_confusion: offsets descend at scene %d (%d after %d)",
                             s, offsets_host[s + 1], offsets_host[s]);
            GF_CHECK_ARG(offsets_host[S] == N, "gf_semantic_confusion: offsets[S] = %d, N = %d", offsets_host[S], N);
        }
    }
    if (N == 0 || (labels == nullptr && preds == nullptr)) return GF_OK;
    hipLaunchKernelGGL(k_semantic_confusion, dim3((unsigned)gf_div_up(N, SE_RUN)), dim3(SE_THREADS),
                       (size_t)(C + 1) * C * sizeof(int32_t), (hipStream_t)stream, scores, labels, offsets, S, N, C, lut, L,
                       ignore_label, map_ignore, map_other, preds, (unsigned long long*)conf);
    GF_CHECK_LAUNCH("gf_semantic_confusion");
    return GF_OK;
}
