// fp32 tile products of the token-side kernels (decoder stages: decoder_layer*.hip; voxel transformer: backbone_attn.hip):
// 16-row tiles on v_mfma_f32_16x16x4_f32 with operands loaded straight from row-major activations (LDS tiles or global rows)
// and row-major nn.Linear weights [out,in].  Lane (j = lane&15, g = lane>>4) loads 16 bytes at column 4g of row j; the MFMA k
// index is only a summation index, so both operands use the same 4g+kk permutation and no packing is needed.
#pragma once
#include "common.h"

__device__ __forceinline__ f32x4 gf_mfma4(float4 a, float4 b, f32x4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
    return acc;
}

// one 16-row tile: epi(r, col, act(sum_k A[r][k] W[col][k] + b[col]) (+ addend[r][col])) for the column tiles ct = wave,
// wave+nw, ...  A may live in LDS or global memory (row stride lda); rows >= nvalid read as zero and are not emitted.
// A phase of the token-side kernels is one of these between two barriers, and what it costs is its dependent memory round
// trips, not its 16-64 MFMAs (cycle stamps, round 6: ~5 000 cycles per phase whatever its size): the bias and the
// epilogue's global operand (`addend`, row stride add_ld: a residual row the caller would otherwise read inside `epi`) are
// therefore requested BEFORE the products, beside the weights, instead of one after the other behind them.
template <bool RELU, typename Epi>
__device__ __forceinline__ void gf_tile_gemm(const float* A, int lda, int nvalid, int K, const float* __restrict__ W,
                                             const float* __restrict__ bias, int N, int wave, int nwaves, int lane,
                                             Epi epi, const float* __restrict__ addend = nullptr, int add_ld = 0) {
    const int j = lane & 15, g = lane >> 4;
    const int KC = K >> 4;
    for (int ct = wave; ct < (N >> 4); ct += nwaves) {
        const float* xa = A + (size_t)j * lda + 4 * g;
        const float* wb = W + (size_t)(ct * 16 + j) * K + 4 * g;
        const int col = ct * 16 + j;
        const float bs = bias[col];
        float ad[4] = {0.f, 0.f, 0.f, 0.f};
        if (addend) {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (4 * g + i < nvalid) ad[i] = addend[(size_t)(4 * g + i) * add_ld + col];
        }
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
        for (int kc = 0; kc < KC; kc++) {
            float4 a = j < nvalid ? *reinterpret_cast<const float4*>(xa + kc * 16) : make_float4(0.f, 0.f, 0.f, 0.f);
            float4 b = *reinterpret_cast<const float4*>(wb + kc * 16);
            acc = gf_mfma4(a, b, acc);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int r = 4 * g + i;
            if (r >= nvalid) continue;
            float v = acc[i] + bs;
            if (RELU) v = fmaxf(v, 0.f);
            if (addend) v += ad[i];
            epi(r, col, v);
        }
    }
}

// The same product with its weight operands ALREADY in registers: a token-side kernel is a chain of small products between
// barriers, one wave per SIMD, and every phase used to open with its own weight fetch (~1 500-2 000 cycles of a ~4 500-cycle
// phase: cycle stamps, round 6).  gf_tile_w_load requests a phase's operands -- NT column tiles per wave x KC 16-channel
// steps, + bias -- any number of phases ahead (the kernels do it at entry, all phases at once: one round trip for the lot);
// gf_tile_gemm_w consumes them.  Same arithmetic and order as gf_tile_gemm.
template <int NT, int KC>
struct GfTileW {
    float4 b[NT][KC];
    float bias[NT];
};
template <int NT, int KC>
__device__ __forceinline__ void gf_tile_w_load(GfTileW<NT, KC>& w, const float* __restrict__ W, const float* __restrict__ bias,
                                               int N, int K, int wave, int nwaves, int lane) {
    const int j = lane & 15, g = lane >> 4;
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const int ct = wave + t * nwaves;
        const bool on = ct < (N >> 4);
        const float* wb = W + (size_t)((on ? ct : 0) * 16 + j) * K + 4 * g;
        w.bias[t] = on ? bias[ct * 16 + j] : 0.f;
#pragma unroll
        for (int kc = 0; kc < KC; kc++)
            w.b[t][kc] = (on && kc < (K >> 4)) ? *reinterpret_cast<const float4*>(wb + kc * 16) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
template <bool RELU, int NT, int KC, typename Epi>
__device__ __forceinline__ void gf_tile_gemm_w(const float* A, int lda, int nvalid, int K, int N, int wave, int nwaves, int lane,
                                               const GfTileW<NT, KC>& w, Epi epi, const float* __restrict__ addend = nullptr,
                                               int add_ld = 0) {
    const int j = lane & 15, g = lane >> 4;
    const float* xa = A + (size_t)j * lda + 4 * g;
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const int ct = wave + t * nwaves;
        if (ct >= (N >> 4)) break;
        const int col = ct * 16 + j;
        float ad[4] = {0.f, 0.f, 0.f, 0.f};
        if (addend) {
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (4 * g + i < nvalid) ad[i] = addend[(size_t)(4 * g + i) * add_ld + col];
        }
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < KC; kc++) {
            if (kc < (K >> 4)) {
                float4 a = j < nvalid ? *reinterpret_cast<const float4*>(xa + kc * 16) : make_float4(0.f, 0.f, 0.f, 0.f);
                acc = gf_mfma4(a, w.b[t][kc], acc);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int r = 4 * g + i;
            if (r >= nvalid) continue;
            float v = acc[i] + w.bias[t];
            if (RELU) v = fmaxf(v, 0.f);
            if (addend) v += ad[i];
            epi(r, col, v);
        }
    }
}

// out[r][col] = sum_o A[r][o] W[o][col]: the product with a row-major nn.Linear weight [out,in] summed over its OUT index
// (training: the gradient towards a layer's input).  A: LDS tile of 16 rows (rows that do not exist hold zeros), K = number
// of summed rows of W (row stride ldw), N = columns produced (multiple of 16)
template <typename Epi>
__device__ __forceinline__ void gf_tile_gemm_t(const float* A, int lda, int K, const float* __restrict__ W, int ldw, int N,
                                               int wave, int nwaves, int lane, Epi epi) {
    const int j = lane & 15, g = lane >> 4;
    const int KC = K >> 4;
    for (int ct = wave; ct < (N >> 4); ct += nwaves) {
        const float* xa = A + (size_t)j * lda + 4 * g;
        const float* wb = W + (size_t)(4 * g) * ldw + ct * 16 + j;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
        for (int kc = 0; kc < KC; kc++) {
            const float4 a = *reinterpret_cast<const float4*>(xa + kc * 16);
            const float* w = wb + (size_t)kc * 16 * ldw;
            const float4 b = make_float4(w[0], w[ldw], w[2 * (size_t)ldw], w[3 * (size_t)ldw]);
            acc = gf_mfma4(a, b, acc);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) epi(4 * g + i, ct * 16 + j, acc[i]);
    }
}
