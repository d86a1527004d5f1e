// Constants and LayerNorm helpers of the decoder's token-side kernels (decoder_layer.hip: inference,
// decoder_layer_train.hip: training): d_model 64, 4 heads x 16 channels; the tile products come from tile_gemm.h.
#pragma once
#include "tile_gemm.h"

#define DL_D 64
#define DL_H 4
#define DL_DK 16
#define DL_THREADS 1024
#define DL_MAXFF 256

#define DL_LD 68     // padded LDS row (floats): 16 rows x float4 reads without bank conflicts
#define DL_LDH 260

// torch.nn.LayerNorm over 64 channels (biased variance, eps inside the root) of the rows of an LDS tile;
// one wave per row, one channel per lane
template <typename Out>
__device__ __forceinline__ void dl_tile_layernorm_p(const float (*S)[DL_LD], int nvalid, float wl, float bl, int wave,
                                                    int nwaves, int lane, Out out);
template <typename Out>
__device__ __forceinline__ void dl_tile_layernorm(const float (*S)[DL_LD], int nvalid, const float* __restrict__ w,
                                                  const float* __restrict__ b, int wave, int nwaves, int lane,
                                                  Out out) {
    dl_tile_layernorm_p(S, nvalid, w[lane], b[lane], wave, nwaves, lane, out);
}
// (wl, bl: the lane's channel of the norm's weight and bias, loaded by the caller -- ahead of the phase, if it likes)
template <typename Out>
__device__ __forceinline__ void dl_tile_layernorm_p(const float (*S)[DL_LD], int nvalid, float wl, float bl, int wave,
                                                    int nwaves, int lane, Out out) {
    for (int r = wave; r < nvalid; r += nwaves) {
        const float v = S[r][lane];
        // (gf_wave_sum: the same butterfly as six __shfl_xor steps without the LDS crossbar -- a norm of 16 rows by four
        //  waves was 48 dependent ds_bpermute round trips, ~5 300 cycles)
        const float s = gf_wave_sum(v);
        const float mu = s / (float)DL_D;
        const float dv = v - mu;
        const float q = gf_wave_sum(dv * dv);
        const float rstd = 1.0f / sqrtf(q / (float)DL_D + 1e-5f);
        out(r, lane, dv * rstd * wl + bl);
    }
}

