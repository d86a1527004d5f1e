// Steps that the sparse convolution forward kernels repeat (spconv_conv.hip: k_conv_os, k_conv_flat, k_conv_g16, k_conv_g16p;
// spconv_lw.hip: k_conv_lw), each defined once.  All of them are forced inline and were checked to leave the kernels' machine
// code as it was (tools/isa_diff.sh); where a kernel's code would change, that kernel keeps the step written out and says so.
#pragma once
#include "common.h"

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));  // what a raw_buffer_load_b128 returns

__device__ __forceinline__ float4 gf_as_float4(u32x4 v) {
    return make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
}

// Gathers and weight loads go through buffer descriptors -- a 32-bit per-lane offset instead of 64-bit pointer arithmetic,
// a scalar offset for the (uniform) weight block, and the hardware range check turns "missing neighbour" (an offset past
// `bytes`, e.g. 0xffffffff) into zeros without a branch or memory traffic.  (0x00020000: raw 32-bit data format.)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t gf_buffer_rsrc(const void* p, int bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, bytes, 0x00020000);
}

// Fused BatchNorm + ReLU prologue of the transposed kernels on this lane's four channels: act(x) = max(x*sc + sh, 0) on a
// present row, 0 on a missing one (whose gather read zeros: without the flag it would become max(sh, 0)).
__device__ __forceinline__ float4 gf_act_present(float4 x, bool present, const float4& sc, const float4& sh) {
    x.x = present ? fmaxf(fmaf(x.x, sc.x, sh.x), 0.f) : 0.f;
    x.y = present ? fmaxf(fmaf(x.y, sc.y, sh.y), 0.f) : 0.f;
    x.z = present ? fmaxf(fmaf(x.z, sc.z, sh.z), 0.f) : 0.f;
    x.w = present ? fmaxf(fmaf(x.w, sc.w, sh.w), 0.f) : 0.f;
    return x;
}

// Epilogue activation: the consumer's eval-mode BatchNorm + ReLU, once per output element (four channels of one row).
__device__ __forceinline__ float4 gf_relu_affine(float4 v, float4 os, float4 ot) {
    v.x = fmaxf(fmaf(v.x, os.x, ot.x), 0.f); v.y = fmaxf(fmaf(v.y, os.y, ot.y), 0.f);
    v.z = fmaxf(fmaf(v.z, os.z, ot.z), 0.f); v.w = fmaxf(fmaf(v.w, os.w, ot.w), 0.f);
    return v;
}

// This lane's 16 bytes of packed-weight block `blk` (1 KiB each, gf_conv_pack_weights): a conflict-free ds_read_b128 of the
// copy staged in LDS, or a load through the weight descriptor with the (uniform) block as the scalar offset.
extern __shared__ __attribute__((aligned(16))) float4 s_w[];  // the workgroup's dynamic LDS: the packed weights, staged by the kernel
template <bool LDSW>
__device__ __forceinline__ void gf_conv_w(float4& dst, __amdgpu_buffer_rsrc_t rs_w, int blk, int lane) {
    if (LDSW) {
        dst = s_w[blk * 64 + lane];
    } else {
        dst = gf_as_float4(__builtin_amdgcn_raw_buffer_load_b128(rs_w, (unsigned)lane * 16u, (unsigned)blk * 1024u, 0));
    }
}

// Fixed-order sum of four waves' partial tiles (this lane's float4 of each, `stride` float4 apart in LDS): (0 + 1) + (2 + 3).
__device__ __forceinline__ float4 gf_sum4(float4 p0, float4 p1, float4 p2, float4 p3) {
    return make_float4((p0.x + p1.x) + (p2.x + p3.x), (p0.y + p1.y) + (p2.y + p3.y), (p0.z + p1.z) + (p2.z + p3.z),
                       (p0.w + p1.w) + (p2.w + p3.w));
}
__device__ __forceinline__ float4 gf_lds_sum4(const float4* p, int stride) {
    return gf_sum4(p[0], p[stride], p[2 * stride], p[3 * stride]);
}
