// Training-batch augmentation and collate on the GPU (geoformer_amd/augment.py; reference: InstDataset.trainMerge,
// datasets/scannetv2_inst.py:142-232 and 267-387, numpy / scipy on the DataLoader workers).
//
// Per scene, in the reference's order: x @ m (jitter / flip / rotation), * scale, two elastic distortions (three noise
// grids per pass, six separable 3-tap box blurs each, trilinear displacement), - min, crop to max_npoint, label remap,
// getCroppedInstLabel, per-instance statistics, collate.  Every stage is one launch over all scenes of a batch (or over
// one scene: the parity mode draws from numpy between stages), blockIdx.y = scene.  Per-scene scalars live in a record
// of GF_AUG_REC 64-bit words (include/geoformer_hip.h, GF_AUG_R_*).
//
// The coordinate path is fp64 like numpy's; the build compiles with -ffp-contract=off, so no multiply-add is fused
// that numpy does not fuse.  Per-scene extrema are reduced with integer atomics on order-preserving keys, per-instance
// sums as int64 fixed point (2^-32): both exact, so the result does not depend on the order the blocks run in.
//
// Few-shot episodes (FSInstDataset.trainMergeFS, datasets/scannetv2_fs_inst.py:330-365 and 397-566) reuse every stage
// of the query up to the crop; the collate kernels take a mode (fs = 1: binary label against the scene's sampled class,
// scene-local instance ids, raw colours, no instance_infos).  The support scenes take their own three launches
// (k_sup_*): no augmentation and no crop, xyz = xyz_origin * scale - min, the mask of one instance id.
#include "common.h"

#define AUG_T 256

namespace {

// ---- order-preserving 64-bit keys of doubles (atomicMin / atomicMax on them are min / max on the doubles) ----
__device__ __forceinline__ unsigned long long dkey(double d) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(d);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double dkey_inv(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmax(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ double wave_min_d(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmin(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ long long wave_max_ll(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const long long o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// ---- Philox4x32-10 (Salmon et al., SC'11) and the draws built on it ----
struct U4 {
    uint32_t x, y, z, w;
};
__device__ __forceinline__ U4 philox(U4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = U4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}
// counter (cell, draw << 2 | axis, scene, batch index), key = seed
__device__ __forceinline__ U4 draw_words(unsigned long long seed, long long bi, int scene, int draw, int axis,
                                         uint32_t cell) {
    return philox(U4{cell, (uint32_t)(draw << 2 | axis), (uint32_t)scene, (uint32_t)bi}, (uint32_t)seed,
                  (uint32_t)(seed >> 32));
}
// Box-Muller on the first two words: u1 in (0, 1], u2 in [0, 1); |z| <= sqrt(2 ln 2^32) < 6.67
__device__ __forceinline__ double normal_of(U4 w) {
    const double u1 = ((double)w.x + 1.0) * 2.3283064365386963e-10, u2 = (double)w.y * 2.3283064365386963e-10;
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}
// 53-bit uniform in [0, 1) (numpy's construction from two words)
__device__ __forceinline__ double uniform_of(U4 w) {
    return ((double)(w.x >> 5) * 67108864.0 + (double)(w.y >> 6)) * (1.0 / 9007199254740992.0);
}
enum { DRAW_PARAMS = 0, DRAW_NOISE0 = 1, DRAW_NOISE1 = 2, DRAW_CROP = 3, DRAW_SHIFT = 4 };

__device__ __forceinline__ long long* rec_of(long long* rec, int s) { return rec + (size_t)s * GF_AUG_REC; }
__device__ __forceinline__ double rec_d(const long long* r, int i) { return __longlong_as_double(r[i]); }

// noise-grid extents of a pass: int32(abs max) // gran + 3 per axis (datasets/scannetv2_inst.py:147)
__device__ __forceinline__ void grid_dims(const long long* r, int pass, int gran, int bb[3]) {
    const long long* amax = r + (pass == 0 ? GF_AUG_R_AMAX0 : GF_AUG_R_AMAX1);
#pragma unroll
    for (int a = 0; a < 3; a++) bb[a] = (int)__longlong_as_double(amax[a]) / gran + 3;
}
__device__ __forceinline__ long long grid_cells(const int bb[3]) { return (long long)bb[0] * bb[1] * bb[2]; }

// ======================= draws (rng="device") =======================
__global__ void k_draw(long long* rec, int B, int K, unsigned long long seed, long long bi) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= B) return;
    long long* r = rec_of(rec, s);
    double g[9];
    for (int i = 0; i < 9; i++) g[i] = normal_of(draw_words(seed, bi, s, DRAW_PARAMS, 0, i));
    const double flip = (draw_words(seed, bi, s, DRAW_PARAMS, 1, 0).x & 1u) ? 1.0 : 0.0;
    const double theta = uniform_of(draw_words(seed, bi, s, DRAW_PARAMS, 2, 0)) * 6.283185307179586;
    double m[9];
    for (int i = 0; i < 9; i++) m[i] = (i % 4 == 0 ? 1.0 : 0.0) + g[i] * 0.1;
    m[0] *= flip * 2.0 - 1.0;
    const double c = cos(theta), sn = sin(theta);
    const double R[9] = {c, sn, 0.0, -sn, c, 0.0, 0.0, 0.0, 1.0};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double v = m[i * 3 + 0] * R[0 * 3 + j];
            v = v + m[i * 3 + 1] * R[1 * 3 + j];
            v = v + m[i * 3 + 2] * R[2 * 3 + j];
            r[GF_AUG_R_M + i * 3 + j] = __double_as_longlong(v);
        }
    r[GF_AUG_R_FLIP] = __double_as_longlong(flip);
    r[GF_AUG_R_THETA] = __double_as_longlong(theta);
    for (int a = 0; a < 3; a++) {  // torch.randn(3) * 0.1 in fp32, added to fp64 colours
        const float z = (float)normal_of(draw_words(seed, bi, s, DRAW_SHIFT, a, 0));
        r[GF_AUG_R_SHIFT + a] = __double_as_longlong((double)(z * 0.1f));
    }
    for (int k = 0; k < K; k++)
        for (int a = 0; a < 3; a++)
            r[GF_AUG_R_CROPU + k * 3 + a] = __double_as_longlong(uniform_of(draw_words(seed, bi, s, DRAW_CROP, a, k)));
}

// ======================= transform: xyz_middle = x @ m, xyz = xyz_middle * scale, |xyz| max =======================
__global__ __launch_bounds__(AUG_T) void k_transform(const double* __restrict__ raw, const long long* __restrict__ off,
                                                     long long* rec, double* __restrict__ xm, double* __restrict__ xyz,
                                                     double scale) {
    const int y = blockIdx.y;
    long long* r = rec_of(rec, y);
    double m[9];
#pragma unroll
    for (int i = 0; i < 9; i++) m[i] = rec_d(r, GF_AUG_R_M + i);
    double amax[3] = {0.0, 0.0, 0.0};
    for (long long p = off[y] + blockIdx.x * AUG_T + threadIdx.x; p < off[y + 1]; p += (long long)gridDim.x * AUG_T) {
        const double x0 = raw[p * 8 + 0], x1 = raw[p * 8 + 1], x2 = raw[p * 8 + 2];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double v = x0 * m[j];
            v = v + x1 * m[3 + j];
            v = v + x2 * m[6 + j];
            const double s = v * scale;
            xm[p * 3 + j] = v;
            xyz[p * 3 + j] = s;
            amax[j] = fmax(amax[j], fabs(s));
        }
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const double v = wave_max_d(amax[j]);  // |x| >= 0: the bit patterns order like the values
        if ((threadIdx.x & 63) == 0)
            atomicMax((unsigned long long*)&r[GF_AUG_R_AMAX0 + j], (unsigned long long)__double_as_longlong(v));
    }
}

// ======================= elastic distortion =======================
// raw noise of a pass: per scene 3 grids of bb0*bb1*bb2 cells (C order) at noise + base + axis*cap; a grid larger than
// the scene's capacity is an error (the scene's record gets GF_AUG_ERR_CELLS and no cell is touched)
__device__ __forceinline__ bool scene_grid(const long long* r, int pass, int gran, int bb[3], long long* base,
                                           long long* cap) {
    grid_dims(r, pass, gran, bb);
    *cap = r[pass == 0 ? GF_AUG_R_CAP0 : GF_AUG_R_CAP1];
    *base = r[pass == 0 ? GF_AUG_R_BASE0 : GF_AUG_R_BASE1];
    return grid_cells(bb) <= *cap;
}

__global__ __launch_bounds__(AUG_T) void k_noise(long long* rec, int s0, int pass, int gran, float* __restrict__ noise,
                                                 unsigned long long seed, long long bi) {
    const int y = blockIdx.y, a = blockIdx.z;
    long long* r = rec_of(rec, y);
    int bb[3];
    long long base, cap;
    if (!scene_grid(r, pass, gran, bb, &base, &cap)) {
        if (blockIdx.x == 0 && threadIdx.x == 0 && a == 0) atomicOr((unsigned long long*)&r[GF_AUG_R_ERR], GF_AUG_ERR_CELLS);
        return;
    }
    const long long n = grid_cells(bb);
    float* g = noise + base + a * cap;
    for (long long c = blockIdx.x * AUG_T + threadIdx.x; c < n; c += (long long)gridDim.x * AUG_T)
        g[c] = (float)normal_of(draw_words(seed, bi, s0 + y, pass == 0 ? DRAW_NOISE0 : DRAW_NOISE1, a, (uint32_t)c));
}

// one 3-tap box pass along `axis` (scipy.ndimage.convolve, mode constant 0, fp32 weights 1/3): fp64 sum in tap order
// -1, 0, +1 from 0.0, stored as fp32
__global__ __launch_bounds__(AUG_T) void k_blur(long long* rec, int pass, int gran, int axis,
                                                const float* __restrict__ src, float* __restrict__ dst) {
    const int y = blockIdx.y, a = blockIdx.z;
    const long long* r = rec_of(rec, y);
    int bb[3];
    long long base, cap;
    if (!scene_grid(r, pass, gran, bb, &base, &cap)) return;
    const long long n = grid_cells(bb);
    const float* s = src + base + a * cap;
    float* d = dst + base + a * cap;
    const long long stride = axis == 0 ? (long long)bb[1] * bb[2] : axis == 1 ? bb[2] : 1;
    const int len = bb[axis];
    const double w = (double)(1.0f / 3.0f);
    for (long long c = blockIdx.x * AUG_T + threadIdx.x; c < n; c += (long long)gridDim.x * AUG_T) {
        const int i = (int)((c / stride) % len);
        double acc = 0.0;
        acc = acc + (i > 0 ? (double)s[c - stride] * w : 0.0);
        acc = acc + (double)s[c] * w;
        acc = acc + (i + 1 < len ? (double)s[c + stride] * w : 0.0);
        d[c] = (float)acc;
    }
}

// x + g(x) * mag with g the trilinear interpolation of the three blurred grids on the axes
// linspace(-(b-1) gran, (b-1) gran, b) (scipy RegularGridInterpolator, linear, fill 0 outside); then the per-scene
// reductions the next stage needs: pass 0 -> |x| max (the second pass's grid), pass 1 -> min and max
__global__ __launch_bounds__(AUG_T) void k_displace(const long long* __restrict__ off, long long* rec, int pass, int gran,
                                                    double mag, const float* __restrict__ grids,
                                                    double* __restrict__ xyz) {
    const int y = blockIdx.y;
    long long* r = rec_of(rec, y);
    int bb[3];
    long long base, cap;
    const bool ok = scene_grid(r, pass, gran, bb, &base, &cap);
    const double h = 2.0 * gran;
    double red0[3] = {0.0, 0.0, 0.0}, red1[3] = {0.0, 0.0, 0.0};  // pass 0: |x| max; pass 1: min, max
    if (pass == 1)
        for (int a = 0; a < 3; a++) red0[a] = INFINITY, red1[a] = -INFINITY;
    for (long long p = off[y] + blockIdx.x * AUG_T + threadIdx.x; p < off[y + 1]; p += (long long)gridDim.x * AUG_T) {
        double x[3] = {xyz[p * 3 + 0], xyz[p * 3 + 1], xyz[p * 3 + 2]};
        double g[3] = {0.0, 0.0, 0.0};
        int idx[3];
        double t[3];
        bool inside = ok;
        for (int a = 0; a < 3 && inside; a++) {
            const double lo = -(double)(bb[a] - 1) * gran, hi = (double)(bb[a] - 1) * gran;
            if (!(x[a] >= lo && x[a] <= hi)) {
                inside = false;
                break;
            }
            int i = (int)floor((x[a] - lo) / h);
            i = i < 0 ? 0 : (i > bb[a] - 2 ? bb[a] - 2 : i);
            // the interval of a binary search: grid[i] <= x < grid[i+1] (last interval closed)
            if (i > 0 && x[a] < lo + i * h) i--;
            if (i < bb[a] - 2 && x[a] >= lo + (i + 1) * h) i++;
            idx[a] = i;
            t[a] = (x[a] - (lo + i * h)) / ((lo + (i + 1) * h) - (lo + i * h));
        }
        if (inside) {
            for (int a = 0; a < 3; a++) {
                const float* G = grids + base + a * cap;
                double v = 0.0;
                for (int c = 0; c < 8; c++) {  // corners in itertools.product order (last axis fastest)
                    const int c0 = (c >> 2) & 1, c1 = (c >> 1) & 1, c2 = c & 1;
                    double wgt = c0 ? t[0] : 1.0 - t[0];
                    wgt = wgt * (c1 ? t[1] : 1.0 - t[1]);
                    wgt = wgt * (c2 ? t[2] : 1.0 - t[2]);
                    const long long cell = ((long long)(idx[0] + c0) * bb[1] + (idx[1] + c1)) * bb[2] + (idx[2] + c2);
                    v = v + (double)G[cell] * wgt;
                }
                g[a] = v;
            }
        }
        for (int a = 0; a < 3; a++) {
            const double nx = x[a] + g[a] * mag;
            xyz[p * 3 + a] = nx;
            if (pass == 0) {
                red0[a] = fmax(red0[a], fabs(nx));
            } else {
                red0[a] = fmin(red0[a], nx);
                red1[a] = fmax(red1[a], nx);
            }
        }
    }
    for (int a = 0; a < 3; a++) {
        if (pass == 0) {
            const double v = wave_max_d(red0[a]);
            if ((threadIdx.x & 63) == 0)
                atomicMax((unsigned long long*)&r[GF_AUG_R_AMAX1 + a], (unsigned long long)__double_as_longlong(v));
        } else {
            const double mn = wave_min_d(red0[a]), mx = wave_max_d(red1[a]);
            if ((threadIdx.x & 63) == 0 && mn <= mx) {
                atomicMin((unsigned long long*)&r[GF_AUG_R_MIN + a], dkey(mn));
                atomicMax((unsigned long long*)&r[GF_AUG_R_MAX + a], dkey(mx));
            }
        }
    }
}

// ======================= crop (datasets/scannetv2_inst.py:206-222) =======================
// candidate k: full_scale (fs - 32k, fs - 32k, fs), offset = min(full_scale - range + 0.001, 0) * u_k
__device__ __forceinline__ void crop_offset(const long long* r, int fs, int k, double o[3], double fsk[3]) {
    for (int a = 0; a < 3; a++) {
        const double mn = dkey_inv((unsigned long long)r[GF_AUG_R_MIN + a]);
        const double range = dkey_inv((unsigned long long)r[GF_AUG_R_MAX + a]) - mn;
        fsk[a] = (double)(a < 2 ? fs - 32 * k : fs);
        o[a] = fmin((fsk[a] - range) + 0.001, 0.0) * rec_d(r, GF_AUG_R_CROPU + k * 3 + a);
    }
}

__global__ __launch_bounds__(AUG_T) void k_crop_count(const long long* __restrict__ off, long long* rec, int fs, int K,
                                                      long long max_npoint, const double* __restrict__ xyz) {
    __shared__ int cnt[GF_AUG_MAX_CROP];
    __shared__ double so[GF_AUG_MAX_CROP][3], sf[GF_AUG_MAX_CROP][3];
    const int y = blockIdx.y;
    long long* r = rec_of(rec, y);
    if (off[y + 1] - off[y] <= max_npoint) return;  // the reference's loop does not start: nothing drawn, all kept
    for (int k = threadIdx.x; k < K; k += AUG_T) {
        cnt[k] = 0;
        crop_offset(r, fs, k, so[k], sf[k]);
    }
    __syncthreads();
    double mn[3];
    for (int a = 0; a < 3; a++) mn[a] = dkey_inv((unsigned long long)r[GF_AUG_R_MIN + a]);
    for (long long p = off[y] + blockIdx.x * AUG_T + threadIdx.x; p < off[y + 1]; p += (long long)gridDim.x * AUG_T) {
        double x[3];
        for (int a = 0; a < 3; a++) x[a] = xyz[p * 3 + a] - mn[a];
        for (int k = 0; k < K; k++) {
            bool v = true;
            for (int a = 0; a < 3; a++) {
                const double xo = x[a] + so[k][a];
                v = v && xo >= 0.0 && xo < sf[k][a];
            }
            if (v) atomicAdd(&cnt[k], 1);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += AUG_T)
        if (cnt[k]) atomicAdd((unsigned long long*)&r[GF_AUG_R_COUNTS + k], (unsigned long long)cnt[k]);
}

// the first candidate that keeps at most max_npoint points (the reference's loop stops there); -1: no crop
__global__ void k_crop_choose(const long long* __restrict__ off, long long* rec, int ns, int K, long long max_npoint) {
    const int y = blockIdx.x * blockDim.x + threadIdx.x;
    if (y >= ns) return;
    long long* r = rec_of(rec, y);
    long long chosen = -1;
    if (off[y + 1] - off[y] > max_npoint) {
        chosen = K - 1;
        for (int k = 0; k < K; k++)
            if (r[GF_AUG_R_COUNTS + k] <= max_npoint) {
                chosen = k;
                break;
            }
    }
    r[GF_AUG_R_CHOSEN] = chosen;
}

// ======================= collate =======================
struct LabelLut {
    signed char v[GF_AUG_LUT];  // new label of raw labels 0 .. GF_AUG_LUT-1
};

// fs_mode 0: label through the fold LUT, instances of labels <= 3 dropped; 1: label = (raw label == the scene's
// sampled class), instances of label 0 dropped (datasets/scannetv2_fs_inst.py:433-434)
__global__ __launch_bounds__(AUG_T) void k_keep(GfAugBatch bt, int fs, LabelLut lut, int fs_mode) {
    const int y = blockIdx.y;
    long long* r = rec_of(bt.rec, y);
    const long long chosen = r[GF_AUG_R_CHOSEN];
    const long long cls = r[GF_AUG_R_CLASS];
    double mn[3], o[3] = {0.0, 0.0, 0.0}, fk[3] = {0.0, 0.0, 0.0};
    for (int a = 0; a < 3; a++) mn[a] = dkey_inv((unsigned long long)r[GF_AUG_R_MIN + a]);
    if (chosen >= 0) crop_offset(r, fs, (int)chosen, o, fk);
    uint32_t* bits = bt.bitmap + (size_t)y * (bt.max_inst / 32);
    int err = 0;
    for (long long p = bt.raw_off[y] + blockIdx.x * AUG_T + threadIdx.x; p < bt.raw_off[y + 1];
         p += (long long)gridDim.x * AUG_T) {
        bool keep = true;
        for (int a = 0; a < 3; a++) {
            double xo = bt.xyz[p * 3 + a] - mn[a];
            if (chosen >= 0) {
                xo = xo + o[a];
                keep = keep && xo >= 0.0 && xo < fk[a];
            }
            bt.xyz[p * 3 + a] = xo;  // the cropped coordinate (what .long() of the collate truncates)
        }
        const long long lab = (long long)bt.raw[p * 8 + 6];
        long long ins = (long long)bt.raw[p * 8 + 7];
        int nl;
        if (fs_mode) {
            nl = lab == cls ? 1 : 0;
            if (nl == 0) ins = -100;
        } else {
            nl = lab == -100 ? 2 : (lab >= 0 && lab < GF_AUG_LUT ? lut.v[lab] : 3);
            if (nl <= 3) ins = -100;
        }
        if (ins != -100 && (ins < 0 || ins >= bt.max_inst)) {
            err |= GF_AUG_ERR_INST;
            ins = -100;
        }
        bt.flags[p] = keep ? 1 : 0;
        bt.lab[p] = nl;
        bt.inst[p] = (int32_t)ins;
        if (keep && ins >= 0) atomicOr(&bits[ins >> 5], 1u << (ins & 31));
    }
    if (err) atomicOr((unsigned long long*)&r[GF_AUG_R_ERR], (unsigned long long)err);
}

// getCroppedInstLabel (datasets/scannetv2_inst.py:224-232) on the set of present ids, one block: with n ids present
// the result is {0..n-1}; ids below n keep their value, the largest id fills the lowest hole, the next largest the next
// hole, ...  Then per scene: instance count, running instance base (the scene's first slot of instance_pointnum; also
// the offset of its instance ids, except with fs_mode, whose ids stay scene-local: datasets/scannetv2_fs_inst.py:442
// adds total_inst_num, which is never updated), batch offsets, kept total.
__global__ __launch_bounds__(SCAN_THREADS) void k_relabel(GfAugBatch bt, int fs_mode) {
    __shared__ int holes[GF_AUG_MAX_INST];
    const int per = bt.max_inst / SCAN_THREADS;  // ids per thread (max_inst is a multiple of 32 * SCAN_THREADS / 32)
    long long ibase = 0;
    int err = 0;
    for (int s = 0; s < bt.B; s++) {
        long long* r = rec_of(bt.rec, s);
        const uint32_t* bits = bt.bitmap + (size_t)s * (bt.max_inst / 32);
        const int lo = threadIdx.x * per;
        int mine = 0;
        for (int i = 0; i < per; i++) mine += (bits[(lo + i) >> 5] >> ((lo + i) & 31)) & 1;
        int n;
        const int before = block_excl_scan(mine, &n);
        int rank = before;  // present ids below lo + i
        for (int i = 0; i < per; i++) {
            const int q = lo + i;
            const bool pres = (bits[q >> 5] >> (q & 31)) & 1;
            if (!pres && q < n) holes[q - rank] = q;
            rank += pres;
        }
        __syncthreads();
        rank = before;
        int32_t* map = bt.inst_map + (size_t)s * bt.max_inst;
        for (int i = 0; i < per; i++) {
            const int q = lo + i;
            const bool pres = (bits[q >> 5] >> (q & 31)) & 1;
            map[q] = !pres ? -1 : (q < n ? q : holes[n - 1 - rank]);
            rank += pres;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            r[GF_AUG_R_NINST] = n;
            r[GF_AUG_R_IBASE] = fs_mode ? 0 : ibase;
            r[GF_AUG_R_PBASE] = ibase;
            bt.offsets[s] = bt.start[bt.raw_off[s]];
            err |= (int)r[GF_AUG_R_ERR];
        }
        ibase += n;
    }
    if (threadIdx.x == 0) {
        bt.offsets[bt.B] = bt.start[bt.n_raw];
        bt.head[GF_AUG_H_N] = bt.start[bt.n_raw];
        bt.head[GF_AUG_H_NINST] = (int32_t)ibase;
        bt.head[GF_AUG_H_ERR] = err;
    }
}

// fs_mode: raw colours (no shift drawn) and only the instance counts (no instance_infos)
__global__ __launch_bounds__(AUG_T) void k_collate(GfAugBatch bt, int fs_mode) {
    const int y = blockIdx.y;
    const long long* r = rec_of(bt.rec, y);
    const long long ibase = r[GF_AUG_R_IBASE];
    double shift[3];
    for (int a = 0; a < 3; a++) shift[a] = fs_mode ? 0.0 : rec_d(r, GF_AUG_R_SHIFT + a);
    const int32_t* map = bt.inst_map + (size_t)y * bt.max_inst;
    long long* st = bt.inst_stats + (size_t)y * bt.max_inst * GF_AUG_STAT;
    double pmn[3] = {INFINITY, INFINITY, INFINITY}, pmx[3] = {-INFINITY, -INFINITY, -INFINITY};
    long long lmax[3] = {0, 0, 0};
    for (long long p = bt.raw_off[y] + blockIdx.x * AUG_T + threadIdx.x; p < bt.raw_off[y + 1];
         p += (long long)gridDim.x * AUG_T) {
        if (!bt.flags[p]) continue;
        const long long q = bt.start[p];
        bt.locs[q * 4] = y;
        double xm[3];
        for (int a = 0; a < 3; a++) {
            const long long l = (long long)bt.xyz[p * 3 + a];
            bt.locs[q * 4 + 1 + a] = l;
            lmax[a] = l > lmax[a] ? l : lmax[a];
            xm[a] = bt.xyz_middle[p * 3 + a];
            bt.locs_float[q * 3 + a] = (float)xm[a];
            bt.feats[q * 3 + a] = fs_mode ? bt.raw[p * 8 + 3 + a] : bt.raw[p * 8 + 3 + a] + shift[a];
            pmn[a] = fmin(pmn[a], xm[a]);
            pmx[a] = fmax(pmx[a], xm[a]);
        }
        bt.labels[q] = bt.lab[p];
        const int ins = bt.inst[p];
        if (ins >= 0) {
            const int l = map[ins];
            bt.instance_labels[q] = ibase + l;
            bt.sidx[q] = y * bt.max_inst + l;
            long long* sl = st + (size_t)l * GF_AUG_STAT;
            atomicAdd((unsigned long long*)&sl[0], 1ull);
            for (int a = 0; a < 3 && !fs_mode; a++) {
                atomicAdd((unsigned long long*)&sl[1 + a], (unsigned long long)llrint(xm[a] * 4294967296.0));
                atomicMin((unsigned long long*)&sl[4 + a], dkey(xm[a]));
                atomicMax((unsigned long long*)&sl[7 + a], dkey(xm[a]));
            }
        } else {
            bt.instance_labels[q] = -100;
            bt.sidx[q] = -1;
        }
    }
    long long* rr = rec_of(bt.rec, y);
    for (int a = 0; a < 3; a++) {
        const double mn = wave_min_d(pmn[a]), mx = wave_max_d(pmx[a]);
        const long long lm = wave_max_ll(lmax[a]);
        if ((threadIdx.x & 63) == 0 && mn <= mx) {
            atomicMin((unsigned long long*)&rr[GF_AUG_R_PCMIN + a], dkey(mn));
            atomicMax((unsigned long long*)&rr[GF_AUG_R_PCMAX + a], dkey(mx));
            atomicMax(&bt.head[GF_AUG_H_LMAX + a], (int)lm);
        }
    }
}

__device__ __forceinline__ void instance_info_row(const GfAugBatch& bt, long long q) {
    const int si = bt.sidx[q];
    float* o = bt.instance_infos + q * 9;
    if (si < 0) {
        for (int i = 0; i < 9; i++) o[i] = -100.0f;
    } else {
        const long long* sl = bt.inst_stats + (size_t)si * GF_AUG_STAT;
        const double n = (double)sl[0];
        for (int a = 0; a < 3; a++) {
            o[a] = (float)((double)sl[1 + a] * 2.3283064365386963e-10 / n);
            o[3 + a] = (float)dkey_inv((unsigned long long)sl[4 + a]);
            o[6 + a] = (float)dkey_inv((unsigned long long)sl[7 + a]);
        }
    }
}

// per kept row: the [9] instance record; rows past the kept count: distinct padding coordinates (batch 0xffff) that
// voxelise into one voxel each, behind every real voxel; per instance: its point count; per scene: pc_mins / pc_maxs;
// the spatial shape
__global__ __launch_bounds__(AUG_T) void k_finish(GfAugBatch bt, int fs_min, int fs_mode) {
    const long long N = bt.head[GF_AUG_H_N];
    const long long q = (long long)blockIdx.x * AUG_T + threadIdx.x;
    if (q < N) {
        if (!fs_mode) instance_info_row(bt, q);  // (few-shot queries have no instance_infos)
    } else if (q < bt.n_raw) {
        const long long j = q - N;
        bt.locs[q * 4 + 0] = 0xffff;
        bt.locs[q * 4 + 1] = j & 0xffff;
        bt.locs[q * 4 + 2] = (j >> 16) & 0xffff;
        bt.locs[q * 4 + 3] = 0;
    }
    if (q < (long long)bt.B * bt.max_inst) {
        const int s = (int)(q / bt.max_inst), l = (int)(q % bt.max_inst);
        const long long* r = rec_of(bt.rec, s);
        if (l < r[GF_AUG_R_NINST])
            bt.instance_pointnum[r[GF_AUG_R_PBASE] + l] = (int32_t)bt.inst_stats[(size_t)q * GF_AUG_STAT];
    }
    if (q < (long long)bt.B * 3) {
        const int s = (int)(q / 3), a = (int)(q % 3);
        const long long* r = rec_of(bt.rec, s);
        bt.pc_mins[q] = (float)dkey_inv((unsigned long long)r[GF_AUG_R_PCMIN + a]);
        bt.pc_maxs[q] = (float)dkey_inv((unsigned long long)r[GF_AUG_R_PCMAX + a]);
    }
    if (q < 3) {
        const int e = bt.head[GF_AUG_H_LMAX + q] + 1;
        bt.head[GF_AUG_H_SHAPE + q] = e > fs_min ? e : fs_min;
    }
}

__global__ void k_stats_init(long long* st, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int f = (int)(i % GF_AUG_STAT);
    st[i] = (f >= 4 && f < 7) ? (long long)~0ull : 0;  // count, sums: 0; min keys: largest; max keys: 0 (smallest)
}

// ======================= few-shot support scenes (load_single(aug=False, support=True)) =======================
// per scene: the min of xyz_origin * scale (the offset of locs) and the min / max of xyz_origin (pc_mins / pc_maxs)
// (keep: the test-time block supports' in-box flags, NULL: every point)
__global__ __launch_bounds__(AUG_T) void k_sup_extent(GfAugBatch bt, double scale, const int32_t* __restrict__ keep) {
    const int y = blockIdx.y;
    long long* r = rec_of(bt.rec, y);
    double smn[3] = {INFINITY, INFINITY, INFINITY}, mn[3] = {INFINITY, INFINITY, INFINITY},
           mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long long p = bt.raw_off[y] + blockIdx.x * AUG_T + threadIdx.x; p < bt.raw_off[y + 1];
         p += (long long)gridDim.x * AUG_T) {
        if (keep && !keep[p]) continue;
        for (int a = 0; a < 3; a++) {
            const double x = bt.raw[p * 8 + a];
            smn[a] = fmin(smn[a], x * scale);
            mn[a] = fmin(mn[a], x);
            mx[a] = fmax(mx[a], x);
        }
    }
    for (int a = 0; a < 3; a++) {
        const double s = wave_min_d(smn[a]), lo = wave_min_d(mn[a]), hi = wave_max_d(mx[a]);
        if ((threadIdx.x & 63) == 0 && lo <= hi) {
            atomicMin((unsigned long long*)&r[GF_AUG_R_MIN + a], dkey(s));
            atomicMin((unsigned long long*)&r[GF_AUG_R_PCMIN + a], dkey(lo));
            atomicMax((unsigned long long*)&r[GF_AUG_R_PCMAX + a], dkey(hi));
        }
    }
}

// every point is kept, row = raw row: locs (scene, xyz_origin * scale - min truncated), locs_float, raw colours, the
// mask of the scene's support instance id (masks != NULL) or the raw semantic label (the few-shot test query,
// labels != NULL); the max locs for the spatial shape
__global__ __launch_bounds__(AUG_T) void k_sup_collate(GfAugBatch bt, long long* __restrict__ masks,
                                                       long long* __restrict__ labels, double scale) {
    const int y = blockIdx.y;
    const long long* r = rec_of(bt.rec, y);
    const long long id = r[GF_AUG_R_SUPID];
    double mn[3];
    for (int a = 0; a < 3; a++) mn[a] = dkey_inv((unsigned long long)r[GF_AUG_R_MIN + a]);
    long long lmax[3] = {0, 0, 0};
    for (long long p = bt.raw_off[y] + blockIdx.x * AUG_T + threadIdx.x; p < bt.raw_off[y + 1];
         p += (long long)gridDim.x * AUG_T) {
        bt.locs[p * 4] = y;
        for (int a = 0; a < 3; a++) {
            const double x = bt.raw[p * 8 + a];
            const long long l = (long long)(x * scale - mn[a]);
            bt.locs[p * 4 + 1 + a] = l;
            lmax[a] = l > lmax[a] ? l : lmax[a];
            bt.locs_float[p * 3 + a] = (float)x;
            bt.feats[p * 3 + a] = bt.raw[p * 8 + 3 + a];
        }
        if (masks) masks[p] = (long long)bt.raw[p * 8 + 7] == id ? 1 : 0;
        if (labels) labels[p] = (long long)bt.raw[p * 8 + 6];
    }
    for (int a = 0; a < 3; a++) {
        const long long lm = wave_max_ll(lmax[a]);
        if ((threadIdx.x & 63) == 0) atomicMax(&bt.head[GF_AUG_H_LMAX + a], (int)lm);
    }
}

// batch offsets (the raw ones), pc_mins / pc_maxs, spatial shape, head: N = n_raw, no instances, no padding rows
__global__ __launch_bounds__(AUG_T) void k_sup_finish(GfAugBatch bt, int fs_min) {
    const long long q = (long long)blockIdx.x * AUG_T + threadIdx.x;
    if (q <= bt.B) bt.offsets[q] = (int32_t)bt.raw_off[q];
    if (q < (long long)bt.B * 3) {
        const int s = (int)(q / 3), a = (int)(q % 3);
        const long long* r = rec_of(bt.rec, s);
        bt.pc_mins[q] = (float)dkey_inv((unsigned long long)r[GF_AUG_R_PCMIN + a]);
        bt.pc_maxs[q] = (float)dkey_inv((unsigned long long)r[GF_AUG_R_PCMAX + a]);
    }
    if (q < 3) {
        const int e = bt.head[GF_AUG_H_LMAX + q] + 1;
        bt.head[GF_AUG_H_SHAPE + q] = e > fs_min ? e : fs_min;
    }
    if (q == 0) bt.head[GF_AUG_H_N] = bt.n_raw;
}

// ======================= few-shot test-time block supports (load_single_block, get_region_inst) =======================
// datasets/scannetv2_fs_inst.py:277-309 and 365-395 with scale_factor 1, no augmentation, no permutation.  One batch holds
// B (scene, instance id) pairs; the kept points of scene y are compacted in order to the front of its own raw range
// (rows raw_off[y] ..), the rest of the range holds padding coordinates, so every scene voxelises on its own.

// per scene: the fp64 min / max of the support instance's points and their count
__global__ __launch_bounds__(AUG_T) void k_blk_inst(GfAugBatch bt) {
    const int y = blockIdx.y;
    long long* r = rec_of(bt.rec, y);
    const long long id = r[GF_AUG_R_SUPID];
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    long long cnt = 0;
    for (long long p = bt.raw_off[y] + blockIdx.x * AUG_T + threadIdx.x; p < bt.raw_off[y + 1];
         p += (long long)gridDim.x * AUG_T) {
        if ((long long)bt.raw[p * 8 + 7] != id) continue;
        cnt++;
        for (int a = 0; a < 3; a++) {
            const double x = bt.raw[p * 8 + a];
            mn[a] = fmin(mn[a], x);
            mx[a] = fmax(mx[a], x);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
    for (int a = 0; a < 3; a++) {
        const double lo = wave_min_d(mn[a]), hi = wave_max_d(mx[a]);
        if ((threadIdx.x & 63) == 0 && lo <= hi) {
            atomicMin((unsigned long long*)&r[GF_AUG_R_BMIN + a], dkey(lo));
            atomicMax((unsigned long long*)&r[GF_AUG_R_BMAX + a], dkey(hi));
        }
    }
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd((unsigned long long*)&r[GF_AUG_R_BCNT], (unsigned long long)cnt);
}

// the box test of get_region_inst: middle = (min + max) / 2, size = max - min + 0.1, kept when
// middle - size * 0.5 <= x <= middle + size * 0.5 on every axis (numpy's operation order, fp64); a scene whose instance
// id has no point keeps nothing and sets GF_AUG_ERR_NOINST
__global__ __launch_bounds__(AUG_T) void k_blk_flags(GfAugBatch bt) {
    const int y = blockIdx.y;
    long long* r = rec_of(bt.rec, y);
    const bool any = r[GF_AUG_R_BCNT] > 0;
    double lower[3], upper[3];
    for (int a = 0; a < 3; a++) {
        const double lo = dkey_inv((unsigned long long)r[GF_AUG_R_BMIN + a]);
        const double hi = dkey_inv((unsigned long long)r[GF_AUG_R_BMAX + a]);
        const double middle = (lo + hi) / 2.0;
        const double size = hi - lo + 0.1;
        lower[a] = middle - size * 0.5;
        upper[a] = middle + size * 0.5;
    }
    if (!any && blockIdx.x == 0 && threadIdx.x == 0)
        atomicOr((unsigned long long*)&r[GF_AUG_R_ERR], (unsigned long long)GF_AUG_ERR_NOINST);
    for (long long p = bt.raw_off[y] + blockIdx.x * AUG_T + threadIdx.x; p < bt.raw_off[y + 1];
         p += (long long)gridDim.x * AUG_T) {
        bool keep = any;
        for (int a = 0; a < 3; a++) {
            const double x = bt.raw[p * 8 + a];
            keep = keep && x <= upper[a] && x >= lower[a];
        }
        bt.flags[p] = keep ? 1 : 0;
    }
}

// kept point p of scene y -> row raw_off[y] + (its rank among the scene's kept points): locs (0, trunc(x * scale -
// min)), locs_float, raw colours, the mask of the instance id; the scene's max locs
__global__ __launch_bounds__(AUG_T) void k_blk_collate(GfAugBatch bt, long long* __restrict__ masks, double scale) {
    const int y = blockIdx.y;
    long long* r = rec_of(bt.rec, y);
    const long long id = r[GF_AUG_R_SUPID];
    const long long base = bt.raw_off[y], first = bt.start[base];
    double mn[3];
    for (int a = 0; a < 3; a++) mn[a] = dkey_inv((unsigned long long)r[GF_AUG_R_MIN + a]);
    long long lmax[3] = {0, 0, 0};
    for (long long p = base + blockIdx.x * AUG_T + threadIdx.x; p < bt.raw_off[y + 1];
         p += (long long)gridDim.x * AUG_T) {
        if (!bt.flags[p]) continue;
        const long long q = base + (bt.start[p] - first);
        bt.locs[q * 4] = 0;
        for (int a = 0; a < 3; a++) {
            const double x = bt.raw[p * 8 + a];
            const long long l = (long long)(x * scale - mn[a]);
            bt.locs[q * 4 + 1 + a] = l;
            lmax[a] = l > lmax[a] ? l : lmax[a];
            bt.locs_float[q * 3 + a] = (float)x;
            bt.feats[q * 3 + a] = bt.raw[p * 8 + 3 + a];
        }
        masks[q] = (long long)bt.raw[p * 8 + 7] == id ? 1 : 0;
    }
    for (int a = 0; a < 3; a++) {
        const long long lm = wave_max_ll(lmax[a]);
        if ((threadIdx.x & 63) == 0 && lm > 0) atomicMax((unsigned long long*)&r[GF_AUG_R_BLMAX + a], (unsigned long long)lm);
    }
}

// padding rows behind each scene's kept points (batch 0xffff, distinct, one voxel each behind the real ones); per scene
// sizes[y] = (kept, instance points, spatial shape); offsets = the kept points' running offsets; head N, error bits
__global__ __launch_bounds__(AUG_T) void k_blk_finish(GfAugBatch bt, int32_t* __restrict__ sizes, int fs_min) {
    const int y = blockIdx.y;
    const long long* r = rec_of(bt.rec, y);
    const long long base = bt.raw_off[y], end = bt.raw_off[y + 1];
    const long long kept = bt.start[end] - bt.start[base];
    for (long long q = base + kept + blockIdx.x * AUG_T + threadIdx.x; q < end; q += (long long)gridDim.x * AUG_T) {
        const long long j = q - (base + kept);
        bt.locs[q * 4 + 0] = 0xffff;
        bt.locs[q * 4 + 1] = j & 0xffff;
        bt.locs[q * 4 + 2] = (j >> 16) & 0xffff;
        bt.locs[q * 4 + 3] = 0;
    }
    if (blockIdx.x != 0) return;
    if (threadIdx.x == 0) {
        sizes[y * 5 + 0] = (int32_t)kept;
        sizes[y * 5 + 1] = (int32_t)r[GF_AUG_R_BCNT];
        bt.offsets[y] = bt.start[base];
        if (y == bt.B - 1) {
            bt.offsets[bt.B] = bt.start[bt.n_raw];
            bt.head[GF_AUG_H_N] = bt.start[bt.n_raw];
        }
        if (r[GF_AUG_R_ERR]) atomicOr(&bt.head[GF_AUG_H_ERR], (int)r[GF_AUG_R_ERR]);
    }
    if (threadIdx.x < 3) {
        const int e = (int)r[GF_AUG_R_BLMAX + threadIdx.x] + 1;
        sizes[y * 5 + 2 + threadIdx.x] = e > fs_min ? e : fs_min;
    }
}

int grid_x(int max_scene_points) {
    const int g = gf_div_up(max_scene_points > 0 ? max_scene_points : 1, AUG_T * 4);
    return g < 1 ? 1 : (g > 512 ? 512 : g);
}
int grid_cells_x(long long max_cells) {
    const long long g = (max_cells + AUG_T * 4 - 1) / (AUG_T * 4);
    return g < 1 ? 1 : (g > 512 ? 512 : (int)g);
}

GfAugBatch shifted(const GfAugBatch* b, int s0) {  // the record and point offsets of scenes s0.. (rng="reference")
    GfAugBatch t = *b;
    t.rec = b->rec + (size_t)s0 * GF_AUG_REC;
    t.raw_off = b->raw_off + s0;
    return t;
}

}  // namespace

extern "C" int gf_aug_scan_blocks(int n_raw) { return gf_iscan_blocks(n_raw > 0 ? n_raw : 1); }

extern "C" int gf_aug_draw(const GfAugBatch* b, unsigned long long seed, long long batch_index, int K, void* stream) {
    GF_CHECK_ARG(b && b->B > 0 && K >= 1 && K <= GF_AUG_MAX_CROP, "gf_aug_draw: bad arguments (K=%d)", K);
    hipLaunchKernelGGL(k_draw, dim3(gf_div_up(b->B, 64)), dim3(64), 0, (hipStream_t)stream, b->rec, b->B, K, seed,
                       batch_index);
    GF_CHECK_LAUNCH("gf_aug_draw");
    return GF_OK;
}

extern "C" int gf_aug_transform(const GfAugBatch* b, int s0, int ns, double scale, int max_scene_points, void* stream) {
    GF_CHECK_ARG(b && s0 >= 0 && ns >= 1 && s0 + ns <= b->B, "gf_aug_transform: scenes [%d, %d)", s0, s0 + ns);
    const GfAugBatch t = shifted(b, s0);
    hipLaunchKernelGGL(k_transform, dim3(grid_x(max_scene_points), ns), dim3(AUG_T), 0, (hipStream_t)stream, t.raw,
                       t.raw_off, t.rec, t.xyz_middle, t.xyz, scale);
    GF_CHECK_LAUNCH("gf_aug_transform");
    return GF_OK;
}

extern "C" int gf_aug_elastic(const GfAugBatch* b, int s0, int ns, int pass, int gran, double mag, int fill,
                              unsigned long long seed, long long batch_index, int max_scene_points, long long max_cells,
                              void* stream) {
    GF_CHECK_ARG(b && s0 >= 0 && ns >= 1 && s0 + ns <= b->B && (pass == 0 || pass == 1) && gran >= 1,
                 "gf_aug_elastic: bad arguments (scenes [%d, %d), pass %d, gran %d)", s0, s0 + ns, pass, gran);
    hipStream_t st = (hipStream_t)stream;
    const GfAugBatch t = shifted(b, s0);
    float* raw = t.noise[pass];
    float* w0 = t.work[pass];
    float* w1 = t.work[pass] + t.cells[pass];
    const dim3 gc(grid_cells_x(max_cells), ns, 3);
    if (fill) hipLaunchKernelGGL(k_noise, gc, dim3(AUG_T), 0, st, t.rec, s0, pass, gran, raw, seed, batch_index);
    // axes 0, 1, 2, 0, 1, 2 (datasets/scannetv2_inst.py:150-155): raw -> w0 -> w1 -> w0 -> w1 -> w0 -> w1
    const float* src = raw;
    for (int i = 0; i < 6; i++) {
        float* dst = (i & 1) ? w1 : w0;
        hipLaunchKernelGGL(k_blur, gc, dim3(AUG_T), 0, st, t.rec, pass, gran, i % 3, src, dst);
        src = dst;
    }
    hipLaunchKernelGGL(k_displace, dim3(grid_x(max_scene_points), ns), dim3(AUG_T), 0, st, t.raw_off, t.rec, pass, gran,
                       mag, w1, t.xyz);
    GF_CHECK_LAUNCH("gf_aug_elastic");
    return GF_OK;
}

extern "C" int gf_aug_crop(const GfAugBatch* b, int s0, int ns, int full_scale, int K, long long max_npoint,
                           int max_scene_points, void* stream) {
    GF_CHECK_ARG(b && s0 >= 0 && ns >= 1 && s0 + ns <= b->B && K >= 1 && K <= GF_AUG_MAX_CROP,
                 "gf_aug_crop: bad arguments (scenes [%d, %d), K %d)", s0, s0 + ns, K);
    hipStream_t st = (hipStream_t)stream;
    const GfAugBatch t = shifted(b, s0);
    hipLaunchKernelGGL(k_crop_count, dim3(grid_x(max_scene_points), ns), dim3(AUG_T), 0, st, t.raw_off, t.rec,
                       full_scale, K, max_npoint, t.xyz);
    hipLaunchKernelGGL(k_crop_choose, dim3(gf_div_up(ns, 64)), dim3(64), 0, st, t.raw_off, t.rec, ns, K, max_npoint);
    GF_CHECK_LAUNCH("gf_aug_crop");
    return GF_OK;
}

namespace {

int collate_impl(const GfAugBatch* b, const LabelLut& lut, int fs_mode, int full_scale_min, int full_scale,
                 int max_scene_points, hipStream_t st) {
    const long long nstat = (long long)b->B * b->max_inst * GF_AUG_STAT;
    GF_TRY(hipMemsetAsync(b->bitmap, 0, (size_t)b->B * (b->max_inst / 32) * 4, st));
    GF_TRY(hipMemsetAsync(b->head, 0, GF_AUG_HEAD * 4, st));
    hipLaunchKernelGGL(k_stats_init, dim3(gf_div_up(nstat, 256)), dim3(256), 0, st, b->inst_stats, nstat);
    const dim3 gp(grid_x(max_scene_points), b->B);
    hipLaunchKernelGGL(k_keep, gp, dim3(AUG_T), 0, st, *b, full_scale, lut, fs_mode);
    if (b->n_raw > 0) {
        gf_iscan(b->flags, b->n_raw, b->start, b->cursor, b->block_sums, b->block_off, st);
    } else {
        GF_TRY(hipMemsetAsync(b->start, 0, 4, st));
    }
    hipLaunchKernelGGL(k_relabel, dim3(1), dim3(SCAN_THREADS), 0, st, *b, fs_mode);
    hipLaunchKernelGGL(k_collate, gp, dim3(AUG_T), 0, st, *b, fs_mode);
    long long nq = b->n_raw;
    if (nq < (long long)b->B * b->max_inst) nq = (long long)b->B * b->max_inst;
    hipLaunchKernelGGL(k_finish, dim3(gf_div_up(nq > 3 ? nq : 3, AUG_T)), dim3(AUG_T), 0, st, *b, full_scale_min,
                       fs_mode);
    return GF_OK;
}

bool collate_args_ok(const GfAugBatch* b) {
    return b && b->B > 0 && b->n_raw >= 0 && b->max_inst > 0 && b->max_inst <= GF_AUG_MAX_INST &&
           b->max_inst % SCAN_THREADS == 0;
}

}  // namespace

extern "C" int gf_aug_collate(const GfAugBatch* b, const int32_t* fold_classes, int n_fold, int full_scale_min,
                              int full_scale, int max_scene_points, void* stream) {
    GF_CHECK_ARG(collate_args_ok(b) && fold_classes && n_fold >= 0,
                 "gf_aug_collate: bad arguments (B %d, n_raw %d, max_inst %d)", b ? b->B : 0, b ? b->n_raw : 0,
                 b ? b->max_inst : 0);
    LabelLut lut;  // datasets/scannetv2_inst.py:314-324: 0 -> 0, 1 -> 1, fold class i -> i + 4, -100 -> 2, else 3
    for (int i = 0; i < GF_AUG_LUT; i++) lut.v[i] = 3;
    lut.v[0] = 0;
    lut.v[1] = 1;
    for (int i = 0; i < n_fold; i++) {
        GF_CHECK_ARG(fold_classes[i] >= 0 && fold_classes[i] < GF_AUG_LUT && i + 4 < 127, "gf_aug_collate: fold class");
        lut.v[fold_classes[i]] = (signed char)(i + 4);
    }
    const int rc = collate_impl(b, lut, 0, full_scale_min, full_scale, max_scene_points, (hipStream_t)stream);
    if (rc != GF_OK) return rc;
    GF_CHECK_LAUNCH("gf_aug_collate");
    return GF_OK;
}

extern "C" int gf_aug_collate_fs(const GfAugBatch* b, int full_scale_min, int full_scale, int max_scene_points,
                                 void* stream) {
    GF_CHECK_ARG(collate_args_ok(b), "gf_aug_collate_fs: bad arguments (B %d, n_raw %d, max_inst %d)", b ? b->B : 0,
                 b ? b->n_raw : 0, b ? b->max_inst : 0);
    LabelLut unused;
    for (int i = 0; i < GF_AUG_LUT; i++) unused.v[i] = 0;
    const int rc = collate_impl(b, unused, 1, full_scale_min, full_scale, max_scene_points, (hipStream_t)stream);
    if (rc != GF_OK) return rc;
    GF_CHECK_LAUNCH("gf_aug_collate_fs");
    return GF_OK;
}

extern "C" int gf_aug_support(const GfAugBatch* b, long long* support_masks, double scale, int full_scale_min,
                              int max_scene_points, void* stream) {
    GF_CHECK_ARG(b && b->B > 0 && b->n_raw >= 0 && support_masks, "gf_aug_support: bad arguments (B %d, n_raw %d)",
                 b ? b->B : 0, b ? b->n_raw : 0);
    hipStream_t st = (hipStream_t)stream;
    GF_TRY(hipMemsetAsync(b->head, 0, GF_AUG_HEAD * 4, st));
    const dim3 gp(grid_x(max_scene_points), b->B);
    hipLaunchKernelGGL(k_sup_extent, gp, dim3(AUG_T), 0, st, *b, scale, (const int32_t*)nullptr);
    hipLaunchKernelGGL(k_sup_collate, gp, dim3(AUG_T), 0, st, *b, support_masks, (long long*)nullptr, scale);
    const int nq = 3 * b->B + 1;
    hipLaunchKernelGGL(k_sup_finish, dim3(gf_div_up(nq, AUG_T)), dim3(AUG_T), 0, st, *b, full_scale_min);
    GF_CHECK_LAUNCH("gf_aug_support");
    return GF_OK;
}

extern "C" int gf_aug_test_query(const GfAugBatch* b, double scale, int full_scale_min, int max_scene_points,
                                 void* stream) {
    GF_CHECK_ARG(b && b->B > 0 && b->n_raw >= 0 && b->labels, "gf_aug_test_query: bad arguments (B %d, n_raw %d)",
                 b ? b->B : 0, b ? b->n_raw : 0);
    hipStream_t st = (hipStream_t)stream;
    GF_TRY(hipMemsetAsync(b->head, 0, GF_AUG_HEAD * 4, st));
    const dim3 gp(grid_x(max_scene_points), b->B);
    hipLaunchKernelGGL(k_sup_extent, gp, dim3(AUG_T), 0, st, *b, scale, (const int32_t*)nullptr);
    hipLaunchKernelGGL(k_sup_collate, gp, dim3(AUG_T), 0, st, *b, (long long*)nullptr, b->labels, scale);
    const int nq = 3 * b->B + 1;
    hipLaunchKernelGGL(k_sup_finish, dim3(gf_div_up(nq, AUG_T)), dim3(AUG_T), 0, st, *b, full_scale_min);
    GF_CHECK_LAUNCH("gf_aug_test_query");
    return GF_OK;
}

extern "C" int gf_aug_support_block(const GfAugBatch* b, long long* support_masks, int32_t* scene_sizes, double scale,
                                    int full_scale_min, int max_scene_points, void* stream) {
    GF_CHECK_ARG(b && b->B > 0 && b->n_raw > 0 && support_masks && scene_sizes,
                 "gf_aug_support_block: bad arguments (B %d, n_raw %d)", b ? b->B : 0, b ? b->n_raw : 0);
    hipStream_t st = (hipStream_t)stream;
    GF_TRY(hipMemsetAsync(b->head, 0, GF_AUG_HEAD * 4, st));
    const dim3 gp(grid_x(max_scene_points), b->B);
    hipLaunchKernelGGL(k_blk_inst, gp, dim3(AUG_T), 0, st, *b);
    hipLaunchKernelGGL(k_blk_flags, gp, dim3(AUG_T), 0, st, *b);
    gf_iscan(b->flags, b->n_raw, b->start, b->cursor, b->block_sums, b->block_off, st);
    hipLaunchKernelGGL(k_sup_extent, gp, dim3(AUG_T), 0, st, *b, scale, (const int32_t*)b->flags);
    hipLaunchKernelGGL(k_blk_collate, gp, dim3(AUG_T), 0, st, *b, support_masks, scale);
    hipLaunchKernelGGL(k_blk_finish, gp, dim3(AUG_T), 0, st, *b, scene_sizes, full_scale_min);
    GF_CHECK_LAUNCH("gf_aug_support_block");
    return GF_OK;
}
