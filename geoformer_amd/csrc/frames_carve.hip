// Free-space evidence for a map of posed depth frames: what the frames of a chunk see of a set of world
// points, and the clamped score a frames.Carver keeps per cell.  The host statement is frames.visibility_host /
// frames.CarverHost; see include/geoformer_hip.h for the arguments and every arithmetic step.
//
// A probe is one point in one frame: the point into the camera by the frame's inverse record, the pixel it falls into,
// that pixel's depth (valid by the back-projection's own rule, fs_depth_valid) against the point's, one of five
// classes.  fc_probe is the one statement of it; both launch shapes call it, so they give the same bits.
//
// gf_frames_visibility, variant 0 (per point):  one launch.  k_fc_point: a thread per point loops over the frames; a
//                         workgroup stages FC_STAGE frame records in LDS at a time; the three counts stay in registers;
//                         one plain store per output, one read-modify-write of the state per cell.  No atomics.
// gf_frames_visibility, variant 1 (per probe):  one memset of out, two launches.  k_fc_probe: a thread per (frame, point),
//                         the frame's record through uniform loads, one integer atomicAdd into out for a probe that is
//                         seen, free or occluded; k_fc_finish: a thread per point does the clamp update from out.
//
// A depth pixel is read only after its (j, i) has passed the bounds test against (H, W); the neighbours of the edge
// filter only when they are inside the image.  No thread waits for another thread or workgroup (the barriers of
// k_fc_point order a workgroup's own LDS writes and reads; every thread of the workgroup reaches each of them); integer
// atomics only; nothing is read back.
#include "common.h"
#include "frames_steps.h"

namespace {

constexpr int FC_STAGE = 16;        // frame records one workgroup of k_fc_point holds in LDS at a time
constexpr int FC_RECORD = 16;       // {fx, fy, cx, cy, inv[9], t[3]}: what a probe reads of a frame
constexpr int FC_INV = 12;          // floats of an inverse record: inv row-major, then t
constexpr int FC_MAX_ROWS = 32768;  // the most frame rows of k_fc_probe's grid: a row strides over the frames
enum { FC_OUTSIDE = 0, FC_UNKNOWN = 1, FC_OCCLUDED = 2, FC_SEEN = 3, FC_FREE = 4 };
constexpr int FC_INT_MAX = 2147483647;

struct FcImage {
    const void* depth;
    int W, H;
    float shift, near, far, edge, band, rel;
};

struct FcState {
    int32_t *seen, *free, *score;  // all three or none
    int hit, miss, floor, ceil;
};

template <class D>
__device__ __forceinline__ float fc_depth(const FcImage& im, size_t at) {
    return __fdiv_rn((float)((const D*)im.depth)[at], im.shift);
}

// the class of point x in frame f, whose record is rec[FC_RECORD]; every operation rounded on its own
template <class D, bool EDGE>
__device__ __forceinline__ int fc_probe(const FcImage& im, const float* rec, int f, float x0, float x1, float x2) {
    const float d0 = x0 - rec[13], d1 = x1 - rec[14], d2 = x2 - rec[15];
    const float* inv = rec + 4;
    const float c0 = (inv[0] * d0 + inv[1] * d1) + inv[2] * d2;
    const float c1 = (inv[3] * d0 + inv[4] * d1) + inv[5] * d2;
    const float zc = (inv[6] * d0 + inv[7] * d1) + inv[8] * d2;
    if (!(zc >= im.near)) return FC_OUTSIDE;
    const float u = __fdiv_rn(c0 * rec[0], zc) + rec[2];
    const float v = __fdiv_rn(c1 * rec[1], zc) + rec[3];
    const float fi = floorf(u), fj = floorf(v);
    if (!(fi >= 0.0f && fi < (float)im.W && fj >= 0.0f && fj < (float)im.H)) return FC_OUTSIDE;
    const int i = (int)fi, j = (int)fj;  // 0 <= i < W, 0 <= j < H: exact
    const size_t at = ((size_t)f * im.H + j) * im.W + i;
    float z;
    if (!fs_depth_valid<EDGE>([&](size_t a) { return fc_depth<D>(im, a); }, at, i, j, im.W, im.H, im.near, im.far, im.edge, &z))
        return FC_UNKNOWN;
    const float tol = im.rel * z + im.band;
    if (zc < z - tol) return FC_FREE;
    if (zc > z + tol) return FC_OCCLUDED;
    return FC_SEEN;
}

// one clamp per cell per call, in 64-bit integers: |hit s - miss f| < 2^31 2^16
__device__ __forceinline__ void fc_update(const FcState& st, int p, int s, int f) {
    const i64 ns = (i64)st.seen[p] + s, nf = (i64)st.free[p] + f;
    st.seen[p] = (int32_t)(ns < FC_INT_MAX ? ns : FC_INT_MAX);
    st.free[p] = (int32_t)(nf < FC_INT_MAX ? nf : FC_INT_MAX);
    i64 sc = (i64)st.score[p] + (i64)st.hit * s - (i64)st.miss * f;
    sc = sc > st.floor ? sc : st.floor;
    sc = sc < st.ceil ? sc : st.ceil;
    st.score[p] = (int32_t)sc;
}

// record f of the two tables as a probe reads it
__device__ __forceinline__ void fc_record(const float* __restrict__ table, const float* __restrict__ inv, int f, int k,
                                          float* out) {
    out[k] = k < 4 ? table[(size_t)f * FS_RECORD + k] : inv[(size_t)f * FC_INV + (k - 4)];
}

template <class D, bool EDGE>
__global__ __launch_bounds__(FS_THREADS) void k_fc_point(const float* __restrict__ xyz, int n, FcImage im, int F,
                                                         const float* __restrict__ table, const float* __restrict__ inv,
                                                         int32_t* __restrict__ out, unsigned char* __restrict__ codes,
                                                         FcState st) {
    __shared__ float s_rec[FC_STAGE][FC_RECORD];
    const int p = blockIdx.x * FS_THREADS + threadIdx.x;  // n <= 2^29: fits
    const bool on = p < n;
    float x0 = 0.0f, x1 = 0.0f, x2 = 0.0f;
    if (on) x0 = xyz[(size_t)p * 3], x1 = xyz[(size_t)p * 3 + 1], x2 = xyz[(size_t)p * 3 + 2];
    int seen = 0, free = 0, occ = 0;
    for (int f0 = 0; f0 < F; f0 += FC_STAGE) {  // (every thread of the workgroup takes every round)
        const int nf = min(FC_STAGE, F - f0);
        if (threadIdx.x < nf * FC_RECORD)  // FC_STAGE FC_RECORD == FS_THREADS: one float per thread
            fc_record(table, inv, f0 + threadIdx.x / FC_RECORD, threadIdx.x % FC_RECORD, s_rec[threadIdx.x / FC_RECORD]);
        __syncthreads();
        if (on)
            for (int k = 0; k < nf; ++k) {
                const int c = fc_probe<D, EDGE>(im, s_rec[k], f0 + k, x0, x1, x2);
                seen += c == FC_SEEN;
                free += c == FC_FREE;
                occ += c == FC_OCCLUDED;
                if (codes) codes[(size_t)(f0 + k) * n + p] = (unsigned char)c;
            }
        __syncthreads();
    }
    if (!on) return;
    out[p] = seen;
    out[(size_t)n + p] = free;
    out[2 * (size_t)n + p] = occ;
    if (st.score) fc_update(st, p, seen, free);
}

template <class D, bool EDGE>
__global__ __launch_bounds__(FS_THREADS) void k_fc_probe(const float* __restrict__ xyz, int n, FcImage im, int F,
                                                         const float* __restrict__ table, const float* __restrict__ inv,
                                                         int32_t* __restrict__ out, unsigned char* __restrict__ codes) {
    const int p = blockIdx.x * FS_THREADS + threadIdx.x;
    if (p >= n) return;
    const float x0 = xyz[(size_t)p * 3], x1 = xyz[(size_t)p * 3 + 1], x2 = xyz[(size_t)p * 3 + 2];
    for (int f = blockIdx.y; f < F; f += gridDim.y) {  // f: the same for the whole workgroup
        float rec[FC_RECORD];
#pragma unroll
        for (int k = 0; k < FC_RECORD; ++k) fc_record(table, inv, f, k, rec);
        const int c = fc_probe<D, EDGE>(im, rec, f, x0, x1, x2);
        if (codes) codes[(size_t)f * n + p] = (unsigned char)c;
        if (c >= FC_OCCLUDED)  // rows of out: seen, free, occluded
            atomicAdd(&out[(size_t)(c == FC_SEEN ? 0 : c == FC_FREE ? 1 : 2) * n + p], 1);
    }
}

__global__ __launch_bounds__(FS_THREADS) void k_fc_finish(const int32_t* __restrict__ out, int n, FcState st) {
    const int p = blockIdx.x * FS_THREADS + threadIdx.x;
    if (p < n) fc_update(st, p, out[p], out[(size_t)n + p]);
}

template <class D, bool EDGE>
void fc_launch(const float* xyz, int n, const FcImage& im, int F, const float* table, const float* inv, int32_t* out,
               unsigned char* codes, const FcState& st, int variant, hipStream_t s) {
    const int g = gf_div_up(n, FS_THREADS);
    if (variant == 0) {
        hipLaunchKernelGGL((k_fc_point<D, EDGE>), dim3(g), dim3(FS_THREADS), 0, s, xyz, n, im, F, table, inv, out, codes, st);
    } else {
        hipLaunchKernelGGL((k_fc_probe<D, EDGE>), dim3(g, F < FC_MAX_ROWS ? F : FC_MAX_ROWS), dim3(FS_THREADS), 0, s, xyz, n, im,
                           F, table, inv, out, codes);
        if (st.score) hipLaunchKernelGGL(k_fc_finish, dim3(g), dim3(FS_THREADS), 0, s, out, n, st);
    }
}

bool fc_finite(float v) { return v == v && v >= -3.402823466e38f && v <= 3.402823466e38f; }

}  // namespace

static_assert(FC_STAGE * FC_RECORD == FS_THREADS, "k_fc_point stages one float per thread");

extern "C" int gf_frames_carve_stage_frames(void) { return FC_STAGE; }
extern "C" int gf_frames_carve_threads(void) { return FS_THREADS; }
extern "C" int gf_frames_carve_max_points(void) { return FS_MAX_POINTS; }
extern "C" int gf_frames_visibility_variants(void) { return 2; }

extern "C" int gf_frames_visibility(const float* xyz, int n, const void* depth, int dtype, int F, int H, int W,
                                    float depth_shift, const float* table, const float* inv, float near, float far, float edge,
                                    float band, float rel, int32_t* out, unsigned char* codes, int32_t* seen, int32_t* free,
                                    int32_t* score, int hit, int miss, int floor, int ceil, int variant, void* stream) {
    const char* who = "gf_frames_visibility";
    GF_CHECK_ARG(n >= 0 && n <= FS_MAX_POINTS && gf_resample_max_points() == FS_MAX_POINTS, "%s: n = %d points (0 to %d)", who, n,
                 FS_MAX_POINTS);
    GF_CHECK_ARG(dtype == 0 || dtype == 1, "%s: dtype = %d (0: uint16, 1: float32)", who, dtype);
    GF_CHECK_ARG(F >= 1 && F <= FS_MAX_FRAMES && H >= 1 && H <= FS_MAX_SIDE && W >= 1 && W <= FS_MAX_SIDE,
                 "%s: %d frames of %d x %d pixels (1 to %d frames, each side 1 to %d)", who, F, W, H, FS_MAX_FRAMES, FS_MAX_SIDE);
    GF_CHECK_ARG(depth_shift > 0.0f && fc_finite(depth_shift), "%s: depth_shift = %g (positive and finite)", who,
                 (double)depth_shift);
    GF_CHECK_ARG(near == near && far == far, "%s: near = %g, far = %g (numbers)", who, (double)near, (double)far);
    GF_CHECK_ARG(edge >= 0.0f && fc_finite(edge) && band >= 0.0f && fc_finite(band) && rel >= 0.0f && fc_finite(rel),
                 "%s: edge = %g, band = %g, rel = %g (each >= 0 and finite)", who, (double)edge, (double)band, (double)rel);
    GF_CHECK_ARG(variant == 0 || variant == 1, "%s: variant = %d (0: a thread per point, 1: a thread per probe)", who, variant);
    const bool any = seen || free || score, all = seen && free && score;
    GF_CHECK_ARG(any == all, "%s: seen, free and score: all three or none", who);
    GF_CHECK_ARG(!all || (hit >= 0 && miss >= 0 && floor <= ceil), "%s: hit = %d, miss = %d (each >= 0), floor = %d <= ceil = %d",
                 who, hit, miss, floor, ceil);
    GF_CHECK_ARG(!all || (seen != free && seen != score && free != score), "%s: seen, free and score overlap", who);
    if (n == 0) return GF_OK;
    GF_CHECK_ARG(xyz && depth && table && inv && out, "%s: NULL xyz, depth, table, inv or out", who);
    const FcImage im = {depth, W, H, depth_shift, near, far, edge, band, rel};
    const FcState st = {seen, free, score, hit, miss, floor, ceil};
    hipStream_t s = (hipStream_t)stream;
    if (variant == 1) GF_TRY(hipMemsetAsync(out, 0, (size_t)n * 3 * 4, s));
    if (dtype == 0) {
        if (edge > 0.0f)
            fc_launch<unsigned short, true>(xyz, n, im, F, table, inv, out, codes, st, variant, s);
        else
            fc_launch<unsigned short, false>(xyz, n, im, F, table, inv, out, codes, st, variant, s);
    } else {
        if (edge > 0.0f)
            fc_launch<float, true>(xyz, n, im, F, table, inv, out, codes, st, variant, s);
        else
            fc_launch<float, false>(xyz, n, im, F, table, inv, out, codes, st, variant, s);
    }
    GF_CHECK_LAUNCH(who);
    return GF_OK;
}
