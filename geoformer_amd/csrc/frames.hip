// Scenes from posed depth frames: every valid depth pixel of a set of frames to a world point, and one
// fused point per grid cell.  The host statements are frames.backproject_host and frames.cell_means_host; see
// include/geoformer_hip.h for the arguments and every arithmetic step.
//
// Both entry points compact a flagged range in order with frames_steps.h's count / top / emit (k_fs_count<Pred>, k_fs_top,
// k_fs_emit<Emit>); the flags are computed once (the edge filter reads five depths per pixel).
//
// gf_frames_backproject:  two memsets; count<pixel valid>, top, emit<world point, colour, pixel_of, point_of, and the
//                         workgroup's per-axis minimum by one integer atomicMin on float keys>, k_fr_unkey
// gf_frames_cell_means:   memset sums, d_words; k_fr_sums (64-bit integer atomic adds of the fixed-point coordinates
//                         and the colours, runs of equal cells among adjacent lanes added in the wave first);
//                         count<count >= min_obs>, top, emit<mean, colour, count, new_id>
// gf_frames_compose:      one launch, point_of -> new_id[cell_of[point_of]]
#include "common.h"
#include "post_steps.h"
#include "frames_steps.h"

namespace {

constexpr double FR_REACH = 16384.0;  // metres from the origin the sums are proven for

// the per-axis minimum of the written coordinates, as keys [4]: behind the compaction's own scratch
size_t fr_scratch_bytes(i64 T, int chunk) { return fs_scan_bytes(T, chunk) + 16; }
unsigned* fr_lokey(void* scratch, i64 T, int chunk) { return (unsigned*)(fs_carve(scratch, T, chunk).boff + fs_nb(T, chunk)); }

// ------------------------------------------------------------------------------------------------------------------
// back-projection
// ------------------------------------------------------------------------------------------------------------------
struct FrImage {
    const void* depth;
    const unsigned char* color;
    const float* frames;
    int kind, W, H, Ws, Hs, stride;
    float shift, near, far, edge;
};

__device__ __forceinline__ float fr_depth(const FrImage& im, size_t at) {
    const float d = im.kind ? ((const float*)im.depth)[at] : (float)((const unsigned short*)im.depth)[at];
    return __fdiv_rn(d, im.shift);
}

// sampled pixel t -> frame f, full-resolution pixel (i, j) and its place in depth / color
__device__ __forceinline__ size_t fr_pixel(const FrImage& im, int t, int* f, int* i, int* j) {
    const int per = im.Hs * im.Ws, r = t % per;
    *f = t / per;
    *j = (r / im.Ws) * im.stride;
    *i = (r % im.Ws) * im.stride;
    return ((size_t)*f * im.H + *j) * im.W + *i;  // j < H, i < W: (Ws - 1) stride <= W - 1
}

struct FrValid {
    FrImage im;
    __device__ bool operator()(int t) const {
        int f, i, j;
        const size_t at = fr_pixel(im, t, &f, &i, &j);
        // fs_depth_valid's rule, kept written out: through the helper k_fs_count<FrValid> is 19 lines shorter (447 -> 428)
        const float z = fr_depth(im, at);
        if (!fs_in_range(z, im.near, im.far)) return false;
        if (im.edge > 0.0f) {
            const float lim = im.edge * z;
            const bool inside[4] = {i > 0, i + 1 < im.W, j > 0, j + 1 < im.H};
            const size_t nb[4] = {at - 1, at + 1, at - (size_t)im.W, at + (size_t)im.W};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (inside[k]) {
                    const float zn = fr_depth(im, nb[k]);
                    if (fs_in_range(zn, im.near, im.far) && fabsf(zn - z) > lim) return false;
                }
        }
        return true;
    }
};

struct FrPoint {
    FrImage im;
    float* xyz;
    unsigned char* rgb;
    int32_t *pixel_of, *point_of, *words;
    unsigned* lokey;
    struct State {
        unsigned mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu};
    };
    __device__ bool off() const { return false; }
    __device__ void operator()(int t, int row, State& st) const {
        point_of[t] = row;
        if (row < 0) return;
        int f, i, j;
        const size_t at = fr_pixel(im, t, &f, &i, &j);
        const float* rec = im.frames + (size_t)f * FS_RECORD;
        const float z = fr_depth(im, at);
        const float xc = __fdiv_rn((((float)i + 0.5f) - rec[2]) * z, rec[0]);
        const float yc = __fdiv_rn((((float)j + 0.5f) - rec[3]) * z, rec[1]);
        const float* P = rec + 4;
        bool fin = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = ((P[4 * a] * xc + P[4 * a + 1] * yc) + P[4 * a + 2] * z) + P[4 * a + 3];
            xyz[(size_t)row * 3 + a] = v;  // row < n <= T
            fin = fin && isfinite(v);
            if (v == v) st.mn[a] = min(st.mn[a], gf_float_key(v));
            rgb[(size_t)row * 3 + a] = im.color ? im.color[at * 3 + a] : (unsigned char)0;
        }
        pixel_of[row] = t;
        if (!fin) words[1] = 1;
    }
    // the workgroup's minimum per axis: one atomic per axis, and only when it beats the word read first (the word only
    // falls: frames_steps.h, "a key found or claimed")
    __device__ void finish(const State& st) const {
        __shared__ unsigned s_mn[FS_THREADS / 64][3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            unsigned m = st.mn[a];
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) m = min(m, (unsigned)__shfl_xor((int)m, d, 64));
            if ((threadIdx.x & 63) == 0) s_mn[threadIdx.x >> 6][a] = m;
        }
        __syncthreads();
        if (threadIdx.x < 3) {
            unsigned m = 0xffffffffu;
#pragma unroll
            for (int w = 0; w < FS_THREADS / 64; ++w) m = min(m, s_mn[w][threadIdx.x]);
            if (m < fs_peek(&lokey[threadIdx.x])) atomicMin(&lokey[threadIdx.x], m);
        }
    }
};

__global__ void k_fr_unkey(const unsigned* __restrict__ key, float* __restrict__ lo) {
    if (threadIdx.x < 3) lo[threadIdx.x] = gf_float_unkey(key[threadIdx.x]);  // (no point written: a NaN, never used)
}

// ------------------------------------------------------------------------------------------------------------------
// cell means
// ------------------------------------------------------------------------------------------------------------------
// sums [M, 6] int64: the three fixed-point coordinate sums, the three colour sums.  The body is k_fm_add's
// (frames_stream.hip) without the count, kept written out in both: as one inlined function the <true> instantiations need
// 41 VGPRs instead of 32 (567 -> 570 and 591 -> 599 lines); sharing the addends alone makes them 6 lines shorter
template <bool AGG>
__global__ __launch_bounds__(FS_THREADS) void k_fr_sums(const float* __restrict__ xyz, const unsigned char* __restrict__ rgb,
                                                        const int32_t* __restrict__ cell_of, int n, int M,
                                                        const float* __restrict__ origin, i64* __restrict__ sums,
                                                        int32_t* __restrict__ words) {
    const int p = blockIdx.x * FS_THREADS + threadIdx.x, lane = threadIdx.x & 63;
    int cell = -1;
    i64 v[6] = {0, 0, 0, 0, 0, 0};
    if (p < n) {
        cell = cell_of[p];
        bool ok = cell >= 0 && cell < M;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double e = (double)xyz[(size_t)p * 3 + a] - (double)origin[a];
            ok = ok && e >= 0.0 && e < FR_REACH;
            v[a] = ok ? (i64)floor(e * FS_UNITS) : 0;
            v[3 + a] = rgb[(size_t)p * 3 + a];
        }
        if (!ok) {
            words[1] = 1;
            cell = -1;  // nothing is added for this point
        }
    }
    bool head = true;
    if (AGG) {
        // a run: adjacent lanes holding the same cell.  Runs are numbered by their heads, so two runs of one cell with
        // another cell between them stay two runs (each issues its own atomics).
        const int left = __shfl_up(cell, 1, 64);
        head = lane == 0 || left != cell;
        const u64 heads = __ballot(head);
        if (heads != ~0ull) {  // (wave-uniform; every lane alone in its cell skips the exchange)
            const int run = __popcll(heads & ((2ull << lane) - 1));
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {  // after the step of d, a lane holds its run's lanes [lane, lane + 2 d)
                const bool same = __shfl_down(run, d, 64) == run && lane + d < 64;
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    const i64 o = __shfl_down(v[k], d, 64);
                    if (same) v[k] += o;
                }
            }
        }
    }
    if (head && cell >= 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) atomicAdd((u64*)&sums[(size_t)cell * 6 + k], (u64)v[k]);
    }
}

__global__ __launch_bounds__(FS_THREADS) void k_fr_compose(int32_t* __restrict__ point_of, i64 T,
                                                           const int32_t* __restrict__ cell_of,
                                                           const int32_t* __restrict__ new_id) {
    const i64 t = (i64)blockIdx.x * FS_THREADS + threadIdx.x;
    if (t >= T) return;
    const int p = point_of[t];
    if (p >= 0) point_of[t] = new_id[cell_of[p]];
}

}  // namespace

extern "C" int gf_frames_record_floats(void) { return FS_RECORD; }
extern "C" int gf_frames_max_frames(void) { return FS_MAX_FRAMES; }
extern "C" int gf_frames_max_side(void) { return FS_MAX_SIDE; }
extern "C" int gf_frames_default_chunk(void) { return FS_CHUNK; }

extern "C" size_t gf_frames_backproject_scratch_bytes(long long T, int chunk) {
    if (T < 1 || T > FS_MAX_POINTS || !fs_chunk_ok(chunk)) return 0;
    return fr_scratch_bytes(T, chunk ? chunk : FS_CHUNK);
}

extern "C" int gf_frames_backproject(const void* depth, int kind, float depth_shift, const unsigned char* color,
                                     const float* frames, int F, int W, int H, int stride, float near, float far, float edge,
                                     int chunk, void* scratch, float* xyz, unsigned char* rgb, int32_t* pixel_of,
                                     int32_t* point_of, float* lo, int32_t* d_words, void* stream) {
    GF_CHECK_ARG(F >= 1 && F <= FS_MAX_FRAMES, "gf_frames_backproject: F = %d frames (1 to %d)", F, FS_MAX_FRAMES);
    GF_CHECK_ARG(W >= 1 && W <= FS_MAX_SIDE && H >= 1 && H <= FS_MAX_SIDE,
                 "gf_frames_backproject: images of %d x %d pixels (each side 1 to %d)", W, H, FS_MAX_SIDE);
    GF_CHECK_ARG(stride >= 1, "gf_frames_backproject: stride = %d (>= 1)", stride);
    GF_CHECK_ARG(kind == 0 || kind == 1, "gf_frames_backproject: kind = %d (0 uint16, 1 float32)", kind);
    GF_CHECK_ARG(depth_shift > 0.0f && depth_shift <= 3.402823466e38f,
                 "gf_frames_backproject: depth_shift = %g (positive and finite)", (double)depth_shift);
    GF_CHECK_ARG(edge >= 0.0f && edge <= 3.402823466e38f, "gf_frames_backproject: edge = %g (>= 0 and finite)", (double)edge);
    GF_CHECK_ARG(fs_chunk_ok(chunk), "gf_frames_backproject: chunk = %d (0, or a multiple of 64 from 64 to %d)", chunk,
                 FS_MAX_CHUNK);
    const int Ws = gf_div_up(W, stride), Hs = gf_div_up(H, stride);
    const long long T = (long long)F * Hs * Ws;
    GF_CHECK_ARG(gf_resample_max_points() == FS_MAX_POINTS && T <= FS_MAX_POINTS,
                 "gf_frames_backproject: %lld sampled pixels (at most %d)", T, FS_MAX_POINTS);
    GF_CHECK_ARG(depth && frames && scratch && xyz && rgb && pixel_of && point_of && d_words,
                 "gf_frames_backproject: NULL depth, frames, scratch, xyz, rgb, pixel_of, point_of or d_words");
    hipStream_t st = (hipStream_t)stream;
    if (!chunk) chunk = FS_CHUNK;
    const FrImage im = {depth, color, frames, kind, W, H, Ws, Hs, stride, depth_shift, near, far, edge};
    unsigned* lokey = fr_lokey(scratch, T, chunk);
    GF_TRY(hipMemsetAsync(d_words, 0, 2 * 4, st));
    GF_TRY(hipMemsetAsync(lokey, 0xff, 4 * 4, st));
    fs_compact(FrValid{im}, FrPoint{im, xyz, rgb, pixel_of, point_of, d_words, lokey}, (int)T, chunk, scratch, 0, d_words, st);
    if (lo) hipLaunchKernelGGL(k_fr_unkey, dim3(1), dim3(64), 0, st, lokey, lo);
    GF_CHECK_LAUNCH("gf_frames_backproject");
    return GF_OK;
}

extern "C" size_t gf_frames_cell_means_scratch_bytes(int M, int chunk) {
    if (M < 1 || M > FS_MAX_POINTS || !fs_chunk_ok(chunk)) return 0;
    return fr_scratch_bytes(M, chunk ? chunk : FS_CHUNK) + (size_t)M * 6 * 8;
}

extern "C" int gf_frames_cell_means(const float* xyz, const unsigned char* rgb, const int32_t* cell_of, const int32_t* count,
                                    int n, int M, const float* origin, int min_obs, int aggregate, int chunk, void* scratch,
                                    float* xyz_out, unsigned char* rgb_out, int32_t* count_out, int32_t* new_id,
                                    int32_t* d_words, void* stream) {
    GF_CHECK_ARG(n >= 1 && n <= FS_MAX_POINTS && M >= 1 && M <= FS_MAX_POINTS,
                 "gf_frames_cell_means: n = %d points, M = %d cells (each 1 to %d)", n, M, FS_MAX_POINTS);
    GF_CHECK_ARG(min_obs >= 1, "gf_frames_cell_means: min_obs = %d (>= 1)", min_obs);
    GF_CHECK_ARG(fs_chunk_ok(chunk), "gf_frames_cell_means: chunk = %d (0, or a multiple of 64 from 64 to %d)", chunk,
                 FS_MAX_CHUNK);
    GF_CHECK_ARG(xyz && rgb && cell_of && count && origin && scratch && xyz_out && rgb_out && count_out && new_id && d_words,
                 "gf_frames_cell_means: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    if (!chunk) chunk = FS_CHUNK;
    i64* sums = (i64*)scratch;  // [M, 6], in front of the compaction's own scratch
    void* rest = sums + (size_t)M * 6;
    GF_TRY(hipMemsetAsync(sums, 0, (size_t)M * 6 * 8, st));
    GF_TRY(hipMemsetAsync(d_words, 0, 2 * 4, st));
    if (aggregate)
        hipLaunchKernelGGL(k_fr_sums<true>, dim3(gf_div_up(n, FS_THREADS)), dim3(FS_THREADS), 0, st, xyz, rgb, cell_of, n, M,
                           origin, sums, d_words);
    else
        hipLaunchKernelGGL(k_fr_sums<false>, dim3(gf_div_up(n, FS_THREADS)), dim3(FS_THREADS), 0, st, xyz, rgb, cell_of, n, M,
                           origin, sums, d_words);
    fs_compact(FsKept{count, min_obs}, FsMean{sums, count, origin, xyz_out, rgb_out, count_out, new_id}, M, chunk, rest, 0,
               d_words, st);
    GF_CHECK_LAUNCH("gf_frames_cell_means");
    return GF_OK;
}

extern "C" int gf_frames_compose(int32_t* point_of, long long T, const int32_t* cell_of, const int32_t* new_id, void* stream) {
    GF_CHECK_ARG(T >= 0 && T <= FS_MAX_POINTS, "gf_frames_compose: T = %lld (0 to %d)", T, FS_MAX_POINTS);
    if (T == 0) return GF_OK;
    GF_CHECK_ARG(point_of && cell_of && new_id, "gf_frames_compose: NULL point_of, cell_of or new_id");
    hipLaunchKernelGGL(k_fr_compose, dim3(gf_div_up(T, FS_THREADS)), dim3(FS_THREADS), 0, (hipStream_t)stream, point_of, T,
                       cell_of, new_id);
    GF_CHECK_LAUNCH("gf_frames_compose");
    return GF_OK;
}
