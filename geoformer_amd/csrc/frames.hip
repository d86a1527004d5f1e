// Scenes from posed depth frames: every valid depth pixel of a set of frames to a world point, and one
// fused point per grid cell.  The host statements are frames.backproject_host and frames.cell_means_host; see
// include/geoformer_hip.h for the arguments and every arithmetic step.
//
// Both entry points compact a flagged range in order, and both do it the same fixed way -- no workgroup waits for
// another, there is no look-back and no spin:
//   k_fr_count<Pred>  a workgroup per `chunk` elements, 256 at a time: the flag of every element, one 64-lane ballot per
//                     wave kept as a 64-bit mask word (one bit per element), popcounts summed to the chunk's count
//   k_fr_top          one workgroup: exclusive scan of the chunk counts, 256 at a time with a carry; the total
//   k_fr_emit<Emit>   the same workgroups: an element's row is its chunk's offset + the popcounts of the mask words
//                     before its own in the chunk + the popcount of the bits below its own; Emit writes the outputs
// The flags are computed once (the edge filter reads five depths per pixel); the mask costs one bit per element.
//
// gf_frames_backproject:  two memsets; count<pixel valid>, top, emit<world point, colour, pixel_of, point_of, and the
//                         workgroup's per-axis minimum by one integer atomicMin on float keys>, k_fr_unkey
// gf_frames_cell_means:   memset sums, d_words; k_fr_sums (64-bit integer atomic adds of the fixed-point coordinates
//                         and the colours, runs of equal cells among adjacent lanes added in the wave first);
//                         count<count >= min_obs>, top, emit<mean, colour, count, new_id>
// gf_frames_compose:      one launch, point_of -> new_id[cell_of[point_of]]
#include "common.h"
#include "post_steps.h"

namespace {

typedef unsigned long long u64;
typedef long long i64;

constexpr int FR_THREADS = 256;
constexpr int FR_RECORD = 16;
constexpr int FR_MAX_FRAMES = 1 << 16;
constexpr int FR_MAX_SIDE = 1 << 13;
constexpr int FR_CHUNK = 2048;
constexpr int FR_MAX_CHUNK = 1 << 16;
constexpr int FR_MAX_POINTS = 1 << 29;  // gf_resample_max_points(): asserted in gf_frames_backproject
constexpr double FR_UNITS = 1048576.0;  // fixed-point units per metre
constexpr double FR_REACH = 16384.0;    // metres from the origin the sums are proven for

struct FrScratch {
    u64* masks;   // [ceil(T / 64)]
    int* bcount;  // [nb]
    int* boff;    // [nb]
    unsigned* lokey;  // [4] back-projection: the per-axis minimum of the written coordinates, as keys
};
int fr_nb(i64 T, int chunk) { return (int)((T + chunk - 1) / chunk); }
size_t fr_scratch_bytes(i64 T, int chunk) { return (size_t)((T + 63) / 64) * 8 + (size_t)fr_nb(T, chunk) * 8 + 16 + 64; }
FrScratch fr_carve(void* scratch, i64 T, int chunk) {
    FrScratch s;
    s.masks = (u64*)scratch;
    s.bcount = (int*)(s.masks + (T + 63) / 64);
    s.boff = s.bcount + fr_nb(T, chunk);
    s.lokey = (unsigned*)(s.boff + fr_nb(T, chunk));
    return s;
}
bool fr_chunk_ok(int chunk) { return chunk == 0 || (chunk >= 64 && chunk <= FR_MAX_CHUNK && chunk % 64 == 0); }

// T <= 2^29 and chunk <= 2^16: every index below fits an int
template <class Pred>
__global__ __launch_bounds__(FR_THREADS) void k_fr_count(Pred pred, int T, int chunk, FrScratch s) {
    __shared__ int s_cnt[FR_THREADS / 64];
    const int base = blockIdx.x * chunk, end = min(T, base + chunk);
    int cnt = 0;
    for (int t0 = base + (threadIdx.x & ~63); t0 < end; t0 += FR_THREADS) {  // t0: wave-uniform, a multiple of 64
        const int t = t0 + (threadIdx.x & 63);
        const u64 m = __ballot(t < end && pred(t));
        if ((threadIdx.x & 63) == 0) s.masks[t0 >> 6] = m;
        cnt += __popcll(m);
    }
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
#pragma unroll
        for (int w = 0; w < FR_THREADS / 64; ++w) c += s_cnt[w];
        s.bcount[blockIdx.x] = c;
    }
}

__global__ __launch_bounds__(SCAN_THREADS) void k_fr_top(FrScratch s, int nb, int32_t* __restrict__ total_out) {
    int carry = 0;  // (every thread adds the same totals)
    for (int base = 0; base < nb; base += SCAN_THREADS) {
        const int i = base + threadIdx.x;
        int total;
        const int ex = block_excl_scan(i < nb ? s.bcount[i] : 0, &total);
        if (i < nb) s.boff[i] = carry + ex;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total_out = carry;
}

template <class Emit>
__global__ __launch_bounds__(FR_THREADS) void k_fr_emit(Emit emit, int T, int chunk, FrScratch s) {
    const int base = blockIdx.x * chunk, end = min(T, base + chunk);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int running = s.boff[blockIdx.x];
    typename Emit::State state;
    for (int r0 = base; r0 < end; r0 += FR_THREADS) {  // the round's four words, read by every wave
        int before = running;
        u64 mine = 0;
#pragma unroll
        for (int w = 0; w < FR_THREADS / 64; ++w) {
            const int t0 = r0 + w * 64;
            const u64 m = t0 < end ? s.masks[t0 >> 6] : 0;
            if (w < wave) before += __popcll(m);
            if (w == wave) mine = m;
            running += __popcll(m);
        }
        const int t = r0 + threadIdx.x;
        if (t < end) {
            const bool on = (mine >> lane) & 1;
            emit(t, on ? before + __popcll(mine & ((1ull << lane) - 1)) : -1, state);
        }
    }
    emit.finish(state);  // (every thread of the workgroup arrives here)
}

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
__device__ __forceinline__ bool fr_in_range(const FrImage& im, float z) { return z >= im.near && z <= im.far; }

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
        const float z = fr_depth(im, at);
        if (!fr_in_range(im, z)) return false;
        if (im.edge > 0.0f) {
            const float lim = im.edge * z;
            const bool inside[4] = {i > 0, i + 1 < im.W, j > 0, j + 1 < im.H};
            const size_t nb[4] = {at - 1, at + 1, at - (size_t)im.W, at + (size_t)im.W};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (inside[k]) {
                    const float zn = fr_depth(im, nb[k]);
                    if (fr_in_range(im, zn) && fabsf(zn - z) > lim) return false;
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
    __device__ void operator()(int t, int row, State& st) const {
        point_of[t] = row;
        if (row < 0) return;
        int f, i, j;
        const size_t at = fr_pixel(im, t, &f, &i, &j);
        const float* rec = im.frames + (size_t)f * FR_RECORD;
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
    // falls: a stale read costs an atomic, never loses one)
    __device__ void finish(const State& st) const {
        __shared__ unsigned s_mn[FR_THREADS / 64][3];
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
            for (int w = 0; w < FR_THREADS / 64; ++w) m = min(m, s_mn[w][threadIdx.x]);
            if (m < __hip_atomic_load(&lokey[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                atomicMin(&lokey[threadIdx.x], m);
        }
    }
};

__global__ void k_fr_unkey(const unsigned* __restrict__ key, float* __restrict__ lo) {
    if (threadIdx.x < 3) lo[threadIdx.x] = gf_float_unkey(key[threadIdx.x]);  // (no point written: a NaN, never used)
}

// ------------------------------------------------------------------------------------------------------------------
// cell means
// ------------------------------------------------------------------------------------------------------------------
// sums [M, 6] int64: the three fixed-point coordinate sums, the three colour sums
template <bool AGG>
__global__ __launch_bounds__(FR_THREADS) void k_fr_sums(const float* __restrict__ xyz, const unsigned char* __restrict__ rgb,
                                                        const int32_t* __restrict__ cell_of, int n, int M,
                                                        const float* __restrict__ origin, i64* __restrict__ sums,
                                                        int32_t* __restrict__ words) {
    const int p = blockIdx.x * FR_THREADS + threadIdx.x, lane = threadIdx.x & 63;
    int cell = -1;
    i64 v[6] = {0, 0, 0, 0, 0, 0};
    if (p < n) {
        cell = cell_of[p];
        bool ok = cell >= 0 && cell < M;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double e = (double)xyz[(size_t)p * 3 + a] - (double)origin[a];
            ok = ok && e >= 0.0 && e < FR_REACH;
            v[a] = ok ? (i64)floor(e * FR_UNITS) : 0;
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

struct FrKept {
    const int32_t* count;
    int min_obs;
    __device__ bool operator()(int c) const { return count[c] >= min_obs; }
};

struct FrMean {
    const i64* sums;
    const int32_t* count;
    const float* origin;
    float* xyz_out;
    unsigned char* rgb_out;
    int32_t *count_out, *new_id;
    struct State {};
    __device__ void finish(const State&) const {}
    __device__ void operator()(int c, int row, State&) const {
        new_id[c] = row;
        if (row < 0) return;
        const int cnt = count[c];  // >= min_obs >= 1
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double mean = ((double)sums[(size_t)c * 6 + a] / (double)cnt) * (1.0 / FR_UNITS);
            xyz_out[(size_t)row * 3 + a] = (float)((double)origin[a] + mean);  // row < m <= M
            rgb_out[(size_t)row * 3 + a] = (unsigned char)((sums[(size_t)c * 6 + 3 + a] + cnt / 2) / cnt);
        }
        count_out[row] = cnt;
    }
};

__global__ __launch_bounds__(FR_THREADS) void k_fr_compose(int32_t* __restrict__ point_of, i64 T,
                                                           const int32_t* __restrict__ cell_of,
                                                           const int32_t* __restrict__ new_id) {
    const i64 t = (i64)blockIdx.x * FR_THREADS + threadIdx.x;
    if (t >= T) return;
    const int p = point_of[t];
    if (p >= 0) point_of[t] = new_id[cell_of[p]];
}

template <class Pred, class Emit>
void fr_compact(const Pred& pred, const Emit& emit, int T, int chunk, void* scratch, int32_t* total, hipStream_t st) {
    const FrScratch s = fr_carve(scratch, T, chunk);
    const int nb = fr_nb(T, chunk);
    hipLaunchKernelGGL(k_fr_count<Pred>, dim3(nb), dim3(FR_THREADS), 0, st, pred, T, chunk, s);
    hipLaunchKernelGGL(k_fr_top, dim3(1), dim3(SCAN_THREADS), 0, st, s, nb, total);
    hipLaunchKernelGGL(k_fr_emit<Emit>, dim3(nb), dim3(FR_THREADS), 0, st, emit, T, chunk, s);
}

}  // namespace

extern "C" int gf_frames_record_floats(void) { return FR_RECORD; }
extern "C" int gf_frames_max_frames(void) { return FR_MAX_FRAMES; }
extern "C" int gf_frames_max_side(void) { return FR_MAX_SIDE; }
extern "C" int gf_frames_default_chunk(void) { return FR_CHUNK; }

extern "C" size_t gf_frames_backproject_scratch_bytes(long long T, int chunk) {
    if (T < 1 || T > FR_MAX_POINTS || !fr_chunk_ok(chunk)) return 0;
    return fr_scratch_bytes(T, chunk ? chunk : FR_CHUNK);
}

extern "C" int gf_frames_backproject(const void* depth, int kind, float depth_shift, const unsigned char* color,
                                     const float* frames, int F, int W, int H, int stride, float near, float far, float edge,
                                     int chunk, void* scratch, float* xyz, unsigned char* rgb, int32_t* pixel_of,
                                     int32_t* point_of, float* lo, int32_t* d_words, void* stream) {
    GF_CHECK_ARG(F >= 1 && F <= FR_MAX_FRAMES, "gf_frames_backproject: F = %d frames (1 to %d)", F, FR_MAX_FRAMES);
    GF_CHECK_ARG(W >= 1 && W <= FR_MAX_SIDE && H >= 1 && H <= FR_MAX_SIDE,
                 "gf_frames_backproject: images of %d x %d pixels (each side 1 to %d)", W, H, FR_MAX_SIDE);
    GF_CHECK_ARG(stride >= 1, "gf_frames_backproject: stride = %d (>= 1)", stride);
    GF_CHECK_ARG(kind == 0 || kind == 1, "gf_frames_backproject: kind = %d (0 uint16, 1 float32)", kind);
    GF_CHECK_ARG(depth_shift > 0.0f && depth_shift <= 3.402823466e38f,
                 "gf_frames_backproject: depth_shift = %g (positive and finite)", (double)depth_shift);
    GF_CHECK_ARG(edge >= 0.0f && edge <= 3.402823466e38f, "gf_frames_backproject: edge = %g (>= 0 and finite)", (double)edge);
    GF_CHECK_ARG(fr_chunk_ok(chunk), "gf_frames_backproject: chunk = %d (0, or a multiple of 64 from 64 to %d)", chunk,
                 FR_MAX_CHUNK);
    const int Ws = gf_div_up(W, stride), Hs = gf_div_up(H, stride);
    const long long T = (long long)F * Hs * Ws;
    GF_CHECK_ARG(gf_resample_max_points() == FR_MAX_POINTS && T <= FR_MAX_POINTS,
                 "gf_frames_backproject: %lld sampled pixels (at most %d)", T, FR_MAX_POINTS);
    GF_CHECK_ARG(depth && frames && scratch && xyz && rgb && pixel_of && point_of && d_words,
                 "gf_frames_backproject: NULL depth, frames, scratch, xyz, rgb, pixel_of, point_of or d_words");
    hipStream_t st = (hipStream_t)stream;
    if (!chunk) chunk = FR_CHUNK;
    const FrImage im = {depth, color, frames, kind, W, H, Ws, Hs, stride, depth_shift, near, far, edge};
    const FrScratch s = fr_carve(scratch, T, chunk);
    GF_TRY(hipMemsetAsync(d_words, 0, 2 * 4, st));
    GF_TRY(hipMemsetAsync(s.lokey, 0xff, 4 * 4, st));
    fr_compact(FrValid{im}, FrPoint{im, xyz, rgb, pixel_of, point_of, d_words, s.lokey}, (int)T, chunk, scratch, d_words, st);
    if (lo) hipLaunchKernelGGL(k_fr_unkey, dim3(1), dim3(64), 0, st, s.lokey, lo);
    GF_CHECK_LAUNCH("gf_frames_backproject");
    return GF_OK;
}

extern "C" size_t gf_frames_cell_means_scratch_bytes(int M, int chunk) {
    if (M < 1 || M > FR_MAX_POINTS || !fr_chunk_ok(chunk)) return 0;
    return fr_scratch_bytes(M, chunk ? chunk : FR_CHUNK) + (size_t)M * 6 * 8;
}

extern "C" int gf_frames_cell_means(const float* xyz, const unsigned char* rgb, const int32_t* cell_of, const int32_t* count,
                                    int n, int M, const float* origin, int min_obs, int aggregate, int chunk, void* scratch,
                                    float* xyz_out, unsigned char* rgb_out, int32_t* count_out, int32_t* new_id,
                                    int32_t* d_words, void* stream) {
    GF_CHECK_ARG(n >= 1 && n <= FR_MAX_POINTS && M >= 1 && M <= FR_MAX_POINTS,
                 "gf_frames_cell_means: n = %d points, M = %d cells (each 1 to %d)", n, M, FR_MAX_POINTS);
    GF_CHECK_ARG(min_obs >= 1, "gf_frames_cell_means: min_obs = %d (>= 1)", min_obs);
    GF_CHECK_ARG(fr_chunk_ok(chunk), "gf_frames_cell_means: chunk = %d (0, or a multiple of 64 from 64 to %d)", chunk,
                 FR_MAX_CHUNK);
    GF_CHECK_ARG(xyz && rgb && cell_of && count && origin && scratch && xyz_out && rgb_out && count_out && new_id && d_words,
                 "gf_frames_cell_means: NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    if (!chunk) chunk = FR_CHUNK;
    i64* sums = (i64*)scratch;  // [M, 6], in front of the compaction's own scratch
    void* rest = sums + (size_t)M * 6;
    GF_TRY(hipMemsetAsync(sums, 0, (size_t)M * 6 * 8, st));
    GF_TRY(hipMemsetAsync(d_words, 0, 2 * 4, st));
    if (aggregate)
        hipLaunchKernelGGL(k_fr_sums<true>, dim3(gf_div_up(n, FR_THREADS)), dim3(FR_THREADS), 0, st, xyz, rgb, cell_of, n, M,
                           origin, sums, d_words);
    else
        hipLaunchKernelGGL(k_fr_sums<false>, dim3(gf_div_up(n, FR_THREADS)), dim3(FR_THREADS), 0, st, xyz, rgb, cell_of, n, M,
                           origin, sums, d_words);
    fr_compact(FrKept{count, min_obs}, FrMean{sums, count, origin, xyz_out, rgb_out, count_out, new_id}, M, chunk, rest,
               d_words, st);
    GF_CHECK_LAUNCH("gf_frames_cell_means");
    return GF_OK;
}

extern "C" int gf_frames_compose(int32_t* point_of, long long T, const int32_t* cell_of, const int32_t* new_id, void* stream) {
    GF_CHECK_ARG(T >= 0 && T <= FR_MAX_POINTS, "gf_frames_compose: T = %lld (0 to %d)", T, FR_MAX_POINTS);
    if (T == 0) return GF_OK;
    GF_CHECK_ARG(point_of && cell_of && new_id, "gf_frames_compose: NULL point_of, cell_of or new_id");
    hipLaunchKernelGGL(k_fr_compose, dim3(gf_div_up(T, FR_THREADS)), dim3(FR_THREADS), 0, (hipStream_t)stream, point_of, T,
                       cell_of, new_id);
    GF_CHECK_LAUNCH("gf_frames_compose");
    return GF_OK;
}
