// Steps that the frames kernels repeat (frames, frames_stream, frames_vote, frames_vote_stream, frames_track,
// frames_carve), each defined once, with the limits the six files must agree on.  The device helpers are forced inline
// and were checked to leave the kernels' machine code as it was (tools/isa_diff.sh); where a kernel's code would change,
// that kernel keeps the step written out and says so (DESIGN.md §4 lists them).  Everything is in an unnamed namespace:
// a file that includes this gets kernels of its own.
#pragma once
#include "common.h"

namespace {

typedef unsigned long long u64;
typedef long long i64;

constexpr int FS_THREADS = 256;         // threads of a workgroup, in every kernel of the family but k_ft_match
constexpr int FS_RECORD = 16;           // floats of a frame's record: gf_frames_record_floats()
constexpr int FS_MAX_FRAMES = 1 << 16;  // gf_frames_max_frames()
constexpr int FS_MAX_SIDE = 1 << 13;    // gf_frames_max_side()
constexpr int FS_CHUNK = 2048;          // gf_frames_default_chunk()
constexpr int FS_MAX_CHUNK = 1 << 16;
constexpr int FS_MAX_POINTS = 1 << 29;  // gf_resample_max_points(): asserted by the entry points that take points
constexpr int FS_MAX_PROBES = 128;      // probes before a thread gives up on a table that may be more than half full
constexpr double FS_UNITS = 1048576.0;  // fixed-point units per metre
constexpr u64 FS_EMPTY = 0xffffffffffffffffull;  // no key (a memset of 0xff): no cell, group or row reaches 2^31

// ---- the small pieces ---------------------------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ T fs_peek(const T* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned fs_hash(u64 key, unsigned mask) {
    return (unsigned)((key * 0x9E3779B97F4A7C15ull) >> 32) & mask;
}
inline bool fs_slots_ok(i64 slots, i64 lo, i64 hi) { return slots >= lo && slots <= hi && (slots & (slots - 1)) == 0; }
inline i64 fs_pow2_slots(i64 want, i64 lo, i64 hi) {  // the first power of two from lo that reaches `want`, at most hi
    i64 p = lo;
    while (p < want && p < hi) p <<= 1;
    return p;
}
// a persistent table's default: four slots per stored key, or an eighth of the elements offered
inline i64 fs_default_slots(i64 stored, i64 offered, i64 lo, i64 hi) {
    return fs_pow2_slots(4 * stored > offered / 8 ? 4 * stored : offered / 8, lo, hi);
}
inline int fs_blocks(i64 work, int most) {  // workgroups that stride over `work` elements: 1 to `most`
    const i64 g = (work + FS_THREADS - 1) / FS_THREADS;
    return (int)(g < most ? (g > 0 ? g : 1) : most);
}
inline bool fs_chunk_ok(int chunk) { return chunk == 0 || (chunk >= 64 && chunk <= FS_MAX_CHUNK && chunk % 64 == 0); }

// ---- ordered compaction of a flagged range ------------------------------------------------------------------------
// The same fixed way for every caller -- no workgroup waits for another, there is no look-back and no spin:
//   k_fs_count<Pred>  a workgroup per `chunk` elements, 256 at a time: the flag of every element, one 64-lane ballot per
//                     wave kept as a 64-bit mask word (one bit per element), popcounts summed to the chunk's count
//   k_fs_top          one workgroup: exclusive scan of the chunk counts, 256 at a time with a carry; add + the total
//   k_fs_emit<Emit>   the same workgroups: an element's row is its chunk's offset + the popcounts of the mask words
//                     before its own in the chunk + the popcount of the bits below its own; Emit writes the outputs
// The flags are computed once; the mask costs one bit per element.  Emit has off() (the launch does nothing: the same
// answer for every thread), a State every thread carries through its elements, and finish(state), which every thread of
// a workgroup reaches.
struct FsScratch {
    u64* masks;   // [ceil(T / 64)]
    int* bcount;  // [nb]
    int* boff;    // [nb]
};
inline int fs_nb(i64 T, int chunk) { return (int)((T + chunk - 1) / chunk); }
inline size_t fs_scan_bytes(i64 T, int chunk) { return (size_t)((T + 63) / 64) * 8 + (size_t)fs_nb(T, chunk) * 8 + 64; }
inline FsScratch fs_carve(void* scratch, i64 T, int chunk) {
    FsScratch s;
    s.masks = (u64*)scratch;
    s.bcount = (int*)(s.masks + (T + 63) / 64);
    s.boff = s.bcount + fs_nb(T, chunk);
    return s;
}

// T <= 2^31 - 1 - 2^16 and chunk <= 2^16: base + chunk fits an int
template <class Pred>
__global__ __launch_bounds__(FS_THREADS) void k_fs_count(Pred pred, int T, int chunk, FsScratch s) {
    __shared__ int s_cnt[FS_THREADS / 64];
    const int base = blockIdx.x * chunk, end = min(T, base + chunk);
    int cnt = 0;
    for (int t0 = base + (threadIdx.x & ~63); t0 < end; t0 += FS_THREADS) {  // t0: wave-uniform, a multiple of 64
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
        for (int w = 0; w < FS_THREADS / 64; ++w) c += s_cnt[w];
        s.bcount[blockIdx.x] = c;
    }
}

// *total_out = add + the number of flagged elements
template <int = 0>  // (a template only so that a file that does not compact gets no copy of the kernel)
__global__ __launch_bounds__(SCAN_THREADS) void k_fs_top(FsScratch s, int nb, int add, int32_t* __restrict__ total_out) {
    int carry = 0;  // (every thread adds the same totals)
    for (int base = 0; base < nb; base += SCAN_THREADS) {
        const int i = base + threadIdx.x;
        int total;
        const int ex = block_excl_scan(i < nb ? s.bcount[i] : 0, &total);
        if (i < nb) s.boff[i] = carry + ex;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total_out = add + carry;
}

template <class Emit>
__global__ __launch_bounds__(FS_THREADS) void k_fs_emit(Emit emit, int T, int chunk, FsScratch s) {
    if (emit.off()) return;  // (the same words for every thread)
    const int base = blockIdx.x * chunk, end = min(T, base + chunk);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int running = s.boff[blockIdx.x];
    typename Emit::State state;
    for (int r0 = base; r0 < end; r0 += FS_THREADS) {  // the round's four words, read by every wave
        int before = running;
        u64 mine = 0;
#pragma unroll
        for (int w = 0; w < FS_THREADS / 64; ++w) {
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

// the rows of the elements `pred` flags, in order, handed to `emit` (-1 for an element without one); *total = add + their
// number.  scratch: fs_scan_bytes(T, chunk)
template <class Pred, class Emit>
void fs_compact(const Pred& pred, const Emit& emit, int T, int chunk, void* scratch, int add, int32_t* total, hipStream_t st) {
    const FsScratch s = fs_carve(scratch, T, chunk);
    const int nb = fs_nb(T, chunk);
    hipLaunchKernelGGL(k_fs_count<Pred>, dim3(nb), dim3(FS_THREADS), 0, st, pred, T, chunk, s);
    hipLaunchKernelGGL(k_fs_top<>, dim3(1), dim3(SCAN_THREADS), 0, st, s, nb, add, total);
    hipLaunchKernelGGL(k_fs_emit<Emit>, dim3(nb), dim3(FS_THREADS), 0, st, emit, T, chunk, s);
}

// the cells seen at least min_obs times, and their means from the integer sums [M, 6] (three fixed-point coordinate
// sums, three colour sums)
struct FsKept {
    const int32_t* count;
    int min_obs;
    __device__ bool operator()(int c) const { return count[c] >= min_obs; }
};

struct FsMean {
    const i64* sums;
    const int32_t* count;
    const float* origin;
    float* xyz_out;
    unsigned char* rgb_out;
    int32_t *count_out, *new_id;
    struct State {};
    __device__ bool off() const { return false; }
    __device__ void finish(const State&) const {}
    __device__ void operator()(int c, int row, State&) const {
        new_id[c] = row;
        if (row < 0) return;
        const int cnt = count[c];  // >= min_obs >= 1
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double mean = ((double)sums[(size_t)c * 6 + a] / (double)cnt) * (1.0 / FS_UNITS);
            xyz_out[(size_t)row * 3 + a] = (float)((double)origin[a] + mean);  // row < m <= M
            rgb_out[(size_t)row * 3 + a] = (unsigned char)((sums[(size_t)c * 6 + 3 + a] + cnt / 2) / cnt);
        }
        count_out[row] = cnt;
    }
};

// ---- runs of equal keys among adjacent lanes ------------------------------------------------------------------------
// Whether this lane is the head of its run, and the run's length when it is, read off the one ballot of the heads -- no
// exchange between the lanes.  Runs are numbered by their heads: two runs of one key with another key between them stay
// two runs, and each head acts for its own.
__device__ __forceinline__ bool fs_run(u64 key, int lane, unsigned* len) {
    const u64 left = __shfl_up(key, 1, 64);
    const bool head = lane == 0 || left != key;
    const u64 heads = __ballot(head);
    const u64 above = (heads >> lane) >> 1;  // the heads after this lane
    *len = above ? (unsigned)__ffsll((i64)above) : (unsigned)(64 - lane);
    return head;
}

// ---- open addressing: a key found or claimed (the argument; the loop is in the kernels) ---------------------------
// A key is written once, by a 64-bit CAS on an empty slot, and never changes.  So the slot is read first and the CAS
// issued only on an empty one: a stale read costs an atomic, never loses one (the same holds for the words beside the
// tables that only fall or only rise: read first, atomicMin / atomicMax only when it can change something).
// Termination.  A caller that keeps the table at most half full (slots >= twice the keys it can ever hold) passes
// bounded = 0: a probe always meets its own key or an empty slot.  With fewer slots it passes bounded = 1, and a thread
// gives up after FS_MAX_PROBES probes.  No thread ever waits for another; there is no spin.
// The probing kernels (k_fm_claim, k_fv_insert, k_vs_claim, k_ft_count; k_fm_move and k_vs_move in the unbounded form
// without the "own key" exit: a rehash holds a key once and the new table has a slot per key) keep the loop written
// out and refer to this comment: as a function, every form that was tried changed their code.

// ---- the validity of a depth pixel ------------------------------------------------------------------------------------
__device__ __forceinline__ bool fs_in_range(float z, float near, float far) { return z >= near && z <= far; }

// *z = depth(at), the depth of pixel (i, j) of a W x H image, is valid when it lies in [near, far] and, with the edge
// filter, no in-range depth of its four neighbours inside the image differs from it by more than edge z.  FILTER: 1 the
// filter is on, 0 off, -1 on when edge > 0.  depth(at) reads one pixel.
template <int FILTER, class Depth>
__device__ __forceinline__ bool fs_depth_valid(const Depth& depth, size_t at, int i, int j, int W, int H, float near, float far,
                                               float edge, float* z_out) {
    const float z = depth(at);
    *z_out = z;
    if (!fs_in_range(z, near, far)) return false;
    if (FILTER > 0 || (FILTER < 0 && edge > 0.0f)) {
        const float lim = edge * z;
        const bool inside[4] = {i > 0, i + 1 < W, j > 0, j + 1 < H};
        const size_t nb[4] = {at - 1, at + 1, at - (size_t)W, at + (size_t)W};
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (inside[k]) {
                const float zn = depth(nb[k]);
                if (fs_in_range(zn, near, far) && fabsf(zn - z) > lim) return false;
            }
    }
    return true;
}

}  // namespace
