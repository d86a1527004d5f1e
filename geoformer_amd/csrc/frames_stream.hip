// A map of fused cells that persists between calls: frames.fuse's cells and integer sums, fed one chunk of
// frames at a time.  The host statement is frames.FuserHost; see include/geoformer_hip.h for the arguments, the state
// (all of it owned by the caller) and every arithmetic step.
//
// gf_frames_map_rehash      k_fm_clear (keys all ones, ids -1, first INT_MAX), k_fm_move (every old slot with id >= 0
//                           claims its key in the new table by 64-bit CAS and copies its id)
// gf_frames_map_insert      one memset of the words, then
//   k_fm_claim              one thread per point: the cell key by k_rs_insert's arithmetic, the reach by k_fr_sums'
//                           float64 comparison; the key found or claimed (slot read first, CAS on an empty slot only);
//                           a slot that has no number takes an integer atomicMin of the point index (read first)
//   k_fs_count, k_fs_top, k_fs_emit<FmNumber>   exclusive scan in POINT order of "my slot has no number and I am its
//                           first point": a new cell's first point writes id = M + rank
//   k_fm_cell_of            one thread per point: cell_of = ids[slot]
// gf_frames_map_accumulate  k_fm_add<AGG>: 64-bit integer atomic adds of the fixed-point coordinates and the colours, a
//                           32-bit one of the count; runs of equal cells among adjacent lanes added in the wave first
// gf_frames_map_means       k_fs_count, k_fs_top, k_fs_emit<FsMean>: the kept cells renumbered in order, their means
// gf_frames_map_lookup      one launch, out = table[index] or -1; an index outside the table raises a flag
//
// The compaction (k_fs_count / k_fs_top / k_fs_emit) and the means are frames_steps.h's, and so is the termination
// argument of the probing ("a key found or claimed").  k_fm_claim is unbounded with slots >= 2 (M + n): the table holds
// at most M + n keys.  k_fm_move: the new table has at least as many slots as there are numbered cells, all of distinct
// keys.
//
// A failed insert.  k_fs_emit<FmNumber> and k_fm_cell_of read the three failure words first and return when one is set
// (every thread reads the same words: the branch is uniform), so no id is written; count and sums are not touched by
// the insert at all.  What remains are claimed keys without a number, which the rehash drops.
#include "common.h"
#include "frames_steps.h"

namespace {

constexpr int FM_AXIS_BITS = 21;
constexpr i64 FM_MIN_SLOTS = 64;
constexpr i64 FM_MAX_SLOTS = 1ll << 31;
constexpr i64 FM_MAX_PIXELS = 2147483647ll;  // every count fits an int32, every id too
constexpr int FM_MAX_CELLS = 2147483647 - FS_MAX_CHUNK;  // the cells gf_frames_map_means indexes with ints
constexpr int FM_NO_POINT = 2147483647;  // `first` of a slot no point of the current call has claimed
constexpr double FM_REACH = 4096.0;      // q < 2^32: 2^31 - 1 pixels sum below 2^63

bool fm_slots_ok(i64 slots) { return fs_slots_ok(slots, FM_MIN_SLOTS, FM_MAX_SLOTS); }

struct FmTable {
    u64* keys;
    int32_t *ids, *first;
    unsigned mask;
};

// ------------------------------------------------------------------------------------------------------------------
// rehash
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FS_THREADS) void k_fm_clear(FmTable tab, i64 slots) {
    const i64 stride = (i64)gridDim.x * FS_THREADS;
    for (i64 s = (i64)blockIdx.x * FS_THREADS + threadIdx.x; s < slots; s += stride) {
        tab.keys[s] = FS_EMPTY;
        tab.ids[s] = -1;
        tab.first[s] = FM_NO_POINT;
    }
}

// the new table holds at least one slot per numbered cell and the keys are distinct: a free slot is always found
__global__ __launch_bounds__(FS_THREADS) void k_fm_move(const u64* __restrict__ old_keys, const int32_t* __restrict__ old_ids,
                                                        i64 old_slots, FmTable tab) {
    const i64 stride = (i64)gridDim.x * FS_THREADS;
    for (i64 s = (i64)blockIdx.x * FS_THREADS + threadIdx.x; s < old_slots; s += stride) {
        const int id = old_ids[s];
        const u64 key = old_keys[s];
        if (id < 0 || key == FS_EMPTY) continue;  // empty, or claimed by a failed insert and never numbered
        unsigned slot = fs_hash(key, tab.mask);
        while (true) {
            u64 old = fs_peek(&tab.keys[slot]);
            if (old == FS_EMPTY) old = atomicCAS(&tab.keys[slot], FS_EMPTY, key);
            if (old == FS_EMPTY) break;  // (old == key cannot happen: the old table holds a key once)
            slot = (slot + 1) & tab.mask;
        }
        tab.ids[slot] = id;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// insert
// ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FS_THREADS) void k_fm_claim(const float* __restrict__ xyz, int n, float cell,
                                                         const float* __restrict__ origin, FmTable tab, int bounded,
                                                         int32_t* __restrict__ slot_of, int32_t* __restrict__ words) {
    const int i = blockIdx.x * FS_THREADS + threadIdx.x;
    if (i >= n) return;
    const float lim = (float)(1 << FM_AXIS_BITS);
    float c[3];
    bool ok = true, within = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float p = xyz[(size_t)i * 3 + a], o = origin[a];
        const float t = __fdiv_rn(p - o, cell);
        c[a] = floorf(t);
        ok = ok && isfinite(t) && c[a] >= 0.0f && c[a] < lim;
        const double e = (double)p - (double)o;
        within = within && e >= 0.0 && e < FM_REACH;
    }
    if (!ok) words[1] = 1;
    if (!within) words[3] = 1;
    if (!ok || !within) {
        slot_of[i] = -1;
        return;
    }
    const u64 key = (u64)(unsigned)c[0] | ((u64)(unsigned)c[1] << FM_AXIS_BITS) | ((u64)(unsigned)c[2] << (2 * FM_AXIS_BITS));
    unsigned slot = fs_hash(key, tab.mask);
    for (int probes = 1;; ++probes) {  // (frames_steps.h, "a key found or claimed")
        u64 old = fs_peek(&tab.keys[slot]);
        if (old == FS_EMPTY) old = atomicCAS(&tab.keys[slot], FS_EMPTY, key);
        if (old == FS_EMPTY || old == key) break;
        if (bounded && probes >= FS_MAX_PROBES) {  // fewer than 2 (M + n) slots: give up, the caller rehashes
            words[2] = 1;
            slot_of[i] = -1;
            return;
        }
        slot = (slot + 1) & tab.mask;  // slots >= 2 (M + n) otherwise: a free slot is always found
    }
    // ids change only in k_fs_emit<FmNumber>, a later launch: a plain read.  The minimum only falls: read first
    if (tab.ids[slot] < 0 && i < fs_peek(&tab.first[slot])) atomicMin(&tab.first[slot], i);
    slot_of[i] = (int)slot;
}

struct FmIsNew {
    const int32_t *slot_of, *ids, *first;
    __device__ bool operator()(int i) const {
        const int slot = slot_of[i];
        return slot >= 0 && ids[slot] < 0 && first[slot] == i;
    }
};

__device__ __forceinline__ bool fm_failed(const int32_t* words) { return (words[1] | words[2] | words[3]) != 0; }

struct FmNumber {
    const int32_t* slot_of;
    int32_t* ids;
    const int32_t* words;
    int M;
    struct State {};
    __device__ bool off() const { return fm_failed(words); }
    __device__ void finish(const State&) const {}
    __device__ void operator()(int i, int rank, State&) const {
        if (rank >= 0) ids[slot_of[i]] = M + rank;  // one writer per slot: the slot's first point
    }
};

__global__ __launch_bounds__(FS_THREADS) void k_fm_cell_of(const int32_t* __restrict__ slot_of, const int32_t* __restrict__ ids,
                                                           int n, const int32_t* __restrict__ words,
                                                           int32_t* __restrict__ cell_of) {
    if (fm_failed(words)) return;
    const int i = blockIdx.x * FS_THREADS + threadIdx.x;
    if (i < n) cell_of[i] = ids[slot_of[i]];  // no flag: every slot_of is a slot, every claimed slot has its number
}

// ------------------------------------------------------------------------------------------------------------------
// accumulate
// ------------------------------------------------------------------------------------------------------------------
// k_fr_sums' body (frames.hip) with the count, kept written out in both: as one inlined function the <true>
// instantiations need 41 VGPRs instead of 32 (see there)
template <bool AGG>
__global__ __launch_bounds__(FS_THREADS) void k_fm_add(const float* __restrict__ xyz, const unsigned char* __restrict__ rgb,
                                                       const int32_t* __restrict__ cell_of, int n, int M,
                                                       const float* __restrict__ origin, int32_t* __restrict__ count,
                                                       i64* __restrict__ sums, int32_t* __restrict__ flag) {
    const int p = blockIdx.x * FS_THREADS + threadIdx.x, lane = threadIdx.x & 63;
    int cell = -1;
    i64 v[6] = {0, 0, 0, 0, 0, 0};
    if (p < n) {
        cell = cell_of[p];
        bool ok = cell >= 0 && cell < M;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double e = (double)xyz[(size_t)p * 3 + a] - (double)origin[a];
            ok = ok && e >= 0.0 && e < FM_REACH;
            v[a] = ok ? (i64)floor(e * FS_UNITS) : 0;
            v[3 + a] = rgb[(size_t)p * 3 + a];
        }
        if (!ok) {
            *flag = 1;
            cell = -1;  // nothing is added for this point
        }
    }
    bool head = true;
    int len = 1;
    if (AGG) {
        // a run: adjacent lanes holding the same cell.  Runs are numbered by their heads, so two runs of one cell with
        // another cell between them stay two runs (each issues its own atomics).  Every lane adds 1 to the count: a
        // run's count is its length, read off the ballot.
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
            const u64 above = (heads >> lane) >> 1;  // the heads after this lane
            len = above ? __ffsll((i64)above) : 64 - lane;
        }
    }
    if (head && cell >= 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) atomicAdd((u64*)&sums[(size_t)cell * 6 + k], (u64)v[k]);
        atomicAdd(&count[cell], len);
    }
}

// an index outside [-1, len) reads nothing, gives -1 and raises the flag
__global__ __launch_bounds__(FS_THREADS) void k_fm_lookup(const int32_t* __restrict__ index, i64 T,
                                                          const int32_t* __restrict__ table, int len, int32_t* __restrict__ out,
                                                          int32_t* __restrict__ flag) {
    const i64 t = (i64)blockIdx.x * FS_THREADS + threadIdx.x;
    if (t >= T) return;
    const int p = index[t];
    const bool in = p >= 0 && p < len;
    out[t] = in ? table[p] : -1;
    if (!in && p != -1 && flag) *flag = 1;
}

}  // namespace

extern "C" int gf_frames_map_max_probes(void) { return FS_MAX_PROBES; }
extern "C" double gf_frames_map_reach(void) { return FM_REACH; }
extern "C" long long gf_frames_map_max_pixels(void) { return FM_MAX_PIXELS; }

extern "C" long long gf_frames_map_default_slots(long long M, long long T) {
    if (M < 0 || M > FM_MAX_PIXELS || T < 0 || T > FM_MAX_PIXELS) return 0;
    return fs_default_slots(M, T, FM_MIN_SLOTS, FM_MAX_SLOTS);
}

extern "C" int gf_frames_map_rehash(const unsigned long long* old_keys, const int32_t* old_ids, long long old_slots, int cells,
                                    unsigned long long* new_keys, int32_t* new_ids, int32_t* new_first, long long new_slots,
                                    void* stream) {
    GF_CHECK_ARG(old_slots == 0 || fm_slots_ok(old_slots),
                 "gf_frames_map_rehash: old_slots = %lld (0, or a power of two from %lld to %lld)", old_slots, FM_MIN_SLOTS,
                 FM_MAX_SLOTS);
    GF_CHECK_ARG(fm_slots_ok(new_slots), "gf_frames_map_rehash: new_slots = %lld (a power of two from %lld to %lld)", new_slots,
                 FM_MIN_SLOTS, FM_MAX_SLOTS);
    GF_CHECK_ARG(cells >= 0 && (i64)cells <= new_slots && (old_slots > 0 || cells == 0),
                 "gf_frames_map_rehash: %d numbered cells into %lld slots (at least one slot per cell)", cells, new_slots);
    GF_CHECK_ARG(new_keys && new_ids && new_first && (old_slots == 0 || (old_keys && old_ids)),
                 "gf_frames_map_rehash: NULL old_keys, old_ids, new_keys, new_ids or new_first");
    GF_CHECK_ARG(old_slots == 0 || (old_keys != new_keys && old_ids != new_ids), "gf_frames_map_rehash: the tables overlap");
    hipStream_t st = (hipStream_t)stream;
    const FmTable tab = {new_keys, new_ids, new_first, (unsigned)(new_slots - 1)};
    hipLaunchKernelGGL(k_fm_clear, dim3(fs_blocks(new_slots, 4096)), dim3(FS_THREADS), 0, st, tab, (i64)new_slots);
    if (old_slots > 0 && cells > 0)
        hipLaunchKernelGGL(k_fm_move, dim3(fs_blocks(old_slots, 4096)), dim3(FS_THREADS), 0, st, old_keys, old_ids,
                           (i64)old_slots, tab);
    GF_CHECK_LAUNCH("gf_frames_map_rehash");
    return GF_OK;
}

extern "C" size_t gf_frames_map_insert_scratch_bytes(int n, int chunk) {
    if (n < 0 || n > FS_MAX_POINTS || !fs_chunk_ok(chunk)) return 0;
    return (size_t)(n + 2) / 2 * 8 + fs_scan_bytes(n, chunk ? chunk : FS_CHUNK);  // slot_of [n] (8-byte granules), the scan
}

extern "C" int gf_frames_map_insert(const float* xyz, int n, float cell, const float* origin, unsigned long long* keys,
                                    int32_t* ids, int32_t* first, long long slots, int M, int chunk, void* scratch,
                                    int32_t* cell_of, int32_t* d_words, void* stream) {
    GF_CHECK_ARG(n >= 0 && n <= FS_MAX_POINTS && gf_resample_max_points() == FS_MAX_POINTS,
                 "gf_frames_map_insert: n = %d points (0 to %d)", n, FS_MAX_POINTS);
    GF_CHECK_ARG(M >= 0 && (i64)M + n <= FM_MAX_PIXELS,
                 "gf_frames_map_insert: M = %d cells and n = %d points (M >= 0, M + n <= %lld)", M, n, FM_MAX_PIXELS);
    GF_CHECK_ARG(cell > 0.0f && cell <= 3.402823466e38f, "gf_frames_map_insert: cell = %g (positive and finite)", (double)cell);
    GF_CHECK_ARG(fm_slots_ok(slots), "gf_frames_map_insert: slots = %lld (a power of two from %lld to %lld)", slots, FM_MIN_SLOTS,
                 FM_MAX_SLOTS);
    GF_CHECK_ARG(fs_chunk_ok(chunk), "gf_frames_map_insert: chunk = %d (0, or a multiple of 64 from 64 to %d)", chunk,
                 FS_MAX_CHUNK);
    if (n == 0) return GF_OK;
    GF_CHECK_ARG(xyz && origin && keys && ids && first && scratch && cell_of && d_words,
                 "gf_frames_map_insert: NULL xyz, origin, keys, ids, first, scratch, cell_of or d_words");
    hipStream_t st = (hipStream_t)stream;
    if (!chunk) chunk = FS_CHUNK;
    const FmTable tab = {keys, ids, first, (unsigned)(slots - 1)};
    int32_t* slot_of = (int32_t*)scratch;
    void* rest = (char*)scratch + (size_t)(n + 2) / 2 * 8;
    const int bounded = slots < 2 * ((i64)M + n), g = gf_div_up(n, FS_THREADS);
    GF_TRY(hipMemsetAsync(d_words, 0, 4 * 4, st));
    hipLaunchKernelGGL(k_fm_claim, dim3(g), dim3(FS_THREADS), 0, st, xyz, n, cell, origin, tab, bounded, slot_of, d_words);
    fs_compact(FmIsNew{slot_of, ids, first}, FmNumber{slot_of, ids, d_words, M}, n, chunk, rest, M, d_words, st);
    hipLaunchKernelGGL(k_fm_cell_of, dim3(g), dim3(FS_THREADS), 0, st, slot_of, ids, n, d_words, cell_of);
    GF_CHECK_LAUNCH("gf_frames_map_insert");
    return GF_OK;
}

extern "C" int gf_frames_map_accumulate(const float* xyz, const unsigned char* rgb, const int32_t* cell_of, int n, int M,
                                        const float* origin, int aggregate, int32_t* count, long long* sums, int32_t* d_flag,
                                        void* stream) {
    GF_CHECK_ARG(n >= 0 && n <= FS_MAX_POINTS, "gf_frames_map_accumulate: n = %d points (0 to %d)", n, FS_MAX_POINTS);
    if (n == 0) return GF_OK;
    GF_CHECK_ARG(M >= 1, "gf_frames_map_accumulate: M = %d cells (>= 1)", M);
    GF_CHECK_ARG(xyz && rgb && cell_of && origin && count && sums && d_flag,
                 "gf_frames_map_accumulate: NULL xyz, rgb, cell_of, origin, count, sums or d_flag");
    hipStream_t st = (hipStream_t)stream;
    if (aggregate)
        hipLaunchKernelGGL(k_fm_add<true>, dim3(gf_div_up(n, FS_THREADS)), dim3(FS_THREADS), 0, st, xyz, rgb, cell_of, n, M,
                           origin, count, sums, d_flag);
    else
        hipLaunchKernelGGL(k_fm_add<false>, dim3(gf_div_up(n, FS_THREADS)), dim3(FS_THREADS), 0, st, xyz, rgb, cell_of, n, M,
                           origin, count, sums, d_flag);
    GF_CHECK_LAUNCH("gf_frames_map_accumulate");
    return GF_OK;
}

extern "C" size_t gf_frames_map_means_scratch_bytes(int M, int chunk) {
    if (M < 1 || M > FM_MAX_CELLS || !fs_chunk_ok(chunk)) return 0;
    return fs_scan_bytes(M, chunk ? chunk : FS_CHUNK);
}

extern "C" int gf_frames_map_means(const int32_t* count, const long long* sums, int M, const float* origin, int min_obs,
                                   int chunk, void* scratch, float* xyz_out, unsigned char* rgb_out, int32_t* count_out,
                                   int32_t* new_id, int32_t* d_m, void* stream) {
    GF_CHECK_ARG(M >= 1 && M <= FM_MAX_CELLS, "gf_frames_map_means: M = %d cells (1 to %d)", M, FM_MAX_CELLS);
    GF_CHECK_ARG(min_obs >= 1, "gf_frames_map_means: min_obs = %d (>= 1)", min_obs);
    GF_CHECK_ARG(fs_chunk_ok(chunk), "gf_frames_map_means: chunk = %d (0, or a multiple of 64 from 64 to %d)", chunk, FS_MAX_CHUNK);
    GF_CHECK_ARG(count && sums && origin && scratch && xyz_out && rgb_out && count_out && new_id && d_m,
                 "gf_frames_map_means: NULL pointer");
    if (!chunk) chunk = FS_CHUNK;
    fs_compact(FsKept{count, min_obs}, FsMean{sums, count, origin, xyz_out, rgb_out, count_out, new_id}, M, chunk, scratch, 0, d_m,
               (hipStream_t)stream);
    GF_CHECK_LAUNCH("gf_frames_map_means");
    return GF_OK;
}

extern "C" int gf_frames_map_lookup(const int32_t* index, long long T, const int32_t* table, int len, int32_t* out,
                                    int32_t* d_flag, void* stream) {
    GF_CHECK_ARG(T >= 0 && len >= 0, "gf_frames_map_lookup: T = %lld elements, a table of %d (each >= 0)", T, len);
    if (T == 0) return GF_OK;
    GF_CHECK_ARG(index && table && out, "gf_frames_map_lookup: NULL index, table or out");
    GF_CHECK_ARG((T + FS_THREADS - 1) / FS_THREADS <= 2147483647ll,
                 "gf_frames_map_lookup: T = %lld elements (too many for one launch)", T);
    hipLaunchKernelGGL(k_fm_lookup, dim3((unsigned)((T + FS_THREADS - 1) / FS_THREADS)), dim3(FS_THREADS), 0, (hipStream_t)stream,
                       index, (i64)T, table, len, out, d_flag);
    GF_CHECK_LAUNCH("gf_frames_map_lookup");
    return GF_OK;
}
