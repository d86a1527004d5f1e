// Votes that persist between calls: the pair table of gf_frames_vote kept by the caller, fed one chunk of
// elements at a time.  The host statement is frames.VoterHost; see include/geoformer_hip.h for the arguments and the
// state (all of it owned by the caller: keys uint64 [slots], all ones = empty, and cnt uint32 [slots]).
//
// gf_frames_votes_add      one memset of the two words, then
//   k_vs_claim<AGG>        one thread per sampled element: gf_frames_vote's key group << 32 | value with the same strided
//                          read of the full-resolution image; with AGG only the head lane of a run of equal keys among
//                          adjacent lanes goes on, its run length read off the one ballot of the heads.  The key is found
//                          or claimed (slot read first, 64-bit CAS on an empty slot only).  The head's slot and its add go
//                          to a per-element scratch; NO count is touched.  The claims that won their CAS are counted by
//                          ballot, summed in LDS, one atomic per workgroup on d_words[0]; a thread that runs out of probes
//                          (bounded regime) sets d_words[1]
//   k_vs_commit            reads d_words[1] first and returns when it is set (every thread reads the same word: the
//                          branch is uniform); otherwise every recorded head adds its run length to cnt[slot].  No probing.
// gf_frames_votes_rehash   k_vs_clear (keys all ones, cnt 0), k_vs_move (every old slot with cnt > 0: key claimed in the
//                          new table by CAS, count copied)
// gf_frames_votes_pick     one memset of the scratch (best, total, two words), then k_vs_pick (k_fv_pick over the
//                          persistent table: slots with cnt == 0 skipped, a group >= n raises a word instead of writing)
//                          and k_vs_write (label, votes and total per group; the two words copied out)
//
// A failed add.  Claiming and counting are two launches so that an add that overflows its table changes no count: what
// it leaves are claimed keys with cnt == 0.  Such a slot is debris: k_vs_pick and k_vs_move treat cnt == 0 as absent, and
// no count of pairs includes it.  A successful add leaves none: every claimed key belongs to a head that adds >= 1.
//
// Termination (frames_steps.h, "a key found or claimed").  k_vs_claim is unbounded with slots >= 2 (P + T) (P: the
// occupied slots before the call, T: this call's elements).  k_vs_move: the new table has at least one slot per moved
// pair and the keys are distinct.  No thread waits for another thread or workgroup; there is no spin.  Integer atomics
// and an integer maximum only.
#include "common.h"
#include "frames_steps.h"

namespace {

constexpr i64 VS_MIN_SLOTS = 64;
constexpr i64 VS_MAX_SLOTS = 1ll << 31;  // a slot is recorded as a non-negative int32; >= 2 (P + T) up to P + T = 2^30
constexpr i64 VS_MAX_ELEMENTS = 2147483647ll;  // offered in all: every count and total fits an int32
constexpr i64 VS_MAX_GROUPS = 2147483647ll;
constexpr int VS_PICK_BLOCKS = 1024;  // the workgroups that stride over the table in k_vs_pick

bool vs_slots_ok(i64 slots) { return fs_slots_ok(slots, VS_MIN_SLOTS, VS_MAX_SLOTS); }

struct VsInput {
    const int32_t* group;  // [F, Hs, Ws]
    const void* value;     // [F, H, W], read at (j0 stride, i0 stride)
    int kind, W, H, Ws, Hs, stride, T, ignore, has_ignore;
};

struct VsHead {  // what an element leaves for the commit pass
    int32_t slot;  // the slot of a head lane's key, -1 for every other element
    unsigned add;  // its run length
};

// T <= 2^29: every index of a sampled element fits an int; the value image is addressed in 64 bits
template <bool AGG>
__global__ __launch_bounds__(FS_THREADS) void k_vs_claim(VsInput in, u64* __restrict__ keys, unsigned mask, int bounded,
                                                         VsHead* __restrict__ heads_out, int32_t* __restrict__ words) {
    __shared__ int s_new[FS_THREADS / 64];
    const int t = blockIdx.x * FS_THREADS + threadIdx.x, lane = threadIdx.x & 63;
    u64 key = FS_EMPTY;
    if (t < in.T) {
        const int g = in.group[t];
        // k_fv_insert's key (frames_vote.hip), kept written out in both: through one inlined function either kernel
        // comes out 1 to 4 lines longer
        if (g >= 0) {
            size_t at = (size_t)t;
            if (in.stride != 1) {  // (stride 1: H = Hs and W = Ws, the sampled element is the element)
                const int per = in.Hs * in.Ws, r = t % per;
                at = ((size_t)(t / per) * in.H + (size_t)(r / in.Ws) * in.stride) * in.W + (size_t)(r % in.Ws) * in.stride;
            }
            i64 v;
            if (in.kind == 0)
                v = ((const unsigned char*)in.value)[at];
            else if (in.kind == 1)
                v = ((const unsigned short*)in.value)[at];
            else
                v = ((const int32_t*)in.value)[at];
            if (v >= 0 && !(in.has_ignore && v == (i64)in.ignore)) key = ((u64)(unsigned)g << 32) | (u64)(unsigned)v;
        }
    }
    unsigned add = 1;
    bool go = key != FS_EMPTY;  // (lanes without a vote form runs of FS_EMPTY, dropped here)
    if (AGG) {
        // fs_run, kept written out (through the helper the same 362 lines come out with other registers and order)
        const u64 left = __shfl_up(key, 1, 64);
        const bool head = lane == 0 || left != key;
        const u64 heads = __ballot(head);
        const u64 above = (heads >> lane) >> 1;  // the heads after this lane
        add = above ? (unsigned)__ffsll((i64)above) : (unsigned)(64 - lane);
        go = go && head;
    }
    int slot = -1;
    bool won = false;
    if (go) {
        unsigned s = fs_hash(key, mask);
        for (int probes = 1;; ++probes) {  // (frames_steps.h, "a key found or claimed")
            u64 old = fs_peek(&keys[s]);
            if (old == FS_EMPTY) {
                old = atomicCAS(&keys[s], FS_EMPTY, key);
                won = old == FS_EMPTY;
            }
            if (won || old == key) {
                slot = (int)s;
                break;
            }
            if (bounded && probes >= FS_MAX_PROBES) {  // fewer than 2 (P + T) slots: give up, the commit writes nothing
                words[1] = 1;
                break;
            }
            s = (s + 1) & mask;  // slots >= 2 (P + T) otherwise: a free slot is always found
        }
    }
    if (t < in.T) heads_out[t] = VsHead{slot, add};
    // the new pairs: one atomic per workgroup on their one word (k_fv_pick's comment records what one per wave cost)
    const int mine = __popcll(__ballot(won));
    if (lane == 0) s_new[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int p = 0;
#pragma unroll
        for (int w = 0; w < FS_THREADS / 64; ++w) p += s_new[w];
        if (p) atomicAdd(&words[0], p);
    }
}

__global__ __launch_bounds__(FS_THREADS) void k_vs_commit(const VsHead* __restrict__ heads, int T, unsigned* __restrict__ cnt,
                                                          const int32_t* __restrict__ words) {
    if (words[1]) return;  // the claim pass overflowed: no count changes (the same word for every thread)
    const int t = blockIdx.x * FS_THREADS + threadIdx.x;
    if (t >= T) return;
    const VsHead h = heads[t];
    if (h.slot >= 0) atomicAdd(&cnt[h.slot], h.add);
}

__global__ __launch_bounds__(FS_THREADS) void k_vs_clear(u64* __restrict__ keys, unsigned* __restrict__ cnt, i64 slots) {
    const i64 stride = (i64)gridDim.x * FS_THREADS;
    for (i64 s = (i64)blockIdx.x * FS_THREADS + threadIdx.x; s < slots; s += stride) {
        keys[s] = FS_EMPTY;
        cnt[s] = 0;
    }
}

// the new table holds at least one slot per moved pair and the keys are distinct: a free slot is always found
__global__ __launch_bounds__(FS_THREADS) void k_vs_move(const u64* __restrict__ old_keys, const unsigned* __restrict__ old_cnt,
                                                        i64 old_slots, u64* __restrict__ keys, unsigned* __restrict__ cnt,
                                                        unsigned mask) {
    const i64 stride = (i64)gridDim.x * FS_THREADS;
    for (i64 s = (i64)blockIdx.x * FS_THREADS + threadIdx.x; s < old_slots; s += stride) {
        const unsigned c = old_cnt[s];
        const u64 key = old_keys[s];
        if (c == 0 || key == FS_EMPTY) continue;  // empty, or claimed by a failed add and never counted
        unsigned slot = fs_hash(key, mask);
        while (true) {
            u64 old = fs_peek(&keys[slot]);
            if (old == FS_EMPTY) old = atomicCAS(&keys[slot], FS_EMPTY, key);
            if (old == FS_EMPTY) break;  // (old == key cannot happen: the old table holds a key once)
            slot = (slot + 1) & mask;
        }
        cnt[slot] = c;
    }
}

struct VsPick {
    u64* best;       // [n]
    int32_t* total;  // [n]
    int32_t* words;  // {pairs, group out of range}
};
size_t vs_pick_bytes(i64 n) { return (size_t)n * 12 + 64; }
VsPick vs_carve(void* scratch, i64 n) {
    VsPick p;
    p.best = (u64*)scratch;
    p.total = (int32_t*)(p.best + n);
    p.words = p.total + n;
    return p;
}

// At most VS_PICK_BLOCKS workgroups stride over the table, so the pairs are counted with at most that many atomics on
// their one word.  slots and the stride are multiples of 64: a wave is inside the table or outside it as a whole.
__global__ __launch_bounds__(FS_THREADS) void k_vs_pick(const u64* __restrict__ keys, const unsigned* __restrict__ cnt, i64 slots,
                                                        i64 n, VsPick out) {
    __shared__ int s_pairs[FS_THREADS / 64];
    const i64 stride = (i64)gridDim.x * FS_THREADS;
    int pairs = 0;
    for (i64 s = (i64)blockIdx.x * FS_THREADS + threadIdx.x; s < slots; s += stride) {
        const u64 key = keys[s];
        const unsigned c = cnt[s];
        const bool live = key != FS_EMPTY && c > 0;  // cnt == 0: the debris of a failed add
        pairs += __popcll(__ballot(live));
        if (live) {
            const i64 g = (i64)(key >> 32);
            if (g >= n) {
                out.words[1] = 1;
            } else {
                atomicAdd(&out.total[g], (int)c);
                const u64 mine = ((u64)c << 32) | (u64)(0xffffffffu - (unsigned)key);
                if (mine > fs_peek(&out.best[g])) atomicMax(&out.best[g], mine);  // the word only rises
            }
        }
    }
    if ((threadIdx.x & 63) == 0) s_pairs[threadIdx.x >> 6] = pairs;
    __syncthreads();
    if (threadIdx.x == 0) {
        int p = 0;
#pragma unroll
        for (int w = 0; w < FS_THREADS / 64; ++w) p += s_pairs[w];
        if (p) atomicAdd(&out.words[0], p);
    }
}

__global__ __launch_bounds__(FS_THREADS) void k_vs_write(VsPick in, i64 n, int fill, int32_t* __restrict__ label,
                                                         int32_t* __restrict__ votes, int32_t* __restrict__ total,
                                                         int32_t* __restrict__ words) {
    const i64 g = (i64)blockIdx.x * FS_THREADS + threadIdx.x;
    if (g < 2) words[g] = in.words[g];  // (n >= 1: the first workgroup exists)
    if (g >= n) return;
    const u64 b = in.best[g];  // 0: no vote (a count is at least 1)
    label[g] = b ? (int32_t)(0xffffffffu - (unsigned)b) : fill;
    votes[g] = (int32_t)(b >> 32);
    total[g] = in.total[g];
}

struct VsShape {
    int Ws, Hs;
    i64 T;
};

}  // namespace

extern "C" int gf_frames_votes_max_probes(void) { return FS_MAX_PROBES; }
extern "C" long long gf_frames_votes_max_elements(void) { return VS_MAX_ELEMENTS; }

extern "C" long long gf_frames_votes_default_slots(long long P, long long T) {
    if (P < 0 || P > VS_MAX_ELEMENTS || T < 0 || T > VS_MAX_ELEMENTS) return 0;
    return fs_default_slots(P, T, VS_MIN_SLOTS, VS_MAX_SLOTS);
}

extern "C" size_t gf_frames_votes_add_scratch_bytes(long long T) {
    if (T < 0 || T > FS_MAX_POINTS) return 0;
    return (size_t)T * sizeof(VsHead) + 64;
}

extern "C" size_t gf_frames_votes_pick_scratch_bytes(long long n) {
    if (n < 0 || n > VS_MAX_GROUPS) return 0;
    return vs_pick_bytes(n);
}

// the checks gf_frames_votes_add, _claim and _commit share; *T_out: the sampled elements
static int vs_check_add(const char* who, int kind, int F, int W, int H, int stride, long long slots, long long pairs,
                        VsShape* shape) {
    GF_CHECK_ARG(F >= 0 && W >= 0 && H >= 0, "%s: %d images of %d x %d (each >= 0)", who, F, W, H);
    GF_CHECK_ARG(stride >= 1, "%s: stride = %d (>= 1)", who, stride);
    GF_CHECK_ARG(kind >= 0 && kind <= 2, "%s: kind = %d (0 uint8, 1 uint16, 2 int32)", who, kind);
    const int Ws = gf_div_up(W, stride), Hs = gf_div_up(H, stride);
    const long long per = (long long)Hs * Ws;  // below 2^62
    GF_CHECK_ARG(per <= FS_MAX_POINTS && per * F <= FS_MAX_POINTS && gf_resample_max_points() == FS_MAX_POINTS,
                 "%s: %d x %d x %d sampled elements (at most %d)", who, F, Hs, Ws, FS_MAX_POINTS);
    GF_CHECK_ARG(vs_slots_ok(slots), "%s: slots = %lld (a power of two from %lld to %lld)", who, slots, VS_MIN_SLOTS,
                 VS_MAX_SLOTS);
    GF_CHECK_ARG(pairs >= 0 && pairs <= slots && pairs + per * F <= VS_MAX_ELEMENTS,
                 "%s: pairs = %lld in %lld slots before %lld elements (0 <= pairs <= slots, pairs + elements <= %lld)", who,
                 pairs, slots, per * F, VS_MAX_ELEMENTS);
    shape->Ws = Ws;
    shape->Hs = Hs;
    shape->T = per * F;
    return GF_OK;
}

extern "C" int gf_frames_votes_claim(const int32_t* group, const void* value, int kind, int F, int W, int H, int stride,
                                     int ignore, int has_ignore, unsigned long long* keys, long long slots, long long pairs,
                                     int aggregate, void* scratch, int32_t* d_words, void* stream) {
    VsShape sh;
    const int rc = vs_check_add("gf_frames_votes_claim", kind, F, W, H, stride, slots, pairs, &sh);
    if (rc != GF_OK) return rc;
    if (sh.T == 0) return GF_OK;
    GF_CHECK_ARG(group && value && keys && scratch && d_words, "gf_frames_votes_claim: NULL group, value, keys, scratch or d_words");
    hipStream_t st = (hipStream_t)stream;
    const VsInput in = {group, value, kind, W, H, sh.Ws, sh.Hs, stride, (int)sh.T, ignore, has_ignore != 0};
    const int bounded = slots < 2 * (pairs + sh.T), g = gf_div_up(sh.T, FS_THREADS);
    GF_TRY(hipMemsetAsync(d_words, 0, 2 * 4, st));
    if (aggregate)
        hipLaunchKernelGGL(k_vs_claim<true>, dim3(g), dim3(FS_THREADS), 0, st, in, keys, (unsigned)(slots - 1), bounded,
                           (VsHead*)scratch, d_words);
    else
        hipLaunchKernelGGL(k_vs_claim<false>, dim3(g), dim3(FS_THREADS), 0, st, in, keys, (unsigned)(slots - 1), bounded,
                           (VsHead*)scratch, d_words);
    GF_CHECK_LAUNCH("gf_frames_votes_claim");
    return GF_OK;
}

extern "C" int gf_frames_votes_commit(const void* scratch, long long T, uint32_t* cnt, long long slots, const int32_t* d_words,
                                      void* stream) {
    GF_CHECK_ARG(T >= 0 && T <= FS_MAX_POINTS, "gf_frames_votes_commit: T = %lld elements (0 to %d)", T, FS_MAX_POINTS);
    GF_CHECK_ARG(vs_slots_ok(slots), "gf_frames_votes_commit: slots = %lld (a power of two from %lld to %lld)", slots,
                 VS_MIN_SLOTS, VS_MAX_SLOTS);
    if (T == 0) return GF_OK;
    GF_CHECK_ARG(scratch && cnt && d_words, "gf_frames_votes_commit: NULL scratch, cnt or d_words");
    hipLaunchKernelGGL(k_vs_commit, dim3(gf_div_up(T, FS_THREADS)), dim3(FS_THREADS), 0, (hipStream_t)stream,
                       (const VsHead*)scratch, (int)T, cnt, d_words);
    GF_CHECK_LAUNCH("gf_frames_votes_commit");
    return GF_OK;
}

extern "C" int gf_frames_votes_add(const int32_t* group, const void* value, int kind, int F, int W, int H, int stride,
                                   int ignore, int has_ignore, unsigned long long* keys, uint32_t* cnt, long long slots,
                                   long long pairs, int aggregate, void* scratch, int32_t* d_words, void* stream) {
    VsShape sh;
    int rc = vs_check_add("gf_frames_votes_add", kind, F, W, H, stride, slots, pairs, &sh);
    if (rc != GF_OK) return rc;
    if (sh.T == 0) return GF_OK;
    GF_CHECK_ARG(group && value && keys && cnt && scratch && d_words,
                 "gf_frames_votes_add: NULL group, value, keys, cnt, scratch or d_words");
    rc = gf_frames_votes_claim(group, value, kind, F, W, H, stride, ignore, has_ignore, keys, slots, pairs, aggregate, scratch,
                               d_words, stream);
    if (rc != GF_OK) return rc;
    return gf_frames_votes_commit(scratch, sh.T, cnt, slots, d_words, stream);
}

extern "C" int gf_frames_votes_rehash(const unsigned long long* old_keys, const uint32_t* old_cnt, long long old_slots,
                                      long long pairs, unsigned long long* new_keys, uint32_t* new_cnt, long long new_slots,
                                      void* stream) {
    GF_CHECK_ARG(old_slots == 0 || vs_slots_ok(old_slots),
                 "gf_frames_votes_rehash: old_slots = %lld (0, or a power of two from %lld to %lld)", old_slots, VS_MIN_SLOTS,
                 VS_MAX_SLOTS);
    GF_CHECK_ARG(vs_slots_ok(new_slots), "gf_frames_votes_rehash: new_slots = %lld (a power of two from %lld to %lld)", new_slots,
                 VS_MIN_SLOTS, VS_MAX_SLOTS);
    GF_CHECK_ARG(pairs >= 0 && pairs <= new_slots && (old_slots > 0 || pairs == 0),
                 "gf_frames_votes_rehash: %lld stored pairs into %lld slots (at least one slot per pair)", pairs, new_slots);
    GF_CHECK_ARG(new_keys && new_cnt && (old_slots == 0 || (old_keys && old_cnt)),
                 "gf_frames_votes_rehash: NULL old_keys, old_cnt, new_keys or new_cnt");
    GF_CHECK_ARG(old_slots == 0 || (old_keys != new_keys && old_cnt != new_cnt), "gf_frames_votes_rehash: the tables overlap");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_vs_clear, dim3(fs_blocks(new_slots, 4096)), dim3(FS_THREADS), 0, st, new_keys, new_cnt, (i64)new_slots);
    if (old_slots > 0 && pairs > 0)
        hipLaunchKernelGGL(k_vs_move, dim3(fs_blocks(old_slots, 4096)), dim3(FS_THREADS), 0, st, old_keys, old_cnt, (i64)old_slots,
                           new_keys, new_cnt, (unsigned)(new_slots - 1));
    GF_CHECK_LAUNCH("gf_frames_votes_rehash");
    return GF_OK;
}

extern "C" int gf_frames_votes_pick(const unsigned long long* keys, const uint32_t* cnt, long long slots, long long n, int fill,
                                    void* scratch, int32_t* label, int32_t* votes, int32_t* total, int32_t* d_words,
                                    void* stream) {
    GF_CHECK_ARG(vs_slots_ok(slots), "gf_frames_votes_pick: slots = %lld (a power of two from %lld to %lld)", slots, VS_MIN_SLOTS,
                 VS_MAX_SLOTS);
    GF_CHECK_ARG(n >= 0 && n <= VS_MAX_GROUPS, "gf_frames_votes_pick: n = %lld groups (0 to %lld)", n, VS_MAX_GROUPS);
    if (n == 0) return GF_OK;
    GF_CHECK_ARG(keys && cnt && scratch && label && votes && total && d_words,
                 "gf_frames_votes_pick: NULL keys, cnt, scratch, label, votes, total or d_words");
    hipStream_t st = (hipStream_t)stream;
    const VsPick p = vs_carve(scratch, n);
    GF_TRY(hipMemsetAsync(scratch, 0, vs_pick_bytes(n), st));
    hipLaunchKernelGGL(k_vs_pick, dim3(fs_blocks(slots, VS_PICK_BLOCKS)), dim3(FS_THREADS), 0, st, keys, cnt, (i64)slots, (i64)n, p);
    hipLaunchKernelGGL(k_vs_write, dim3((unsigned)((n + FS_THREADS - 1) / FS_THREADS)), dim3(FS_THREADS), 0, st, p, (i64)n, fill,
                       label, votes, total, d_words);
    GF_CHECK_LAUNCH("gf_frames_votes_pick");
    return GF_OK;
}
