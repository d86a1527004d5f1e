// Per-pixel labels lifted onto fused points by majority vote.  The host statement is frames.vote_host; see
// include/geoformer_hip.h for the arguments and the rule.
//
// gf_frames_vote: four memsets and three launches on the caller's stream, nothing read back:
//   k_fv_insert<AGG>  one thread per sampled pixel: the pair (group, value) as the key group << 32 | value, claimed in an
//                     open-addressing table by 64-bit CAS (k_rs_insert's pattern: the slot is read first and the CAS
//                     issued only on an empty one), then an integer atomicAdd on the slot's count.  With AGG a run of
//                     adjacent lanes holding one key adds once: every lane contributes 1, so a run's sum is its length,
//                     which its head lane reads off the one ballot of the heads -- no exchange between the lanes at all.
//   k_fv_pick         the slots dealt over at most 1024 workgroups: a claimed slot adds its count to total[group] and
//                     offers count << 32 | (0xffffffff - value) to a 64-bit atomicMax on best[group] (read first): the
//                     largest count wins, ties go to the smallest value; the claimed slots are counted by ballot, summed
//                     in registers and LDS, one atomic per workgroup
//   k_fv_write        one thread per group: label and votes decoded from best
// Integer counts, an integer maximum: no result depends on the order in which the pixels arrive.
//
// Termination and the "read first" argument: frames_steps.h, "a key found or claimed".  k_fv_insert is unbounded with
// slots >= 2 T: the table holds at most T distinct pairs.  With fewer slots (`bounded`) a thread that gives up raises the
// overflow word and returns.  No thread ever waits for another.
#include "common.h"
#include "frames_steps.h"

namespace {

constexpr int FV_MIN_SLOTS = 64;
constexpr int FV_MAX_SLOTS = 1 << 30;   // 2 T at T = 2^29
constexpr int FV_PICK_BLOCKS = 1024;    // the workgroups that stride over the table in k_fv_pick

struct FvTable {
    u64* keys;      // [slots]
    unsigned* cnt;  // [slots]
    u64* best;      // [n]
};
// keys, then cnt and best side by side (one memset of zeros); slots is a multiple of 64, so best is 8-byte aligned
size_t fv_scratch_bytes(i64 slots, i64 n) { return (size_t)slots * 12 + (size_t)n * 8 + 64; }
FvTable fv_carve(void* scratch, i64 slots) {
    FvTable t;
    t.keys = (u64*)scratch;
    t.cnt = (unsigned*)(t.keys + slots);
    t.best = (u64*)(t.cnt + slots);
    return t;
}
bool fv_slots_ok(i64 slots) { return fs_slots_ok(slots, FV_MIN_SLOTS, FV_MAX_SLOTS); }

struct FvInput {
    const int32_t* group;  // [F, Hs, Ws]
    const void* value;     // [F, H, W], read at (j0 stride, i0 stride)
    int kind, W, H, Ws, Hs, stride, T, n, ignore, has_ignore;
};

// T <= 2^29: every index of a sampled pixel fits an int; the value image is addressed in 64 bits
template <bool AGG>
__global__ __launch_bounds__(FS_THREADS) void k_fv_insert(FvInput in, FvTable tab, unsigned mask, int bounded,
                                                          int32_t* __restrict__ words) {
    const int t = blockIdx.x * FS_THREADS + threadIdx.x, lane = threadIdx.x & 63;
    u64 key = FS_EMPTY;
    if (t < in.T) {
        const int g = in.group[t];
        if (g >= in.n) words[2] = 1;
        // the key, as in k_vs_claim (frames_vote_stream.hip), kept written out in both: through one inlined function
        // either kernel comes out 1 to 4 lines longer
        if (g >= 0 && g < in.n) {
            size_t at = (size_t)t;
            if (in.stride != 1) {  // (stride 1: H = Hs and W = Ws, the sampled pixel is the pixel)
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
    if (AGG) {
        // fs_run, kept written out (through the helper the kernel is one line longer): only the head of a run of equal
        // keys goes on (lanes without a vote form runs of FS_EMPTY, dropped below)
        const u64 left = __shfl_up(key, 1, 64);
        const bool head = lane == 0 || left != key;
        const u64 heads = __ballot(head);
        if (!head) return;
        const u64 above = (heads >> lane) >> 1;  // the heads after this lane
        add = above ? (unsigned)__ffsll((i64)above) : (unsigned)(64 - lane);
    }
    if (key == FS_EMPTY) return;
    unsigned slot = fs_hash(key, mask);
    for (int probes = 1;; ++probes) {  // (frames_steps.h, "a key found or claimed")
        u64 old = fs_peek(&tab.keys[slot]);
        if (old == FS_EMPTY) old = atomicCAS(&tab.keys[slot], FS_EMPTY, key);
        if (old == FS_EMPTY || old == key) break;
        if (bounded && probes >= FS_MAX_PROBES) {  // fewer than 2 T slots: give up, the caller discards the outputs
            words[1] = 1;
            return;
        }
        slot = (slot + 1) & mask;  // slots >= 2 T otherwise: a free slot is always found
    }
    atomicAdd(&tab.cnt[slot], add);
}

// At most FV_PICK_BLOCKS workgroups stride over the table, so the pairs are counted with at most that many atomics on
// their one word (one per wave of the table -- 32 768 on one address at 2^21 slots -- made this kernel 371 us, not 25).
// slots and the stride are multiples of 64: a wave is inside the table or outside it as a whole, in every round.
__global__ __launch_bounds__(FS_THREADS) void k_fv_pick(FvTable tab, unsigned slots, int32_t* __restrict__ total,
                                                        int32_t* __restrict__ words) {
    __shared__ int s_pairs[FS_THREADS / 64];
    const unsigned stride = gridDim.x * FS_THREADS;  // <= 2^18, slots <= 2^30: s + stride fits
    int pairs = 0;
    for (unsigned s = blockIdx.x * FS_THREADS + threadIdx.x; s < slots; s += stride) {
        const u64 key = tab.keys[s];
        const bool claimed = key != FS_EMPTY;
        pairs += __popcll(__ballot(claimed));
        if (claimed) {
            const unsigned g = (unsigned)(key >> 32), c = tab.cnt[s];  // g < n: checked before the key was made
            atomicAdd(&total[g], (int)c);
            const u64 mine = ((u64)c << 32) | (u64)(0xffffffffu - (unsigned)key);
            if (mine > fs_peek(&tab.best[g])) atomicMax(&tab.best[g], mine);  // the word only rises
        }
    }
    if ((threadIdx.x & 63) == 0) s_pairs[threadIdx.x >> 6] = pairs;
    __syncthreads();
    if (threadIdx.x == 0) {
        int p = 0;
#pragma unroll
        for (int w = 0; w < FS_THREADS / 64; ++w) p += s_pairs[w];
        if (p) atomicAdd(&words[0], p);
    }
}

__global__ __launch_bounds__(FS_THREADS) void k_fv_write(const u64* __restrict__ best, int n, int fill,
                                                         int32_t* __restrict__ label, int32_t* __restrict__ votes) {
    const int g = blockIdx.x * FS_THREADS + threadIdx.x;
    if (g >= n) return;
    const u64 b = best[g];  // 0: no vote (a count is at least 1)
    label[g] = b ? (int32_t)(0xffffffffu - (unsigned)b) : fill;
    votes[g] = (int32_t)(b >> 32);
}

}  // namespace

extern "C" int gf_frames_vote_max_probes(void) { return FS_MAX_PROBES; }

extern "C" int gf_frames_vote_default_slots(long long T, int n) {
    if (T < 0 || T > FS_MAX_POINTS || n < 0 || n > FS_MAX_POINTS) return 0;
    const i64 few = 8 * (i64)n;
    return (int)fs_pow2_slots(2 * (T < few ? T : few), FV_MIN_SLOTS, FV_MAX_SLOTS);  // (at most 2 T <= FV_MAX_SLOTS)
}

extern "C" size_t gf_frames_vote_scratch_bytes(int slots, int n) {
    if (!fv_slots_ok(slots) || n < 0 || n > FS_MAX_POINTS) return 0;
    return fv_scratch_bytes(slots, n);
}

extern "C" int gf_frames_vote(const int32_t* group, const void* value, int kind, int F, int W, int H, int stride, int n,
                              int ignore, int has_ignore, int fill, int slots, int aggregate, void* scratch,
                              int32_t* label, int32_t* votes, int32_t* total, int32_t* d_words, void* stream) {
    GF_CHECK_ARG(F >= 0 && W >= 0 && H >= 0, "gf_frames_vote: %d images of %d x %d (each >= 0)", F, W, H);
    GF_CHECK_ARG(stride >= 1, "gf_frames_vote: stride = %d (>= 1)", stride);
    GF_CHECK_ARG(kind >= 0 && kind <= 2, "gf_frames_vote: kind = %d (0 uint8, 1 uint16, 2 int32)", kind);
    GF_CHECK_ARG(n >= 0 && n <= FS_MAX_POINTS && gf_resample_max_points() == FS_MAX_POINTS,
                 "gf_frames_vote: n = %d groups (0 to %d)", n, FS_MAX_POINTS);
    const int Ws = gf_div_up(W, stride), Hs = gf_div_up(H, stride);
    const long long per = (long long)Hs * Ws;  // below 2^62
    GF_CHECK_ARG(per <= FS_MAX_POINTS && per * F <= FS_MAX_POINTS, "gf_frames_vote: %d x %d x %d sampled elements (at most %d)",
                 F, Hs, Ws, FS_MAX_POINTS);
    const long long T = per * F;
    GF_CHECK_ARG(fv_slots_ok(slots), "gf_frames_vote: slots = %d (a power of two from %d to %d)", slots, FV_MIN_SLOTS,
                 FV_MAX_SLOTS);
    if (T == 0 || n == 0) return GF_OK;
    GF_CHECK_ARG(group && value && scratch && label && votes && total && d_words,
                 "gf_frames_vote: NULL group, value, scratch, label, votes, total or d_words");
    hipStream_t st = (hipStream_t)stream;
    const FvTable tab = fv_carve(scratch, slots);
    const FvInput in = {group, value, kind, W, H, Ws, Hs, stride, (int)T, n, ignore, has_ignore != 0};
    const int bounded = (long long)slots < 2 * T;
    GF_TRY(hipMemsetAsync(tab.keys, 0xff, (size_t)slots * 8, st));
    GF_TRY(hipMemsetAsync(tab.cnt, 0, (size_t)slots * 4 + (size_t)n * 8, st));
    GF_TRY(hipMemsetAsync(total, 0, (size_t)n * 4, st));
    GF_TRY(hipMemsetAsync(d_words, 0, 3 * 4, st));
    if (aggregate)
        hipLaunchKernelGGL(k_fv_insert<true>, dim3(gf_div_up(T, FS_THREADS)), dim3(FS_THREADS), 0, st, in, tab,
                           (unsigned)slots - 1, bounded, d_words);
    else
        hipLaunchKernelGGL(k_fv_insert<false>, dim3(gf_div_up(T, FS_THREADS)), dim3(FS_THREADS), 0, st, in, tab,
                           (unsigned)slots - 1, bounded, d_words);
    hipLaunchKernelGGL(k_fv_pick, dim3(fs_blocks(slots, FV_PICK_BLOCKS)), dim3(FS_THREADS), 0, st, tab, (unsigned)slots, total,
                       d_words);
    hipLaunchKernelGGL(k_fv_write, dim3(gf_div_up(n, FS_THREADS)), dim3(FS_THREADS), 0, st, tab.best, n, fill, label, votes);
    GF_CHECK_LAUNCH("gf_frames_vote");
    return GF_OK;
}
