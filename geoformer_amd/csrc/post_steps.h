// Steps that the post-processing and evaluation kernels repeat (oversegment, mask_split, tile_merge, inst_eval, panoptic,
// resample, render), each defined once.  All of them are forced inline and were checked to leave the kernels' machine
// code as it was (tools/isa_diff.sh); where a kernel's code would change, that kernel keeps the step written out and
// says so (DESIGN.md §4 lists them).
#pragma once
#include "common.h"

// ---- lock-free min-index union-find over parent[] (parent[i] = i at the start) -------------------------------------
// SCOPE is the memory scope of the atomics: __HIP_MEMORY_SCOPE_AGENT for an array in global memory that the whole grid
// hooks, __HIP_MEMORY_SCOPE_WORKGROUP for an LDS array of one workgroup.  The argument is the same for both:
//   * parent[x] <= x always, and parent[x] names a member of x's set: a union puts the LARGER root under the smaller, a
//     find rewrites a word to its grandparent.  So no cycle can form, every walk descends and ends, and the root of a
//     finished set is its smallest index -- a function of the edges alone, whatever the order in which the unions land.
//   * every load of a find is an atomic one.  Only a NON-root's word is rewritten (to its grandparent: still below it,
//     still in its set), and a non-root never becomes a root again, so the atomicCAS on roots in gf_uf_union is not
//     disturbed by the finds that run beside it.
//   * a failed CAS means another thread hooked `hi` first; the loop goes on from hi and lo and finds the new roots.
//   * once nothing is hooked any more (after a kernel boundary or a barrier), gf_uf_root may run beside other
//     gf_uf_root calls: a word only ever moves to an ancestor and a root's word never changes, so every walk still ends
//     at the root.

// root of x while other threads hook roots, halving the path on the way
template <int SCOPE>
__device__ __forceinline__ int gf_find_live(int* parent, int x) {
    for (;;) {
        const int p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, SCOPE);
        if (p == x) return x;
        const int gp = __hip_atomic_load(&parent[p], __ATOMIC_RELAXED, SCOPE);
        if (gp != p) __hip_atomic_store(&parent[x], gp, __ATOMIC_RELAXED, SCOPE);
        x = gp;
    }
}

// joins the sets of a and b
template <int SCOPE>
__device__ __forceinline__ void gf_uf_union(int* parent, int a, int b) {
    for (;;) {
        a = gf_find_live<SCOPE>(parent, a);
        b = gf_find_live<SCOPE>(parent, b);
        if (a == b) break;
        const int hi = max(a, b), lo = min(a, b);
        if (atomicCAS(&parent[hi], hi, lo) == hi) break;
        a = hi;  // hi was hooked by another thread meanwhile: go on from there
        b = lo;
    }
}

// root of i once nothing is hooked any more, stored back into parent[i]
template <int SCOPE>
__device__ __forceinline__ int gf_uf_root(int* parent, int i) {
    int root = i;
    for (;;) {
        const int p = __hip_atomic_load(&parent[root], __ATOMIC_RELAXED, SCOPE);
        if (p == root) break;
        root = p;
    }
    if (root != i) __hip_atomic_store(&parent[i], root, __ATOMIC_RELAXED, SCOPE);
    return root;
}

// ---- count[key] += the number of lanes of the wave that are `on` with that key: ONE atomicAdd per distinct key of the
// wave (a 3000-point cluster would otherwise send every one of its adds to one address).  lane = threadIdx.x & 63;
// wave-uniform control flow: every lane of the wave calls it.
__device__ __forceinline__ void gf_wave_add_per_key(int lane, bool on, int key, int32_t* count) {
    unsigned long long todo = __ballot(on);
    while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const int k0 = __shfl(key, lead, 64);
        const unsigned long long same = __ballot(on && key == k0);
        if (lane == lead) atomicAdd(&count[k0], __popcll(same));
        todo &= ~same;
    }
}

// ---- inclusive Hillis-Steele scan of one int per thread over a workgroup of THREADS threads through the LDS array a
// (THREADS words): leaves the sum of v over the threads 0 .. t in a[t]; a[THREADS - 1] is the total
template <int THREADS>
__device__ __forceinline__ void gf_lds_incl_scan(int32_t* a, int t, int v) {
    a[t] = v;
    __syncthreads();
    for (int off = 1; off < THREADS; off <<= 1) {
        const int o = t >= off ? a[t - off] : 0;
        __syncthreads();
        a[t] += o;
        __syncthreads();
    }
}

// ---- presence table to ascending slots, one workgroup of THREADS threads per table.  table: presence (0/1) of the K
// keys (class rank * 1000 + id mod 1000) in, the key's slot among the present keys (or -1) out, in place: every thread
// owns one contiguous run of keys (t = threadIdx.x).  gt_id[slot] = the id of the slot's key (slots below max_gt only).
// Returns the number of present keys up to the end of the thread's run: thread THREADS - 1 holds G and stores it.
// sums: LDS, THREADS words.  sorted_cls (LDS, the class ids ascending) is filled by the caller right before the call;
// the scan's first barrier stands between.
template <int THREADS>
__device__ __forceinline__ int gf_presence_to_slots(int32_t* table, int K, const int32_t* sorted_cls, int32_t* sums,
                                                    int t, int max_gt, long long* gt_id) {
    const int per = (K + THREADS - 1) / THREADS;
    const int b = min(K, t * per), e = min(K, b + per);
    int s = 0;
    for (int k = b; k < e; ++k) s += table[k] != 0;
    gf_lds_incl_scan<THREADS>(sums, t, s);
    const int incl = sums[t];
    int slot = incl - s;
    for (int k = b; k < e; ++k) {
        if (table[k] != 0) {
            if (slot < max_gt) gt_id[slot] = (long long)sorted_cls[k / 1000] * 1000 + k % 1000;
            table[k] = slot++;
        } else {
            table[k] = -1;
        }
    }
    return incl;
}

// the class of a ground-truth id class * 1000 + instance: floor division, as numpy's //
__device__ __forceinline__ long long gf_floor_div_1000(long long g) {
    long long q = g / 1000;
    if (g % 1000 != 0 && g < 0) --q;
    return q;
}

// ---- the scene of point p in packed offsets [S + 1]: the last s with offsets[s] <= p (empty scenes before it share the
// value), inside [0, S - 1]
__device__ __forceinline__ int gf_scene_of(const int32_t* offsets, int S, long long p) {
    int lo = 0, hi = S;  // first index in [0, S] whose offset exceeds p
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] > p)
            hi = mid;
        else
            lo = mid + 1;
    }
    return max(lo - 1, 0);
}

// ---- a float as an unsigned word whose integer order is the float order (-inf lowest, +inf highest among the
// non-NaN), and back
__device__ __forceinline__ uint32_t gf_float_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float gf_float_unkey(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
