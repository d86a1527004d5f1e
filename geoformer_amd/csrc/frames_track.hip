// Instance ids that persist over successive snapshots: one update of a tracker keyed by the persistent cell
// numbers of a Fuser.  The host statement is frames.TrackerHost; see include/geoformer_hip.h for the arguments and the
// state (all of it owned by the caller: track_of int32 [map_cap], -1 beyond M, and table int32 [FT_COLUMNS, table_cap]).
//
// gf_frames_track_update   two memsets of the scratch (zeros: words, a, b, retired, cnt; ones: best, row_of, keys), then
//   k_ft_count<AGG>        one thread per point: cells must ascend and the owner lie in [-1, p) (a word each is raised and
//                          the point dropped otherwise); the row r (kept owner) and the track t (alive track of the cell)
//                          are derived, t goes to scratch for the apply pass.  With AGG only the head lane of a run of
//                          equal (r, t) among adjacent lanes goes on, with the run's length.  a[r], b[t] by integer adds;
//                          the pair r << 32 | t is found or claimed in an open-addressing table (slot read first, 64-bit
//                          CAS on an empty slot only) and its count added.  A thread that runs out of probes (bounded
//                          regime) raises the overflow word.
//   k_ft_best              strides over the slots: every stored pair offers itself as the best of its row and of its track
//                          by a CAS loop on "the best slot so far" under a total order (IoU by int64 cross-product, then
//                          the smaller index), whose maximum is unique: the result does not depend on arrival order.
//   k_ft_match             ONE workgroup: per row the mutual test and the threshold, new ids by an ordered scan over the
//                          rows, then the table: matched, new, missed and retired tracks.
//   k_ft_apply<AGG>        one thread per point: track_of and ids written, size moved by integer adds (run lengths).
//   k_ft_finish            strides over the tracks: an alive track left without a cell retires; the words copied out.
// k_ft_best, k_ft_match, k_ft_apply and k_ft_finish read the four flag words first and return when one is raised (the
// same words for every thread: the branch is uniform): a failed update writes nothing but scratch.
//
// Termination.  k_ft_count (frames_steps.h, "a key found or claimed") is unbounded with slots >= 2 m: the table holds at
// most m pairs; with fewer (`bounded`) a thread gives up after FS_MAX_PROBES probes.
// k_ft_best: a word changes only to a slot that is larger under the total order, so every failed CAS means another
// thread's progress and the word changes at most `pairs` times.  No thread waits for another thread or workgroup; there
// is no spin.  Integer atomics only; the one floating-point operation is the threshold (one double multiplication, one
// compare).
#include "common.h"
#include "frames_steps.h"

namespace {

constexpr int FT_MATCH_THREADS = 1024;
constexpr int FT_MAX_ROWS = 4096;  // rows of one update: FT_MATCH_THREADS threads scan four rows each
constexpr i64 FT_MAX_TRACKS = 1ll << 30;
constexpr i64 FT_MIN_SLOTS = 64;
constexpr i64 FT_MAX_SLOTS = 1ll << 30;  // 2 m at m = 2^29
constexpr int FT_BLOCKS = 2048;  // the most workgroups that stride over the slots or the tracks
constexpr int FT_WORDS = 16;
enum { W_ORDER = 0, W_OWNER = 1, W_OVERFLOW = 2, W_NEW = 3, W_RETIRED = 4, W_PAIRS = 5, W_ROOM = 6, W_LAST = 7 };
enum { C_CLS = 0, C_SCORE = 1, C_BORN = 2, C_SEEN = 3, C_HITS = 4, C_MISSES = 5, C_SIZE = 6, C_ALIVE = 7, FT_COLUMNS = 8 };

bool ft_slots_ok(i64 slots) { return fs_slots_ok(slots, FT_MIN_SLOTS, FT_MAX_SLOTS); }

struct FtScratch {
    int32_t* words;    // [FT_WORDS]   zeroed
    int32_t* a;        // [p]          zeroed: the points of a row
    int32_t* b;        // [T]          zeroed: the points of a track
    int32_t* retired;  // [T]          zeroed: 1 for a track retired by this update
    int32_t* cnt;      // [slots]      zeroed
    int32_t* best_row;    // [p]       ones: the slot of the row's best pair
    int32_t* best_track;  // [T]       ones
    int32_t* row_of;      // [T]       ones: the row a track matched
    u64* keys;            // [slots]   ones
    int32_t* prev;        // [m]       the track of every point before the update (never initialised: written by count)
    size_t zero_bytes, ones_at, ones_bytes, bytes;
};
size_t ft_up(size_t v) { return (v + 15) & ~(size_t)15; }
FtScratch ft_carve(void* scratch, i64 m, i64 p, i64 T, i64 slots) {
    FtScratch s;
    char* base = (char*)scratch;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        char* q = base + at;
        at += ft_up(bytes);
        return q;
    };
    s.words = (int32_t*)take(FT_WORDS * 4);
    s.a = (int32_t*)take((size_t)p * 4);
    s.b = (int32_t*)take((size_t)T * 4);
    s.retired = (int32_t*)take((size_t)T * 4);
    s.cnt = (int32_t*)take((size_t)slots * 4);
    s.zero_bytes = s.ones_at = at;
    s.best_row = (int32_t*)take((size_t)p * 4);
    s.best_track = (int32_t*)take((size_t)T * 4);
    s.row_of = (int32_t*)take((size_t)T * 4);
    s.keys = (u64*)take((size_t)slots * 8);
    s.ones_bytes = at - s.ones_at;
    s.prev = (int32_t*)take((size_t)m * 4);
    s.bytes = at;
    return s;
}

struct FtIn {
    const int32_t* cells;       // [m]
    const int32_t* owner;       // [m]
    const unsigned char* keep;  // [p]
    const int32_t* cls;         // [p]
    const float* score;         // [p]
    int m, p;
};

struct FtState {
    int32_t* track_of;  // [>= M'], -1 from M on
    int32_t* table;     // [FT_COLUMNS, cap]
    i64 cap;
    int M, T, room;  // room: the entries of track_of
    __device__ __forceinline__ int32_t& col(int c, int t) const { return table[(i64)c * cap + t]; }
};

__device__ __forceinline__ bool ft_failed(const int32_t* words) {
    return (words[W_ORDER] | words[W_OWNER] | words[W_OVERFLOW] | words[W_ROOM]) != 0;
}

// m <= 2^29: a point's index fits an int.  Every index used as an address is checked here: c in [0, M) before track_of,
// the owner in [0, p) before keep, the track in [0, T) before the table.
template <bool AGG>
__global__ __launch_bounds__(FS_THREADS) void k_ft_count(FtIn in, FtState st, FtScratch sc, unsigned mask, int bounded) {
    const int i = blockIdx.x * FS_THREADS + threadIdx.x, lane = threadIdx.x & 63;
    int r = -1, t = -1;
    if (i < in.m) {
        const int c = in.cells[i], o = in.owner[i];
        const bool ascends = c >= 0 && (i == 0 || in.cells[i - 1] < c);
        const bool in_range = o >= -1 && o < in.p;
        if (!ascends) sc.words[W_ORDER] = 1;
        if (!in_range) sc.words[W_OWNER] = 1;
        if (c >= st.room) sc.words[W_ROOM] = 1;  // the map is too short: nothing is written, the caller grows it
        if (i == in.m - 1) sc.words[W_LAST] = c;
        if (ascends && in_range) {
            if (o >= 0 && in.keep[o]) r = o;
            if (c < st.M) {
                const int was = st.track_of[c];
                if (was >= 0 && was < st.T && st.col(C_ALIVE, was)) t = was;
            }
        }
        sc.prev[i] = t;
    }
    const u64 key = ((u64)(unsigned)r << 32) | (u64)(unsigned)t;  // (-1, -1) for a lane without a point: it adds nothing
    unsigned add = 1;
    bool go = true;
    if (AGG) go = fs_run(key, lane, &add);
    if (!go) return;
    if (r >= 0) atomicAdd(&sc.a[r], (int)add);
    if (t >= 0) atomicAdd(&sc.b[t], (int)add);
    if (r < 0 || t < 0) return;
    unsigned s = fs_hash(key, mask);
    for (int probes = 1;; ++probes) {  // (frames_steps.h, "a key found or claimed")
        u64 old = fs_peek(&sc.keys[s]);
        if (old == FS_EMPTY) {
            old = atomicCAS(&sc.keys[s], FS_EMPTY, key);
            if (old == FS_EMPTY) {
                atomicAdd(&sc.words[W_PAIRS], 1);
                old = key;
            }
        }
        if (old == key) {
            atomicAdd(&sc.cnt[s], (int)add);
            return;
        }
        if (bounded && probes >= FS_MAX_PROBES) {  // fewer than 2 m slots: give up, every later launch returns at once
            sc.words[W_OVERFLOW] = 1;
            return;
        }
        s = (s + 1) & mask;  // slots >= 2 m otherwise: a free slot is always found
    }
}

// whether the pair (n1, union u1, index i1) comes before (n2, u2, i2): the larger IoU, exactly; then the smaller index.
// n <= 2^29 and u <= 2^30: a product is below 2^59.
__device__ __forceinline__ bool ft_before(int n1, int u1, int i1, int n2, int u2, int i2) {
    const i64 l = (i64)n1 * (i64)u2, r = (i64)n2 * (i64)u1;
    return l > r || (l == r && i1 < i2);
}

// *word becomes `slot` unless it holds a slot that comes before it.  `by_row`: the word is a row's (candidates differ in
// the track; the index of the order is the track), else a track's.
__device__ __forceinline__ void ft_offer(int32_t* word, int slot, int n, int uni, int index, bool by_row, const FtScratch& sc) {
    int cur = fs_peek(word);
    while (true) {
        if (cur >= 0) {
            const u64 k2 = sc.keys[cur];
            const int r2 = (int)(k2 >> 32), t2 = (int)(unsigned)k2, n2 = sc.cnt[cur];
            const int u2 = sc.a[r2] + sc.b[t2] - n2;
            if (!ft_before(n, uni, index, n2, u2, by_row ? t2 : r2)) return;
        }
        const int old = atomicCAS(word, cur, slot);
        if (old == cur) return;
        cur = old;
    }
}

__global__ __launch_bounds__(FS_THREADS) void k_ft_best(FtIn in, FtState st, FtScratch sc, i64 slots, int same_class) {
    if (ft_failed(sc.words)) return;
    const i64 stride = (i64)gridDim.x * FS_THREADS;
    for (i64 s = (i64)blockIdx.x * FS_THREADS + threadIdx.x; s < slots; s += stride) {
        const u64 key = sc.keys[s];
        if (key == FS_EMPTY) continue;
        const int r = (int)(key >> 32), t = (int)(unsigned)key, n = sc.cnt[s];  // (r < p and t < T: k_ft_count's checks)
        if (n <= 0) continue;
        if (same_class && in.cls[r] != st.col(C_CLS, t)) continue;
        const int uni = sc.a[r] + sc.b[t] - n;
        ft_offer(&sc.best_row[r], (int)s, n, uni, t, true, sc);
        ft_offer(&sc.best_track[t], (int)s, n, uni, r, false, sc);
    }
}

// One workgroup.  Rows: thread x owns the rows [x per, (x + 1) per) with per = ceil(p / FT_MATCH_THREADS) <= 4, so the new
// ids ascend with the row.  What one thread writes to global memory and another reads after the barrier is visible: both
// are in this workgroup.
__global__ __launch_bounds__(FT_MATCH_THREADS) void k_ft_match(FtIn in, FtState st, FtScratch sc, double iou, int max_misses,
                                                              int min_points, int update, int32_t* __restrict__ track) {
    __shared__ int s_scan[FT_MATCH_THREADS];
    __shared__ int s_retired;
    if (ft_failed(sc.words)) return;
    const int x = threadIdx.x, per = (in.p + FT_MATCH_THREADS - 1) / FT_MATCH_THREADS;
    const int r0 = x * per, r1 = min(in.p, r0 + per);
    if (x == 0) s_retired = 0;
    int fresh = 0;
    for (int r = r0; r < r1; ++r) {
        int tid = -1;
        const int s = sc.best_row[r];
        if (s >= 0) {
            const int t = (int)(unsigned)sc.keys[s], n = sc.cnt[s];
            const int uni = sc.a[r] + sc.b[t] - n;
            if (sc.best_track[t] == s && (double)n >= iou * (double)uni) {
                tid = t;
                sc.row_of[t] = r;
            }
        }
        if (tid < 0 && in.keep[r] && sc.a[r] >= min_points) {
            tid = -2;  // a new track: its id after the scan
            ++fresh;
        }
        track[r] = tid;
    }
    s_scan[x] = fresh;
    __syncthreads();
    for (int d = 1; d < FT_MATCH_THREADS; d <<= 1) {  // inclusive scan
        const int v = x >= d ? s_scan[x - d] : 0;
        __syncthreads();
        s_scan[x] += v;
        __syncthreads();
    }
    int id = st.T + s_scan[x] - fresh;
    for (int r = r0; r < r1; ++r) {
        if (track[r] != -2) continue;
        track[r] = id;
        st.col(C_CLS, id) = in.cls[r];
        st.col(C_SCORE, id) = __float_as_int(in.score[r]);
        st.col(C_BORN, id) = update;
        st.col(C_SEEN, id) = update;
        st.col(C_HITS, id) = 1;
        st.col(C_MISSES, id) = 0;
        st.col(C_SIZE, id) = 0;  // (k_ft_apply adds the cells)
        st.col(C_ALIVE, id) = 1;
        ++id;
    }
    if (x == FT_MATCH_THREADS - 1) sc.words[W_NEW] = s_scan[x];
    int gone = 0;
    for (int t = x; t < st.T; t += FT_MATCH_THREADS) {
        if (!st.col(C_ALIVE, t)) continue;
        const int r = sc.row_of[t];
        if (r >= 0) {
            st.col(C_HITS, t) += 1;
            st.col(C_MISSES, t) = 0;
            st.col(C_SEEN, t) = update;
            if (in.score[r] >= __int_as_float(st.col(C_SCORE, t))) {
                st.col(C_SCORE, t) = __float_as_int(in.score[r]);
                st.col(C_CLS, t) = in.cls[r];
            }
        } else if (sc.b[t] > 0) {  // in view and missed
            const int misses = st.col(C_MISSES, t) + 1;
            st.col(C_MISSES, t) = misses;
            if (misses > max_misses) {
                st.col(C_ALIVE, t) = 0;
                st.col(C_SIZE, t) = 0;
                sc.retired[t] = 1;
                ++gone;
            }
        }
    }
    if (gone) atomicAdd(&s_retired, gone);
    __syncthreads();
    if (x == 0) sc.words[W_RETIRED] = s_retired;
}

template <bool AGG>
__global__ __launch_bounds__(FS_THREADS) void k_ft_apply(FtIn in, FtState st, FtScratch sc, const int32_t* __restrict__ track,
                                                         int32_t* __restrict__ ids) {
    if (ft_failed(sc.words)) return;
    const int i = blockIdx.x * FS_THREADS + threadIdx.x, lane = threadIdx.x & 63;
    int was = -1, now = -1;
    if (i < in.m) {
        const int o = in.owner[i];
        const int tid = o >= 0 && in.keep[o] ? track[o] : -1;
        was = sc.prev[i];
        // a matched track redraws its boundary and a retired one lets go; a track that was merely missed holds its cells
        const bool cleared = was >= 0 && (sc.row_of[was] >= 0 || sc.retired[was]);
        now = tid >= 0 ? tid : (cleared ? -1 : was);
        if (tid >= 0 || cleared) st.track_of[in.cells[i]] = now;  // (a cell from M on holds -1 already)
        ids[i] = now;
    }
    const u64 key = ((u64)(unsigned)was << 32) | (u64)(unsigned)now;
    unsigned add = 1;
    bool go = was != now;
    if (AGG) go = fs_run(key, lane, &add) && go;
    if (!go) return;
    if (was >= 0 && !sc.retired[was]) atomicSub(&st.col(C_SIZE, was), (int)add);  // (a retired track's size is 0 already)
    if (now >= 0) atomicAdd(&st.col(C_SIZE, now), (int)add);
}

__global__ __launch_bounds__(FS_THREADS) void k_ft_finish(FtState st, FtScratch sc, int32_t* __restrict__ retired,
                                                          int32_t* __restrict__ words) {
    const bool failed = ft_failed(sc.words);
    const int x = blockIdx.x * FS_THREADS + threadIdx.x, stride = gridDim.x * FS_THREADS;
    int gone = 0;
    if (!failed) {
        for (int t = x; t < st.T; t += stride) {
            int flag = sc.retired[t];
            if (!flag && st.col(C_ALIVE, t) && st.col(C_SIZE, t) == 0) {  // every cell taken over: nothing left to follow
                st.col(C_ALIVE, t) = 0;
                flag = 1;
                ++gone;
            }
            retired[t] = flag;
        }
        if (gone) atomicAdd(&words[W_RETIRED], gone);  // (zeroed by the caller's memset; k_ft_match's count is added below)
    }
    if (x < FT_WORDS && x != W_RETIRED) words[x] = sc.words[x];
    if (x == W_RETIRED && !failed && sc.words[W_RETIRED]) atomicAdd(&words[W_RETIRED], sc.words[W_RETIRED]);
}

}  // namespace

extern "C" int gf_frames_track_max_rows(void) { return FT_MAX_ROWS; }
extern "C" int gf_frames_track_max_probes(void) { return FS_MAX_PROBES; }
extern "C" long long gf_frames_track_max_tracks(void) { return FT_MAX_TRACKS; }
extern "C" int gf_frames_track_columns(void) { return FT_COLUMNS; }
extern "C" int gf_frames_track_words(void) { return FT_WORDS; }

extern "C" long long gf_frames_track_default_slots(long long p, long long live) {
    if (p < 0 || p > FT_MAX_ROWS || live < 0 || live > FT_MAX_TRACKS) return 0;
    return fs_pow2_slots(8 * (p + live), FT_MIN_SLOTS, FT_MAX_SLOTS);
}

extern "C" size_t gf_frames_track_scratch_bytes(long long m, long long p, long long T, long long slots) {
    if (m < 0 || m > FS_MAX_POINTS || p < 0 || p > FT_MAX_ROWS || T < 0 || T > FT_MAX_TRACKS || !ft_slots_ok(slots)) return 0;
    return ft_carve(nullptr, m, p, T, slots).bytes + 16;
}

extern "C" int gf_frames_track_update(const int32_t* cells, const int32_t* owner, long long m, const int32_t* cls,
                                      const float* score, const unsigned char* keep, int p, int32_t* track_of, long long M,
                                      long long map_cap, int32_t* table, long long T, long long table_cap, double iou,
                                      int max_misses, int min_points, int same_class, int update, long long slots,
                                      int aggregate, void* scratch, int32_t* ids, int32_t* track, int32_t* retired,
                                      int32_t* d_words, void* stream) {
    const char* who = "gf_frames_track_update";
    GF_CHECK_ARG(m >= 0 && m <= FS_MAX_POINTS && gf_resample_max_points() == FS_MAX_POINTS, "%s: m = %lld points (0 to %d)", who,
                 m, FS_MAX_POINTS);
    GF_CHECK_ARG(p >= 0 && p <= FT_MAX_ROWS, "%s: p = %d rows (0 to %d)", who, p, FT_MAX_ROWS);
    GF_CHECK_ARG(M >= 0 && M <= map_cap && map_cap <= 2147483647ll, "%s: M = %lld cells in a map of %lld (0 <= M <= capacity < 2^31)",
                 who, M, map_cap);
    GF_CHECK_ARG(T >= 0 && T + p <= table_cap && table_cap <= FT_MAX_TRACKS,
                 "%s: T = %lld tracks and %d rows in a table of %lld (T + p <= capacity <= %lld)", who, T, p, table_cap, FT_MAX_TRACKS);
    GF_CHECK_ARG(iou >= 0.0 && iou <= 1.0, "%s: iou = %g (0 to 1)", who, iou);
    GF_CHECK_ARG(max_misses >= 0 && min_points >= 1 && update >= 0, "%s: max_misses = %d (>= 0), min_points = %d (>= 1), update = %d (>= 0)",
                 who, max_misses, min_points, update);
    GF_CHECK_ARG(ft_slots_ok(slots), "%s: slots = %lld (a power of two from %lld to %lld)", who, slots, FT_MIN_SLOTS, FT_MAX_SLOTS);
    GF_CHECK_ARG(scratch && d_words && (T == 0 || retired), "%s: NULL scratch, d_words or retired", who);
    GF_CHECK_ARG(m == 0 || (cells && owner && track_of && ids), "%s: NULL cells, owner, track_of or ids", who);
    GF_CHECK_ARG(p == 0 || (cls && score && keep && track), "%s: NULL cls, score, keep or track", who);
    GF_CHECK_ARG(table_cap == 0 || table, "%s: NULL table", who);
    hipStream_t s = (hipStream_t)stream;
    const FtScratch sc = ft_carve(scratch, m, p, T, slots);
    const FtIn in = {cells, owner, keep, cls, score, (int)m, p};
    const FtState st = {track_of, table, (i64)table_cap, (int)M, (int)T, (int)map_cap};
    GF_TRY(hipMemsetAsync(scratch, 0, sc.zero_bytes, s));
    GF_TRY(hipMemsetAsync((char*)scratch + sc.ones_at, 0xff, sc.ones_bytes, s));
    GF_TRY(hipMemsetAsync(d_words, 0, FT_WORDS * 4, s));
    const int g = gf_div_up(m, FS_THREADS), bounded = slots < 2 * m;
    if (m > 0) {
        if (aggregate)
            hipLaunchKernelGGL(k_ft_count<true>, dim3(g), dim3(FS_THREADS), 0, s, in, st, sc, (unsigned)(slots - 1), bounded);
        else
            hipLaunchKernelGGL(k_ft_count<false>, dim3(g), dim3(FS_THREADS), 0, s, in, st, sc, (unsigned)(slots - 1), bounded);
        if (T > 0 && p > 0)
            hipLaunchKernelGGL(k_ft_best, dim3(fs_blocks(slots, FT_BLOCKS)), dim3(FS_THREADS), 0, s, in, st, sc, (i64)slots,
                               same_class != 0);
    }
    hipLaunchKernelGGL(k_ft_match, dim3(1), dim3(FT_MATCH_THREADS), 0, s, in, st, sc, iou, max_misses, min_points, update, track);
    if (m > 0) {
        if (aggregate)
            hipLaunchKernelGGL(k_ft_apply<true>, dim3(g), dim3(FS_THREADS), 0, s, in, st, sc, (const int32_t*)track, ids);
        else
            hipLaunchKernelGGL(k_ft_apply<false>, dim3(g), dim3(FS_THREADS), 0, s, in, st, sc, (const int32_t*)track, ids);
    }
    hipLaunchKernelGGL(k_ft_finish, dim3(fs_blocks(T > FT_WORDS ? T : FT_WORDS, FT_BLOCKS)), dim3(FS_THREADS), 0, s, st, sc, retired,
                       d_words);
    GF_CHECK_LAUNCH(who);
    return GF_OK;
}
