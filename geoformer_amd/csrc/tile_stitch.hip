// Per-point semantic scores of a scan that was run as T overlapping tiles, stitched from the tiles' scores (the host
// statement is postprocess.stitch_tiles_host; the tile plan is scene.tile_plan; see include/geoformer_hip.h for the
// arguments).
//
// As in tile_merge.hip the device sees integer tables only: tile_of / local_of int32 [N, 4], core_of int32 [N], and the
// tiles as a table of one GfTileScore each.
//   k_ts_stitch  one workgroup of 256 threads per 256 consecutive points of the scan, in two steps:
//                1. one thread per point: one 16-byte read each of its tile_of and local_of rows (and core_of in core
//                   mode); every slot that counts is resolved to the address of its source row -- the tile id checked
//                   against [0, T), the local index against [0, n_s) -- and the addresses are packed to the front, in
//                   slot order, in LDS (4 x 8 bytes per point) beside their number
//                2. one thread per output float of the workgroup's 256 * C consecutive floats, k = thread + 256 * i
//                   (a wave's store is 64 consecutive floats; (point, class) of k advance by 256 / C and 256 % C, so
//                   a thread divides once): the point's addresses from LDS, one float from each row, summed in slot
//                   order, divided (mean mode), stored
// The plan's tables are read once per point, not once per float; a source row is read as C consecutive floats by the C
// lanes of its point, and within a tile the local indices ascend with the scan's point order, so neighbouring points
// mostly read neighbouring rows.  No atomics and no memset: every cell of out is written by exactly one thread, and the
// outputs are bit-identical from call to call.  Every point * C + class is formed in 64 bits.
#include "common.h"

namespace {

static_assert(sizeof(GfTileScore) == 8 * GF_TILE_SCORE_FIELDS, "the row of include/geoformer_hip.h");
constexpr int TS_THREADS = 256;             // = the points of a workgroup
constexpr int TS_SLOTS = 4;

typedef unsigned long long u64;

// the address of point (s, l)'s row of C floats, or NULL when (s, l) names no row
__device__ __forceinline__ const float* ts_row(const long long* __restrict__ tab, int T, int C, int s, int l) {
    if ((unsigned)s >= (unsigned)T) return nullptr;
    const GfTileScore* row = gf_row<GfTileScore>(tab, s);
    if ((u64)(long long)l >= (u64)row->n_s) return nullptr;  // (a negative index is a huge one)
    return (const float*)row->scores + (long long)l * C;
}

__global__ __launch_bounds__(TS_THREADS) void k_ts_stitch(const long long* __restrict__ tab, int T,
                                                          const int4* __restrict__ tile_of,
                                                          const int4* __restrict__ local_of,
                                                          const int32_t* __restrict__ core_of, long long N, int C,
                                                          int mode, int step_p, int step_c, float* __restrict__ out) {
    __shared__ const float* s_src[TS_SLOTS][TS_THREADS];
    __shared__ int s_cnt[TS_THREADS];
    const int tid = threadIdx.x;
    const long long g0 = (long long)blockIdx.x * TS_THREADS;
    const int np = (int)min((long long)TS_THREADS, N - g0);  // the points of this workgroup (>= 1)
    if (tid < np) {
        const int4 tl = tile_of[g0 + tid], lc = local_of[g0 + tid];
        const int t4[TS_SLOTS] = {tl.x, tl.y, tl.z, tl.w}, l4[TS_SLOTS] = {lc.x, lc.y, lc.z, lc.w};
        int cnt = 0;
        if (mode == GF_TILE_STITCH_CORE) {
            const int core = core_of[g0 + tid];
#pragma unroll
            for (int j = 0; j < TS_SLOTS; ++j) {
                if (cnt == 0 && t4[j] == core) {  // the first slot of the core tile, valid or not
                    const float* p = ts_row(tab, T, C, t4[j], l4[j]);
                    s_src[0][tid] = p;
                    cnt = p ? 1 : -1;
                }
            }
            cnt = max(cnt, 0);
        } else {
#pragma unroll
            for (int j = 0; j < TS_SLOTS; ++j) {
                const float* p = ts_row(tab, T, C, t4[j], l4[j]);
                if (p) {
#pragma unroll
                    for (int q = 0; q < TS_SLOTS; ++q)  // (static LDS indices: cnt == q)
                        if (cnt == q) s_src[q][tid] = p;
                    ++cnt;
                }
            }
        }
        s_cnt[tid] = cnt;
    }
    __syncthreads();
    const int total = np * C;  // <= 256 * 64
    int p = tid / C, c = tid - p * C;
    float* dst = out + g0 * C;
    for (int k = tid; k < total; k += TS_THREADS) {
        const int cnt = s_cnt[p];
        float acc = 0.0f;
        if (cnt > 0) acc = s_src[0][p][c];
        if (cnt > 1) acc = acc + s_src[1][p][c];
        if (cnt > 2) acc = acc + s_src[2][p][c];
        if (cnt > 3) acc = acc + s_src[3][p][c];
        if (mode == GF_TILE_STITCH_MEAN && cnt > 0) acc = __fdiv_rn(acc, (float)cnt);
        dst[k] = acc;
        p += step_p;
        c += step_c;
        if (c >= C) {
            c -= C;
            ++p;
        }
    }
}

}  // namespace

extern "C" int gf_tile_stitch_max_classes(void) { return gf_semantic_confusion_max_classes(); }

extern "C" int gf_tile_stitch_scores(const long long* table, const long long* table_host, int T, const int32_t* tile_of,
                                     const int32_t* local_of, const int32_t* core_of, long long N, int C, int mode,
                                     float* out, void* stream) {
    const int cap = gf_tile_stitch_max_classes();
    GF_CHECK_ARG(T >= 1 && T <= 65535, "gf_tile_stitch_scores: T = %d tiles (1 to 65535)", T);
    GF_CHECK_ARG(C >= 1 && C <= cap, "gf_tile_stitch_scores: C = %d classes (1 to %d)", C, cap);
    GF_CHECK_ARG(mode == GF_TILE_STITCH_CORE || mode == GF_TILE_STITCH_MEAN,
                 "gf_tile_stitch_scores: mode = %d (GF_TILE_STITCH_CORE or GF_TILE_STITCH_MEAN)", mode);
    GF_CHECK_ARG(N >= 0 && N <= 0x7fffffffLL * TS_THREADS, "gf_tile_stitch_scores: N = %lld points", N);
    GF_CHECK_ARG(table && table_host, "gf_tile_stitch_scores: NULL table or table_host");
    for (int s = 0; s < T; ++s) {
        const GfTileScore* r = gf_row<GfTileScore>(table_host, s);
        GF_CHECK_ARG(r->n_s >= 0 && r->n_s <= 0x7fffffffLL, "gf_tile_stitch_scores: tile %d: n_s = %lld", s, r->n_s);
        GF_CHECK_ARG(r->n_s == 0 || r->scores != 0, "gf_tile_stitch_scores: tile %d: NULL scores with n_s = %lld", s, r->n_s);
    }
    if (N == 0) return GF_OK;
    GF_CHECK_ARG(tile_of && local_of && out && (mode != GF_TILE_STITCH_CORE || core_of),
                 "gf_tile_stitch_scores: NULL tile_of, local_of, core_of or out");
    GF_CHECK_ARG((((uintptr_t)tile_of | (uintptr_t)local_of) & 15) == 0,
                 "gf_tile_stitch_scores: tile_of and local_of must be 16-byte aligned");
    hipLaunchKernelGGL(k_ts_stitch, dim3(gf_div_up(N, TS_THREADS)), dim3(TS_THREADS), 0, (hipStream_t)stream, table, T,
                       (const int4*)tile_of, (const int4*)local_of, core_of, N, C, mode, TS_THREADS / C, TS_THREADS % C,
                       out);
    GF_CHECK_LAUNCH("gf_tile_stitch_scores");
    return GF_OK;
}
