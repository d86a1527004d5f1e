// Scene labelling from the picked masks: one label per point and one table row per picked instance
// (util/visualize.py:219-227 paints the picked instances from the last to the first, skipping score < min_score, a later
// paint wins: the owner of a point is the LOWEST rank r in pick with score >= min_score whose mask covers the point).
// Every kernel reads a device scene table (one GfLblScene of include/geoformer_hip.h per scene); S scenes take
// three launches whatever S, n and p are:
//   k_lm_pack    grid (chunks, ranks, S): one workgroup per (rank r, chunk of LM_CHUNK points) reads its piece of mask
//                row pick[r] ONCE (the only pass over the int32 masks), writes the ballot-packed bits [p, ceil(N / 64)]
//                and the chunk's partial of the row's geometry (count, xyz sum, box);
//   k_lm_owner   grid (N / 1024, S): one wave per 64-point word finds the first rank whose packed word has the point's
//                bit (rows that are not kept are packed as zeros; the packed rows are 1/32 of the int32 rows and stay in
//                L2) -> owner, ids, and the workgroup's per-rank histogram;
//   k_lm_table   grid (ranks / 4, S): one wave per rank folds the chunk partials in chunk order into the table row.
// Nothing is accumulated with atomics in global memory: a partial belongs to one (rank, chunk) whose extent depends on
// N alone, and both reductions run in a fixed order, so a scene's table is bit-identical alone or in any batch.
#include "common.h"

#define LM_CHUNK GF_LBL_CHUNK          // points per workgroup: 4 waves x LM_WORDS words x 64 lanes
#define LM_WORDS (LM_CHUNK / 256)      // 64-point words per wave
#define LM_OWN_SPLIT GF_LBL_OWN_SPLIT  // k_lm_owner's workgroups per chunk: own_part holds that many records per partial
#define LM_OWN_THREADS (LM_CHUNK / LM_OWN_SPLIT)  // 1024: 16 waves, one 64-point word each
// k_lm_table writes the float row as fp32 words at the struct's offsets: through GfLblRowF the stores are scheduled
// differently
#define LM_ATF(member) ((int)(offsetof(GfLblRowF, member) / sizeof(float)))
#define LM_PARTF 9                     // fp32 per partial: xyz sum, box min, box max
static_assert(sizeof(GfLblScene) == 8 * GF_LBL_SCENE_FIELDS && sizeof(GfLblRowI) == 4 * GF_LBL_TABLE_INTS &&
                  sizeof(GfLblRowF) == 4 * GF_LBL_TABLE_FLOATS, "the rows of include/geoformer_hip.h");

__device__ __forceinline__ float lm_wave_min(float m) {
    m = fminf(m, gf_shfl_xor<32>(m));
    m = fminf(m, gf_shfl_xor<16>(m));
    m = fminf(m, gf_shfl_xor<8>(m));
    m = fminf(m, gf_shfl_xor<4>(m));
    m = fminf(m, gf_shfl_xor<2>(m));
    m = fminf(m, gf_shfl_xor<1>(m));
    return m;
}

__global__ __launch_bounds__(256) void k_lm_pack(const long long* __restrict__ table, float min_score,
                                                 unsigned long long* __restrict__ bits, float* __restrict__ part_f,
                                                 int32_t* __restrict__ part_cnt) {
    const GfLblScene* t = gf_row<GfLblScene>(table, blockIdx.z);
    const long long N = t->N, n = t->n, p = t->p;
    const long long nch = (N + LM_CHUNK - 1) / LM_CHUNK, W2 = (N + 63) / 64;
    const long long r = blockIdx.y, c = blockIdx.x;
    if (r >= p || c >= nch) return;
    const long long row = ((const long long*)t->pick)[r];
    const bool valid = row >= 0 && row < n;  // (a pick outside the masks is an empty row, never an address)
    const bool kept = valid && ((const float*)t->scores)[row] >= min_score;  // the bits serve the owner: kept rows only
    const int32_t* m = (const int32_t*)t->masks + (valid ? row : 0) * N;
    const float* xyz = (const float*)t->xyz;
    unsigned long long* out = bits + t->bits_off + r * W2;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long w0 = c * (LM_CHUNK / 64) + (long long)wave * LM_WORDS;
    // the loads of the wave's 16 words first, all in flight together: unconditional, a point past the end reads the
    // row's last one (a load under a per-lane condition is waited for before the next is issued)
    int v[LM_WORDS];
#pragma unroll
    for (int k = 0; k < LM_WORDS; k++) v[k] = 0;
    if (valid) {  // (uniform over the workgroup)
#pragma unroll
        for (int k = 0; k < LM_WORDS; k++) {
            const long long pt = (w0 + k) * 64 + lane;
            v[k] = m[pt < N ? pt : N - 1];
        }
    }
    // bits, then the xyz of the lanes that are on: every gather is issued before the first is used (inside the loop
    // over the words each would be an L2 round trip of its own, sixteen in a row where a mask is dense); a lane that
    // is off reads point 0, one cache line for all of them
    bool on[LM_WORDS];
    float x[LM_WORDS], y[LM_WORDS], z[LM_WORDS];
#pragma unroll
    for (int k = 0; k < LM_WORDS; k++) {
        on[k] = v[k] != 0 && (w0 + k) * 64 + lane < N;
        const unsigned long long bb = __ballot(on[k]);
        if (lane == 0 && w0 + k < W2) out[w0 + k] = kept ? bb : 0ull;
        const float* q = xyz + (on[k] ? (w0 + k) * 64 + lane : 0) * 3;
        x[k] = q[0], y[k] = q[1], z[k] = q[2];
    }
    int cnt = 0;
    float sx = 0.f, sy = 0.f, sz = 0.f;
    float lx = INFINITY, ly = INFINITY, lz = INFINITY, hx = -INFINITY, hy = -INFINITY, hz = -INFINITY;
#pragma unroll
    for (int k = 0; k < LM_WORDS; k++) {
        if (on[k]) {
            cnt++;
            sx += x[k], sy += y[k], sz += z[k];
            lx = fminf(lx, x[k]), ly = fminf(ly, y[k]), lz = fminf(lz, z[k]);
            hx = fmaxf(hx, x[k]), hy = fmaxf(hy, y[k]), hz = fmaxf(hz, z[k]);
        }
    }
    __shared__ float s_f[4][LM_PARTF];
    __shared__ int s_c[4];
    cnt = gf_wave_sum_i(cnt);
    sx = gf_wave_sum(sx), sy = gf_wave_sum(sy), sz = gf_wave_sum(sz);
    lx = lm_wave_min(lx), ly = lm_wave_min(ly), lz = lm_wave_min(lz);
    hx = gf_wave_max(hx), hy = gf_wave_max(hy), hz = gf_wave_max(hz);
    if (lane == 0) {
        s_c[wave] = cnt;
        float* f = s_f[wave];
        f[0] = sx, f[1] = sy, f[2] = sz, f[3] = lx, f[4] = ly, f[5] = lz, f[6] = hx, f[7] = hy, f[8] = hz;
    }
    __syncthreads();
    const long long o = t->part_off + r * nch + c;
    if (threadIdx.x < LM_PARTF) {
        const int j = threadIdx.x;
        float a = s_f[0][j];
#pragma unroll
        for (int w = 1; w < 4; w++) a = j < 3 ? a + s_f[w][j] : (j < 6 ? fminf(a, s_f[w][j]) : fmaxf(a, s_f[w][j]));
        part_f[o * LM_PARTF + j] = a;
    } else if (threadIdx.x == 64) {
        part_cnt[o] = (s_c[0] + s_c[1]) + (s_c[2] + s_c[3]);
    }
}

__global__ __launch_bounds__(LM_OWN_THREADS) void k_lm_owner(const long long* __restrict__ table,
                                                             const unsigned long long* __restrict__ bits,
                                                             float min_score, int32_t* __restrict__ owner,
                                                             int32_t* __restrict__ ids, int32_t* __restrict__ own_part) {
    __shared__ int s_lab[GF_NMS_MAX_N];  // label id of rank r, -1 where the rank is not kept
    __shared__ int s_hist[GF_NMS_MAX_N];
    const GfLblScene* t = gf_row<GfLblScene>(table, blockIdx.y);
    const long long N = t->N, n = t->n;
    const int p = (int)t->p;
    const long long nob = (N + LM_OWN_THREADS - 1) / LM_OWN_THREADS, W2 = (N + 63) / 64;
    const long long c = blockIdx.x;
    if (c >= nob) return;
    const long long* pick = (const long long*)t->pick;
    const float* scores = (const float*)t->scores;
    const long long* labels = (const long long*)t->label_ids;
    for (int r = threadIdx.x; r < p; r += LM_OWN_THREADS) {
        const long long row = pick[r];
        const bool kept = row >= 0 && row < n && scores[row] >= min_score;
        s_lab[r] = kept ? (int)labels[row] : -1;
        s_hist[r] = 0;
    }
    __syncthreads();
    // one wave per 64-point word.  The word of rank r is the same address for the whole wave (scalar loads); eight ranks'
    // words are fetched together, since the walk over the ranks is a chain of L2 latencies otherwise.  Rows that are not
    // kept were packed as zeros (k_lm_pack).
    const int lane = threadIdx.x & 63;
    const long long w = c * (LM_OWN_THREADS / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (w < W2) {  // (wave-uniform)
        const unsigned long long* sb = bits + t->bits_off + w;
        int own = -1;
        unsigned long long open = ~0ull;  // lanes without an owner yet
        for (int r0 = 0; r0 < p && open; r0 += 8) {
            unsigned long long word[8];
#pragma unroll
            for (int j = 0; j < 8; j++) word[j] = sb[(long long)(r0 + j < p ? r0 + j : p - 1) * W2];
#pragma unroll
            for (int j = 0; j < 8; j++) {
                if (r0 + j >= p) break;
                if (((word[j] & open) >> lane) & 1ull) own = r0 + j;
                open &= ~word[j];
            }
        }
        const long long pt = w * 64 + lane;
        if (pt < N) {
            owner[t->pt_off + pt] = own;
            ids[t->pt_off + pt] = own < 0 ? 0 : s_lab[own] * 1000 + own + 1;
            if (own >= 0) atomicAdd(&s_hist[own], 1);  // (LDS, integers: exact in any order)
        }
    }
    __syncthreads();
    int32_t* hp = own_part + t->part_off * LM_OWN_SPLIT + c * p;
    for (int r = threadIdx.x; r < p; r += LM_OWN_THREADS) hp[r] = s_hist[r];
}

__global__ __launch_bounds__(256) void k_lm_table(const long long* __restrict__ table,
                                                  const float* __restrict__ part_f,
                                                  const int32_t* __restrict__ part_cnt,
                                                  const int32_t* __restrict__ own_part, float min_score,
                                                  int32_t* __restrict__ tab_i, float* __restrict__ tab_f) {
    const GfLblScene* t = gf_row<GfLblScene>(table, blockIdx.y);
    const long long N = t->N, n = t->n, p = t->p;
    const long long nch = (N + LM_CHUNK - 1) / LM_CHUNK;
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (r >= p) return;
    // lane l folds chunks l, l + 64, ... in ascending order, then the wave's fixed tree
    int cnt = 0, owned = 0;
    float s[3] = {0.f, 0.f, 0.f}, lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (long long c = lane; c < nch; c += 64) {
        const long long o = t->part_off + r * nch + c;
        const float* f = part_f + o * LM_PARTF;
        cnt += part_cnt[o];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            s[j] += f[j];
            lo[j] = fminf(lo[j], f[3 + j]);
            hi[j] = fmaxf(hi[j], f[6 + j]);
        }
    }
    const long long nob = (N + LM_OWN_THREADS - 1) / LM_OWN_THREADS;
    for (long long c = lane; c < nob; c += 64) owned += own_part[t->part_off * LM_OWN_SPLIT + c * p + r];
    cnt = gf_wave_sum_i(cnt), owned = gf_wave_sum_i(owned);
#pragma unroll
    for (int j = 0; j < 3; j++) s[j] = gf_wave_sum(s[j]), lo[j] = lm_wave_min(lo[j]), hi[j] = gf_wave_max(hi[j]);
    if (lane != 0) return;
    const long long row = ((const long long*)t->pick)[r];
    const bool valid = row >= 0 && row < n;
    const float score = valid ? ((const float*)t->scores)[row] : 0.f;
    GfLblRowI* ti = (GfLblRowI*)tab_i + (t->row_off + r);
    float* tf = tab_f + (t->row_off + r) * GF_LBL_TABLE_FLOATS;
    ti->count = cnt;
    ti->owned = owned;
    ti->label_id = valid ? (int)((const long long*)t->label_ids)[row] : 0;
    ti->pick = (int)row;
    ti->kept = valid && score >= min_score;
    const float inv = (float)cnt;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        tf[LM_ATF(centroid) + j] = cnt ? s[j] / inv : 0.f;
        tf[LM_ATF(box_min) + j] = cnt ? lo[j] : 0.f;
        tf[LM_ATF(box_max) + j] = cnt ? hi[j] : 0.f;
    }
    tf[LM_ATF(score)] = score;
}

extern "C" int gf_label_map_batched(const long long* table, int S, long long max_points, int max_picks, float min_score,
                                    void* bits, float* part_f, int32_t* part_cnt, int32_t* own_part, int32_t* owner,
                                    int32_t* ids, int32_t* tab_i, float* tab_f, void* stream) {
    GF_CHECK_ARG(table && bits && part_f && part_cnt && own_part && owner && ids && tab_i && tab_f,
                 "gf_label_map_batched: null argument");
    GF_CHECK_ARG(S >= 0 && S <= 65535 && max_points >= 0 && max_picks >= 0 && max_picks <= GF_NMS_MAX_N,
                 "gf_label_map_batched: bad sizes S=%d max_points=%lld max_picks=%d", S, max_points, max_picks);
    const long long nch = (max_points + LM_CHUNK - 1) / LM_CHUNK;
    GF_CHECK_ARG(nch <= 0x7fffffffLL, "gf_label_map_batched: %lld points in a scene", max_points);
    if (S == 0) return GF_OK;
    hipStream_t st = (hipStream_t)stream;
    if (max_picks > 0 && nch > 0)
        hipLaunchKernelGGL(k_lm_pack, dim3((unsigned)nch, max_picks, S), dim3(256), 0, st, table, min_score,
                           (unsigned long long*)bits, part_f, part_cnt);
    if (nch > 0)
        hipLaunchKernelGGL(k_lm_owner, dim3((unsigned)gf_div_up(max_points, LM_OWN_THREADS), S), dim3(LM_OWN_THREADS), 0, st,
                           table, (const unsigned long long*)bits, min_score, owner, ids, own_part);
    if (max_picks > 0)  // (a scene without points still gets its rows: count 0)
        hipLaunchKernelGGL(k_lm_table, dim3((max_picks + 3) / 4, S), dim3(256), 0, st, table, part_f, part_cnt,
                           own_part, min_score, tab_i, tab_f);
    GF_CHECK_LAUNCH("gf_label_map_batched");
    return GF_OK;
}
