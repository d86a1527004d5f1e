// 3D boxes of instances and the IoU of boxes (the statements are postprocess.instance_boxes_host / box_iou_host).
// A box is upright: oriented about z only.  Per group of points the call gives a count, the axis-aligned box and the
// box of least footprint among A headings of a table of (cos, sin) pairs.
//
// gf_instance_boxes_batched, S scenes, two memsets and two launches whatever S, the group counts and the forms:
//   k_box_extents  grid (chunks, groups, S), 256 threads: one workgroup per (group r, chunk of BOX_CHUNK points) finds
//                  the chunk's members of the group (rows form: masks[pick[r]] != 0; ids form: group[pt] == r), stages
//                  their xyz in LDS (in any order: only extents are taken) and walks them once per slot: thread a < A
//                  takes the extents of u and v at heading a, thread A those of x and y themselves, thread A + 1 those
//                  of z.  Every thread of a wave reads the same LDS word (a broadcast).  The four words of a slot are
//                  merged into kmin / kmax[row, slot] with integer atomicMin / atomicMax on order-preserving keys
//                  (gf_float_key); kmin starts as all-ones, kmax and the counts as zeros.
//   k_box_rows     one wave per group: the area of every heading, the least (lowest index among equals) by a fixed
//                  tree, and the two float64 rows.
// Only extents and integer counts are reduced, and a maximum of integers does not depend on the order of arrival: the
// outputs are bit-identical from call to call and to the numpy statement.  Coordinates are finite (no NaN, no inf).
//
// gf_box_iou_batched, one launch: one thread per (prediction, ground truth) pair of every scene, float64, every
// operation rounded on its own, no sin / cos: the boxes carry them.
#include "common.h"
#include "post_steps.h"

#define BOX_FLOATS GF_BOX_FLOATS
#define BOX_AT(member) (offsetof(GfBox, member) / sizeof(double))
#define BOX_THREADS 256
#define BOX_CHUNK 2048                    // points per workgroup: eight per thread
#define BOX_PER_THREAD (BOX_CHUNK / BOX_THREADS)
#define BOX_MAX_ANGLES 192                // A + 2 slots <= BOX_THREADS
#define BOX_MAX_GROUPS 65535              // grid.y
static_assert(sizeof(GfBoxScene) == 8 * GF_BOX_SCENE_FIELDS && sizeof(GfBoxIouScene) == 8 * GF_BOX_IOU_FIELDS &&
                  sizeof(GfBox) == 8 * GF_BOX_FLOATS, "the rows of include/geoformer_hip.h");

extern "C" int gf_box_chunk(void) { return BOX_CHUNK; }
extern "C" int gf_box_max_angles(void) { return BOX_MAX_ANGLES; }
extern "C" int gf_box_max_groups(void) { return BOX_MAX_GROUPS; }

__global__ __launch_bounds__(BOX_THREADS) void k_box_extents(const long long* __restrict__ table,
                                                             const float* __restrict__ ang, int A,
                                                             uint32_t* __restrict__ kmin, uint32_t* __restrict__ kmax,
                                                             int32_t* __restrict__ cnt) {
    __shared__ float s_x[BOX_CHUNK], s_y[BOX_CHUNK], s_z[BOX_CHUNK];
    __shared__ int s_n;
    const GfBoxScene* t = gf_row<GfBoxScene>(table, blockIdx.z);
    const long long N = t->N, n = t->n, p = t->p;
    const long long nch = (N + BOX_CHUNK - 1) / BOX_CHUNK;
    const long long r = blockIdx.y, c = blockIdx.x;
    if (r >= p || c >= nch) return;  // (uniform over the workgroup)
    const bool rows = t->form == GF_BOX_FORM_ROWS;
    const int32_t* g = (const int32_t*)t->group;
    int want = (int)r;  // ids form: the members are the points whose group is r
    if (rows) {
        const long long row = ((const long long*)t->pick)[r];
        if (row < 0 || row >= n) return;  // (a pick outside the masks is an empty group, never an address)
        g += row * N;
    }
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    // the chunk's words first, all in flight together: unconditional, a point past the end reads the last one
    const long long p0 = c * BOX_CHUNK + threadIdx.x;
    int v[BOX_PER_THREAD];
#pragma unroll
    for (int k = 0; k < BOX_PER_THREAD; k++) {
        const long long pt = p0 + (long long)k * BOX_THREADS;
        v[k] = g[pt < N ? pt : N - 1];
    }
    const float* xyz = (const float*)t->xyz;
#pragma unroll
    for (int k = 0; k < BOX_PER_THREAD; k++) {
        const long long pt = p0 + (long long)k * BOX_THREADS;
        const bool on = pt < N && (rows ? v[k] != 0 : v[k] == want);
        if (on) {
            const int slot = atomicAdd(&s_n, 1);  // (LDS, integers; at most BOX_CHUNK points reach here)
            const float* q = xyz + pt * 3;
            s_x[slot] = q[0], s_y[slot] = q[1], s_z[slot] = q[2];
        }
    }
    __syncthreads();
    const int m = s_n;
    if (m == 0) return;
    const int a = threadIdx.x;
    if (a >= A + 2) return;
    // slot a < A: heading a; slot A: x and y as they are; slot A + 1: z (its second pair stays empty)
    uint32_t lo0 = 0xffffffffu, hi0 = 0u, lo1 = 0xffffffffu, hi1 = 0u;
    if (a < A) {
        const float cs = ang[2 * a], sn = ang[2 * a + 1];
        for (int i = 0; i < m; i++) {
            const float x = s_x[i], y = s_y[i];
            const uint32_t ku = gf_float_key(__fadd_rn(__fmul_rn(x, cs), __fmul_rn(y, sn)));
            const uint32_t kv = gf_float_key(__fsub_rn(__fmul_rn(y, cs), __fmul_rn(x, sn)));
            lo0 = min(lo0, ku), hi0 = max(hi0, ku), lo1 = min(lo1, kv), hi1 = max(hi1, kv);
        }
    } else if (a == A) {
        for (int i = 0; i < m; i++) {
            const uint32_t ku = gf_float_key(s_x[i]), kv = gf_float_key(s_y[i]);
            lo0 = min(lo0, ku), hi0 = max(hi0, ku), lo1 = min(lo1, kv), hi1 = max(hi1, kv);
        }
    } else {
        for (int i = 0; i < m; i++) {
            const uint32_t kz = gf_float_key(s_z[i]);
            lo0 = min(lo0, kz), hi0 = max(hi0, kz);
        }
    }
    const long long row_out = t->row_off + r;
    const long long k2 = (row_out * (A + 2) + a) * 2;
    atomicMin(&kmin[k2], lo0);
    atomicMax(&kmax[k2], hi0);
    if (a <= A) {
        atomicMin(&kmin[k2 + 1], lo1);
        atomicMax(&kmax[k2 + 1], hi1);
    } else {
        atomicAdd(&cnt[row_out], m);  // (integers: exact in any order)
    }
}

// lo, hi: the slot's two minima / maxima (u, v); zlo, zhi: the first word of the z slot's
__device__ __forceinline__ void box_write_row(GfBox& o, const uint32_t* lo, const uint32_t* hi, uint32_t kzlo,
                                              uint32_t kzhi, float cs, float sn, int index, int count) {
    // sizes and frame-local centres in float64 from the fp32 extents: exact
    const double ulo = gf_float_unkey(lo[0]), uhi = gf_float_unkey(hi[0]);
    const double vlo = gf_float_unkey(lo[1]), vhi = gf_float_unkey(hi[1]);
    const double zlo = gf_float_unkey(kzlo), zhi = gf_float_unkey(kzhi);
    const double lu = __dmul_rn(__dadd_rn(ulo, uhi), 0.5), lv = __dmul_rn(__dadd_rn(vlo, vhi), 0.5);
    const double c = cs, s = sn;
    o.cx = __dsub_rn(__dmul_rn(lu, c), __dmul_rn(lv, s));
    o.cy = __dadd_rn(__dmul_rn(lu, s), __dmul_rn(lv, c));
    o.cz = __dmul_rn(__dadd_rn(zlo, zhi), 0.5);
    o.du = __dsub_rn(uhi, ulo);
    o.dv = __dsub_rn(vhi, vlo);
    o.dz = __dsub_rn(zhi, zlo);
    o.c = c;
    o.s = s;
    o.angle = (double)index;
    o.count = (double)count;
}

// (area, index) <- the lesser of the lane's own and lane ^ D's: the lesser area, the lower index among equals; an index
// of INT_MAX marks a lane without a heading
template <int D>
__device__ __forceinline__ void box_take(float& best, int& at) {
    const float ob = gf_shfl_xor<D>(best);
    const int oa = gf_shfl_xor_i<D>(at);
    const bool take = oa != 0x7fffffff && (at == 0x7fffffff || ob < best || (ob == best && oa < at));
    best = take ? ob : best;
    at = take ? oa : at;
}

// one wave per row of the packed outputs
__global__ __launch_bounds__(256) void k_box_rows(const float* __restrict__ ang, int A, long long rows,
                                                  const uint32_t* __restrict__ kmin, const uint32_t* __restrict__ kmax,
                                                  const int32_t* __restrict__ cnt,
                                                  int32_t* __restrict__ count, double* __restrict__ aligned,
                                                  double* __restrict__ oriented) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;  // (wave-uniform)
    const int m = cnt[row];
    const uint32_t* lo = kmin + row * (A + 2) * 2;
    const uint32_t* hi = kmax + row * (A + 2) * 2;
    // lane l: headings l, l + 64, ... in ascending order, a strict compare keeps the lowest index among equal areas
    float best = INFINITY;
    int at = 0x7fffffff;
    if (m > 0) {
        for (int a = lane; a < A; a += 64) {
            const float du = __fsub_rn(gf_float_unkey(hi[2 * a]), gf_float_unkey(lo[2 * a]));
            const float dv = __fsub_rn(gf_float_unkey(hi[2 * a + 1]), gf_float_unkey(lo[2 * a + 1]));
            const float area = __fmul_rn(du, dv);
            if (area < best || at == 0x7fffffff) best = area, at = a;
        }
    }
    box_take<32>(best, at), box_take<16>(best, at), box_take<8>(best, at);
    box_take<4>(best, at), box_take<2>(best, at), box_take<1>(best, at);
    if (lane != 0) return;
    double* oa = aligned + row * BOX_FLOATS;
    double* oo = oriented + row * BOX_FLOATS;
    count[row] = m;
    if (m <= 0) {
        for (int j = 0; j < BOX_FLOATS; j++) oa[j] = 0.0, oo[j] = 0.0;
        return;
    }
    const uint32_t kzlo = lo[2 * (A + 1)], kzhi = hi[2 * (A + 1)];
    box_write_row(*(GfBox*)oa, lo + 2 * A, hi + 2 * A, kzlo, kzhi, 1.f, 0.f, 0, m);
    box_write_row(*(GfBox*)oo, lo + 2 * at, hi + 2 * at, kzlo, kzhi, ang[2 * at], ang[2 * at + 1], at, m);
}

extern "C" size_t gf_instance_boxes_scratch_bytes(long long rows, int A) {
    if (rows < 0 || A < 1 || A > BOX_MAX_ANGLES) return 0;
    return (size_t)rows * ((size_t)(A + 2) * 4 + 1) * sizeof(uint32_t);
}

extern "C" int gf_instance_boxes_batched(const long long* table, int S, long long max_points, int max_groups,
                                         long long rows, const float* angles, int A, void* scratch, int32_t* count,
                                         double* aligned, double* oriented, void* stream) {
    GF_CHECK_ARG(S >= 0 && S <= 65535 && max_points >= 0 && max_groups >= 0 && max_groups <= BOX_MAX_GROUPS && rows >= 0,
                 "gf_instance_boxes_batched: bad sizes S=%d max_points=%lld max_groups=%d rows=%lld", S, max_points,
                 max_groups, rows);
    GF_CHECK_ARG(A >= 1 && A <= BOX_MAX_ANGLES, "gf_instance_boxes_batched: %d angles (1 to %d)", A, BOX_MAX_ANGLES);
    const long long nch = (max_points + BOX_CHUNK - 1) / BOX_CHUNK;
    GF_CHECK_ARG(nch <= 0xffffffLL && rows <= 0x7fffffffLL, "gf_instance_boxes_batched: %lld points in a scene, %lld rows",
                 max_points, rows);
    if (S == 0 || rows == 0) return GF_OK;
    GF_CHECK_ARG(table && angles && scratch && count && aligned && oriented, "gf_instance_boxes_batched: null argument");
    hipStream_t st = (hipStream_t)stream;
    // scratch: kmax [rows, A + 2, 2] and cnt [rows] (zeros), then kmin [rows, A + 2, 2] (all-ones)
    const size_t half = (size_t)rows * (A + 2) * 2;
    uint32_t* kmax = (uint32_t*)scratch;
    int32_t* cnt = (int32_t*)(kmax + half);
    uint32_t* kmin = kmax + half + rows;
    GF_TRY(hipMemsetAsync(kmax, 0, (half + rows) * sizeof(uint32_t), st));
    GF_TRY(hipMemsetAsync(kmin, 0xff, half * sizeof(uint32_t), st));
    if (max_groups > 0 && nch > 0)
        hipLaunchKernelGGL(k_box_extents, dim3((unsigned)nch, max_groups, S), dim3(BOX_THREADS), 0, st, table, angles, A,
                           kmin, kmax, cnt);
    hipLaunchKernelGGL(k_box_rows, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, angles, A, rows, kmin, kmax, cnt,
                       count, aligned, oriented);
    GF_CHECK_LAUNCH("gf_instance_boxes_batched");
    return GF_OK;
}

// ---- IoU of upright boxes ------------------------------------------------------------------------------------------------
// the overlap of [-ha, ha] with [d - hb, d + hb]: exactly 2 ha for d == 0 and ha == hb
__device__ __forceinline__ double box_overlap_1d(double d, double ha, double hb) {
    const double hi = fmin(ha, __dadd_rn(d, hb)), lo = fmax(-ha, __dsub_rn(d, hb));
    const double o = __dsub_rn(hi, lo);
    return o > 0.0 ? o : 0.0;
}

// One pass of Sutherland-Hodgman: the convex polygon (pu, pv)[0 .. m) against the half-plane sign * w >= -h, with w the
// first coordinate (axis 0) or the second (axis 1); written as w' = sign * w >= -h so that the four passes share the code.
// Returns the number of vertices of the result (at most 8 are kept: a rectangle cut four times has no more).
__device__ __forceinline__ int box_clip(const double* pu, const double* pv, int m, int axis, double sign, double h,
                                        double* qu, double* qv) {
    const double k = sign > 0.0 ? -h : h;  // the line w = k; inside: sign * w >= sign * k
    int out = 0;
    for (int i = 0; i < m; i++) {
        const int j = i == 0 ? m - 1 : i - 1;
        const double cw = axis ? pv[i] : pu[i], co = axis ? pu[i] : pv[i];
        const double lw = axis ? pv[j] : pu[j], lo = axis ? pu[j] : pv[j];
        const bool cin = sign > 0.0 ? cw >= k : cw <= k, lin = sign > 0.0 ? lw >= k : lw <= k;
        if (cin != lin) {  // the edge from the previous vertex crosses the line
            const double tt = __ddiv_rn(__dsub_rn(k, lw), __dsub_rn(cw, lw));
            const double io = __dadd_rn(lo, __dmul_rn(tt, __dsub_rn(co, lo)));
            if (out < 8) {
                qu[out] = axis ? io : k, qv[out] = axis ? k : io;
                out++;
            }
        }
        if (cin && out < 8) {
            qu[out] = pu[i], qv[out] = pv[i];
            out++;
        }
    }
    return out;
}

__global__ __launch_bounds__(256) void k_box_iou(const long long* __restrict__ table, const double* __restrict__ a,
                                                 const double* __restrict__ b, double* __restrict__ out) {
    const GfBoxIouScene* t = gf_row<GfBoxIouScene>(table, blockIdx.y);
    const long long P = t->P, G = t->G;
    const long long pair = (long long)blockIdx.x * 256 + threadIdx.x;
    if (pair >= P * G) return;
    // the rows stay float64 words at the struct's offsets: read through GfBox, the loads are scheduled differently
    enum : int { CX = BOX_AT(cx), CY = BOX_AT(cy), CZ = BOX_AT(cz), DU = BOX_AT(du), DV = BOX_AT(dv), DZ = BOX_AT(dz),
                 C = BOX_AT(c), S = BOX_AT(s) };
    const double* A = a + (t->a_off + pair / G) * BOX_FLOATS;
    const double* B = b + (t->b_off + pair % G) * BOX_FLOATS;
    const double hau = __dmul_rn(A[DU], 0.5), hav = __dmul_rn(A[DV], 0.5), haz = __dmul_rn(A[DZ], 0.5);
    const double hbu = __dmul_rn(B[DU], 0.5), hbv = __dmul_rn(B[DV], 0.5), hbz = __dmul_rn(B[DZ], 0.5);
    const double volA = __dmul_rn(__dmul_rn(A[DU], A[DV]), A[DZ]), volB = __dmul_rn(__dmul_rn(B[DU], B[DV]), B[DZ]);
    const double oz = box_overlap_1d(__dsub_rn(B[CZ], A[CZ]), haz, hbz);
    double area;
    if (A[S] == 0.0 && B[S] == 0.0) {  // both along the axes: interval overlaps
        area = __dmul_rn(box_overlap_1d(__dsub_rn(B[CX], A[CX]), hau, hbu),
                         box_overlap_1d(__dsub_rn(B[CY], A[CY]), hav, hbv));
    } else {
        // a's rectangle in b's frame, counter-clockwise, cut by b's four sides
        const double ca = A[C], sa = A[S], cb = B[C], sb = B[S];
        const double dx = __dsub_rn(A[CX], B[CX]), dy = __dsub_rn(A[CY], B[CY]);
        const double cu = __dadd_rn(__dmul_rn(dx, cb), __dmul_rn(dy, sb));
        const double cv = __dsub_rn(__dmul_rn(dy, cb), __dmul_rn(dx, sb));
        const double cr = __dadd_rn(__dmul_rn(ca, cb), __dmul_rn(sa, sb));
        const double sr = __dsub_rn(__dmul_rn(sa, cb), __dmul_rn(ca, sb));
        const double ux = __dmul_rn(hau, cr), uy = __dmul_rn(hau, sr);  // half the u side
        const double vx = __dmul_rn(hav, sr), vy = __dmul_rn(hav, cr);  // half the v side is (-vx, vy)
        double pu[8], pv[8], qu[8], qv[8];
        pu[0] = __dadd_rn(__dsub_rn(cu, ux), vx), pv[0] = __dsub_rn(__dsub_rn(cv, uy), vy);
        pu[1] = __dadd_rn(__dadd_rn(cu, ux), vx), pv[1] = __dsub_rn(__dadd_rn(cv, uy), vy);
        pu[2] = __dsub_rn(__dadd_rn(cu, ux), vx), pv[2] = __dadd_rn(__dadd_rn(cv, uy), vy);
        pu[3] = __dsub_rn(__dsub_rn(cu, ux), vx), pv[3] = __dadd_rn(__dsub_rn(cv, uy), vy);
        int m = box_clip(pu, pv, 4, 0, 1.0, hbu, qu, qv);
        m = box_clip(qu, qv, m, 0, -1.0, hbu, pu, pv);
        m = box_clip(pu, pv, m, 1, 1.0, hbv, qu, qv);
        m = box_clip(qu, qv, m, 1, -1.0, hbv, pu, pv);
        double acc = 0.0;  // the shoelace sum in vertex order
        for (int i = 0; i < m; i++) {
            const int j = i + 1 == m ? 0 : i + 1;
            acc = __dadd_rn(acc, __dsub_rn(__dmul_rn(pu[i], pv[j]), __dmul_rn(pu[j], pv[i])));
        }
        area = m >= 3 ? __dmul_rn(fabs(acc), 0.5) : 0.0;
    }
    double inter = __dmul_rn(area, oz);
    if (!(volA > 0.0) || !(volB > 0.0)) inter = 0.0;  // a box without volume overlaps nothing
    const double den = __dsub_rn(__dadd_rn(volA, volB), inter);
    out[t->out_off + pair] = den > 0.0 ? __ddiv_rn(inter, den) : 0.0;
}

extern "C" int gf_box_iou_batched(const long long* table, int S, long long max_pairs, const double* a, const double* b,
                                  double* out, void* stream) {
    GF_CHECK_ARG(S >= 0 && S <= 65535 && max_pairs >= 0 && max_pairs <= 0x7fffffffLL,
                 "gf_box_iou_batched: bad sizes S=%d max_pairs=%lld", S, max_pairs);
    if (S == 0 || max_pairs == 0) return GF_OK;
    GF_CHECK_ARG(table && a && b && out, "gf_box_iou_batched: null argument");
    hipLaunchKernelGGL(k_box_iou, dim3((unsigned)((max_pairs + 255) / 256), S), dim3(256), 0, (hipStream_t)stream, table,
                       a, b, out);
    GF_CHECK_LAUNCH("gf_box_iou_batched");
    return GF_OK;
}
