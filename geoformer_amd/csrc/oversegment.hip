// Geometric over-segmentation of one scene from its radius-limited kNN rows (gf_knn_radius' format): per-point normals
// (gf_point_normals) and a smoothness-constrained connected-components labelling (gf_smooth_components).  The host
// statement is postprocess.oversegment_host (stages A-D); see include/geoformer_hip.h for the arguments.
//
// gf_point_normals, one launch.  OS_GROUP = 8 lanes own a point (8 points per wave): lane l of the group takes the row
// entries l, l + 8, ..., so the group reads its row of I as consecutive words and every entry costs one 12-byte gather
// of xyz.  The ten sums (count, sum d, sum d d^T of the differences d = x_j - x_i) are reduced over the group by three
// DPP steps, every lane then holds the same words and runs the same OS_SWEEPS cyclic Jacobi sweeps on the 3x3
// covariance; lane 0 stores the point's 16 bytes.  One thread per point would issue the k gathers of a point from one
// lane and leave a 150k-point scene with two waves per SIMD to hide them; 8 lanes per point give eight times the
// waves and k / 8 gathers per lane, at the price of the Jacobi arithmetic (a few hundred flops) done eight-fold.
//
// gf_smooth_components, five launches, none of them repeated "until nothing changes":
//   k_sc_init     parent[i] = i, count[i] = 0
//   k_sc_hook     one thread per row entry: the edge test, then post_steps.h's lock-free min-index union
//                 (gf_uf_union): the root of a finished set is its smallest index.
//   k_sc_flatten  root[i] = find(i) for flat points (parent is read-only now), count[root] += 1 (integer atomicAdd) while
//                 the count is below min_points -- all the dissolve needs to know
//   k_sc_dissolve ids[i] = root[i] where count[root[i]] >= min_points, else -1; -1 for non-flat points
//   k_sc_attach   non-flat points only: the first entry j of the row that is flat, kept and has the point on its
//                 plane gives ids[i] = ids[j].  Reads ids of flat points, writes ids of non-flat points: no race.
// The partition and its min-index ids are a function of the inputs alone, so the result is bit-identical from call to
// call whatever the order in which the unions land.  No floating-point atomics.  An index outside [0, n) in a row is
// skipped, never followed, and only columns 0 .. min(deg[i], k - 1) of a row are read.
#include "common.h"
#include "post_steps.h"

namespace {

constexpr int OS_GROUP = 8;     // lanes per point in k_point_normals
constexpr int OS_THREADS = 256;
constexpr int OS_SWEEPS = 6;    // cyclic Jacobi sweeps of the 3x3 eigenproblem (fixed)
constexpr float OS_SIGN_EPS = 1e-6f;

__device__ __forceinline__ float os_group_sum(float s) {  // over the 8 lanes of a group: the same word in every lane
    s += gf_shfl_xor<4>(s);
    s += gf_shfl_xor<2>(s);
    s += gf_shfl_xor<1>(s);
    return s;
}

// one Jacobi rotation that annihilates a_pq of the symmetric matrix {app, aqq, apq, arp, arq} (r: the third index) and
// applies it to the columns p, q of the eigenvector matrix (v0p .. v2q: their three rows)
__device__ __forceinline__ void os_rotate(float& app, float& aqq, float& apq, float& arp, float& arq, float& v0p,
                                          float& v0q, float& v1p, float& v1q, float& v2p, float& v2q) {
    if (apq == 0.0f) return;
    const float theta = (aqq - app) / (2.0f * apq);
    const float t = copysignf(1.0f, theta) / (fabsf(theta) + sqrtf(fmaf(theta, theta, 1.0f)));
    const float c = 1.0f / sqrtf(fmaf(t, t, 1.0f)), s = t * c;
    app = fmaf(-t, apq, app);
    aqq = fmaf(t, apq, aqq);
    apq = 0.0f;
    const float rp = arp, rq = arq;
    arp = fmaf(c, rp, -s * rq);
    arq = fmaf(s, rp, c * rq);
    float vp = v0p, vq = v0q;
    v0p = fmaf(c, vp, -s * vq);
    v0q = fmaf(s, vp, c * vq);
    vp = v1p, vq = v1q;
    v1p = fmaf(c, vp, -s * vq);
    v1q = fmaf(s, vp, c * vq);
    vp = v2p, vq = v2q;
    v2p = fmaf(c, vp, -s * vq);
    v2q = fmaf(s, vp, c * vq);
}

__global__ __launch_bounds__(OS_THREADS) void k_point_normals(const float* __restrict__ xyz,
                                                              const int32_t* __restrict__ I,
                                                              const int32_t* __restrict__ deg, int n, int k,
                                                              float4* __restrict__ out) {
    const long long g = ((long long)blockIdx.x * OS_THREADS + threadIdx.x) / OS_GROUP;
    const int l = threadIdx.x % OS_GROUP;
    const bool live = g < n;
    const int i = live ? (int)g : 0;  // (every lane stays in the shuffles)
    float m = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, xx = 0.0f, xy = 0.0f, xz = 0.0f, yy = 0.0f, yz = 0.0f, zz = 0.0f;
    if (live) {
        const float px = xyz[(size_t)i * 3 + 0], py = xyz[(size_t)i * 3 + 1], pz = xyz[(size_t)i * 3 + 2];
        const int last = min(deg[i], k - 1);
        for (int c = l; c <= last; c += OS_GROUP) {
            const int j = I[(size_t)i * k + c];
            if ((unsigned)j >= (unsigned)n) continue;
            const float dx = xyz[(size_t)j * 3 + 0] - px, dy = xyz[(size_t)j * 3 + 1] - py,
                        dz = xyz[(size_t)j * 3 + 2] - pz;
            m += 1.0f;
            sx += dx; sy += dy; sz += dz;
            xx = fmaf(dx, dx, xx); xy = fmaf(dx, dy, xy); xz = fmaf(dx, dz, xz);
            yy = fmaf(dy, dy, yy); yz = fmaf(dy, dz, yz); zz = fmaf(dz, dz, zz);
        }
    }
    m = os_group_sum(m);
    sx = os_group_sum(sx); sy = os_group_sum(sy); sz = os_group_sum(sz);
    xx = os_group_sum(xx); xy = os_group_sum(xy); xz = os_group_sum(xz);
    yy = os_group_sum(yy); yz = os_group_sum(yz); zz = os_group_sum(zz);
    if (!live || l != 0) return;
    float4 res = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
    if (m >= 3.0f) {
        const float inv = 1.0f / m;
        const float mx = sx * inv, my = sy * inv, mz = sz * inv;
        // covariance about the neighbourhood's own mean
        float a00 = fmaf(-mx, mx, xx * inv), a01 = fmaf(-mx, my, xy * inv), a02 = fmaf(-mx, mz, xz * inv);
        float a11 = fmaf(-my, my, yy * inv), a12 = fmaf(-my, mz, yz * inv), a22 = fmaf(-mz, mz, zz * inv);
        float v00 = 1.0f, v01 = 0.0f, v02 = 0.0f, v10 = 0.0f, v11 = 1.0f, v12 = 0.0f, v20 = 0.0f, v21 = 0.0f, v22 = 1.0f;
#pragma unroll 1
        for (int s = 0; s < OS_SWEEPS; ++s) {
            os_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
            os_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
            os_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
        }
        // the smallest eigenvalue's column (the lowest index among equal ones)
        const bool b1 = a11 < a00;
        float l0 = b1 ? a11 : a00, nx = b1 ? v01 : v00, ny = b1 ? v11 : v10, nz = b1 ? v21 : v20;
        const bool b2 = a22 < l0;
        l0 = b2 ? a22 : l0; nx = b2 ? v02 : nx; ny = b2 ? v12 : ny; nz = b2 ? v22 : nz;
        const float r = 1.0f / sqrtf(fmaf(nx, nx, fmaf(ny, ny, nz * nz)));
        nx *= r; ny *= r; nz *= r;
        const float lead = fabsf(nx) > OS_SIGN_EPS ? nx : fabsf(ny) > OS_SIGN_EPS ? ny : fabsf(nz) > OS_SIGN_EPS ? nz : 1.0f;
        if (lead < 0.0f) { nx = -nx; ny = -ny; nz = -nz; }
        const float tr = a00 + a11 + a22;
        if (tr > 0.0f) res = make_float4(nx, ny, nz, fmaxf(l0, 0.0f) / tr);  // (all points in one place: invalid)
    }
    out[i] = res;
}

__device__ __forceinline__ bool sc_flat(const float4* __restrict__ nrm, int i, float flatness) {
    const float s = nrm[i].w;
    return s >= 0.0f && s <= flatness;
}

__device__ __forceinline__ float sc_plane_dist(const float4& nv, const float* __restrict__ xyz, int from, int to) {
    const float dx = xyz[(size_t)to * 3 + 0] - xyz[(size_t)from * 3 + 0],
                dy = xyz[(size_t)to * 3 + 1] - xyz[(size_t)from * 3 + 1],
                dz = xyz[(size_t)to * 3 + 2] - xyz[(size_t)from * 3 + 2];
    return fabsf(fmaf(nv.x, dx, fmaf(nv.y, dy, nv.z * dz)));
}

__global__ __launch_bounds__(OS_THREADS) void k_sc_init(int n, int32_t* __restrict__ parent,
                                                        int32_t* __restrict__ count) {
    const int i = blockIdx.x * OS_THREADS + threadIdx.x;
    if (i >= n) return;
    parent[i] = i;
    count[i] = 0;
}

__global__ __launch_bounds__(OS_THREADS) void k_sc_hook(const float* __restrict__ xyz, const float4* __restrict__ nrm,
                                                        const int32_t* __restrict__ I,
                                                        const int32_t* __restrict__ deg, int n, int k,
                                                        float cos_thresh, float offset, float flatness,
                                                        int32_t* parent) {
    const long long e = (long long)blockIdx.x * OS_THREADS + threadIdx.x;
    if (e >= (long long)n * k) return;
    const int i = (int)(e / k), c = (int)(e % k);
    if (c > deg[i]) return;
    const int j = I[e];
    if ((unsigned)j >= (unsigned)n || j == i) return;
    if (!sc_flat(nrm, i, flatness) || !sc_flat(nrm, j, flatness)) return;
    const float4 ni = nrm[i], nj = nrm[j];
    if (fabsf(fmaf(ni.x, nj.x, fmaf(ni.y, nj.y, ni.z * nj.z))) < cos_thresh) return;
    if (sc_plane_dist(ni, xyz, i, j) > offset) return;
    gf_uf_union<__HIP_MEMORY_SCOPE_AGENT>(parent, i, j);
}

__global__ __launch_bounds__(OS_THREADS) void k_sc_flatten(const float4* __restrict__ nrm, int n, float flatness,
                                                           int min_points, const int32_t* __restrict__ parent,
                                                           int32_t* __restrict__ root, int32_t* count) {
    const int i = blockIdx.x * OS_THREADS + threadIdx.x;
    if (i >= n) return;
    int r = -1;
    if (sc_flat(nrm, i, flatness)) {
        r = i;
        for (int p = parent[r]; p != r; p = parent[r]) r = p;
        // the count only has to tell whether the set reaches min_points: once it does, the adds to that word (tens of
        // thousands for a floor) stop.  A stale read only costs one more add; the count never exceeds the set's size.
        if (__hip_atomic_load(&count[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < min_points) atomicAdd(&count[r], 1);
    }
    root[i] = r;
}

__global__ __launch_bounds__(OS_THREADS) void k_sc_dissolve(int n, int min_points, const int32_t* __restrict__ root,
                                                            const int32_t* __restrict__ count,
                                                            int32_t* __restrict__ ids) {
    const int i = blockIdx.x * OS_THREADS + threadIdx.x;
    if (i >= n) return;
    const int r = root[i];
    ids[i] = (r >= 0 && count[r] >= min_points) ? r : -1;
}

__global__ __launch_bounds__(OS_THREADS) void k_sc_attach(const float* __restrict__ xyz, const float4* __restrict__ nrm,
                                                          const int32_t* __restrict__ I,
                                                          const int32_t* __restrict__ deg, int n, int k, float offset,
                                                          const int32_t* __restrict__ root, int32_t* ids) {
    const int i = blockIdx.x * OS_THREADS + threadIdx.x;
    if (i >= n || root[i] >= 0) return;  // flat points keep what k_sc_dissolve gave them
    const int last = min(deg[i], k - 1);
    for (int c = 0; c <= last; ++c) {
        const int j = I[(size_t)i * k + c];
        if ((unsigned)j >= (unsigned)n || root[j] < 0) continue;
        const int id = ids[j];  // a flat point's: final since k_sc_dissolve
        if (id < 0) continue;
        if (sc_plane_dist(nrm[j], xyz, j, i) <= offset) {
            ids[i] = id;
            return;
        }
    }
}

size_t sc_words(int n) { return ((size_t)(n > 0 ? n : 0) + 63) & ~(size_t)63; }

}  // namespace

extern "C" size_t gf_point_normals_scratch_bytes(int n) {
    (void)n;
    return 0;
}

extern "C" int gf_point_normals(const float* xyz, const int32_t* I, const int32_t* deg, int n, int k, float* out,
                                void* stream) {
    GF_CHECK_ARG(n >= 0 && k >= 1, "gf_point_normals: n = %d points, k = %d columns", n, k);
    GF_CHECK_ARG(n == 0 || (xyz && I && deg && out), "gf_point_normals: NULL xyz, I, deg or out");
    GF_CHECK_ARG(((uintptr_t)out & 15) == 0, "gf_point_normals: out must be 16-byte aligned");
    if (n == 0) return GF_OK;
    hipLaunchKernelGGL(k_point_normals, dim3(gf_div_up((long long)n * OS_GROUP, OS_THREADS)), dim3(OS_THREADS), 0,
                       (hipStream_t)stream, xyz, I, deg, n, k, (float4*)out);
    GF_CHECK_LAUNCH("gf_point_normals");
    return GF_OK;
}

extern "C" size_t gf_smooth_components_scratch_bytes(int n) { return 3 * sc_words(n) * sizeof(int32_t); }

extern "C" int gf_smooth_components(const float* xyz, const float* normals4, const int32_t* I, const int32_t* deg, int n,
                                    int k, float cos_thresh, float offset, float flatness, int min_points,
                                    int32_t* ids_out, void* scratch, void* stream) {
    GF_CHECK_ARG(n >= 0 && k >= 1, "gf_smooth_components: n = %d points, k = %d columns", n, k);
    GF_CHECK_ARG(min_points >= 1, "gf_smooth_components: min_points = %d (at least 1)", min_points);
    GF_CHECK_ARG(n == 0 || (xyz && normals4 && I && deg && ids_out && scratch),
                 "gf_smooth_components: NULL xyz, normals4, I, deg, ids_out or scratch");
    GF_CHECK_ARG(((uintptr_t)normals4 & 15) == 0, "gf_smooth_components: normals4 must be 16-byte aligned");
    GF_CHECK_ARG((long long)n * k <= 0x7fffffffLL * OS_THREADS, "gf_smooth_components: n * k = %lld row entries",
                 (long long)n * k);
    if (n == 0) return GF_OK;
    hipStream_t st = (hipStream_t)stream;
    int32_t* parent = (int32_t*)scratch;
    int32_t* count = parent + sc_words(n);
    int32_t* root = count + sc_words(n);
    const float4* nrm = (const float4*)normals4;
    const dim3 pts(gf_div_up(n, OS_THREADS)), blk(OS_THREADS);
    hipLaunchKernelGGL(k_sc_init, pts, blk, 0, st, n, parent, count);
    hipLaunchKernelGGL(k_sc_hook, dim3(gf_div_up((long long)n * k, OS_THREADS)), blk, 0, st, xyz, nrm, I, deg, n, k,
                       cos_thresh, offset, flatness, parent);
    hipLaunchKernelGGL(k_sc_flatten, pts, blk, 0, st, nrm, n, flatness, min_points, parent, root, count);
    hipLaunchKernelGGL(k_sc_dissolve, pts, blk, 0, st, n, min_points, root, count, ids_out);
    hipLaunchKernelGGL(k_sc_attach, pts, blk, 0, st, xyz, nrm, I, deg, n, k, offset, root, ids_out);
    GF_CHECK_LAUNCH("gf_smooth_components");
    return GF_OK;
}
