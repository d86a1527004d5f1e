// Headless rendering of a scene's points: a z-buffered point splat and a resolve pass (the host statement is
// render.splat_host / render.resolve_host; see include/geoformer_hip.h for the arguments and the arithmetic).
//
// The z-buffer is one 64-bit word per sub-pixel, (depthkey << 32 | point index), preset to all-ones by the caller's
// memset; the splat lowers it with atomicMin, so the nearest point wins, the lower index among equal depths, whatever
// the order of arrival: integer atomics only, bit-identical from call to call.
//   k_rd_splat_thread  max_radius <= RD_SMALL_RADIUS: one thread per (point, view), grid (ceil(N / 256), V).  The
//                      thread projects its point and walks the (2r + 1)^2 box of its disc (at most 49 cells, 37 of them
//                      in the disc).  The view's camera record is read through a uniform address (scalar loads).
//   k_rd_splat_wave    above: the same grid, but a wave projects its 64 points, one per lane, and then takes the points
//                      that survived one after the other (ballot, the point's pixel, radius and depth key broadcast
//                      with __shfl): the 64 lanes cover the point's box, cell = lane + 64 i, so a radius-16 disc
//                      (1089 cells) is 18 steps of the wave and not 1089 of one lane, and the radii of a perspective
//                      view may differ from lane to lane without divergence.
//   Both read the cell with a plain load first and skip the atomic when the key is not smaller: the cell only ever
//   decreases, so a stale (larger) value read from a cache costs an atomic and never loses one.
//   k_rd_resolve       one thread per output pixel, block 64 x 4, grid (ceil(W / 64), ceil(H / 4), V), the
//                      supersampling factor a template parameter: S x S sub-pixels each, per sub-pixel its key, the 8
//                      neighbours at the shading stride, the right and the lower neighbour (keys that neighbouring
//                      threads read too: L1 / L2 hits), one index store; per pixel three byte stores.
// No footprint leaves the image and no index leaves [0, N) whatever the camera records or the keys hold: every
// coordinate is clipped against the image before it becomes an address, every radius is clamped to max_radius, and a
// key whose low word is not below N is background.  Every offset into keys / index / image is formed in 64 bits.
#include "common.h"
#include "post_steps.h"

namespace {

constexpr int RD_F = 20;  // floats per camera record
constexpr int RD_MAX_VIEWS = 64;
constexpr int RD_MAX_SIDE = 4096;
constexpr int RD_MAX_RADIUS = 16;
constexpr int RD_MAX_SS = 4;
constexpr int RD_SMALL_RADIUS = 3;  // the largest max_radius of the thread-per-point kernel
constexpr int RD_MAX_STRIDE = 16;
constexpr int RD_THREADS = 256;

typedef unsigned long long u64;

// camera record: eye 0..2, R 3..11, kind 12, scale 13, cx 14, cy 15, near 16, spx 17, rmin 18, rmax 19
__device__ __forceinline__ bool rd_project(const float* __restrict__ c, float px, float py, float pz, int Ws, int Hs,
                                           int maxr, int& iu, int& iv, int& r, unsigned& dk) {
    const float d0 = px - c[0], d1 = py - c[1], d2 = pz - c[2];
    const float xc = (c[3] * d0 + c[4] * d1) + c[5] * d2;
    const float yc = (c[6] * d0 + c[7] * d1) + c[8] * d2;
    const float zc = (c[9] * d0 + c[10] * d1) + c[11] * d2;
    float rm = c[19];
    if (!(rm <= (float)maxr)) rm = (float)maxr;  // (a record above the caller's bound, or NaN)
    float u, v, rf = c[18];
    if (c[12] != 0.0f) {
        if (!(zc >= c[16])) return false;
        u = __fdiv_rn(xc * c[13], zc) + c[14];
        v = __fdiv_rn(yc * c[13], zc) + c[15];
        const float q = floorf(__fdiv_rn(c[17], zc));
        if (q > rf) rf = q;
    } else {
        u = xc * c[13] + c[14];
        v = yc * c[13] + c[15];
    }
    if (rf > rm) rf = rm;
    if (!(rf >= 0.0f)) rf = 0.0f;
    const float m = rm + 1.0f;
    if (!(u >= -m && u < (float)Ws + m)) return false;  // NaN fails both
    if (!(v >= -m && v < (float)Hs + m)) return false;
    iu = (int)floorf(u);
    iv = (int)floorf(v);
    r = (int)rf;
    dk = gf_float_key(zc);
    return true;
}

__device__ __forceinline__ void rd_lower(u64* cell, u64 key) {
    if (key < *cell) atomicMin(cell, key);
}

__global__ __launch_bounds__(RD_THREADS) void k_rd_splat_thread(const float* __restrict__ xyz,
                                                                const unsigned char* __restrict__ keep, long long N,
                                                                const float* __restrict__ cams, int Ws, int Hs, int maxr,
                                                                u64* keys) {
    const long long i = (long long)blockIdx.x * RD_THREADS + threadIdx.x;
    if (i >= N) return;
    if (keep && !keep[i]) return;
    int iu, iv, r;
    unsigned dk;
    if (!rd_project(cams + (long long)blockIdx.y * RD_F, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], Ws, Hs, maxr, iu, iv,
                    r, dk))
        return;
    const u64 key = ((u64)dk << 32) | (u64)i;
    u64* img = keys + (long long)blockIdx.y * Hs * Ws;
    const int r2 = r * r + r;
    for (int dy = -r; dy <= r; ++dy) {
        const int y = iv + dy;
        if ((unsigned)y >= (unsigned)Hs) continue;
        for (int dx = -r; dx <= r; ++dx) {
            const int x = iu + dx;
            if ((unsigned)x >= (unsigned)Ws || dx * dx + dy * dy > r2) continue;
            rd_lower(img + (long long)y * Ws + x, key);
        }
    }
}

__global__ __launch_bounds__(RD_THREADS) void k_rd_splat_wave(const float* __restrict__ xyz,
                                                              const unsigned char* __restrict__ keep, long long N,
                                                              const float* __restrict__ cams, int Ws, int Hs, int maxr,
                                                              u64* keys) {
    const int lane = threadIdx.x & (GF_WAVE - 1);
    const long long i = (long long)blockIdx.x * RD_THREADS + threadIdx.x;
    int iu = 0, iv = 0, r = 0;
    unsigned dk = 0;
    bool ok = i < N && (!keep || keep[i]);
    if (ok)
        ok = rd_project(cams + (long long)blockIdx.y * RD_F, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], Ws, Hs, maxr, iu,
                        iv, r, dk);
    u64* img = keys + (long long)blockIdx.y * Hs * Ws;
    u64 live = __ballot(ok);  // (every lane of the wave is here: none has returned)
    while (live) {
        const int src = __ffsll((long long)live) - 1;
        live &= live - 1;
        const int su = __shfl(iu, src, GF_WAVE), sv = __shfl(iv, src, GF_WAVE), sr = __shfl(r, src, GF_WAVE);
        const u64 key = ((u64)(unsigned)__shfl((int)dk, src, GF_WAVE) << 32) | (u64)(i - lane + src);
        const int side = 2 * sr + 1, cells = side * side, r2 = sr * sr + sr;
        // (row, column) of cell lane + 64 k without a division per step: side <= 33, so (n + 0.5) / side is at least
        // 0.5 / 33 away from an integer and the approximate reciprocal gives the exact quotient
        const float inv = __builtin_amdgcn_rcpf((float)side);
        int row = (int)(((float)lane + 0.5f) * inv), col = lane - row * side;
        const int step_r = (int)(((float)GF_WAVE + 0.5f) * inv), step_c = GF_WAVE - step_r * side;
        for (int c = lane; c < cells; c += GF_WAVE) {
            const int dx = col - sr, dy = row - sr, x = su + dx, y = sv + dy;
            if ((unsigned)x < (unsigned)Ws && (unsigned)y < (unsigned)Hs && dx * dx + dy * dy <= r2)
                rd_lower(img + (long long)y * Ws + x, key);
            row += step_r;
            col += step_c;
            if (col >= side) {
                col -= side;
                ++row;
            }
        }
    }
}

struct RdShade {
    int lut[9];
    int stride;
    float dz;
    int background, outline;
};

// gf_float_unkey written another way (written out: the shared form makes k_rd_resolve 2 % shorter, a change to measure)
__device__ __forceinline__ float rd_depth(unsigned dk) {
    return __uint_as_float((dk & 0x80000000u) ? (dk ^ 0x80000000u) : ~dk);
}

template <int S>
__global__ __launch_bounds__(RD_THREADS) void k_rd_resolve(const u64* __restrict__ keys, int W, int H,
                                                           const unsigned char* __restrict__ rgb,
                                                           const int32_t* __restrict__ ids, long long N, RdShade sh,
                                                           unsigned char* __restrict__ image,
                                                           int32_t* __restrict__ index) {
    const int x = blockIdx.x * GF_WAVE + threadIdx.x, y = blockIdx.y * (RD_THREADS / GF_WAVE) + threadIdx.y;
    if (x >= W || y >= H) return;
    const int Ws = W * S, Hs = H * S, st = sh.stride;
    const long long plane = (long long)blockIdx.z * Hs * Ws;
    const u64* img = keys + plane;
    int32_t* idx = index + plane;
    const u64 n = (u64)N;
    int sum[3] = {0, 0, 0};
#pragma unroll
    for (int sy = 0; sy < S; ++sy) {
#pragma unroll
        for (int sx = 0; sx < S; ++sx) {
            const int px = x * S + sx, py = y * S + sy;
            const long long at = (long long)py * Ws + px;
            const u64 k = img[at];
            const unsigned lo = (unsigned)k;
            const bool fg = (u64)lo < n;
            idx[at] = fg ? (int)lo : -1;
            int c[3] = {(sh.background >> 16) & 255, (sh.background >> 8) & 255, sh.background & 255};
            if (fg) {
                const float z = rd_depth((unsigned)(k >> 32));
                int o = 0;
#pragma unroll
                for (int ny = -1; ny <= 1; ++ny) {
#pragma unroll
                    for (int nx = -1; nx <= 1; ++nx) {
                        if (nx == 0 && ny == 0) continue;
                        const int qx = px + nx * st, qy = py + ny * st;
                        if ((unsigned)qx >= (unsigned)Ws || (unsigned)qy >= (unsigned)Hs) continue;
                        const u64 kn = img[(long long)qy * Ws + qx];
                        if ((u64)(unsigned)kn < n && rd_depth((unsigned)(kn >> 32)) + sh.dz < z) ++o;
                    }
                }
                bool edge = false;
                if (ids) {
                    const int mine = ids[lo];
                    if (px + 1 < Ws) {
                        const unsigned ln = (unsigned)img[at + 1];
                        edge = !((u64)ln < n) || ids[ln] != mine;
                    }
                    if (!edge && py + 1 < Hs) {
                        const unsigned ln = (unsigned)img[at + Ws];
                        edge = !((u64)ln < n) || ids[ln] != mine;
                    }
                }
                if (edge) {
                    c[0] = (sh.outline >> 16) & 255, c[1] = (sh.outline >> 8) & 255, c[2] = sh.outline & 255;
                } else {
                    int w = sh.lut[0];  // (selects, not an indexed read: the table stays in scalar registers)
#pragma unroll
                    for (int j = 1; j < 9; ++j) w = o == j ? sh.lut[j] : w;
                    const unsigned char* p = rgb + 3 * (long long)lo;
#pragma unroll
                    for (int j = 0; j < 3; ++j) c[j] = ((int)p[j] * w + 128) >> 8;
                }
            }
#pragma unroll
            for (int j = 0; j < 3; ++j) sum[j] += c[j];
        }
    }
    unsigned char* out = image + (((long long)blockIdx.z * H + y) * W + x) * 3;
#pragma unroll
    for (int j = 0; j < 3; ++j) out[j] = (unsigned char)((sum[j] + S * S / 2) / (S * S));
}

}  // namespace

extern "C" int gf_render_camera_floats(void) { return RD_F; }
extern "C" int gf_render_max_views(void) { return RD_MAX_VIEWS; }
extern "C" int gf_render_max_side(void) { return RD_MAX_SIDE; }
extern "C" int gf_render_max_radius(void) { return RD_MAX_RADIUS; }
extern "C" int gf_render_max_supersample(void) { return RD_MAX_SS; }

extern "C" int gf_render_splat(const float* xyz, const unsigned char* keep, long long N, const float* cams, int V, int Ws,
                               int Hs, int max_radius, long long* keys, void* stream) {
    const int side = RD_MAX_SIDE * RD_MAX_SS;
    GF_CHECK_ARG(N >= 0 && N <= 0x7fffffffLL, "gf_render_splat: N = %lld points (0 to 2^31 - 1)", N);
    GF_CHECK_ARG(V >= 1 && V <= RD_MAX_VIEWS, "gf_render_splat: V = %d views (1 to %d)", V, RD_MAX_VIEWS);
    GF_CHECK_ARG(Ws >= 1 && Ws <= side && Hs >= 1 && Hs <= side, "gf_render_splat: a grid of %d x %d sub-pixels (1 to %d)",
                 Ws, Hs, side);
    GF_CHECK_ARG(max_radius >= 0 && max_radius <= RD_MAX_RADIUS, "gf_render_splat: max_radius = %d (0 to %d)", max_radius,
                 RD_MAX_RADIUS);
    GF_CHECK_ARG(cams && keys, "gf_render_splat: NULL cams or keys");
    if (N == 0) return GF_OK;
    GF_CHECK_ARG(xyz, "gf_render_splat: NULL xyz");
    const dim3 grid(gf_div_up(N, RD_THREADS), V), block(RD_THREADS);
    if (max_radius <= RD_SMALL_RADIUS)
        hipLaunchKernelGGL(k_rd_splat_thread, grid, block, 0, (hipStream_t)stream, xyz, keep, N, cams, Ws, Hs, max_radius,
                           (u64*)keys);
    else
        hipLaunchKernelGGL(k_rd_splat_wave, grid, block, 0, (hipStream_t)stream, xyz, keep, N, cams, Ws, Hs, max_radius,
                           (u64*)keys);
    GF_CHECK_LAUNCH("gf_render_splat");
    return GF_OK;
}

extern "C" int gf_render_resolve(const long long* keys, int V, int W, int H, int S, const unsigned char* rgb,
                                 const int32_t* ids, long long N, const int32_t* h_lut, int stride, float dz,
                                 int background, int outline, unsigned char* image, int32_t* index, void* stream) {
    GF_CHECK_ARG(N >= 0 && N <= 0x7fffffffLL, "gf_render_resolve: N = %lld points (0 to 2^31 - 1)", N);
    GF_CHECK_ARG(V >= 1 && V <= RD_MAX_VIEWS, "gf_render_resolve: V = %d views (1 to %d)", V, RD_MAX_VIEWS);
    GF_CHECK_ARG(W >= 1 && W <= RD_MAX_SIDE && H >= 1 && H <= RD_MAX_SIDE,
                 "gf_render_resolve: an image of %d x %d pixels (1 to %d)", W, H, RD_MAX_SIDE);
    GF_CHECK_ARG(S >= 1 && S <= RD_MAX_SS, "gf_render_resolve: S = %d (1 to %d)", S, RD_MAX_SS);
    GF_CHECK_ARG(stride >= 1 && stride <= RD_MAX_STRIDE, "gf_render_resolve: stride = %d (1 to %d)", stride, RD_MAX_STRIDE);
    GF_CHECK_ARG(background >= 0 && background <= 0xffffff && outline >= 0 && outline <= 0xffffff,
                 "gf_render_resolve: background and outline are 0xRRGGBB");
    GF_CHECK_ARG(keys && image && index && h_lut && (rgb || N == 0),
                 "gf_render_resolve: NULL keys, rgb, h_lut, image or index");
    RdShade sh;
    for (int o = 0; o < 9; ++o) {
        GF_CHECK_ARG(h_lut[o] >= 0 && h_lut[o] <= 256, "gf_render_resolve: lut[%d] = %d (0 to 256)", o, h_lut[o]);
        sh.lut[o] = h_lut[o];
    }
    sh.stride = stride;
    sh.dz = dz;
    sh.background = background;
    sh.outline = outline;
    const dim3 grid(gf_div_up(W, GF_WAVE), gf_div_up(H, RD_THREADS / GF_WAVE), V), block(GF_WAVE, RD_THREADS / GF_WAVE);
    gf_with<int, 1, 2, 3, 4>(S, [&](auto s) {
        hipLaunchKernelGGL(k_rd_resolve<decltype(s)::value>, grid, block, 0, (hipStream_t)stream, (const u64*)keys, W, H,
                           rgb, ids, N, sh, image, index);
    });
    GF_CHECK_LAUNCH("gf_render_resolve");
    return GF_OK;
}
