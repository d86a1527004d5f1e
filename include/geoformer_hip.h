/*
 * geoformer_hip.h -- C ABI of libgeoformer_hip.so, the MI355X (gfx950) native layer under
 * GeoFormer's per-scene forward/backward hot path.
 *
 * Boundary rules
 *   - plain pointers and sizes only (no torch types); every pointer is a DEVICE pointer
 *     unless the parameter name starts with h_;
 *   - every call is asynchronous on the hipStream_t passed as `stream` (void*), allocates
 *     nothing and keeps no global state: the caller owns outputs and scratch;
 *   - return value 0 = ok, negative = gf_status; gf_last_error() gives the message of the
 *     calling thread's last failure.
 *
 * Each entry point names the reference interface it stands in for.  Reference paths are
 * relative to the VinAIResearch/GeoFormer checkout; "spconv" is llijiang/spconv@740a5b7
 * (un-vendored dependency of the reference, docs/INSTALL.md:27-47) and "faiss" the
 * faiss-gpu package (docs/INSTALL.md:69-73).
 */
#ifndef GEOFORMER_HIP_H
#define GEOFORMER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GF_ABI_VERSION 7

typedef enum {
    GF_OK = 0,
    GF_ERR_INVALID_ARG = -1,
    GF_ERR_LAUNCH = -2,
    GF_ERR_UNSUPPORTED = -3,
    GF_ERR_CALLBACK = -4, /* a caller-supplied callback reported a failure (gf_unet_fwd_phased) */
} gf_status;

int gf_abi_version(void);
const char* gf_last_error(void);

/* ===================================================================================
 * Foreground selection of the forward, fused (geoformer.py:423-439): arg-max over the class scores, the
 * foreground test (mode 0: class >= cls, mode 1: class == cls), the ascending index list of the foreground points
 * and the gathered rows of the per-point tensors, all before the one read-back of the count.
 *   scores fp32 [N,C]; locs fp32 [N,3]; batch_idxs int32 [N]; feats fp32 [N,F] or, with feat_rows int32 [N]
 *   (the p2v map), fp32 [M,F] voxel rows read as feats[feat_rows[p]]  (sources, any may be NULL together with its
 *   output);  fg_idxs int64 [N], locs_out [N,3], bidx_out [N], feats_out [N,F],
 *   scores_out [N,C]: capacity N, the first *d_count rows are valid;  scratch: gf_fg_scratch_bytes(N).
 *   h_count (may be NULL): a word of PINNED host memory the count is ALSO stored to, with system scope, by the scan that
 *   finds it -- i.e. before the gathers of the four outputs run, and without a copy command or an event in between: the
 *   caller sets it to a negative value before the call and polls it (gf_host_wait_word); everything it then queues on
 *   `stream` is behind the gathers by stream order.  N = 0 stores 0 to it from the host.
 * =================================================================================== */
size_t gf_fg_scratch_bytes(int N);
int gf_fg_select(const float* scores, int N, int C, int cls, int mode, const float* locs, const int32_t* batch_idxs,
                 const float* feats, const int32_t* feat_rows, int F, void* scratch, long long* fg_idxs, float* locs_out,
                 int32_t* bidx_out, float* feats_out, float* scores_out, int32_t* d_count, int32_t* h_count, void* stream);
/* Host helper: spin (pause instructions, no system call) until *word != pending or timeout_us have passed; returns the
 * word's value (== pending: timed out).  `word`: host memory a device kernel stores to with system scope (h_count above). */
int gf_host_wait_word(const volatile int32_t* word, int pending, long long timeout_us);

/* ===================================================================================
 * Host helper (CPU code, no launch): the reference's per-scene sampling draw
 * np.random.choice(n, k, replace=False) (geoformer.py:575-577) on numpy's legacy MT19937 state, bit for bit.
 *   key uint32[624], *pos: the state as np.random.get_state() returns it (updated in place, hand it back with
 *   set_state);  out int64[k] = permutation(n)[:k].
 * =================================================================================== */
int gf_host_legacy_choice(uint32_t* key, int32_t* pos, long long n, long long k, long long* out);
/* Draw the next `nwords` outputs of the state (key, pos) AHEAD into a per-thread buffer (the caller's state is not
 * touched): a gf_host_legacy_choice that starts from exactly this state reads its words from there -- the draw of the
 * forward's sampling indices (geoformer.py:575-577) then only pays the rejections and the swaps behind the count's
 * read-back.  Too few words drawn ahead: the draw runs on the generator itself.  Same values, same final state. */
int gf_host_legacy_prefetch(const uint32_t* key, int pos, long long nwords);
/* The draw and what geoformer.py:575-579 does with it, from the host's side in ONE call (the device idles between the
 * arrival of the foreground count and the first sampling launch): the same draw as 32-bit indices into the caller's PINNED
 * buffer `pinned` (pinned_cap entries, >= k; with >= n the shuffle runs in place there) and ONE launch that reads them
 * there (device-visible host memory) and writes d_idx32[k], d_idx64[k] (the model's `sampling_indices`) and
 * xyz_dst[k,3] = xyz_src[idx] (n rows).
 * key / pos: the generator's state, advanced in place.  The pinned buffer may be rewritten once the copy has left it
 * (stream order).  fps_m > 0: gf_furthest_point_sampling(xyz_dst, 1, k, fps_m, fps_idx, fps_scratch) is queued behind the
 * gather in the same call (geoformer.py:580-581 / pointnet2_utils.furthest_point_sample on the drawn points). */
int gf_host_draw_sample(uint32_t* key, int32_t* pos, long long n, long long k, int32_t* pinned, long long pinned_cap,
                        int32_t* d_idx32, long long* d_idx64, const float* xyz_src, float* xyz_dst, int fps_m,
                        int32_t* fps_idx, void* fps_scratch, void* stream);

/* ===================================================================================
 * Sparse convolution (stands in for spconv.ops.get_indice_pairs / indice_conv /
 * indice_subm_conv / indice_inverse_conv, reached from geoformer.py:42-53 and
 * geoformer_modules.py:15-35,63-105 through SubMConv3d / SparseConv3d /
 * SparseInverseConv3d).
 *
 * Rulebooks are OUTPUT-STATIONARY neighbour tables: nbr[k*ld + o] = input row feeding
 * output row o through kernel offset k (k = (kx*K+ky)*K+kz), or -1.  The canonical
 * (in,out) pair lists of spconv are the non-negative entries of row k in ascending o.
 * =================================================================================== */

/* Number of 32-bit words in the occupancy bitmap of a [B,X,Y,Z] grid. */
size_t gf_index_words(int B, int X, int Y, int Z);
/* Scratch bytes gf_index_build / gf_rules_down2 need for a bitmap of `words` words. */
size_t gf_index_scratch_bytes(size_t words);

/* Build the occupancy-bitmap rank index of a voxel set.
 *   coords  int32 [M,4] (batch,x,y,z), unique rows          (SparseConvTensor.indices)
 *   bitmap  uint32[words]  out      prefix int32[words] out
 *   perm    int32 [M] out: rank (ascending linear index) -> row
 *   d_M     optional device int32 overriding M (M is then a capacity) */
int gf_index_build(const int32_t* coords, int M, const int32_t* d_M, int B, int X, int Y, int Z, uint32_t* bitmap,
                   int32_t* prefix, int32_t* perm, void* scratch, void* stream);

/* Submanifold 3x3x3 (padding 1) neighbour table from an index.
 *   perm may be NULL when rows are already in ascending linear order (levels >= 2).
 *   nbr    int32 [27*ld] out, ld >= M rounded up to 16 (may be NULL when only `steps` is wanted)
 *   gmask  uint32[ceil(M/16)] out: OR of the offsets present in each 16-row group
 *   steps  optional int32 [gf_rules_steps_words(ld)] out: the same relation as a STEP TABLE -- per 16-row group g only
 *          the present offsets, ascending, four steps per 16-byte entry:
 *              steps[((g*7 + s/4)*16 + row)*4 + s%4] = input row of (row, s-th present offset of g) or -1;
 *          the first three blocks of every group are always written (-1 padded).  gf_conv_fwd's counted-loop
 *          kernel reads this instead of nbr. */
size_t gf_rules_steps_words(int ld);
int gf_rules_subm3(const int32_t* coords, int M, const int32_t* d_M, int X, int Y, int Z, const uint32_t* bitmap,
                   const int32_t* prefix, const int32_t* perm, int32_t* nbr, int ld, uint32_t* gmask, int32_t* steps,
                   void* stream);

/* Strided 2x2x2 / stride 2 rulebook: builds the OUTPUT level's index and tables.
 *   in shape (X,Y,Z) -> out shape (X/2,Y/2,Z/2) (floor; inputs mapping outside are dropped)
 *   bitmap_out/prefix_out: index of the output voxel set (rows in ascending linear order)
 *   out_coords int32 [cap,4] out      d_M_out device int32 out (number of output voxels)
 *   child  int32 [8*ld] out: child[k*ld + o] = input row under offset k, or -1
 *   parent int32 [M] out (output row or -1)      koff int32 [M] out (kernel offset 0..7)
 *   up     int32 [8*ld_up] out: one-hot table of the inverse conv (up[k*ld_up+i] = parent[i] iff k==koff[i])
 *   gmask_down uint32[ceil(cap/16)], gmask_up uint32[ceil(M/16)] out */
int gf_rules_down2(const int32_t* coords, int M, const int32_t* d_M, int B, int X, int Y, int Z,
                   uint32_t* bitmap_out, int32_t* prefix_out, void* scratch, int32_t* out_coords,
                   int32_t* d_M_out, int32_t* child, int ld, int32_t* parent, int32_t* koff, int32_t* up, int ld_up,
                   uint32_t* gmask_down, uint32_t* gmask_up, void* stream);

/* The chain of `nlevels` successive down-sampling rulebooks (the six SparseConv3d(k=2,s=2) of the U-Net,
 * geoformer_modules.py:83-96) in one call and one workspace; the tail of small levels runs in a single launch.
 *   plan (host only): offsets[l*10 + f] = int32-element offset into the workspace of field f of level l, f in
 *     (bitmap, prefix, scratch, out_coords[cap_{l+1},4], child[8,cap_{l+1}], parent[cap_l], koff[cap_l],
 *      up[8,cap_l], gmask_down[cap_{l+1}/16], gmask_up[cap_l/16]);  caps[l] = capacity (leading dimension) of
 *     level l (caps[0] = M0 rounded up to 16), shapes[3*l..] = grid of level l; *ws_elems = workspace size in
 *     int32 elements; *nlevels_out = levels actually built (stops when a grid side drops below 2).
 *   chain: counts[l+1] (device) = number of voxels of level l+1; tables as gf_rules_down2 writes them. */
int gf_rules_down2_chain_plan(int M0, int B, int X, int Y, int Z, int nlevels, long long* offsets, int* caps, int* shapes,
                              long long* ws_elems, int* nlevels_out);
int gf_rules_down2_chain(const int32_t* coords, int M0, int B, int X, int Y, int Z, int nlevels, int32_t* ws,
                         int32_t* counts, void* stream);

/* Weight pre-packing: spconv's parameter layout [k,k,k,Cin,Cout] (= [K,Cin,Cout], kept as the
 * state-dict layout, checkpoint.py:47-49) -> the per-lane MFMA B-operand order the conv kernel
 * streams with one 16-byte load per lane.  Wp holds gf_conv_packed_floats(K,Cin,Cout) floats
 * (channels zero-padded to multiples of 16). */
size_t gf_conv_packed_floats(int K, int Cin, int Cout);
int gf_conv_pack_weights(const float* W, int K, int Cin, int Cout, float* Wp, void* stream);
/* Packed weights of the INPUT GRADIENT's convolution in one launch: the pack of W'[k] = W[flip ? K-1-k : k]^T, a
 * [K,Cout,Cin] operand (gf_conv_packed_floats(K, Cout, Cin) floats); flip = 1 for submanifold tables (gf_conv_wgrad's
 * comment: weights W[K-1-k]^T over the same table), 0 for the child <-> up tables. */
int gf_conv_pack_weights_t(const float* W, int K, int Cin, int Cout, int flip, float* Wp, void* stream);

/* FLAT STEP TABLE of a [K,ld] relation (nbr + gmask as gf_rules_subm3 / gf_rules_down2 write them; the reference's
 * spconv keeps this as its indice pairs, spconv/ops.py get_indice_pairs via geoformer_modules.py:52-129): one 64-byte
 * record of 16 input rows per (16-row group, PRESENT offset), group-major and offset-ascending, behind a header, the
 * per-group step offsets and a bin table: the groups sorted by their number of steps (descending) and dealt to `nbins`
 * bins in snake order, one {group, first step, steps, offset mask} descriptor per (round, bin).  gf_conv_fwd_flat's
 * LDS-weight kernel walks a bin's records linearly.  nbins: 0 = the library's bin count (1024 = one per SIMD), which is
 * also what gf_conv_fwd_flat reads a table with; any other value than that count is an argument error (the signature
 * is kept for the ABI: pass 0).  K <= 31.  flat: int32 [gf_rules_flat_words(K, ld)] out. */
size_t gf_rules_flat_words(int K, int ld);
int gf_rules_flat_steps(const int32_t* nbr, const uint32_t* gmask, int K, int M, int ld, int nbins, int32_t* flat,
                        void* stream);

/* Forward gather-GEMM (output-stationary): out[o,:] = sum_k act(in[nbr[k][o],:]) @ W[k] (+ residual[o,:])
 *   in fp32 [M_in,Cin]   Wp = packed W (gf_conv_pack_weights)   out fp32 [M_out,Cout]
 *   (M_in bounds the buffer descriptor the gathers go through)
 *   1 <= K <= 32, Cin <= 512 (496 with in_scale / in_shift): wider inputs are rejected
 *   nbr may be NULL with K == 1 (identity map: plain GEMM, the k=1 "i_branch" conv)
 *   in_scale/in_shift  optional fp32 [Cin]: act(x) = max(x*scale + shift, 0) fused on the
 *                      gathered rows (eval-mode BatchNorm1d + ReLU, geoformer_modules.py:19-26)
 *   residual           optional fp32 [M_out,Cout] added in the epilogue (geoformer_modules.py:33).  It may be `out`
 *                      itself (in-place accumulation; the training executor's input gradients rely on it): in every
 *                      launch shape each output element's residual is read by the lanes that write that element,
 *                      before they write it.  `in` must not overlap `out`.
 *   out_scale/out_shift optional fp32 [Cout], 16-byte aligned: out = max(out*scale + shift, 0) in the epilogue (the
 *                      CONSUMER's BatchNorm + ReLU applied once per output element; gf_resblock_fwd uses it for bn1)
 *   steps              optional step table of the same relation (gf_rules_subm3); nbr may then be NULL for the
 *                      launch shapes that read it (16 output channels, Cin 16 or 32, level-1 sized inputs)
 */
int gf_conv_fwd(const float* in, const float* Wp, const int32_t* nbr, const uint32_t* gmask, const int32_t* steps, int K,
                int M_in, int M_out, int ld, int Cin, int Cout, const float* in_scale, const float* in_shift,
                const float* residual, const float* out_scale, const float* out_shift, float* out, void* stream);

/* gf_conv_fwd with two outputs: out = the raw sums (+ residual), out_act = max(out*out_scale + out_shift, 0).  A
 * pre-activation residual block (geoformer_modules.py:10-35) reads its input twice -- raw as the residual operand,
 * through BatchNorm + ReLU as the first convolution's input -- so the producer writes both and the consumer's
 * convolution gathers activated rows (one activation per element instead of one per gathered element).  Implemented for
 * the level-1 launch shape (16 output channels over a step table); gf_conv_dual_supported() tells beforehand. */
int gf_conv_dual_supported(int M_out, int ld, int Cin, int Cout, int has_steps);
int gf_conv_fwd_dual(const float* in, const float* Wp, const int32_t* nbr, const uint32_t* gmask, const int32_t* steps,
                     int K, int M_in, int M_out, int ld, int Cin, int Cout, const float* in_scale, const float* in_shift,
                     const float* residual, const float* out_scale, const float* out_shift, float* out, float* out_act,
                     void* stream);

/* gf_conv_fwd with the relation's flat step table (gf_rules_flat_steps; NULL = none) and an optional second output
 * (out_act as gf_conv_fwd_dual; NULL = one output).  With a table, the shapes whose packed weights fit the LDS
 * (K = 27, 16 / 32 output channels, 16-channel multiples in) run the LDS-weight kernel, which also has both outputs;
 * every other shape is gf_conv_fwd / gf_conv_fwd_dual (same results to fp32 summation order). */
int gf_conv_fwd_flat(const float* in, const float* Wp, const int32_t* nbr, const uint32_t* gmask, const int32_t* steps,
                     const int32_t* flat, int K, int M_in, int M_out, int ld, int Cin, int Cout, const float* in_scale,
                     const float* in_shift, const float* residual, const float* out_scale, const float* out_shift,
                     float* out, float* out_act, void* stream);

/* Pre-activation residual block (ResidualBlock, model/geoformer/geoformer_modules.py:10-35) in eval mode, one
 * call:  out = conv1(relu(bn1(conv0(relu(bn0(x)))))) + (Wpi ? x . Wi : x).
 *   x fp32 [M,Cin]; Wp0 (K,Cin,Cout), Wp1 (K,Cout,Cout), Wpi (1,Cin,Cout) or NULL: gf_conv_pack_weights output;
 *   nbr/gmask/K/ld: the level's submanifold table; s0,t0 [Cin], s1,t1 [Cout]: folded BatchNorm (scale, shift);
 *   tmp, idn (NULL iff Wpi NULL), out fp32 [M,Cout]. */
int gf_resblock_fwd(const float* x, const float* Wp0, const float* Wp1, const float* Wpi, const int32_t* nbr,
                    const uint32_t* gmask, const int32_t* steps, int K, int M, int ld, int Cin, int Cout, const float* s0, const float* t0,
                    const float* s1, const float* t1, float* tmp, float* idn, float* out, void* stream);

/* Weight gradient of the same operator: dW[k] = sum_o in[nbr[k][o],:]^T dOut[o,:]  (dW fp32
 * [K,Cin,Cout], zeroed by the call).  The input gradient needs no entry point of its own: it is
 * gf_conv_fwd over the transposed table with per-offset transposed weights
 * (submanifold: same table, weights W[K-1-k]^T; strided/inverse: child <-> up tables). */
int gf_conv_wgrad(const float* in, const float* dout, const int32_t* nbr, int K, int M_out, int ld, int Cin, int Cout,
                  float* dW, void* stream);
/* The same with the table's group masks (gmask as gf_conv_fwd takes it, K <= 32): (group, offset) pairs without a
 * single neighbour are skipped -- 61 % of them on a scanned room's level 1.  gmask or nbr NULL: gf_conv_wgrad. */
int gf_conv_wgrad_masked(const float* in, const float* dout, const int32_t* nbr, const uint32_t* gmask, int K, int M_out,
                         int ld, int Cin, int Cout, float* dW, void* stream);
/* dW += ... : the same without the zero fill (a caller that clears all of a step's weight gradients at once). */
int gf_conv_wgrad_masked_acc(const float* in, const float* dout, const int32_t* nbr, const uint32_t* gmask, int K,
                             int M_out, int ld, int Cin, int Cout, float* dW, void* stream);

/* The sparse U-Net in TRAINING mode (batch statistics, saved activations, backward) as a layer program run from native
 * code: GeoFormer.input_conv -> UBlock x7 -> output_layer with requires_grad (model/geoformer/geoformer.py:39-53,
 * 398-401; ResidualBlock / UBlock: model/geoformer/geoformer_modules.py:10-35,52-129; the training loop's backward:
 * train.py:63-75).  The host compiles the module tree ONCE into a list of ops over numbered feature buffers; a call
 * runs a contiguous range of ops (the two voxel transformers of the deepest levels stay framework modules, so a step
 * is three ranges) with exactly the launches the per-module route makes through gf_conv_fwd, gf_conv_pack_weights(_t),
 * gf_conv_wgrad_masked and gf_bn_relu_train_fwd / _bwd -- without ~1 500 framework calls and ~230 autograd nodes per
 * step.
 *   op kinds     0  dst = relu(batchnorm(src))      batch statistics; running statistics updated; mean / invstd saved
 *                1  dst = conv(src) (+ aux)         table 0: 1x1x1 (plain rows), 1: submanifold 3x3x3 of `level`,
 *                                                   2: 2x2x2 stride 2 from `level` to level+1, 3: its inverse
 *                2  dst = [src | aux]               the skip concatenation (UBlock.forward, geoformer_modules.py:116)
 *   buffers      act[i] / grad[i]: fp32 [rows(level of i), C of i], 16-byte aligned, caller-owned for the whole step
 *   backward     ops in reverse; an op ACCUMULATES into a source's gradient when ghas[src] != 0 and sets ghas[src];
 *                a residual operand's gradient is the output's gradient itself: grad[aux] is re-pointed at grad[dst]
 *                (copied when ghas[dst] == 2: a gradient tensor the caller does not own).  Parameter gradients land
 *                in pgrad at the op's pgrad_off: dW [K,Cin,Cout], or dgamma [C] followed by dbeta [C]. */
typedef struct GfTrainOp {
    int kind, level, table, src, dst, aux, Cin, Cout, no_dgrad, pad_;
    const float* w;                                 /* convolution weights [K,Cin,Cout] */
    const float *gamma, *beta;                      /* BatchNorm */
    float *running_mean, *running_var;
    float eps, momentum;
    long long wp_off;                               /* packed forward weights: floats into `wp` */
    long long pgrad_off;                            /* floats into `pgrad` */
    long long stats_off;                            /* save_mean [C] then save_invstd [C]: floats into `stats` */
} GfTrainOp;
typedef struct GfTrainLevel {
    int M, ld;                                      /* voxels of the level; leading dimension of its 27-offset table */
    const int32_t* nbr; const uint32_t* gmask; const int32_t* steps;
    int M_coarse, ld_down;                          /* the level below: rows, leading dimension of child */
    const int32_t* child; const uint32_t* gmask_down;
    int ld_up, pad_; const int32_t* up; const uint32_t* gmask_up;
    const int32_t* flat;                            /* flat step table of the 27-offset relation (gf_rules_flat_steps) or NULL */
} GfTrainLevel;
/* floats of `scratch` a range of ops needs (BatchNorm partials + the transposed weight pack of the widest op) */
size_t gf_unet_train_scratch_floats(const GfTrainOp* ops, int nops, const GfTrainLevel* levels);
int gf_unet_train_fwd(const GfTrainOp* ops, int op_begin, int op_end, const GfTrainLevel* levels, float* const* act,
                      float* wp, float* stats, float* scratch, void* stream);
int gf_unet_train_bwd(const GfTrainOp* ops, int op_begin, int op_end, const GfTrainLevel* levels, float* const* act,
                      float** grad, unsigned char* ghas, const float* stats, float* pgrad, float* scratch, void* stream);

/* The whole sparse U-Net of the eval forward in one call: input conv -> UBlock x nlevels -> output BatchNorm + ReLU
 * (GeoFormer.input_conv / unet / output_layer, model/geoformer/geoformer.py:42-53,398-401; UBlock and ResidualBlock,
 * model/geoformer/geoformer_modules.py:10-35,52-129; two blocks per level before and after the inner level, all
 * BatchNorm in eval mode).  Issues exactly the launches the per-module route makes through gf_index_build,
 * gf_rules_subm3, gf_rules_down2_chain, gf_conv_fwd, gf_resblock_fwd and gf_backbone_transformer, from native code
 * and out of one workspace; the rulebook chain runs on `side_stream` beside the level-1 convolutions and the call
 * waits once on the host for the chain's voxel counts.
 *   All pointers inside the parameter structs are DEVICE pointers except tr_params (host array of device pointers,
 *   the table gf_backbone_transformer takes); packed weights come from gf_conv_pack_weights; (s, t) pairs are
 *   eval-mode BatchNorm folded to y = max(x*s + t, 0) and must be 16-byte aligned. */
#define GF_UNET_MAX_LEVELS 8
typedef struct GfResBlockParams {
    const float *wp0, *wp1, *wpi;   /* conv_branch.2 / conv_branch.5 / i_branch.0 weights; wpi NULL iff Cin == Cout */
    const float *s0, *t0, *s1, *t1; /* conv_branch.0 [Cin] and conv_branch.3 [Cout] */
} GfResBlockParams;
typedef struct GfUnetLevelParams {
    int C;                          /* channel width of the level (multiple of 16) */
    int tr_layers;                  /* > 0: the level ends with the voxel transformer of that many layers */
    GfResBlockParams blocks[2];     /* UBlock.blocks: C -> C */
    GfResBlockParams tail[2];       /* UBlock.blocks_tail: 2C -> C, C -> C (unused on the deepest level) */
    const float *down_wp, *down_s, *down_t; /* UBlock.conv: BN(C) + ReLU + SparseConv3d(C, C_next, k=2, s=2) */
    const float *up_wp, *up_s, *up_t;       /* UBlock.deconv: BN(C_next) + ReLU + SparseInverseConv3d(C_next, C, k=2) */
    const float* const* tr_params;  /* see gf_backbone_transformer */
} GfUnetLevelParams;
typedef struct GfUnetParams {
    int nlevels;                    /* 7 in GeoFormer */
    int cin;                        /* channels of the voxel features handed in (<= 16) */
    const float* input_wp;          /* packed [27,16,16] input-conv weights, input channels zero-padded to 16 */
    const float *out_s, *out_t;     /* output_layer BatchNorm folded, [16] */
    GfUnetLevelParams level[GF_UNET_MAX_LEVELS];
} GfUnetParams;
/* bytes of workspace gf_unet_fwd needs for a scene of M0 voxels on a [B,X,Y,Z] grid (capacity bound, host only) */
size_t gf_unet_ws_bytes(const GfUnetParams* P, int M0, int B, int X, int Y, int Z);
/*   feats fp32 [M0,cin] voxel features, coords int32 [M0,4] (b,x,y,z) unique rows, ws 256-byte aligned device
 *   workspace, host_counts PINNED host int32 [nlevels]: receives the voxel count of every level,
 *   out fp32 [M0,16]; side_stream may be NULL (everything on `stream`).  Everything queued on side_stream is
 *   joined into `stream` before the call returns control of the tables to later launches. */
int gf_unet_fwd(const GfUnetParams* P, const float* feats, const int32_t* coords, int M0, int B, int X, int Y, int Z,
                void* ws, size_t ws_bytes, int32_t* host_counts, float* out, void* stream, void* side_stream);
/* The same in two phases, for the staggered serving loop (geoformer_amd/serving.py):
 *   phase A = level-1 index and table, the first level's convolutions (input conv + two residual blocks) and the
 *             down-sampling rulebook chain, all queued without a host wait; the CONVOLUTIONS wait for the n_gate recorded
 *             events (hipEvent_t handles), the integer work does not;
 *   `between(user, events_out, max_events)` is then called on the host (may be NULL): it may queue any other work on
 *             other streams and returns the number of recorded events it stored in events_out (<= max_events = 8), or a
 *             negative number to abort the call (GF_ERR_CALLBACK);
 *   phase B = everything below the first level and the whole up pass, behind those events.
 * The loop uses `between` to issue the PREVIOUS scene's sampling / BFS stretch (whose events phase B then waits for):
 * this scene's phase A runs under that scene's foreground read-back and first sampling picks, when the chip is idle. */
typedef int (*GfUnetBetween)(void* user, void** events_out, int max_events);
int gf_unet_fwd_phased(const GfUnetParams* P, const float* feats, const int32_t* coords, int M0, int B, int X, int Y, int Z,
                       void* ws, size_t ws_bytes, int32_t* host_counts, float* out, void* stream, void* side_stream,
                       void* const* gate_events, int n_gate, GfUnetBetween between, void* user);

/* The same with the rulebooks AHEAD of `stream`: index, tables and the down-sampling chain read the voxel coordinates and
 * nothing else.  input_events: the n_input (>= 0) recorded hipEvent_t the COORDINATES wait for (none: they have been
 * resident all along); every rulebook launch goes to side_stream behind those events and behind the end of this host
 * thread's previous gf_unet_fwd* call (which read the same workspace) -- not behind what `stream` still has queued.  In a
 * loop of forwards they then run under the previous scene's sampling / BFS stretch (test.py:52-96 calls the model scene
 * after scene).  `feats` is read on side_stream as well (the zero-padded input rows are made there): it waits for the same
 * events, or was produced on side_stream itself.  Same launches and results; side_stream NULL: gf_unet_fwd. */
int gf_unet_fwd_ahead(const GfUnetParams* P, const float* feats, const int32_t* coords, int M0, int B, int X, int Y, int Z,
                      void* ws, size_t ws_bytes, int32_t* host_counts, float* out, void* stream, void* side_stream,
                      void* const* input_events, int n_input);

/* ===================================================================================
 * Training criterion: Hungarian matching on the device (model/matcher.py:79-126 moves the cost matrix to the host
 * and calls scipy.optimize.linear_sum_assignment per scene)
 * =================================================================================== */

/* Linear sum assignment of queries to ground-truth instances, minimising the total cost.
 *   cost fp32 [nq, K] row-major (device); present int32 [K]: instances that take part (ascending order = the column
 *   order scipy sees); out: match_q int32 [K] = query assigned to instance k (-1: absent or left over),
 *   match_of_q int32 [nq] = instance of query q (-1: none), n_match int32 [1] = min(nq, number present),
 *   status int32 [1]: 0 ok, 1 problem larger than the kernel's tables (512 x 1024), 2 infeasible (non-finite costs).
 * Same solver as scipy (shortest augmenting paths in float64, same scan order and tie-breaking, transposed when there
 * are fewer instances than queries), so the assignment equals scipy's on the same fp32 matrix. */
int gf_lsap(const float* cost, int nq, int K, const int32_t* present, int32_t* match_q, int32_t* match_of_q,
            int32_t* n_match, int32_t* status, void* stream);

/* Dice and focal loss of one scene's matched (query, instance) pairs for one decoder layer
 * (compute_dice_loss / compute_sigmoid_focal_loss on the matched rows, /root/reference/criterion.py:26-58,137-190), and
 * their gradient.  mask_logits fp32 [nq,n]; inst_masks fp32 0/1 [K,n]; match_q [K] / match_of_q [nq] / n_match [1] as
 * gf_lsap wrote them.  fwd: sums fp32, gf_pair_losses_sums_floats(K) floats (first [K,4] row sums: p t, p, t, focal
 * term -- kept for the backward --, then the partial sums of the row segments),
 * out[0] = sum_k dice_k / (n_match + 1e-6), out[1] = sum_k mean_j focal_kj / (n_match + 1e-6).
 * bwd: grad_out fp32 [2] (d loss / d out), d_logits fp32 [nq,n] written in full (zero rows for unmatched queries). */
size_t gf_pair_losses_sums_floats(int K);
int gf_pair_losses_fwd(const float* mask_logits, const float* inst_masks, const int32_t* match_q, int nq, int K, int n,
                       const int32_t* n_match, float* sums, float* out, void* stream);
int gf_pair_losses_bwd(const float* mask_logits, const float* inst_masks, const int32_t* match_of_q, const float* sums,
                       int nq, int K, int n, const int32_t* n_match, const float* grad_out, float* d_logits, void* stream);

/* Training-mode BatchNorm1d (+ ReLU) over voxel rows x[M,C], forward and backward: the pre-activation pair in front of
 * every sparse convolution of the U-Net (geoformer_modules.py:10-35,52-129; BatchNorm1d(eps 1e-4, momentum 0.1),
 * geoformer.py:39), three launches per direction (csrc/bn_train.hip).  C a multiple of 4, M >= 2, pointers 16-byte aligned.
 *   fwd: y = relu((x - mean) * invstd * gamma + beta) with the batch's biased variance; running_mean / running_var
 *        (optional, both or none) updated in place with `momentum` (unbiased variance), save_mean / save_invstd [C]
 *        written for the backward.
 *   bwd: dx (optional) [M,C], dgamma / dbeta (optional) [C] from x, y (the forward's output: ReLU mask), dy.
 * scratch: gf_bn_train_scratch_floats(M, C) floats. */
size_t gf_bn_train_scratch_floats(int M, int C);
int gf_bn_relu_train_fwd(const float* x, int M, int C, const float* gamma, const float* beta, float eps, float momentum,
                         int relu, float* running_mean, float* running_var, float* y, float* save_mean,
                         float* save_invstd, float* scratch, void* stream);
int gf_bn_relu_train_bwd(const float* x, const float* y, const float* dy, int M, int C, const float* gamma,
                         const float* save_mean, const float* save_invstd, int relu, float* dx, float* dgamma,
                         float* dbeta, float* scratch, void* stream);
/* gf_bn_relu_train_bwd with dx = (the layer's input gradient) + addend[M,C] (the gradient the input already received
 * through another consumer, e.g. a residual block's identity branch); addend may be NULL or dx itself. */
int gf_bn_relu_train_bwd_add(const float* x, const float* y, const float* dy, int M, int C, const float* gamma,
                             const float* save_mean, const float* save_invstd, int relu, const float* addend, float* dx,
                             float* dgamma, float* dbeta, float* scratch, void* stream);

/* The same pair for the channel-major layouts x[B,C,L]: nn.BatchNorm1d over [B,C,L] (semantic head, mask tower:
 * geoformer.py:55-70, B = 1, L = number of points) and nn.BatchNorm2d over [B,C,H,W] with L = H*W (the set-abstraction
 * MLP, lib/pointnet2/pytorch_utils.py:9-32).  No alignment requirement on L.  scratch: gf_bn_train_cl_scratch_floats. */
size_t gf_bn_train_cl_scratch_floats(int B, int C, long long L);
int gf_bn_relu_train_cl_fwd(const float* x, int B, int C, long long L, const float* gamma, const float* beta, float eps,
                            float momentum, int relu, float* running_mean, float* running_var, float* y,
                            float* save_mean, float* save_invstd, float* scratch, void* stream);
int gf_bn_relu_train_cl_bwd(const float* x, const float* y, const float* dy, int B, int C, long long L,
                            const float* gamma, const float* save_mean, const float* save_invstd, int relu, float* dx,
                            float* dgamma, float* dbeta, float* scratch, void* stream);

/* ===================================================================================
 * PG_OP (lib/pointgroup_ops/src/pointgroup_ops_api.cpp:6-23)
 * =================================================================================== */

/* voxelize_idx on the GPU (reference: PG_OP.voxelize_idx, lib/pointgroup_ops/src/voxelize/voxelize.cpp:10-152, CPU):
 * voxel ids in order of first occurrence, input_map[N] point -> voxel, rule rows [count, point ids ascending, 0 pad]
 * (modes 3/4) or [1, front()/back()] (modes 0,1 / 2), output coords = coords of rule[1].
 *   coords int64 [N,ncol] on the device (ncol 4 = (b,x,y,z) or 3), every field in [0, 65535];
 *   _count: fills input_map int32 [N] and d_M_maxActive int32[3] = {M, maxActive, error flag} (device);
 *   _fill (after the caller read M and maxActive): output_coords int64 [M,ncol], output_map int32 [M,1+maxActive];
 *   the same scratch (gf_voxelize_idx_scratch_bytes(N)) must be handed to both calls. */
size_t gf_voxelize_idx_scratch_bytes(int N);
int gf_voxelize_idx_count(const long long* coords, int N, int ncol, int mode, void* scratch, int32_t* input_map,
                          int32_t* d_M_maxActive, void* stream);
int gf_voxelize_idx_fill(const long long* coords, int N, int ncol, int mode, void* scratch, const int32_t* input_map,
                         int M, int maxActive, long long* out_coords, int32_t* out_map, void* stream);

/* The host side of feeding a scene (what the reference's drivers do with blocking `.cuda()` calls from their own thread,
 * test.py:56 / train.py:63-75, after a host voxelize_idx in the dataset's collate, datasets/scannetv2_inst.py:389-455) on
 * a NATIVE worker thread: per job, n_copies x (memcpy src -> pinned, hipMemcpyAsync pinned -> dev on `stream`), an event
 * ("copied": the pinned buffers may be rewritten), then -- coords_dev != NULL -- gf_voxelize_idx_count on the uploaded
 * coordinates, the read-back of its three words into head_host (pinned) and a second event ("head").  gf_feeder_submit
 * returns at once; the caller's thread never touches the bytes.  slot 0..3 names the job's state and events; a slot takes
 * a new job after gf_feeder_wait_issued(slot).  Waits release the interpreter lock when called through ctypes. */
#define GF_FEEDER_MAX_COPIES 16
typedef struct {
    int slot, n_copies;
    const void* src[GF_FEEDER_MAX_COPIES];
    void* pinned[GF_FEEDER_MAX_COPIES];
    void* dev[GF_FEEDER_MAX_COPIES];
    size_t bytes[GF_FEEDER_MAX_COPIES];
    const long long* coords_dev; /* device int64 [N,ncol]: one of the `dev` targets, or NULL (no voxelisation) */
    int N, ncol, mode, pad_;
    void* scratch;               /* gf_voxelize_idx_scratch_bytes(N) */
    int32_t* input_map;          /* device int32 [N] */
    int32_t* head_dev;           /* device int32 [3] */
    int32_t* head_host;          /* pinned int32 [3] */
    void* stream;
} GfFeederJob;
void* gf_feeder_create(int device);
int gf_feeder_submit(void* feeder, const GfFeederJob* job);
int gf_feeder_wait_issued(void* feeder, int slot); /* the job's calls are queued on its stream (or: its error status) */
int gf_feeder_wait_copied(void* feeder, int slot); /* after wait_issued: the uploads have left the pinned buffers */
int gf_feeder_wait_head(void* feeder, int slot);   /* after wait_issued: head_host holds {M, maxActive, error} */
int gf_feeder_destroy(void* feeder);

/* PG_OP.voxelize_fp (voxelize.cu:9-31): out[row,:] = sum_i mult * feats[rules[row,i],:], i in rule
 * order, mult = 1/count when average (mode 4).  rules int32 [M, 1+maxActive].  out fp32 [M,C]. */
int gf_voxelize_fp(const float* feats, const int32_t* rules, int M, int maxActive, int C, int average, float* out,
                   void* stream);
/* PG_OP.voxelize_bp / point_recover_fp (voxelize.cu:34-53): d_feats[rules[row,i],:] += mult*d_out[row,:];
 * d_feats must be zeroed by the caller (pointgroup_ops.py:69). */
int gf_voxelize_bp(const float* d_out, const int32_t* rules, int M, int maxActive, int C, int average, float* d_feats,
                   void* stream);

/* ===================================================================================
 * pointnet2._ext (lib/pointnet2/_ext_src/src/bindings.cpp:8-21)
 * =================================================================================== */

/* gather_points (sampling_gpu.cu:11-33): out[b,c,j] = points[b,c,idx[b,j]] */
int gf_gather_points(const float* points, const int32_t* idx, int b, int c, int n, int m, float* out, void* stream);
/* gather_points_grad (sampling_gpu.cu:37-60): grad_points[b,c,idx[b,j]] += grad_out[b,c,j] (zeroed by caller) */
int gf_gather_points_grad(const float* grad_out, const int32_t* idx, int b, int c, int n, int m, float* grad_points,
                          void* stream);
/* group_points (group_points_gpu.cu:11-42): out[b,c,j,s] = points[b,c,idx[b,j,s]] */
int gf_group_points(const float* points, const int32_t* idx, int b, int c, int n, int npoints, int nsample, float* out,
                    void* stream);
/* group_points_grad (group_points_gpu.cu:46-78) */
int gf_group_points_grad(const float* grad_out, const int32_t* idx, int b, int c, int n, int npoints, int nsample,
                         float* grad_points, void* stream);
/* ball_query (ball_query_gpu.cu:12-57): first nsample indices in ascending order with d2 < radius^2,
 * padded with the first hit; rows without a hit are all zero.  idx int32 [b,m,nsample] (fully written). */
int gf_ball_query(const float* new_xyz, const float* xyz, int b, int n, int m, float radius, int nsample, int32_t* idx,
                  void* stream);
/* furthest_point_sampling (sampling_gpu.cu:72-232) incl. the |p|^2 <= 1e-3 skip, the m > n padding
 * and the launch-geometry tie-break of the reference.  xyz fp32 [b,n,3] -> idxs int32 [b,m].
 * scratch: gf_fps_scratch_bytes(b) bytes (zeroed by the call); gf_fps_error_flag() points at a device int set to 1 when
 * some exchange gave up waiting for a workgroup of its point set (picks then wrong). */
size_t gf_fps_scratch_bytes(int b);
int gf_furthest_point_sampling(const float* xyz, int b, int n, int m, int32_t* idxs, void* scratch, void* stream);
const int32_t* gf_fps_error_flag(void* scratch, int b);
/* Same sequence, continued: idxs[b, 0..m_known) already hold its first m_known picks (an earlier call with a
 * smaller m on the same points); fills idxs[b, m_known..m).  Lets a consumer of the first picks (the geodesic BFS
 * needs 256 of 2048) start while the rest is still being drawn. */
int gf_furthest_point_sampling_resume(const float* xyz, int b, int n, int m, int m_known, int32_t* idxs,
                                      void* scratch, void* stream);

/* ===================================================================================
 * Geodesic stage (model/geoformer/geodesic_utils.py)
 * =================================================================================== */

/* Radius-limited kNN graph (stands in for find_knn, geodesic_utils.py:11-24, on the geodesic path):
 * for every point the k nearest points with sqrt(d2) <= radius, ordered by (d2, index), itself
 * included (normally column 0); missing entries are (inf, -1).
 *   D fp32 [n,k] (sqrt(d2) when sqrt_out, else squared like faiss)   I int32 [n,k]
 *   deg int32 [n] optional: number of valid entries after column 0
 *   scratch: gf_knn_scratch_bytes(n); gf_knn_error_flag() points at a device int set to 1 when some
 *   point had more in-radius neighbours than the kernel's list capacity (rows then truncated). */
size_t gf_knn_scratch_bytes(int n);
int gf_knn_radius(const float* xyz, int n, int k, float radius, int sqrt_out, float* D, int32_t* I, int32_t* deg,
                  void* scratch, void* stream);
const int32_t* gf_knn_error_flag(void* scratch, int n);

/* Hop-synchronous geodesic BFS (cal_geodesic_vectorize, geodesic_utils.py:91-164) for nq sources of
 * one scene.  D/I are kNN rows INCLUDING column 0 (which is skipped, :110-111), D already sqrt'ed.
 *   geo fp32 [nq,n] out (-1 = not reached within max_step hops)
 *   keys_ws: nq*n uint64, queue_ws: nq * gf_geodesic_bfs_queue_words(n) int32 (scratch).
 *   D/I rows must be sorted by distance with (inf,-1) padding (the order gf_knn_radius and faiss emit). */
size_t gf_geodesic_bfs_queue_words(int n);
int gf_geodesic_bfs(const float* D, const int32_t* I, const int32_t* deg, int n, int K, const int32_t* src, int nq,
                    float radius, int max_step, float* geo, void* keys_ws, void* queue_ws, void* stream);
/* Same, with the workgroup size per query chosen by the caller: wg_threads = 1024 (one query per compute unit,
 * fastest when the launch has the device to itself), 512 or 256 (several queries share a compute unit, so the
 * launch fits beside another resident kernel -- the host runs it next to furthest point sampling).
 * queue_words: int32 words of queue_ws per query as allocated (checked: at least gf_geodesic_bfs_queue_words(n) = 4 n).
 * (ABI 3.) */
int gf_geodesic_bfs_cfg(const float* D, const int32_t* I, const int32_t* deg, int n, int K, const int32_t* src, int nq,
                        float radius, int max_step, float* geo, void* keys_ws, void* queue_ws, size_t queue_words,
                        int wg_threads, void* stream);
/* ===================================================================================
 * Mask head (GeoFormer.mask_heads_forward, model/geoformer/geoformer.py:286-324), fused
 * =================================================================================== */

/* logits[q,p] = W2_q relu(W1_q [rel(q,p) ; feat_p] + b1_q) + b2_q,  rel = qxyz_q - coords_p and, where
 * geo[q,p] < 0, rel += sqrt_max_geo[q] * sign(rel).
 *   feat fp32 [N,C] (C = 16), coords fp32 [N,3], geo fp32 [nq,N] or NULL (then no fix-up),
 *   qxyz fp32 [nq,3], sqrt_max_geo fp32 [nq] (NULL iff geo NULL),
 *   w1 fp32 [nq,C,3+C] (row c = [3 coordinate taps, C feature taps], the layout
 *   parse_dynamic_params produces, geoformer.py:264-284), b1 [nq,C], w2 [nq,C], b2 [nq]
 *   out fp32 [nq,N]. */
int gf_mask_head(const float* feat, const float* coords, const float* geo, const float* qxyz,
                 const float* sqrt_max_geo, const float* w1, const float* b1, const float* w2, const float* b2, int N,
                 int nq, int C, float* out, void* stream);
/* Same, with w1 / b1 / w2 / b2 pointing INTO one parameter matrix of row stride ldp floats (the controller's
 * [nq, 16*19+16+16+1] output, split as geoformer.py:264-284 does: w1 | w2 | b1 | b2), read in place; ldp = 0: dense. */
int gf_mask_head_packed(const float* feat, const float* coords, const float* geo, const float* qxyz,
                        const float* sqrt_max_geo, const float* w1, const float* b1, const float* w2, const float* b2,
                        int ldp, int N, int nq, int C, float* out, void* stream);
/* E episodes over ONE scene in one launch: the few-shot test loop re-queries a cached scene once per (label, run)
 * (test_fs.py:157-174; GeoFormerFS.get_mask_prediction, model/geoformer/geoformer_fs.py:326-355 once per call).
 * Parameters [E*nq, ...] and logits out fp32 [E*nq, N] are episode-major (row e*nq + q); feat / coords are the
 * scene's, geo [nq,N], qxyz [nq,3] and sqrt_max_geo [nq] the scene's queries', shared by every episode.  Row e*nq + q
 * of `out` equals what gf_mask_head_packed writes to row q for episode e's parameters (split_ws = NULL).
 * split_ws: NULL, or gf_mask_head_split_bytes(N) bytes of scratch (8-byte aligned): the 16-channel feature product then
 * runs on the bf16 matrix pipe over the EXACT three-piece bf16 split of both fp32 operands (six of the nine piece products;
 * what is dropped is below 3 * 2^-24 of the result: one fp32 rounding), 1.3x faster; NULL keeps the fp32 MFMA. */
size_t gf_mask_head_split_bytes(int N);
int gf_mask_head_episodes(const float* feat, const float* coords, const float* geo, const float* qxyz,
                          const float* sqrt_max_geo, const float* w1, const float* b1, const float* w2, const float* b2,
                          int ldp, int N, int nq, int E, int C, void* split_ws, float* out, void* stream);

/* Backward of the fused mask head (training): given gout = dL/dlogits fp32 [nq,N], writes the gradient of the packed
 * per-query parameters (w1 | w2 | b1 | b2 columns, row stride ldp >= 337; the w1/b1/w2 pointers point into the packed
 * parameter matrix like for gf_mask_head_packed) into dparams fp32 [nq,ldp] and of the mask features into dfeat fp32
 * [N,16] (zero on entry).  The hidden activations are recomputed, nothing of the forward is kept; no gradient flows
 * into coords / geo / qxyz (geoformer.py:296-310 treats them as data).  scratch: gf_mask_head_bwd_scratch_floats. */
size_t gf_mask_head_bwd_scratch_floats(int N, int nq);
int gf_mask_head_bwd(const float* feat, const float* coords, const float* geo, const float* qxyz,
                     const float* sqrt_max_geo, const float* w1, const float* b1, const float* w2, const float* gout,
                     int ldp, int N, int nq, int C, float* dparams, float* dfeat, float* scratch, void* stream);
/* The same for E episodes over one scene (the decoder layers of a training step, geoformer.py:286-324 once per layer:
 * same features / coordinates / geodesic rows / query positions, E sets of generated parameters): parameters, gout and
 * dparams have E * nq rows, episode-major; dfeat is the sum over all of them; scratch:
 * gf_mask_head_bwd_scratch_floats(N, E * nq). */
int gf_mask_head_bwd_episodes(const float* feat, const float* coords, const float* geo, const float* qxyz,
                              const float* sqrt_max_geo, const float* w1, const float* b1, const float* w2,
                              const float* gout, int ldp, int N, int nq, int E, int C, float* dparams, float* dfeat,
                              float* scratch, void* stream);

/* ===================================================================================
 * Per-point MLP chains of the eval forward, fused: mask_tower (geoformer.py:64-71), semantic head
 * (geoformer.py:54-62): Conv1d(k=1)/Linear + eval BatchNorm1d + ReLU stacks over the rows of x
 * =================================================================================== */

/* out[p,:] = L_n(... L_1(x[p,:])) with L_l(h) = act_l((W_l h) * scale_l + shift_l), act = ReLU where relu[l] != 0.
 * The caller folds bias and eval-mode BatchNorm into (scale, shift).
 *   x fp32 [N, channels[0]], out fp32 [N, channels[n_layers]], n_layers <= 4,
 *   W / scale / shift: HOST arrays of n_layers DEVICE pointers (W_l row-major [channels[l+1], channels[l]]),
 *   channels: HOST int[n_layers+1] (inputs multiples of 16, all widths <= 64; the last output width is free), relu: HOST int[n_layers]. */
int gf_pointwise_mlp(const float* x, int N, int n_layers, const float* const* W, const float* const* scale,
                     const float* const* shift, const int* channels, const int* relu, float* out, void* stream);
/* Same with a row indirection of the input: out[p] = MLP(x[rows[p]]), rows int32 [N] (the semantic head reading the
 * voxel features through p2v_map, geoformer.py:541-547, without materialising the gathered tensor). */
int gf_pointwise_mlp_rows(const float* x, const int32_t* rows, int N, int n_layers, const float* const* W,
                          const float* const* scale, const float* const* shift, const int* channels, const int* relu,
                          float* out, void* stream);

/* Set-abstraction MLP + max-pool, fused (PointnetSAModuleVotes: SharedMLP + max_pool2d over the samples,
 * lib/pointnet2/pointnet2_modules.py:335-349):  out[b,:,i] = max_s L_n(...L_1(grouped[b,:,i,s])), layers as above
 * (Conv2d 1x1 + eval BatchNorm2d + ReLU folded into W / scale / shift).
 *   grouped fp32 [B, channels[0], npoint, nsample] (gf_group_points layout), out fp32 [B, channels[n], npoint];
 *   channels[0] arbitrary <= 64 (e.g. 3 + 16), hidden widths multiples of 16, all <= 64. */
int gf_group_mlp_max(const float* grouped, int B, int npoint, int nsample, int n_layers, const float* const* W,
                     const float* const* scale, const float* const* shift, const int* channels, const int* relu,
                     float* out, void* stream);

/* The whole set-abstraction stage for given sample indices in two launches (PointnetSAModuleVotes.forward with
 * inds, lib/pointnet2/pointnet2_modules.py:305-349; QueryAndGroup, pointnet2_utils.py:326-356):
 *   new_xyz[b,i] = xyz[b, inds[b,i]];  idx = ball_query(radius, nsample, xyz, new_xyz);
 *   input channels of sample s of centre i: (xyz[idx] - new_xyz[i]) (* 1/radius with normalize_xyz) if use_xyz,
 *   then feats[:, idx];  out[b,:,i] = max_s MLP(...)   -- without materialising the grouped tensor.
 *   xyz fp32 [B,n,3], feats fp32 [B,C,n], inds int32 [B,npoint]; outputs new_xyz fp32 [B,npoint,3],
 *   idx int32 [B,npoint,nsample] (the ball-query result), out fp32 [B,channels[n_layers],npoint];
 *   channels[0] must equal C + 3*use_xyz. */
int gf_ball_query_centres(const float* xyz, const int32_t* centre_idx, int b, int n, int m, float radius, int nsample,
                          float* new_xyz, int32_t* idx, void* stream);
/* The same query for ONE point set through a hash grid with cells of `radius` (27 buckets around each centre instead
 * of every point): identical rows, ~8x less work at 2048 centres x 50 000 points.  Centres as indices into xyz
 * (centre_idx, new_xyz then receives their coordinates) or as coordinates (centres fp32 [m,3], new_xyz may be NULL).
 *   scratch: gf_knn_scratch_bytes(n). */
int gf_point_grid_build(const float* xyz, int n, float radius, void* scratch, void* stream);
int gf_ball_query_grid(const float* xyz, int n, const int32_t* centre_idx, const float* centres, int m, float radius,
                       int nsample, void* scratch, int grid_ready, float* new_xyz, int32_t* idx, void* stream);
/* gf_point_grid_build: the grid alone (same points, radius and scratch), e.g. early on another stream; the query is
 * then called with grid_ready = 1 and launches nothing but itself. */
int gf_sa_group_mlp_max(const float* xyz, const float* feats, const int32_t* inds, int B, int n, int C, int npoint,
                        float radius, int nsample, int use_xyz, int normalize_xyz, int n_layers,
                        const float* const* W, const float* const* scale, const float* const* shift,
                        const int* channels, const int* relu, float* new_xyz, int32_t* idx, float* out, void* scratch,
                        int grid_ready, void* stream);
/* scratch: NULL, or gf_knn_scratch_bytes(n) bytes -> grid ball query (B = 1; grid_ready as above) */

/* Soft-max over the middle dimension of x[n0,n1,inner] (training path of the decoder's vector cross-attention,
 * model/transformer_detr.py:449: F.softmax(sim / sqrt(d), dim=1) on [nq,nc,B,d]):
 *   y = softmax_{n1}(scale * x);   gx = scale * y * (gy - sum_{n1} gy * y). */
int gf_softmax_dim1_fwd(const float* x, int n0, int n1, int inner, float scale, float* y, void* stream);
int gf_softmax_dim1_bwd(const float* y, const float* gy, int n0, int n1, int inner, float scale, float* gx,
                        void* stream);

/* ===================================================================================
 * Token-side stages of the decoder between two cross-attentions, fused (inference)
 * (TransformerDecoderLayer.forward_pre_rel, model/transformer_detr.py:425-463; TransformerDecoder.forward,
 *  model/transformer_detr.py:130-166)
 * =================================================================================== */

/* One launch = [post part of layer l] + [pre part of layer l+1]; either half may be absent (NULL table).
 *   post: tgt = relu(out_mlp(attn_out)) + tgt2; tgt += linear2(relu(linear1(norm3(tgt)))); inter_out = norm(tgt)
 *   pre : t2 = norm1(tgt); q = k = t2 + query_pos; tgt += self_attn(q, k, t2); tgt2 = norm2(tgt);
 *         q1_out = attn_mlp[0](tgt2)   (the query half of the next cross-attention's first linear)
 *   attn_out fp32 [B,nq,64] (gf_decoder_cross_attn output), tgt_in fp32 [nq,B,64] (first stage only),
 *   query_pos fp32 [nq,B,64], inter_out fp32 [nq,B,64], q1_out fp32 [B,nq,64],
 *   state: gf_decoder_token_state_bytes(nq,B) bytes, carried unchanged from one stage to the next,
 *   post_params (HOST array of 10 device pointers): out_mlp.W[64,64] .b | norm3.w .b | linear1.W[ff,64] .b |
 *                linear2.W[64,ff] .b | decoder.norm.w .b
 *   pre_params  (10): norm1.w .b | self_attn.in_proj_weight[192,64] in_proj_bias | out_proj.W .b | norm2.w .b |
 *                attn_mlp[0].W[64,64] .b.       d = 64, nhead = 4, ff % 16 == 0, ff <= 256. */
size_t gf_decoder_token_state_bytes(int nq, int B);
int gf_decoder_token_stage(const float* attn_out, const float* tgt_in, const float* query_pos, int nq, int B, int d,
                           int nhead, int ff, const float* const* post_params, const float* const* pre_params,
                           void* state, float* inter_out, float* q1_out, void* stream);

/* Training form of the decoder's token-side stages (what train.py:63-75 runs through TransformerDecoderLayer
 * .forward_pre_rel, model/transformer_detr.py:425-463, with its dropouts): forward with hashed dropout masks and a native
 * backward, 2 + 1 launches forward and 4 + 2 backward per layer instead of ~95 framework launches.  All tensors fp32
 * [B, T, 64] row-major (row = b * T + t); d_model 64, 4 heads.
 *   pre  (x, query_pos) -> (t2n, q1):  t2 = norm1(x); q = k = t2 + query_pos;
 *                                      x1 = x + drop(out_proj(MHA(q, k, t2))); t2n = norm2(x1); q1 = W1 t2n + b1
 *   post (ca, t2n) -> (x3, inter):     x2 = relu(out_mlp(ca)) + drop(t2n);
 *                                      x3 = x2 + drop(linear2(drop(relu(linear1(norm3(x2)))))); inter = norm(x3)
 *   params: HOST arrays of 10 DEVICE pointers in gf_decoder_token_stage's pre / post order.
 *   Dropout: element kept iff the hash of gf_backbone_transformer_train_fwd's comment says so, with
 *     site = 8 * layer + {0 attention weights, 1 attention branch, 2 the normed query added after the cross-attention,
 *     3 hidden layer, 4 feed-forward branch}, row = b * T + t, col = channel (attention weights: 4 * key + head).
 *   save / work: the *_save_bytes / *_work_bytes sizes; grads: *_grad_floats floats, the 10 parameters' gradients back
 *   to back in table order (every value written; post: the last two are this layer's share of decoder.norm's).
 *   Backward inputs that are NULL count as zero (at least one must be given).  Fixed summation orders. */
size_t gf_decoder_pre_train_save_bytes(int T, int B);
size_t gf_decoder_pre_train_work_bytes(int T, int B);
long long gf_decoder_pre_grad_floats(void);
int gf_decoder_pre_train_fwd(const float* x, const float* qpos, int T, int B, const float* const* params, float p,
                             unsigned seed, int layer, void* save, float* t2n, float* q1, void* stream);
int gf_decoder_pre_train_bwd(const float* x, const float* qpos, const float* t2n, const float* d_t2n, const float* d_q1,
                             int T, int B, const float* const* params, float p, unsigned seed, int layer, void* save,
                             void* work, float* dx, float* dqpos, float* grads, void* stream);
size_t gf_decoder_post_train_save_bytes(int T, int B, int ff);
size_t gf_decoder_post_train_work_bytes(int T, int B, int ff);
long long gf_decoder_post_grad_floats(int ff);
int gf_decoder_post_train_fwd(const float* ca, const float* t2n, int T, int B, int ff, const float* const* params,
                              float p, unsigned seed, int layer, void* save, float* x3, float* inter, void* stream);
int gf_decoder_post_train_bwd(const float* ca, const float* x3, const float* d_x3, const float* d_inter, int T, int B,
                              int ff, const float* const* params, float p, unsigned seed, int layer, void* save,
                              void* work, float* d_ca, float* d_t2n, float* grads, void* stream);

/* ===================================================================================
 * Proposal extraction of the eval forward (GeoFormer.generate_proposal,
 * model/geoformer/geoformer.py:193-262), fused
 * =================================================================================== */

/* Per query q over its mask-logit row: member(p) = 1/(1+exp(-logit)) >= logit_thresh,
 *   npoints[q] = #members, mask_score = sum prob / (npoints + 1e-6),
 *   cls_pred[q] = argmax cls_logits[q], cls_score = softmax(cls_logits[q])[cls_pred],
 *   sem_score = sum_{members} sem_prob[p, cls_pred] / (npoints + 1e-6),
 *   scores[q] = mask_score * sqrt(cls_score) * sem_score,
 *   final[q] = cls_pred >= min_class && npoints >= npoint_thresh && mask_score >= score_thresh.
 *   mask_logits fp32 [nq,N], cls_logits fp32 [nq,ncls], sem_prob fp32 [ncls,N] CLASS-MAJOR (soft-max of the
 *   semantic scores of the foreground points, transposed); outputs int32 [nq] / fp32 [nq]. */
int gf_proposal_stats(const float* mask_logits, const float* cls_logits, const float* sem_prob, int nq, int N,
                      int ncls, float logit_thresh, float score_thresh, int npoint_thresh, int min_class,
                      int* cls_pred, int* npoints, float* scores, int* final_mask, void* stream);

/* Few-shot form (GeoFormerFS.generate_proposal, model/geoformer/geoformer_fs.py:205-238): members as above,
 *   mask_score = sum prob / (npoints + 1e-6), scores[q] = mask_score * sqrt(sim[q]),
 *   final[q] = sim[q] >= sim_thresh && npoints >= npoint_thresh && mask_score >= score_thresh.
 *   mask_logits fp32 [nq,N], sim fp32 [nq] (cosine similarity of the query to the support prototype). */
int gf_proposal_stats_fs(const float* mask_logits, const float* sim, int nq, int N, float logit_thresh,
                         float score_thresh, int npoint_thresh, float sim_thresh, int* npoints, float* scores,
                         int* final_mask, void* stream);

/* proposals[i, fg_idxs[p]] = 1 for every member p of query sel[i]; proposals int32 [n_sel,num_points] must be
 * zero-filled by the caller, fg_idxs int64 [N] (row of each foreground point in the scene), sel int32 [n_sel]. */
int gf_proposal_scatter(const float* mask_logits, const int* sel, int n_sel, int N, const long long* fg_idxs,
                        float logit_thresh, int num_points, int* proposals, void* stream);

/* Ingredients of the decoder's relative position embedding for one scene (geoformer.py:619-651):
 *   geo_ctx[q,j] = geo[q, inds[j]]   (geo fp32 [nq,n], inds int32 [nc] = the context points' FPS indices),
 *   max_geo[q]   = max_j geo_ctx[q,j], or the largest such maximum where row q is entirely unreachable (< 0). */
int gf_relpos_prepare(const float* geo, const int32_t* inds, int nq, int n, int nc, float* geo_ctx, float* max_geo,
                      void* stream);

/* The accepted queries of gf_proposal_stats in ascending order with their classes / scores (geoformer.py:236-243),
 * compacted on the device: sel int32 [nq], cls_out int64 [nq], scores_out fp32 [nq] (capacity nq), *d_count = how many.
 * nq == 0: the arrays may be NULL, *d_count = 0. */
int gf_proposal_select(const int32_t* final_, const int32_t* cls_pred, const float* scores, int nq, int32_t* sel,
                       long long* cls_out, float* scores_out, int32_t* d_count, void* stream);

/* inter[i,j] = number of points in both proposal i and proposal j (matrix NMS, util/utils_3d.py:95-141: the
 * einsum over the [n,N] float masks; exact because the masks are 0/1).  masks int32 [n,N] (gf_proposal_scatter
 * output), inter int32 [n,n], scratch: gf_mask_intersections_scratch_bytes(n, N). */
size_t gf_mask_intersections_scratch_bytes(int n, int N);
int gf_mask_intersections(const int32_t* masks, int n, int N, void* scratch, int32_t* inter, void* stream);

/* ===================================================================================
 * Batched post-processing of an eval forward over S scenes (csrc/batch_post.hip): generate_proposal
 * (model/geoformer/geoformer.py:193-262) and matrix NMS (util/utils_3d.py:95-141) once per scene, in a fixed number of
 * launches.  Each call reads a device scene table of int64 rows.
 * =================================================================================== */
/* Every scene table below is an int64 [S, GF_*_FIELDS] array whose row is the struct declared next to the constant:
 * every member one int64 word (a pointer is its address), in column order.  Kernels, host checks and the Python side
 * read a row through the struct's member names only. */
/* Proposal scene table, int64 [S, GF_PROP_SCENE_FIELDS], one GfPropScene per scene. */
#define GF_PROP_SCENE_FIELDS 6
typedef struct {
    long long logits;     /* mask-logit pointer (fp32 [nq, N_b]) */
    long long N;          /* N_b, the scene's foreground points */
    long long fg_off;     /* first column of the scene in sem_prob / first entry in fg_idxs */
    long long pt_off;     /* first point of the scene in the batch */
    long long num_points; /* the scene's points */
    long long pad_;       /* 0 */
} GfPropScene;
/* gf_proposal_stats per (scene, query): the same formula and workgroup shape (bit-identical per query).
 *   cls_logits fp32 [S, nq, ncls], sem_prob fp32 CLASS-MAJOR [ncls, sem_stride] over the batch's foreground points;
 *   outputs int32 / fp32 [S, nq]. */
int gf_proposal_stats_batched(const long long* table, int S, int nq, const float* cls_logits, const float* sem_prob,
                              long long sem_stride, int ncls, float logit_thresh, float score_thresh, int npoint_thresh,
                              int min_class, int* cls_pred, int* npoints, float* scores, int* final_mask, void* stream);
/* gf_proposal_select per scene: row b of sel / cls_out / scores_out ([S, nq]) holds scene b's accepted queries in
 * ascending order, counts int32 [S] how many.  nq == 0: the arrays may be NULL, every count is 0. */
int gf_proposal_select_batched(const int32_t* final_, const int32_t* cls_pred, const float* scores, int S, int nq,
                               int32_t* sel, long long* cls_out, float* scores_out, int32_t* counts, void* stream);
/* gf_proposal_scatter of every scene into ONE zero-filled int32 buffer: scene b's block [counts[b], num_points_b]
 * starts at element sum_{c<b} counts[c] * num_points_c; members go to column fg_idxs[fg_off + p] - pt_off (scene-local).
 * total_rows = sum of counts (<= 65535), max_N = the largest N_b. */
int gf_proposal_scatter_batched(const long long* table, int S, int nq, const int32_t* sel, const int32_t* counts,
                                int total_rows, int max_N, const long long* fg_idxs, float logit_thresh, int* packed,
                                void* stream);

/* NMS scene table, int64 [S, GF_NMS_SCENE_FIELDS], one GfNmsScene per scene. */
#define GF_NMS_SCENE_FIELDS 8
typedef struct {
    long long masks;     /* masks pointer (int32 [n_b, N_b], nonzero = member) */
    long long N, n;      /* N_b, n_b */
    long long bits_off;  /* uint64 words into the bits scratch, n_b * ceil(N_b / 64) of them */
    long long inter_off; /* int32 elements into inter, n_b * n_b of them */
    long long scores;    /* scores pointer (fp32 [n_b]) */
    long long cats;      /* categories pointer (int64 [n_b]) */
    long long pick_off;  /* int32 elements into picks, n_b of them */
} GfNmsScene;
#define GF_NMS_MAX_N 1024
/* gf_mask_intersections per scene: inter + inter_off is scene b's [n_b, n_b] block.  max_waves / max_pairs: the
 * largest n_b * ceil(N_b / 64) / n_b * n_b over the scenes. */
int gf_mask_intersections_batched(const long long* table, int S, long long max_waves, long long max_pairs, void* bits,
                                  int32_t* inter, void* stream);
/* Matrix NMS per scene, one workgroup each (n_b <= GF_NMS_MAX_N), on the intersection blocks of
 * gf_mask_intersections_batched.  Same [n, n] algebra as util/utils_3d.py:95-141 in fp32: proposals sorted by score,
 * descending, EQUAL SCORES BY ASCENDING INDEX; iou = I / (d_i + d_j - I); compensation = max same-class IoU with a
 * higher-ranked proposal; decay = min over rows of exp(-sigma iou^2) / exp(-sigma comp^2) (kernel 0, gaussian) or
 * (1 - iou) / (1 - comp) (kernel 1, linear); kept where score * decay >= final_score_thresh.  picks + pick_off gets
 * the kept proposals' indices in descending-score order, pick_counts int32 [S] how many. */
int gf_matrix_nms_batched(const long long* table, int S, const int32_t* inter, int kernel, float sigma,
                          float final_score_thresh, int32_t* picks, int32_t* pick_counts, void* stream);
/* Greedy NMS per scene (util/utils_3d.py:76-93), one workgroup each (n_b <= GF_NMS_MAX_N), on the same scene table
 * (the categories pointer is not read and may be 0) and intersection blocks.  Proposals in descending score order, EQUAL
 * SCORES BY ASCENDING INDEX; a proposal still alive is picked and suppresses every later proposal j with
 * iou[pick, j] > threshold, iou = I / ((d_pick + d_j) - I) in fp32 (strict comparison; a NaN never suppresses; a
 * suppressed proposal suppresses nothing).  picks + pick_off gets the picked indices in pick order, pick_counts int32
 * [S] how many (0 for a scene with n_b == 0). */
int gf_greedy_nms_batched(const long long* table, int S, const int32_t* inter, float threshold, int32_t* picks,
                          int32_t* pick_counts, void* stream);
/* The same walk over a caller-given row-major fp32 [n, n] matrix (the row is the pick: ious[pick * n + j]; it need not
 * be symmetric), n <= GF_NMS_MAX_N: picks int32 [n], pick_count int32 [1]. */
int gf_greedy_nms_ious(const float* ious, const float* scores, int n, float threshold, int32_t* picks,
                       int32_t* pick_count, void* stream);

/* ===================================================================================
 * Scene labelling from the picked masks of S scenes (csrc/label_map.hip): one label per point and one table row per
 * picked instance, as util/visualize.py:219-227 paints them (from the last pick to the first, score < min_score
 * skipped, a later paint wins): the owner of a point is the LOWEST rank r in pick whose score is >= min_score and whose
 * mask covers the point.  Three launches for any S, n, p; no read-back; no atomics in global memory (bit-identical
 * results from call to call, and for a scene alone or in a batch).
 * Label scene table, int64 [S, GF_LBL_SCENE_FIELDS], one GfLblScene per scene.
 * Scratch: bits, part_f fp32 [records, 9], part_cnt int32 [records], own_part int32 [GF_LBL_OWN_SPLIT * records].
 * Outputs:
 *   owner int32: rank into pick or -1;  ids int32: label_ids[pick[owner]] * 1000 + owner + 1, 0 without an owner;
 *   tab_i int32 [rows, GF_LBL_TABLE_INTS], one GfLblRowI per rank;  tab_f fp32 [rows, GF_LBL_TABLE_FLOATS], one GfLblRowF.
 * max_points / max_picks: the largest N_b / p_b over the scenes. */
#define GF_LBL_SCENE_FIELDS 12
#define GF_LBL_CHUNK 4096
#define GF_LBL_OWN_SPLIT 4
#define GF_LBL_TABLE_INTS 5
#define GF_LBL_TABLE_FLOATS 10
typedef struct {
    long long masks;     /* masks pointer (int32 [n_b, N_b], nonzero = member) */
    long long N, n;      /* N_b, n_b */
    long long p;         /* p_b (<= GF_NMS_MAX_N) */
    long long pick;      /* pick pointer (int64 [p_b], rows of masks; a value outside [0, n_b) is an empty, not-kept row) */
    long long scores;    /* scores pointer (fp32 [n_b]) */
    long long label_ids; /* label_ids pointer (int64 [n_b]) */
    long long xyz;       /* xyz pointer (fp32 [N_b, 3]) */
    long long bits_off;  /* uint64 words into bits, p_b * ceil(N_b / 64) of them */
    long long part_off;  /* records into part_f / part_cnt / own_part, p_b * ceil(N_b / GF_LBL_CHUNK) of them */
    long long row_off;   /* rows into tab_i / tab_f, p_b of them */
    long long pt_off;    /* elements into owner / ids, N_b of them */
} GfLblScene;
typedef struct {
    int count;    /* points of the mask */
    int owned;    /* points with owner == r */
    int label_id;
    int pick;     /* pick[r] */
    int kept;     /* score >= min_score */
} GfLblRowI;
typedef struct {
    float centroid[3], box_min[3], box_max[3]; /* xyz each, over the whole mask; zeros when count == 0 */
    float score;
} GfLblRowF;
int gf_label_map_batched(const long long* table, int S, long long max_points, int max_picks, float min_score,
                         void* bits, float* part_f, int32_t* part_cnt, int32_t* own_part, int32_t* owner, int32_t* ids,
                         int32_t* tab_i, float* tab_f, void* stream);

/* ===================================================================================
 * Overlap tables of the ScanNet instance evaluation for one scene (assign_instances_for_scan, util/eval.py:290-355,
 * with get_instances, util/utils_3d.py:18-73): everything the evaluation derives from the N points.
 *   masks int32 [n_rows,N] (gf_proposal_scatter layout; any nonzero is a member), rows int32 [n] (may be NULL: row i
 *   is mask i, n <= n_rows; otherwise the picked rows in order, an index outside [0,n_rows) selects nothing),
 *   gt_ids int64 [N] in the val_gt encoding nyu40_id * 1000 + inst + 1 (0 = unannotated), class_ids int32 [C] the
 *   evaluated nyu40 ids (distinct, positive; 1 <= C <= 64).  A point is void iff floor(gt_ids / 1000) is not among
 *   class_ids; every other distinct id is an instance, numbered 0..G-1 in ascending id order (np.unique's).
 *   Outputs: *d_G = G; for G <= max_gt: gt_id int64 [max_gt] (first G valid), gt_count int32 [max_gt] (points of each
 *   instance), inter int32 [n, G+1] packed in a buffer of n * (max_gt + 1) words: inter[i, g] = |mask_i AND id_g|,
 *   inter[i, G] = |mask_i AND void| (the row sum is the mask's point count).  G > max_gt: only *d_G is meaningful and
 *   nothing is written past the capacities; the caller grows them and repeats the call.
 *   Exact integer counts (integer atomics), four commands on `stream`, no host synchronisation.
 *   scratch: gf_instance_overlaps_scratch_bytes(N, C).  (ABI 6.) */
size_t gf_instance_overlaps_scratch_bytes(int N, int C);
int gf_instance_overlaps(const int32_t* masks, int n_rows, int N, const int32_t* rows, int n, const long long* gt_ids,
                         const int32_t* class_ids, int C, int max_gt, void* scratch, int32_t* d_G, long long* gt_id,
                         int32_t* gt_count, int32_t* inter, void* stream);

/* ===================================================================================
 * Semantic-segmentation evaluation of a batch of S scenes packed one after the other: per-point prediction and
 * per-scene confusion matrices from the forward's class scores (semantic_scores.max(1)[1], geoformer.py:423, counted
 * as the benchmark's evaluate_semantic_label.py does).
 *   scores fp32 [N,C] contiguous, 1 <= C <= gf_semantic_confusion_max_classes().
 *   preds int32 [N] (may be NULL): the FIRST maximal class of each row -- start from class 0, replace on strict '>' in
 *   ascending class order, exactly gf_fg_select's rule: a NaN wins only in column 0, and `preds >= 4` is the
 *   foreground that call selects, ties and NaNs included.
 *   labels int64 [N], or NULL for prediction only (conf is not touched, offsets / conf may be NULL).
 *   offsets int32 [S+1] (device): ascending scene offsets, offsets[0] = 0, offsets[S] = N; a scene may be empty.
 *   offsets_host: the same table in host memory, or NULL.  Given, it is checked before anything is launched
 *   (offsets[0] != 0, a descending pair or offsets[S] != N is GF_ERR_INVALID_ARG).  Not given, nothing is read back:
 *   the kernel never leaves [0,N) x [0,S) whatever the table holds, a malformed one only loses counts.
 *   Label mapping: m = map_ignore when label == ignore_label; else lut[label] for 0 <= label < L (lut int32 [L],
 *   device), map_other for every other label; lut NULL (L = 0): the identity over 0..C-1, map_other elsewhere.
 *   m outside 0..C-1 means "ignored".
 *   conf int64 [S, C+1, C]: conf[s, m, pred] for the points of scene s, row C for the ignored ones.  The call ADDS to
 *   conf (the caller zeroes it): conf[s].sum() grows by exactly the scene's point count per call.
 * One launch on `stream`, no host synchronisation: a workgroup owns gf_semantic_confusion_run_points() consecutive
 * points, counts them per scene in an LDS table of (C+1)*C words and adds its non-zero bins with 64-bit integer
 * atomics -- exact and independent of order. */
int gf_semantic_confusion_max_classes(void);
int gf_semantic_confusion_run_points(void);
int gf_semantic_confusion(const float* scores, const long long* labels, const int32_t* offsets,
                          const int32_t* offsets_host, int S, int N, int C, const int32_t* lut, int L,
                          long long ignore_label, int map_ignore, int map_other, int32_t* preds, long long* conf,
                          void* stream);

/* ===================================================================================
 * Panoptic labels and the tables of panoptic quality (Kirillov et al., "Panoptic Segmentation", CVPR 2019) of a batch
 * of S scenes packed one after the other: things from the label map (gf_label_map_batched), stuff from the semantic
 * head (gf_semantic_confusion's preds), against the ground truth of gf_instance_overlaps.
 *   Per point: owner int32 (rank into pick, or -1), ids int32 (the label map's ids; may be NULL when pan is NULL),
 *   sem int32 (the semantic class), gt_ids int64 (val_gt encoding nyu40_id * 1000 + inst + 1, 0 = unannotated).
 *   offsets int32 [S+1] (device) and offsets_host (host copy or NULL): as gf_semantic_confusion; given, offsets_host
 *   is checked before anything is launched.  Not given, nothing is read back: no index leaves [0,N) x [0,S).
 *   class_ids int32 [C] the evaluated nyu40 ids (distinct, positive; 1 <= C <= 64), is_stuff int32 [C],
 *   stuff_of_sem int32 [L]: semantic class -> index into class_ids of a stuff class, or -1; n_stuff = the number of
 *   stuff classes; P = the largest pick count of the batch; R = P + n_stuff + 1 <= gf_panoptic_max_rows() rows.
 *   Row of a point: owner when 0 <= owner < P; else P + (rank of class_ids[stuff_of_sem[sem]] among the stuff classes
 *   in class_ids order) when 0 <= sem < L names a stuff class; else R - 1 (unlabelled).  An owner or a semantic class
 *   outside its range is never an address.
 *   Column of a point: q = floor(gt / 1000); q not among class_ids: void; a thing: key rank(q) * 1000 + (gt - q * 1000);
 *   a stuff class: key rank(q) * 1000 (all its instances are ONE segment).  The scene's distinct keys in ascending
 *   order are columns 0..G_s-1, the void column is the LAST one, index max_gt; columns G_s..max_gt-1 stay zero.
 *   Outputs: d_G int32 [S]; gt_id int64 [S, max_gt] (the original id of a thing, nyu40_id * 1000 of a stuff segment;
 *   zero past G_s); inter int32 [S, R, max_gt + 1]: inter[s, r, g] = points of scene s with row r and column g;
 *   pan int32 [N] (may be NULL): ids[i] on a thing row, class_ids[j] * 1000 on a stuff row, 0 where unlabelled.
 *   G_s > max_gt: only d_G[s] is meaningful for that scene (its part of inter is zero) and nothing is written past
 *   the capacities; the other scenes are complete.  The caller grows max_gt and repeats the call.
 *   Four commands on `stream` whatever S, N and P are (presence memset; keys + pan; one slot scan per scene; count),
 *   no host synchronisation; owner, sem and gt_ids are read once.  The count: a workgroup owns
 *   gf_panoptic_run_points() consecutive points, cut at the scene boundaries; a scene whose R * (G_s + 1) bins fit the
 *   LDS table is counted there and flushed as one integer atomic per non-zero bin, a larger one by wave-aggregated
 *   global integer atomics (one per distinct pair per wave).  Exact and independent of the schedule.
 *   gt_ids NULL (pan given): the labels alone, one launch; scratch, d_G, gt_id and inter are not touched (may be NULL).
 *   scratch: gf_panoptic_overlaps_scratch_bytes(S, N, C). */
int gf_panoptic_max_rows(void);
int gf_panoptic_run_points(void);
size_t gf_panoptic_overlaps_scratch_bytes(int S, int N, int C);
int gf_panoptic_overlaps(const int32_t* owner, const int32_t* ids, const int32_t* sem, const long long* gt_ids,
                         const int32_t* offsets, const int32_t* offsets_host, int S, int N, const int32_t* class_ids,
                         const int32_t* is_stuff, int C, const int32_t* stuff_of_sem, int L, int n_stuff, int P,
                         int max_gt, void* scratch, int32_t* pan, int32_t* d_G, long long* gt_id, int32_t* inter,
                         void* stream);

/* ===================================================================================
 * Mask logits pooled over a scene's over-segments (superpoints; ScanNet's *.segs.json, field segIndices) for the S
 * kept scenes of an eval forward (csrc/segment_pool.hip), between the mask head and gf_proposal_stats*:
 *     out[q, p] = mean of in[q, p'] over the foreground points p' of the scene in p's segment
 *   Segment scene table, int64 [S, gf_segment_pool_scene_fields()], one GfSegScene (below) per scene.
 *   table (device) and table_host (the same rows on the host, or NULL): given, table_host is checked before anything
 *   is launched -- out == in (the pooling is out of place), a NULL pointer with N_b > 0, N_b > max_N, rows that do not
 *   follow each other or do not add up to n_fg are GF_ERR_INVALID_ARG.  Not given, nothing is read back and a scene
 *   whose row fails these checks is skipped on the device: no address leaves its buffer.
 *   keys_sorted int64 [n_fg], order int32 [n_fg]: the batch's foreground rows sorted STABLY by one key per row that
 *   orders them by scene first (so scene b keeps the positions fg_off .. fg_off + N_b) and is equal for two rows exactly
 *   when they are pooled together; order[j] = the foreground row at sorted position j.  A row without a segment has a
 *   key of its own.  The run boundaries are found on the device from neighbouring keys.
 *   nq < 1, a negative size, n_fg > 2^31 - 16 or a NULL pointer with n_fg > 0 is GF_ERR_INVALID_ARG; S == 0 or
 *   n_fg == 0 succeeds with nothing launched.  max_N = the largest N_b.
 *   Eight commands on `stream` whatever S, nq and the segments are (run flags; a three-launch scan; run table; pool;
 *   combine; open runs), no host synchronisation.  The logits are read once and written once.  A workgroup owns
 *   gf_segment_pool_chunk_points() consecutive sorted positions of ONE scene, counted from the scene's first, and 16
 *   queries; a segment inside a chunk gets its mean in the launch that read it, a segment cut by chunk boundaries is
 *   summed per chunk, its partial sums are added in chunk order by the chunk it begins in, and the result is written
 *   by a last launch.  No floating-point atomics: every (query, segment) sum is formed once, in fp32, in an order that
 *   depends only on the positions inside the scene, and every member receives that one word divided by the member
 *   count -- bit-identical from call to call and for a scene alone or inside a batch; a segment of one row returns
 *   its logit bit for bit.
 *   scratch: gf_segment_pool_scratch_bytes(S, n_fg, nq). */
typedef struct {
    long long in, out; /* logits in / out pointers (fp32 [nq, N_b]) */
    long long N;       /* N_b, the scene's foreground points */
    long long off;     /* fg_off: the scene's first foreground row in the batch; the rows of the scenes follow each other */
} GfSegScene;
int gf_segment_pool_scene_fields(void); /* = sizeof(GfSegScene) / 8 */
int gf_segment_pool_chunk_points(void);
size_t gf_segment_pool_scratch_bytes(int S, long long n_fg, int nq);
int gf_segment_pool_batched(const long long* table, const long long* table_host, int S, int nq,
                            const long long* keys_sorted, const int32_t* order, long long n_fg, long long max_N,
                            void* scratch, void* stream);

/* ===================================================================================
 * Geometric over-segmentation of one scene (csrc/oversegment.hip; the statement is postprocess.oversegment_host):
 * the over-segment ids gf_segment_pool_batched pools over, from the points alone.  Both functions read kNN rows in
 * gf_knn_radius' format -- I int32 [n,k], deg int32 [n] = valid entries after column 0 -- but accept ANY rows: only
 * columns 0 .. min(deg[i], k - 1) of row i are read, and an entry outside [0, n) is skipped, never followed.
 * n < 0, k < 1, a NULL pointer with n > 0 (and min_points < 1) are GF_ERR_INVALID_ARG before anything is launched;
 * n == 0 succeeds with nothing launched.  Every launch goes on `stream`; no host synchronisation, no read-back.
 *
 * gf_point_normals (stage A, one launch, no scratch): out fp32 [n,4] = (nx, ny, nz, sigma), 16-byte aligned.  The
 *   neighbourhood of point i is the row's entries that count (the row normally lists i itself).  Fewer than 3,
 *   or all of them in one place (the covariance's trace is not positive): (0, 0, 0, -1).  Otherwise the fp32 covariance of
 *   the differences x_j - x_i about their own mean, its eigenvectors by a fixed number of cyclic Jacobi sweeps, the unit
 *   eigenvector of the smallest eigenvalue l0 with its first component of magnitude > 1e-6 made positive, and
 *   sigma = max(l0, 0) / (l0 + l1 + l2).
 *
 * gf_smooth_components (stages B-D, five launches): ids_out int32 [n] from ANY rows and ANY normals4 (fp32 [n,4],
 *   16-byte aligned).  A point is flat when 0 <= sigma <= flatness.  A row entry (i, j), j != i, links two flat points
 *   when |n_i . n_j| >= cos_thresh and |n_i . (x_j - x_i)| <= offset (one direction suffices).  A connected component
 *   of flat points gets its smallest point index as id; one with fewer than min_points points gets -1.  A non-flat
 *   point takes the id of the first entry j of its row that is flat, kept and has |n_j . (x_i - x_j)| <= offset, else
 *   -1.  Union-find over an int32 parent array, the larger root hooked under the smaller by atomicCAS; integer atomics
 *   only.  The ids are a function of the inputs alone: bit-identical from call to call.
 *   scratch: gf_smooth_components_scratch_bytes(n). */
size_t gf_point_normals_scratch_bytes(int n);
int gf_point_normals(const float* xyz, const int32_t* I, const int32_t* deg, int n, int k, float* out, void* stream);
size_t gf_smooth_components_scratch_bytes(int n);
int gf_smooth_components(const float* xyz, const float* normals4, const int32_t* I, const int32_t* deg, int n, int k,
                         float cos_thresh, float offset, float flatness, int min_points, int32_t* ids_out,
                         void* scratch, void* stream);

/* ===================================================================================
 * Picked instance masks split into spatially connected clusters (csrc/mask_split.hip; the statement is
 * postprocess.mask_components_host): DBSCAN of every picked mask over ONE scene's radius graph, each mask restricting
 * the graph to its own points.  masks int32 [n_rows, N] (nonzero = member), pick int64 [p] rows of masks (a value
 * outside [0, n_rows) is an empty row), kNN rows I int32 [N,k] / deg int32 [N] read as gf_smooth_components reads them:
 * columns 0 .. min(deg[i], k - 1) of row i, an entry outside [0, N) skipped and never followed.
 *
 * gf_mask_components (seven launches for any N, p, k): for pick rank r with member set M,
 *   cnt(i) = 1 + the read entries j of row i with j != i and j in M (a repeated entry counts each time); i in M is a
 *   CORE point when cnt(i) >= min_samples.  A read entry (i, j) with both ends core joins them (one direction
 *   suffices); a cluster's id is its smallest core index.  A member that is not core (a BORDER point) takes the smallest
 *   cluster id among the core entries of its own row, -1 without one.  A cluster of fewer than min_points points (core
 *   and border) is dissolved to -1.
 *   comp int32 [p, N]: the cluster id of every member point or -1;  tab int32 [p, GF_MSP_TABLE_INTS]: one GfMspRow
 *   per rank.
 *   Integer atomics only: comp and tab are a function of the inputs, bit-identical from call to call, and a pick's rows
 *   are the same alone or among other picks.  scratch: gf_mask_components_scratch_bytes(N, p), 8-byte aligned.
 * gf_mask_keep_largest (one launch): masks_out int32 [n_rows, N] (not overlapping masks) -- a picked row keeps its
 *   values at the points of its largest kept cluster and is zero elsewhere (all zero without a kept cluster); every
 *   other row is copied.
 * N < 0, p < 0, p > GF_NMS_MAX_N, k < 1, min_samples < 1, min_points < 1, or a NULL pointer with N > 0 and p > 0, are
 * GF_ERR_INVALID_ARG before anything is launched; N == 0 or p == 0 succeeds with nothing launched (masks_out is then
 * not written).  Every launch goes on `stream`; no host synchronisation, no read-back. */
enum { GF_MSP_TABLE_INTS = 5 }; /* columns of tab */
typedef struct {
    int members;
    int clusters;     /* clusters kept */
    int kept_points;  /* points in kept clusters */
    int largest;      /* id of the largest kept cluster (ties: the smaller id) or -1 */
    int largest_size; /* its size */
} GfMspRow;
size_t gf_mask_components_scratch_bytes(int N, int p);
int gf_mask_components(const int32_t* masks, int n_rows, int N, const long long* pick, int p, const int32_t* I,
                       const int32_t* deg, int k, int min_samples, int min_points, int32_t* comp, int32_t* tab,
                       void* scratch, void* stream);
int gf_mask_keep_largest(const int32_t* masks, int n_rows, int N, const long long* pick, int p, const int32_t* comp,
                         const int32_t* tab, int32_t* masks_out, void* stream);

/* ===================================================================================
 * Instances of a scan that was run as T overlapping tiles, joined across the tiles (csrc/tile_merge.hip; the statement
 * is postprocess.merge_tiles_host, the tile plan scene.tile_plan).  The device receives integer tables only:
 *   tile_of, local_of int32 [N, 4], 16-byte aligned: the tiles of each of the scan's N points in ascending order, -1
 *   padded, and the point's index inside each of them.
 *   Tile scene table, int64 [T, GF_TILE_SCENE_FIELDS], one GfTileScene per tile s (an empty tile has n_s = 0).
 *   table (device) and table_host (the same rows on the host): table_host is checked before anything is launched -- a
 *   negative size, p_s over the cap, first row / first word that do not follow the tile before, picks that do not add
 *   up to P, P > gf_tile_merge_max_rows() or T > 65535 are GF_ERR_INVALID_ARG.
 * Rows 0 .. P-1 are the picked masks of all tiles, tile-major, then by rank in pick.
 *
 * gf_tile_pack_picks (one launch): bits uint32 -- per tile-local point j of tile s the ceil(p_s / 32) consecutive words
 *   at first word + j * ceil(p_s / 32): bit k of word w is set when the mask of pick w * 32 + k holds the point.
 * gf_tile_overlaps (two memsets, one launch): inter int32 [P, P] (symmetric) and shared int32 [P, T], zeroed by the
 *   call; only entries across two tiles are written.  For rows a of tile s and b of tile t != s:
 *   inter[a, b] = the points of the scan that lie in both tiles and in both masks; shared[a, t] = the points of mask a
 *   that also lie in tile t.  One thread per point of the scan; a point in one tile costs the read of its tile_of row.
 *   Integer atomics, one per distinct (tile pair, bitset pair) of a wave.
 * gf_tile_merge (one launch of ONE workgroup of 1024 threads): rows a < b are joined when row_tile[a] != row_tile[b],
 *   cls[a] == cls[b], inter[a, b] >= min_shared and (double)inter[a, b] >= iom * (double)min(shared[a, row_tile[b]],
 *   shared[b, row_tile[a]]) (one double multiplication and a compare).  comp int32 [P]: the smallest row of each row's
 *   connected component; members int32 [P]: the component's rank among the representatives (the global id);
 *   d_G int32 [1] = G; inst_cls int64 [P], inst_scores fp32 [P] (first G valid): the representative's class and the
 *   largest member score, the same word copied (integer-ordered maximum; the scores hold no NaN).
 * gf_tile_assemble (two memsets, one launch): masks int32 [G, N] (0 / 1) and count int32 [G], zeroed by the call:
 *   masks[members[r], g] = 1 for every row r and point g of its mask, through the bitsets; count = the points of each
 *   instance (a word is counted by the atomicOr that finds it 0).  A member id outside [0, G) is skipped.
 * Every output is a function of the inputs: bit-identical from call to call.  Every launch goes on `stream`; no host
 * synchronisation, no read-back. */
enum { GF_TILE_SCENE_FIELDS = 7 }; /* int64 words per row of the tile scene table */
typedef struct {
    long long masks;       /* masks pointer (int32 [n_rows, n_s], nonzero = member) */
    long long n_rows, n_s;
    long long pick;        /* pick pointer (int64 [p_s], rows of masks; a value outside [0, n_rows) is an empty row) */
    long long p_s;         /* <= gf_tile_merge_max_picks() */
    long long first_row;   /* the p_s of the tiles before */
    long long first_word;  /* uint32 words into bits: the n * ceil(p / 32) of the tiles before */
} GfTileScene;
int gf_tile_merge_max_rows(void);
int gf_tile_merge_max_picks(void);
int gf_tile_pack_picks(const long long* table, const long long* table_host, int T, int P, uint32_t* bits, void* stream);
int gf_tile_overlaps(const long long* table, const long long* table_host, int T, const int32_t* tile_of,
                     const int32_t* local_of, long long N, const uint32_t* bits, int P, int32_t* inter, int32_t* shared,
                     void* stream);
int gf_tile_merge(const int32_t* inter, const int32_t* shared, const long long* cls, const float* scores,
                  const int32_t* row_tile, int P, int T, double iom, int min_shared, int32_t* comp, int32_t* members,
                  int32_t* d_G, long long* inst_cls, float* inst_scores, void* stream);
int gf_tile_assemble(const long long* table, const long long* table_host, int T, const int32_t* tile_of,
                     const int32_t* local_of, long long N, const uint32_t* bits, const int32_t* members, int P, int G,
                     int32_t* masks, int32_t* count, void* stream);

/* Per-point semantic scores of a scan stitched from the scores of its T tiles (csrc/tile_stitch.hip; the statement is
 * postprocess.stitch_tiles_host).  tile_of, local_of as above; core_of int32 [N]: the tile whose core holds the point.
 *   Tile score table, int64 [T, GF_TILE_SCORE_FIELDS], one GfTileScore per tile s (an empty tile has n_s = 0).
 *   table (device) and table_host (the same rows on the host): table_host is checked before the launch -- a negative
 *   n_s, a NULL pointer with n_s > 0, T outside 1..65535, C outside 1..gf_tile_stitch_max_classes(), a mode other than
 *   the two below or N < 0 are GF_ERR_INVALID_ARG; N == 0 succeeds with nothing launched.
 * gf_tile_stitch_scores (one launch, no memset: every cell of out is written): out fp32 [N, C].
 *   GF_TILE_STITCH_CORE: out[g] = the row of g in tile core_of[g] (the first slot j with tile_of[g, j] == core_of[g]),
 *     the same words copied; zeros when there is no such slot.
 *   GF_TILE_STITCH_MEAN: over the slots j = 0..3 in that order whose tile holds the point: acc = the row of the first
 *     one, then acc = acc + row (fp32, one add per slot, no multiplication), and out[g] = acc / (float)count, the
 *     correctly rounded division (exact for the counts 1, 2 and 4 of scene.tile_plan); zeros without a slot.
 *   A tile id outside [0, T) or a local index outside [0, n_s) contributes nothing and is never an address.  No
 *   atomics: bit-identical from call to call.  The launch goes on `stream`; no host synchronisation, no read-back. */
enum { GF_TILE_SCORE_FIELDS = 2 }; /* int64 words per row of the tile score table */
typedef struct {
    long long scores; /* scores pointer (fp32 [n_s, C], contiguous, the tile's points in the tile's own order) */
    long long n_s;
} GfTileScore;
enum { GF_TILE_STITCH_CORE = 0, GF_TILE_STITCH_MEAN = 1 };
int gf_tile_stitch_max_classes(void); /* = gf_semantic_confusion_max_classes(): the scores only ever go there */
int gf_tile_stitch_scores(const long long* table, const long long* table_host, int T, const int32_t* tile_of,
                          const int32_t* local_of, const int32_t* core_of, long long N, int C, int mode, float* out,
                          void* stream);

/* ===================================================================================
 * Instances of a scan that was run under V views (rotations / mirrors of the same N points), joined across the views
 * (csrc/view_merge.hip; the statement is postprocess.merge_views_host).  Every view holds all N points in the scan's
 * own order, so there are no point tables:
 *   View table, int64 [V, GF_TILE_SCENE_FIELDS], one GfTileScene per view v: masks, n_rows, n_s = N, pick, p_s,
 *   first_row; first_word is unused (0).  table (device) and table_host (the same rows on the host): table_host is
 *   checked before anything is launched -- a negative size, n_s != N, a NULL pointer with p_s > 0, a first row that does
 *   not follow the view before or picks that do not add up to P are GF_ERR_INVALID_ARG, and so are, in every call,
 *   P > gf_view_merge_max_rows(), V outside 1..gf_view_merge_max_views() and N outside [0, 2^31 - 1).
 * Rows 0 .. P-1 are the picked masks of all views, view-major, then by rank in pick; row_view int32 [P] is the view of
 * each row and view_first int32 [V + 1] the first row of each view (view_first[V] = P).  W = ceil(N / 32).
 *
 * gf_view_pack (one memset, one launch): bits uint32 [P, W], row-major bitsets -- bit p % 32 of word p / 32 of row a is
 *   set when the row's mask holds point p; the unused bits of the last word are 0; a pick outside [0, n_rows) is an
 *   empty row.  cnt int32 [P]: the points of each row (zeroed by the call; one integer add per wave).
 * gf_view_overlaps (one launch): inter int32 [P, P], inter[a, b] = the points in both rows; symmetric, the diagonal is
 *   cnt.  Every cell is defined by the call, whatever it held: stored by the one workgroup that owns it, or -- where
 *   few row blocks would leave the chip idle and the words are split over workgroups as well -- zeroed by a memset of
 *   the call and summed with integer atomic adds.
 * gf_view_best (one launch): best int32 [P, V]: best[a, v] = the row b of view v != row_view[a] with cls[b] == cls[a] and
 *   inter[a, b] > 0 of the largest IoU inter / (cnt[a] + cnt[b] - inter), compared exactly (cross-multiplied in int64),
 *   the smaller row on ties; -1 without such a row and for v == row_view[a].
 * gf_view_merge (one launch of ONE workgroup of 1024 threads): rows a < b are joined when best[a, row_view[b]] == b,
 *   best[b, row_view[a]] == a and (double)inter[a, b] >= iou * (double)(cnt[a] + cnt[b] - inter[a, b]) (one double
 *   multiplication and a compare).  comp int32 [P]: the smallest row of each row's connected component.  A component
 *   is kept when it has members in at least min_views views and its smallest row holds a point; members int32 [P]: the
 *   rank of the row's component among the kept ones (the global id) or -1; d_G int32 [1] = G.  First G valid of
 *   [P]: inst_cls int64 (the smallest row's class), inst_support int32 (the number of views with a member) and
 *   inst_scores fp32: m_v = the largest member score of view v or 0.0f, acc = m_0, acc = acc + m_v for v = 1 .. V-1
 *   (fp32, one rounded add each), acc / (float)V correctly rounded.  inst_first int32 [P + 1] (first G + 1 valid) and
 *   inst_rows int32 [P]: the member rows of instance g are inst_rows[inst_first[g] .. inst_first[g + 1]), ascending
 *   (hence sorted by view).
 * gf_view_assemble (one memset, one launch; every cell of masks is written): masks int32 [G, N] (0 / 1):
 *   votes = the views with a member row that holds the point; 1 when votes > 0 and (double)votes >= vote *
 *   (double)inst_support[g].  count int32 [G]: the points of each mask (zeroed by the call; one integer add per wave).
 * gf_view_mean_scores (one launch, no atomics): out fp32 [N, C] = (((s_0 + s_1) + s_2) + ...) / (float)V in view
 *   order, the correctly rounded division; score table int64 [V, GF_TILE_SCORE_FIELDS], one GfTileScore per view with
 *   n_s = N; C in 1..gf_tile_stitch_max_classes().
 * Integer atomics only; every output is a function of the inputs: bit-identical from call to call.  Every launch goes
 * on `stream`; no host synchronisation, no read-back.
 * =================================================================================== */
int gf_view_merge_max_rows(void);
int gf_view_merge_max_views(void);
int gf_view_pack(const long long* table, const long long* table_host, int V, int P, long long N, uint32_t* bits,
                 int32_t* cnt, void* stream);
int gf_view_overlaps(const uint32_t* bits, int P, long long N, int32_t* inter, void* stream);
int gf_view_best(const int32_t* inter, const int32_t* cnt, const long long* cls, const int32_t* row_view,
                 const int32_t* view_first, int P, int V, int32_t* best, void* stream);
int gf_view_merge(const int32_t* inter, const int32_t* cnt, const int32_t* best, const long long* cls,
                  const float* scores, const int32_t* row_view, int P, int V, double iou, int min_views, int32_t* comp,
                  int32_t* members, int32_t* d_G, long long* inst_cls, float* inst_scores, int32_t* inst_support,
                  int32_t* inst_first, int32_t* inst_rows, void* stream);
int gf_view_assemble(const uint32_t* bits, const int32_t* inst_first, const int32_t* inst_rows, const int32_t* row_view,
                     const int32_t* inst_support, int P, int G, long long N, double vote, int32_t* masks, int32_t* count,
                     void* stream);
int gf_view_mean_scores(const long long* table, const long long* table_host, int V, long long N, int C, float* out,
                        void* stream);

/* ===================================================================================
 * Headless rendering of a scene's points to images (csrc/render.hip; stands where util/visualize.py opens a viewer;
 * the statement is render.splat_host / render.resolve_host): a z-buffered point splat with 64-bit atomicMin, then a
 * resolve pass.  A whole call is memset (the caller's), splat, resolve: three stream operations for any V.
 * =================================================================================== */

/* Limits, as functions: the width of a camera record in floats (20), the views of one call (64), the side of an
 * image in pixels (4096), the disc radius in sub-pixels (16) and the supersampling factor (4). */
int gf_render_camera_floats(void);
int gf_render_max_views(void);
int gf_render_max_side(void);
int gf_render_max_radius(void);
int gf_render_max_supersample(void);

/* gf_render_splat: keys [V, Hs, Ws] (64-bit, preset by the caller to all-ones = background with one asynchronous memset
 * of 0xFF bytes on `stream`) <- min over the points whose disc covers the sub-pixel of (depthkey << 32 | point index).
 *   xyz fp32 [N, 3]; keep uint8 [N] or NULL (NULL: every point; 0 drops the point); cams fp32 [V, 20], per view
 *     {eye[3], R[9] row-major (rows: image right, image down, forward), kind (0 orthographic, 1 perspective),
 *      scale (orthographic: sub-pixels per metre; perspective: focal length in sub-pixels), cx, cy, near, spx, rmin,
 *      rmax}; Ws x Hs: the sub-pixel grid (each 1 .. gf_render_max_side() * gf_render_max_supersample());
 *   max_radius: 0 .. gf_render_max_radius(), the caller's bound on every record's rmax: radii are clamped to it, and it
 *     picks the launch shape (<= 3: a thread per (point, view); above: a wave per 64 points, lanes over each footprint).
 *   Per (view, point), float32, every operation rounded on its own, in this order:
 *     d = p - eye; xc = (R00 d0 + R01 d1) + R02 d2, yc and zc with rows 1 and 2;
 *     orthographic: u = xc scale + cx, v = yc scale + cy, r = rmin;
 *     perspective: culled when !(zc >= near); u = (xc scale) / zc + cx, v = (yc scale) / zc + cy;
 *       r = min(rmax, max(rmin, floor(spx / zc)));
 *       (as compares: r = rmin; if (q > r) r = q; if (r > rmax) r = rmax; if (!(r >= 0)) r = 0, with rmax taken as
 *       max_radius when it is not <= max_radius, so a NaN q leaves rmin and no record makes a larger disc);
 *     culled when u is NaN or outside [-(rmax + 1), Ws + rmax + 1) (v: Hs), before any conversion to an integer;
 *     (iu, iv) = (floor u, floor v); r as an integer;
 *     depthkey = zc's bits, all flipped when negative, the sign bit flipped otherwise (ascending with zc);
 *     atomicMin of the key on every sub-pixel (iu + dx, iv + dy) inside the image with dx^2 + dy^2 <= r^2 + r.
 *   Equal depths resolve to the lower point index: the result does not depend on the order of arrival, bit-identical
 *   from call to call.  No footprint leaves the image whatever the records hold.  N == 0 succeeds with nothing
 *   launched; NULL xyz / cams / keys, N < 0 or N >= 2^31, V outside 1 .. gf_render_max_views(), a side or max_radius
 *   outside its range are GF_ERR_INVALID_ARG with nothing launched. */
int gf_render_splat(const float* xyz, const unsigned char* keep, long long N, const float* cams, int V, int Ws, int Hs,
                    int max_radius, long long* keys, void* stream);

/* gf_render_resolve (one launch, no memset: every cell of image and index is written): keys [V, H S, W S] as
 * gf_render_splat left them -> index int32 [V, H S, W S], the winning point of every sub-pixel (-1: background), and
 * image uint8 [V, H, W, 3].  rgb uint8 [N, 3]; ids int32 [N] or NULL; h_lut: HOST, 9 int32 in 0..256 (Q8, 256 =
 * unchanged); stride 1..16 sub-pixels; background, outline: 0xRRGGBB.  Per foreground sub-pixel with point i, depth z
 * (recovered exactly from the key's high word): o = the number of its 8 neighbours at (+-stride, +-stride) inside
 * the image that are foreground with z_nb + dz < z (one fp32 add, one compare); colour = (rgb[i] * lut[o] + 128) >> 8
 * per channel; with ids, the outline colour instead when the right or the lower neighbour (inside the image) is
 * background or holds a point of another id.  Background sub-pixels take the background colour.  A pixel is the
 * integer mean (sum + S S / 2) / (S S) per channel over its S x S block.  A key whose index is not in [0, N) counts as
 * background.  W, H outside 1 .. gf_render_max_side(), S outside 1 .. gf_render_max_supersample(), V as above, a bad
 * table, stride or colour, N < 0 or a NULL pointer (ids aside; rgb may be NULL when N == 0) are GF_ERR_INVALID_ARG. */
int gf_render_resolve(const long long* keys, int V, int W, int H, int S, const unsigned char* rgb, const int32_t* ids,
                      long long N, const int32_t* h_lut, int stride, float dz, int background, int outline,
                      unsigned char* image, int32_t* index, void* stream);

/* ===================================================================================
 * Scans of any density (csrc/resample.hip; the statements are postprocess.grid_subsample_host and
 * postprocess.nearest_point_host): a voxel-grid subsample whose representatives are real points, and the nearest point
 * of one set for every point of another.  Integer atomics and 64-bit minima only: no result depends on the order in
 * which the points arrive, bit-identical from call to call.  Every launch goes on `stream`; nothing is read back.
 * =================================================================================== */

/* Limits, as functions: the points of one set (2^29), the cells per axis of the subsample (2^21) and the cells per
 * axis between the corners of the nearest-point grid (2^30: the range its 27-cell walk is proven for). */
int gf_resample_max_points(void);
int gf_grid_subsample_max_cells(void);
double gf_nearest_point_max_cells(void);

/* gf_grid_subsample: xyz fp32 [N, 3]; cell > 0, finite; mode 0 = first, 1 = center; origin: DEVICE fp32 [3], or NULL
 * for the per-axis minimum of xyz (found on the device).  Per point and axis, fp32, every operation rounded on its own:
 * t = (x - origin) / cell (correctly rounded division), c = floor(t); the point is valid when t is finite and
 * 0 <= c < gf_grid_subsample_max_cells().  Cells are numbered in order of their lowest point index.
 *   cell_of int32 [N]: the number of every point's cell;   count int32 [N], first M written: the points of a cell;
 *   rep int32 [N], first M written: mode 0: the cell's lowest point index; mode 1: the point of the cell minimising
 *     (d2, index), d = x - (origin + (c + 0.5) * cell) (add, multiply, add), d2 = (dx dx + dy dy) + dz dz;
 *   d_words int32 [2] (device): {M, 1 when some point is invalid -- the outputs then mean nothing};
 *   scratch: gf_grid_subsample_scratch_bytes(N).
 * N < 0 or above gf_resample_max_points(), a cell that is not positive and finite, another mode, or a NULL pointer
 * (origin aside) with N > 0 are GF_ERR_INVALID_ARG with nothing launched; N == 0 succeeds with nothing launched (and
 * nothing written). */
size_t gf_grid_subsample_scratch_bytes(int N);
int gf_grid_subsample(const float* xyz, int N, float cell, int mode, const float* origin, void* scratch, int32_t* rep,
                      int32_t* cell_of, int32_t* count, int32_t* d_words, void* stream);

/* gf_nearest_point: query fp32 [Q, 3], xyz fp32 [n, 3], max_dist > 0, finite; r2 = max_dist * max_dist (fp32).  Per
 * query: among the points with d2 <= r2, d2 = (dx dx + dy dy) + dz dz of d = query - point (fp32), the one minimising
 * (d2, index): idx int32 [Q], d2 fp32 [Q]; (-1, inf) without one.  A point with a non-finite coordinate is never a
 * candidate; a query with one gets (-1, inf), and so does, without a walk, a query more than a cell outside the
 * points' bounding box.  The search walks the 27 cells of a hash grid (cells of max_dist * 1.001, coordinates taken
 * in fp64 from the points' minimum corner) around the query's own.
 *   d_flag int32 [1] (device): 1 when the points' bounding box spans gf_nearest_point_max_cells() cells or more on an
 *     axis -- beyond the range the walk is proven complete for: the caller must not use the result;
 *   scratch: gf_nearest_point_scratch_bytes(n).
 * Q < 0, n < 0 or above gf_resample_max_points(), a max_dist that is not positive and finite, or a NULL pointer (xyz
 * may be NULL when n == 0) are GF_ERR_INVALID_ARG with nothing launched; Q == 0 succeeds with nothing launched. */
size_t gf_nearest_point_scratch_bytes(int n);
int gf_nearest_point(const float* query, int Q, const float* xyz, int n, float max_dist, void* scratch, int32_t* idx,
                     float* d2, int32_t* d_flag, void* stream);

/* ===================================================================================
 * Backbone voxel transformer of the two deepest U-Net levels, fused (inference)
 * (UBlock: model/geoformer/geoformer_modules.py:64-68,120-127; TransformerEncoder(d_model=128, N,
 *  heads=4, d_ff=64): model/transformer.py:62-188)
 * =================================================================================== */

/* out = after(TransformerEncoder(xyz, before(feats))) per scene in n_layers + 2 launches (n_scenes <= 4096).
 *   feats fp32 [M,c] (c % 16 == 0, c <= 384), coords int32 [M,4] (b,x,y,z) with the rows of a scene contiguous,
 *   scene_offsets int32 [n_scenes+1] (device), out fp32 [M,c],
 *   scratch: gf_backbone_transformer_scratch_bytes(M) bytes,
 *   params: HOST array of gf_backbone_transformer_num_params(n_layers) DEVICE pointers, nn.Linear weights
 *   row-major [out,in], in this order:
 *     before.W[128,c] before.b | position.W[128,3] position.b |
 *     per layer: norm1.alpha norm1.bias  q.W q.b  k.W k.b  v.W v.b  out.W out.b  norm2.alpha norm2.bias
 *                ff1.W[64,128] ff1.b  ff2.W[128,64] ff2.b |
 *     norm.alpha norm.bias | after.W[c,128] after.b */
size_t gf_backbone_transformer_scratch_bytes(int M);
int gf_backbone_transformer_num_params(int n_layers);
int gf_backbone_transformer(const float* feats, const int* coords, const int* scene_offsets, int n_scenes, int M,
                            int c, int n_layers, const float* const* params, void* scratch, float* out,
                            void* stream);

/* Training form of the same stack (what train.py:63-75 runs through the framework modules of
 * geoformer_modules.py:64-68,120-127 and transformer.py:62-188 with their dropouts, p = transformer.py's 0.1): the
 * forward keeps what the backward needs in `save`, the backward returns the gradient of the input rows and of every
 * parameter -- n_layers + 2 and 2 n_layers + 2 launches instead of ~250 framework launches per level and step.
 *   coords int32 [M,4] with the scene id in column 0, ascending (scene offsets are found on the device);
 *   p: dropout probability of the four dropout sites of a layer (0: every element kept -- modules in eval mode);
 *   seed: the call's dropout seed (the same value must be passed to the backward): an element is kept iff
 *     (h >> 8) >= (uint32)(p * 2^24),  h = fmix32(fmix32(seed ^ (row * 64 + site)) + col * 0x9E3779B1),
 *     fmix32 = MurmurHash3's finaliser, site = 4 * layer + {0 attention weights, 1 attention branch, 2 hidden layer,
 *     3 feed-forward branch}, row = the token's row in the batch, col = the channel (attention weights: 4 * key's
 *     index in its scene + head); kept elements are scaled by 1 / (1 - p);
 *   save: gf_backbone_transformer_train_save_bytes(M, n_layers) bytes, written by the forward, read by the backward;
 *   work: gf_backbone_transformer_train_work_bytes(M, n_layers, n_scenes) bytes of scratch for the backward;
 *   dfeats fp32 [M,c]; grads: gf_backbone_transformer_grad_floats(c, n_layers) floats, the parameters' gradients
 *   back to back in the order of the parameter table, each in its parameter's layout (every value is written).
 *   c % 16 == 0, c <= 384.  Summation orders are fixed: the same inputs give the same bits. */
size_t gf_backbone_transformer_train_save_bytes(int M, int n_layers);
size_t gf_backbone_transformer_train_work_bytes(int M, int n_layers, int n_scenes);
long long gf_backbone_transformer_grad_floats(int c, int n_layers);
int gf_backbone_transformer_train_fwd(const float* feats, const int* coords, int n_scenes, int M, int c, int n_layers,
                                      const float* const* params, float p, unsigned seed, void* save, float* out,
                                      void* stream);
int gf_backbone_transformer_train_bwd(const float* feats, const float* dout, int n_scenes, int M, int c, int n_layers,
                                      const float* const* params, float p, unsigned seed, void* save, void* work,
                                      float* dfeats, float* grads, void* stream);

/* ===================================================================================
 * Decoder cross-attention (TransformerDecoderLayer.forward_pre_rel, model/transformer_detr.py:443-454
 * with the relative embedding of GeoFormer.forward_decoder, model/geoformer/geoformer.py:619-651), fused
 * =================================================================================== */

/* Packs attn_mlp.0.weight (W1), attn_mlp.2.weight (W2) and v_mlp.0.weight (Wv), each [64,64] (out,in),
 * into MFMA A-operand lane order; Wpack holds gf_decoder_wpack_floats() floats. */
size_t gf_decoder_wpack_floats(void);
int gf_decoder_pack_weights(const float* W1, const float* W2, const float* Wv, float* Wpack, void* stream);

/* out[b,i,:] = sum_j softmax_j(sim_ij / 8) * (Kv[b,j,:] + Wv r_ij),   sim_ij = W2 relu(Q1[b,i,:] - K1[b,j,:] + W1 r_ij) + b2,
 * r_ij = [sin(P), cos(P)], P = 2*pi*((g3 - lo)/(hi - lo)) . gaussB,  g3 = geo_ctx[b,i,j] on all three axes, or
 * max_geo[b,i] + |qloc[b,i] - cloc[b,j]| per axis where geo_ctx < 0.
 *   geo_ctx [B,nq,nc], max_geo [B,nq], qloc [B,nq,3], cloc [B,nc,3], lo/hi [B,3] (the pc_dims pair as the
 *   caller passes it -- GeoFormer passes [maxs, mins]), gaussB [3,32],
 *   Q1 = W1 q + b1 [B,nq,64], K1 = W1 k [B,nc,64], Kv = Wv k + bv [B,nc,64], b2 [64];  out [B,nq,64]. */
int gf_decoder_cross_attn(const float* geo_ctx, const float* max_geo, const float* qloc, const float* cloc,
                          const float* lo, const float* hi, const float* gaussB, const float* Q1, const float* K1,
                          const float* Kv, const float* Wpack, const float* b2, int B, int nq, int nc, int d, float* out,
                          float* stat_m, float* stat_l, void* stream);
/* The same with the workgroup shape chosen: wg_waves = 16 (gf_decoder_cross_attn) or 8 -- 512 threads at 120 registers
 * fit on a compute unit BESIDE a 512-thread workgroup of gf_geodesic_bfs_cfg, for a serving loop that runs one scene's
 * decoder under the next scene's sampling / BFS stretch (GeoFormer.forward_split).  Results agree to rounding (the
 * per-wave partial soft-max states are merged over 8 instead of 16 waves). */
int gf_decoder_cross_attn_cfg(const float* geo_ctx, const float* max_geo, const float* qloc, const float* cloc,
                              const float* lo, const float* hi, const float* gaussB, const float* Q1, const float* K1,
                              const float* Kv, const float* Wpack, const float* b2, int B, int nq, int nc, int d,
                              float* out, float* stat_m, float* stat_l, int wg_waves, void* stream);

/* Backward of gf_decoder_cross_attn (training).  stat_m / stat_l fp32 [B,nq,64]: per (query, channel) maximum and
 * sum of the scaled soft-max logits, written by the forward when the two pointers are given (NULL otherwise); out =
 * the forward's output, gout = dL/dout fp32 [B,nq,64]; W2 fp32 [64,64] the second pair-MLP weight (unpacked).
 * Outputs: dQ1 fp32 [B,nq,64] (overwritten), dK1 / dKv fp32 [B,nc,64] (zero on entry), dW fp32 [3,64,64] = the PAIR
 * parts of dW1, dW2, dWv (overwritten; the hoisted parts W1 q, W1 k, Wv k are the caller's GEMMs).  Everything of size
 * nq*nc*64 is recomputed.  scratch: gf_decoder_cross_attn_bwd_scratch_floats(B,nq,nc) floats. */
size_t gf_decoder_cross_attn_bwd_scratch_floats(int B, int nq, int nc);
int gf_decoder_cross_attn_bwd(const float* geo_ctx, const float* max_geo, const float* qloc, const float* cloc,
                              const float* lo, const float* hi, const float* gaussB, const float* Q1, const float* K1,
                              const float* Kv, const float* Wpack, const float* W2, const float* out, const float* stat_m,
                              const float* stat_l, const float* gout, int B, int nq, int nc, int d, float* dQ1, float* dK1,
                              float* dKv, float* dW, float* scratch, void* stream);

/* ===================================================================================
 * Natives GeoFormer inherits but never executes -- binding completeness
 * =================================================================================== */

/* PG_OP.sec_mean / sec_min / sec_max (sec_mean.cu:12-86): kind 0/1/2; offsets int32 [nProposal+1]; out [nProposal,C] */
int gf_sec_op(int kind, const float* inp, const int32_t* offsets, int nProposal, int C, float* out, void* stream);
/* PG_OP.roipool_fp/bp (roipool.cu:12-57): segment max + arg-max; bp adds d_out to d_feats[argmax] (caller zeroes) */
int gf_roipool_fp(const float* feats, const int32_t* offsets, int nProposal, int C, float* out, int32_t* maxidx,
                  void* stream);
int gf_roipool_bp(const float* d_out, const int32_t* maxidx, int nProposal, int C, float* d_feats, void* stream);
/* PG_OP.get_iou (get_iou.cu:12-38): iou [nProposal,nInstance]; instance_labels int64 [N] */
int gf_get_iou(const int32_t* proposals_idx, const int32_t* proposals_offset, const long long* instance_labels,
               const int32_t* instance_pointnum, int nInstance, int nProposal, float* iou, void* stream);
/* PG_OP.ballquery_batch_p (bfs_cluster.cu:15-89): idx int32 [n*meanActive], start_len int32 [n,2], starts in point
 * order; d_cumsum (device int32) = total pair count (the reference's return value). */
size_t gf_ballquery_batch_p_scratch_bytes(int n);
int gf_ballquery_batch_p(const float* xyz, const int32_t* batch_idxs, const int32_t* batch_offsets, int n, int meanActive,
                         float radius, int32_t* idx, int32_t* start_len, int32_t* d_cumsum, void* scratch, void* stream);
/* PG_OP.bfs_cluster (bfs_cluster.cpp:28-111): HOST pointers (the reference runs it on CPU tensors).
 * h_cluster_idxs capacity [N,2], h_cluster_offsets capacity [N+1]. */
int gf_bfs_cluster_host(const int32_t* h_semantic_label, const int32_t* h_ball_query_idxs, const int32_t* h_start_len,
                        int N, int threshold, int32_t* h_cluster_idxs, int32_t* h_cluster_offsets, int32_t* h_nCluster,
                        int32_t* h_sumNPoint);
/* pointnet2._ext.three_nn / three_interpolate / three_interpolate_grad (interpolate_gpu.cu:12-157) */
int gf_three_nn(const float* unknown, const float* known, int b, int n, int m, float* dist2, int32_t* idx, void* stream);
int gf_three_interpolate(const float* points, const int32_t* idx, const float* weight, int b, int c, int m, int n,
                         float* out, void* stream);
int gf_three_interpolate_grad(const float* grad_out, const int32_t* idx, const float* weight, int b, int c, int n, int m,
                              float* grad_points, void* stream);

/* ===================================================================================
 * Training-batch augmentation and collate (datasets/scannetv2_inst.py:267-387 InstDataset.trainMerge; csrc/augment.hip,
 * geoformer_amd/augment.py).  All device pointers; every call queues its launches on `stream` and syncs nothing.
 *   A batch of B raw scenes: raw fp64 [n_raw, 8] (xyz, rgb, label, instance), raw_off int64 [B+1] (device).
 *   rec int64 [B, GF_AUG_REC]: per-scene record (GF_AUG_R_* words, doubles stored as their bit patterns); the caller
 *   initialises it (caps / bases of the noise grids, key sentinels) and, with rng="reference", writes the draws.
 *   noise[p] fp32: raw noise of elastic pass p, scene s's three grids at rec[s][BASE_p] + axis * rec[s][CAP_p];
 *   work[p]: 2 * cells[p] floats (the blurred grids end in work[p] + cells[p]).
 *   Outputs at capacity n_raw rows (the first head[GF_AUG_H_N] are the batch; rows behind them hold padding coordinates
 *   (batch 0xffff) that voxelise into one voxel each behind all real voxels), instance_pointnum capacity B * max_inst.
 *   head int32 [GF_AUG_HEAD]: kept points, instances, error bits (GF_AUG_ERR_*), max locs (3), spatial shape (3).
 * =================================================================================== */
#define GF_AUG_REC 320
#define GF_AUG_MAX_INST 4096 /* instance ids per scene: 0 .. max_inst-1 (or -100) */
#define GF_AUG_MAX_CROP 64   /* crop candidates */
#define GF_AUG_LUT 128       /* raw semantic labels the remap table covers */
#define GF_AUG_STAT 10       /* per instance: count, fixed-point sums (3), min keys (3), max keys (3) */
#define GF_AUG_HEAD 16
enum {
    GF_AUG_R_M = 0, GF_AUG_R_SHIFT = 9, GF_AUG_R_FLIP = 12, GF_AUG_R_THETA = 13, GF_AUG_R_AMAX0 = 14,
    GF_AUG_R_AMAX1 = 17, GF_AUG_R_MIN = 20, GF_AUG_R_MAX = 23, GF_AUG_R_CHOSEN = 26, GF_AUG_R_ERR = 27,
    GF_AUG_R_CAP0 = 28, GF_AUG_R_BASE0 = 29, GF_AUG_R_CAP1 = 30, GF_AUG_R_BASE1 = 31, GF_AUG_R_PCMIN = 32,
    GF_AUG_R_PCMAX = 35, GF_AUG_R_NINST = 38, GF_AUG_R_IBASE = 39, GF_AUG_R_COUNTS = 64, GF_AUG_R_CROPU = 128,
    /* ABI 7: first instance_pointnum slot of the scene (== IBASE except in few-shot queries, whose ids stay local);
     * few-shot query: the scene's sampled class; few-shot support: the support instance id (both set by the caller) */
    GF_AUG_R_PBASE = 40, GF_AUG_R_CLASS = 41, GF_AUG_R_SUPID = 42,
    /* few-shot test-time block supports: the instance's min / max keys and point count, the scene's max locs */
    GF_AUG_R_BMIN = 43, GF_AUG_R_BMAX = 46, GF_AUG_R_BCNT = 49, GF_AUG_R_BLMAX = 50
};
enum { GF_AUG_H_N = 0, GF_AUG_H_NINST = 1, GF_AUG_H_ERR = 2, GF_AUG_H_LMAX = 3, GF_AUG_H_SHAPE = 6 };
enum { GF_AUG_ERR_CELLS = 1, GF_AUG_ERR_INST = 2, GF_AUG_ERR_NOINST = 4 };
typedef struct {
    int B, n_raw, max_inst, pad_;
    const double* raw;
    const long long* raw_off;
    long long* rec;
    double* xyz_middle; /* [n_raw, 3] */
    double* xyz;        /* [n_raw, 3]: scaled, distorted, then cropped */
    float* noise[2];
    float* work[2];
    long long cells[2];
    int32_t* flags;      /* [n_raw] */
    int32_t* lab;        /* [n_raw] */
    int32_t* inst;       /* [n_raw] */
    int32_t* start;      /* [n_raw + 1] */
    int32_t* cursor;     /* [n_raw] */
    int32_t* block_sums; /* [gf_aug_scan_blocks(n_raw)] */
    int32_t* block_off;  /* [gf_aug_scan_blocks(n_raw)] */
    int32_t* sidx;       /* [n_raw] */
    uint32_t* bitmap;    /* [B * max_inst / 32] */
    int32_t* inst_map;   /* [B * max_inst] */
    long long* inst_stats; /* [B * max_inst * GF_AUG_STAT] */
    long long* locs;     /* [n_raw, 4] */
    float* locs_float;   /* [n_raw, 3] */
    double* feats;       /* [n_raw, 3] */
    long long* labels;   /* [n_raw] */
    long long* instance_labels; /* [n_raw] */
    float* instance_infos;      /* [n_raw, 9] */
    int32_t* instance_pointnum; /* [B * max_inst] */
    int32_t* offsets;    /* [B + 1] */
    float* pc_mins;      /* [B, 3] */
    float* pc_maxs;      /* [B, 3] */
    int32_t* head;       /* [GF_AUG_HEAD] */
} GfAugBatch;
int gf_aug_scan_blocks(int n_raw);
/* rng="device": Philox4x32-10 draws of every scene (jitter, flip, angle -> m; colour shift; K crop offsets) into rec */
int gf_aug_draw(const GfAugBatch* b, unsigned long long seed, long long batch_index, int K, void* stream);
/* scenes [s0, s0+ns): xyz_middle = x @ m, xyz = xyz_middle * scale, per-scene |xyz| max (grid of elastic pass 0) */
int gf_aug_transform(const GfAugBatch* b, int s0, int ns, double scale, int max_scene_points, void* stream);
/* elastic pass 0 / 1 (gran, mag): fill = 1 draws the raw noise (Philox; else the caller uploaded it), six box blurs,
 * xyz += g(xyz) * mag; pass 0 leaves the |xyz| max of pass 1's grid, pass 1 the per-scene min / max */
int gf_aug_elastic(const GfAugBatch* b, int s0, int ns, int pass, int gran, double mag, int fill,
                   unsigned long long seed, long long batch_index, int max_scene_points, long long max_cells,
                   void* stream);
/* the K crop candidates of every scene with more than max_npoint points counted in one launch; rec[CHOSEN] = the first
 * that fits (-1: no crop) */
int gf_aug_crop(const GfAugBatch* b, int s0, int ns, int full_scale, int K, long long max_npoint, int max_scene_points,
                void* stream);
/* all scenes: kept points in order, label remap (fold_classes: HOST int32[n_fold]), getCroppedInstLabel, per-instance
 * statistics, the collate's outputs, head */
int gf_aug_collate(const GfAugBatch* b, const int32_t* fold_classes, int n_fold, int full_scale_min, int full_scale,
                   int max_scene_points, void* stream);

/* Few-shot episodes (datasets/scannetv2_fs_inst.py:330-365, 397-566 FSInstDataset.trainMergeFS; ABI 7).
 * Query: gf_aug_draw / _transform / _elastic / _crop as above, then gf_aug_collate_fs instead of gf_aug_collate:
 *   labels = (raw label == rec[s][GF_AUG_R_CLASS]) as 0/1, instances of label 0 -> -100, getCroppedInstLabel per scene
 *   with scene-local ids (the reference's offset total_inst_num stays 0), instance_pointnum concatenated over the scenes,
 *   feats = raw colours (no shift), instance_infos not written (may be NULL).
 * Support: gf_aug_support on a batch of raw support scenes (no draws, no crop; rec: GF_AUG_R_MIN / _PCMIN initialised to
 *   -1, _PCMAX to 0, GF_AUG_R_SUPID set): locs = (scene, trunc(xyz * scale - min(xyz * scale))), locs_float, feats,
 *   support_masks int64 [n_raw] = (instance == rec[s][GF_AUG_R_SUPID]), offsets = raw_off, pc_mins / pc_maxs of xyz,
 *   head N = n_raw (no padding rows), max locs and spatial shape.  Uses raw, raw_off, rec, locs, locs_float, feats,
 *   offsets, pc_mins, pc_maxs, head of b. */
int gf_aug_collate_fs(const GfAugBatch* b, int full_scale_min, int full_scale, int max_scene_points, void* stream);
int gf_aug_support(const GfAugBatch* b, long long* support_masks, double scale, int full_scale_min,
                   int max_scene_points, void* stream);

/* Few-shot test time (datasets/scannetv2_fs_inst.py:568-700 FSInstDataset.testMergeFS).
 * Query: gf_aug_test_query on a batch of raw scenes (no draws, no crop, rec as for gf_aug_support): the support path
 *   with the raw semantic labels (int64, into labels) instead of a mask; pc_mins / pc_maxs also stay in rec
 *   (GF_AUG_R_PCMIN / _PCMAX keys, the reference keeps them in fp64).
 * Block supports: gf_aug_support_block on B (scene, rec[s][GF_AUG_R_SUPID]) pairs (rec: GF_AUG_R_BMIN, _MIN, _PCMIN
 *   initialised to -1, the rest 0): the instance's bounding box (fp64, get_region_inst with scale_factor 1), the in-box
 *   points in order compacted to the front of the scene's own raw range (flags / start / cursor / block_* scratch),
 *   locs = (0, trunc(xyz * scale - min of the kept xyz * scale)), locs_float, feats (fp64), support_masks int64
 *   [n_raw]; rows behind a scene's kept points hold padding coordinates (batch 0xffff) so each range voxelises on its
 *   own.  scene_sizes int32 [B, 5]: kept points, instance points, spatial shape (max locs + 1, at least
 *   full_scale_min); offsets = running kept counts; pc_mins / pc_maxs of the kept xyz as GF_AUG_R_PCMIN / _PCMAX keys;
 *   head N = kept total, head ERR |= GF_AUG_ERR_NOINST when an instance id has no point in its scene. */
int gf_aug_test_query(const GfAugBatch* b, double scale, int full_scale_min, int max_scene_points, void* stream);
int gf_aug_support_block(const GfAugBatch* b, long long* support_masks, int32_t* scene_sizes, double scale,
                         int full_scale_min, int max_scene_points, void* stream);

/* ===================================================================================
 * 3D boxes of instances and the IoU of boxes (csrc/boxes.hip; the statements are postprocess.instance_boxes_host and
 * postprocess.box_iou_host).  A box is upright: oriented about z only, the heading convention of indoor detection.
 * Only extents (integer maxima of order-preserving keys) and integer counts are reduced: every output is a function of
 * the inputs, bit-identical from call to call and to the statement.  Coordinates are finite.  Every launch goes on
 * `stream`; no host synchronisation, no read-back.
 * =================================================================================== */

/* A box is one GfBox, GF_BOX_FLOATS float64; an empty group is a row of zeros.
 * Box scene table, int64 [S, GF_BOX_SCENE_FIELDS], one GfBoxScene per scene:
 *   GF_BOX_FORM_ROWS: group = masks int32 [n, N], nonzero = member (masks may overlap; NULL when n == 0); pick int64
 *     [p]: group r is row pick[r]; a pick outside [0, n) is an empty group, never an address.
 *   GF_BOX_FORM_IDS: group = int32 [N] with values in [-1, p), -1 = no group (any other value outside [0, p) names no
 *     group either); n and pick are not read.
 * Limits, as functions: the points of one workgroup's chunk, the most angles, the most groups of one scene. */
enum { GF_BOX_SCENE_FIELDS = 8, GF_BOX_FLOATS = 10, GF_BOX_IOU_FIELDS = 5 };
enum { GF_BOX_FORM_ROWS = 0, GF_BOX_FORM_IDS = 1 };
typedef struct {
    double cx, cy, cz; /* centre */
    double du, dv, dz; /* sizes: du lies along (c, s), dv along (-s, c), dz along z */
    double c, s;       /* heading */
    double angle;      /* index of the heading in `angles` */
    double count;      /* points of the group */
} GfBox;
typedef struct {
    long long form;    /* GF_BOX_FORM_ROWS / GF_BOX_FORM_IDS */
    long long N, n, p;
    long long group;   /* groups pointer, by form */
    long long pick;    /* pick pointer (int64 [p]) */
    long long xyz;     /* xyz pointer (fp32 [N, 3]) */
    long long row_off; /* rows into count / aligned / oriented, p of them */
} GfBoxScene;
typedef struct {
    long long P, G;
    long long a_off, b_off; /* rows of a / of b */
    long long out_off;      /* elements of out */
} GfBoxIouScene;
int gf_box_chunk(void);
int gf_box_max_angles(void);
int gf_box_max_groups(void);

/* gf_instance_boxes_batched (two memsets, two launches for any S, p and forms): per group its point count, its
 * axis-aligned box and the box of least footprint among the A headings of `angles`.
 *   max_points / max_groups: the largest N / p of the table; rows: the sum of p; angles fp32 [A, 2] = (c, s) pairs,
 *   1 <= A <= gf_box_max_angles(); scratch: gf_instance_boxes_scratch_bytes(rows, A), preset by the call.
 *   count int32 [rows]; aligned, oriented float64 [rows, GF_BOX_FLOATS].
 * Aligned: the minima and maxima of the members' fp32 x, y, z; c = 1, s = 0, index 0.
 * Oriented: per angle a the extents of u = fl(fl(x c) + fl(y s)) and v = fl(fl(y c) - fl(x s)) over the members, fp32,
 *   every operation rounded on its own; area_a = fl(fl(umax - umin) fl(vmax - vmin)); the box is the angle of least
 *   area, the lowest index among equals.
 * Both: sizes max - min and the frame's centre (min + max) / 2 in float64 from the fp32 extents (exact); cx = lu c - lv s,
 *   cy = lu s + lv c in float64, every operation rounded on its own.  Extents are ordered as their keys are: -0 below +0.
 * Bad sizes, A outside its range or a NULL pointer with rows > 0 are GF_ERR_INVALID_ARG with nothing launched; S == 0
 * or rows == 0 succeeds with nothing launched. */
size_t gf_instance_boxes_scratch_bytes(long long rows, int A);
int gf_instance_boxes_batched(const long long* table, int S, long long max_points, int max_groups, long long rows,
                              const float* angles, int A, void* scratch, int32_t* count, double* aligned,
                              double* oriented, void* stream);

/* gf_box_iou_batched (one launch, one thread per pair): the 3D IoU of every (a, b) pair of every scene.
 *   IoU table, int64 [S, GF_BOX_IOU_FIELDS], one GfBoxIouScene per scene;
 *   a, b: packed boxes, float64 [., GF_BOX_FLOATS]; out: float64, scene block [P, G] row-major at out_off; max_pairs:
 *   the largest P G of the table.
 * float64, every + - * / rounded on its own, no sin / cos.  Per axis the overlap of two intervals with half sizes ha,
 *   hb whose centres are d apart is max(0, min(ha, d + hb) - max(-ha, d - hb)).  Both boxes with s == 0 (their sides
 *   along the axes): area = overlap in x times overlap in y.  Otherwise: a's rectangle is taken into b's frame
 *   (counter-clockwise from the (-u, -v) corner) and cut by b's four sides in the order u >= -hu, u <= hu, v >= -hv,
 *   v <= hv (Sutherland-Hodgman, at most 8 vertices), area = |shoelace sum in vertex order| / 2.
 *   inter = area times the overlap in z, 0 when either box has no volume; IoU = inter / (volA + volB - inter), 0 where
 *   that denominator is <= 0; vol = (du dv) dz. */
int gf_box_iou_batched(const long long* table, int S, long long max_pairs, const double* a, const double* b, double* out,
                       void* stream);

/* ===================================================================================
 * Scenes from posed depth frames (csrc/frames.hip; the statements are frames.backproject_host and
 * frames.cell_means_host): every depth pixel of a set of frames to a world point, and one fused point per grid cell
 * as the mean of the points gf_grid_subsample put into it.  Ballots, integer scans and 64-bit integer atomic adds
 * only: no result depends on the order in which pixels or points arrive, bit-identical from call to call.  No
 * workgroup ever waits for another: a compaction is count, scan, write as three launches.  Every launch goes on
 * `stream`; nothing is read back.
 * =================================================================================== */

/* Limits, as functions: the width of a frame record in floats (16), the frames of one call (65536), the side of a
 * depth image in pixels (8192) and the default number of elements a workgroup compacts (2048). */
int gf_frames_record_floats(void);
int gf_frames_max_frames(void);
int gf_frames_max_side(void);
int gf_frames_default_chunk(void);

/* gf_frames_backproject (two memsets, four launches): the valid pixels of F depth images as world points, compacted
 * in ascending order of the sampled-pixel index t = (f Hs + j0) Ws + i0.
 *   depth: kind 0: uint16 [F, H, W]; kind 1: fp32 [F, H, W];   depth_shift: fp32, positive and finite;
 *   color: uint8 [F, H, W, 3] or NULL;
 *   frames fp32 [F, 16]: {fx, fy, cx, cy, P[12]}, P rows 0..2 of the camera-to-world pose, row-major (camera axes: x
 *     right, y down, z forward; pixel i covers [i, i + 1));
 *   stride >= 1: the sampled pixel (i0, j0) is the pixel (i, j) = (i0 stride, j0 stride); Ws = ceil(W / stride), Hs
 *     likewise; near, far: any floats; edge: >= 0 and finite, 0 = no edge filter;
 *   chunk: the sampled pixels one workgroup compacts: a multiple of 64 in 64 .. 65536, or 0 for the default.  The block
 *     counts are scanned by one workgroup, 256 at a time with a carry: more than 256 chunks is its second regime.
 * Per sampled pixel, fp32, every operation rounded on its own, in this order:
 *   z = (float)d / depth_shift (correctly rounded); invalid when !(z >= near) || !(z <= far);
 *   with edge > 0: invalid when one of the pixels (i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1) that lies inside the
 *     image and is itself in [near, far] has |zn - z| > edge z (one subtraction, one multiplication, one compare);
 *   xc = ((((float)i + 0.5) - cx) z) / fx, yc = ((((float)j + 0.5) - cy) z) / fy (correctly rounded divisions);
 *   X = ((P0 xc + P1 yc) + P2 z) + P3, Y with P4..P7, Z with P8..P11.
 * Outputs: xyz fp32 [T, 3], rgb uint8 [T, 3] (0 without color), pixel_of int32 [T]: the first n rows written;
 *   point_of int32 [F, Hs, Ws]: the row of every valid pixel, -1 elsewhere (every cell written);
 *   lo fp32 [3] (device) or NULL: the per-axis minimum of the written coordinates (by integer minima of ordered keys: -0
 *     below +0; not used when n == 0) -- the default origin of the grid the points go into next;
 *   d_words int32 [2] (device): {n, 1 when a written coordinate is not finite};
 *   scratch: gf_frames_backproject_scratch_bytes(T, chunk), T = F Hs Ws.
 * F outside 1 .. gf_frames_max_frames(), W or H outside 1 .. gf_frames_max_side(), T above
 * gf_resample_max_points(), another kind, a bad depth_shift, stride, edge or chunk, or a NULL pointer (color aside)
 * are GF_ERR_INVALID_ARG with nothing launched. */
size_t gf_frames_backproject_scratch_bytes(long long T, int chunk);
int gf_frames_backproject(const void* depth, int kind, float depth_shift, const unsigned char* color, const float* frames,
                          int F, int W, int H, int stride, float near, float far, float edge, int chunk, void* scratch,
                          float* xyz, unsigned char* rgb, int32_t* pixel_of, int32_t* point_of, float* lo,
                          int32_t* d_words, void* stream);

/* gf_frames_cell_means (two memsets, four launches): one fused point per cell that at least min_obs points fell into.
 *   xyz fp32 [n, 3], rgb uint8 [n, 3]; cell_of int32 [n] in [0, M) and count int32 [M] >= 1 as gf_grid_subsample gave
 *   them; origin: DEVICE fp32 [3], no coordinate above the points' (gf_grid_subsample's origin); min_obs >= 1;
 *   chunk: the cells one workgroup compacts, as above.
 * Per point and axis, float64: e = (double)x - (double)o, q = (int64)floor(e 1048576.0) (units of 2^-20 m; the
 *   multiplication is exact); per cell sum_q by 64-bit integer atomic adds (adjacent lanes of a wave that hold the same
 *   cell add their values first and issue one atomic when aggregate != 0: integer sums, so the same result), and
 *   mean = (float)((double)o + ((double)sum_q / (double)count) (1.0 / 1048576.0)), every operation rounded on its own.
 *   Colour per channel: (sum + count / 2) / count on 64-bit integer sums.
 *   A point with !(0 <= e < 16384) raises the flag: within 2^14 m the 2^29 points of a call sum below 2^63.
 * Kept cells (count >= min_obs) hold their order and are renumbered densely:
 *   xyz_out fp32 [M, 3], rgb_out uint8 [M, 3], count_out int32 [M]: the first m rows written;
 *   new_id int32 [M]: the row of a kept cell, -1 for a dropped one;
 *   d_words int32 [2] (device): {m, flag};   scratch: gf_frames_cell_means_scratch_bytes(M, chunk).
 * n or M outside 1 .. gf_resample_max_points(), min_obs < 1, a bad chunk or a NULL pointer are GF_ERR_INVALID_ARG with
 * nothing launched. */
size_t gf_frames_cell_means_scratch_bytes(int M, int chunk);
int gf_frames_cell_means(const float* xyz, const unsigned char* rgb, const int32_t* cell_of, const int32_t* count, int n,
                         int M, const float* origin, int min_obs, int aggregate, int chunk, void* scratch, float* xyz_out,
                         unsigned char* rgb_out, int32_t* count_out, int32_t* new_id, int32_t* d_words, void* stream);

/* gf_frames_compose (one launch): point_of int32 [T] of gf_frames_backproject, in place, to the fused point of every
 * pixel: new_id[cell_of[p]] where p >= 0, -1 elsewhere.  T == 0 succeeds with nothing launched. */
int gf_frames_compose(int32_t* point_of, long long T, const int32_t* cell_of, const int32_t* new_id, void* stream);

/* gf_frames_vote (csrc/frames_vote.hip; the statement is frames.vote_host; four memsets, three launches): per group the
 * value most of its elements hold -- per-pixel labels lifted onto the fused points through point_of.
 *   group int32 [F, Hs, Ws]: the group of every sampled element; Hs = ceil(H / stride), Ws likewise;
 *   value: kind 0: uint8, kind 1: uint16, kind 2: int32; [F, H, W], read at (j0 stride, i0 stride) for the sampled
 *     element (f, j0, i0): with stride 1 the shape of group, otherwise the full-resolution image as the sensor wrote it.
 *     F = H = 1, W = T, stride = 1 is the plain one-dimensional form;
 *   n: the number of groups; ignore, has_ignore: a value that does not vote (when has_ignore != 0); fill: the label of a
 *     group without a vote.
 * Element t votes when 0 <= group[t] < n, value[t] >= 0 and value[t] is not the ignored value.  group[t] >= n sets
 * d_words[2] (and does not vote); group[t] < 0 is no vote.  Per group g: total[g] = its votes; among its distinct values
 * the one with the largest count wins, ties go to the smallest value; label[g] = the winner or fill, votes[g] = the
 * winner's count or 0.  Integer counts and one integer maximum of count << 32 | (0xffffffff - value): no result depends
 * on the order of the elements, bit-identical from call to call, with and without `aggregate` (adjacent lanes of a wave
 * that hold the same pair add once, with the length of their run).
 *   slots: the entries (8-byte key group << 32 | value, 4-byte count) of the open-addressing table of the distinct
 *     pairs: a power of two from 64 to 2^30.  With slots >= 2 T the table is never more than half full and probing is
 *     unbounded; with fewer a thread gives up after gf_frames_vote_max_probes() (128) probes and sets d_words[1].
 *     gf_frames_vote_default_slots(T, n): the smallest power of two >= 2 min(T, 8 n), at least 64 (0 for T or n outside
 *     0 .. gf_resample_max_points()).
 *   Outputs label, votes, total int32 [n]; d_words int32 [3] (device): {distinct pairs, overflow, group out of range}.
 *     With overflow clear every vote was counted and the outputs are exact; with it set they are unspecified.
 *   scratch: gf_frames_vote_scratch_bytes(slots, n) (0 for a bad slots or n).
 * T = F Hs Ws or n above gf_resample_max_points(), a negative F, W, H or n, stride < 1, another kind, a bad slots or a
 * NULL pointer are GF_ERR_INVALID_ARG with nothing launched; T == 0 or n == 0 succeeds with nothing launched (and
 * nothing written).  Everything goes on `stream`; nothing is read back. */
int gf_frames_vote_max_probes(void);
int gf_frames_vote_default_slots(long long T, int n);
size_t gf_frames_vote_scratch_bytes(int slots, int n);
int gf_frames_vote(const int32_t* group, const void* value, int kind, int F, int W, int H, int stride, int n, int ignore,
                   int has_ignore, int fill, int slots, int aggregate, void* scratch, int32_t* label, int32_t* votes,
                   int32_t* total, int32_t* d_words, void* stream);

/* ===================================================================================
 * A map that persists between calls (csrc/frames_stream.hip; the statement is frames.FuserHost): the cells and the
 * integer sums of gf_grid_subsample + gf_frames_cell_means, fed one chunk of frames at a time.  A cell keeps the number
 * it got when it was first seen.  The caller owns every piece of state and passes pointers:
 *   keys uint64 [slots], ids int32 [slots], first int32 [slots]: an open-addressing table, slots a power of two from 64
 *     to 2^31.  keys: cx | cy << 21 | cz << 42, all ones = empty; ids: the cell's number, -1 = claimed in the current call
 *     and not numbered yet; first: the lowest point index of the current call that claimed the slot, INT_MAX before;
 *   count int32 [cap], sums int64 [cap, 6] (three coordinate sums in units of 2^-20 m, three colour sums), zero beyond
 *     the cells in use.
 * Integer atomics and minima only; no thread waits for another thread or workgroup; every launch goes on `stream`;
 * nothing is read back.  Every argument is checked before the first launch (GF_ERR_INVALID_ARG, nothing launched).
 * =================================================================================== */

/* Limits, as functions: the probes of a thread in a table of fewer than 2 (M + n) slots (128); the metres from the
 * origin the sums are proven for (4096: q < 2^32, so that the 2^31 - 1 pixels a map takes at most sum below 2^63 and
 * every count fits an int32); that number of pixels; the default table of a map of M cells before a call of T points:
 * the smallest power of two >= max(4 M, T / 8), at least 64 (0 for M or T outside 0 .. 2^31 - 1). */
int gf_frames_map_max_probes(void);
double gf_frames_map_reach(void);
long long gf_frames_map_max_pixels(void);
long long gf_frames_map_default_slots(long long M, long long T);

/* gf_frames_map_rehash (two launches): clears the table of new_slots entries (keys all ones, ids -1, first INT_MAX),
 * then moves every slot of the old table with id >= 0 into it: key and id copied, ids untouched by construction.  A
 * claim without a number (the debris of a failed gf_frames_map_insert) is dropped.  `cells`: the numbered cells of the
 * old table; new_slots >= cells is required: the keys are distinct, so every one finds a free slot and the probing ends
 * (a caller that grows the table keeps two slots per cell and more; a same-size rehash that only cleans may find the
 * table fuller).  old_slots == 0 (old pointers unused) only clears: a new map.  The tables must not overlap. */
int gf_frames_map_rehash(const unsigned long long* old_keys, const int32_t* old_ids, long long old_slots, int cells,
                         unsigned long long* new_keys, int32_t* new_ids, int32_t* new_first, long long new_slots,
                         void* stream);

/* gf_frames_map_insert (one memset, five launches): the cells of n points (the compact xyz fp32 [n, 3] of one
 * gf_frames_backproject call), numbered into a map that holds M cells.
 *   claim   per point, fp32: t = (x - origin) / cell (correctly rounded division), c = floor t, valid when t is finite
 *           and 0 <= c < 2^21 per axis (gf_grid_subsample's rule; an invalid point sets d_words[1]); float64:
 *           !(0 <= (double)x - (double)o < gf_frames_map_reach()) sets d_words[3].  The key is found or claimed (the slot
 *           is read first, the 64-bit CAS issued on an empty slot only); a slot with id < 0 takes an integer atomicMin of
 *           the point index on `first` (read first).  With slots >= 2 (M + n) probing is unbounded; with fewer a thread
 *           gives up after gf_frames_map_max_probes() probes and sets d_words[2].
 *   rank    exclusive scan in point order of "my slot has id < 0 and first == my index", as count / top / emit over
 *           workgroups of `chunk` points (a multiple of 64 in 64 .. 65536, 0 = gf_frames_default_chunk()); top writes
 *           d_words[0] = M + the new cells.
 *   number  emit: a new cell's first point writes id = M + rank; then one more launch: cell_of[i] = ids[slot of i].
 *           Both return without writing when d_words[1], [2] or [3] is set (a wave-uniform branch on a word read).
 * origin: DEVICE fp32 [3].  cell_of int32 [n]; d_words int32 [4] (device): {M', invalid point, table overflow, beyond
 * reach}.  With a flag set, the table holds claims without a number and must be cleaned by gf_frames_map_rehash; no id,
 * count or sum has changed.  scratch: gf_frames_map_insert_scratch_bytes(n, chunk) (0 for a bad n or chunk).
 * n outside 0 .. gf_resample_max_points(), M < 0, M + n > 2^31 - 1, a bad cell, slots or chunk, or a NULL pointer are
 * GF_ERR_INVALID_ARG; n == 0 succeeds with nothing launched. */
size_t gf_frames_map_insert_scratch_bytes(int n, int chunk);
int gf_frames_map_insert(const float* xyz, int n, float cell, const float* origin, unsigned long long* keys, int32_t* ids,
                         int32_t* first, long long slots, int M, int chunk, void* scratch, int32_t* cell_of,
                         int32_t* d_words, void* stream);

/* gf_frames_map_accumulate (one launch): per point, q = (int64)floor(((double)x - (double)o) 1048576.0) per axis and the
 * colour bytes added to sums[cell_of[i]] by 64-bit integer atomic adds, and 1 to count[cell_of[i]] by a 32-bit one.
 * With aggregate != 0 adjacent lanes of one cell add within the wave first (runs numbered by their head lanes from one
 * ballot; a run's count is its length; a wave whose lanes are all alone skips the exchange): the same result.
 *   cell_of int32 [n] in [0, M), as gf_frames_map_insert wrote it; M: the cells of the map after that insert, <= the rows
 *   of count and sums.  A point beyond reach (the insert's float64 comparison, which owns the check: a caller who
 *   honours its word never gets here with one) or a cell outside [0, M) adds nothing and sets *d_flag (device int32;
 *   only ever set, never cleared here).
 * n outside 0 .. gf_resample_max_points(), M < 1 with n > 0, or a NULL pointer are GF_ERR_INVALID_ARG; n == 0 succeeds
 * with nothing launched. */
int gf_frames_map_accumulate(const float* xyz, const unsigned char* rgb, const int32_t* cell_of, int n, int M,
                             const float* origin, int aggregate, int32_t* count, long long* sums, int32_t* d_flag,
                             void* stream);

/* gf_frames_map_means (three launches): gf_frames_cell_means without its summing pass, on the stored count int32 [M]
 * and sums int64 [M, 6]: mean = (float)((double)o + ((double)sum_q / (double)count) (1.0 / 1048576.0)), colour
 * (sum + count / 2) / count; cells with count >= min_obs keep their order and are renumbered densely.
 *   xyz_out fp32 [M, 3], rgb_out uint8 [M, 3], count_out int32 [M]: the first m rows written; new_id int32 [M]: the row
 *   of a kept cell, -1 for a dropped one; d_m int32 [1] (device): m.  Nothing of the map is written.
 *   scratch: gf_frames_map_means_scratch_bytes(M, chunk) (0 for a bad M or chunk).
 * M outside 1 .. 2^31 - 1 - 65536, min_obs < 1, a bad chunk or a NULL pointer are GF_ERR_INVALID_ARG. */
size_t gf_frames_map_means_scratch_bytes(int M, int chunk);
int gf_frames_map_means(const int32_t* count, const long long* sums, int M, const float* origin, int min_obs, int chunk,
                        void* scratch, float* xyz_out, unsigned char* rgb_out, int32_t* count_out, int32_t* new_id,
                        int32_t* d_m, void* stream);

/* gf_frames_map_lookup (one launch): out[t] = table[index[t]] where 0 <= index[t] < len, -1 elsewhere, for T elements
 * (out may be index): a pixel's row to its cell (table = cell_of) and a pixel's cell to its fused point (table =
 * new_id).  An index below -1 or at or above len reads nothing and sets *d_flag (device int32, or NULL; only ever set,
 * never cleared here).  T < 0, len < 0 or a NULL index, table or out are GF_ERR_INVALID_ARG; T == 0 succeeds with
 * nothing launched. */
int gf_frames_map_lookup(const int32_t* index, long long T, const int32_t* table, int len, int32_t* out, int32_t* d_flag,
                         void* stream);

/* ===================================================================================
 * Votes that persist between calls (csrc/frames_vote_stream.hip; the statement is frames.VoterHost): gf_frames_vote's
 * table of the distinct (group, value) pairs, kept by the caller and fed one chunk of elements at a time.  The caller
 * owns the state and passes pointers:
 *   keys uint64 [slots]: group << 32 | value, all ones = empty; cnt uint32 [slots]: the pair's votes.  slots: a power
 *     of two from 64 to 2^31 (a slot is recorded as a non-negative int32).  A claimed key with cnt == 0 is the debris of
 *     a failed add: absent for every reader, dropped by the rehash.
 * Integer atomics and one integer maximum only; no thread waits for another thread or workgroup; every launch goes on
 * `stream`; nothing is read back.  Every argument is checked before the first launch (GF_ERR_INVALID_ARG, nothing
 * launched).
 * =================================================================================== */

/* Limits, as functions: the probes of a thread in a table of fewer than 2 (P + T) slots (128); the elements a table
 * takes in all, counted as offered (2^31 - 1: every count and total fits an int32); the default table of P stored pairs
 * before a call of T elements: the smallest power of two >= max(4 P, T / 8), at least 64 (0 for P or T outside
 * 0 .. 2^31 - 1); the scratch of an add of T elements (8 bytes per element; 0 for T outside 0 .. 2^29) and of a pick
 * over n groups (12 bytes per group; 0 for n outside 0 .. 2^31 - 1). */
int gf_frames_votes_max_probes(void);
long long gf_frames_votes_max_elements(void);
long long gf_frames_votes_default_slots(long long P, long long T);
size_t gf_frames_votes_add_scratch_bytes(long long T);
size_t gf_frames_votes_pick_scratch_bytes(long long n);

/* gf_frames_votes_add (one memset, two launches) = gf_frames_votes_claim, then gf_frames_votes_commit.  group, value,
 * kind, F, W, H, stride, ignore, has_ignore: gf_frames_vote's, read in the same way; element t votes when
 * group[t] >= 0, value[t] >= 0 and value[t] is not the ignored value (no upper bound on the group here: the pick has it).
 *   claim   the two words zeroed; one thread per sampled element builds the key; with aggregate != 0 only the head lane
 *           of a run of equal keys among adjacent lanes goes on, with the run's length.  The key is found or claimed
 *           (the slot read first, the 64-bit CAS issued on an empty slot only); the head's slot and its add go to
 *           scratch; no count changes.  d_words[0]: the keys claimed (the new pairs), one atomic per workgroup.  With
 *           slots >= 2 (pairs + T) probing is unbounded; with fewer a thread gives up after gf_frames_votes_max_probes()
 *           probes and sets d_words[1].
 *   commit  returns without writing when d_words[1] is set (a uniform branch on a word read); otherwise every recorded
 *           head adds its run length to cnt[slot].
 * pairs: the occupied slots of the table before the call (the stored pairs: the caller cleans debris by a rehash).
 * d_words int32 [2] (device): {new pairs, overflow}.  With overflow set no count has changed and the table holds
 * debris.  scratch: gf_frames_votes_add_scratch_bytes(T), the same buffer for claim and commit.
 * T = F Hs Ws above gf_resample_max_points(), a negative F, W or H, stride < 1, another kind, a bad slots, pairs outside
 * 0 .. slots, pairs + T above gf_frames_votes_max_elements() or a NULL pointer are GF_ERR_INVALID_ARG; T == 0 succeeds
 * with nothing launched (and nothing written). */
int gf_frames_votes_claim(const int32_t* group, const void* value, int kind, int F, int W, int H, int stride, int ignore,
                          int has_ignore, unsigned long long* keys, long long slots, long long pairs, int aggregate,
                          void* scratch, int32_t* d_words, void* stream);
int gf_frames_votes_commit(const void* scratch, long long T, uint32_t* cnt, long long slots, const int32_t* d_words,
                           void* stream);
int gf_frames_votes_add(const int32_t* group, const void* value, int kind, int F, int W, int H, int stride, int ignore,
                        int has_ignore, unsigned long long* keys, uint32_t* cnt, long long slots, long long pairs,
                        int aggregate, void* scratch, int32_t* d_words, void* stream);

/* gf_frames_votes_rehash (two launches): clears the table of new_slots entries (keys all ones, cnt 0), then moves every
 * slot of the old table with cnt > 0 into it, key and count copied; debris is dropped.  `pairs`: the stored pairs of
 * the old table; new_slots >= pairs is required: the keys are distinct, so every one finds a free slot and the probing
 * ends (a caller that grows the table keeps two slots per pair and more; a same-size rehash that only cleans may find
 * the table fuller).  old_slots == 0 (old pointers unused) only clears: a new table.  The tables must not overlap. */
int gf_frames_votes_rehash(const unsigned long long* old_keys, const uint32_t* old_cnt, long long old_slots, long long pairs,
                           unsigned long long* new_keys, uint32_t* new_cnt, long long new_slots, void* stream);

/* gf_frames_votes_pick (one memset, two launches): gf_frames_vote's second half over the stored table, per group
 * 0 <= g < n: total[g] = its votes; the value with the largest count wins, ties go to the smallest value (one 64-bit
 * integer maximum of count << 32 | (0xffffffff - value)); label[g] = the winner or fill, votes[g] = its count or 0.
 * Slots with cnt == 0 are skipped; a stored group >= n sets d_words[1] and writes nothing.  At most 1024 workgroups
 * stride over the table.  Outputs label, votes, total int32 [n]; d_words int32 [2] (device): {stored pairs, group out of
 * range}.  scratch: gf_frames_votes_pick_scratch_bytes(n).  Nothing of the table is written.  A bad slots, n outside
 * 0 .. 2^31 - 1 or a NULL pointer are GF_ERR_INVALID_ARG; n == 0 succeeds with nothing launched (and nothing written). */
int gf_frames_votes_pick(const unsigned long long* keys, const uint32_t* cnt, long long slots, long long n, int fill,
                         void* scratch, int32_t* label, int32_t* votes, int32_t* total, int32_t* d_words, void* stream);

/* ===================================================================================
 * frames_track.hip -- instance ids that persist over successive snapshots.  One update of a
 * tracker keyed by the persistent cell numbers of a map (gf_frames_map_*): this run's rows are matched to the tracks so
 * far by exact mask IoU over the cells both saw, one to one.  The statement is frames.TrackerHost.  The state belongs
 * to the caller: track_of int32 [map_cap] (the track of every cell, -1 for none and from M on) and table int32
 * [gf_frames_track_columns(), table_cap], one column per track, the rows {cls, score (the bits of a float), born,
 * seen, hits, misses, size, alive}.  A retired track has alive 0 and size 0; cells that still name it read as none.
 * Integer atomics only; no thread waits for another thread or workgroup; every launch goes on `stream`; nothing is
 * read back.  Every argument is checked before the first launch (GF_ERR_INVALID_ARG, nothing launched).
 * =================================================================================== */

/* Limits, as functions: the rows of one update (4096); the probes of a thread in a pair table of fewer than 2 m slots
 * (128); the tracks of a table (2^30); the rows of the table (8) and the words of d_words (16); the default pair table
 * for p rows and `live` alive tracks: the smallest power of two >= 8 (p + live), at least 64 (0 for an argument out of
 * range); the scratch of an update (0 for an argument out of range: m outside 0 .. gf_resample_max_points(), p above
 * the rows, T above the tracks, slots no power of two from 64 to 2^30). */
int gf_frames_track_max_rows(void);
int gf_frames_track_max_probes(void);
long long gf_frames_track_max_tracks(void);
int gf_frames_track_columns(void);
int gf_frames_track_words(void);
long long gf_frames_track_default_slots(long long p, long long live);
size_t gf_frames_track_scratch_bytes(long long m, long long p, long long T, long long slots);

/* gf_frames_track_update (three memsets, five launches).  Point i of the snapshot is cell cells[i] (int32 [m], >= 0 and
 * strictly ascending) and belongs to row owner[i] (int32 [m], -1 .. p - 1) of this run; cls int32 [p], score fp32 [p],
 * keep uint8 [p] describe the rows.  M: the cells of the map before the update, T: the tracks.
 *   count    one thread per point: r = owner when >= 0 and kept, t = track_of[cell] when the cell is < M and the track
 *            alive (t is kept in scratch); a[r], b[t] and the pair count n[r, t] by integer adds, the pair in an
 *            open-addressing table of `slots` entries (64-bit CAS on an empty slot only).  With aggregate != 0 a run of
 *            equal (r, t) among adjacent lanes adds once.  With slots >= 2 m probing is unbounded; with fewer a thread
 *            gives up after gf_frames_track_max_probes() probes.  Raises d_words[0] (cells negative or not ascending),
 *            [1] (owner out of range), [2] (pair table overflow), [6] (a cell >= map_cap); [7] = cells[m - 1].
 *   best     per stored pair (same cls as the track's when same_class): a CAS loop on the best slot of its row and of
 *            its track under the total order (larger IoU n / (a + b - n), by int64 cross-products; then the smaller
 *            index), whose maximum is unique.
 *   match    one workgroup: row and track match when each is the other's best and (double)n >= iou * (double)union.
 *            track[r] = the matched track; else, for a kept row with a[r] >= min_points, a new id T, T + 1, .. in
 *            ascending r (table_cap >= T + p is required); else -1.  Then the table: a matched track gets hits + 1,
 *            misses 0, seen = update and, when score[r] >= its score, the row's score and cls; a new one born = seen =
 *            update, hits 1; an alive unmatched track with b[t] > 0 gets misses + 1 and retires above max_misses; a
 *            track with b[t] == 0 is untouched.
 *   apply    one thread per point, tid = track[r]: tid >= 0 writes track_of[cell] = tid; else a cell whose old track
 *            matched or retired in this update is set to -1; else it is unchanged.  ids[i] = the cell's track after
 *            that (-1 for none).  size follows by integer adds.
 *   finish   an alive track with size 0 retires; retired int32 [T] = 1 for every track retired by this update;
 *            d_words[3] = new tracks, [4] = retired tracks, [5] = stored pairs.
 * With one of d_words[0], [1], [2], [6] raised nothing but scratch and d_words has been written: track_of, table, ids,
 * track and retired are as before.  d_words int32 [gf_frames_track_words()] (device).  scratch:
 * gf_frames_track_scratch_bytes(m, p, T, slots).  m, p, T or slots out of range, M above map_cap, T + p above table_cap,
 * iou outside 0 .. 1, max_misses < 0, min_points < 1, update < 0 or a NULL pointer are GF_ERR_INVALID_ARG. */
int gf_frames_track_update(const int32_t* cells, const int32_t* owner, long long m, const int32_t* cls, const float* score,
                           const unsigned char* keep, int p, int32_t* track_of, long long M, long long map_cap,
                           int32_t* table, long long T, long long table_cap, double iou, int max_misses, int min_points,
                           int same_class, int update, long long slots, int aggregate, void* scratch, int32_t* ids,
                           int32_t* track, int32_t* retired, int32_t* d_words, void* stream);

/* ===================================================================================
 * frames_carve.hip -- what posed depth frames see of world points, and the free-space score of a map's cells
 * (DESIGN.md section 30).  The statement is frames.visibility_host / frames.CarverHost.  The state (seen, free, score,
 * int32 per cell) belongs to the caller.  No scratch; no thread waits for another thread or workgroup; every launch
 * goes on `stream`; nothing is read back.  Every argument is checked before the first launch (GF_ERR_INVALID_ARG,
 * nothing launched).
 * =================================================================================== */

/* Limits, as functions: the frame records a workgroup of the per-point shape stages in LDS at a time (16), the threads
 * of a workgroup (256), the points of one call (gf_resample_max_points()), the launch shapes (2). */
int gf_frames_carve_stage_frames(void);
int gf_frames_carve_threads(void);
int gf_frames_carve_max_points(void);
int gf_frames_visibility_variants(void);

/* gf_frames_visibility.  xyz fp32 [n, 3] world points; depth uint16 (dtype 0) or fp32 (dtype 1) [F, H, W], a value d
 * is d / depth_shift metres; table fp32 [F, gf_frames_record_floats()] (only {fx, fy, cx, cy} are read); inv fp32
 * [F, 12]: per frame the inverse of the record's 3 x 3 block, row-major, then its translation t
 * (frames.inverse_records).  One probe = point X in frame f, float32, every operation rounded on its own:
 *   d = X - t;  c_a = ((inv[a,0] d0 + inv[a,1] d1) + inv[a,2] d2);  zc = c_2
 *   !(zc >= near)                                        -> 0 outside
 *   u = ((c_0 fx) / zc) + cx, v likewise; i = floor u, j = floor v;  !(0 <= i < W && 0 <= j < H) as floats -> 0 outside
 *   z = depth[f, j, i] / depth_shift, read only now;  !(near <= z <= far), or with edge > 0 an in-image 4-neighbour zn
 *   with near <= zn <= far and |zn - z| > edge z         -> 1 unknown
 *   tol = (rel z) + band;  zc < z - tol -> 4 free;  zc > z + tol -> 2 occluded;  else 3 seen
 * out int32 [3, n]: per point the probes over the F frames that were seen, free, occluded.  codes uint8 [F, n] or NULL:
 * the class of every probe.  seen, free, score int32 [n], all three or all NULL: seen += s and free += f (saturating
 * at 2^31 - 1), score = min(ceil, max(floor, score + hit s - miss f)), in 64-bit integers, one clamp per call.
 * variant 0: one launch, a thread per point loops over the frames (records staged in LDS, counts in registers, plain
 * stores).  variant 1: a memset of out, a thread per (frame, point) with one integer atomicAdd per probe that is not
 * outside or unknown, and a finishing launch for the state.  The same bits either way.  n == 0 succeeds with nothing
 * launched.  n, F, H, W, dtype or variant out of range, depth_shift not positive and finite, near or far NaN, edge,
 * band or rel negative or not finite, hit or miss negative, floor > ceil, some but not all of the state pointers, state
 * pointers that coincide, or a NULL xyz, depth, table, inv or out are GF_ERR_INVALID_ARG. */
int gf_frames_visibility(const float* xyz, int n, const void* depth, int dtype, int F, int H, int W, float depth_shift,
                         const float* table, const float* inv, float near, float far, float edge, float band, float rel,
                         int32_t* out, unsigned char* codes, int32_t* seen, int32_t* free, int32_t* score, int hit, int miss,
                         int floor, int ceil, int variant, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GEOFORMER_HIP_H */
