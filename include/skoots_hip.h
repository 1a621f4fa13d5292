/* skoots_hip.h -- C ABI of libskoots_hip.so (MI355X / gfx950).
 *
 * The reference (buswinka/skoots) has no FFI: its hot path sits behind the Python
 * function skoots.lib.eval.eval() and the library functions it calls.  Each entry
 * point below names the reference code it replaces (file:line, relative to the
 * reference tree).  The Python host mirror of the reference interface lives in
 * skoots_amd/lib/ and binds these symbols with ctypes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host;
 *   - volumes are C-contiguous (X, Y, Z) with Z fastest, exactly the reference's
 *     (C, X, Y, Z) tensors per channel;
 *   - `stream` is a hipStream_t passed as void*; all work is stream-ordered, no
 *     entry point synchronises unless its comment says so;
 *   - no entry point allocates device memory: callers pass workspaces;
 *   - return value: SK_OK, or a negative code; sk_last_error() gives the text.
 */
#ifndef SKOOTS_HIP_H
#define SKOOTS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SK_OK 0
#define SK_ERR_ARG (-1)
#define SK_ERR_HIP (-2)
#define SK_ERR_CAPACITY (-3)

#define SK_F16 0
#define SK_F32 1
#define SK_I16 2
#define SK_I32 3
#define SK_U8 4
#define SK_U16 5 /* sk_pool_volume and sk_resample_volume */

const char* sk_last_error(void);
int sk_abi_version(void);

/* ------------------------------------------------------------------------ *
 * Stage 3: offset following + label assignment
 * ------------------------------------------------------------------------ */

/* Planar (3, X, Y, Z) fp16 vectors -> interleaved (X, Y, Z, 4) fp16 (4th lane 0).
 * Internal staging layout for the follow kernel: one 8-byte load per hop instead
 * of three cache lines.  No reference counterpart (layout choice). */
int sk_vec_interleave(const void* vec_planar, void* vec4, int64_t nvox, void* stream);

/* Inverse of sk_vec_interleave: (X,Y,Z,4) fp16 -> planar (3,X,Y,Z) fp16, the layout of
 * the reference's `vectors` zarr array (skoots/lib/eval.py:103). */
int sk_vec_deinterleave(const void* vec4, void* vec_planar, int64_t nvox, void* stream);

/* skoots.lib.vector_to_embedding.vector_to_embedding (vector_to_embedding.py:79-174)
 * on one crop: vec (3, w, h, d) planar, fp16 or fp32 (vec_dtype SK_F16/SK_F32);
 * embed (3, w, h, d) fp32.  step_scale_host[(n)*3]: row 0 = float(scale), row i>=1 =
 * float(decay^i) * float(scale) (fp32 product), prepared by the host mirror. */
int sk_vector_to_embedding(const void* vec, int vec_dtype, float* embed, int w, int h, int d,
                           const float* step_scale_host, int n_iter, void* stream);

/* skoots.lib.skeleton.index_skeleton_by_embed (skeleton.py:656-695):
 * out[i] = labels[round/clamp(embed[:, i])]; labels (LX, LY, LZ) int16 or int32,
 * embed (3, n) fp32, out (n) int32. */
int sk_index_skeleton_by_embed(const void* labels, int label_dtype, int lx, int ly, int lz,
                               const float* embed, int64_t n, int32_t* out, void* stream);

/* Fused stage 3 (eval.py:245-284): for every voxel of planes [z_lo, z_hi), find the
 * stage-3 crop that writes it last (owner tables built by the host from the
 * reference's crop generator, cropper.py:97-144), run the N-step follow inside that
 * crop's window with the reference's arithmetic, add the crop origin, gather the
 * label.  (X,Y,Z) is the GLOBAL volume; labels is the full (X,Y,Z) int16|int32 volume.
 * vec4 ((.,.,.,4) fp16) is an array over the z-window [win_lo, win_hi): shape
 * (X, Y, win_hi-win_lo, 4) -- the whole volume on one GPU, slab + halo when Z-sharded; the
 * window must contain every crop that owns a written plane.  out (int32) holds exactly
 * the written planes: shape (X, Y, z_hi-z_lo).  owner_{x,y,z}:
 * int32[X|Y|Z] origin of the owning crop per GLOBAL coordinate, or -1 (voxel stays 0). */
int sk_follow_assign(const void* vec4, const void* labels, int label_dtype, int32_t* out,
                     int X, int Y, int Z, int win_lo, int win_hi, const int32_t* owner_x,
                     const int32_t* owner_y, const int32_t* owner_z, int eff_w, int eff_h,
                     int eff_d, const float* step_scale_host, int n_iter, int z_lo, int z_hi,
                     void* stream);

/* ------------------------------------------------------------------------ *
 * Stage 1 tail: gate + dilate + threshold + interior scatter
 * ------------------------------------------------------------------------ */

/* eval.py:145-176 for a batch of n_tiles (<= 16) tiles in one launch.  out5 holds the 5-channel
 * network outputs, fp16 or fp32 (thresholds follow torch's scalar casting for that dtype); tile i
 * starts at element offset tile_offsets_host[i] and is addressed with the element strides
 * (stride_c, stride_x, stride_y, 1), extent (w, h, d) -- a (B,5,w,h,d) batch or views into a
 * larger (5,X,Y,Z) array alike.  For tile i the tile-local box [box_lo_host[3i..], box_hi_host[3i..])
 * (the tile interior, or the part of it this tile writes LAST in the reference's scatter
 * order, so that tiles can be scattered in any order / concurrently) is written into the
 * volume arrays at origins_host[3i..] + box: vec4 (X,Y,Z,4) fp16 and/or vec_planar (3,X,Y,Z)
 * fp16 (either may be NULL), skeleton (X,Y,Z) uint8 in {0,1}.  Dilation = 3x3x3 max then 3x3x1
 * max twice, zero padded at the tile faces (morphology.py:155-199). */
int sk_gate_dilate_scatter(const void* out5, int out_dtype, int n_tiles,
                           const int64_t* tile_offsets_host, int64_t stride_c, int64_t stride_x,
                           int64_t stride_y, int w, int h, int d, const int* origins_host,
                           const int* box_lo_host, const int* box_hi_host, void* vec4,
                           void* vec_planar, uint8_t* skeleton, int X, int Y, int Z,
                           float prob_thr, float skel_thr, void* stream);

/* skoots.lib.morphology.binary_dilation / binary_dilation_2d (morphology.py:155-199)
 * as library functions on a (w,h,d) fp32 map: max over a (2rx+1,2ry+1,2rz+1) window,
 * zero padded. */
int sk_max_filter3d(const float* in, float* out, int w, int h, int d, int rx, int ry, int rz,
                    void* stream);

/* ------------------------------------------------------------------------ *
 * Stage 2: skeleton labelling (skoots.lib.flood_fill.efficient_flood_fill,
 * flood_fill.py:13-122)
 * ------------------------------------------------------------------------ */

/* Bytes of workspace sk_ccl_crop needs for a crop of n voxels. */
size_t sk_ccl_workspace_bytes(int64_t crop_voxels);

/* flood_all (flood_fill.py:125-140) for one crop of the flood grid: 6-connected
 * labelling of src>0 inside the box [x0,x0+w) x [y0,y0+h) x [z0,z0+d) of the
 * (X,Y,Z) uint8 volume; components are numbered in raster order of their first
 * voxel (scipy.ndimage.label order) starting at state[0]+2, written to the int32
 * labels volume (same box).  state (device int32[4]): [0] running max id (init 1,
 * becomes 0 after an empty crop, exactly as the reference), [1] components in this
 * crop, [2] total components so far, [3] scratch. */
int sk_ccl_crop(const uint8_t* src, int32_t* labels, int X, int Y, int Z,
                int x0, int y0, int z0, int w, int h, int d,
                void* workspace, size_t workspace_bytes, int32_t* state, void* stream);

/* Seam scan (replaces get_adjacent_labels, flood_fill.py:237-261, with true
 * adjacency): for plane `v` of `axis` (0=x,1=y,2=z) emit the pairs
 * (labels[plane v], labels[plane v-1]) of face-adjacent nonzero voxels into
 * pairs (int32[2*capacity]); *count (device int32) is advanced atomically.
 * Duplicates are possible; the host sorts and uniques. */
int sk_seam_pairs(const int32_t* labels, int X, int Y, int Z, int axis, int v,
                  int32_t* pairs, int32_t* count, int capacity, void* stream);

/* HOST function (no GPU work): collision graph + depth-first components + "last id
 * represents the component" (flood_fill.py:82-105).  pairs_host: n pairs in the
 * reference's emission order.  Writes up to capacity (to_replace, replace_with)
 * entries; returns the number written or a negative code. */
int sk_seam_components_host(const int32_t* pairs_host, int n_pairs, int32_t* to_replace_host,
                            int32_t* replace_with_host, int capacity);

/* Device-side seam merge of the Z-sharded labelling (no reference counterpart: the reference is single device; the
 * partition is that of flood_fill.py:82-117).  Together they let a rank go from its local labelling to the merged global
 * ids without reading anything back to the host between the collectives:
 *   sk_compact_nonzero: flat positions of the non-zero labels into positions[capacity] (any order); *count (device,
 *     pre-zeroed) counts ALL of them, also past the capacity -- the caller detects an overflow from it later.
 *   sk_seam_union: meta (ranks, row_stride) int32 rows [components, pairs, -, - | pairs in rank-local ids ...] as
 *     all-gathered; offsets (ranks + 1) int64 exclusive prefix sums of the component counts (device); lut
 *     (lut_size, pre-filled with the identity) <- smallest global id of every id's component.  One workgroup.
 *   sk_relabel_lut_offset: labels[i] = lut[labels[i] + *offset] for labels[i] > 0 (offset: device scalar). */
int sk_compact_nonzero(const int32_t* labels, int64_t n, int64_t* positions, uint64_t* count, int64_t capacity, void* stream);
int sk_seam_union(const int32_t* meta, int ranks, int row_stride, int pair_capacity, const int64_t* offsets, int32_t* lut,
                  int64_t lut_size, void* stream);
int sk_relabel_lut_offset(int32_t* labels, int64_t n, const int32_t* lut, int64_t lut_size, const int64_t* offset, void* stream);

/* labels[i] = lut[labels[i]] for 0 <= labels[i] < lut_size (in place; flood_fill.py:177-234). */
int sk_relabel_lut(int32_t* labels, int64_t n, const int32_t* lut, int lut_size, void* stream);

/* ------------------------------------------------------------------------ *
 * Renumber (fastremap.renumber call, eval.py:304-306)
 * ------------------------------------------------------------------------ */

size_t sk_renumber_workspace_bytes(int64_t n, int max_label);

/* Distributed renumber, step 1: first[v] = min over this array of the GLOBAL C-order
 * index of label v (atomicMin into a table the caller pre-filled with 0xFFFFFFFF).
 * labels is the (X, Y, zl) slab at planes [z_off, z_off+zl) of a volume with Zg planes;
 * the ranks then all-reduce(MIN) the table, rank it and apply sk_relabel_lut. */
int sk_first_seen(const int32_t* labels, int X, int Y, int zl, int z_off, int Zg, int max_label,
                  uint32_t* first, void* stream);

/* Relabel to 1..K by first appearance in C order, 0 preserved, in place.
 * labels int32 (n), values in [0, max_label].  *n_labels (device int32) = K. */
int sk_renumber(int32_t* labels, int64_t n, int max_label, void* workspace,
                size_t workspace_bytes, int32_t* n_labels, void* stream);

/* ------------------------------------------------------------------------ *
 * Stage 1 body: U-Net layers (the network the reference builds with
 * cfg_to_bism_model, skoots/lib/utils.py:17-107, and runs at eval.py:117-143).
 * Graph and parity reference: oracle/unet_spec.py.  Activations are channels-last
 * fp16 (B, X, Y, Z, C).  A conv writes RAW outputs (bias added) plus per-block
 * GroupNorm partial sums; sk_groupnorm_finalize + sk_groupnorm_silu then normalise
 * and activate the tensor in place, so every conv input is already activated.
 * ------------------------------------------------------------------------ */

typedef struct sk_conv_src {
    const void* data;    /* (B, sx, sy, sz, c) fp16 channels-last                            */
    const float* affine; /* NULL: data is activated.  (B, 2, c) fp32: data is a RAW conv output, */
                         /* silu(a*x + b) is applied while it is staged / loaded              */
    int c;               /* channels of this source (multiple of 32 for ksize 3)            */
    int upsample;        /* 1: source is half resolution, read at (x>>1, y>>1, z>>1)        */
} sk_conv_src;

/* Implicit-GEMM 3-D convolution on the matrix cores (v_mfma_f32_32x32x16_f16).
 * ksize 3: stride 1, zero pad 1, input = channel concat of n_src (<= 2) sources, the
 * second optionally nearest-upsampled x2 (torch.cat([skip, interpolate(x)]) never
 * materialised).  ksize 2: stride 2, no pad.  ksize 1: pointwise.  weight: packed by
 * sk_conv3d_pack_weight_host; bias (cout) fp32; out (B, ox, oy, oz, cout) fp16 raw.
 * gn_partial: (B, sk_conv3d_num_blocks, cout/4, 2) fp32 per-block (sum, sumsq) per channel quad, or NULL.  What is
 * summed: ksize 3 (conv3_px_kernel, conv3_m16_kernel, conv3_kernel) the values as STORED, i.e. the results rounded to 16
 * bits -- the statistics of the tensor the GroupNorm pass reads; ksize 1 / 2 (gather_gemm_kernel, pointwise_lds_kernel, down2_act_kernel) the
 * fp32 accumulators; sk_conv3d_split, sk_conv3d_box_split, sk_conv3d_mix8 and the split / mix8 down convs the fp32
 * accumulators for every ksize (tests/test_hip_conv16_exact.py tells the two apart).  zero_page: 4 KiB; bytes [0, 1024) must
 * be zero and stay zero (source of the halo / padding lanes of the LDS-DMA), bytes
 * [2048, 3072) are write-only scratch for the ksize-3 kernel's masked store lanes.  Required for ksize 3 and for
 * the LDS-staged ksize-2 kernel ((cin, cout) = (32, 64) | (64, 128)).  A RAW source (affine != NULL) is activated
 * while it is staged / loaded: ksize 3 in LDS by the staging lanes, ksize 2 and 1 on load. */
int sk_conv3d(const sk_conv_src* srcs, int n_src, const void* weight, const float* bias,
              void* out, int B, int ox, int oy, int oz, int cout, int ksize,
              float* gn_partial, void* zero_page, void* stream);

/* sk_conv3d with a STORE BOX (round 3): store_box = {lo_x, lo_y, lo_z, hi_x, hi_y, hi_z} (host, tile-local, half open)
 * or NULL.  The convolution and its GroupNorm partial sums cover the whole tile as always; output voxels outside the
 * box may be left unwritten -- for a tensor whose only reader looks at a box of it (the last block's conv: the heads
 * evaluate the scatter's box, 28 % of a 300x300x20 tile).  Honoured by the COUT-32 kernels (conv3_px_kernel, and since
 * round 4 conv3_m16_kernel); wider layers store the whole tile, which satisfies the contract too. */
int sk_conv3d_box(const sk_conv_src* srcs, int n_src, const void* weight, const float* bias, void* out,
                  int B, int ox, int oy, int oz, int cout, int ksize, float* gn_partial,
                  void* zero_page, const int* store_box, void* stream);

/* sk_conv3d_box for the split precision (round 4; tensors and weight as sk_conv3d_split): the last block's conv of the
 * precision="split" network stores only the heads' box -- 28 % of the 14.7 GB a 64-tile batch of [hi | lo] lines is. */
int sk_conv3d_box_split(const sk_conv_src* srcs, int n_src, const void* weight, const float* bias, void* out,
                        int B, int ox, int oy, int oz, int cout, int ksize, float* gn_partial,
                        void* zero_page, const int* store_box, void* stream);

/* 2x2x2 stride-2 down conv with the GroupNorm + SiLU of its INPUT folded in (the fused form of north_star's
 * "fused GroupNorm+SiLU" for the two skip tensors): in_raw (B, 2ox, 2oy, 2oz, cin) fp16 is the RAW output of the
 * producing conv, affine (B, 2, cin) its GroupNorm coefficients.  The kernel stages the input through LDS, activates
 * it there (bit-identical to sk_groupnorm_silu), WRITES THE ACTIVATED VALUES BACK to in_raw -- afterwards the
 * tensor is activated, as its other consumer (the decoder's skip conv) needs it -- and computes the conv from LDS.
 * (cin, cout) = (32, 64) | (64, 128); weight / bias / out / gn_partial / zero_page as sk_conv3d with ksize 2
 * (which runs the same kernel without activation when its source has affine == NULL). */
int sk_conv3d_down_act(void* in_raw, const float* affine, const void* weight, const float* bias, void* out,
                       int B, int ox, int oy, int oz, int cin, int cout, float* gn_partial,
                       void* zero_page, void* stream);

/* sk_conv3d_down_act for the split precision (round 4): in_raw (B, 2ox, 2oy, 2oz, 2 cin) and out (B, ox, oy, oz, 2 cout)
 * hold [hi | lo] fp16 pairs per voxel line, weight = sk_conv3d_pack_weight_split_host(ksize 2).  Activates hi + lo with
 * the arithmetic of sk_groupnorm_silu_split (bit-identical), writes the pair back, three MFMA products per K step.
 * Same partial-sum rows as sk_conv3d_num_blocks(.., ksize 2) reports. */
int sk_conv3d_down_act_split(void* in_raw, const float* affine, const void* weight, const float* bias, void* out,
                             int B, int ox, int oy, int oz, int cin, int cout, float* gn_partial,
                             void* zero_page, void* stream);

/* sk_conv3d_down_act_split for precision "mix8": the same conv, but the activated input is written back as a mix8 line
 * [hi fp16 (cin) | per 32-channel chunk: x8 (32 bytes) | lo8 (32 bytes)] (sk_groupnorm_silu_mix8's format) -- for a skip
 * tensor whose other reader is sk_conv3d_upfold_mix8. */
int sk_conv3d_down_act_mix8(void* in_raw, const float* affine, const void* weight, const float* bias, void* out,
                            int B, int ox, int oy, int oz, int cin, int cout, float* gn_partial,
                            void* zero_page, void* stream);

/* Decoder conv over cat([skip, nearest-upsample x2 (up)]) with the upsample FOLDED INTO THE WEIGHTS of the upsampled
 * channels (csrc/conv3d_up.hip): 3x3x3, stride 1, zero pad 1, the same function as sk_conv3d(ksize 3) with sources
 * {skip, up (upsample = 1)} -- the first conv of each decoder level (oracle/unet_spec.py; skoots/lib/utils.py:17-107)
 * -- at 8 instead of 27 tap-chunks for the upsampled channels: an output voxel of parity p along an axis reads
 * U[x-1], U[x], U[x+1] = two distinct voxels of the low-resolution tensor, so per parity class (px, py, pz) the 27 taps
 * collapse to 2x2x2 taps whose weights are sums of the kernel's (formed on the host in fp32, rounded to fp16 once:
 * results agree with sk_conv3d to the fp16 rounding of those sums, exactly on integer-valued weights).
 * skip (B, ox, oy, oz, c_skip), up (B, ox/2, oy/2, oz/2, c_up): fp16, ACTIVATED; weight: sk_conv3d_pack_weight_upfold_host;
 * out (B, ox, oy, oz, cout) fp16 raw; gn_partial (B, sk_conv3d_upfold_num_blocks, cout/4, 2) or NULL.  cout = 32 | 64
 * (64: two launches of 32 output channels each).
 * sk_conv3d_upfold_num_blocks < 0: the geometry is not covered (an odd extent, oz/2 > 24) -- use sk_conv3d. */
int sk_conv3d_upfold(const void* skip, int c_skip, const void* up, int c_up, const void* weight,
                     const float* bias, void* out, int B, int ox, int oy, int oz, int cout,
                     float* gn_partial, void* stream);
int sk_conv3d_upfold_num_blocks(int ox, int oy, int oz, int cout);
/* HOST: torch-layout weight (cout, c_skip + c_up, 3, 3, 3) fp32 -> fragments of sk_conv3d_upfold.  Bytes needed / written. */
int64_t sk_conv3d_pack_weight_upfold_host(const float* w_host, int cout, int c_skip, int c_up, void* dst_host);
/* The same on split tensors (precision "split": every voxel line [hi (C) | lo (C)] fp16, value = hi + lo; out the same with
 * cout): three MFMA phases per logical chunk as sk_conv3d_split; the folded weights are summed in double and split afterwards. */
int sk_conv3d_upfold_split(const void* skip, int c_skip, const void* up, int c_up, const void* weight,
                           const float* bias, void* out, int B, int ox, int oy, int oz, int cout,
                           float* gn_partial, void* stream);
int64_t sk_conv3d_pack_weight_upfold_split_host(const float* w_host, int cout, int c_skip, int c_up, void* dst_host);
/* The same for precision "mix8": skip and up hold mix8 lines (sk_groupnorm_silu_mix8 / sk_conv3d_down_act_mix8), out is a RAW
 * split pair; per logical chunk one fp16 phase (hi halves x w_hi) and one block-scaled fp8 phase (K = 128 = two taps x
 * {w_lo . x8, w . lo8}; the folded weights are summed in double, then split into fp16 hi and the fp8 images).
 * weight + weight_scale_exp: sk_conv3d_pack_weight_upfold_mix8_host. */
int sk_conv3d_upfold_mix8(const void* skip, int c_skip, const void* up, int c_up, const void* weight, int weight_scale_exp,
                          const float* bias, void* out, int B, int ox, int oy, int oz, int cout,
                          float* gn_partial, void* stream);
int64_t sk_conv3d_pack_weight_upfold_mix8_host(const float* w_host, int cout, int c_skip, int c_up, void* dst_host,
                                               int* scale_exp);

/* Rows of gn_partial per batch item that sk_conv3d writes for this output shape. */
int sk_conv3d_num_blocks(int B, int ox, int oy, int oz, int cout, int ksize);

/* HOST (ABI 24; no GPU needed): which kernel a conv launch runs, and with what geometry -- the answer of the one function
 * the launches themselves ask.  family: SK_CONV_ENTRY for sk_conv3d, _box, _split, _box_split and _mix8, SK_CONV_ENTRY_DOWN_ACT
 * for sk_conv3d_down_act, _split and _mix8 (srcs[0].c = cin, ksize 2).  Of srcs only c, upsample and affine != NULL are read.
 * SK_ERR_ARG, with the launch's own message, for a shape the launch refuses.  name: the instantiation, e.g. "px",
 * "m16<4,3,2>", "conv3<64,3,split>", "down2<128,64>", "gather<32,2>", "pointwise<32,64>".  The plan fields are those of the
 * 3x3x3 kernels (zero for ksize 1 / 2); grid workgroups of 256 threads with lds bytes of dynamic LDS. */
enum { SK_CONV_FP16 = 0, SK_CONV_SPLIT = 1, SK_CONV_MIX8 = 2 };
enum { SK_CONV_ENTRY = 0, SK_CONV_ENTRY_DOWN_ACT = 1 };
typedef struct sk_conv_route {
    char name[32];
    int mode, tz, nzc, pitch, nposp, npatch, xc, nxc, xs;
    int64_t plan_lds;     /* the plane ring of the plan; lds adds what the kernel keeps behind it */
    int num_blocks;       /* rows of gn_partial per batch item: sk_conv3d_num_blocks */
    int64_t grid, lds;
} sk_conv_route;
int sk_conv3d_route(int family, int precision, const sk_conv_src* srcs, int n_src, int B, int ox, int oy, int oz,
                    int cout, int ksize, sk_conv_route* route);
/* The i-th kernel name a launch of this precision can reach in the release build, NULL past the end. */
const char* sk_conv3d_route_name(int precision, int i);

/* HOST: torch-layout weight (cout, cin, k, k, k) fp32 -> MFMA A-fragment order fp16.
 * Returns the bytes needed / written (dst_host == NULL only queries). */
int64_t sk_conv3d_pack_weight_host(const float* w_host, int cout, int cin, int ksize,
                                   void* dst_host);

/* One-pass stem (round 4): sk_conv3d_stem's normalisation + the conv ONCE, storing the RAW fp16 result (B, Xt, Yt, Zt, 32)
 * next to its GroupNorm partial sums -- for a consumer that activates a raw source itself (sk_conv3d with
 * sk_conv_src.affine: the single-chunk 32 -> 32 conv in LDS).  HipUNet.stem_single_pass selects it; the default stays the
 * two-pass form (statistics, then apply), which measured the same time end to end. */
int sk_conv3d_stem_raw(const void* image, int X, int Y, int Z, const int32_t* origins_host, int B, int Xt,
                       int Yt, int Zt, float mean, float stdv, const float* weight, const float* bias,
                       int cout, void* out_raw, float* gn_partial, void* workspace, size_t workspace_bytes,
                       void* stream);

/* Stem: first conv of the network (Cin = 1), fused with its GroupNorm + SiLU by running the
 * (cheap) conv twice instead of writing a raw tensor and re-reading it.
 * sk_conv3d_stem: cuts B tiles of extent (Xt,Yt,Zt) at origins_host[3*b..] out of the (X,Y,Z)
 *   fp16 image volume, normalises (x - mean)/std in fp16 arithmetic exactly as eval.py:139 into
 *   the zero-framed workspace, runs the conv (weights split into fp16 hi + lo, exact products,
 *   fp32 accumulation) and writes ONLY the GroupNorm partials (B, stem_num_blocks, 8, 2).
 * sk_conv3d_stem_apply (after sk_groupnorm_finalize): recomputes the conv from the same
 *   workspace, applies the affine (B, 2, 32) + SiLU and stores out (B, Xt, Yt, Zt, 32) fp16
 *   ACTIVATED.  weight (27, 32) fp32 [tap=(dx*3+dy)*3+dz][cout]. */
int sk_conv3d_stem(const void* image, int X, int Y, int Z, const int32_t* origins_host, int B,
                   int Xt, int Yt, int Zt, float mean, float std, const float* weight,
                   const float* bias, int cout, float* gn_partial, void* workspace,
                   size_t workspace_bytes, void* stream);
int sk_conv3d_stem_apply(int B, int Xt, int Yt, int Zt, const float* weight, const float* bias,
                         const float* affine, void* out, int cout, const void* workspace,
                         void* stream);
int sk_conv3d_stem_num_blocks(int X, int Y, int Z);
size_t sk_conv3d_stem_workspace_bytes(int B, int Xt, int Yt, int Zt);

/* GroupNorm statistics -> per-channel affine, reduced in a fixed order (deterministic):
 * gn_partial (B, nblocks, C/4, 2); affine (B, 2, C): a = gamma*rstd, b = beta - mean*a.
 * With more than 4096 rows per sample gn_partial is first compacted IN PLACE (a second kernel level instead of
 * one block reading every row); it is consumed by this call either way. */
int sk_groupnorm_finalize(float* gn_partial, int B, int nblocks, int groups, int C,
                          int64_t voxels, const float* gamma, const float* beta, float eps,
                          float* affine, void* stream);

/* Fused GroupNorm affine + SiLU, in place on (B, voxels, C) fp16. */
int sk_groupnorm_silu(void* x, const float* affine, int B, int64_t voxels, int C, void* stream);

/* Heads: 1x1x1 conv C->5, tanh on [0:3], sigmoid on [3:5]; out5 (B, 5, X, Y, Z) planar fp16 =
 * the reference's output layout (eval.py:145-147).  x: (B, X, Y, Z, C) fp16, activated if
 * affine == NULL, else RAW with affine (B, 2, C) applied (+ SiLU) on load.  weight (5, C) fp32,
 * bias (5).  box_lo/hi_host (int[3], tile-local, may be NULL = whole tile): only that box of every
 * tile is evaluated and written -- the eval pipeline needs just the interior + dilation reach. */
int sk_heads(const void* x, const float* affine, const float* weight, const float* bias, void* out5,
             int B, int X, int Y, int Z, int C, const int* box_lo_host, const int* box_hi_host,
             void* stream);

/* "split" precision mode: every activation is a pair of fp16 tensors hi + lo interleaved per voxel,
 * (B, x, y, z, 2C) = [hi (C) | lo (C)], value = hi + lo (~22 significant bits); weights are split the same way.
 * A product runs as three fp16 MFMAs with fp32 accumulation: w_lo*x_hi + w_hi*x_hi + w_hi*x_lo (the dropped
 * lo*lo term is ~2^-22 relative).  Meets the max-abs 1e-3 tolerance BASELINE.json's north_star states against
 * the fp32 oracle (the plain fp16-operand path sits at 4-7e-3, the reference's own fp16 autocast at eval.py:142
 * likewise) at ~3x the matrix-core work of the fp16 path instead of the 11x of the exact-fp32 instruction.
 * Same semantics as the entry points without the suffix; `c` of a source is its LOGICAL channel count,
 * sources must be activated (affine == NULL). */
int sk_conv3d_split(const sk_conv_src* srcs, int n_src, const void* weight, const float* bias,
                    void* out, int B, int ox, int oy, int oz, int cout, int ksize,
                    float* gn_partial, void* zero_page, void* stream);
/* HOST: torch-layout fp32 weight -> fragments for sk_conv3d_split (ksize 3: [lo, hi, hi] chunk triples of an
 * expanded 3*cin contraction; ksize 1 / 2: hi fragments then lo fragments).  Bytes needed / written. */
int64_t sk_conv3d_pack_weight_split_host(const float* w_host, int cout, int cin, int ksize,
                                         void* dst_host);
/* Precision "mix8" (round 4), 3x3x3, C -> C with C = 32 | 64 | 128: the split conv's two correction products (w_lo x, w x_lo) as
 * ONE block-scaled fp8 matrix product next to the fp16 product w_hi x_hi -- C = 32: v_mfma_scale_f32_16x16x128_f8f6f4, K = 128 =
 * two tap rows x {w_lo . x8, w . lo8} (conv3_m16_kernel); C = 64 | 128: v_mfma_scale_f32_32x32x64_f8f6f4, K = 64 = one tap x
 * {w_lo . x8, w . lo8} per 32-channel chunk (conv3_kernel) -- 2 to 2.1 instead of 3 MFMA passes per tap.
 * src: ONE activated source of 2 C-half lines [hi fp16 (C) | per 32-channel chunk: x8 = e4m3(16 x) (32 bytes) | lo8 =
 * e4m3(2^15 (x - hi)) (32 bytes)] (written by sk_conv3d_stem_apply_mix8 / sk_groupnorm_silu_mix8); weight + weight_scale_exp from
 * sk_conv3d_pack_weight_mix8_host; out / gn_partial / zero_page / store_box as sk_conv3d_box_split (out is a RAW split pair
 * [hi | lo]).  Error of the corrections: 2^-4 relative on terms that are 2^-11 of the result (tools/fp8_correction_study.py). */
int sk_conv3d_mix8(const sk_conv_src* srcs, int n_src, const void* weight, int weight_scale_exp, const float* bias,
                   void* out, int B, int ox, int oy, int oz, int cout, float* gn_partial, void* zero_page,
                   const int* store_box, void* stream);
/* HOST: torch-layout fp32 weight (C, C, 3, 3, 3) -> [fp16 fragments of w_hi | fp8 fragments of (w_lo 2^(b+11), w 2^b)];
 * *scale_exp = b, the largest power of two with 2^b max|w| <= 240.  Bytes needed / written. */
int64_t sk_conv3d_pack_weight_mix8_host(const float* w_host, int cout, int cin, void* dst_host, int* scale_exp);
/* sk_conv3d_stem_apply storing the mix8 line [hi | x8 | lo8]: out (B, Xt, Yt, Zt, 64 halves). */
int sk_conv3d_stem_apply_mix8(int B, int Xt, int Yt, int Zt, const float* weight, const float* bias,
                              const float* affine, void* out, int cout, const void* workspace,
                              void* stream);
/* GroupNorm affine + SiLU in place, RAW split pair [hi | lo] in -> mix8 line out (C = 32 | 64 | 128). */
int sk_groupnorm_silu_mix8(void* x, const float* affine, int B, int64_t voxels, int C, void* stream);
/* sk_conv3d_stem_apply storing the activation as a split pair: out (B, Xt, Yt, Zt, 64). */
int sk_conv3d_stem_apply_split(int B, int Xt, int Yt, int Zt, const float* weight, const float* bias,
                               const float* affine, void* out, int cout, const void* workspace,
                               void* stream);
/* Fused GroupNorm affine + SiLU in place on a split tensor (B, voxels, 2C), fp32 arithmetic. */
int sk_groupnorm_silu_split(void* x, const float* affine, int B, int64_t voxels, int C, void* stream);
/* sk_heads on a split tensor x (B, X, Y, Z, 2C); out5 stays (B, 5, X, Y, Z) fp16 (the reference's
 * autocast output dtype, eval.py:142-147). */
int sk_heads_split(const void* x, const float* affine, const float* weight, const float* bias,
                   void* out5, int B, int X, int Y, int Z, int C, const int* box_lo_host,
                   const int* box_hi_host, void* stream);

/* fp32 precision mode (parity reference of the fast path): the same layers with fp32 activations
 * (B, x, y, z, C) and torch-layout fp32 weights (cout, cin, k, k, k) on the exact-fp32 matrix
 * instruction.  Same source / upsample / concat semantics and GroupNorm partial layout as
 * sk_conv3d (sources must be activated: affine == NULL); any cout when gn_partial is NULL.
 * B and every output extent must be >= 1 (SK_ERR_ARG otherwise, as for every other bad argument:
 * nothing is launched). */
int sk_conv3d_f32(const sk_conv_src* srcs, int n_src, const float* weight, const float* bias,
                  float* out, int B, int ox, int oy, int oz, int cout, int ksize,
                  float* gn_partial, void* stream);
int sk_conv3d_f32_num_blocks(int ox, int oy, int oz);
int sk_groupnorm_silu_f32(float* x, const float* affine, int B, int64_t voxels, int C, void* stream);

/* ------------------------------------------------------------------------ *
 * Training step (BASELINE.json configs[4]; skoots/train/engine.py:456-499): forward with saved
 * tensors, fused Tversky losses, backward, AdamW.  fp32 on channels-last (B, x, y, z, C).
 * The forward uses sk_conv3d_f32 + sk_groupnorm_finalize_stats + sk_train_gn_silu.
 * ------------------------------------------------------------------------ */

/* sk_groupnorm_finalize that also keeps stats (B, groups, 2) = (mean, rstd) for the backward. */
int sk_groupnorm_finalize_stats(float* gn_partial, int B, int nblocks, int groups, int C,
                                int64_t voxels, const float* gamma, const float* beta, float eps,
                                float* affine, float* stats, void* stream);

/* z = silu(a*y + b), out of place (y, the raw conv output, is needed again by the backward). */
int sk_train_gn_silu(const float* y, const float* affine, float* z, int B, int64_t voxels, int C,
                     void* stream);

/* Backward of GroupNorm(groups) + SiLU: dz -> dy (may alias dz), dgamma (C), dbeta (C).
 * workspace: sk_train_gn_bwd_workspace_floats(B, voxels, C) floats. */
int sk_train_gn_silu_bwd(const float* dz, const float* y, const float* affine, const float* stats,
                         const float* gamma, int B, int64_t voxels, int C, int groups, float* dy,
                         float* dgamma, float* dbeta, float* workspace, void* stream);
int64_t sk_train_gn_bwd_workspace_floats(int B, int64_t voxels, int C);
int sk_train_gn_bwd_num_blocks(int64_t voxels);

/* Fused loss of the step (engine.py:465-493): logits (B, X*Y*Z, 5) = the head conv's raw output
 * (tanh / sigmoid are applied inside); masks, skeleton_masks (B, X*Y*Z) fp32 (> 0 = foreground,
 * engine.py:468-472); baked (B, 3, X*Y*Z) fp32.  Three Tversky terms (train/loss.py:157-209,
 * per sample then batch mean) on: exp(-|E - baked|^2 / 2 sigma^2) with E = index + tanh(l)*scale
 * (lib/embedding_to_prob.py:5-51, lib/vector_to_embedding.py:104-105), the probability map and the
 * skeleton map.  loss_params_host (3, 4) = alpha, beta, eps, relative weight for (embed, prob,
 * skeleton).  losses: DEVICE buffer of 16 floats; [0:4] = embed, prob, skeleton, weighted total.
 * dlogits (B, X*Y*Z, 5) = d total / d logits, or NULL for the forward value only.
 * workspace: sk_train_loss_workspace_floats(B, voxels) floats. */
int sk_train_loss(const float* logits, const float* masks, const float* skeleton_masks,
                  const float* baked, int B, int X, int Y, int Z, const float* vector_scale_host,
                  const float* sigma_host, const float* loss_params_host, float* losses,
                  float* dlogits, float* workspace, void* stream);
int64_t sk_train_loss_workspace_floats(int B, int64_t voxels);
int sk_train_loss_num_blocks(int64_t voxels);

/* baked_embed_to_prob (lib/embedding_to_prob.py:5-51): embedding, baked (B, 3, voxels) fp32 ->
 * out (B, voxels) = exp(sum_k (E_k - S_k)^2 / (-2 (sigma_k + eps)^2)). */
int sk_baked_embed_to_prob(const float* embedding, const float* baked, float* out, int B,
                           int64_t voxels, const float* sigma_host, float eps, void* stream);

/* Stand-alone Tversky value (train/loss.py:95-212): predicted, ground_truth (B, voxels) fp32
 * (ground_truth != 0 = foreground); loss = batch mean of 1 - (TP+eps)/(TP+alpha(FP+1e-10)+beta FN+eps),
 * a sample without foreground contributing the constant 1 - eps/(alpha 1e-10 + eps).
 * Every non-zero value of ground_truth, whatever its sign or id, counts as ONE foreground.  The reference
 * expands a ground truth with several ids into one mask per id (train/loss.py:175-182), so this equals the
 * reference for binary ground truth only -- what its callers pass (masks.gt(0), engine.py:468).  sk_train_loss
 * and sk_train_cldice_term_field count `> 0` instead: a negative value is background there, foreground here.
 * workspace: sk_train_loss_workspace_floats(B, voxels) floats. */
int sk_train_tversky(const float* predicted, const float* ground_truth, int B, int64_t voxels,
                     float alpha, float beta, float eps, float* loss, float* workspace,
                     void* stream);

/* Soft skeleton (train/loss.py:269-310, soft_skeletonize): img, skel (B, X, Y, Z) fp32, every axis
 * extent >= 1, 0 <= iter <= SK_CLDICE_MAX_ITER.  e_0 = img, e_{k+1} = min(min(p_x, p_y), p_z) with
 * p_a the 3-wide min along axis a, open_k = 3x3x3 max of e_{k+1} (out-of-range neighbours ignored),
 * d_k = relu(e_k - open_k); skel = d_0, then skel += relu(d_k - skel * d_k) for k = 1..iter.
 * Bit-identical to the reference in fp32.  workspace: sk_train_soft_skeleton_workspace_floats(...). */
#define SK_CLDICE_MAX_ITER 16
int sk_train_soft_skeleton(const float* img, float* skel, int B, int X, int Y, int Z, int iter,
                           float* workspace, void* stream);
int64_t sk_train_soft_skeleton_workspace_floats(int B, int X, int Y, int Z);

/* soft_dice_cldice(iter, alpha, smooth)(pred, gt) (train/loss.py:344-391): pred, gt (B, X, Y, Z)
 * fp32.  loss (DEVICE, 1 float) = (1 - alpha) dice + alpha cl_dice, dice = 1 - (2 sum p g + 1) /
 * (sum g + sum p + 1) (smooth fixed at 1, as the reference calls it), cl_dice = 1 - 2 tprec tsens /
 * (tprec + tsens), tprec = (sum S_p g + smooth) / (sum S_p + smooth), tsens = (sum S_t p + smooth) /
 * (sum S_t + smooth), S = the soft skeletons; every sum runs over the whole batch.  dpred (B, X, Y, Z)
 * = d loss / d pred (torch autograd's routing: max-pool ties to the first maximum in x, y, z scan
 * order, torch.min ties split in halves, relu' = 0 at 0; no gradient into gt), or NULL for the value
 * only; it must not alias pred or gt.  Deterministic (no atomics).  Arguments as sk_train_soft_skeleton;
 * alpha and smooth finite.  workspace: sk_train_soft_dice_cldice_workspace_floats(B, X, Y, Z, iter). */
int sk_train_soft_dice_cldice(const float* pred, const float* gt, int B, int X, int Y, int Z, int iter,
                              float alpha, float smooth, float* loss, float* dpred, float* workspace,
                              void* stream);
int64_t sk_train_soft_dice_cldice_workspace_floats(int B, int X, int Y, int Z, int iter);

/* A soft-clDice term of the fused step (sk_train_loss's layout: logits (B, X*Y*Z, 5), target
 * (B, X*Y*Z), baked (B, 3, X*Y*Z), host vector_scale / sigma).  term 0 = embed, 1 = probability,
 * 2 = skeleton.  sk_train_cldice_term_field: prob (B, X*Y*Z) = the term's probability field
 * (sk_train_loss's embedding probability, sigmoid(logits[..., 4]), sigmoid(logits[..., 3])) and
 * gt = (target > 0); baked may be NULL for terms 1, 2.  sk_train_cldice_chain, after sk_train_loss
 * (run with this term's weight 0): dlogits += weight * dprob * d prob / d logits (through
 * E = index + tanh(l) scale for term 0, p (1 - p) for 1, 2), losses[term] = term_loss[0] and
 * losses[3] += weight * term_loss[0]; dlogits and dprob both NULL = losses only. */
int sk_train_cldice_term_field(const float* logits, const float* target, const float* baked, int B,
                               int X, int Y, int Z, const float* vector_scale_host,
                               const float* sigma_host, int term, float* prob, float* gt,
                               void* stream);
int sk_train_cldice_chain(const float* logits, const float* baked, int B, int X, int Y, int Z,
                          const float* vector_scale_host, const float* sigma_host, int term,
                          float weight, const float* dprob, const float* term_loss, float* losses,
                          float* dlogits, void* stream);

/* Data gradient of a conv layer from dy (B, ox, oy, oz, cout) and the layer's own weight
 * (cout, cin_total, k, k, k), read transposed / tap-flipped in place.
 *   ksize 1, 3: dx (B, ox, oy, oz, cin_n) = gradient w.r.t. input channels [cin_lo, cin_lo+cin_n)
 *               (one half of a concatenated input; an upsampled half is pooled afterwards with
 *               sk_train_sumpool2).
 *   ksize 2 (stride 2): dx (B, 2ox, 2oy, 2oz, cin_total); cin_lo = 0, cin_n = cin_total.
 * accumulate != 0 adds into dx (a tensor with two consumers). */
int sk_train_conv_dgrad(const float* dy, const float* weight, float* dx, int B, int ox, int oy,
                        int oz, int cout, int cin_total, int cin_lo, int cin_n, int ksize,
                        int accumulate, void* stream);

/* Weight and bias gradient of a conv layer: srcs as in sk_conv3d_f32 (activated fp32 inputs, the
 * second optionally nearest-upsampled), dy (B, ox, oy, oz, cout) -> dweight (cout, cin, k, k, k),
 * dbias (cout) or NULL.  workspace: sk_train_conv_wgrad_workspace_floats(...) floats. */
int sk_train_conv_wgrad(const sk_conv_src* srcs, int n_src, const float* dy, int B, int ox, int oy,
                        int oz, int cout, int ksize, float* dweight, float* dbias,
                        float* workspace, void* stream);
int64_t sk_train_conv_wgrad_workspace_floats(int B, int ox, int oy, int oz, int cout, int cin,
                                             int ksize);

/* HOST (ABI 24; no GPU needed): which kernel a weight-gradient launch runs and how it cuts the work -- the answer of the one
 * function that sk_train_conv_wgrad (SK_WGRAD_FP32), sk_train_conv_wgrad_f16 (SK_WGRAD_F16; has_zero_page: zero_page != NULL)
 * and sk_train_stem_wgrad_f16 (SK_WGRAD_STEM_F16: only B and the extents are read) ask themselves.  Of srcs only c and upsample
 * are read.  name: e.g. "wgrad<9>", "wgrad16x", "wgrad16t<8>", "wgrad_stem16".  nchunk partial rows (nchunk_b voxel chunks of
 * `chunk` voxels per batch item; for "wgrad16x" its own count nchunk_x of 16 x 16 footprints x nxs segments of xseg planes),
 * ngroup tap groups, ncol_chunk columns a chunk of "wgrad16y"; workspace_floats: sk_train_conv_wgrad_workspace_floats. */
enum { SK_WGRAD_FP32 = 0, SK_WGRAD_F16 = 1, SK_WGRAD_STEM_F16 = 2 };
typedef struct sk_wgrad_route {
    char name[32];
    int nchunk, nchunk_b;
    int64_t chunk;
    int ngroup, nchunk_x, nxs, xseg, ncol_chunk;
    int64_t grid, workspace_floats;
} sk_wgrad_route;
int sk_train_conv_wgrad_route(int entry, const sk_conv_src* srcs, int n_src, int B, int ox, int oy, int oz, int cout,
                              int ksize, int has_zero_page, sk_wgrad_route* route);
/* The i-th kernel name the entry can reach in the release build, NULL past the end. */
const char* sk_train_conv_wgrad_route_name(int entry, int i);

/* Mixed-precision pieces (TrainUNet precision="mixed"): fp16 copies feed the fp16 MFMA kernels.
 * sk_train_absmax_scale: scale (3 floats, device) <- [2^k, 2^-k, scratch] with max|x| * 2^k in [2^12, 2^13).
 * sk_train_cast_f32_f16: y = fp16(x * scale[0]) (scale NULL: 1).  sk_train_cast_f16_f32: y (+)= float(x) * scale[1].
 * sk_train_conv_wgrad_f16: sk_train_conv_wgrad with fp16 sources and fp16 dy (scaled by dy_scale[0], or
 *   unscaled if dy_scale is NULL) on v_mfma_f32_32x32x16_f16; fp32 partial sums, result multiplied by
 *   dy_scale[1].  Same workspace size as the fp32 entry point.  zero_page (>= 1 KiB of zeros, or NULL):
 *   with it and channel counts % 32 == 0 the operands move as whole 64-byte lines (LDS-DMA + ds_read_b64_tr_b16).
 * sk_train_pack_weight: device-side sk_conv3d_pack_weight_host of the CURRENT fp32 weight (Co, Ci, k, k, k);
 *   transposed != 0 packs the data-gradient operator of input channels [c_lo, c_lo + c_n) instead
 *   (rows = those input channels, K = Co, taps flipped).  dst: k^3 * (cin_eff/16) * (cout_eff/32) KiB.
 */
int sk_train_pack_weight(const float* weight, int Co, int Ci, int ksize, int transposed, int c_lo,
                         int c_n, void* dst, void* stream);
/* transposed == 2: transposed WITHOUT the tap flip -- the stride-2 (ksize 2) data gradient in scatter form:
 * fragment block p (of 8, each (Co/16)*(Ci/32) KiB) is the pointwise operator W_p^T of parity p; run it with
 * sk_conv3d(ksize 1) into t16[p] (B, cx, cy, cz, Ci) and assemble with sk_train_interleave2:
 * dx (B, 2cx, 2cy, 2cz, Ci) (+)= t16[parity][coarse voxel] * scale[1]. */
int sk_train_interleave2(const void* t16, float* dx, int B, int cx, int cy, int cz, int C,
                         const float* scale, int accumulate, void* stream);
/* Lean mixed data flow: sk_train_gn_silu_f16: raw fp16 conv output -> z16 (and z32 if not NULL).
 * sk_train_gn_silu_bwd_f16: dz (fp32) and the RAW fp16 output -> dy16 = fp16(dy * scale[0]) with scale (3 floats,
 * device: 2^k, 2^-k, bound) chosen from an upper bound of max|dy| formed in the reduction pass; dgamma, dbeta as
 * sk_train_gn_silu_bwd.  workspace: sk_train_gn_bwd_f16_workspace_floats(B, voxels, C) floats. */
int sk_train_gn_silu_f16(const void* y16, const float* affine, void* z16, float* z32, int B,
                         int64_t voxels, int C, void* stream);
int sk_train_gn_silu_bwd_f16(const float* dz, const void* y16, const float* affine, const float* stats,
                             const float* gamma, int B, int64_t voxels, int C, int groups, void* dy16,
                             float* scale, float* dgamma, float* dbeta, float* workspace, void* stream);
int64_t sk_train_gn_bwd_f16_workspace_floats(int B, int64_t voxels, int C);
int sk_train_absmax_scale(const float* x, int64_t n, float* scale, void* stream);
int sk_train_cast_f32_f16(const float* x, void* y, int64_t n, const float* scale, void* stream);
int sk_train_cast_f16_f32(const void* x, float* y, int64_t n, const float* scale, int accumulate,
                          void* stream);
int sk_train_conv_wgrad_f16(const sk_conv_src* srcs, int n_src, const void* dy, const float* dy_scale,
                            int B, int ox, int oy, int oz, int cout, int ksize, float* dweight,
                            float* dbias, float* workspace, const void* zero_page, void* stream);

/* coarse (B, cx, cy, cz, C) = 2x2x2 block sums of fine (B, 2cx, 2cy, 2cz, C). */
int sk_train_sumpool2(const float* fine, float* coarse, int B, int cx, int cy, int cz, int C,
                      void* stream);
/* sk_train_gn_silu_bwd_f16h: sk_train_gn_silu_bwd_f16 with the incoming gradient itself a scaled fp16 tensor (the
 *   output of the consumer's fast data-gradient conv): true dz = dz16 * dz_scale[1].  No fp32 copy in between.
 * sk_train_sumpool2_f16: sk_train_sumpool2 from a scaled fp16 fine tensor: coarse = scale[1] * sum of the 8 children. */
int sk_train_gn_silu_bwd_f16h(const void* dz16, const float* dz_scale, const void* y16, const float* affine,
                              const float* stats, const float* gamma, int B, int64_t voxels, int C, int groups,
                              void* dy16, float* scale, float* dgamma, float* dbeta, float* workspace, void* stream);
int sk_train_sumpool2_f16(const void* fine16, const float* scale, float* coarse, int B, int cx, int cy, int cz, int C,
                          void* stream);
/* The stem as a fast block of the mixed step.  sk_train_stem_fwd_f16: image (B, X, Y, Z) fp32 (rounded to fp16 as the
 *   MFMA operand, weights exact through a hi + lo split), weight_t (27, 32) fp32 tap-major, bias (32) -> RAW y16
 *   (B, X, Y, Z, 32) fp16 + gn_partial (B, sk_conv3d_stem_num_blocks(X, Y, Z), 8, 2); workspace:
 *   sk_conv3d_stem_workspace_bytes(B, X, Y, Z).  B <= 64, Z even.
 * sk_train_stem_wgrad_f16: image fp32 and the scaled fp16 dy (B, X, Y, Z, 32) -> dweight (32, 1, 3, 3, 3), dbias (32),
 *   multiplied by dy_scale[1]; workspace: sk_train_conv_wgrad_workspace_floats(B, X, Y, Z, 32, 1, 3). */
int sk_train_stem_fwd_f16(const float* image, int B, int X, int Y, int Z, const float* weight_t, const float* bias,
                          void* y16, float* gn_partial, void* workspace, size_t workspace_bytes, void* stream);
int sk_train_stem_wgrad_f16(const float* image, const void* dy16, const float* dy_scale, int B, int X, int Y, int Z,
                            float* dweight, float* dbias, float* workspace, void* stream);
/* Heads of the mixed step on the fp16 activation z16 (nvox, 32): logits (nvox, 5) fp32 = z W^T + b with W (5, 32);
 * weight / bias gradients from z16 and dlogits (nvox, 5) fp32 (deterministic two-stage reduction; workspace:
 * sk_train_heads_wgrad_workspace_floats(nvox) floats).  nvox counts the voxels of all batch items. */
/* sk_train_interleave2_add16: sk_train_interleave2 (no accumulate) plus a second scaled fp16 gradient of the same fine
 * tensor, add16 (B, 2cx, 2cy, 2cz, C) * add_scale[1] -- the two contributions to a skip tensor in one pass. */
int sk_train_interleave2_add16(const void* t16, const void* add16, const float* add_scale, float* dx, int B, int cx,
                               int cy, int cz, int C, const float* scale, void* stream);
/* 16-bit hand-off of a gradient to the GroupNorm backward that consumes it (sk_train_gn_silu_bwd_f16h): the producer
 * writes the scaled 16-bit tensor AND its scale vector out_scale (3 floats, device) = [s, 1/s, bound], s a power of two
 * derived from the input scales so that the result cannot overflow (no max pass, no fp32 tensor).
 * sk_train_interleave2_h: sk_train_interleave2 / _add16 (add16 may be NULL) with a 16-bit result dx16 (B, 2cx, 2cy, 2cz, C).
 * sk_train_sumpool2_hh: sk_train_sumpool2_f16 with a 16-bit result coarse16 (B, cx, cy, cz, C), s = scale[0] / 8.
 * sk_train_heads_dgrad_f16: data gradient of the heads, dx[v][c] = sum_k dlogits[v][k] W[k][c] (W (5, C) fp32), from the
 *   fp32 dlogits (nvox, 5) and dl_scale = sk_train_absmax_scale(dlogits).  C % 8 == 0. */
int sk_train_interleave2_h(const void* t16, const void* add16, const float* add_scale, void* dx16, float* out_scale, int B,
                           int cx, int cy, int cz, int C, const float* scale, void* stream);
int sk_train_sumpool2_hh(const void* fine16, const float* scale, void* coarse16, float* out_scale, int B, int cx, int cy, int cz,
                         int C, void* stream);
int sk_train_heads_dgrad_f16(const float* dlogits, const float* dl_scale, const float* weight, void* dx16, float* out_scale,
                             int64_t nvox, int C, void* stream);
int sk_train_heads_fwd_f16(const void* z16, const float* weight, const float* bias, float* logits, int64_t nvox,
                           void* stream);
int64_t sk_train_heads_wgrad_workspace_floats(int64_t nvox);
int sk_train_heads_wgrad_f16(const void* z16, const float* dlogits, float* dweight, float* dbias, int64_t nvox,
                             float* workspace, void* stream);

/* One AdamW update (torch.optim.AdamW semantics; engine.py:281-285, config.py:96-101) over a
 * flat parameter buffer; step counts from 1. */
int sk_train_adamw(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n,
                   float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                   void* stream);

/* ------------------------------------------------------------------------ *
 * Training-target baking (skoots/lib/skeleton.py:448-528 with its Triton kernel :51-251, and
 * average_baked_skeletons :18-48).  masks (X, Y, Z) int32 instance ids; the skeletons as a CSR table: ids (K,
 * ascending), offsets (K+1), points (offsets[K], 3) fp32 voxel coordinates.  baked (3, X, Y, Z) fp32 = the
 * nearest point of the voxel's own skeleton under anisotropy_host (3) (first minimal point on ties, exact
 * distances), 0 for background / unknown ids; distance (X, Y, Z) fp32 or NULL.
 * sk_average_baked_skeletons: out[c, v] = sum of the zero-padded 3x3x3 neighbourhood / number of entries > 0. */
int sk_bake_skeleton(const int32_t* masks, const int32_t* ids, const int32_t* offsets,
                     const float* points, int K, int X, int Y, int Z, const float* anisotropy_host,
                     float* baked, float* distance, void* stream);
int sk_average_baked_skeletons(const float* baked, float* out, int C, int X, int Y, int Z,
                               void* stream);

/* ------------------------------------------------------------------------ *
 * Training-crop augmentation (skoots/train/merged_transform.py:402-762, TransformFromCfg).
 *
 * sk_aug_resample: one gather over the crop-2 output (w2, h2, d2) that composes, for each output voxel, the flips,
 * the crop-2 origin (in the crop-1 window of extents (w1, h1, d1)), the per-z-slice inverse affine (torchvision's
 * rescaled theta: theta[0..2] = the grid's x row, [3..5] its y row; nearest, align_corners False, 0 outside the
 * slice), the elastic map (field (1, 3, field_d, field_h, field_w) fp32 on the device, interpolated trilinearly to
 * (w1, h1, d1) on the fly and scaled by magnitude = (z, y, x); nearest, align_corners True, 0 outside) and the
 * crop-1 origin in the source (1, src_x, src_y, src_z).  image uint8 / fp16 / fp32 (SK_U8 / SK_F16 / SK_F32), masks
 * uint8 / int16 / int32 (SK_U8 / SK_I16 / SK_I32), both contiguous; out_image fp32 and out_masks int32, (w2, h2, d2)
 * contiguous.  invert (255 - v) and brightness (clamp(v + brightness_val, 0, 255)) are applied in the same pass,
 * which also leaves the per-z partial sums of out_image / 255 in the workspace (sk_aug_workspace_bytes).
 *
 * sk_aug_intensity (two launches, in place on out_image, same workspace): contrast blend + clamp with one mean per
 * z-slice (contrast != 0), + noise * noise_gamma (noise (w2, h2, d2) fp32 or NULL), then (v - mean) / std where
 * own_mean / own_std ask for the image's mean / unbiased std instead of the given values.  Reductions run in a fixed
 * order without atomics.
 *
 * sk_skeleton_to_mask: out (X, Y, Z) fp32 = 1 at trunc(point + offset) for every point (n_points, 3) fp32 and every
 * row of the offset table (n_offsets, 3) int32 that lands inside, 0 elsewhere.  Every check runs before any write. */
typedef struct {
    int src_x, src_y, src_z;
    int c1_x0, c1_y0, c1_z0, w1, h1, d1;
    int c2_x0, c2_y0, c2_z0, w2, h2, d2;
    int flip_x, flip_y, flip_z;
    int affine;
    float theta[6];
    int elastic, field_d, field_h, field_w;
    float magnitude[3];
    int invert, brightness;
    float brightness_val;
} sk_aug_params;
size_t sk_aug_workspace_bytes(int w2, int h2, int d2);
int sk_aug_resample(const sk_aug_params* params, const void* image, int image_dtype, const void* masks,
                    int masks_dtype, const float* field, float* out_image, int32_t* out_masks, void* workspace,
                    size_t workspace_bytes, void* stream);
int sk_aug_intensity(float* image, int w2, int h2, int d2, int contrast, float contrast_val, const float* noise,
                     float noise_gamma, int own_mean, float mean, int own_std, float std_value, void* workspace,
                     size_t workspace_bytes, void* stream);
int sk_skeleton_to_mask(const float* points, int64_t n_points, const int32_t* offsets, int n_offsets, int X, int Y,
                        int Z, float* out, void* stream);

/* ------------------------------------------------------------------------ *
 * Training skeletons (skoots/train/generate_skeletons.py:65-157 calculate_skeletons, whose per-object
 * skimage.morphology.skeletonize(crop, method="lee") is scikit-image 0.18.3's Lee thinning): the thinning of every
 * object in its own crop, one workgroup per object, bit for bit the sequential algorithm.
 *
 * boxes_host[6 i .. 6 i + 5] = (x0, y0, z0, x1, y1, z1): object i (id ids[i]) is thinned in the binary crop
 * labels[x0:x1, y0:y1, z0:z1] == ids[i]; labels (X, Y, Z) int32.  An object whose padded crop fits the kernel's LDS
 * (24 bytes per 32-voxel word of the padded crop, 152 KiB at most) is thinned there, a larger one in the workspace.
 *
 * sk_skeletonize_workspace_bytes: bytes of workspace (16-byte aligned) for these boxes; 0 if a box is empty.
 * sk_skeletonize: counts[i] = skeleton voxels of object i, stats[2 i] = passes, stats[2 i + 1] = the most re-check
 * rounds of one sub-iteration; *error = 0, or bit 0 (a round bound hit) / bit 1 (the pass bound hit).  The skeletons
 * stay in the workspace for sk_skeletonize_emit.  Synchronises `stream` (the crop table is copied from the host).
 * sk_skeletonize_emit: points[offsets[i] ..] = the skeleton voxels of object i in raster order of its crop, as int32
 * crop coordinates (x, y, z); offsets (n + 1) int32 is the exclusive prefix sum of counts; no row at or beyond
 * n_points is written.
 *
 * sk_skeleton_graph (ABI 16): the skeletons that sk_skeletonize left in the workspace, read as
 * graphs -- called after it with the same boxes and workspace, like sk_skeletonize_emit; one workgroup per object.  A
 * link is an unordered pair of skeleton voxels of one object that are 26-neighbours, the degree of a voxel the number
 * of its links.  graph (n, 12) int64, row i: [0] skeleton voxels (= counts[i]), [1] voxels of degree 0, [2] of degree
 * 1 (endpoints), [3] of degree 2 (chain voxels), [4] of degree >= 3 (junction voxels), [5..11] links by direction
 * class (|dx|, |dy|, |dz|) = (1,0,0) (0,1,0) (0,0,1) (1,1,0) (1,0,1) (0,1,1) (1,1,1).  Every link is counted once;
 * [2] + 2 [3] + the degrees of the junction voxels = 2 sum([5..11]).  All sums are integers reduced inside the
 * workgroup: the same on every run.  An empty skeleton gives a row of zeros.
 * sk_skeleton_graph_row_values: 12, the values per row. */
size_t sk_skeletonize_workspace_bytes(const int32_t* boxes_host, int n);
int sk_skeletonize(const int32_t* labels, int X, int Y, int Z, const int32_t* ids, const int32_t* boxes_host, int n,
                   void* workspace, size_t workspace_bytes, int32_t* counts, int32_t* stats, int32_t* error,
                   void* stream);
int sk_skeletonize_emit(const int32_t* boxes_host, int n, const void* workspace, size_t workspace_bytes,
                        const int32_t* offsets, int64_t n_points, int32_t* points, void* stream);
int sk_skeleton_graph_row_values(void);
int sk_skeleton_graph(const int32_t* boxes_host, int n, const void* workspace, size_t workspace_bytes,
                      int64_t* graph, void* stream);

/* Every skeleton branch traced (ABI 26; no reference counterpart): the skeletons in the thinning
 * workspace read as nodes and branches, one workgroup per object, integers only, the same bytes on every run.
 *
 * Definitions, per object.  A link is an unordered pair of 26-neighbouring skeleton voxels, the degree of a voxel the
 * number of its links, a chain voxel one of degree 2.  A NODE is an isolated voxel (type 0), an endpoint (type 1, degree
 * 1), a junction (type 2: a 26-connected component of voxels of degree >= 3, of any size) or a ring anchor (type 3: the
 * first voxel, lexicographically in (x, y, z), of a cycle of chain voxels only).  A node's first voxel is its
 * lexicographically smallest; the links between two of its own voxels are internal and belong to no branch.  A BRANCH
 * is a maximal run of >= 1 chain voxels with the two links that end it at node voxels, or a single link between voxels
 * of two different nodes, or a ring from its anchor round and back (n - 1 chain voxels, n links).  Both ends may lie in
 * one node or be one voxel (a self-loop).  End a is the end with the smaller (rank of the end voxel in (x, y, z) order,
 * direction code of the branch's first link there); the direction code is the bit index 9 (dx + 1) + 3 (dy + 1) +
 * (dz + 1) of the 27-bit neighbourhood code.  A ring has a = b = its anchor and the smaller of the anchor's two codes.
 *
 * nodes (Nn, 8) int32: [0] object index, [1] type, [2] voxels, [3] internal links, [4..6] first voxel in volume
 * coordinates (crop origin added), [7] branch ends attached (a self-loop counts 2, a ring anchor has 2).
 * branches (Nb, 18) int32: [0] object index, [1] node row of end a, [2] node row of end b (rows of `nodes`), [3] chain
 * voxels, [4..10] links by the direction classes of sk_skeleton_graph, terminal links included, [11..13] end voxel a,
 * [14..16] end voxel b, volume coordinates, [17] direction code at a.
 * owner (n_points) int32, aligned with the points of sk_skeletonize_emit: a chain voxel holds its branch row, a node
 * voxel -1 - its node row.  Rows come object by object; within an object nodes by first voxel and branches by (end
 * voxel a, direction code at a), rings too.
 *
 * sk_skeleton_pack: the arguments of sk_skeletonize; writes the crops of `labels == ids[i]` into the workspace WITHOUT
 * thinning them -- `labels` holds skeletons already (or any binary objects) -- and fills counts; stats and *error are
 * zeroed.  After it sk_skeleton_graph, sk_skeletonize_emit and the calls below work on the workspace as after
 * sk_skeletonize.  Synchronises `stream`.
 * sk_skeleton_branches_scratch_bytes: bytes of scratch for these boxes and counts (host arrays; 44 per skeleton voxel
 * + 16); 0 if a box is refused, a count is negative or exceeds its crop, or the counts sum to 2^31 or more.
 * sk_skeleton_branches_count: node_branch_counts (n, 2) int32 = nodes and branches of every object; offsets (n + 1)
 * int32 on the device is the exclusive prefix sum of counts, as for sk_skeletonize_emit.  An object whose plane does
 * not hold exactly offsets[i + 1] - offsets[i] voxels inside its crop gets (-1, -1) and is not traced.
 * sk_skeleton_branches_emit: the rows, at node_offsets / branch_offsets (n + 1) int32 on the device, the exclusive
 * prefix sums of the counts; no node row at or beyond n_nodes, no branch row at or beyond n_branches and no owner at or
 * beyond n_points is written.  The scratch is working memory: the passes do not hand anything to each other in it.
 * Every argument is checked before anything is launched (SK_ERR_ARG): null pointers, sizes of workspace and scratch,
 * alignment (workspace 16 bytes, everything else 4), totals below 2^31.
 * sk_skeleton_nodes_row_values: 8; sk_skeleton_branches_row_values: 18. */
int sk_skeleton_pack(const int32_t* labels, int X, int Y, int Z, const int32_t* ids, const int32_t* boxes_host, int n,
                     void* workspace, size_t workspace_bytes, int32_t* counts, int32_t* stats, int32_t* error,
                     void* stream);
int sk_skeleton_nodes_row_values(void);
int sk_skeleton_branches_row_values(void);
size_t sk_skeleton_branches_scratch_bytes(const int32_t* boxes_host, const int32_t* counts_host, int n);
int sk_skeleton_branches_count(const int32_t* boxes_host, int n, const void* workspace, size_t workspace_bytes,
                               const int32_t* offsets, int64_t n_points, void* scratch, size_t scratch_bytes,
                               int32_t* node_branch_counts, void* stream);
int sk_skeleton_branches_emit(const int32_t* boxes_host, int n, const void* workspace, size_t workspace_bytes,
                              const int32_t* offsets, int64_t n_points, void* scratch, size_t scratch_bytes,
                              const int32_t* node_offsets, const int32_t* branch_offsets, int64_t n_nodes,
                              int64_t n_branches, int32_t* nodes, int32_t* branches, int32_t* owner, void* stream);

/* ------------------------------------------------------------------------ *
 * Validation metrics (skoots/validate/lib.py:190-229 mask_iou): iou (N, M) fp32 of the N
 * ground-truth and M predicted instances, intersection / union of voxel counts, 0 for pairs that do not touch.
 * gt, pred (n) int32; lut_gt (max_gt + 1) / lut_pred (max_pred + 1) int32 map an id to its 1-based row / column
 * (0 = ignore: background or unlisted).  workspace: sk_mask_iou_workspace_bytes(N, M). */
size_t sk_mask_iou_workspace_bytes(int N, int M);
int sk_mask_iou(const int32_t* gt, const int32_t* pred, int64_t n, const int32_t* lut_gt, int max_gt, int N,
                const int32_t* lut_pred, int max_pred, int M, float* iou, void* workspace,
                size_t workspace_bytes, void* stream);

/* Dice and soft-clDice matrices (ABI 6; skoots/validate/lib.py:232-315 mask_dice / mask_soft_cldice, the metrics of
 * skoots/validate/__main__.py).  Volumes are (1, X, Y, Z) int32 with z fastest, at most 2^31 - 1 voxels; iters in
 * [0, 12] (the reference's soft_cldice uses 3).
 *
 * sk_label_soft_skeleton2d: skel (X, Y, Z) uint8 = 1 where a voxel lies on its own instance's soft skeleton
 * (train/loss.py:295-310 on `labels == id`, 4-D branch): per (Y, Z) slice, D(u) = own-label cross-erosion depth
 * capped at iters + 1 (in-slice 4-neighbours; out-of-slice neighbours are ignored), and u is on the skeleton iff
 * labels(u) > 0 and no voxel of its in-slice 3x3 window has its label and D >= min(D(u), iters) + 1.
 *
 * sk_mask_metrics: whichever of iou / dice / cldice (N, M) fp32 is non-NULL, rows / columns as in sk_mask_iou (same
 * luts).  One pass builds three int32 contingency tables: voxel counts, pred-skeleton counts at x >= 1 and
 * gt-skeleton counts at x >= 1.  A pair with no common voxel (any x) is 0 in every matrix.  Otherwise
 *   iou    = float(|A & B|) / float(|A | B|)
 *   dice   = float(2 |A & B|) / float(|A| + |B|)
 *   cldice = 1 - (2 (tprec tsens)) / (tprec + tsens)   (the loss, as the reference stores it), with
 *            tprec = (float(S_p) + 1) / (float(T_p) + 1), tsens = (float(S_g) + 1) / (float(T_g) + 1);
 *            S_p = pred-b skeleton voxels inside gt a, T_p = pred-b skeleton voxels, S_g / T_g the same for gt a,
 *            all over x >= 1.  Bit-exact to the reference while every T is below 2^24.
 * cldice = NULL skips the skeleton.  workspace: sk_mask_metrics_workspace_bytes(N, M); it needs
 * (N + 1) (M + 1) <= 2^31 - 1.  Every argument is checked before the first write. */
int sk_label_soft_skeleton2d(const int32_t* labels, int X, int Y, int Z, int iters, uint8_t* skel, void* stream);
size_t sk_mask_metrics_workspace_bytes(int N, int M);
int sk_mask_metrics(const int32_t* gt, const int32_t* pred, int X, int Y, int Z, const int32_t* lut_gt, int max_gt,
                    int N, const int32_t* lut_pred, int max_pred, int M, int iters, float* iou, float* dice,
                    float* cldice, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------ *
 * Training command: dataset statistics
 * ------------------------------------------------------------------------ */

/* Adds the histogram of the n bytes at x into the 256 counters hist256 (the caller zeroes them; a second call adds
 * into the same counters).  Replaces the per-volume host loops of skoots/train/dataloader.py:246-310 (dataset.sum,
 * subtract_square_sum) for a volume that lives on the device: the sum is sum_v v h[v], exactly, and
 * sum (x - other)^2 = sum_v h[v] (v - other)^2 for any `other`.  x may have any alignment; n in [0, 2^40]; hist256 is
 * 8-byte aligned.  Integer atomics: exact and identical from run to run.  Every argument is checked before the
 * first write. */
int sk_u8_histogram(const uint8_t* x, int64_t n, unsigned long long* hist256, void* stream);

/* ------------------------------------------------------------------------ *
 * eval() outputs: deflate encoder for the zarr chunks and the TIFF pages
 * ------------------------------------------------------------------------ */

/* Compresses n_streams inputs of stream_bytes bytes each (src: contiguous, any alignment) into n_streams complete
 * zlib streams (RFC 1950: 78 01, RFC 1951 blocks, Adler-32 big-endian), written back to back into dst: stream i is
 * dst[dst_offsets[i] .. dst_offsets[i + 1]); dst_offsets has n_streams + 1 entries (device, 8-byte aligned).  Replaces
 * zlib.compress(chunk, 1) on the host (the reference leaves its arrays to zarr / skimage, eval.py:101-111, 309-310).
 * dst must hold n_streams * sk_deflate_bound(stream_bytes) bytes: the worst case of one stream, in which every 16 KiB
 * piece is a stored block (n + 8 <= bound(n) <= n + n / 1024 + 64).  A zero-length stream is the 8-byte empty stream.
 * elem_bytes (1, 2 or 4) is a hint: the match distances tried are 1 and k * elem_bytes, k = 1..64; the format does
 * not change with it.  all_zero (device, n_streams bytes) may be NULL; when given, all_zero[i] = 1 says that input i
 * held only zero bytes, and such a stream is left out of dst (dst_offsets[i + 1] == dst_offsets[i]): the zarr writer
 * does not store fill-value chunks.  The bytes depend on the input alone: the same on every run, for every n_streams.
 * workspace: sk_deflate_workspace_bytes(n_streams, stream_bytes), 16-byte aligned.  sk_deflate_bound and
 * sk_deflate_workspace_bytes are host functions that touch no device.  Every argument is checked before the first
 * write. */
size_t sk_deflate_bound(int64_t stream_bytes);
size_t sk_deflate_workspace_bytes(int n_streams, int64_t stream_bytes);
int sk_deflate_streams(const uint8_t* src, int n_streams, int64_t stream_bytes, int elem_bytes, uint8_t* dst,
                       int64_t* dst_offsets, uint8_t* all_zero, void* workspace, size_t workspace_bytes, void* stream);

/* sk_deflate_streams with a choice of code.  huffman = 0: the fixed code of RFC 1951 3.2.6, byte for byte what
 * sk_deflate_streams writes.  huffman = 1: the same parse, and every 16 KiB piece is written in the form with the
 * fewest bytes among stored (5 + n), the fixed code and a dynamic code built for the piece (3.2.7, header included);
 * on equal bytes the order is stored, fixed, dynamic.  So a stream is never longer than with huffman = 0, and
 * sk_deflate_bound and sk_deflate_workspace_bytes hold for both.  The dynamic code: optimal code lengths under the
 * limit 15 (ties in the order (count, symbol); see sk_deflate_code_host), HDIST = 1 with one length of zero when the
 * piece has no match, one length of 1 when it has one distance symbol, complete codes otherwise; the length sequence
 * uses 16, 17 and 18.  The same argument checks run before any launch; any other huffman is refused
 * (SK_ERR_ARG, "sk_deflate_streams_coded: huffman = ...").  The bytes depend on the input alone. */
int sk_deflate_streams_coded(const uint8_t* src, int n_streams, int64_t stream_bytes, int elem_bytes, int huffman,
                             uint8_t* dst, int64_t* dst_offsets, uint8_t* all_zero, void* workspace,
                             size_t workspace_bytes, void* stream);

/* Host function, no device touched: the code builder the piece kernel runs (the same text, compiled for the host).
 * freq[n_symbols] (1 <= n_symbols <= 286, sum below 2^32) -> lengths[n_symbols] (0 for an unused symbol, else
 * 1..limit, 1 <= limit <= 15) and the canonical codes of RFC 1951 3.2.2 (most significant bit first, 0 for an unused
 * symbol).  The result is a function of freq alone: the used symbols are ordered by (count, symbol), merged with the
 * two-queue method (leaf before internal node on equal weights), depths beyond the limit are repaired on the
 * per-depth counts, and lengths are dealt out along the order, longest to the rarest.  Sum freq * length is the
 * Huffman optimum whenever an optimal code fits the limit; the Kraft sum is exactly 1 with two or more used symbols.
 * One used symbol gets length 1, none gets no length.  More used symbols than 2^limit is refused. */
int sk_deflate_code_host(const uint32_t* freq, int n_symbols, int limit, uint8_t* lengths, uint16_t* codes);

/* Host function, no device touched: the header of a dynamic block for lit_lengths[286] and dist_lengths[30] (each
 * 0..15), as the piece kernel writes it: BFINAL = bfinal, BTYPE = 10, HLIT, HDIST, HCLEN, the code-length code's
 * lengths (limit 7), the run-length coded length sequence.  out (at least 576 bytes) receives the bits, least
 * significant bit of out[0] first, the rest zero; *n_bits their number. */
int sk_deflate_header_host(const uint8_t* lit_lengths, const uint8_t* dist_lengths, int bfinal, uint8_t* out,
                           size_t out_bytes, int64_t* n_bits);

/* ------------------------------------------------------------------------ *
 * Reading eval()'s files back: inflate decoder for zarr chunks and TIFF strips
 * ------------------------------------------------------------------------ */

/* status[i] of sk_inflate_streams: 0, or why stream i was refused */
#define SK_INFLATE_E_HEADER 1        /* RFC 1950 header: method not 8, window above 32 KiB, check bits wrong, or FDICT set */
#define SK_INFLATE_E_BLOCK_TYPE 2    /* reserved block type 3 */
#define SK_INFLATE_E_STORED 3        /* stored block: LEN is not the complement of NLEN */
#define SK_INFLATE_E_CODES 4         /* dynamic block: over-subscribed or incomplete code-length set, bad repeat, no end-of-block code */
#define SK_INFLATE_E_SYMBOL 5        /* bits that are no code of the block, literal/length symbol 286 / 287, distance code 30 / 31 */
#define SK_INFLATE_E_DISTANCE 6      /* distance reaches before the start of the output */
#define SK_INFLATE_E_INPUT 7         /* input exhausted before the stream (and its Adler-32) ended */
#define SK_INFLATE_E_OUTPUT_LONG 8   /* the stream holds more bytes than expected */
#define SK_INFLATE_E_OUTPUT_SHORT 9  /* the stream ended with fewer bytes than expected */
#define SK_INFLATE_E_ADLER 10        /* Adler-32 of the output differs from the trailer */
#define SK_INFLATE_E_RANGE 11        /* src_offsets / dst_offsets of the stream are negative or decreasing */

/* Inflates n_streams independent streams.  Stream i is src[src_offsets[i] .. src_offsets[i+1]) (any alignment) and
 * must inflate to exactly dst_offsets[i+1] - dst_offsets[i] bytes at dst + dst_offsets[i]; both offset arrays live
 * on the device (n_streams + 1 entries, 8-byte aligned).  wrapper: 0 = raw RFC 1951, 1 = RFC 1950 (header checked,
 * FDICT refused, Adler-32 verified).  status[i] (device) = 0 or one SK_INFLATE_E_* code; a failed stream never stops
 * the others.  Replaces zlib.decompress per chunk / strip on the host (the reference leaves reading to zarr / skimage,
 * eval.py:61, 160-176).  All three block types, any number of blocks, empty stored blocks, every window size; bytes
 * after the end of a stream are ignored.  status[i] == 0 exactly when zlib inflates the stream without error to its
 * end and to the expected number of bytes (zlib's rules for code-length sets included).  The decoder reads nothing
 * outside a stream's src range and writes nothing outside its dst range whatever the bytes are; of a refused stream
 * the dst range holds an undefined prefix.  One wave per stream: the speed comes from many streams per call.  The
 * output depends on the stream alone.  Arguments are checked before the launch. */
int sk_inflate_streams(const uint8_t* src, const int64_t* src_offsets, int n_streams, uint8_t* dst,
                       const int64_t* dst_offsets, int wrapper, int32_t* status, void* stream);

/* Undoes TIFF predictor 2 (horizontal differencing) in place: n_rows rows of row_pixels pixels,
 * samples_per_pixel (1..16) samples of bytes_per_sample (1, 2, 4) little-endian bytes each; sums wrap modulo
 * 2^bits as libtiff's do.  rows is aligned to its samples. */
int sk_tiff_undo_predictor(void* rows, int64_t n_rows, int row_pixels, int samples_per_pixel, int bytes_per_sample,
                           void* stream);

/* ------------------------------------------------------------------------ *
 * Reading the reference's stores: Blosc-1 frames with the LZ4 codec
 * ------------------------------------------------------------------------ */

/* status[i] of sk_lz4_streams, status of sk_blosc_decode_host / sk_blosc_plan_host: 0, or why it was refused */
#define SK_LZ4_E_RANGE 1         /* a table row outside [0, src_bytes) / [0, dst_bytes), negative, of an unknown kind, or stored with src_len != dst_len */
#define SK_LZ4_E_INPUT 2         /* a token, a length byte, a literal run or an offset reaches past the end of the stream (a stream that ends right after a match included) */
#define SK_LZ4_E_OFFSET 3        /* offset 0, or an offset that reaches before the start of the output */
#define SK_LZ4_E_OUTPUT_LONG 4   /* the stream expands to more bytes than expected */
#define SK_LZ4_E_OUTPUT_SHORT 5  /* the input ended after a literal run before dst_len bytes were produced */
#define SK_BLOSC_E_HEADER 6      /* shorter than 16 bytes, version not 2, cbytes not the frame's length, nbytes not dst_bytes, typesize 0, blocksize 0 */
#define SK_BLOSC_E_CODEC 7       /* inner codec not lz4, bitshuffle, or byte shuffle with a typesize above 16 */
#define SK_BLOSC_E_FRAME 8       /* the block table, a block start or a split prefix reaches outside the frame, or a split block that does not divide */

#define SK_LZ4_KIND_LZ4 0        /* one LZ4 raw block */
#define SK_LZ4_KIND_STORED 1     /* the bytes as they are */

/* Expands n_streams independent streams.  table (device, int64 (n_streams, 5), 8-byte aligned) holds per stream
 * src_begin, src_len, dst_begin, dst_len, kind: src[src_begin .. + src_len) (any alignment) must expand to exactly
 * dst_len bytes at dst + dst_begin.  status[i] (device) = 0 or one SK_LZ4_E_* code: 0 exactly when the row lies
 * inside both buffers and the stream parses as an LZ4 raw block (token, literal length extended by 255s, literals,
 * 2-byte little-endian offset, match length extended likewise, + 4), ends at src_len after a literal run and has
 * produced dst_len bytes.  A failed stream never stops the others.  One wave64 workgroup per stream; matches read a
 * 64 KiB ring of the output in LDS, never dst.  Every row is checked in the kernel: nothing is read outside a row's
 * src range and nothing written outside its dst range whatever the bytes are; of a refused stream the dst range holds
 * an undefined prefix.  Arguments are checked before the launch.  No reference counterpart (numcodecs / c-blosc on the host). */
int sk_lz4_streams(const uint8_t* src, int64_t src_bytes, const int64_t* table, int n_streams, uint8_t* dst,
                   int64_t dst_bytes, int32_t* status, void* stream);

/* Undoes Blosc's byte shuffle: for every row (begin, bytes) of blocks (device, int64 (n_blocks, 2), 8-byte aligned),
 * with ne = bytes / typesize, dst[begin + e * typesize + j] = src[begin + j * ne + e] and the bytes % typesize tail
 * bytes are copied.  typesize 2..16, src != dst, begin of any alignment.  Nothing outside a block's range is read in
 * src or written in dst; rows with a negative begin or bytes <= 0 are left alone. */
int sk_blosc_unshuffle(const uint8_t* src, uint8_t* dst, const int64_t* blocks, int n_blocks, int typesize, void* stream);

/* HOST, no GPU work.  Walks one frame that must expand to dst_bytes: header and block-table checks and the walk over
 * the split prefixes, every offset checked against frame_bytes before it is used.  Fills streams (cap_streams rows of
 * 5, as sk_lz4_streams takes them, offsets relative to the frame and to its output) and blocks (cap_blocks rows of
 * begin, bytes: the blocks that are byte-shuffled) as far as the capacities reach; counts[0..3] = rows of each the
 * frame has, typesize, 1 if blocks have to be unshuffled.  *status = 0 or SK_BLOSC_E_*.  The one frame parser: the
 * host decoder and the device path's table both come from it. */
int sk_blosc_plan_host(const uint8_t* frame, int64_t frame_bytes, int64_t dst_bytes, int64_t* streams,
                       int64_t cap_streams, int64_t* blocks, int64_t cap_blocks, int64_t* counts, int32_t* status);

/* HOST, no GPU work.  Decodes a whole frame into dst[0 .. dst_bytes): the same walk, the same LZ4 decoder text as
 * the kernel compiled as host C++, the same acceptance rules and status codes.  *status = 0 or the first
 * SK_LZ4_E_* / SK_BLOSC_E_* code met; of a refused frame dst holds undefined bytes.  Thread-safe. */
int sk_blosc_decode_host(const uint8_t* frame, int64_t frame_bytes, uint8_t* dst, int64_t dst_bytes, int32_t* status);

/* ------------------------------------------------------------------------ *
 * --convert: eval()'s stores and .trch tensors -> the pages of a TIFF stack
 * ------------------------------------------------------------------------ */

#define SK_CONVERT_U8 0
#define SK_CONVERT_F16 1
#define SK_CONVERT_F32 2

#define SK_CONVERT_CAST 0   /* astype(np.uint8) */
#define SK_CONVERT_TRUNC 1  /* store array, max < 2: ((x + 1) / 2) * 255, truncated */
#define SK_CONVERT_ROUND 2  /* .trch tensor, min < 0: the same, .float().round() */

/* src: contiguous (C, X, Y, Z) of src_dtype (SK_CONVERT_U8 / _F16 / _F32); dst: contiguous (Z, X, Y, C) uint8, the
 * pages x.transpose(3, 1, 2, 0) gives; C = 1..4.  One pass, replacing the torch / numpy chain of
 * skoots/utils/convert_trch_to_tif.py:48-55 (mode 1), :59-65 (mode 2) and the transposes at :55 / :73.
 *   mode 0  plain cast: truncate toward zero, keep the low 8 bits (uint8: a copy).  The reference's astype(np.uint8)
 *           defines no result outside [0, 256): what this gives there is UNPINNED.
 *   mode 1  t = ((x + 1) / 2) * 255 with every operation rounded in the array's own float type (fp16: three fp16
 *           roundings; uint8: the add wraps in uint8, the division promotes to fp32), truncated; 0 where x == 0.
 *   mode 2  the same t, converted to fp32, rounded half to even; 0 where x == 0.
 * In modes 1 and 2 a t outside [0, 256) is unpinned in the same way (low 8 bits of the saturated int32).
 * No workspace.  Arguments are checked before the launch. */
int sk_convert_pages_u8(const void* src, int src_dtype, int mode, int C, int X, int Y, int Z, uint8_t* dst,
                        void* stream);

/* ------------------------------------------------------------------------ *
 * Multiscale pyramids: one pooling pass per level (ABI 31)
 * ------------------------------------------------------------------------ */

#define SK_POOL_MODE 0
#define SK_POOL_MEAN 1
#define SK_POOL_MAX 2

/* src: contiguous (X, Y, Z) of dtype, Z innermost; dst: contiguous (ceil(X / fx), ceil(Y / fy), ceil(Z / fz)) of the
 * same dtype; every factor 1 or 2, not all 1.  The block of an output voxel (xo, yo, zo) is the source voxels
 * [xo fx, xo fx + fx) x [yo fy, yo fy + fy) x [zo fz, zo fz + fz) that exist: at the far edge of an odd extent it is
 * clipped, so it holds n = 1, 2, 4 or 8 voxels.
 *   how = SK_POOL_MODE  dtype SK_I32 / SK_I16 / SK_U8: the value that occurs most often in the block; among values of
 *                       the same count the smallest in the dtype's order (signed for int32 / int16).  sparse != 0: zeros
 *                       are not counted unless the whole block is zero.  The result is defined by the counts of the
 *                       block's values alone, so it does not depend on the order in which a lane visits the block.
 *   how = SK_POOL_MEAN  dtype SK_U8 / SK_U16: (sum + n / 2) / n in integer arithmetic (round half up); sparse ignored.
 *   how = SK_POOL_MAX   dtype SK_U8 / SK_U16: the largest value; sparse ignored.
 * One launch, no workspace, nothing allocated; the same bits on every run.  Every argument is checked before the launch
 * (SK_ERR_ARG): null pointers, extents < 1, factors, how, the dtype of the reduction, element alignment,
 * ceil(X / fx) ceil(Y / fy) < 2^31. */
int sk_pool_volume(const void* src, int dtype, int X, int Y, int Z, int fx, int fy, int fz, int how, int sparse,
                   void* dst, void* stream);

/* ------------------------------------------------------------------------ *
 * Exact change of grid by any ratio per axis (ABI 32; no reference counterpart)
 * ------------------------------------------------------------------------ */

#define SK_RESAMPLE_NEAREST 0
#define SK_RESAMPLE_LINEAR 1
#define SK_RESAMPLE_AREA 2

#define SK_RESAMPLE_PATH_GATHER 0 /* nearest on every axis: no arithmetic */
#define SK_RESAMPLE_PATH_ACC32 1  /* weighted sums in 32 bits: W vmax < 2^32 after the reduction */
#define SK_RESAMPLE_PATH_ACC64 2  /* weighted sums in 64 bits */

/* src: contiguous (X, Y, Z) of dtype, Z innermost; dst: contiguous (Xo, Yo, Zo) of the same dtype.  Both cover the same
 * physical extent (pixel-centre convention, no align_corners).  An axis of n source voxels and m output voxels has one
 * operator: per output index i a list of integer taps (k, w) and a total W.
 *   SK_RESAMPLE_NEAREST  one tap, k = ((2 i + 1) n) div (2 m), w = 1, W = 1: the source voxel that holds the output
 *                        voxel's centre; a centre on a boundary takes the upper voxel.
 *   SK_RESAMPLE_LINEAR   num = (2 i + 1) n - m, den = 2 m, k0 = floor(num / den), r = num - k0 den; taps
 *                        (clamp(k0), den - r) and (clamp(k0 + 1), r), clamped to 0 .. n - 1; W = den.
 *   SK_RESAMPLE_AREA     output cell i covers [i n, (i + 1) n) in units of 1 / m of a source voxel; for k from (i n) div m
 *                        to ceil((i + 1) n / m) - 1 the weight is min((k + 1) m, (i + 1) n) - max(k m, i n); W = n.
 * The output voxel is floor((2 S + W) / (2 W)), S the sum of wx wy wz v over the product of the three tap lists and
 * W = Wx Wy Wz: the exact quotient rounded to nearest, halves up.  The weights of an axis are divided by a common factor
 * first (linear: gcd(2 m, 2 n, |n - m|), area: gcd(n, m)), which changes no result.  Integers only: the same bits on
 * every run.  dtype: SK_U8 / SK_U16 for every operator; SK_I32 / SK_I16 with SK_RESAMPLE_NEAREST on all three axes.
 *
 * workspace: sk_resample_workspace_bytes(...) bytes of device memory, 4-byte aligned, for the three tap tables, which a
 * prologue launch per axis fills on the same stream; nothing is allocated, nothing comes back to the host.  Limits,
 * checked before any launch (SK_ERR_ARG; the workspace query then returns 0): null pointers, extents < 1 or > 2^30, a ratio
 * outside n / 8 <= m <= 8 n (halve with sk_pool_volume first), operator codes, the dtype of the operators, the unreduced
 * Wx Wy Wz (linear 2 m, area n, nearest 1) times the dtype's largest value >= 2^63, Xo Yo >= 2^31, more than 65535 z chunks
 * (a chunk is at least 64 output voxels for Zo >= 64), element alignment, a workspace that is too small.
 * sk_resample_path: HOST, no GPU needed: which kernel the launch runs, SK_RESAMPLE_PATH_*, or SK_ERR_ARG. */
size_t sk_resample_workspace_bytes(int dtype, int X, int Y, int Z, int Xo, int Yo, int Zo, int op_x, int op_y, int op_z);
int sk_resample_path(int dtype, int X, int Y, int Z, int Xo, int Yo, int Zo, int op_x, int op_y, int op_z);
int sk_resample_volume(const void* src, void* dst, int dtype, int X, int Y, int Z, int Xo, int Yo, int Zo, int op_x, int op_y,
                       int op_z, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------ *
 * Exact rank and tap filters (ABI 33; the reference declares median_filter, mean_filter, dilate,
 * binary_erosion and gauss_filter in skoots/lib/morphology.py, and the first three cannot run)
 * ------------------------------------------------------------------------ */

#define SK_FILTER_BORDER_ZERO 0   /* a sample outside 0 <= i < n is 0 */
#define SK_FILTER_BORDER_EDGE 1   /* clamp(i, 0, n - 1) */
#define SK_FILTER_BORDER_MIRROR 2 /* j = i mod 2 n (non-negative); j < n ? j : 2 n - 1 - j: numpy's symmetric */

#define SK_FILTER_PATH_EXTREME 0     /* rank 0 or n - 1: one min / max pass over the window */
#define SK_FILTER_PATH_RADIX 1       /* any other rank: bitwise radix descent over the key bits */
#define SK_FILTER_PATH_ACC32 2       /* taps, sums in 32 bits: W vmax < 2^32 */
#define SK_FILTER_PATH_ACC64 3       /* taps, sums in 64 bits */
#define SK_FILTER_PATH_NETWORK 4     /* the median of radius (1, 1, 0) and (1, 1, 1): a min / max exchange network */
#define SK_FILTER_PATH_VECTOR_ROWS 8 /* or-ed in: rows are dword multiples on dword-aligned bases, 16-byte loads and stores */

#define SK_FILTER_METHOD_AUTO 0    /* what sk_filter_path names */
#define SK_FILTER_METHOD_RADIX 1   /* the radix descent for every rank and window, the ends included */
#define SK_FILTER_METHOD_NETWORK 2 /* the exchange network; refused where it is not built */

/* in: contiguous (X, Y, Z) of dtype, Z innermost; out: the same shape and dtype, another buffer.  The border rule gives
 * the source index of any integer i on an axis of extent n, windows wider than the volume included.
 * sk_filter_rank: radii rx, ry, rz in 0 .. 2; the window of an output voxel holds n = (2 rx + 1)(2 ry + 1)(2 rz + 1)
 * bordered samples and the output is the rank-th smallest of them, rank in 0 .. n - 1 counted from 0.  dtype SK_U8,
 * SK_U16 or SK_F32; float32 is ordered by value (-0.0 and 0.0 are equal and either may come back, infinities are
 * ordinary values, a NaN anywhere is outside the definition).  method chooses the selection, SK_FILTER_METHOD_*: every
 * method gives the same bits, and the forced ones exist so that they can be timed and tested against each other.
 * sk_filter_taps: per axis an odd number 1 .. 17 of integer taps >= 0 whose sum W_axis is in 1 .. 4096 (HOST arrays,
 * read before the call returns).  The output is (S + W / 2) / W in integers, S the sum of wx wy wz v over the product
 * of the three lists applied to the bordered samples, W = Wx Wy Wz: the exact weighted mean rounded to nearest, halves
 * up, rounded once.  dtype SK_U8 or SK_U16.  Sums are 32-bit where W vmax < 2^32 and 64-bit otherwise; both are exact.
 * One launch on the caller's stream, no workspace, nothing allocated; the same bits on every run.  Checked before the
 * launch (SK_ERR_ARG): null pointers, in == out, element alignment, dtype, extents < 1 or > 2^30, border, radius, rank,
 * method,
 * tap counts, negative taps, tap sums, more than 2^31 - 1 workgroups.
 * sk_filter_path: HOST, no GPU needed: the kernel a geometry takes, SK_FILTER_PATH_* (or SK_ERR_ARG).  With any tap
 * list not NULL it answers for sk_filter_taps (rx, ry, rz and rank are ignored), else for sk_filter_rank.  aligned:
 * whether in and out are dword aligned.  sk_filter_tile(0 / 1 / 2): the rank kernels' tile, rows in x, rows in y and
 * bytes along z (4, 8, 128), for tests that place their sizes around it. */
int sk_filter_tile(int axis);
int sk_filter_path(int dtype, int X, int Y, int Z, int rx, int ry, int rz, int rank, const int* taps_x, int nx,
                   const int* taps_y, int ny, const int* taps_z, int nz, int aligned);
int sk_filter_rank(const void* in, void* out, int dtype, int X, int Y, int Z, int rx, int ry, int rz, int rank, int border,
                   int method, void* stream);
int sk_filter_taps(const void* in, void* out, int dtype, int X, int Y, int Z, const int* taps_x, int nx, const int* taps_y,
                   int ny, const int* taps_z, int nz, int border, void* stream);

/* ------------------------------------------------------------------------ *
 * Tile histograms and look-up-table transforms (ABI 34; not in the reference)
 * ------------------------------------------------------------------------ */

#define SK_EQUALIZE_HIST_ONE 0    /* a workgroup counts one tile in LDS, several copies of the table */
#define SK_EQUALIZE_HIST_PLANES 1 /* tz == 1: a table per z-plane, a chunk of planes per workgroup */
#define SK_EQUALIZE_HIST_ZTILES 2 /* tz >= 2: several z-tiles per workgroup */
#define SK_EQUALIZE_HIST_GLOBAL 3 /* tile columns of fewer than 16 rows: 64-bit global atomics, no LDS */

#define SK_EQUALIZE_APPLY_Z_ONE 0    /* bits 0 .. 1: one table along z */
#define SK_EQUALIZE_APPLY_Z_TILE 1   /*   the table of the voxel's own z-tile */
#define SK_EQUALIZE_APPLY_Z_INTERP 2 /*   two z-tiles, weighted */
#define SK_EQUALIZE_APPLY_XY 4       /* or-ed in: x or y interpolates, four corner columns */
#define SK_EQUALIZE_APPLY_ACC32 8    /* or-ed in: weighted sums in 32 bits; neither ACC bit: a plain look-up */
#define SK_EQUALIZE_APPLY_ACC64 16   /* or-ed in: weighted sums in 64 bits */
#define SK_EQUALIZE_APPLY_GATHER 32  /* or-ed in: cells of fewer than 16 rows, tables read from global memory, not staged */

/* in: contiguous (X, Y, Z) of dtype SK_U8 or SK_U16, Z innermost.  bin(v) = min(v >> shift, bins - 1); SK_U8 takes
 * bins = 256 and shift = 0, SK_U16 bins in {256, 1024, 4096} and shift in 0 .. 8.
 * Tiles: tx, ty, tz >= 1, 0 = the whole axis, a side larger than the extent = the extent; with the side t so replaced,
 * tile k of an axis of extent n covers [k t, min((k + 1) t, n)) and there are ceil(n / t) of them.
 * sk_tile_histograms: out_counts is an int64 device table (nx, ny, nz, bins), zeroed by the call on the stream;
 * [kx, ky, kz, b] counts the voxels of that tile with bin(v) == b.  Exact for every volume the extents admit (a
 * workgroup counts fewer than 2^32 voxels in its 32-bit LDS counters and adds them to the table with 64-bit integer
 * atomics) and the same on every run.
 * sk_apply_tile_luts: luts is an int32 device table (nx, ny, nz, bins) with values in 0 .. the dtype's maximum (the
 * CALLER's promise: values are used modulo 2^16).  interpolate == 0: out = luts[tile of the voxel][bin(v)].
 * interpolate == 1: per axis, for index i, side t and n tiles, p = 2 i + 1 - t, k0 = floor(p / (2 t)), w1 = p - 2 t k0,
 * w0 = 2 t - w1; the two tiles are clamp(k0, 0, n - 1) with weight w0 and clamp(k0 + 1, 0, n - 1) with weight w1 (tile
 * centres at their nominal places, clipped tiles included; beyond the first and the last centre the nearest tile
 * alone).  out = (S + W / 2) / W in integers, S the sum over the 8 corner tiles of wx wy wz luts[corner][bin(v)],
 * W = 8 tx ty tz: the exact weighted mean rounded to nearest, halves up, rounded once.
 * An axis with one tile, or with t == 1, has both weights on one tile: S = 2 t S' and W = 2 t W' with S', W' the sums
 * without that axis, and (2 t S' + t W') / (2 t W') = floor((2 S' + W') / (2 W')) = (S' + W' / 2) / W' (for odd W',
 * 2 S' + W' is odd and no multiple of 2 W', so the missing half does not matter).  The kernels therefore sum over the
 * axes that do interpolate only, in 32 bits where that W' times the dtype's maximum is below 2^32 and in 64 bits
 * otherwise; both are exact.  W' times the maximum must stay below 2^62.
 * One launch each on the caller's stream (the histograms after a memset of the table), no workspace, nothing
 * allocated.  Checked before any launch (SK_ERR_ARG): null pointers, in == out, element alignment (8 bytes for
 * out_counts, 4 for luts), dtype, extents < 1 or > 2^30, negative tile sides, bins, shift, interpolate, more than
 * 2^31 - 1 workgroups.
 * sk_equalize_path: HOST, no GPU needed: the kernel a geometry takes, which = 0 SK_EQUALIZE_HIST_* of the histograms,
 * which = 1 the SK_EQUALIZE_APPLY_* bits of the apply pass (or SK_ERR_ARG). */
int sk_equalize_path(int which, int dtype, int X, int Y, int Z, int tx, int ty, int tz, int bins, int shift, int interpolate);
int sk_tile_histograms(const void* in, int dtype, int X, int Y, int Z, int tx, int ty, int tz, int bins, int shift,
                       long long* out_counts, void* stream);
int sk_apply_tile_luts(const void* in, void* out, int dtype, int X, int Y, int Z, int tx, int ty, int tz, const int* luts, int bins,
                       int shift, int interpolate, void* stream);

/* ------------------------------------------------------------------------ *
 * Instance measurements: volume, box, moments and face area of every instance
 * ------------------------------------------------------------------------ */

/* One pass over an (X, Y, Z) int32 instance mask (z fastest) measures every instance at once; the reference sketches
 * the step with one full-volume mask per id (skoots/validate/compare.py: stats_per_instance) and one Python iteration
 * per id (validate/lib.py: mask_to_bbox).  lut (max_id + 1 entries) maps a raw id to its row 1..N as in sk_mask_iou;
 * ids <= 0 or above max_id, and rows outside 1..N, are background.  Row r fills
 *   sums[(r - 1) * 13 ..]  int64: n, Sx, Sy, Sz, Sxx, Syy, Szz, Sxy, Sxz, Syz over the voxel indices, then fx, fy, fz,
 *                          the exposed faces whose normal lies along x / y / z;
 *   boxes[(r - 1) * 6 ..]  int32: min x, y, z, then max x, y, z, inclusive (mask_to_bbox's convention); a row without
 *                          voxels keeps INT32_MAX / -1.
 * A face of a voxel of row a is exposed when the neighbour across it lies outside the volume or has another row,
 * background included: a face between two instances counts once for each.  The entry point initialises both outputs
 * itself (stream-ordered) and measures in one launch; background voxels take no atomic, and only integer atomics are
 * used, so the result is exact and the same on every run.  Checked before anything is written: extents and N not
 * negative, X Y Z max(X, Y, Z)^2 < 2^63 (the second moments stay inside int64), no NULL pointer.  An empty volume or
 * N == 0 returns SK_OK and writes nothing.  sk_instance_stats_row_values(0) = 13 and (1) = 6: the int64 / int32
 * values per row, for a caller that sizes the buffers. */
int sk_instance_stats_row_values(int which);
int sk_instance_stats(const int32_t* labels, int X, int Y, int Z, const int32_t* lut, int max_id, int N, int64_t* sums,
                      int32_t* boxes, void* stream);

/* Marching-cubes cell classes of every instance (ABI 15): what the reference measures with
 * skimage.measure.marching_cubes on one binary mask per id (skoots/validate/stats.py:30-48), as one pass.  labels, lut,
 * max_id and N are those of sk_instance_stats.  Cell (x, y, z) is the 2 x 2 x 2 block of voxels with that low corner;
 * bit b of its configuration for row a is set when the voxel (x + (b & 1), y + ((b >> 1) & 1), z + ((b >> 2) & 1)) has
 * row a.  For every row a among the corners of a cell whose configuration is not 255,
 *   cells[(a - 1) * n_classes + class_of[configuration]] += 1      (int64),
 * so a cell shared by k instances counts once for each of them.  class_of: 256 bytes in device memory; an entry
 * >= n_classes is skipped.  closed = 0 has the cells 0 .. extent - 2 of every axis (a surface cut by the volume's face
 * stays open, as in the reference; no cell when an extent is 1); closed = 1 has -1 .. extent - 1, the mask padded with one
 * layer of background, and a corner outside the volume matches no row.  The entry point zeroes cells itself
 * (stream-ordered); integer atomics only, so the result is exact and the same on every run.  Checked before anything is
 * written: extents, N and max_id not negative, X Y Z < 2^62, n_classes in 1..32, closed 0 or 1, no NULL pointer,
 * pointers aligned to their elements.  An empty volume or N == 0 returns SK_OK and writes nothing. */
int sk_instance_mesh_cells(const int32_t* labels, int X, int Y, int Z, const int32_t* lut, int max_id, int N,
                           const uint8_t* class_of, int n_classes, int closed, int64_t* cells, void* stream);

/* The marching-cubes mesh of every instance (ABI 18): the triangles whose area section 21 measures,
 * written out.  labels, lut, max_id, N, closed, the cells and "a cell shared by k instances belongs to each of them" are
 * those of sk_instance_mesh_cells.  tri_table: 256 uint64 in device memory, one per configuration: bits 60 .. 63 the
 * number of triangles (more than 5 counts as 5), bits 4 i .. 4 i + 3 edge number i % 3 of triangle i / 3
 * (skoots_amd/validate/mc_triangles.py; edge e = 4 axis + k starts at the k-th corner, ascending, whose bit `axis` is
 * clear).  The voxel key of (x, y, z) is its linear index in the volume padded by one layer,
 * ((x + 1) (Y + 2) + y + 1) (Z + 2) + z + 1.  A vertex of row a is a cell edge (an axis-neighbour voxel pair inside
 * the corner range of the cells) whose two voxels have exactly one of row a; its edge key is the voxel key of its low
 * voxel x 3 + axis, and its position the midpoint of the two voxels.
 * sk_instance_mesh_count: counts[(a - 1) * 2] = vertices and counts[(a - 1) * 2 + 1] = triangles of row a (int64; the
 * entry point zeroes counts itself, stream-ordered).
 * sk_instance_mesh_emit: one record of 2 int64 per vertex, (row, edge key), and one of 5 int64 per triangle,
 * (row, edge key of its three vertices in scikit-image's winding, order key = voxel key of the cell's low corner x 8 +
 * the triangle's position in its configuration), in no particular order, at slots taken with one global atomic per
 * workgroup tile and kind.  A record whose slot is at or beyond its capacity (in records) is not written;
 * produced[0] / produced[1] (zeroed by the entry point) are the vertex / triangle records the volume has, whatever the
 * capacities, so a caller compares them with the count pass.  vertices / triangles may be NULL at capacity 0.
 * Integer atomics only: the SET of records is the same on every run.  Checked before anything is launched or written:
 * extents, N, max_id and capacities not negative, X Y Z < 2^62 and (X + 2) (Y + 2) (Z + 2) < 2^60 (the keys stay in
 * int64), capacities < 2^58, closed 0 or 1, no NULL pointer, pointers aligned to their elements.  An empty volume or
 * N == 0 returns SK_OK and writes nothing; an extent of 1 in open mode has no cell: zeros. */
int sk_instance_mesh_count(const int32_t* labels, int X, int Y, int Z, const int32_t* lut, int max_id, int N,
                           const uint64_t* tri_table, int closed, int64_t* counts, void* stream);
int sk_instance_mesh_emit(const int32_t* labels, int X, int Y, int Z, const int32_t* lut, int max_id, int N,
                          const uint64_t* tri_table, int closed, int64_t* vertices, int64_t vertex_capacity,
                          int64_t* triangles, int64_t triangle_capacity, int64_t* produced, void* stream);

/* Exact squared Euclidean distance transform of every instance at once (ABI 17).  labels, lut,
 * max_id and N are those of sk_instance_stats; r(v) is the row of voxel v (1 .. N, 0 for background).  wx, wy, wz are
 * the squares of the voxel spacing, fl(sx sx) and so on, formed in double by the caller.  For a voxel p with r(p) > 0
 *   dist2[p] = min over voxels q with r(q) != r(p) of  fl(wx dx^2 + fl(wy dy^2 + wz dz^2)),   dx = px - qx, ...
 * where every square is an exact integer converted to double and every product and sum is rounded once (no fused
 * multiply-add; w (d d), never (w d) d); dist2[p] = 0 where r(p) = 0.  Another instance is "not this instance" exactly
 * like background: a face shared by two instances bounds both.  closed = 0 counts the voxels of the volume only
 * (scipy.ndimage.distance_transform_edt's meaning), and a voxel whose row is the only value of the whole volume gets
 * +inf; closed = 1 measures the volume padded with one layer of background on all six sides.  The minimum is nested
 * and rounding is monotone, so the three passes of the implementation (z, y, x; each a pruned walk along its axis)
 * give exactly this value at any spacing; at integer-valued spacings sqrt(dist2) equals scipy's result bit for bit.
 * dist2 and scratch: X Y Z doubles each, distinct; the passes go dist2 -> scratch -> dist2.  row_max (N, may be NULL):
 * row_max[r - 1] is the bit pattern of the largest dist2 of row r (non-negative doubles order like unsigned integers,
 * +inf last, so a 64-bit integer atomic max is exact and independent of the order of arrival), 0 for a row without
 * voxels; the entry point zeroes it itself (stream-ordered).  Nothing accumulates in floating point: the outputs are
 * the same on every run.  Checked before anything is launched or written: extents, N and max_id not negative, every
 * extent <= 2^26 (d^2 exact in double), X Y Z < 2^62, closed 0 or 1, the weights finite and > 0, no NULL pointer but
 * row_max, pointers aligned to their elements, dist2 != scratch.  An empty volume or N == 0 returns SK_OK and writes
 * nothing.
 * sk_label_edt_pass is one of the three passes, under the same checks: axis 2 (z; src is not read and may be NULL)
 * writes dst = the minimum of w dz^2 along z, axis 1 and 0 write dst = min over the axis of fl(w d^2 + src(q)); row_max
 * (may be NULL) is zeroed and filled from dst.  sk_label_edt is the passes 2, 1, 0 with wz, wy, wx;
 * tools/bench_edt.py times them one by one. */
int sk_label_edt_pass(const int32_t* labels, int X, int Y, int Z, const int32_t* lut, int max_id, int N, int axis,
                      double w, int closed, const double* src, double* dst, uint64_t* row_max, void* stream);
int sk_label_edt(const int32_t* labels, int X, int Y, int Z, const int32_t* lut, int max_id, int N, double wx, double wy,
                 double wz, int closed, double* dist2, double* scratch, uint64_t* row_max, void* stream);

/* Surface voxels of every instance, and exact distances between surface voxel sets (ABI 19): what
 * validate/compare.py: compare() is made of.  labels, lut, max_id and N are those of sk_instance_stats; r(v) is the row
 * of voxel v, 1 .. N, and 0 for background, unlisted ids and every position outside the volume.
 * A surface voxel of row a is a voxel v with r(v) = a of whose six face neighbours at least one has a row != a; outside
 * counts as row 0, so no instance has an empty surface (scipy: m & ~binary_erosion(m), default structure,
 * border_value 0).  Its surface key is (a - 1) X Y Z + ((x Y + y) Z + z), int64: sorted ascending, the keys of a row are
 * one contiguous segment in x-major order, and key mod X Y Z is the voxel.
 * sk_instance_surface_count: counts[a - 1] = surface voxels of row a (int64; zeroed by the entry point, stream-ordered).
 * sk_instance_surface_emit: the surface keys, in no particular order, at slots taken with one global atomic per
 * workgroup and tile.  A key whose slot is at or beyond `capacity` is not written; produced[0] (zeroed by the entry
 * point) is the number of surface voxels the volume has, whatever the capacity.  keys may be NULL at capacity 0.
 * Integer atomics only: the SET of keys is the same on every run.  Checked before anything is launched or written:
 * extents, N, max_id and capacity not negative, every extent <= 2^26, N X Y Z < 2^63 (the keys stay in int64),
 * capacity < 2^60, no NULL pointer, pointers aligned to their elements.  An empty volume or N == 0 returns SK_OK and
 * writes nothing.
 *
 * sk_surface_distances: q_keys / t_keys are keys as above (only key mod X Y Z is used), cut into q_segments / t_segments
 * segments by q_offsets / t_offsets (segments + 1 int64 each: segment s is [offsets[s], offsets[s + 1])).  pairs: P x 2
 * int32, the query segment and the target segment of pair k, 0-based; a segment may appear in any number of pairs.
 * out_offsets: P + 1 int64, out_offsets[0] = 0 and out_offsets[k + 1] - out_offsets[k] = the queries of pair k.  With
 * (wx, wy, wz) = (fl(sx sx), fl(sy sy), fl(sz sz)) formed in double by the caller, for the i-th key q of the query
 * segment of pair k and its target segment T
 *   d2[out_offsets[k] + i] = min over t in T of  fl(wx dx^2 + fl(wy dy^2 + wz dz^2)),   dx = qx - tx, ...
 * where every square is an exact integer converted to double and every product and sum is rounded once (no fused
 * multiply-add; w (d d), never (w d) d), as in sk_label_edt; +inf when T is empty.  A minimum does not depend on the
 * order, and the pruning of the implementation skips only candidates that cannot be smaller (rounding is monotone), so
 * the value is exactly this at any spacing and for keys in any order; sorted keys make the pruning effective.  At
 * integer-valued spacings sqrt(d2) equals scipy.ndimage.distance_transform_edt(~T, sampling) at q bit for bit.  Every
 * output has one writer and nothing accumulates: the same bits on every run.  All arrays are device memory.  Checked
 * before anything is launched or written: extents, P and segment counts not negative, every extent <= 2^26, the weights
 * finite and > 0, pointers aligned to their elements, no NULL pointer (keys and d2 may be NULL where they have no
 * element); then the offsets and pairs are read back (the call synchronises the stream) and checked: offsets not
 * negative and monotone, every pair inside the segment counts, out_offsets as stated.  That q_keys / t_keys hold
 * q_offsets[q_segments] / t_offsets[t_segments] elements and d2 out_offsets[P] is the caller's to ensure: the lengths
 * are not arguments (validate/lib.py: surface_distances checks them).  SK_ERR_CAPACITY when the host copies of the
 * tables cannot be allocated.  P == 0 or no query returns SK_OK and writes nothing.  The work is sum over pairs of queries x targets at most and has no other bound: the caller
 * limits a call (validate/lib.py: LAUNCH_BUDGET).  sk_surface_distance_tile(): the target voxels per LDS tile (1024),
 * for tests that place their sizes around it. */
int sk_surface_distance_tile(void);
int sk_instance_surface_count(const int32_t* labels, int X, int Y, int Z, const int32_t* lut, int max_id, int N,
                              int64_t* counts, void* stream);
int sk_instance_surface_emit(const int32_t* labels, int X, int Y, int Z, const int32_t* lut, int max_id, int N,
                             int64_t capacity, int64_t* keys, int64_t* produced, void* stream);
int sk_surface_distances(const int64_t* q_keys, const int64_t* q_offsets, int q_segments, const int64_t* t_keys,
                         const int64_t* t_offsets, int t_segments, const int32_t* pairs, int P,
                         const int64_t* out_offsets, int X, int Y, int Z, double wx, double wy, double wz, double* d2,
                         void* stream);

/* ------------------------------------------------------------------------ *
 * flood_and_stitch (skoots/utils/flood_and_stitch.py)
 * ------------------------------------------------------------------------ */

/* flood_and_stitch.py:63-69 (scipy.ndimage.label on every slice): P planes of H x W uint8 (foreground = nonzero),
 * labelled 4-connected, every plane on its own, all planes in one launch sequence.  Voxel (p, h, w) is read at
 * mask[p in_sp + h in_sh + w in_sw] and written at labels[p out_sp + h out_sh + w out_sw] (element strides, all
 * positive), so any axis of a contiguous volume is a plane axis in place; the kernels are tuned for in_sw = out_sw = 1.
 * Ids are GLOBAL: 1 + the component's rank among all components in (plane, row, column) order of first voxels, so
 * plane p owns offsets[p] + 1 .. offsets[p + 1] in scipy's order.  offsets: P + 1 int32 (exclusive prefix of the
 * planes' component counts), *total = offsets[P]; both device.  P H W < 2^31 - 4096, and the planes' 16 x 64 tiles
 * and their 2048-voxel chunks (a plane's last one may be partial) number at most 2^22 each: a workgroup per tile and per
 * chunk, so tens of millions of tiny planes are refused, not launched.  workspace: the query's bytes (0 for extents the
 * entry point refuses). */
size_t sk_label_planes_workspace_bytes(int P, int H, int W);
int sk_label_planes(const uint8_t* mask, int P, int H, int W, int64_t in_sp, int64_t in_sh, int64_t in_sw, int32_t* labels,
                    int64_t out_sp, int64_t out_sh, int64_t out_sw, int32_t* offsets, int32_t* total, void* workspace,
                    size_t workspace_bytes, void* stream);

/* flood_and_stitch.py:93-101 for every label of every slice at once: one row (id_a, id_b, n) per pair of components of
 * planes p and p + 1 of the global-id labels (strides as above) that share n > 0 voxel positions; one launch for all
 * plane pairs.  rows: capacity x 3 int32, compacted, in no particular order.  The pairs are counted in an
 * open-addressing table of `capacity` slots inside `workspace` (the query's bytes, 8-byte aligned; zeroed here).
 * counts (3 uint32, device): [0] pairs stored, [1] 0 if every pair found a slot; otherwise the refused pairs, each
 * counted once per top-left corner of its overlap region -- exact where every such region has one corner, never too
 * small otherwise (the exact number of distinct refused pairs would need the very table that is full); [2] rows
 * written = [0].  With counts[1] != 0 the rows are incomplete: run again with capacity >= 2 (counts[0] + counts[1]). */
size_t sk_plane_overlaps_workspace_bytes(int capacity);
int sk_plane_overlaps(const int32_t* labels, int P, int H, int W, int64_t sp, int64_t sh, int64_t sw, int32_t* rows, int capacity,
                      uint32_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/* flood_and_stitch.py:74-128, the two greedy stitching passes, on tables only (stitch_host.cpp; plain C++, every
 * pointer HOST).  offsets_host: n_planes + 1 entries as sk_label_planes writes them; rows_host: n_rows x 3 as
 * sk_plane_overlaps writes them, sorted by (id_a, id_b).  lut_host[id] (offsets[n_planes] + 1 entries, lut[0] = 0) = the
 * label component `id` carries after both passes (before the final renumbering), *max_label_host the largest.
 * SK_ERR_ARG for malformed tables, SK_ERR_CAPACITY if a new id would pass INT32_MAX. */
int sk_stitch_walk_host(const int32_t* offsets_host, int n_planes, const int32_t* rows_host, int64_t n_rows, int32_t* lut_host,
                        int32_t* max_label_host);

/* ------------------------------------------------------------------------ *
 * Connected pieces of a label volume (ABI 20; no reference counterpart)
 * ------------------------------------------------------------------------ */

/* sk_label_components: the connected pieces of every value of an (X, Y, Z) int32 volume at once.  Two voxels are joined
 * when they are neighbours and hold the same value.  which = 1 labels the positive values at `connectivity` 6, 18 or 26
 * (the 3, 9 or 13 backward neighbours of a voxel); which = 0 labels the zero voxels, always 6-connected (connectivity
 * must still be one of the three).  Voxels of the other kind -- and negative values in either mode -- get piece 0.
 * ranks: X Y Z int32, the piece of every voxel, 1 .. P in the raster (C) order of the pieces' first voxels over the
 * whole volume: for a one-value mask scipy.ndimage.label's numbering.  *n_components = P (device).  parent: X Y Z int32
 * of scratch that ends as the voxel index of the first voxel of every voxel's piece, -1 for the other kind.  workspace:
 * the query's bytes (0 for extents the entry point refuses).  Extents must be positive and X Y Z < 2^31: parents are
 * int32 voxel indices.  Stream-ordered, no allocation, no workgroup waits for another; the result is the same on every
 * run. */
size_t sk_label_components_workspace_bytes(int X, int Y, int Z);
int sk_label_components(const int32_t* labels, int X, int Y, int Z, int connectivity, int which, int32_t* parent,
                        int32_t* ranks, int32_t* n_components, void* workspace, size_t workspace_bytes, void* stream);

/* sk_component_table: one int64 row per piece of `piece` (the ranks above, pieces 1 .. P; other values are skipped) from
 * one pass with integer atomics only, so the rows are the same on every run.  rows: P x sk_component_table_row_values()
 * (= 6), written whole by the entry point:
 *   [0] value             the value of `labels` the piece's voxels hold (0 for a zero piece)
 *   [1] voxels            [2] first_voxel  the smallest voxel index (x Y + y) Z + z; -1 for a row no voxel names
 *   [3] border_bits       bit 0 / 1: a voxel at x = 0 / X - 1, bit 2 / 3: y = 0 / Y - 1, bit 4 / 5: z = 0 / Z - 1
 *   [4] min_neighbour_id  [5] max_neighbour_id  zero pieces only: the smallest and the largest positive value among the
 *                         6-neighbours of the piece's voxels, both 0 when there is none; equal when the pocket touches
 *                         exactly one id.  0 for the pieces of positive values.
 * P == 0 returns SK_OK and writes nothing. */
int sk_component_table_row_values(void);
int sk_component_table(const int32_t* labels, const int32_t* piece, int X, int Y, int Z, int P, int64_t* rows, void* stream);

/* out[v] = lut[piece[v]] for n voxels (0 where piece[v] is outside [0, n_lut)); with only_pieces != 0 only the voxels
 * with piece[v] > 0 are written and the others keep what `out` holds: the fill step of a clean-up. */
int sk_apply_piece_lut(const int32_t* piece, const int32_t* lut, int n_lut, int32_t* out, int64_t n, int only_pieces,
                       void* stream);

/* ------------------------------------------------------------------------ *
 * Geodesic assignment (ABI 27; no reference counterpart)
 * ------------------------------------------------------------------------ */

/* What utils/split.py cuts a fused instance with.  Definition:
 *   labels and seeds are (X, Y, Z) int32 volumes, Z fastest; costs = (cx, cy, cz) are integers in 1..255.
 *   A path is a chain of 6-neighbours that all hold the same positive `labels` value.  Its cost is the sum of its steps,
 *   cx for a step along x, cy along y, cz along z.
 *   For every voxel v with labels[v] > 0, cost[v] is the smallest path cost to v from any voxel s that holds a seed
 *   (seeds[s] > 0), and owner[v] the smallest `seeds` value among the seeds that attain that cost.
 *   A voxel that is itself a seed has cost 0.
 *   A voxel that no seed of its own value reaches has owner = 0 and cost = -1.  So does the background (and a seed that
 *   lies on the background seeds nothing).
 *   max_cost (-1 = none): a voxel further away than max_cost counts as unreached.
 * This is the unique fixed point of key(v) = min(own seed, min over same-valued 6-neighbours u of key(u) + step) over the
 * pair (cost, seed) compared lexicographically; adding to the cost alone keeps that order, so the result does not depend
 * on the order of execution and is the same on every run.
 *
 * The state is one 64-bit key per voxel, cost << 32 | seed, all ones for "none", in TWO buffers of X Y Z words: a round
 * reads one and writes the other, so a key is never read while it is written.  flags: 2 * sk_geodesic_tiles(X, Y, Z)
 * int32 ("this tile changed in the round before", two alternating copies; a tile whose own flag and whose six face
 * neighbours' flags are clear leaves at once).
 *   sk_geodesic_init    keys <- the seeds, both copies of the flags, *error <- 0, or 1 when either volume holds a negative
 *                       value (device word; the caller refuses the result);
 *   sk_geodesic_rounds  rounds first_round .. first_round + n_rounds - 1, one launch each, 1 <= n_rounds <=
 *                       sk_geodesic_max_rounds(); an even round reads keys_a and writes keys_b, an odd one the other way,
 *                       so first_round continues where the call before stopped (0 after init, with the seeds in
 *                       keys_a).  changed[k] (device, n_rounds int32, zeroed by the call) <- the tiles round
 *                       first_round + k lowered a key in.  Once a round has changed nothing both buffers hold the
 *                       answer and further rounds change nothing.  The caller loops: a round settles at least one more
 *                       voxel for good, so X Y Z + 1 rounds always suffice; the tiles a shortest path crosses, re-entries
 *                       counted, are what it takes.
 *   sk_geodesic_finish  keys -> owner and cost as defined above.
 * Refused before anything is launched (SK_ERR_ARG): extents not positive, X Y Z >= 2^31, a cost outside 1..255,
 * max(costs) X Y Z >= 2^31 (every cost stays an int32), max_cost < -1, NULL or misaligned pointers, keys_a == keys_b.
 * Stream-ordered, no allocation, no synchronisation; no workgroup waits for another. */
int sk_geodesic_tiles(int X, int Y, int Z);
int sk_geodesic_max_rounds(void);
int sk_geodesic_init(const int32_t* labels, const int32_t* seeds, int X, int Y, int Z, uint64_t* keys, int32_t* flags,
                     int32_t* error, void* stream);
int sk_geodesic_rounds(const int32_t* labels, int X, int Y, int Z, int cx, int cy, int cz, int64_t max_cost, uint64_t* keys_a,
                       uint64_t* keys_b, int32_t* flags, int first_round, int n_rounds, int32_t* changed, void* stream);
int sk_geodesic_finish(const uint64_t* keys, int64_t n, int32_t* owner, int32_t* cost, void* stream);

/* ------------------------------------------------------------------------ *
 * Nearest-instance transform (ABI 21; no reference counterpart)
 * ------------------------------------------------------------------------ */

/* sk_nearest_label: for every voxel of an (X, Y, Z) int32 volume, the squared distance to the nearest voxel of any
 * instance and that instance's row: what utils/grow.py grows instances with.  labels, lut, max_id, N and wx, wy, wz are
 * those of sk_label_edt; r(v) is the row of voxel v (1 .. N, 0 for background and unlisted ids) and a site is a voxel
 * with r > 0.  For a voxel p and a site q
 *   value(p, q) = fl(wx dx^2 + fl(wy dy^2 + wz dz^2)),   dx = px - qx, ...
 * every square an exact integer in double, every product and sum rounded once (no fused multiply-add; w (d d)), and
 *   D2(p) = min over sites q of value(p, q).
 * nearest(p) is the row of the site the nested minimum chooses when it is taken as three passes, along z, then y, then
 * x: each pass minimises fl(w d^2 + g_prev(q)) along its axis (g_prev = 0 on a site and +inf elsewhere before the z
 * pass) and, where several positions give the same value, keeps the smallest coordinate.  A site has D2 = 0 and
 * nearest = r(p).  Rounding is monotone, so the passes give D2 bit for bit; the implementation walks outward from the
 * voxel and stops where nothing farther can win or tie.
 * limit2 (+inf allowed) bounds the search: where D2(p) <= limit2 the outputs are dist2[p] = D2(p) and nearest[p];
 * elsewhere -- and where no site exists, or D2 is not finite -- dist2[p] = +inf and nearest[p] = 0.  A pass reads at
 * most 2 floor(sqrt(limit2 / w)) positions per voxel; with limit2 = +inf it is O(extent) per voxel, the price of
 * exactness without a lower envelope.  where (X Y Z bytes, or NULL = every voxel): a voxel with where = 0 that is not a
 * site gets +inf and 0 without a search.  where never restricts which sites count: distances are Euclidean, through
 * anything, not geodesic.
 * dist2, scratch_d2: X Y Z doubles each; nearest, scratch_row: X Y Z int32 each; four distinct buffers.  The passes go
 * (dist2, nearest) -> (scratch_d2, scratch_row) -> (dist2, nearest).  Checked before anything is launched or written:
 * extents, N and max_id not negative, every extent <= 2^26, X Y Z < 2^62, the weights finite and > 0, limit2 not NaN
 * and >= 0, no NULL pointer but where, pointers aligned to their elements, the four buffers distinct.  An empty volume
 * returns SK_OK and writes nothing; N == 0 fills dist2 with +inf and nearest with 0.  The outputs are the same on every
 * run.
 * sk_nearest_label_pass is one of the three passes, under the same checks: axis 2 (z; the sources are not read and may
 * be NULL) writes the nearest site along z of every voxel; axis 1 and 0 minimise fl(w d^2 + src_d2(q)) along the axis
 * and carry src_row of the chosen position, a site keeping (0, r(p)).  Every pass bounds its walk by limit2; only axis
 * 0 reads where and turns values above limit2 into (+inf, 0).  sk_nearest_label is the passes 2, 1, 0 with wz, wy, wx;
 * tools/bench_grow.py times them one by one. */
int sk_nearest_label_pass(const int32_t* labels, int X, int Y, int Z, const int32_t* lut, int max_id, int N, int axis,
                          double w, double limit2, const double* src_d2, const int32_t* src_row, const uint8_t* where,
                          double* dst_d2, int32_t* dst_row, void* stream);
int sk_nearest_label(const int32_t* labels, int X, int Y, int Z, const int32_t* lut, int max_id, int N, double wx,
                     double wy, double wz, double limit2, const uint8_t* where, double* dist2, int32_t* nearest,
                     double* scratch_d2, int32_t* scratch_row, void* stream);

/* ------------------------------------------------------------------------ *
 * Local thickness (ABI 22; no reference counterpart)
 * ------------------------------------------------------------------------ */

/* sk_local_thickness_paint: the sphere-painting transform behind the local thickness of every instance.  dist2 is the
 * output D2 of sk_label_edt on an (X, Y, Z) volume (either mode), wx, wy, wz the same weights.  With
 *   d2(p, c) = fl(wx dx^2 + fl(wy dy^2 + wz dz^2)),   dx = px - cx, ...
 * every square an exact integer in double, every product and sum rounded once (no fused multiply-add; w (d d)), the
 * local thickness of a voxel p of an instance is
 *   T2(p) = max over voxels c of the volume with d2(p, c) < D2(c) of D2(c),
 * the squared radius of the largest open ball around a voxel centre that holds voxels of p's instance only and holds
 * p; T2 = 0 on the background.  The inequality is strict: the nearest outside voxel of c lies at D2(c) exactly and is
 * not in the ball.  D2(c) is the minimum of the same rounded expression over the voxels of other rows, so a ball never
 * reaches another row and no labels are read; c = p qualifies, so T2 >= D2, and per row max T2 = max D2.
 * thick2 (X Y Z doubles) must hold a copy of dist2 on entry.  centres holds n_centres flat voxel indices
 * (x Y + y) Z + z, in any order, repeats allowed; the caller guarantees 0 <= centres[i] < X Y Z (they are not checked
 * on the device).  For every centre c with finite dist2[c] > 0 the call raises thick2[p] to dist2[c] at every voxel p
 * with d2(p, c) < dist2[c]; a centre with dist2[c] = +inf (an instance alone in the volume, open mode) or 0 paints
 * nothing.  After a call, or any sequence of calls, whose centres together cover every voxel with
 * dist2 > min(wx, wy, wz) -- a smaller ball holds its own centre only -- thick2 is T2.  The maximum is taken with
 * integer atomics on the bit pattern and does not depend on the order: the same on every run, however the centres are
 * split over calls.  The work is the sum of the centres' bounding boxes and has no bound of its own; the caller splits
 * the list (lib/morphology.py: PAINT_BUDGET).
 * Checked before anything is launched or written: extents not negative and <= 2^26, X Y Z < 2^62, the weights finite
 * and > 0, n_centres >= 0, no NULL pointer, pointers aligned to 8 bytes, thick2 != dist2.  n_centres == 0 or an empty
 * volume returns SK_OK and writes nothing. */
int sk_local_thickness_paint(const double* dist2, int X, int Y, int Z, double wx, double wy, double wz,
                             const int64_t* centres, int64_t n_centres, double* thick2, void* stream);

/* ------------------------------------------------------------------------ *
 * Contacts between instances (ABI 23; no reference counterpart)
 * ------------------------------------------------------------------------ */

/* sk_instance_contacts: which rows of an (X, Y, Z) int32 instance mask touch, and across how many voxel pairs.  labels,
 * lut, max_id and N are those of sk_instance_stats; r(v) is the row of voxel v (1 .. N, 0 for background: ids <= 0, ids
 * above max_id, rows outside 1 .. N).  Take two voxels p and q = p + d inside the volume, d in {-1, 0, 1}^3 and not
 * zero, every unordered voxel pair once.  The pair is a contact of class
 *   0, 1, 2   d has one nonzero component, x / y / z: a shared face with its normal along that axis;
 *   3, 4, 5   two nonzero components, x and y / x and z / y and z: a shared edge;
 *   6         three: a shared corner.
 * connectivity 6 counts the classes 0 .. 2, 18 the classes 0 .. 5, 26 all seven; the others stay 0.  A contact counts
 * when r(p) != r(q) and both rows are positive; with background = 1 also when exactly one of them is.  It is booked
 * under (lo, hi) = (min, max) of the two rows.  rows receives one row of 9 int64 per distinct (lo, hi) that has a
 * contact -- lo, hi, c0 .. c6 -- in no particular order, and counts[0] their number.
 * The pairs are collected in an open-addressing table of `capacity` slots (a power of two) in `workspace`
 * (sk_instance_contacts_workspace_bytes(capacity) bytes, 0 for a capacity that is not in [1, 2^40]); rows holds
 * capacity rows.  A key that finds no slot within a bounded number of probes is refused for the whole launch: nothing
 * is written for it, and every refused insertion adds 1 to counts[1].  counts[1] == 0 says that rows is complete and
 * exact, and then the set of rows is the same on every run; otherwise counts[0] + counts[1] is at least the number of
 * distinct pairs, and the caller repeats the call with a larger table (validate/lib.py: instance_contacts).  A refusal is
 * never a fault.  Integer atomics only; one pass over the mask and one over the table, no workgroup waits for another.
 * Checked before anything is launched or written (SK_ERR_ARG): extents, N and max_id not negative, X Y Z < 2^62,
 * connectivity in {6, 18, 26}, background in {0, 1}, capacity a power of two in [1, 2^40], workspace_bytes at least the
 * query's, no NULL pointer, pointers aligned to their elements.  An empty volume or N == 0 writes counts = {0, 0} and
 * returns SK_OK (labels and lut are not looked at).  sk_instance_contacts_row_values() = 9. */
int sk_instance_contacts_row_values(void);
size_t sk_instance_contacts_workspace_bytes(int64_t capacity);
int sk_instance_contacts(const int32_t* labels, int X, int Y, int Z, const int32_t* lut, int max_id, int N,
                         int connectivity, int background, int64_t* rows, int64_t capacity, int64_t* counts,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------ *
 * Overlaps between the instances of two masks (ABI 28; the reference declares the consumer,
 * skoots/validate/lib.py: sparse_mask_iou, and raises NotImplementedError in it)
 * ------------------------------------------------------------------------ */

/* sk_instance_overlaps: which rows of one (X, Y, Z) int32 instance mask share voxels with which rows of another of the
 * same shape, and how many.  Each mask has its own header as sk_instance_stats reads it -- (labels_a, lut_a, max_a, N)
 * and (labels_b, lut_b, max_b, M); ra(v) is the row of voxel v in a (1 .. N, 0 for background: ids <= 0, ids above
 * max_a, rows outside 1 .. N) and rb(v) its row in b (0 .. M).  rows receives one row of 3 int64 -- ra, rb, voxels --
 * per pair (ra, rb) that at least one voxel carries, voxels being their number, in no particular order, and counts[0]
 * the number of rows.  With background = 0 only pairs with ra >= 1 and rb >= 1 are produced; with background = 1 also
 * the pairs with exactly one side 0.  The pair (0, 0) is never produced.  The count does not depend on the geometry:
 * the volumes are read as one line of X Y Z voxels.
 * The pairs are collected in an open-addressing table of `capacity` slots (a power of two) in `workspace`
 * (sk_instance_overlaps_workspace_bytes(capacity) bytes, 0 for a capacity that is not in [1, 2^40]); rows holds
 * capacity rows.  A key that finds no slot within a bounded number of probes is refused for the whole launch: nothing
 * is written for it, and every refused insertion adds 1 to counts[1].  counts[1] == 0 says that rows is complete and
 * exact, and then the set of rows is the same on every run; otherwise counts[0] + counts[1] is at least the number of
 * distinct pairs, and the caller repeats the call with a larger table (validate/lib.py: instance_overlaps).  A refusal is
 * never a fault.  Integer atomics only; one pass over the masks and one over the table, no workgroup waits for another.
 * Checked before anything is launched or written (SK_ERR_ARG): extents, N, M, max_a and max_b not negative,
 * X Y Z < 2^62, background in {0, 1}, capacity a power of two in [1, 2^40], workspace_bytes at least the query's, rows,
 * counts and workspace not NULL and aligned to 8 bytes; then, unless the call is empty, the labels and lut of every
 * side that has instances not NULL and aligned to 4 bytes (16-byte alignment of both labels pointers, or the same
 * offset from it, lets the pass read 16 bytes per load; any other 4-byte alignment is read voxel by voxel).  A side
 * without instances (N == 0 or M == 0) is all background: its labels and lut are not looked at and may be NULL.  An
 * empty call -- X Y Z == 0, or N == 0 and M == 0, or background == 0 and either of them 0 -- writes counts = {0, 0} and
 * returns SK_OK; no mask pointer is looked at.  sk_instance_overlaps_row_values() = 3. */
int sk_instance_overlaps_row_values(void);
size_t sk_instance_overlaps_workspace_bytes(int64_t capacity);
int sk_instance_overlaps(const int32_t* labels_a, int X, int Y, int Z, const int32_t* lut_a, int max_a, int N,
                         const int32_t* labels_b, const int32_t* lut_b, int max_b, int M, int background, int64_t* rows,
                         int64_t capacity, int64_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------ *
 * Instances within a distance of each other (ABI 29; no reference counterpart)
 * ------------------------------------------------------------------------ */

/* sk_instance_proximity: which rows of one (X, Y, Z) int32 instance mask lie within a distance of which rows of
 * another of the same shape, how close they come, and how many voxels lie that close: sk_instance_contacts (one mask,
 * reach 1) and sk_instance_overlaps (two masks, reach 0) at reach D.  Each mask has its header as sk_instance_overlaps
 * takes it -- (labels_a, lut_a, max_a, N) and (labels_b, lut_b, max_b, M); ra(p) in 0 .. N and rb(q) in 0 .. M are the
 * rows, 0 the background.  wx, wy, wz are the spacing squared and limit2 is D^2, doubles as sk_nearest_label takes them.
 * For a voxel p of a and a voxel q of b
 *   d2(p, q) = fl(wx dx^2 + fl(wy dy^2 + wz dz^2)),   dx = px - qx, ...
 * every square an exact integer in double, every product and sum rounded once (no fused multiply-add; w (d d)): the
 * expression of sk_nearest_label, bit for bit.
 * A voxel pair (p, q) COUNTS when ra(p) >= 1, rb(q) >= 1 and d2(p, q) <= limit2 (at the limit counts); with
 * exclude_same = 1 also ra(p) != rb(q) is required -- the one-mask mode, in which labels_b may be labels_a.  Voxels
 * outside the volume do not exist.  An overlap (p = q) counts with d2 = 0.
 * rows receives one row of 4 int64 -- ra, rb, near_voxels, gap2_bits -- per key that has a counting pair, in no
 * particular order, and counts[0] their number:
 *   key (ra, rb), rb >= 1   near_voxels is the number of voxels p of ra for which SOME q of rb counts (a voxel is counted
 *                           once per partner, however many q are in reach), gap2_bits the bit pattern of the minimum
 *                           of d2 over the counting pairs of the key;
 *   key (ra, 0)             the union row: near_voxels is the number of voxels of ra for which some q of ANY row counts,
 *                           gap2_bits the minimum over all of them.
 * One direction per call: the voxels counted are those of a; swap the masks for b's side.  gap2 is symmetric.
 * Reach: per axis h is the largest k >= 0 with fl(w k^2) <= limit2, found by search.  The kernel stages the rows of b of
 * a 4 x 16 x 64 tile grown by (hx, hy, hz) on all sides in LDS; a reach whose window does not fit the 160 KiB of a CU is
 * refused with SK_ERR_ARG before anything is launched -- never truncated.  Every reach with hx, hy, hz <= 5 is taken.
 * sk_instance_proximity_reach answers without a GPU: out_host holds 8 int32, out[0 .. 2] = hx, hy, hz (each capped at
 * 2^26), out[3] = 1 when the kernel takes them, out[4] = the LDS bytes of one workgroup at that reach, out[5] = the
 * workgroups one CU holds at it -- the least of what its 160 KiB of LDS, its 32 wave slots and the registers the kernel
 * is compiled for allow -- out[6] = the threads of the workgroup launched at that reach (512 where two windows fit a
 * CU, 1024 where one does), out[7] = 0 (out[4 .. 6] are 0 when refused); it returns SK_ERR_ARG only for weights or a
 * limit2 that sk_instance_proximity refuses, or a NULL or unaligned out.  sk_instance_proximity_resident (needs the
 * GPU) writes what the runtime's occupancy query says for the same kernel and dynamic LDS: the two agree (tested).
 * The pairs are collected in an open-addressing table of `capacity` slots (a power of two) in `workspace`
 * (sk_instance_proximity_workspace_bytes(capacity) bytes, 0 for a capacity that is not in [1, 2^40]); rows holds
 * capacity rows.  A key that finds no slot within a bounded number of probes is refused for the whole launch: nothing
 * is written for it, and every refused insertion adds 1 to counts[1].  counts[1] == 0 says that rows is complete and
 * exact, and then the set of rows is the same on every run; otherwise the caller repeats the call with a larger table
 * (validate/lib.py: instance_proximity).  A refusal is never a fault.  Integer adds, and an integer minimum on the bit
 * pattern (non-negative doubles order as their bits, as in sk_local_thickness_paint); no workgroup waits for another.
 * Checked before anything is launched or written (SK_ERR_ARG): extents, N, M, max_a and max_b not negative,
 * X Y Z < 2^62, the weights finite and > 0, limit2 not NaN, >= 0 and finite, exclude_same in {0, 1}, the reach,
 * capacity a power of two in [1, 2^40], workspace_bytes at least the query's, rows, counts and workspace not NULL and
 * aligned to 8 bytes; then, unless the call is empty, labels and lut of both sides not NULL and aligned to 4 bytes.  An
 * empty call -- X Y Z == 0, N == 0 or M == 0 -- writes counts = {0, 0} and returns SK_OK; no mask pointer is looked at.
 * sk_instance_proximity_row_values() = 4. */
int sk_instance_proximity_row_values(void);
size_t sk_instance_proximity_workspace_bytes(int64_t capacity);
int sk_instance_proximity_reach(double wx, double wy, double wz, double limit2, int32_t* out_host);
int sk_instance_proximity_resident(double wx, double wy, double wz, double limit2, int32_t* workgroups_host);
int sk_instance_proximity(const int32_t* labels_a, int X, int Y, int Z, const int32_t* lut_a, int max_a, int N,
                          const int32_t* labels_b, const int32_t* lut_b, int max_b, int M, double wx, double wy, double wz,
                          double limit2, int exclude_same, int64_t* rows, int64_t capacity, int64_t* counts,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------ *
 * The image under every instance (ABI 25; no reference counterpart)
 * ------------------------------------------------------------------------ */

/* sk_instance_intensity: one pass over an (X, Y, Z) int32 instance mask and an image of the same shape (z fastest both)
 * measures the image under every instance.  labels, lut, max_id and N are those of sk_instance_stats.  image holds
 * unsigned samples of elem_bytes = 1 or 2 bytes; the histogram bin of a sample v is min(v >> shift, 255), shift 0 .. 8
 * (0 for 1-byte samples).  Row r fills
 *   moments[(r - 1) * 6 ..]  int64: n, S v, S v^2, S v x, S v y, S v z over the row's voxels, x, y, z the voxel indices;
 *   extrema[(r - 1) * 2 ..]  int32: min v, max v; a row without voxels keeps INT32_MAX / -1;
 *   hist[(r - 1) * 256 ..]   int64: the voxels per bin.  hist may be NULL: then no histogram work is done.
 * The entry point initialises the outputs itself (stream-ordered) and measures in one launch; background voxels take
 * no atomic, and only integer atomics are used, so the result is exact and the same on every run.  Checked before
 * anything is launched or written (SK_ERR_ARG): extents, N and max_id not negative; elem_bytes 1 or 2; shift 0 .. 8 and
 * 0 with elem_bytes 1; with V = 255 or 65535 and m = max(X, Y, Z), X Y Z V max(V, m) < 2^63 (every sum stays inside
 * int64; formed in 128 bits); then, unless N == 0, no NULL pointer but hist, and pointers aligned to their elements.
 * An empty volume returns SK_OK with the outputs initialised, N == 0 returns SK_OK and writes nothing.
 * sk_instance_intensity_row_values(0) = 6, (1) = 2, (2) = 256: the values per row of the three outputs. */
int sk_instance_intensity_row_values(int which);
int sk_instance_intensity(const int32_t* labels, int X, int Y, int Z, const int32_t* lut, int max_id, int N,
                          const void* image, int elem_bytes, int shift, int64_t* moments, int32_t* extrema,
                          int64_t* hist, void* stream);

/* ------------------------------------------------------------------------ *
 * Diagnostics (no reference counterpart; not on the hot path)
 * ------------------------------------------------------------------------ */

/* Box probe: one launch of a bare v_mfma_f32_16x16x32_f16 register loop (512 workgroups of 4 waves, `iters` x 8
 * MFMAs per wave, pseudo-random operands).  vary_operands = 0: every MFMA multiplies the same register pair;
 * 1: four A x four B fragments in rotation, so that the operand data changes with every instruction as in a real
 * kernel (the chip holds a lower clock then: the rate a matrix kernel on real data can reach).  The caller times it
 * with events on `stream`; *flops (host, may be NULL) receives the FLOPs of the launch.  bench.py prints both rates
 * next to its line: devices differ, so figures from two boxes compare only beside them.  scratch: >= 512 KiB. */
int sk_mfma_probe(void* scratch, size_t scratch_bytes, int iters, int vary_operands, double* flops, void* stream);

/* CU-masked streams (round 4 experiment, tools/cu_*_probe.py; no reference counterpart: the reference runs everything on
 * the default stream of one device, eval.py:57; NOT used by the product path -- DESIGN.md section 8 records why).
 * sk_stream_create_cu_mask wraps hipExtStreamCreateWithCUMask (the stream must belong to the HIP runtime instance the
 * kernels are launched from): bit i of the little-endian word array enables a compute unit; on MI355X bit 8 c + x is
 * compute unit c of XCD x, and an XCD with no bit set gets all its CUs.  sk_debug_where launches n_blocks one-wave
 * workgroups that each record (XCC id, HW id register) after spinning spin_cycles: which CUs a mask really selects. */
int sk_stream_create_cu_mask(const uint32_t* mask_words, int n_words, void** stream_out);
int sk_stream_destroy(void* stream);
int sk_debug_where(unsigned* out, int n_blocks, int spin_cycles, void* stream);

/* Phase-timing builds (-DSK_TIMING, tools/conv_phase_timing.py) dump per-wave cycle sums of the conv kernels into
 * this device buffer, [4096 workgroups][4 waves][16 slots] int64 (bytes must cover all of it); NULL detaches it.
 * The release library stores the pointer and never writes through it. */
int sk_debug_set_timing_buffer(void* device_ptr, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* SKOOTS_HIP_H */
