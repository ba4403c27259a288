/* hla.h -- C ABI of libhla.so: the MI355X (gfx950) implementation of the
 * HighlyAccurate per-pair localisation hot path.
 *
 * This is the drop-in boundary.  The reference is pure Python on PyTorch, so the
 * "FFI" a maintainer binds is ctypes; every entry point below
 * names the reference function it replaces (file:line under /root/reference).
 *
 * Conventions
 *   - plain pointers + sizes only; all pointers are DEVICE pointers unless marked [host]
 *   - the caller allocates every buffer (PyTorch's caching allocator in practice);
 *     the library never allocates or frees device memory and keeps no global state
 *     except a thread-local last-error string, the opt-in timing log (hla_prof_*) and
 *     per-device "kernel attribute set / refused" bits (dynamic-LDS opt-in of the large-LDS kernels; a refused request
 *     makes hla_vgg_backward fall back to its smaller-footprint weight-gradient kernels), and one internal stream per device with
 *     its fork / join events (hla_s2g_lm_solve)
 *   - kernels are launched on the CURRENT device: the caller makes the device that owns the
 *     buffers and the stream current before the call (highlyaccurate_amd/_lib.py on_device)
 *   - all work is enqueued on the given hipStream_t (passed as void*) -- or, inside hla_s2g_lm_solve, on an internal
 *     stream that is forked from it and joined on it before the call returns; no implicit
 *     synchronisation, no host<->device copies except the small [host] structs
 *     passed by value
 *   - return 0 on success, negative hla_status on error; hla_last_error() explains
 *   - activations are NHWC ("channels last"): element (b,y,x,c) at ((b*H+y)*W+x)*C+c
 */
#ifndef HLA_H
#define HLA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* hla_stream_t; /* hipStream_t */

typedef enum hla_status {
  HLA_OK = 0,
  HLA_ERR_ARG = -1,       /* bad argument / unsupported shape */
  HLA_ERR_HIP = -2,       /* a HIP runtime call failed */
  HLA_ERR_WORKSPACE = -3  /* workspace too small */
} hla_status;

typedef enum hla_dtype {
  HLA_F32 = 0,  /* exact-fp32 MFMA (v_mfma_f32_32x32x2_f32): the parity mode      */
  HLA_BF16 = 1, /* bf16 MFMA (v_mfma_f32_32x32x16_bf16), fp32 accumulate: perf mode */
  HLA_F16 = 2,  /* fp16 MFMA (v_mfma_f32_32x32x16_f16), fp32 accumulate: same speed, 3 more mantissa bits,
                   narrower range -- fine for inference on [0,1] images, not recommended for the backward pass */
  HLA_F16X3 = 3 /* split-fp16: fp32 activations and weights in memory; every operand enters the matrix cores as
                   hi + lo = fp16(s x) + fp16(s x - hi) (power-of-two scale s per tensor and sample), one product =
                   three fp16 MFMAs (hi hi + hi lo + lo hi), fp32 accumulate.  fp32-class results (meets the fp32
                   parity gates) at 1/3 of the fp16 MFMA rate instead of the 1/16 of HLA_F32: the matched-accuracy
                   throughput mode, for training too: hla_vgg_backward with this dtype runs split-fp16 data- and
                   weight-gradient kernels on the fp32 activations the split forward saved (gradient maps stay fp32; a
                   per-sample maximum of every gradient map is recorded by the kernel that writes it, as the forward does
                   for activations).  Workspaces have the HLA_F32 layout; packed weights the HLA_F32 size + 256 B of scales. */
} hla_dtype;

const char* hla_last_error(void);

/* Bumped whenever a struct or signature in this file changes.  A binding must refuse a library whose
 * hla_abi_version() differs from the HLA_ABI_VERSION it was written against, and should compare hla_sizeof_struct()
 * with its own struct sizes (ctypes structs are positional: a mismatch corrupts silently).  highlyaccurate_amd/_lib.py
 * does both at load time, and rebuilds or refuses a binary whose hla_source_hash() is not the hash of the sources
 * next to it (the library is git-ignored but shipped prebuilt). */
#define HLA_ABI_VERSION 33
int hla_abi_version(void);
const char* hla_source_hash(void); /* sha256 (hex) of the csrc sources, this header and the compiler flags at build time */
typedef enum hla_struct_id {
  HLA_STRUCT_VGG_PARAMS = 0, HLA_STRUCT_VGG_GRADS = 1, HLA_STRUCT_S2G_LEVEL = 2, HLA_STRUCT_S2G_CONFIG = 3,
  HLA_STRUCT_S2G_LEVEL_GRAD = 4, HLA_STRUCT_PROF_RECORD = 5, HLA_STRUCT_POSE_LOSS_ARGS = 6, HLA_STRUCT_FILL_REGION = 7,
  HLA_STRUCT_VGG_BRANCH = 8
} hla_struct_id;
size_t hla_sizeof_struct(int id);  /* sizeof of the struct with that hla_struct_id, 0 for an unknown id */

/* ------------------------------------------------------------------------- *
 * VGGUnet.forward  (VGG.py:121-203; L2_norm VGG.py:511-514)
 * ------------------------------------------------------------------------- */

/* Device pointers to the 17 weight and 7 bias tensors exactly as PyTorch holds
 * them (OIHW fp32, contiguous), in state-dict order:
 *   w[0..6]  conv0,conv2,conv5,conv7,conv10,conv12,conv14   (b[0..6] their biases)
 *   w[7..12] conv_dec1.1, conv_dec1.3, conv_dec2.1, conv_dec2.3, conv_dec3.1, conv_dec3.3
 *   w[13..16] conf0.1, conf1.1, conf2.1, conf3.1                                    */
typedef struct hla_vgg_params {
  const float* w[17];
  const float* b[7];
} hla_vgg_params;

enum {
  HLA_VGG_WANT_CONF = 1,   /* compute the confidence maps (VGG.py:160-163)                              */
  HLA_VGG_DEFER_NORM = 2,  /* leave feat[] un-normalised and only report inv_norm (the LM loop folds the
                              scale into its normal equations: one full read+write pass less per map)  */
  HLA_VGG_SAVE_FOR_BACKWARD = 4, /* training: also keep relu(conv0) and the three max-pool argmax maps in the
                              workspace; the caller keeps the workspace alive until hla_vgg_backward   */
  HLA_VGG_FOLD_DECODER = 16, /* VGGUnet_G2S (VGG.py:206-345): every map behind the encoder is FOLDED, [h,w] -> [2h,w/2]
                              (an NCHW reshape in the reference; on NHWC storage the identity on memory).  The decoder
                              layers conv_dec1.1 .. conv_dec3.3, their up-sampling / concatenation, the confidence heads
                              1..3 and feat[0..3] take the folded geometry: feat[l] is [B,2h_l,w_l/2,C], conf[l >= 1] is
                              [B,2h_l,w_l/2]; conf[0] stays on the unfolded x15 (VGG.py:322).  The encoder, its pooling
                              and un-pooling are unchanged.  Needs W % 16 == 0 and first_row8 == 0 */
  HLA_VGG_FEAT16 = 8       /* dtype HLA_BF16 / HLA_F16 only, needs HLA_VGG_DEFER_NORM: feat[] are written as fp16 (saturating; also
                              in bf16 mode) instead of fp32 (inv_norm is that of the rounded maps); not with
                              HLA_VGG_SAVE_FOR_BACKWARD.  For hla_s2g_lm_solve with hla_s2g_level.feat_dtype set */
};

/* Weights are re-laid-out once into MFMA fragment order (bf16 or fp32) and reused until they change.
 * hla_vgg_pack_weights reads params->w[0..10] (conv0..conv_dec2.3) AND params->b[0] (conv0's bias rides in the padded k slots
 * of its fragments: the fused conv0 + conv2 kernel adds it inside the matrix product for the 16-bit types) and fills `packed`
 * (hla_vgg_packed_weight_bytes(dtype) bytes).  Call it again after an optimizer step -- also when only conv0's bias changed. */
size_t hla_vgg_packed_weight_bytes(int dtype);
int hla_vgg_pack_weights(const hla_vgg_params* params, void* packed, int dtype, hla_stream_t stream);

/* Bytes of scratch hla_vgg_forward needs for this shape. */
size_t hla_vgg_workspace_bytes(int B, int H, int W, int level, int dtype);
/* The same for a forward made with `flags`: HLA_VGG_FOLD_DECODER plans the partial-sum slots of the folded decoder's tile counts
 * (every other offset is unchanged; without that flag the result equals hla_vgg_workspace_bytes). */
size_t hla_vgg_workspace_bytes_flags(int B, int H, int W, int level, int dtype, int flags);

/* B, H, W  H and W multiples of 8, >= 8, and H*W < 2^23 pixels (8 388 608, e.g. below 2896 x 2896): the convolution kernels
 *          address a sample's activation map with signed 32-bit BYTE offsets and the largest map is H x W x 64 fp32.
 *          hla_vgg_forward / hla_vgg_backward return HLA_ERR_ARG above that.  B is unbounded (samples use 64-bit bases).
 * x        [B,3,H,W] NCHW fp32 (what the reference's DataLoader hands over).  With HLA_VGG_SAVE_FOR_BACKWARD the kernels of
 *          hla_vgg_backward read x AGAIN (conv0's weight gradient): the caller keeps it alive AND UNMODIFIED until then
 * x_plane  elements between consecutive channel planes of x: 0 = H*W (a dense tensor); larger when x is a window of H rows
 *          inside a taller image (rows stay W apart, samples 3*x_plane apart) -- mode='test' runs the ground extractor on the
 *          image rows that can reach the LM loop without first copying them out
 * params   biases b[0..6] and the confidence-head weights w[13..15] are read from here
 * packed_weights  output of hla_vgg_pack_weights for the same dtype
 * feat[l]  [B,H/2^(3-l),W/2^(3-l),C_l] NHWC fp32, C = 256,128,64 for l = 0..2 (x15,x18,x21):
 *          L2-normalised per sample, or raw when HLA_VGG_DEFER_NORM
 * conf[l]  [B,h_l,w_l] fp32 = sigmoid(-sigmoid(conv(relu(.)))), or NULL
 * inv_norm [3][B] fp64 out: 1/max(||map_l of sample b||_2, 1e-12) (VGG.py:511-514), or NULL
 * level    the reference's VGGUnet(level); 4 additionally computes x24 / conf3: feat[3] is [B,H,W,64] with the
 *          16 real channels first and zeros behind them, and params->w[11], w[12], w[16] must point at conv_dec3.1 /
 *          conv_dec3.3 / conf3.1 weights ZERO-PADDED to [64,128,3,3], [64,64,3,3], [1,64,3,3]; inv_norm is [4,B].
 *          3 -> maps 0..2 (the dead dec3/conf3 work of VGG.py:153-155,163 is skipped).
 * first_row8  0, or f in [4, H/8): a promise that the caller reads feat[0] / feat[1] / feat[2] only from rows f / 2f / 4f
 *          on (the LM loop reads rows h_l/2.. only, models_kitti.py:1194-1199).  Every layer then computes just the rows
 *          those depend on; rows above are left unwritten, and inv_norm covers the computed rows only (usable only where
 *          the per-sample scale cancels, as in LM_update).  conf[l], if requested, is likewise only valid from rows
 *          f / 2f / 4f on.  Ignored (treated as 0) at level 4 and with HLA_VGG_SAVE_FOR_BACKWARD.                */
int hla_vgg_forward(const float* x, size_t x_plane, const hla_vgg_params* params, const void* packed_weights, void* const feat[4],
                    float* const conf[4], double* inv_norm, void* workspace, size_t workspace_bytes, int B, int H,
                    int W, int level, int dtype, int flags, int first_row8, hla_stream_t stream);

/* hla_vgg_forward with a first COLUMN as well (hla_vgg_forward is this call with first_col32 = 0, col_gate = NULL).
 * first_col32  0, or c >= 1 with 128 c < W, the column twin of first_row8: a promise that the caller reads feat[0] / feat[1] /
 *          feat[2] only from columns 16c+2 / 32c+6 / 64c+14 on.  Every layer then starts at its 32-pixel tile column c (the H/4
 *          layers), 2c (H/2) or 4c (conv0 + conv2) and reads the source columns left of it as zero: columns 16c / 32c / 64c up to
 *          the promised ones are written but are NOT the full forward's values, the columns left of them stay unwritten, the
 *          promised ones are the full forward's bit for bit; inv_norm covers the written columns.  Applies at level 3 with
 *          HLA_VGG_DEFER_NORM and a dtype other than HLA_F16X3, without HLA_VGG_SAVE_FOR_BACKWARD / HLA_VGG_FOLD_DECODER /
 *          HLA_VGG_WANT_CONF; treated as 0 otherwise (the whole map is computed).
 * col_gate  NULL, or [B] int32 on the device: the FIX-UP pass of an earlier call with the same arguments and first_col32 > 0,
 *          on the same buffers (workspace included, untouched in between).  For every sample with col_gate[b] != 0 the layers
 *          are computed again over the columns that call left unwritten or wrong, and inv_norm again: that sample's maps,
 *          sum-of-squares partials and inv_norm are then what a call with first_col32 = 0 leaves, bit for bit.  A sample with
 *          col_gate[b] == 0 is not touched (its workgroups return at once).  hla_s2g_lm_solve sets such flags (reach_flag). */
int hla_vgg_forward_cols(const float* x, size_t x_plane, const hla_vgg_params* params, const void* packed_weights,
                         void* const feat[4], float* const conf[4], double* inv_norm, void* workspace, size_t workspace_bytes,
                         int B, int H, int W, int level, int dtype, int flags, int first_row8, int first_col32,
                         const int* col_gate, hla_stream_t stream);

/* The fix-up pass alone: hla_vgg_forward_cols with a col_gate (required here) and the choice of how it is launched.
 * one_launch  non-zero (what hla_vgg_forward_cols does): for HLA_BF16 / HLA_F16, and with no hla_prof session open, the pass is ONE
 *          launch with a workgroup per sample -- a flagged sample's workgroup walks the ten layers over its columns and forms its
 *          inv_norm -- so that the usual case, no sample flagged, costs one launch and not eleven in a dependent chain; a flagged
 *          sample is then carried by one compute unit and takes milliseconds.  0, HLA_F32 or a profiled run: ten gated conv
 *          launches and a gated inv_norm.  The results are the same, bit for bit. */
int hla_vgg_fixup(const float* x, size_t x_plane, const hla_vgg_params* params, const void* packed_weights, void* const feat[4],
                  double* inv_norm, void* workspace, size_t workspace_bytes, int B, int H, int W, int level, int dtype, int flags,
                  int first_row8, int first_col32, const int* col_gate, int one_launch, hla_stream_t stream);

/* One network of hla_vgg_forward_pair: the per-network arguments of hla_vgg_forward, with the same meaning. */
typedef struct hla_vgg_branch {
  const float* x;
  size_t x_plane;
  const hla_vgg_params* params;
  const void* packed_weights;
  void* feat[4];
  float* conf[4];
  double* inv_norm;
  void* workspace;
  size_t workspace_bytes;
  int H, W, first_row8;
  int first_col32;
} hla_vgg_branch;

/* The inference forward of TWO networks on batches of one size B (the satellite and the ground extractor of LM_S2GP): computes
 * exactly what hla_vgg_forward(br[0]...) followed by hla_vgg_forward(br[1]...) computes, bit for bit, into the same outputs.
 * When it can, every convolution layer of the two networks runs as ONE launch whose workgroups are dealt to two segments (10
 * launches -- conv0 + conv2 fused and the nine 3x3 layers -- instead of 20, and one inv_norm launch for both): level 3, no HLA_VGG_SAVE_FOR_BACKWARD / HLA_VGG_FOLD_DECODER /
 * HLA_VGG_WANT_CONF, and every layer's two launches on the same side of the small-grid threshold (they must be one kernel).
 * Otherwise it makes the two hla_vgg_forward calls and returns what they return: being unable to pair is never an error.
 * paired_out (may be NULL) receives 1 when the paired launches were issued and 0 when the two plain forwards ran. */
int hla_vgg_forward_pair(const hla_vgg_branch br[2], int B, int level, int dtype, int flags, int* paired_out, hla_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Backward of VGGUnet (autograd through VGG.py:121-203 in the reference).
 * ------------------------------------------------------------------------- */
/* fp32 gradient buffers with PyTorch's layouts (OIHW weights), overwritten: dw[0..10] = conv0..conv_dec2.3
 * (required), db[0..6] (NULL to skip), dw[13..16] = conf0.1..conf3.1 (required iff the matching d_conf is given).
 * Level 4: dw[11], dw[12] (required) and dw[16] have the ZERO-PADDED shapes [64,128,3,3], [64,64,3,3], [1,64,3,3]; the real
 * gradients are their leading [32,128], [16,32], [1,16] blocks.  At level 3 these three get no gradient. */
typedef struct hla_vgg_grads {
  float* dw[17];
  float* db[7];
} hla_vgg_grads;

size_t hla_vgg_packed_weight_T_bytes(int dtype);
/* transposed + tap-flipped fragment packing used by the data-gradient convolutions */
int hla_vgg_pack_weights_T(const hla_vgg_params* params, void* packed_T, int dtype, hla_stream_t stream);
size_t hla_vgg_bwd_workspace_bytes(int B, int H, int W, int level, int dtype);
/* The same for a backward made with `flags` (HLA_VGG_BWD_FOLD_DECODER: the weight-gradient partials of the folded tile counts). */
size_t hla_vgg_bwd_workspace_bytes_flags(int B, int H, int W, int level, int dtype, int flags);

/* x, x_plane, params  as in the forward call
 * fwd_workspace    the workspace of the forward call made with HLA_VGG_SAVE_FOR_BACKWARD | HLA_VGG_DEFER_NORM and the SAME dtype
 *                  (HLA_F16X3: it also holds the per-sample activation maxima the split weight-gradient kernels scale by)
 * feat[l], inv_norm  its outputs (raw maps + 1/norm)
 * d_feat[l]        d(loss)/d(L2-normalised map l), NHWC fp32 (what hla_s2g_lm_solve_bwd produces)
 * conf[l], d_conf[l]  the forward's confidence maps and d(loss)/d(conf map l) [B,h_l,w_l] fp32 (what
 *                  hla_s2g_lm_solve_bwd produces with using_weight=1, models_kitti.py:994-996); both arrays or
 *                  single entries may be NULL: then the heads get no gradient, as in the reference's default run.
 * flags            HLA_VGG_BWD_SCALE_INVARIANT: the consumer of the normalised maps does not depend on their per-sample
 *                  scale (LM_update renormalises both maps, models_kitti.py:982-990), so d_feat[l] is orthogonal to feat[l]
 *                  and the L2_norm Jacobian  dx = a*dy - a^3 (x.dy) x  (a = 1/||x||) reduces to a*dy: the (x.dy) pass and the
 *                  re-read of feat are skipped.  (In the reference that dot product is fp32 rounding noise, ~1e-7 |x||dy|.)
 *                  With this flag (level 3, no d_conf, first_row8 == 0, H <= 1024) the call also finds, per map row, the
 *                  column interval in which d_feat[l] is not exactly zero and skips every tile of every data- and
 *                  weight-gradient launch whose gradient is zero as a consequence (the satellite maps' gradient covers
 *                  ~10 % of the texels: the fan the camera sees).  Values do not change (weight gradients: the order of
 *                  the partial sums does); HLA_VGG_BWD_DENSE switches it off.
 * first_row8       0, or f in [4, H/8): a promise that d_feat[0] / d_feat[1] / d_feat[2] (and d_conf) are zero above rows
 *                  f / 2f / 4f -- the LM loop only reads rows h_l/2.. of the ground maps, so that is where its gradient
 *                  lives.  The rows of d_feat[l] above f * 2^l - 2 are then not even read (they may be uninitialised).  Every activation's gradient is then exactly zero above a first row that follows from the layer
 *                  graph, and the data- and weight-gradient launches skip those rows.  Needs HLA_VGG_BWD_SCALE_INVARIANT;
 *                  ignored (0) otherwise and at level 4. */
#define HLA_VGG_BWD_SCALE_INVARIANT 1
#define HLA_VGG_BWD_DENSE 2           /* visit every tile even where the incoming gradient is exactly zero (A/B and tests) */
#define HLA_VGG_BWD_WGRAD_TWO_PHASE 4 /* weight gradients on the two-phase kernels (512 workgroups, what a device that refuses the
                                         wave-specialised kernels' 96-115 KB LDS request runs) instead of the wave-specialised
                                         ones: the same products in another split-K grouping (A/B and tests); implies the next */
#define HLA_VGG_BWD_FOLD_DECODER 16    /* backward of a forward made with HLA_VGG_FOLD_DECODER (same geometry rules; the decoder's
                                         launches take the dense walk, first_row8 must be 0) */
#define HLA_VGG_BWD_WGRAD0_UNFUSED 8  /* conv2's data gradient stored as a map and conv0's weight gradient computed from it by a
                                         kernel of its own (rounds 1-5), instead of inside that data gradient's epilogue, where the
                                         map is never written (level 3; A/B and tests) */
int hla_vgg_backward(const float* x, size_t x_plane, const hla_vgg_params* params, const void* packed_weights_T,
                     const void* fwd_workspace, const float* const feat[4], const double* inv_norm,
                     const float* const d_feat[4], const float* const conf[4], const float* const d_conf[4],
                     const hla_vgg_grads* grads, void* workspace, size_t workspace_bytes, int B, int H, int W, int level,
                     int dtype, int flags, int first_row8, hla_stream_t stream);

/* Diagnostics for the data-dependent trimming of the last hla_vgg_backward call that used `workspace` (its stream must have
 * completed): live and total tiles per sample of every data- and weight-gradient launch, summed.  Both are 0 when that call
 * took the dense walk.  Synchronous (one small device-to-host copy). */
int hla_vgg_backward_live_tiles(const void* workspace, int B, int H, int W, int level, int dtype, long long* live,
                                long long* total);

/* ------------------------------------------------------------------------- *
 * Dataset-side satellite tile: KITTI_dataset.py:128-157, Ford_dataset.py:185-209
 *   four Pillow resampling stages (NEAREST rotations in 16.16 fixed point, BILINEAR shifts in double with uint8
 *   truncation), TF.center_crop and ToTensor, evaluated lazily per output pixel; bit-identical to Pillow 12.2.
 * ------------------------------------------------------------------------- */
/* src     [B,S,S,3] uint8 (HWC) satellite images
 * stages  [B,4,8] fp64: per stage {kind (0 nearest / 1 bilinear), c0..c5, pad}.  For a nearest stage c[] are the
 *         16.16 fixed-point integers FIX(m0), FIX(m1), FIX(m2 + m0/2 + m1/2), FIX(m3), FIX(m4), FIX(m5 + m3/2 + m4/2),
 *         FIX(v) = floor(v*65536 + 0.5), of Image.rotate's matrix; for a bilinear stage the six AFFINE coefficients
 *         (highlyaccurate_amd/input_pipeline.py builds both)
 * out     [B,3,crop,crop] fp32 in [0,1] */
int hla_sat_tile(const unsigned char* src, const double* stages, float* out, int B, int S, int crop, hla_stream_t stream);

/* Ground image: torchvision Resize([out_h,out_w]) + ToTensor (KITTI_dataset.py:300-311, Ford_dataset.py:141-155) =
 * Pillow's antialiased BILINEAR resample: horizontal pass, uint8 intermediate, vertical pass, integer taps scaled by 2^22.
 * src [B,H,W,3] uint8; {h,v}bounds [n_out][2] = first input index, tap count; {h,v}taps [n_out][ksize] int32
 * (highlyaccurate_amd/input_pipeline.py builds them); mid [B,H,out_w,3] uint8 scratch; out [B,3,out_h,out_w] fp32 in [0,1] */
int hla_resize_bilinear(const unsigned char* src, const int* hbounds, const int* htaps, int hksize, const int* vbounds,
                        const int* vtaps, int vksize, unsigned char* mid, float* out, int B, int H, int W, int out_h,
                        int out_w, hla_stream_t stream);

/* ------------------------------------------------------------------------- *
 * jacobian.grid_sample  (jacobian.py:138-205) -- the stand-alone operator
 * ------------------------------------------------------------------------- */
/* image   [N,IH,IW,C] NHWC fp32;  optical [N,H,W,2] pixel coords (x,y)
 * jac     [M,N,H,W,2] or NULL;    out [N,H,W,C] NHWC;  jac_out [M,N,H,W,C] NHWC or NULL */
int hla_grid_sample(const float* image, const float* optical, const float* jac, float* out, float* jac_out,
                    int N, int C, int IH, int IW, int H, int W, int M, hla_stream_t stream);

/* Backward of hla_grid_sample: what autograd derives from the reference's chain of torch ops (jacobian.py:168-198, with
 * the corner coordinates constants as under its no_grad block, jacobian.py:146-166), in one kernel.  Same layouts.
 *   image, optical, jac   the forward's inputs (jac may be NULL: M is then ignored)
 *   d_out     [N,H,W,C]   cotangent of out,      NULL = zeros
 *   d_jac_out [M,N,H,W,C] cotangent of jac_out,  NULL = zeros;  needs jac and M > 0
 *   d_image   [N,IH,IW,C] ACCUMULATED into (the caller zero-fills it), NULL = not wanted
 *   d_optical [N,H,W,2]   WRITTEN,  NULL = not wanted
 *   d_jac     [M,N,H,W,2] WRITTEN,  NULL = not wanted;  needs jac and M > 0
 * A NULL output removes its work from the kernel, not only its store.  With both cotangents NULL, or all three outputs
 * NULL, no kernel is launched (the wanted written outputs are zero-filled, d_image is left as it is).
 * With the forward's rules  inb = 0<=ix<=IW-1 && 0<=iy<=IH-1,  x0 = floor(ix), x1 = min(x0+1, IW-1), y0, y1 alike,
 * wx0 = x1-ix, wx1 = ix-x0, wy0 = y1-iy, wy1 = iy-y0,  the taps nw, ne, sw, se,  g = d_out[c],
 * a[c] = sum_m d_jac_out[m][c] jac[m].x,  b[c] = sum_m d_jac_out[m][c] jac[m].y:
 *   ddx = wy0 (ne-nw) + wy1 (se-sw)     ddy = wx0 (sw-nw) + wx1 (se-ne)     cross = nw-ne-sw+se
 *   d_image[nw] += g wx0 wy0 - a wy0 - b wx0        d_image[ne] += g wx1 wy0 + a wy0 - b wx1
 *   d_image[sw] += g wx0 wy1 - a wy1 + b wx0        d_image[se] += g wx1 wy1 + a wy1 + b wx1
 *   d_optical = ( sum_c g ddx + b cross ,  sum_c g ddy + a cross )     (cross: jac_out through the bilinear weights)
 *   d_jac[m]  = ( sum_c d_jac_out[m][c] ddx ,  sum_c d_jac_out[m][c] ddy )
 * and everything is zero for a sample that is not in bounds.  Any C and any M.  d_image is summed with fp32 atomic adds,
 * whose order varies: it is NOT bitwise reproducible from run to run (d_optical and d_jac are). */
int hla_grid_sample_bwd(const float* image, const float* optical, const float* jac, const float* d_out,
                        const float* d_jac_out, float* d_image, float* d_optical, float* d_jac,
                        int N, int C, int IH, int IW, int H, int W, int M, hla_stream_t stream);

/* ------------------------------------------------------------------------- *
 * The LM pose loop: project_map_to_grd + LM_update, N_iters x levels steps
 *   KITTI  models_kitti.py:700-1041, loop 1176-1283 (level-first 1352-1459)
 *   Ford   models_ford.py:173-466,  loop 682-835
 * ------------------------------------------------------------------------- */
typedef struct hla_s2g_level {
  const void* sat_feat;  /* [B,A,A,C]  NHWC, elements of feat_dtype */
  const void* grd_feat;  /* [B,h-grd_row_skip,w,C]  NHWC, same element type (rows grd_row_skip..h-1 of the level's map) */
  const float* grd_conf; /* [B,h-grd_row_skip,w] fp32 or NULL (needed iff using_weight) */
  const float* xyz;      /* [h,w,3] fp32 ground-plane points in the camera frame
                            (models_kitti.py:655-682 / models_ford.py:110-155) */
  const double* sat_inv_norm; /* [B] or NULL: sat_feat is raw, multiply by this (HLA_VGG_DEFER_NORM) */
  const double* grd_inv_norm; /* [B] or NULL: same for grd_feat */
  int A, h, w, C;
  int row0;              /* first ground-image row that takes part: h/2 for proj=='geo' (models_kitti.py:1194-1199); 0 for
                            proj=='polar' (1200-1205: the whole map, with the table of grd_img2cam_polar, 684-698, in xyz) */
  int grd_row_skip;      /* rows [0,grd_row_skip) of the ground map are not stored (<= row0): only the bottom half is
                            ever read (models_kitti.py:1194-1199), so a caller may extract features for the rows whose
                            receptive field reaches it and nothing above -- see DESIGN.md "dead rows"; 0 = full map */
  double meter_per_pixel;/* metres per satellite-feature pixel at this level */
  double centre;         /* A/2 (KITTI, float) or A//2 (Ford, integer) */
  int feat_dtype;        /* element type of sat_feat / grd_feat: HLA_F32 (always for the backward and for hla_g2s_*), HLA_F16 or
                            HLA_BF16.  The 16-bit maps hla_vgg_forward writes with HLA_VGG_FEAT16 are ALWAYS fp16 -- also when
                            the convolutions ran with dtype HLA_BF16 -- so they must be passed as HLA_F16 (HLA_BF16 here would
                            reinterpret fp16 bits; it is only for bf16 maps a caller made itself).  Inference in the
                            reduced-precision modes: half the bytes through the HBM-bound LM loop; all LM arithmetic stays
                            fp32 / fp64 */
  /* args.use_gt_depth with a depth map (models_kitti.py:741-748; hla_s2g_lm_solve / _bwd and their workspace functions, KITTI
     chain only).  All six NULL / 0: the flat-ground projection through `xyz`, as before.  With `depth` set, the point of pixel
     (r, c) of sample b is  ray[r,c,:] * depth[b, depth_row[r], depth_col[c]]  -- three fp32 products, then used as the table
     entry is -- and its ground mask is  depth != -1  and nothing else: a depth of 0 (the point at the camera) and a negative
     depth other than -1 (a point behind the camera) take part; the z > 0 rule of `xyz` is NOT applied.  `xyz` is not read
     then (it may stay set); row0 / grd_row_skip keep their meaning; count_in_view counts on the lifted points.  No gradient is
     taken w.r.t. the depth.  hla_g2s_* and cfg->ford = 1 refuse a non-NULL depth. */
  const float* ray;      /* [h,w,3] fp32: K^-1 [u,v,1], the `xyz_w` of grd_img2cam (models_kitti.py:673) at this level's size */
  const float* depth;    /* [B,depth_h,depth_w] fp32, one map per sample; -1 marks a hole */
  const int* depth_row;  /* [h] int32 in [0,depth_h): source row of level row r under F.interpolate(depth, (h, w)) (nearest) */
  const int* depth_col;  /* [w] int32 in [0,depth_w): source column of level column c.  Both are the caller's to make and to keep
                            inside their ranges (device arrays: the library cannot check them) */
  int depth_h, depth_w;
} hla_s2g_level;

typedef struct hla_s2g_config {
  int ford;               /* 0: KITTI camera chain, 1: Ford cam->body->world chain */
  int n_levels, n_iters;
  int level_first;        /* 0: iter-outer/level-inner, 1: level-outer/iter-inner */
  int using_weight;       /* weight = grd_conf (models_kitti.py:994-996) */
  int use_hessian;        /* damping * diag(H) instead of damping * I */
  int dof;                /* 3: (u,v,theta); 2: rotation_range==0; 1: shift ranges == 0 (KITTI only) */
  double shift_range_lat, shift_range_lon, rotation_range; /* metres, metres, degrees */
  double damping[3];      /* lambda per pose component (already 10^(-6+11*sigmoid) if trained) */
  const unsigned char* keep;  /* args.dropout (models_kitti.py:968-974): [steps][keep_stride] bytes in execution order, 1 = the
                                 pixel (index within the rows row0..h-1 of that step's level) takes part; NULL = no dropout */
  size_t keep_stride;
  int optimizer;          /* 0: LM_update; 1: SGD_update (models_kitti.py:1056-1084: pose -= 0.01 * 2 J'(s - g), raw features,
                             no weights, no re-initialisation); 2: ADAM_update (1086-1125, beta1/beta2 below).  1 and 2 are
                             the reference's ablation optimisers; they ignore grd_conf and keep.  3: GN_update (Ford only,
                             models_ford.py:534-598: LM_update without damping and without renormalising the ground map;
                             reads grd_conf, ignores keep).  1-3 exist in the iteration-first loop only, as in the
                             reference; hla_s2g_lm_solve_bwd differentiates all four */
  double beta1, beta2;
  int count_in_view;      /* != 0 (and normal_eq given): slot 14 of normal_eq = the number of pixels of the WHOLE level map whose
                             satellite coordinates fall inside the map in that step -- what `assert mask.sum() > 0`
                             (jacobian.py:172) tests, summed over the batch.  One small extra launch per step. */
  int grd_grad_overwrite; /* hla_s2g_lm_solve_bwd only.  != 0: rows row0..h-1 of every level's d_grd_feat are WRITTEN, not added to
                             (the level's first visit of the reversed loop stores, the later ones add): the caller need not
                             zero-fill those rows (rows above row0 are never touched either way).  0: accumulate into the buffer */
  int deterministic;      /* hla_s2g_lm_solve_bwd only.  0: d(loss)/d(sat map) is scattered with fp32 atomics (their order, and with it
                             the last bits of every gradient behind it, varies from run to run).  != 0: it is accumulated in 64-bit
                             fixed point in the workspace (integer atomics commute) and written -- every element, no zero-fill needed --
                             to d_sat_feat by a closing pass: the same inputs give bitwise the same gradients.  The quantum is a
                             power of two per (level, sample): 2^-P of a bound of that sample's contributions at the level's first
                             visit (P = 40 for the value 1, or the value itself, 16..46); d_damping[3] counts the (step, sample)
                             pairs whose bound outgrew the first one's by more than 2^(50 - P), i.e. put the 63-bit range at
                             risk (must be 0: repeat the call with a smaller P).  Costs 8 B per satellite-map element of
                             workspace, its memset and the closing pass */
  int proj;               /* hla_g2s_* only.  0: proj == 'geo', the camera chain.  1: proj == 'nn', the
                             in-plane similarity warp of the (folded) ground map (models_kitti.py:289-332).  hla_s2g_* require 0 */
  int reach_mode;         /* hla_s2g_lm_solve only (0 elsewhere).  0: off.
                             1, DETECT: the loop runs on satellite maps that are valid from column reach_col0[l] on.  The init
                                launch clears reach_flag[b]; a pixel that takes part in a step (in view, ground mask set) and has a
                                bilinear tap left of that column sets reach_flag[b] = 1.  A pixel whose contribution is masked to zero
                                reads its (zero-weighted) taps at that column instead of column 0.  A sample whose flag stays 0
                                has read only valid columns: its trace and normal_eq are those of the loop on the whole maps; a
                                flagged sample's are not meaningful.
                             2, GATED: the whole loop again for the samples with reach_flag[b] != 0 only (reach_col0 is ignored: the
                                maps are whole, see hla_vgg_forward's col_gate); every workgroup of a sample whose flag is 0 returns
                                at once and that sample's trace / normal_eq entries are left as they are.  Runs on `stream` alone,
                                as ONE launch with a workgroup per sample (the init step and all steps of a flagged sample on one
                                CU: slower per flagged sample than the loop of launches, nothing to pay when no flag is set) with
                                optimizer 0 / 3, using_weight = 0, count_in_view = 0, C = 64 / 128 / 256 and HLA_BF16 or HLA_F16
                                maps on all levels; otherwise as the gated loop of launches.  The results are the same bits either way. */
  int* reach_flag;        /* [B] int32 on the device; required iff reach_mode != 0 */
  int reach_col0[4];      /* reach_mode 1: per level, the first column of levels[l].sat_feat that holds valid values, in [0, A_l) (maps
                             made with hla_vgg_forward_cols' first_col32: 16c+2 / 32c+6 / 64c+14); 0 = the whole map */
} hla_s2g_config;

size_t hla_s2g_workspace_bytes(const hla_s2g_config* cfg, const hla_s2g_level* levels, int B);

/* R_FL [B,3,3], T_FL [B,3] fp32 (Ford only, else NULL)
 * pose0    [B,3] fp32 (shift_u, shift_v, theta) normalised units, or NULL for zeros
 * rand_uv  [n_steps,2,B] fp32: the (rand_u, rand_v) re-initialisation draws of every step
 *          (models_kitti.py:1028-1033), drawn by the caller from torch's CPU generator
 * trace    [B,n_iters,n_levels,3] fp32 out: (shift_u, shift_v, theta) after every step
 * normal_eq[n_steps,B,16] fp64 out or NULL: ||s||^2, ||g||^2, H(6), J^T s (3), J^T g (3), pixels in view (count_in_view), pad
 * stream   from B = 16 on the loop may run part of the batch on an internal stream of the library (one per device, created on
 *          first use); it starts behind the work already on `stream` and is joined on `stream` before the call returns, so
 *          `stream` orders the whole call as if every launch were on it.  Not while `stream` is being captured. */
int hla_s2g_lm_solve(const hla_s2g_config* cfg, const hla_s2g_level* levels, const float* R_FL,
                     const float* T_FL, const float* pose0, const float* rand_uv, float* trace,
                     double* normal_eq, void* workspace, size_t workspace_bytes, int B, hla_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Multi-view localisation (no reference function; the reference's drivers carry --stereo / --sequence, which no model reads):
 * ONE LM loop over V ground images per satellite tile, each with its own rigid transform (R_v, T_v) from its camera to the ONE
 * body pose being solved for -- several calibrated cameras, or earlier frames carried forward by odometry.  Ford chain only
 * (models_ford.py:173-264 takes the extrinsics), inference only: there is no backward.
 *
 * One step is the reference's LM_update (models_ford.py:384-466) applied to the UNION of the views' pixels.  View v of sample b
 * produces the 14 sums of normal_eq at the common pose, de-normalised as hla_s2g_lm_solve does it (sat_inv_norm[b] for s and J,
 * grd_inv_norm[b*V+v] for g); the V vectors are added in fp64 in view order, ((0 + s_0) + s_1) + ..., and the step is solved from
 * the total, so both norms and their 1e-6 clamps apply to the total.  Damping, use_hessian, GN's ng := 1, the +-2.5
 * re-initialisation rule with the caller's draws and dof are those of hla_s2g_lm_solve.  (Per-view normalisation,
 * sum_v H_v / ||s_v||^2, is NOT what this computes.)  Hence: V = 1 is hla_s2g_lm_solve's step; a duplicated view changes nothing
 * beyond fp64 rounding; permuting the views changes only the fp64 addition order; a view whose table has no point with z > 0
 * contributes fourteen exact zeros (the result is bit for bit that of the call without it); a view that is merely OUTSIDE the
 * satellite map still contributes its ||g||^2, as out-of-map pixels of a single view do.
 *
 * levels   per level, for this entry point:
 *            sat_feat [B,A,A,C]; sat_inv_norm [B] or NULL
 *            grd_feat [B*V, h-grd_row_skip, w, C]: view v of sample b is index b*V+v; grd_conf [B*V, h-grd_row_skip, w] likewise
 *            grd_inv_norm [B*V] or NULL
 *            xyz      V tables back to back, [V,h,w,3]: the cameras may differ in intrinsics (one image size for all views)
 *            row0, grd_row_skip, meter_per_pixel, centre, feat_dtype, A, h, w, C: as in hla_s2g_lm_solve; all depth fields NULL / 0
 * cfg      ford = 1; optimizer 0 (LM) or 3 (GN, iteration-first only); using_weight, use_hessian, level_first, dof, damping and the
 *          ranges as in hla_s2g_lm_solve.  Refused with HLA_ERR_ARG and no launch: ford = 0, keep != NULL, a depth field,
 *          reach_mode != 0, count_in_view != 0, optimizer 1 / 2, proj != 0, V outside 1..8 (a cap: Ford carries seven cameras)
 * R, T     [B,V,3,3], [B,V,3] fp32: camera v -> body
 * pose0    [B,3] or NULL;  rand_uv [n_steps,2,B]: per SAMPLE, as in hla_s2g_lm_solve;  trace [B,n_iters,n_levels,3] out
 * normal_eq [n_steps,B,16] fp64 out or NULL: the TOTAL sums, slots 14 / 15 zero
 * view_sums [n_steps,B,V,16] fp64 out or NULL: each view's de-normalised sums, slots 14 / 15 zero
 * Two launches per step plus one init launch, all on `stream` (no internal stream: also while `stream` is being captured).  The
 * results of sample b do not depend, bit for bit, on B, on its batch mates or on repeats.
 * hla_s2g_views_workspace_bytes returns 0 and sets the last error on bad sizes. */
size_t hla_s2g_views_workspace_bytes(const hla_s2g_config* cfg, const hla_s2g_level* levels, int B, int V);
int hla_s2g_lm_solve_views(const hla_s2g_config* cfg, const hla_s2g_level* levels, int V, const float* R, const float* T,
                           const float* pose0, const float* rand_uv, float* trace, double* normal_eq, double* view_sums,
                           void* workspace, size_t workspace_bytes, int B, hla_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Pose scoring (no reference function: the objective of LM_update, models_kitti.py:982-996 / models_ford.py:414-430, read back
 * at given poses).  For ONE level, B samples and K candidate poses per sample, without Jacobians.  Over the pixels of rows
 * row0..h-1 of the level's ground map, for sample b and hypothesis k:
 *   s = the bilinearly sampled satellite feature x (ground mask x in-bounds), the weights of the LM loop's own sampling
 *   g = the ground feature x ground mask
 *   w = grd_conf x ground mask iff cfg->using_weight, else the ground mask
 *   (both maps times their *_inv_norm when the level carries them: the sums are rescaled in the closing pass, like normal_eq)
 * sums [B,K,8] fp64 out:
 *   [0] sum s^2   [1] sum g^2   [2] sum s g   [3] sum w s^2   [4] sum w g^2   [5] sum w s g
 *   [6] pixels of those rows with the ground mask set AND inside the satellite map (an exact integer)
 *   [7] pixels of those rows with the ground mask set
 *   without using_weight, [3..5] are bitwise copies of [0..2]
 * cost [B,K] fp32 out: with ns = max(sqrt(sums[0]), 1e-6), ng = max(sqrt(sums[1]), 1e-6),
 *   sums[3]/ns^2 + sums[4]/ng^2 - 2 sums[5]/(ns ng)  =  sum w (s/ns - g/ng)^2, formed in fp64 and rounded once.  In [0, 4]; a pose
 *   with nothing in view scores sum w g^2 / ng^2 (1 without weights), BELOW the ~2 of a mismatch: rank with sums[6] at hand
 * cfg      read: ford, using_weight, shift_range_lat, shift_range_lon, rotation_range.  cfg->keep must be NULL
 * level    ONE hla_s2g_level; depth must be NULL (depth-lifted scoring is not built); feat_dtype HLA_F32 / HLA_F16 / HLA_BF16;
 *          C in {16, 64, 128, 256}; row0 / grd_row_skip as in hla_s2g_lm_solve
 * R_FL, T_FL  Ford only, else NULL;  poses [B,K,3] fp32 (shift_u, shift_v, theta), normalised units;  K >= 1
 * Two launches; per-tile fp32 partials in the workspace, reduced in a fixed order in fp64.  The tile size follows from the level
 * alone: sums and cost of (b, k) do not depend, bit for bit, on the other hypotheses, on k's position, on K, on B or on repeats. */
size_t hla_s2g_pose_score_workspace_bytes(const hla_s2g_config* cfg, const hla_s2g_level* level, int B, int K);
int hla_s2g_pose_score(const hla_s2g_config* cfg, const hla_s2g_level* level, const float* R_FL, const float* T_FL,
                       const float* poses, int K, double* sums, float* cost, void* workspace, size_t workspace_bytes, int B,
                       hla_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Backward of the LM pose loop (what autograd does in the reference through models_kitti.py:1176-1283,
 * SURVEY Appendix C): d(loss)/d(trace) -> d(loss)/d(feature maps).  Gradients are taken w.r.t. the
 * L2-NORMALISED maps (inv_norm * stored map when the level carries inv norms); buffers are ACCUMULATED into
 * (the caller zero-fills them -- hla_zero_fill does it in one launch; d_grd_feat rows row0.. need not be with
 * cfg->grd_grad_overwrite, d_sat_feat not at all with cfg->deterministic), d_sat_feat with fp32 atomics unless cfg->deterministic.
 * ------------------------------------------------------------------------- */
/* ------------------------------------------------------------------------- *
 * The same loop in the ground -> satellite direction: LM_G2SP (models_kitti.py:22-499, proj == 'geo')
 *   get_warp_sat2real 53-84, seq_warp_real2camera 86-161, project_grd_to_map 163-303, LM_update 333-379,
 *   loop 415-468.  Every satellite-map pixel samples the ground map where it projects to in the camera.
 * cfg        ford = 0, dof = 3, level_first = 0, use_hessian = 0 (the reference has no such variants here);
 *            damping[3] = the `damping` parameter (train_damping) or args.damping
 * levels[l]  sat_feat [B,A,A,C], grd_feat [B,h,w,C] (whole map: grd_row_skip = 0), grd_conf [B,h,w] iff using_weight,
 *            meter_per_pixel; xyz / row0 / centre are not read (the satellite grid is implicit, centre = A/2 integer)
 * camera_k   [B,3,3] fp32 intrinsics of the ori_h x ori_w ground IMAGE (left_camera_k, train_kitti.py:47)
 * trace      [B,N_iters,L,3] = (shift_u, shift_v, heading) after every step; no re-initialisation rule here.
 * normal_eq  [steps,B,16] or NULL: the 12 sums of every step in slots 2..13 (slots 0,1 = 1), needed by the backward
 *
 * cfg->proj = 1: proj == 'nn' (inplane_grd_to_map 289-332 instead of 53-161).  Satellite pixel (row i, col j) of a level with
 *            side A samples the ground map -- VGGUnet_G2S's folded one, [B,h,w,C] with any h, w -- at
 *              (u, v) = R(theta) (j - A/2, i - A/2) + T + A/2,   R = [[cos, -sin], [sin, cos]],
 *              T = (-shift_range_lon * shift_u, shift_range_lat * shift_v) / levels[l].meter_per_pixel   (291-312),
 *              theta = heading * rotation_range * pi / 180,
 *            with the Jacobian of 313-330: d(u,v)/d(shift_u) = (-shift_range_lon / mpp, 0), d(u,v)/d(shift_v) =
 *            (0, shift_range_lat / mpp), d(u,v)/d(heading) = rotation_range * pi / 180 * dR/dtheta (j - A/2, i - A/2); the mask
 *            is all ones and grid_sample's rules are the same (zero outside [0,w-1] x [0,h-1], clamped far corner).
 *            using_weight must be 0; C may also be 16; camera_k (may be NULL), ori_h and ori_w are not read.  The backward
 *            differentiates the pose through (u, v) and through d(u,v)/d(heading) (d2R/dtheta2 is not zero). */
size_t hla_g2s_workspace_bytes(const hla_s2g_config* cfg, const hla_s2g_level* levels, int B);
int hla_g2s_lm_solve(const hla_s2g_config* cfg, const hla_s2g_level* levels, const float* camera_k, int ori_h, int ori_w,
                     const float* pose0, float* trace, double* normal_eq, void* workspace, size_t workspace_bytes,
                     int B, hla_stream_t stream);

/* Pose scoring in the ground -> satellite direction (no reference function: the matching term of LM_G2SP, i.e. the projection
 * of project_grd_to_map, models_kitti.py:163-303, or of inplane_grd_to_map, 289-332, and the residual of LM_update, 333-379, read
 * back at given poses).  For ONE level, B samples and K candidate poses per sample, without Jacobians.  Over the A x A pixels of
 * the level's satellite map, for sample b and hypothesis k:
 *   f = the ground feature sampled where the pixel projects: the set-up, weights and hard in-bounds mask of hla_g2s_lm_solve
 *   s = the satellite feature;   w = the projected confidence iff cfg->using_weight, else 1
 *   a pixel is IN VIEW when its projection is in bounds, 0 <= u <= w-1 and 0 <= v <= h-1, tested in fp64
 *   (both maps times their *_inv_norm when the level carries them: the sums are rescaled in the closing pass, like normal_eq)
 * sums [B,K,8] fp64 out, [0..5] over the pixels in view:
 *   [0] sum f^2   [1] sum s^2   [2] sum f s   [3] sum w f^2   [4] sum w s^2   [5] sum w f s
 *   [6] pixels in view (an exact integer)     [7] sum s^2 over ALL A^2 pixels (the same for every k)
 *   without using_weight, [3..5] are bitwise copies of [0..2]
 * cost [B,K] fp32 out: with nf = max(sqrt(sums[0]), 1e-6), ns = max(sqrt(sums[1]), 1e-6),
 *   sums[3]/nf^2 + sums[4]/ns^2 - 2 sums[5]/(nf ns)  =  sum w (f/nf - s/ns)^2 over the overlap, formed in fp64 and rounded once;
 *   in [0, 4]; +inf when nothing is in view.  (The loop's own objective, sum w (f - s)^2 over all pixels with f = 0 out of view,
 *   rewards a pose for seeing less; without weights it is sums[0] - 2 sums[2] + sums[7].)
 * cfg      read: proj, using_weight, shift_range_lat, shift_range_lon, rotation_range; ford must be 0
 * level    ONE hla_s2g_level as hla_g2s_lm_solve takes it: feat_dtype HLA_F32, grd_row_skip = 0, depth NULL; C in {64, 128, 256},
 *          also 16 with proj 1; no weights with proj 1
 * camera_k, ori_h, ori_w  as in hla_g2s_lm_solve (not read with proj 1);  poses [B,K,3] fp32 (shift_u, shift_v, heading), K >= 1
 * A pose of any value, finite or not, reads only inside the sample's own maps.  Two launches; per-tile fp32 partials in the
 * workspace, reduced in a fixed order in fp64.  The tile size follows from C alone: sums and cost of (b, k) do not depend, bit
 * for bit, on the other hypotheses, on k's position, on K, on B or on repeats.
 * hla_g2s_pose_score_workspace_bytes returns 0 and sets the last error on bad arguments. */
size_t hla_g2s_pose_score_workspace_bytes(const hla_s2g_config* cfg, const hla_s2g_level* level, int B, int K);
int hla_g2s_pose_score(const hla_s2g_config* cfg, const hla_s2g_level* level, const float* camera_k, int ori_h, int ori_w,
                       const float* poses, int K, double* sums, float* cost, void* workspace, size_t workspace_bytes, int B,
                       hla_stream_t stream);

typedef struct hla_s2g_level_grad {
  float* d_sat_feat; /* [B,A,A,C] fp32 */
  float* d_grd_feat; /* [B,h,w,C] fp32 */
  float* d_grd_conf; /* [B,h,w] fp32 or NULL (only written when using_weight) */
} hla_s2g_level_grad;

size_t hla_s2g_bwd_workspace_bytes(const hla_s2g_config* cfg, const hla_s2g_level* levels, int B);

/* trace, normal_eq: outputs of the forward call (normal_eq is required here);  d_trace [B,n_iters,n_levels,3] fp32
 * d_damping [4] fp64 out (overwritten): [0..2] d(loss)/d(lambda_i) summed over samples and steps (for train_damping; summed per
 *           sample in step order, then over the samples in sample order: reproducible), [3] cfg->deterministic's range counter */
int hla_s2g_lm_solve_bwd(const hla_s2g_config* cfg, const hla_s2g_level* levels, const hla_s2g_level_grad* grads,
                         const float* R_FL, const float* T_FL, const float* pose0, const float* trace,
                         const double* normal_eq, const float* d_trace, double* d_damping, void* workspace,
                         size_t workspace_bytes, int B, hla_stream_t stream);

/* Backward of hla_s2g_pose_score (no reference function; what autograd gives for the cost formula above, which is the residual
 * of LM_update, models_kitti.py:982-996 / models_ford.py:414-430 -- the surface the reference trains by metric learning with
 * triplet_loss, models_kitti.py:579-595, 1607-1624).  Given d(loss)/d(cost) it writes d(loss)/d(the level's maps); poses get no
 * gradient.
 *   cfg, level, R_FL, T_FL, poses, K   the forward's; feat_dtype must be HLA_F32 (16-bit maps are refused), cfg->keep and
 *                                      level->depth NULL as in the forward, cfg->deterministic 0
 *   sums   [B,K,8] fp64   the forward's output;   d_cost [B,K] fp32
 *   grad   d_sat_feat [B,A,A,C], d_grd_feat [B,h-grd_row_skip,w,C] and, iff cfg->using_weight, d_grd_conf [B,h-grd_row_skip,w]:
 *          fp32 NHWC, all OVERWRITTEN (the call clears what it accumulates into; the stored ground rows above row0 are zero).
 *          Gradients are taken w.r.t. the L2-NORMALISED maps (inv_norm x stored map), hla_s2g_lm_solve_bwd's convention:
 *          hla_vgg_backward with HLA_VGG_BWD_SCALE_INVARIANT consumes them as they are (sum map x d_map = 0 per sample)
 * With s, g the masked normalised values, N = sums[0], G = sums[1], a = sums[3], e = sums[4], c = sums[5], ns = max(sqrt N, 1e-6),
 * ng = max(sqrt G, 1e-6) and w as in the forward:
 *   d cost/d s    = 2 w s/ns^2 - 2 a s/ns^4 - 2 w g/(ns ng) + 2 c s/(ns^3 ng)     (pixels in view; through lm_pixel's tap weights)
 *   d cost/d g    = 2 w g/ng^2 - 2 e g/ng^4 - 2 w s/(ns ng) + 2 c g/(ng^3 ns)     (pixels with the ground mask)
 *   d cost/d conf = ground mask x sum_channels (s/ns - g/ng)^2
 * where a clamped norm is a constant (its second and fourth term are absent), and without weights the first two terms, which
 * cancel identically, are not formed.  The per-(sample, hypothesis) scalars are formed in fp64 from `sums` and rounded once.
 * d_grd_feat and d_grd_conf are summed over k in ascending order in registers and stored once: the same bits from run to run and
 * whatever B is.  d_sat_feat is summed with fp32 atomics: NOT bitwise reproducible.  A hypothesis with d_cost == 0 or
 * sums[6] == 0 costs no map traffic.  hla_s2g_pose_score_bwd_workspace_bytes returns 0 and sets the last error on bad arguments. */
size_t hla_s2g_pose_score_bwd_workspace_bytes(const hla_s2g_config* cfg, const hla_s2g_level* level, int B, int K);
int hla_s2g_pose_score_bwd(const hla_s2g_config* cfg, const hla_s2g_level* level, const hla_s2g_level_grad* grad,
                           const float* R_FL, const float* T_FL, const float* poses, int K, const double* sums,
                           const float* d_cost, void* workspace, size_t workspace_bytes, int B, hla_stream_t stream);

/* Backward of hla_g2s_pose_score (no reference function; what autograd gives for the cost formula of hla_g2s_pose_score -- the
 * ground -> satellite counterpart of the surface the reference trains by metric learning with triplet_loss,
 * models_kitti.py:579-595).  Given d(loss)/d(cost) it writes d(loss)/d(the level's maps); poses get no gradient.
 *   cfg, level, camera_k, ori_h, ori_w, poses, K   the forward's (fp32 maps, grd_row_skip 0, depth NULL, ford 0); also cfg->keep
 *                                                  NULL and cfg->deterministic 0
 *   sums   [B,K,8] fp64   the forward's output;   d_cost [B,K] fp32
 *   grad   d_sat_feat [B,A,A,C], d_grd_feat [B,h,w,C] and, iff cfg->using_weight, d_grd_conf [B,h,w]: fp32 NHWC, all OVERWRITTEN
 *          (the call clears what it accumulates into; without using_weight d_grd_conf is not touched).  Gradients are taken
 *          w.r.t. the L2-NORMALISED maps (inv_norm x stored map), hla_g2s_lm_solve_bwd's convention: hla_vgg_backward with
 *          HLA_VGG_BWD_SCALE_INVARIANT consumes them as they are
 * With f, s, w as in the forward, N = sums[0], S = sums[1], a = sums[3], e = sums[4], c = sums[5], nf = max(sqrt N, 1e-6),
 * ns = max(sqrt S, 1e-6), per satellite pixel IN VIEW (the forward's decision, bit for bit) and per channel:
 *   d cost/d f = 2 w f/nf^2 - 2 a f/nf^4 - 2 w s/(nf ns) + 2 c f/(nf^3 ns)     (to the four ground taps, clamped-corner weights)
 *   d cost/d s = 2 w s/ns^2 - 2 e s/ns^4 - 2 w f/(nf ns) + 2 c s/(ns^3 nf)     (on the satellite pixel itself)
 *   d cost/d w = sum_channels (f/nf - s/ns)^2                                  (to the same four taps of grd_conf)
 * where a clamped norm is a constant (its second and fourth term are absent), and without weights the first two terms, which
 * cancel identically, are not formed.  A pixel out of view gets nothing for that hypothesis; sums[7] does not enter.  The
 * per-(sample, hypothesis) scalars are formed in fp64 from `sums` and rounded once.  d_sat_feat is summed over k in ascending
 * order in registers and every element is stored once: the same bits from run to run and whatever B is.  d_grd_feat and
 * d_grd_conf are summed with fp32 atomics: NOT bitwise reproducible.  A hypothesis with d_cost == 0 or sums[6] == 0 costs no map
 * traffic.  hla_g2s_pose_score_bwd_workspace_bytes returns 0 and sets the last error on bad arguments. */
size_t hla_g2s_pose_score_bwd_workspace_bytes(const hla_s2g_config* cfg, const hla_s2g_level* level, int B, int K);
int hla_g2s_pose_score_bwd(const hla_s2g_config* cfg, const hla_s2g_level* level, const hla_s2g_level_grad* grad,
                           const float* camera_k, int ori_h, int ori_w, const float* poses, int K, const double* sums,
                           const float* d_cost, void* workspace, size_t workspace_bytes, int B, hla_stream_t stream);

/* Backward of hla_g2s_lm_solve (autograd through the same reference lines).  grads[l]: d_sat_feat [B,A,A,C] and
 * d_grd_feat [B,h,w,C] are ACCUMULATED into (zero them first), likewise d_grd_conf [B,h,w] iff using_weight;
 * d_damping[3] (fp64) is overwritten with d(loss)/d(lambda) -- in this direction lambda IS the `damping` parameter
 * (models_kitti.py:41,358).  Gradients are w.r.t. the L2-normalised maps, as hla_vgg_backward expects. */
size_t hla_g2s_bwd_workspace_bytes(const hla_s2g_config* cfg, const hla_s2g_level* levels, int B);
int hla_g2s_lm_solve_bwd(const hla_s2g_config* cfg, const hla_s2g_level* levels, const hla_s2g_level_grad* grads,
                         const float* camera_k, int ori_h, int ori_w, const float* pose0, const float* trace,
                         const double* normal_eq, const float* d_trace, double* d_damping, void* workspace,
                         size_t workspace_bytes, int B, hla_stream_t stream);


/* Zero-fill up to 16 (strided) regions of device memory in ONE launch: what a caller of hla_s2g_lm_solve_bwd has to clear in front
 * of it (three d_sat_feat maps, the rows of the d_grd_feat maps its consumer reads above row0, d_grd_conf) -- as separate
 * fill launches these were ~10 of the ~25 small launches between the LM loop and its backward (the reference: autograd's own
 * zeros_like / accumulate nodes).  Region i = n_chunks pieces of chunk_bytes, stride_bytes apart, starting at ptr; ptr,
 * chunk_bytes and stride_bytes must be multiples of 4 (a region whose three are multiples of 16 is cleared with 16-byte stores). */
typedef struct hla_fill_region {
  void* ptr;
  size_t chunk_bytes, stride_bytes;
  int n_chunks;
} hla_fill_region;
int hla_zero_fill(const hla_fill_region* regions, int n_regions, int max_blocks, hla_stream_t stream);
/* max_blocks: 0 = as fast as the memory system takes it (up to 2048 workgroups per region); > 0 caps the workgroups per region --
 * a background fill on a side stream that leaves the chip to the kernels it runs under (training clears the LM backward's
 * 1.4 GB of gradient buffers that way while the forward's convolutions run) */

/* ------------------------------------------------------------------------- *
 * loss_func, loss_method 0  (models_ford.py:1041-1093; models_kitti.py imports the same function)
 * ------------------------------------------------------------------------- */
/* The pose loss of one training step and its gradient, one launch each (the reference: ~25 tensor ops + ~40 autograd nodes).
 *   d_k[n,l] = mean_b |x_k[b,n,l] - gt_k[b]|  (k = 0 lat, 1 lon, 2 theta; models_ford.py:1073-1079)
 *   losses   = coe[0] d_0 + coe[1] d_1 + coe[2] d_2                                   (models_ford.py:1086)
 * out[1 + 8 L], in the order of the reference's return tuple (models_ford.py:1091-1092):
 *   [0] mean(losses); then L values each of: losses[0]-losses[-1], d_0[0]-d_0[-1], d_1[0]-d_1[-1], d_2[0]-d_2[-1],
 *   losses[-1], d_0[-1], d_1[-1], d_2[-1].
 * gt_dtype selects the result type like torch's promotion does: fp32 inputs with fp32 ground truth give fp32 results
 * (KITTI), with fp64 ground truth fp64 results (the Ford loader hands float64).  `out` and `g_out` hold that type. */
enum { HLA_POSE_LOSS_F32 = 0, HLA_POSE_LOSS_F64 = 1 };
typedef struct hla_pose_loss_args {
  const float* x[3];          /* shift_lats, shift_lons, thetas [B,N,L] fp32: element (b,n,l) at x[k][b s0 + n s1 + l s2] */
  long long x_stride[3][3];   /* (s0, s1, s2) per input, in elements (three columns of one [B,N,L,3] trace: (3NL, 3L, 3)) */
  const void* gt[3];          /* gt_shift_lat, gt_shift_lon, gt_theta [B], fp32 or fp64 per gt_dtype */
  long long gt_stride[3];     /* in elements */
  double coe[3];              /* coe_shift_lat, coe_shift_lon, coe_theta */
  int B, N, L;                /* N * L <= 512 */
  int gt_dtype;
} hla_pose_loss_args;
int hla_pose_loss(const hla_pose_loss_args* args, void* out, hla_stream_t stream);
/* g_out[j]: d(scalar)/d(out piece j) (j = 0: one value; j = 1..8: L values, contiguous) or NULL (= zero).
 * dx[k]: gradient w.r.t. x[k], every element (b,n,l) written at dx[k][b t0 + n t1 + l t2], (t0,t1,t2) = dx_stride[k]. */
int hla_pose_loss_bwd(const hla_pose_loss_args* args, const void* const g_out[9], float* const dx[3],
                      const long long dx_stride[3][3], hla_stream_t stream);

/* ------------------------------------------------------------------------- *
 * LM_S2GP.orien_corr  (models_kitti.py:1543-1605) and triplet_loss (1607-1624): the coarse heading search
 * ------------------------------------------------------------------------- */
/* One level of orien_corr behind the polar resampling.  The caller samples the WINDOW of the polar satellite map the shifts
 * read -- the columns of the reference's polar_sat1 (1582-1585): -n .. W+n-1 of polar_coordinates(level) (1518-1541) modulo its
 * width for 0 < n <= that width, n = ceil(rotation_range / (90 / W)), S = 2n + 1 -- with hla_grid_sample from the raw satellite map
 * (and takes d_P1 back through hla_orien_window_bwd).
 *   P1            [B,H,W+S-1,C] NHWC fp32;  p1_inv_norm [B] fp64 or NULL: P1 is multiplied by it (the map was sampled raw,
 *                 HLA_VGG_DEFER_NORM; sampling is linear)
 *   grd_feat      [B,H,W,C] NHWC fp32;  grd_inv_norm [B] fp64 or NULL likewise.  With f = grd_inv_norm * grd_feat:
 *                 g = f / max(||f||_2, 1e-12) per sample (F.normalize, 1572)
 *   S             the number of shifts (the width of the reference's conv2d output)
 *   dot   [B,S] fp64 out   sum_{h,w,c} P1[b,h,w+s,c] g[b,h,w,c]                (the grouped conv2d, 1588-1589)
 *   E     [B,S] fp64 out   sum_{h,w<W,c} P1[b,h,w+s,c]^2                       (avg_pool2d, divisor_override=1, 1591-1592)
 *   gnorm [B]   fp64 out   ||f||_2
 *   corr  [B,S] fp32 out   2 - 2 dot / max(sqrt(E), 1e-6)                      (1593-1594)
 * Block partials are fp32 and reduced in a fixed order in fp64: the result does not depend on the order the blocks finish in.
 * C in {16, 64, 128, 256}; any H, W (B, H <= 65535), S >= 1.  workspace: hla_orien_corr_workspace_bytes (serves both calls). */
size_t hla_orien_corr_workspace_bytes(int B, int H, int W, int C, int S);
int hla_orien_corr(const float* P1, const float* grd_feat, const double* p1_inv_norm, const double* grd_inv_norm, double* dot,
                   double* E, double* gnorm, float* corr, void* workspace, size_t workspace_bytes, int B, int H, int W, int C,
                   int S, hla_stream_t stream);
/* Backward (what autograd derives from 1572-1594): d_corr [B,S] fp32 and the forward's dot, E, gnorm ->
 *   d_P1       [B,H,W+S-1,C]  w.r.t. p1_inv_norm * P1:  sum_s ddot[s] g[.,x-s,.] + 2 (p1_inv_norm P1) beta[x], where
 *              ddot = -2 d_corr / D, D = max(sqrt(E), 1e-6), beta[x] = sum of d_corr dot / D^3 over the shifts whose window covers
 *              column x and whose sqrt(E) is not clamped (no gradient flows through a clamped E)
 *   d_grd_feat [B,H,W,C]     w.r.t. f:  (d_g - g (g . d_g)) / ||f||,  d_g = sum_s ddot[s] P1[.,w+s,.]  (the projection is the second
 *              normalisation's; what hla_vgg_backward takes as d_feat)
 * Both are WRITTEN, in gather form: no atomics, bitwise reproducible. */
int hla_orien_corr_bwd(const float* P1, const float* grd_feat, const double* p1_inv_norm, const double* grd_inv_norm,
                       const double* dot, const double* E, const double* gnorm, const float* d_corr, float* d_P1,
                       float* d_grd_feat, void* workspace, size_t workspace_bytes, int B, int H, int W, int C, int S,
                       hla_stream_t stream);
/* Backward of that window sampling (hla_grid_sample(image, optical) -> out, no jac) to the image, for this consumer: near the
 * centre of the polar fan a texel collects about a thousand largely cancelling terms, which hla_grid_sample_bwd's fp32 atomics
 * sum to 7-10 fp32 ulps of the map's maximum, differently in every run.  Here they are summed in fp64 (hardware fp64 atomics) and
 * rounded once: the result is the correctly rounded sum up to 1e-16 relative, whatever the order.
 *   optical [N,H,W,2], d_out [N,H,W,C] fp32;  acc [N,IH,IW,C] fp64 scratch (cleared by the call);  d_image [N,IH,IW,C] fp32 WRITTEN */
int hla_orien_window_bwd(const float* optical, const float* d_out, double* acc, float* d_image, int N, int C, int IH, int IW,
                         int H, int W, hla_stream_t stream);
/* triplet_loss of one level (1611-1622): sum_{b,s} log(1 + exp(10 (corr[b,gt_b] - corr[b,s]))) / (B (S - 1)) with
 * gt_b = (S-1)/2 + round(gt_heading[b] * rotation_range / degree_per_pixel) (fp32, half to even, as the reference's tensors; an
 * index outside [-S,S), where the reference raises, gives NaN).  loss[0] (fp32) is written, or added to when accumulate != 0
 * (the sum over the levels, 1624).  gt_heading: element b at gt_heading[b * gt_stride]. */
int hla_orien_triplet_loss(const float* corr, const float* gt_heading, long long gt_stride, double rotation_range,
                           double degree_per_pixel, float* loss, int accumulate, int B, int S, hla_stream_t stream);
/* d_corr [B,S] fp32 (written) = g_loss[0] * d(loss of this level)/d(corr) */
int hla_orien_triplet_loss_bwd(const float* corr, const float* gt_heading, long long gt_stride, double rotation_range,
                               double degree_per_pixel, const float* g_loss, float* d_corr, int B, int S, hla_stream_t stream);

/* ------------------------------------------------------------------------- *
 * LM_G2SP.corr  (models_kitti.py:501-577) and triplet_loss (579-595): the dense translation search
 * ------------------------------------------------------------------------- */
/* One level of corr behind the projection.  The caller samples the centre crop of the ground map projected at the zero pose
 * (project_grd_to_map, 163-287; TF.center_crop to crop_H x crop_W, 546-548) with hla_grid_sample from the raw ground map, and
 * takes d_g2s back through hla_orien_window_bwd.
 *   sat           [B,A,A,C] NHWC fp32;  sat_inv_norm [B] fp64 or NULL: sat is multiplied by it (HLA_VGG_DEFER_NORM); s below
 *   g2s           [B,Hc,Wc,C] NHWC fp32, the sampled crop before F.normalize;  g2s_inv_norm [B] fp64 or NULL likewise (sampling
 *                 is linear).  With f = g2s_inv_norm * g2s:  g = f / max(||f||_2, 1e-12) per sample (F.normalize, 549)
 *   Ny = A - Hc + 1, Nx = A - Wc + 1   the shifts (the reference's conv2d output)
 *   dot   [B,Ny,Nx] fp64 out   sum_{y<Hc,x<Wc,c} g[b,y,x,c] s[b,y+dy,x+dx,c]      (the grouped conv2d, 551-552)
 *   E     [B,Ny,Nx] fp64 out   sum_{y<Hc,x<Wc,c} s[b,y+dy,x+dx,c]^2               (avg_pool2d, divisor_override=1, and the channel sum, 554-555)
 *   gnorm [B]       fp64 out   ||f||_2
 *   corr  [B,Ny,Nx] fp32 out   2 - 2 dot / max(sqrt(E), 1e-6)                     (556-557), rounded once
 * The contraction runs on the fp32-input MFMA; no fp32 accumulator collects more than 4096 products before it is added to an
 * fp64 sum, and the partial sums of different workgroups are stored and added in fp64 in a fixed order: the result does not
 * depend on B, on the grid or on the run.  C in {16, 64, 128, 256}; 1 <= Hc, Wc <= A <= 16384; B <= 65535.
 * workspace: hla_g2s_corr_workspace_bytes (serves both calls; 0 with hla_last_error set for sizes that are refused). */
size_t hla_g2s_corr_workspace_bytes(int B, int A, int Hc, int Wc, int C);
int hla_g2s_corr(const float* sat, const float* g2s, const double* sat_inv_norm, const double* g2s_inv_norm, double* dot, double* E,
                 double* gnorm, float* corr, void* workspace, size_t workspace_bytes, int B, int A, int Hc, int Wc, int C,
                 hla_stream_t stream);
/* Backward (what autograd derives from 549-557): d_corr [B,Ny,Nx] fp32 and the forward's dot, E, gnorm.  With D = max(sqrt(E), 1e-6),
 * ddot = -2 d_corr / D and beta = d_corr dot / D^3 where sqrt(E) > 1e-6, else 0 (no gradient flows through a clamped E):
 *   d_sat [B,A,A,C]    w.r.t. s:  sum_{dy,dx} ddot[dy,dx] g[r-dy,x-dx,c] + 2 s[r,x,c] Bsum[r,x],  Bsum the sum of beta over the shifts
 *                      whose window covers (r,x)
 *   d_g2s [B,Hc,Wc,C]  w.r.t. f:  (d_g - g (g . d_g)) / ||f||,  d_g[y,x,c] = sum_{dy,dx} ddot[dy,dx] s[y+dy,x+dx,c]; zero through the
 *                      norm where ||f|| is clamped
 * Both are WRITTEN (no zero fill by the caller), in gather form with fp64 sums: no atomics, bitwise reproducible. */
int hla_g2s_corr_bwd(const float* sat, const float* g2s, const double* sat_inv_norm, const double* g2s_inv_norm, const double* dot,
                     const double* E, const double* gnorm, const float* d_corr, float* d_sat, float* d_g2s, void* workspace,
                     size_t workspace_bytes, int B, int A, int Hc, int Wc, int C, hla_stream_t stream);
/* triplet_loss of one level (579-595): sum_{b,dy,dx} log(1 + exp(10 (corr[b,h_b,w_b] - corr[b,dy,dx]))) / (B (Ny Nx - 1)) with
 *   w_b = round(Nx/2 + gt_shift_u[b] * shift_range_lon / meters_per_pixel),  h_b = round(Ny/2 - gt_shift_v[b] * shift_range_lat / meters_per_pixel)
 * (587-588: fp32 like the reference's tensors, Nx/2 a true division, half to even).  h in [-Ny,Ny) and w in [-Nx,Nx) wrap like a
 * Python index; outside, where the reference raises, the loss is NaN.  meters_per_pixel is the level's
 * utils.get_meter_per_pixel() * 2^(3-level).  loss[0] (fp32) is written, or added to when accumulate != 0 (the sum over the levels,
 * 595).  Element b of gt_shift_u at gt_shift_u[b * gt_u_stride], of gt_shift_v likewise. */
int hla_g2s_corr_triplet_loss(const float* corr, const float* gt_shift_u, long long gt_u_stride, const float* gt_shift_v,
                              long long gt_v_stride, double shift_range_lat, double shift_range_lon, double meters_per_pixel,
                              float* loss, int accumulate, int B, int Ny, int Nx, hla_stream_t stream);
/* d_corr [B,Ny,Nx] fp32 (written) = g_loss[0] * d(loss of this level)/d(corr) */
int hla_g2s_corr_triplet_loss_bwd(const float* corr, const float* gt_shift_u, long long gt_u_stride, const float* gt_shift_v,
                                  long long gt_v_stride, double shift_range_lat, double shift_range_lon, double meters_per_pixel,
                                  const float* g_loss, float* d_corr, int B, int Ny, int Nx, hla_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Measurement hooks (no reference counterpart; used by bench.py for the roofline numbers).
 * When enabled, every kernel launch of the entry points above is bracketed by two hipEvents
 * on its own stream; hla_prof_fetch synchronises them and returns one record per launch.
 * ------------------------------------------------------------------------- */
#define HLA_PROF_NKERNELS 22 /* (17 before lm_repair_loop got an id of its own, 18 before hla_g2s_corr's two, 20 before hla_s2g_lm_solve_views' two: a caller that sizes a table by it recompiles) */
typedef struct hla_prof_record {
  int kernel_id;  /* index for hla_prof_kernel_name */
  float ms;       /* event-to-event duration on the launch stream */
  double flops;   /* algorithmic FLOPs of the launch (2*9*Cin*Cout*rows*W*B for a conv, the rows it computes), else 0.  A
                     data-dependent launch of hla_vgg_backward (the satellite branch: only the tiles whose gradient is not exactly
                     zero) reports the EXECUTED share: dense FLOPs x live tiles / tiles, the live count read back through a pinned
                     host slot behind the kernel that wrote it */
  double bytes;   /* algorithmic HBM bytes of the launch (maps read once + outputs), scaled likewise, else 0 */
} hla_prof_record;
int hla_prof_enable(int on);
const char* hla_prof_kernel_name(int kernel_id);
int hla_prof_fetch(hla_prof_record* out, int max_records, int* n_out); /* also clears the log */
/* What the matrix pipe of this device SUSTAINS: back-to-back v_mfma_f32_32x32x16_{bf16,f16} on register-resident operands (no LDS,
 * no memory), two waves per SIMD, every CU busy for about ms_target milliseconds (0 < ms_target <= 200); synchronises the stream.
 * dtype HLA_BF16 / HLA_F16; data 0 = zero operands (reaches the nominal peak), 1 = random values, 2 = random with half the
 * elements zero (post-ReLU-like activations): on real data the package power limit, not the pipe, sets the rate.
 * tflops_out: achieved TFLOP/s.  bench.py reports it as roofline.mfma_sustained next to the nominal roofline.peak. */
int hla_prof_mfma_peak(int dtype, int data, float ms_target, float* tflops_out, hla_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* HLA_H */
