/*
 * hrp.h - C ABI of libhrp_hip.so: the MI355X (gfx950) kernels behind the HoRoPose image->pose path.
 *
 * Every entry point is `extern "C"`, takes plain pointers / sizes / POD descriptors (no torch, no C++
 * types), launches asynchronously on the caller's hipStream_t (passed as void*), returns 0 on success
 * or a negative hrp_status (text via hrp_last_error()).  The caller owns every buffer (device pointers,
 * e.g. tensor.data_ptr()); the library allocates nothing and keeps no state, so all calls are
 * hipGraph-capturable.
 *
 * Statelessness vs the handle sketched in SURVEY 8(b) (hrp_create / hrp_destroy, hrp_allreduce_bucket): not built, on
 * purpose.  Packed weights, workspaces and launch tables are caller-owned buffers, so there is nothing for a handle to
 * hold; the gradient all-reduce goes through torch.distributed (RCCL) on the caller's flat gradient arena
 * (hrpe_amd/parallel.py).  What IS process-global: the per-kernel "dynamic LDS limit raised" flags and the tuning
 * knobs read from the environment on first use (static locals of the launch functions).  They are written once
 * with idempotent values, so concurrent first calls from several host threads are harmless, but the library is
 * designed for ONE launching thread per process (one process per GPU); hrp_last_error() is thread-local.
 *
 * Tensor layout: activations are NHWC ("pixel-major": N, H, W, C with C contiguous), element type
 * hrp_dtype (fp32 for parity runs, bf16 for speed); per-channel parameters and statistics are fp32.
 * Convolution weights are consumed in the packed layout written by hrp_pack_weights.
 *
 * Reference interface each entry replaces (file:line in Oliverbansk/Holistic-Robot-Pose-Estimation;
 * the reference reaches these through PyTorch ATen/cuDNN calls, it has no native code of its own):
 *   hrp_conv2d_fwd            nn.Conv2d forward       lib/models/backbones/HRnet.py:22-25, 65-71, 284-288,
 *                                                     200-204, 218-233, 331-337, 364-368, 377-383;
 *                             nn.Linear forward       lib/models/full_net.py:95-97, 129-131; depth_layer :159-165
 *   hrp_conv2d_bwd_weight / hrp_colsum                autograd of the above (loss.backward(), scripts/train_full.py:61);
 *                             the data gradient is hrp_conv2d_fwd itself on the transposed packing (dst_t of
 *                             hrp_pack_weights) with mirrored taps - there is no separate hrp_conv2d_bwd_data entry
 *   hrp_ew_fwd                BatchNorm2d + ReLU + residual add + nn.Upsample(nearest) + fuse sum
 *                                                     HRnet.py:45-55, 82-96, 197-208, 256-263, 539-540
 *   hrp_ew_bwd_reduce/_apply  autograd of the above
 *   hrp_bn_running_update     BatchNorm2d running statistics (momentum 0.1, HRnet.py:18)
 *   hrp_bn_fold               BatchNorm2d eval mode folded to scale/shift
 *   hrp_avgpool_fwd/_bwd      F.avg_pool2d over the whole map      HRnet.py:547-548
 *   hrp_nchw_to_nhwc          x.to(torch.float) + layout change at the stem   lib/models/full_net.py:242-243
 *   hrp_softargmax3d_fwd/_bwd HeatmapIntegralPose (hrnet branch)   lib/utils/integral.py:147-177
 *   hrp_pose_geometry_fwd/_bwd uvd_to_xyz, uvz2xyz_singlepoint, depth = gamma*k/1000
 *                                                     lib/utils/transforms.py:33-73, 133-162; full_net.py:281-305
 *   hrp_fk_project_fwd/_bwd   URDFRobot.get_keypoints[_root] + point_projection_from_3d_tensor
 *                                                     lib/utils/urdf_robot.py:82-111, 169-199;
 *                                                     lib/utils/urdfpytorch/urdf.py:3115-3140, 2344-2462;
 *                                                     lib/utils/geometries.py:100-115; lib/utils/transforms.py:17-21
 *   hrp_pnp_solve             BPnP / BPnP_m3d / BPnP_fast forward: cv2.solvePnP EPnP start + iterative LM, one call per sample
 *                                                     lib/utils/BPnP.py:24-47, 129-151, 255-278
 *   hrp_pnp_bwd               their backward (implicit-function gradient through get_coefs)
 *                                                     lib/utils/BPnP.py:50-111, 154-236, 280-341, 344-357
 *   hrp_pnp_solve_robust      BPnP_fast's cv2.solvePnPRansac start and refinement: consensus over P3P hypotheses, LM on the inliers
 *                                                     lib/utils/BPnP.py:255-278 (:267-271)
 *   hrp_pnp_bwd_masked        hrp_pnp_bwd over the points of a mask (the inliers)
 *   hrp_pnp_solve_pooled      one robust pose from all the points of a sequence (fixed-camera calibration), where the reference
 *                             solves frame by frame          scripts/test.py:121-122; lib/models/ctrnet/CtRNet.py:68-89
 *   hrp_kin_solve             joint angles (and the pose) from key-points by LM; nothing in the reference does this, which only
 *                             has the `known_joint` switch          scripts/test.py
 *   hrp_kin_solve_views       hrp_kin_solve's joints from the key-points of several fixed, calibrated cameras at once
 *   hrp_dream_augment         DreamDataset's colour jitter, occlusion fill and ImageEnhance.Sharpness over the working frame,
 *                             and the convert("L") sums of ImageEnhance.Contrast
 *                                                     lib/dataset/dream.py:226-255; roboutils.py:163-195; augmentations.py:96-123
 *   hrp_dream_crop_resize     resize_image + CropResizeToAspectAugmentation with the Contrast / Brightness / Color tail
 *                                                     lib/dataset/roboutils.py:128-156; augmentations.py:96-123, 170-242
 *   hrp_eval_batch            the validation metrics of one batch (both compute_metrics_batch calls + the geodesic rotation
 *                             distance) into epoch-length device accumulators
 *                                                     lib/core/function.py:137-179; lib/utils/metrics.py:36-113;
 *                                                     lib/utils/geometries.py:21-41, 100-115, 154-162
 *   hrp_depth_loss            what the DepthNet trainer's step derives from the model output: the depth loss (l1 | mse; plain,
 *                             xy branch, multi_kp), its gradient, and the per-image errors of the validation pass into
 *                             epoch-length device accumulators
 *                                                     scripts/train_depthnet.py:220-268, 276-303
 *   hrp_sim2real_monitor      the self-supervised trainer's per-step bookkeeping: the seven supervised terms it logs, next to the
 *                             mask terms of hrp_sim2real_loss, into meters that live on the device
 *                                                     scripts/train_sim2real.py:313-400, 558-569, 649-660;
 *                                                     lib/utils/transforms.py:17-21
 *   hrp_jpeg_decode           the JPEG decode behind DreamDataset's np.asarray(Image.open(rgb_path)) for baseline files: entropy
 *                             decoding, inverse DCT, chroma up-sampling and colour conversion of a batch
 *                                                     lib/dataset/dream.py:110
 *   hrp_jpeg_decode_sync      the same with a long segment (a file without restart markers) decoded by one workgroup from
 *                             speculative start points
 *   hrp_track_prepare         the loader's crop / K / box / k_value geometry (get_bbox, resize_image, get_K_crop_resize,
 *                             bbox_transform, get_extended_bbox, k_values) from the LAST pose estimate instead of the annotation,
 *                             and the crop + bilinear resize of both views straight from the frame, in one launch
 *                                                     lib/dataset/dream.py:171-216, 287-394; roboutils.py:59-156, 224-257;
 *                                                     lib/utils/geometries.py:360-395; lib/core/function.py:43-48, 88-98
 *   hrp_track_seed            tracker acquisition from a detector's key-points (CtRNet's KeyPointSegNet, hrp_kp_readout_fwd)
 *   hrp_track_verify          the estimate against the detector's foreground map (skeleton support, box coverage, silhouette
 *                             IoU); a stream that disagrees drops its estimate    scripts/train_sim2real.py (the IoU measure)
 *   hrp_track_update          the projection of the model's FK key-points into the original image, which becomes the estimate the
 *                             next frame is cropped from          lib/utils/geometries.py:100-115; lib/dataset/dream.py:171-216
 *   hrp_kp_readout_fwd        CtRNet's key-point branch: ConvTranspose2d read-out + spatial soft-argmax, the heat-map kept in fp32
 *                             registers                           lib/models/ctrnet/keypoint_seg_resnet.py:29-33, 75-100, 137-143
 */
#ifndef HRP_H
#define HRP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* HRP_F32X3 (convolutions and the weight packing only): fp32 tensors, every product formed as three bf16 MFMAs on split operands
 * (x = hi + lo; x w ~ hi hi + hi lo + lo hi: ~2^-16 relative per product, a third of the bf16 matrix rate instead of the fp32 matrix
 * cores' sixteenth).  hrp_pack_weights(dtype = HRP_F32X3) writes the packed rows pre-split ([8 hi | 8 lo] bf16 per 32-byte row); the
 * convolution kernels split the activations on the fly.  Everything else about such a problem is HRP_F32. */
typedef enum { HRP_F32 = 0, HRP_BF16 = 1, HRP_F32X3 = 2 } hrp_dtype;

typedef enum {
  HRP_OK = 0,
  HRP_ERR_ARG = -1,     /* bad descriptor (shape / alignment / unsupported combination) */
  HRP_ERR_LAUNCH = -2,  /* HIP reported an error at launch */
  HRP_ERR_NODEV = -3    /* no usable gfx950 device */
} hrp_status;

#define HRP_MAX_TAPS 16

/* Per-channel statistics (BN forward sum/sumsq, BN backward sums): every workgroup reduces its share in fp32 in a fixed order
 * and adds ONE partial per channel with an fp64 atomic.  The order of those atomics varies from run to run; in fp64 the
 * rounding of the total does not depend on it in practice (fp32 partials, < 2^11 of them per slot), so the fp32 constants
 * every consumer derives - and with them every ReLU decision of a training step - repeat bit for bit.  (Round 2 used fp32
 * atomics: the last bit of a sum moved between runs, a bf16 rounding then flipped and a ReLU mask with it: ~1 % run-to-run
 * spread of bf16 gradients.)  Same-address atomics serialise (~20 ns each on MI355X), so every statistics buffer has
 * HRP_STAT_SLOTS replicas laid out [slot][2*C] doubles; a workgroup adds into slot (blockIdx & (SLOTS-1)) and readers sum
 * the slots.  The caller zeroes all slots before the producing launch. */
#define HRP_STAT_SLOTS 8

/* One convolution "problem": out[n, oy, ox, co] = sum_t sum_ci in[n, oy*IS+dy[t], ox*IS+dx[t], ci] * W[t][co][ci].
 * Covers conv k1/k3 stride 1/2 forward, its data gradient (stride 1: mirrored taps, stride 2: one call per
 * output parity class with out_stride = 2), and nn.Linear (H = W = 1). */
typedef struct hrp_conv_desc {
  const void* x;       /* input  [N, H, W, x_pitch], first Cin channels used                     */
  const void* w;       /* packed weights, see hrp_pack_weights: [chunk][tap][Cout_pad][CK]        */
  void* y;             /* output [N, y_H, y_W, y_pitch]                                           */
  const void* res;     /* optional residual added in the epilogue, geometry of y (res_pitch)      */
  const float* bias;   /* optional [Cout]                                                         */
  const float* scale;  /* optional per-channel affine applied after bias: v*scale+shift           */
  const float* shift;
  double* stats;       /* optional [HRP_STAT_SLOTS][2*Cout]: += sum(y), sum(y*y) over output pixels */
  int32_t dtype;       /* hrp_dtype of x, w, y, res                                               */
  int32_t N, H, W, Cin, x_pitch;
  int32_t Ho, Wo, Cout; /* logical output grid walked by the kernel                               */
  int32_t y_H, y_W, y_pitch, res_pitch;
  int32_t out_stride, out_off_y, out_off_x; /* (oy,ox) is stored at (oy*out_stride+off_y, ox*...+off_x) */
  int32_t in_stride;   /* IS */
  int32_t ntaps;
  int32_t dy[HRP_MAX_TAPS], dx[HRP_MAX_TAPS];
  int32_t wtap[HRP_MAX_TAPS]; /* tap slot of the packed weights used by tap t                     */
  int32_t w_ntaps;     /* tap slots per chunk in the packed weights                               */
  int32_t w_cout_pad;  /* Cout rounded up to 32 (row count per tap in the packed weights)         */
  int32_t relu;
  /* Data-gradient launches only (all NULL / 0 otherwise): the BatchNorm-backward REDUCE pass of the activation whose
   * gradient this launch produces, folded into the epilogue.  y is the gradient of act = relu(bn(bnb_x)); with these
   * set, `stats` receives  sum(g), sum(g * (bnb_x - mean) * invstd)  with g = y masked by the ReLU bit mask - exactly
   * what hrp_ew_bwd_reduce would compute from y in a separate pass over y and bnb_x (the reference runs it inside
   * autograd's native_batch_norm_backward, HRnet.py:41-57).  Needs: no res / relu / bias / scale, out_stride 1,
   * Cout a multiple of the 16-byte vector, 16-byte aligned rows; y itself is stored unmasked. */
  const void* bnb_x;        /* forward input of the BatchNorm [N, Ho, Wo, bnb_x_pitch], dtype of y             */
  const uint8_t* bnb_mask;  /* ReLU bit mask of the activation (hrp_ew_desc.mask), one byte per vector          */
  const float* bnb_consts;  /* [2 * Cout]: mean, invstd of the BatchNorm input (hrp_ew_desc.consts_out)        */
  int32_t bnb_x_pitch, bnb_mask_pitch;
  /* ---- fields below: row-strip kernels only (hrp_conv_rowstrip_channels(d) != 0: the 3x3 stride-1 C -> C layers of the
   * HRNet branches, bf16, dense NHWC rows of 4 KiB: C = 32 @ W = 64, C = 64 @ W = 32, C = 128 @ W = 16, C = 256 @ W = 8,
   * H a multiple of 8).  Any other problem that sets them is HRP_ERR_ARG: callers ask hrp_conv_rowstrip_channels first.
   * (The bnb_stats form of the epilogue reduce, with or without bnb_mask / res, is also taken by the pointwise kernel:
   * hrp_conv_pointwise.)
   * bnb_x with bnb_stats set: the BatchNorm constants of the epilogue reduce are derived in the kernel from bnb_stats (the forward
   * sum / sum-of-squares slots of bnb_x), bnb_gamma, bnb_beta, bnb_count, bnb_eps; with bnb_mask == NULL the ReLU mask is
   * recomputed from bnb_x itself, mask = (bn(bnb_x) > 0) - the arithmetic the forward prologue (pro_mode 1) applied -, else
   * the bit mask is read ([pixels][C / 8] bytes).  `res` (== y: accumulate onto the other producers of the gradient) is
   * allowed here: the sums are taken over the final stored value. */
  const double* bnb_stats;
  const float* bnb_gamma;
  const float* bnb_beta;
  float bnb_count, bnb_eps;
  /* Input transform applied while x is staged (reference HRnet.py:41-50: conv2(relu(bn1(conv1(x)))) and its autograd):
   *   pro_mode 1: x' = relu(gamma * (x - mean) * invstd + beta) - train-mode BatchNorm of x from pro_stats (the sum /
   *               sum-of-squares slots written by the epilogue of x's producer): the activation is never materialised
   *               for this layer's forward (replaces an hrp_ew_fwd pass);
   *   pro_mode 2: x' = gamma * invstd * (g - k0 - xhat * k1),  g = x * [bn(pro_x2) > 0],  xhat = (pro_x2 - mean) * invstd,
   *               k0 / k1 = slot sums of pro_bsums / count: x is the gradient of relu(bn(pro_x2)), x' the gradient of
   *               pro_x2 - what hrp_ew_bwd_apply computes in a pass of its own;
   *   pro_mode 3: x' = relu(gamma * (x - mean) * invstd + beta + pro_x2) - the block-end activation of the PREVIOUS BasicBlock
   *               (HRnet.py:52-56: x = that block's raw conv2 output, pro_x2 = its input, pro_stats the statistics of x) applied while
   *               this block's first convolution stages its rows; pro_side (required) receives x', pro_mask (required, an OUTPUT in
   *               this mode) its ReLU bits in the layout of hrp_ew_desc.mask - replaces that block's hrp_ew_fwd pass;
   *   pro_side  (optional, geometry of x): x' is also written there, every pixel once - the operand the weight gradient
   *               of the neighbouring layer reads (forward: the activation; backward: the BatchNorm input gradient). */
  int32_t pro_mode, pro_reserved;
  const void* pro_x2;
  const double* pro_stats;
  const double* pro_bsums;
  const float* pro_gamma;
  const float* pro_beta;
  float pro_count, pro_eps;
  void* pro_side;
  /* pro_mode 2 only: pro_mask (optional) = the ReLU bit mask hrp_ew_fwd wrote for the activation ([pixels][C / 8] bytes, bit i =
   * channel i of the 16-byte vector was > 0) instead of recomputing the mask from pro_x2 - the activation then may have had
   * further summands (the residual of a block output, HRnet.py:52-56); pro_side2 (optional, geometry of x) = the masked gradient
   * g itself, i.e. the gradient of an identity (residual) summand of that activation, written (pro_side2_acc 0) or accumulated. */
  const uint8_t* pro_mask;
  void* pro_side2;
  int32_t pro_side2_acc, pro_reserved2;
  /* res_mask (optional, row-strip kernels, with res): ReLU bit mask ([pixels][Cout / 8] bytes) applied to the residual before it
   * is added: y = conv(x') + [bit] * res.  The data gradient of a block's first conv then produces the WHOLE gradient of the
   * block input in one write - conv1's data gradient plus the gradient of the identity shortcut, which is the block output's
   * gradient masked by the block-end ReLU (HRnet.py:52-56) - instead of accumulating onto a tensor another launch wrote. */
  const uint8_t* res_mask;
  /* ---- pointwise kernel only (hrp_conv_pointwise(d) != 0, Cin 32 / 64, Cout a multiple of 64): the tail of a train-mode Bottleneck,
   * out = relu(bn3(conv3(h)) + shortcut) (HRnet.py:88-96), WITHOUT storing conv3's raw output - a 64 -> 256 product is cheaper to
   * recompute from its 33 MB input than its 134 MB output is to write and read back (B = 64).  tail_mode:
   *   1  statistics only: stats += sum / sum of squares of the (unrounded) product over the pixels; nothing is stored (y unused)
   *   2  y = relu(bn(product) + res): batch statistics from tail_stats (the slots a mode-1 launch filled), tail_gamma / _beta / _count /
   *      _eps; res = the shortcut (geometry of y, required); the ReLU bits of y go to tail_mask ([pixels][Cout / 8] bytes, the
   *      layout of hrp_ew_desc.mask)
   *   3  backward reduce of that BatchNorm: the product is recomputed, g = tail_g masked by tail_mask;
   *      stats += sum g, sum g * xhat (the slots hrp_bn_param_grad and mode 4 read); nothing is stored
   *   4  backward apply: y = gamma invstd (g - k0 - xhat k1), k0 / k1 = slot sums of tail_bsums / tail_count - the gradient of the
   *      product, which the ordinary data- and weight-gradient launches of the layer then read; tail_side (optional, geometry of y)
   *      = or += (tail_side_acc) g: the gradient of the identity shortcut. */
  /*   5  mode 2 with a PROJECTION shortcut (the first block of a stack, HRnet.py:139-150: downsample = conv1x1 + BatchNorm):
   *      y = relu(bn(product) + bn2(product2)), product2 = tail_x2 (geometry and channels of x) times tail_w2 (packed like w, same
   *      Cout), batch statistics tail_stats2 / tail_gamma2 / tail_beta2 (count and eps as the first).  Its statistics and its backward
   *      are mode 1 / 3 / 4 launches of their own on (tail_x2, tail_w2): neither raw product is ever stored. */
  int32_t tail_mode, tail_side_acc;
  const double* tail_stats;
  const double* tail_bsums;
  const float* tail_gamma;
  const float* tail_beta;
  float tail_count, tail_eps;
  uint8_t* tail_mask;
  const void* tail_g;
  void* tail_side;
  const void* tail_x2;
  const void* tail_w2;
  const double* tail_stats2;
  const float* tail_gamma2;
  const float* tail_beta2;
} hrp_conv_desc;

/* Weight gradient: dW[co][ci][t] (+)= sum_{n,oy,ox} dy[n,oy,ox,co] * x[n, oy*IS+dy[t], ox*IS+dx[t], ci],
 * written in fp32 straight into the PyTorch-shaped gradient tensor [Cout][dw_cin][ntaps], dw_cin <= Cin: the real input
 * channels.  Channels of x at or beyond dw_cin (padding up to Cin) and lanes of dy at or beyond Cout are masked at the store. */
typedef struct hrp_wgrad_desc {
  const void* x;       /* forward input  [N, H, W, x_pitch] */
  const void* dy;      /* output grad    [N, Ho, Wo, dy_pitch] */
  float* dw;           /* fp32 [Cout][dw_cin][ntaps] */
  int32_t dtype;
  int32_t N, H, W, Cin, x_pitch;
  int32_t Ho, Wo, Cout, dy_pitch;
  int32_t in_stride, ntaps;
  int32_t dy_t[HRP_MAX_TAPS], dx_t[HRP_MAX_TAPS];
  int32_t dw_cin;      /* row length (in taps groups) of dw: element (co,ci,t) at (co*dw_cin+ci)*ntaps+t */
  int32_t dw_tap_stride; /* 0: ntaps.  > 0: taps per (co,ci) in dw when this launch computes only the tap group  */
  int32_t dw_tap_off;    /* [dw_tap_off, dw_tap_off + ntaps) of a larger kernel (4x4 / 7x7 kernels run as groups  */
                         /* of 4 / 9 taps): element (co,ci,t) at (co*dw_cin+ci)*dw_tap_stride + dw_tap_off + t     */
  int32_t accumulate;  /* 0: dw is overwritten, 1: add to existing */
  void* workspace;     /* optional scratch of hrp_wgrad_workspace_bytes(): partial sums are written there
                          and reduced by a second launch instead of fp32 atomics into dw */
  int64_t workspace_bytes;
  int32_t phase;       /* 0: the whole gradient.  1 (needs the workspace): partial sums only - the caller folds them
                          later with a HRP_BATCH_WGRAD_FOLD launch (the workspace must stay untouched until then) */
  int32_t reserved;
} hrp_wgrad_desc;

/* The deferred second half of a weight gradient (phase 1 above): dw (+)= sum over the G partial slabs.  Filled by
 * hrp_wgrad_fold_desc_of (single launches) / hrp_batch_wgrad_fold_descs (batched launches); G == 0: nothing to fold
 * (the launch took the atomics path).  One HRP_BATCH_WGRAD_FOLD launch folds up to HRP_BATCH_MAX problems of ANY tap
 * count / element type: a training step folds all its ~600 weight gradients in ~20 launches at the end of the lanes
 * instead of one 6-10 us launch behind every weight-gradient launch. */
typedef struct hrp_wgrad_fold_desc {
  const float* workspace;  /* [G][pairs][nte * 1024] */
  float* dw;
  int32_t G, pairs, n_cib, nte, nb;
  int32_t Cout, dw_cin, ntaps, dw_tap_stride, dw_tap_off, accumulate;
  int32_t reserved;
} hrp_wgrad_fold_desc;

/* Weight packing table entry (one launch packs every conv / linear weight of a network).
 * src: fp32 [Cout][Cin][ntaps] (PyTorch [Cout][Cin][KH][KW]).  CK = 32 bytes / sizeof(elem).
 * dst   (forward):       [ceil(Cin/CK)][tap][Cout_pad][CK],  value W[co][chunk*CK+k][tap]
 * dst_t (data gradient): [ceil(Cout/CK)][tap][Cin_pad][CK],  value W[chunk*CK+k][ci][tap]
 * Cout_pad / Cin_pad = round_up(.., 32); everything outside the real extents is zero. */
typedef struct hrp_pack_entry {
  const float* src;
  void* dst;           /* forward packing or NULL */
  void* dst_t;         /* transposed (data-gradient) packing or NULL */
  int32_t Cout, Cin, ntaps;
  int32_t pad_t;       /* extra tap slots per chunk of the transposed packing (never written: they stay what the caller put    */
                       /* there - zeros).  A data gradient refers to such a slot (hrp_conv_desc.wtap) for a tap it does not have: */
                       /* the four output-parity classes of a stride-2 3x3 layer (1 / 2 / 2 / 4 taps) then all run as 4-tap       */
                       /* problems of ONE batched launch */
} hrp_pack_entry;

#define HRP_EW_MAX_IN 4
/* inputs of the fused element-wise op: out = act( sum_j f_j(in_j[up_j(p)]) ),
 * f_j = identity | per-channel affine | train-mode batch-norm from (sum, sumsq) statistics */
typedef enum { HRP_EW_IDENTITY = 0, HRP_EW_AFFINE = 1, HRP_EW_BN_TRAIN = 2 } hrp_ew_mode;

typedef struct hrp_ew_input {
  const void* ptr;     /* [N, H/up, W/up, pitch] */
  int32_t pitch;
  int32_t up;          /* nearest-neighbour upsample factor (1, 2, 4, 8) */
  int32_t mode;        /* hrp_ew_mode */
  const float* a;      /* AFFINE: scale[C]; BN_TRAIN: gamma[C] */
  const float* b;      /* AFFINE: shift[C]; BN_TRAIN: beta[C]  */
  const double* stats; /* BN_TRAIN: [HRP_STAT_SLOTS][2C] sum, sumsq of this input over its own pixels */
  float count;         /* BN_TRAIN: number of pixels the statistics were taken over */
  float eps;
} hrp_ew_input;

typedef struct hrp_ew_desc {
  hrp_ew_input in[HRP_EW_MAX_IN];
  int32_t nin;
  void* out;           /* [N, H, W, out_pitch] */
  int32_t out_pitch;
  int32_t dtype;
  int32_t N, H, W, C;
  int32_t relu;        /* 0: none, 1: ReLU, 2: LeakyReLU with slope 0.01 (nn.LeakyReLU(); the backward descriptor carries it on) */
  uint8_t* mask;       /* optional with relu: one byte per 16-byte output vector (8 bf16 / 4 fp32 channels),   */
  int32_t mask_pitch;  /* bit i = (channel i of the vector > 0); [N*H*W][mask_pitch] bytes.  The backward then  */
                       /* reads 1/16 of the bytes of `out` for the ReLU mask.  Vector path only (C, pitches and */
                       /* pointers 16-byte aligned), an error otherwise.                                        */
  float* consts_out;   /* optional, in[0].mode == HRP_EW_BN_TRAIN: [2C] mean, invstd of input 0 as this launch  */
                       /* derived them from the statistic slots (read by hrp_conv_desc.bnb_consts in backward) */
} hrp_ew_desc;

/* Backward of one input j of an ew op.  g = dOut * (out > 0 if relu), pooled (summed) over the
 * up x up footprint.  reduce: sums[0:C] += sum g, sums[C:2C] += sum g * xhat (BN/affine inputs).
 * apply: din = identity: g | affine: a*g | bn_train: a*invstd*(g - sums0/count - xhat*sums1/count). */
typedef struct hrp_ew_bwd_desc {
  const void* dout;    /* [N, H, W, dout_pitch] */
  const void* out;     /* forward output (relu mask), may be NULL when relu == 0 */
  int32_t dout_pitch, out_pitch;
  hrp_ew_input in;     /* the forward input this call differentiates (ptr = forward input values) */
  void* din;           /* [N, H/up, W/up, din_pitch]; apply only */
  int32_t din_pitch;
  double* sums;        /* [HRP_STAT_SLOTS][2C] */
  int32_t dtype;
  int32_t N, H, W, C;  /* geometry of out */
  int32_t relu;
  int32_t accumulate;  /* apply: din += */
  const uint8_t* mask; /* optional ReLU bit mask written by hrp_ew_fwd (see hrp_ew_desc.mask); replaces `out` */
  int32_t mask_pitch;
  void* din2;          /* apply, optional, in.up == 1 only: second output = the masked gradient g itself, i.e. */
  int32_t din2_pitch;  /* the gradient of an identity (residual) input of the same activation - saves the   */
  int32_t accumulate2; /* separate identity launch that would re-read dout / out; din2 += when accumulate2  */
  /* in.up > 1 (an upsampled input of a fuse layer, HRnet.py:197-208, 256-263): optional fp32 [N, H/up, W/up, C] dense tensor holding
   * the output gradient already masked and summed over the up x up window of every input pixel (hrp_ew_pool2, applied log2(up)
   * times).  Reduce and apply then read it instead of pooling dout under the mask again - the 2 / 4 / 8-fold terms of one fuse sum
   * each pooled the same [N, H, W, C] gradient twice (six passes over it per stage-4 output; now one). */
  const float* pooled;
} hrp_ew_bwd_desc;

/* Table entry for the one-launch batch-norm bookkeeping kernels. */
typedef struct hrp_bn_entry {
  const double* stats; /* [HRP_STAT_SLOTS][2C] forward sums (running_update) or backward sums (param_grad) */
  float* a;            /* running_update: running_mean | fold: gamma | param_grad: dgamma */
  float* b;            /* running_update: running_var  | fold: beta  | param_grad: dbeta  */
  const float* c;      /* fold: running_mean */
  const float* d;      /* fold: running_var  */
  float* out_scale;    /* fold */
  float* out_shift;    /* fold */
  int64_t* counter;    /* running_update: num_batches_tracked (may be NULL) */
  int32_t C;
  float count, momentum, eps;
  int32_t accumulate;  /* param_grad: += */
} hrp_bn_entry;

/* Kinematic chain descriptor for hrp_fk_project_* (built by the host from a URDF). */
#define HRP_FK_MAX_JOINTS 32
#define HRP_FK_MAX_KP 24
typedef struct hrp_fk_chain {
  int32_t njoints;                       /* joints in base->leaf order                          */
  int32_t parent[HRP_FK_MAX_JOINTS];     /* index of the parent joint's child frame, -1 = base */
  int32_t type[HRP_FK_MAX_JOINTS];       /* 0 fixed, 1 revolute/continuous, 2 prismatic        */
  int32_t cfg[HRP_FK_MAX_JOINTS];        /* column of q driving the joint, -1 none             */
  float mimic_mul[HRP_FK_MAX_JOINTS], mimic_off[HRP_FK_MAX_JOINTS];
  float origin[HRP_FK_MAX_JOINTS][12];   /* rows of the 3x4 origin transform                   */
  float axis[HRP_FK_MAX_JOINTS][3];      /* unit axis                                          */
  int32_t nkp;
  int32_t kp_frame[HRP_FK_MAX_KP];       /* joint index whose child frame carries the keypoint, -1 = base */
  float kp_offset[HRP_FK_MAX_KP][3];
  int32_t dof;
} hrp_fk_chain;

const char* hrp_last_error(void);
int hrp_version(void);
/* first 16 hex digits of the sha256 over the library's sources (csrc/*.hip, csrc/*.h, this header, the Makefile, sorted by
 * name) this binary was compiled from; __graft_entry__.build() compares it with the tree it runs in */
const char* hrp_source_hash(void);
int hrp_device_ok(void);  /* 1 when the current HIP device is gfx950 */

int hrp_nchw_to_nhwc(const float* src, void* dst, int dtype, int N, int C, int H, int W, int dst_pitch, void* stream);
int hrp_nhwc_to_nchw(const void* src, float* dst, int dtype, int N, int C, int H, int W, int src_pitch, void* stream);
int hrp_nchw_grad_from_nhwc(const void* src, float* dst, int dtype, int N, int C, int H, int W, int src_pitch, void* stream);
/* Dataset bytes straight into the trunk's input layout: dst = float(src) * (1.0f / divisor) - what
 * `.float() / 255.` (lib/core/function.py:26,29) evaluates to on the device, where ATen multiplies by the fp32
 * reciprocal of a host scalar - as NHWC or (s2d != 0) the 2x2 space-to-depth form of the ResNet stem. */
int hrp_u8_nchw_to_nhwc(const uint8_t* src, void* dst, int dtype, int N, int C, int H, int W, int dst_pitch,
                        float divisor, int s2d, void* stream);
int hrp_pack_weights(const hrp_pack_entry* table_dev, int count, int dtype, int max_elems, void* stream);
/* The same packing for a whole network's table with a compact grid: entry i is packed by the workgroups first_block[i] ..
 * first_block[i + 1] - 1 (first_block_dev: count + 1 int32 on the device, EXACTLY hrp_pack_blocks() workgroups per entry;
 * total_blocks = first_block[count]).  hrp_pack_weights gives every entry the workgroups of the largest one. */
int hrp_pack_blocks(int Cout, int Cin, int ntaps, int dtype, int has_dst, int has_dst_t);   /* host only */
int hrp_pack_weights_compact(const hrp_pack_entry* table_dev, const int32_t* first_block_dev, int count, int total_blocks,
                             int dtype, void* stream);
/* ResNet stem (lib/models/backbones/Resnet.py:21-25): the 7x7 stride-2 convolution runs as a 4x4 stride-1
 * convolution over the 2x2 space-to-depth image.  dst[n, y, x, (dy*2+dx)*C + c] = src[n, c, 2y+dy, 2x+dx]. */
int hrp_nchw_to_nhwc_s2d(const float* src, void* dst, int dtype, int N, int C, int H, int W, int dst_pitch, void* stream);
/* dst[i] (+)= idx[i] >= 0 ? src[idx[i]] : 0 - the re-layout of the stem weight into its 4x4 / 12-channel form and
 * of the weight gradient back into the [64, 3, 7, 7] parameter. */
int hrp_gather_f32(const float* src, const int32_t* idx, float* dst, int n, int accumulate, void* stream);
/* stream-ordered memset(p, 0, bytes) (gradient buffers only partly written by a strided data gradient) */
int hrp_fill_zero(void* p, int64_t bytes, void* stream);
/* nn.MaxPool2d(3, stride 2, padding 1) (Resnet.py:25) on NHWC; argmax (optional, [N,Ho,Wo,C] bytes) keeps the window
 * slot 0..8 of the first maximum for the backward, which is a gather over the <= 4 windows of an input pixel. */
int hrp_maxpool3x3s2_fwd(const void* x, int dtype, int N, int H, int W, int C, int pitch, void* y, int y_pitch,
                         uint8_t* argmax, void* stream);
int hrp_maxpool3x3s2_bwd(const void* dy, int dy_pitch, const uint8_t* argmax, void* dx, int dtype, int N, int H, int W,
                         int C, int pitch, int accumulate, void* stream);

int hrp_conv2d_fwd(const hrp_conv_desc* d, void* stream);
/* 32 / 64 / 128 / 256 (the channel count) when hrp_conv2d_fwd (and a HRP_BATCH_CONV launch) will run problem d on a row-strip
 * kernel - the only ones that honour pro_mode / pro_side / pro_mask / pro_side2 - else 0.  Host only. */
int hrp_conv_rowstrip_channels(const hrp_conv_desc* d);
/* 1 when hrp_conv2d_fwd will run problem d on the pointwise kernel (csrc/conv_pw.h: dense bf16 1x1 stride-1 layers with 32 ..
 * 256 input channels and >= 131 072 output pixels - the Bottleneck 1x1 layers at 64 x 64, HRnet.py:60-98), else 0.  Such a
 * problem placed in a HRP_BATCH_CONV launch runs the general tile program: callers launch it on its own.  Host only. */
int hrp_conv_pointwise(const hrp_conv_desc* d);
/* 1 when d is one output-parity class of the data gradient of a 3x3 stride-2 padding-1 layer in the form the parity-fused kernel
 * (csrc/conv_parity.h) takes: bf16, in_stride 1, out_stride 2, offsets in {0, 1}^2, y_H = 2 Ho and y_W = 2 Wo, the class's 1 / 2 /
 * 2 / 4 taps on slots of a 9- or 10-slot packing (further taps, up to four, must read the zero slot 9), Cin a multiple of 16, Cout
 * of 8, 16-byte pitches, nothing of the epilogue set but `res`.  A HRP_BATCH_CONV prepare whose n problems are the four classes of
 * n / 4 layers (equal x, w, y, res and shapes; any order, any mix of padded and unpadded tap counts) runs one fused problem per
 * layer; any other batch takes the ordinary path.  Reads no pointer.  Host only. */
int hrp_conv_parity_fusable(const hrp_conv_desc* d);
/* Process-wide switch of that grouping, on by default: 0 makes every later HRP_BATCH_CONV prepare take the ordinary path, also for
 * complete quadruples (four padded 4-tap problems share one launch of the ordinary kernel) - the reference side of an A/B
 * measurement in one process.  -> the previous setting. */
int hrp_conv_parity_fuse_enable(int on);
/* CT * 1000 + PT * 100 + WC * 10 + WP - the tile configuration (csrc/conv_tile.h: 32 CT WC output channels x 32 PT WP pixels per
 * workgroup, WC x WP waves) - when hrp_conv2d_fwd will run problem d on the general tile program, + 10000 when that launch splits K
 * (two workgroups per output tile, fp32 atomics): 2214, 2114, 1122, 1214 or 1114.  0 when d runs on the row-strip or the pointwise
 * kernel, is not a valid problem, or fits no configuration.  The answer comes out of the launcher's own candidate walk.  Host only. */
int hrp_conv_tile_config(const hrp_conv_desc* d);
int hrp_conv2d_bwd_weight(const hrp_wgrad_desc* d, void* stream);
/* scratch bytes hrp_conv2d_bwd_weight wants for this problem (0 is never returned for a valid problem) */
int64_t hrp_wgrad_workspace_bytes(const hrp_wgrad_desc* d);
/* out[c] (+)= sum over rows of x[rows, pitch] (bias gradients) */
/* workspace (hrp_colsum_workspace_bytes(rows, C) bytes, no initialisation; NULL: fp32 atomics, order-dependent last bits): the
 * row groups' partial sums are parked there and added in a fixed order by a second small launch */
int64_t hrp_colsum_workspace_bytes(int64_t rows, int C);
int hrp_colsum(const void* x, int dtype, int64_t rows, int C, int pitch, float* out, int accumulate, void* workspace,
               int64_t workspace_bytes, void* stream);

/* ---- optimizer step of the training loop (torch.nn.utils.clip_grad_norm_ + torch.optim.Adam.step, the pair
 * scripts/train_full.py:42 / lib/core/function.py use), table driven: one launch per pass for all parameters.
 * A chunk is up to HRP_OPT_CHUNK consecutive elements of one tensor. */
#define HRP_OPT_CHUNK 4096
typedef struct hrp_opt_tensor {
  float* param;        /* fp32 master parameter                    */
  float* grad;         /* fp32 gradient (scaled in place by the clip coefficient, as clip_grad_norm_ does) */
  float* exp_avg;      /* Adam first moment                         */
  float* exp_avg_sq;   /* Adam second moment                        */
  int64_t numel;
} hrp_opt_tensor;
typedef struct hrp_opt_chunk {
  int32_t tensor;      /* index into the tensor table               */
  int32_t offset;      /* first element, in units of HRP_OPT_CHUNK  */
} hrp_opt_chunk;
/* Sum of grad^2 over all chunks.  chunk_sums == NULL: sumsq_slots[HRP_STAT_SLOTS] += (fp32 atomics; the caller zeroes the
 * slots; the total depends on the order the chunks finish in, to an ulp).  chunk_sums = nchunks floats of scratch: every
 * chunk writes its own sum and a second launch folds them in a FIXED order into sumsq_slots[0] (the other slots are set to
 * 0): the same bits on every data-parallel rank that holds the same gradients - what keeps replicas identical through
 * hrp_opt_adam_step's clip coefficient (torch.nn.utils.clip_grad_norm_ under DataParallel runs once, on one device). */
int hrp_opt_grad_sumsq(const hrp_opt_tensor* tensors_dev, const hrp_opt_chunk* chunks_dev, int nchunks,
                       float* sumsq_slots, float* chunk_sums, void* stream);
/* total_norm = sqrt(sum of the slots); clip = min(1, max_norm / (total_norm + 1e-6)) (max_norm <= 0: no clipping);
 * g = grad * clip (written back); *step_dev is the number of the step being taken (the caller increments it
 * before the launch); Adam without weight decay / amsgrad:
 *   m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;  p -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps) */
int hrp_opt_adam_step(const hrp_opt_tensor* tensors_dev, const hrp_opt_chunk* chunks_dev, int nchunks,
                      const float* sumsq_slots, float max_norm, const float* step_dev,
                      float lr, float beta1, float beta2, float eps, void* stream);
/* The same step with its hyper-parameters in DEVICE memory: parameter groups, torch.optim.Adam's weight_decay, and a learning
 * rate that a scheduler changes between replays of a captured HIP graph (LambdaLR over Adam, lib/utils/utils.py:147-189;
 * hrp_opt_adam_step bakes lr into the captured launch).  One row per parameter group: */
typedef struct hrp_opt_group {
  float lr, beta1, beta2, eps;
  float weight_decay;  /* L2 as torch.optim.Adam (not AdamW): the moments see g + weight_decay * p */
  float reserved[3];   /* 32 bytes per row */
} hrp_opt_group;
/* tensor_group_dev[i] = the group (row of groups_dev, in [0, ngroups)) of row i of the tensor table.  Every workgroup reads its
 * chunk's tensor, that tensor's group and the group's five numbers when it RUNS (a few dwords per chunk, uniform over the
 * workgroup): a replayed graph applies what the table holds at that moment.  The clip is global over all groups
 * (clip_grad_norm_(model.parameters()): hrp_opt_grad_sumsq as above) and the clipped gradient is written back WITHOUT the decay
 * term; with p the parameter before the update,
 *   ge = g + weight_decay p;  m = b1 m + (1-b1) ge;  v = b2 v + (1-b2) ge^2;  p -= lr / (1 - b1^step) * m / (sqrt(v) / sqrt(1 - b2^step) + eps)
 * A group with weight_decay == 0 runs hrp_opt_adam_step's instructions: one such group gives the same bits as that entry. */
int hrp_opt_adam_step_groups(const hrp_opt_tensor* tensors_dev, const hrp_opt_chunk* chunks_dev, int nchunks,
                             const float* sumsq_slots, float max_norm, const float* step_dev,
                             const hrp_opt_group* groups_dev, int ngroups, const int32_t* tensor_group_dev, void* stream);
/* Writes row `index` of a table of ngroups rows: a one-thread launch on `stream`, ordered like any other work there.  The values
 * travel as launch arguments (no staging buffer that the host could overwrite while an earlier launch is queued).  NOT to be
 * captured into the graph that holds the step: a captured setter would rewrite the captured values at every replay. */
int hrp_opt_set_group(hrp_opt_group* groups_dev, int ngroups, int index, float lr, float beta1, float beta2, float eps,
                      float weight_decay, void* stream);
/* Gradient accumulation over micro-batches (PlannedModule.set_grad_accumulation): one streaming pass over a plan's flat
 * gradient arena,   acc[i] = (first ? 0 : acc[i]) + scale * src[i]   fp32, n elements, src and acc 16-byte aligned and
 * distinct.  first != 0 does not read acc (whatever it held, NaNs included, is overwritten: no memset in front).  scale == 1
 * gives the exact fp32 sum acc + src; any other scale rounds the product and the sum separately (no FMA): the bits of
 * acc + (src * scale) formed by two fp32 element-wise passes. */
int hrp_grad_accumulate(const float* src, float* acc, int64_t n, int first, float scale, void* stream);

int hrp_ew_fwd(const hrp_ew_desc* d, void* stream);
int hrp_ew_bwd_reduce(const hrp_ew_bwd_desc* d, void* stream);
/* dst[n, y, x, c] (fp32, dense [N, H/2, W/2, C]) = sum over the 2 x 2 window of src[n, 2y + dy, 2x + dx, c] * bit: the first level
 * (src_dtype HRP_BF16 / HRP_F32 of the plan, mask = the ReLU bits of hrp_ew_desc.mask, one byte per 16-byte vector) pools the masked
 * output gradient of a fuse sum, further levels (src_dtype HRP_F32, mask NULL, src = the previous level) halve it again.  Fixed
 * summation order ((a + b) + (c + d)); H, W even, C a multiple of 8. */
int hrp_ew_pool2(const void* src, int src_dtype, int src_pitch, const uint8_t* mask, int mask_pitch, int N, int H, int W, int C, float* dst,
                 void* stream);
int hrp_ew_bwd_apply(const hrp_ew_bwd_desc* d, void* stream);

/* ---- batched launches ---------------------------------------------------------------------------------------
 * n <= HRP_BATCH_MAX independent problems of one kernel family in ONE launch (blockIdx -> (problem, tile)).  The
 * reference runs the 2-4 branches of a HighResolutionModule one after the other (HRnet.py:247-252 `for i in
 * range(self.num_branches): x[i] = self.branches[i](x[i])`) and its two trunks one after the other
 * (full_net.py:252-302); they are independent until the fuse layers / the heads, so the same layer of every branch
 * of both trunks is one launch here.  Problems may differ in shape (each gets its own tile configuration inside
 * the launch) but share the family, the element type and - convolutions, weight gradients - the tap count (but for the parity
 * classes of 3x3 stride-2 data gradients, which may mix 1 / 2 / 4 taps when every layer is complete: hrp_conv_parity_fusable).
 *
 *   hrp_batch_prepare  host only (no HIP call): validates the n descriptors, chooses tiles, fills `info` and, when
 *                      table_host != NULL, the launch table (hrp_batch_table_bytes(family, n) bytes of HOST memory).
 *                      The caller copies the table to device memory it owns - once: descriptors are static - and
 *                      keeps `info`.  HRP_BATCH_WGRAD: info->ws_bytes[i] is the scratch problem i needs in ITS OWN
 *                      descriptor's `workspace` (problems of one launch run concurrently: disjoint regions); with
 *                      table_host == NULL the call only fills ws_bytes (size query).
 *   hrp_batch_launch   asynchronous on `stream`, hipGraph-capturable.
 * A group the library cannot batch (split-K linear layers, scalar-path element-wise problems, mixed tap counts ..)
 * makes prepare return HRP_ERR_ARG: launch those problems one by one. */
typedef enum {
  HRP_BATCH_CONV = 0, HRP_BATCH_WGRAD = 1, HRP_BATCH_EW_FWD = 2, HRP_BATCH_EW_BWD_REDUCE = 3, HRP_BATCH_EW_BWD_APPLY = 4,
  HRP_BATCH_WGRAD_FOLD = 5   /* descriptors: hrp_wgrad_fold_desc */
} hrp_batch_family;
#define HRP_BATCH_MAX 32
typedef struct hrp_batch_info {
  int32_t family, n, dtype;
  int32_t variant;                  /* library-internal kernel selector (tap count, input count ..) */
  int32_t grid, lds_bytes;          /* main launch */
  int32_t grid2;                    /* HRP_BATCH_WGRAD: the launch that folds the partial slabs into dW */
  int32_t grid3, lds_bytes3;        /* HRP_BATCH_WGRAD: the launch of the problems on the eight-wave program (3x3 stride-1 bf16)  */
  int32_t blk0[HRP_BATCH_MAX + 1];  /* first block of problem i (table order) in the main launch */
  int32_t blk2[HRP_BATCH_MAX + 1];  /* ... in the second launch */
  int64_t ws_bytes[HRP_BATCH_MAX];  /* HRP_BATCH_WGRAD: workspace bytes problem i (CALLER order) needs */
} hrp_batch_info;
int64_t hrp_batch_table_bytes(int family, int n);
int hrp_batch_prepare(int family, const void* descs, int n, void* table_host, hrp_batch_info* info);
int hrp_batch_launch(const void* table_dev, const hrp_batch_info* info, void* stream);
/* Parity-fused HRP_BATCH_CONV launch (hrp_conv_parity_fusable): -> the number of fused problems, n / 4, and in out[0 .. n / 4) the
 * tile configuration of each in table order, CT * 1000 + PT * 100 + 14 as hrp_conv_tile_config reports it (1214, 1114 or 2114):
 * problem i owns the blocks blk0[i] .. blk0[i + 1].  0 for a prepared conv batch that took the ordinary path.  Host only. */
int hrp_batch_conv_parity_configs(const void* table_host, const hrp_batch_info* info, int32_t* out);
/* fold descriptors of a phase-1 weight-gradient launch: of a single launch (the tiling hrp_conv2d_bwd_weight will
 * choose for d) / of the n problems of a prepared HRP_BATCH_WGRAD table (host copy), in the CALLER's order */
int hrp_wgrad_fold_desc_of(const hrp_wgrad_desc* d, hrp_wgrad_fold_desc* out);
int hrp_batch_wgrad_fold_descs(const void* table_host, const hrp_batch_info* info, hrp_wgrad_fold_desc* out);
/* What a weight-gradient launch will run (host only, no HIP call; answered by the launcher's own tiling code): of a single
 * launch (hrp_conv2d_bwd_weight on d, an invalid d returns that call's error) / of the n problems of a prepared
 * HRP_BATCH_WGRAD table (host copy), in the CALLER's order. */
typedef enum { HRP_WGRAD_FOUR_WAVE = 0, HRP_WGRAD_EIGHT_WAVE_BF16 = 1, HRP_WGRAD_EIGHT_WAVE_F32X3 = 2 } hrp_wgrad_program;
typedef struct hrp_wgrad_config {
  int32_t program;     /* hrp_wgrad_program */
  int32_t arrange;     /* four-wave: NB, 1 / 2 = 32 / 64-channel blocks.  eight-wave: PAIRS, 1 / 4 32 x 32 pairs per workgroup */
  int32_t nks, BM;     /* k-steps of 16 pixels per wave and tile (0: HRP_F32, whose k-loop is not unrolled); pixels per tile */
  int32_t TI, TH, TW;  /* images, rows and columns of a pixel tile */
  int32_t ring, xmode; /* stage buffers of the eight-wave bf16 tile ring (else 0); workgroup numbering 0 / 1 / 2 */
  int32_t G, ntiles;   /* workgroups (= partial slabs) per channel-block pair; pixel tiles they share: g walks g, g + G, .. */
  int32_t pairs;       /* channel-block pairs: the launch has G * pairs workgroups */
  int32_t use_ws;      /* 1: partial slabs in the workspace, then the fold.  0: fp32 atomics into dw */
  int32_t reserved[3];
} hrp_wgrad_config;
int hrp_wgrad_config_of(const hrp_wgrad_desc* d, hrp_wgrad_config* out);
int hrp_batch_wgrad_configs(const void* table_host, const hrp_batch_info* info, hrp_wgrad_config* out);

/* ---- segmentation-mask network of the self-supervised trainer (BASELINE config 5), the parts that are not convolutions -------
 * (reference lib/models/ctrnet/mask_inference.py:44-57 preprocess_img_tensor, keypoint_seg_resnet.py:134-149, CtRNet.py:102-111;
 *  the convolutions run through hrp_conv2d_fwd - the ASPP rates 12 / 24 / 36 as shifted one-tap problems, plan.py.)
 * hrp_pil_resize_table      host only: Pillow's bicubic resampling table of one axis (Resample.c precompute_coeffs +
 *                           normalize_coeffs_8bpc): out_size rows of HRP_PIL_KMAX + 2 ints [first input index, taps, weights in
 *                           2^-22 units]; the caller uploads it.
 * hrp_pil_resize_normalize  src: NCHW [N, 3, H, W], float32 holding 0 .. 255 (truncated to a byte like np.uint8) or (src_u8) bytes ->
 *                           Image.resize to Ho x Wo (horizontal pass, 8-bit rounding, vertical pass, 8-bit rounding: bit-exact with
 *                           Pillow) -> / 255 -> (x - mean) / std -> NHWC with dst_pitch channels per pixel, or (s2d) the 2 x 2
 *                           space-to-depth layout of the ResNet stem, [N, Ho/2, Wo/2, 12 of dst_pitch].  mean3 / std3: host arrays.
 * hrp_broadcast_hw          dst[n, p, c] = src[n, c] for p < HW (bilinear up-sampling of a 1 x 1 map: ASPP's image-pooling branch)
 * hrp_bilinear_nhwc_to_nchw F.interpolate(mode="bilinear", align_corners=False) of an NHWC tensor to H x W, written as fp32 NCHW;
 *                           act 1: sigmoid of the result */
#define HRP_PIL_KMAX 12
int hrp_pil_resize_table(int in_size, int out_size, int32_t* out);
int hrp_pil_resize_normalize(const void* src, int src_u8, int N, int H, int W, const int32_t* xtab_dev, const int32_t* ytab_dev,
                             int Ho, int Wo, void* dst, int dtype, int dst_pitch, int s2d, const float* mean3, const float* std3,
                             void* stream);
int hrp_broadcast_hw(const float* src, int src_pitch, void* dst, int dtype, int N, int HW, int C, int dst_pitch, void* stream);
int hrp_bilinear_nhwc_to_nchw(const void* src, int dtype, int N, int h, int w, int C, int pitch, float* dst, int H, int W, int act,
                              void* stream);

/* ---- fused inference BasicBlock (csrc/conv_block.h): out = relu(bn2(conv2(relu(bn1(conv1(x))))) + x) in ONE launch -------------
 * Replaces the four modules of BasicBlock.forward in eval mode (reference HRnet.py:41-57; scripts/test.py:267-273 is the
 * caller whose frames per second it serves) for the 3x3 C -> C blocks of the two high-resolution branches (C = 32 @ W = 64,
 * C = 64 @ W = 32, bf16): BatchNorm folded to per-channel scale / shift (hrp_bn_fold), the intermediate activation lives in
 * LDS only - x is read once and out written once (2 tensor passes instead of 5).
 * A workgroup (8 waves, two roles) walks a band of rows of one image in 4-row steps: waves 0-3 run conv1 + bn1 + ReLU into a
 * 16-row ring of the intermediate in LDS, waves 4-7 run conv2 + bn2 + residual (from the LDS ring of x) + ReLU two steps
 * behind; both keep their weights in registers; the rows of x arrive by direct-to-LDS DMA one step ahead.
 *   conv1: the first convolution as hrp_conv2d_fwd would take it (x, w, scale, shift, relu = 1; no bias / res / stats; y unused)
 *   conv2: the second one (w, scale, shift, relu = 1, res == conv1.x, y = the block output; x unused: never materialised)   */
#define HRP_BLOCK_MAX 2
typedef struct hrp_block_desc {
  hrp_conv_desc conv1, conv2;
} hrp_block_desc;
typedef struct hrp_block_info {
  int32_t n, grid, lds_bytes, reserved;
  int32_t first_wg[HRP_BLOCK_MAX];     /* first workgroup of problem i                                                   */
  int32_t bands[HRP_BLOCK_MAX];        /* row bands per image of problem i (one workgroup each)                           */
} hrp_block_info;
/* 32 / 64 when the fused kernel takes the block, else 0 (host only) */
int hrp_block_channels(const hrp_block_desc* d);
/* hrp_block_prepare  host only: validates the n <= HRP_BLOCK_MAX problems (two: a 32-channel and a 64-channel block, in this
 *                    order - the two high-resolution branches of one trunk), chooses the bands and writes the launch table
 *                    (hrp_block_table_bytes() bytes of HOST memory the caller keeps: passed to the kernel by value).
 * hrp_block_launch   asynchronous on `stream`, hipGraph-capturable. */
int64_t hrp_block_table_bytes(void);
int hrp_block_prepare(const hrp_block_desc* descs, int n, void* table, hrp_block_info* info);
int hrp_block_launch(const void* table, const hrp_block_info* info, void* stream);

int hrp_bn_running_update(const hrp_bn_entry* table_dev, int count, void* stream);
int hrp_bn_fold(const hrp_bn_entry* table_dev, int count, void* stream);
int hrp_bn_param_grad(const hrp_bn_entry* table_dev, int count, void* stream);

int hrp_avgpool_fwd(const void* x, int dtype, int N, int HW, int C, int pitch, float* out, int out_pitch, void* stream);
int hrp_avgpool_bwd(const float* dout, int dout_pitch, void* dx, int dtype, int N, int HW, int C, int pitch, int accumulate, void* stream);

/* logits [B, H, W, J*D] (channel = j*D + d) -> uvd [B, J, 3] in [-0.5, 0.5); ms = saved (max, sum) [B, J, 2] */
int hrp_softargmax3d_fwd(const void* logits, int dtype, int B, int J, int D, int H, int W, int pitch,
                         int root, int fix_root, float* uvd, float* ms, void* stream);
int hrp_softargmax3d_bwd(const void* logits, int dtype, int B, int J, int D, int H, int W, int pitch,
                         int root, int fix_root, const float* uvd, const float* ms, const float* duvd,
                         void* dlogits, int dpitch, void* stream);

/* gamma [B], k_value [B], uvd [B,J,3], K [B,9] -> depth [B] (m), xyz_int [B,J,3], root_uv [B,2], trans [B,3] */
int hrp_pose_geometry_fwd(const float* gamma, const float* k_value, const float* uvd, const float* K,
                          int B, int J, int root, float image_size, float depth_factor,
                          float* depth, float* xyz, float* root_uv, float* trans, void* stream);
int hrp_pose_geometry_bwd(const float* gamma, const float* k_value, const float* uvd, const float* K,
                          int B, int J, int root, float image_size, float depth_factor,
                          const float* d_depth, const float* d_xyz, const float* d_root_uv, const float* d_trans,
                          float* d_gamma, float* d_uvd, void* stream);

/* HeatmapIntegralJoint (reference lib/utils/integral.py:206-232): per (sample, channel j < J) softmax over the HW
 * positions of logits [B, HW, pitch], coord[b, j] = E[flat index] / HW in [0, 1); ms [B, J, 2] keeps (max, sum) for the
 * backward pass, which overwrites dlogits[b, p, j] = softmax * (p / HW - coord) * dcoord. */
int hrp_softargmax_flat_fwd(const void* logits, int dtype, int B, int J, int HW, int pitch, float* coord, float* ms, void* stream);
int hrp_softargmax_flat_bwd(const void* logits, int dtype, int B, int J, int HW, int pitch, const float* coord, const float* ms,
                            const float* dcoord, void* dlogits, int dpitch, void* stream);

/* out[n] = rotmat_to_rot6d(rot6d_to_rotmat(a[n]) @ rot6d_to_rotmat(b[n]))  (dense fp32 [N, 6]): the update of the
 * rot_iterative_matmul regressor (reference full_net.py:346-362, lib/utils/geometries.py:100-131).  Backward: exact, by
 * forward-mode differentiation of the same code; da / db may be NULL; acc_*: add to the existing gradient. */
int hrp_rot6d_compose_fwd(const float* a, const float* b, float* out, int N, void* stream);
int hrp_rot6d_compose_bwd(const float* a, const float* b, const float* dout, float* da, float* db, int N, int acc_a, int acc_b,
                          void* stream);

/* q [B,dof], rot6d [B,6], trans [B,3], K [B,9] (may be NULL -> no uv) -> xyz [B,nkp,3], uv [B,nkp,2].
 * root > 0 re-roots the chain at keypoint `root` (urdf_robot.py:194-198). One wavefront per sample. */
int hrp_fk_project_fwd(const hrp_fk_chain* chain_dev, const float* q, const float* rot6d, const float* trans,
                       const float* K, int B, int root, float* xyz, float* uv, float* root_rot6d, void* stream);
/* Soft-silhouette rasteriser of the render-and-compare path (reference lib/utils/mesh_renderer.py:78-109: pytorch3d's MeshRasterizer +
 * SoftSilhouetteShader; the trainer uses channel 3 of the rendering, urdf_robot.py:257).  PARITY UNPINNED - pytorch3d is not in the
 * reference tree or the build container; csrc/silhouette.hip restates its published algorithm and lists what is not modelled.
 *   alpha[b, y, x] = 1 - prod over faces kept at the pixel of (1 - sigmoid(-s / sigma)),  s = signed squared NDC distance to the
 *   face's nearest edge (negative inside), kept = inside or s < blur_radius.
 * uv / xyz: posed vertices in pixels and in the camera frame (hrp_mesh_pose with K).  logp: [B, H, W] 64-bit workspace that the
 * backward reads again.  hrp_silhouette_bwd: d_uv[B, V, 2] = gradient of sum(d_alpha * alpha) (zeroed by the call). */
typedef struct hrp_silhouette_desc {
  const float* uv;        /* [B, V, 2] */
  const float* xyz;       /* [B, V, 3] (z: faces behind the camera are skipped) */
  const int32_t* faces;   /* [F, 3] vertex indices */
  int32_t B, V, F, H, W;
  float sigma, blur_radius;
  float* alpha;           /* [B, H, W] */
  int64_t* logp;          /* [B, H, W] */
  int32_t* count;         /* optional [B, H, W] (zeroed by the call): faces kept at the pixel.  pytorch3d keeps the faces_per_pixel =
                             100 NEAREST faces (mesh_renderer.py:99); every kept face enters the product here, so the result is
                             pytorch3d's exactly where count <= 100 - the caller can check that instead of assuming it */
} hrp_silhouette_desc;
int hrp_silhouette_fwd(const hrp_silhouette_desc* d, void* stream);
int hrp_silhouette_bwd(const hrp_silhouette_desc* d, const float* d_alpha, float* d_uv, void* stream);

/* Mesh posing of the render-and-compare path (reference lib/utils/mesh_renderer.py:126-173 get_robot_mesh - every link's
 * vertices moved by the link's pose, on the CPU, per sample - and lib/utils/urdf_robot.py:242-275: camera pose of the robot
 * base, optionally re-rooted at a key-point link, flipped when the translation has negative depth):
 *   xyz[b, v] = M_b * (T_link(v)(q_b) * verts[v]),   M_b = B2C_b (root_kp < 0) or B2C_b * T_root(q_b)^-1;  M_b -> -M_b if M_b.t.z < 0
 * `chain_dev` is an hrp_fk_chain whose key-point table lists the MESH links (offsets unused): vert_link[v] and root_kp index it.
 * K (optional, [B, 9]): uv[b, v] = pinhole projection of xyz (the renderer's PerspectiveCameras with focal (-fx, -fy)).
 * Forward only: the trainer detaches the joint angles on this path and the silhouette's pose gradient comes from the rasteriser. */
int hrp_mesh_pose(const hrp_fk_chain* chain_dev, const float* q, const float* rot6d, const float* trans, int B, int root_kp,
                  const float* verts, const uint8_t* vert_link, int V, const float* K, float* xyz, float* uv, void* stream);
/* gradient of sum(d_xyz * xyz) with respect to rot6d [B, 6] and trans [B, 3] (the joint angles are detached on this path,
 * urdf_robot.py:267; the mirror of a sample behind the camera is a constant sign) */
int hrp_mesh_pose_bwd(const hrp_fk_chain* chain_dev, const float* q, const float* rot6d, const float* trans, int B, int root_kp,
                      const float* verts, const uint8_t* vert_link, int V, const float* d_xyz, float* d_rot6d, float* d_trans, void* stream);
int hrp_fk_project_bwd(const hrp_fk_chain* chain_dev, const float* q, const float* rot6d, const float* trans,
                       const float* K, int B, int root, const float* d_xyz, const float* d_uv,
                       float* d_q, float* d_rot6d, float* d_trans, void* stream);
/* The same pair for either rotation representation of the network (reference urdf_robot.py:86-92, 118-138; full_net.py:186-189):
 * rot_dim 6 = two rows of the rotation matrix (Zhou et al.), 4 = quaternion (w, x, y, z), normalised by (norm + 1e-9) as
 * geometries.py:21-41; root_rot comes back in the same representation (quaternion: geometries.py:63-82). */
int hrp_fk_project_rot_fwd(const hrp_fk_chain* chain_dev, const float* q, const float* rot, int rot_dim, const float* trans,
                           const float* K, int B, int root, float* xyz, float* uv, float* root_rot, void* stream);
int hrp_fk_project_rot_bwd(const hrp_fk_chain* chain_dev, const float* q, const float* rot, int rot_dim, const float* trans,
                           const float* K, int B, int root, const float* d_xyz, const float* d_uv,
                           float* d_q, float* d_rot, float* d_trans, void* stream);

/* small fp32 helpers used by the regression heads */
int hrp_copy_cols(const float* src, int src_pitch, float* dst, int dst_pitch, int rows, int cols, int accumulate, void* stream);
/* n <= HRP_COPY_MAX such copies in ONE launch (the [B, C] vectors at the plan boundary: the external inputs of
 * RootNetwithRegInt.forward - k_value, K, init_pose, init_rot, full_net.py:236-248 -, its eight outputs :392-395 and their gradients
 * coming back from the loss); src == NULL: the block is zero-filled (an output the loss does not use). */
#define HRP_COPY_MAX 16
typedef struct hrp_copy_desc {
  const float* src;
  float* dst;
  int src_pitch, dst_pitch, rows, cols;
  int accumulate, reserved;
} hrp_copy_desc;
int hrp_copy_cols_batch(const hrp_copy_desc* descs, int n, void* stream);
int hrp_scale_rows(float* x, int pitch, int rows, int cols, const float* row_scale, float s, void* stream);
/* y (+)= x * m element-wise on [rows, cols] fp32 (dropout masks of the regression heads, full_net.py:98-99) */
int hrp_mul_f32(const float* x, int x_pitch, const float* m, int m_pitch, float* y, int y_pitch, int rows, int cols,
                int accumulate, void* stream);
/* nn.Linear of the regression heads (lib/models/full_net.py:95-100, 129-134 fc_pose_1/2, decpose, fc_rot_1/2, decrot,
 * called 4 x 6 times per forward by the iterative regressors :318-331, 365-378) and its autograd, fp32, M = batch rows.
 * w is the PyTorch-shaped parameter [N][K] itself (no packing), bias [N] / res [M, res_pitch] optional.
 *   fwd:        y[M,N]  = x[M,K] w^T + bias + res
 *   bwd_data:   dx[M,K] (+)= dy[M,N] w
 *   bwd_weight: dw[N,K] (+)= dy^T x ;  dbias[N] (+)= column sums of dy (dbias may be NULL)
 * fwd / bwd_data split their reduction over workgroups.  workspace (hrp_linear_workspace_bytes(M, K, N) bytes, 16-byte aligned,
 * no initialisation, used by one launch at a time): the partial sums are parked there and a second small launch adds them in
 * a fixed order - the result is bit-reproducible.  workspace NULL: fp32 atomics into the (zeroed) output: the last bits
 * depend on the arrival order and vary from run to run. */
int64_t hrp_linear_workspace_bytes(int M, int K, int N);
int hrp_linear_fwd(const float* x, int x_pitch, const float* w, const float* bias, const float* res, int res_pitch,
                   float* y, int y_pitch, int M, int K, int N, void* workspace, int64_t workspace_bytes, void* stream);
int hrp_linear_bwd_data(const float* dy, int dy_pitch, const float* w, float* dx, int dx_pitch, int M, int K, int N,
                        int accumulate, void* workspace, int64_t workspace_bytes, void* stream);
int hrp_linear_bwd_weight(const float* x, int x_pitch, const float* dy, int dy_pitch, float* dw, float* dbias, int M, int K,
                          int N, int accumulate, void* stream);

/* The training loss of configs/panda/full.yaml (lib/core/function.py:191-322, projections of :119-122) and its gradient
 * with respect to the model's predictions in one launch.  All tensors dense fp32.  weights: pose, rot, uv, depth, trans,
 * kp2d, kp3d, kp2d_int, kp3d_int, align_3d (the *_loss_weight keys of the yaml, :57-66).  out[0..9]: loss_joint, loss_rot,
 * loss_uv, loss_depth, loss_trans, loss_error3d, loss_error2d, loss_error2d_int, loss_error3d_int, loss_error3d_align (the
 * names of function.py:313-319); out[10]: the weighted total.  d_*: gradient of out[10] (all seven, or all NULL). */
typedef struct hrp_pose_loss_desc {
  const float *pose, *rot, *trans, *root_uv, *depth, *xyz_int, *xyz_fk;   /* [B,P] [B,rot_dim] [B,3] [B,2] [B,1] [B,J,3] [B,J,3] */
  const float *gt_pose, *gt_root_rot, *gt_root_trans, *gt_root_uv;       /* [B,P] [B,6] [B,3] [B,2] */
  const float *gt_kp3d, *gt_kp2d, *mask, *K;                             /* [B,J,3] [B,J,2] [B,J] [B,9] */
  float *d_pose, *d_rot, *d_trans, *d_root_uv, *d_depth, *d_xyz_int, *d_xyz_fk;
  float* out;                                                            /* [11] */
  float weights[10];
  int32_t B, P, J, root;
  float image_size;
  int32_t rot_dim;     /* width of rot / gt_root_rot / d_rot: 0 or 6 = two rows of the rotation matrix, 4 = quaternion (w x y z) */
} hrp_pose_loss_desc;
int hrp_pose_loss(const hrp_pose_loss_desc* d, void* stream);
/* The DepthNet trainer's loss (scripts/train_depthnet.py:231-250, nn.L1Loss on model(images, k) / 1000 against the root depth):
 * *loss = mean |pred * scale - gt| over n dense fp32 values; d_pred (optional) = sign(pred * scale - gt) * scale / n. */
int hrp_l1_loss(const float* pred, const float* gt, float scale, int n, float* loss, float* d_pred, void* stream);

/* Mask losses of the self-supervised (render-and-compare) trainer, reference scripts/train_sim2real.py:435-468 (BASELINE
 * config 5), with their analytic gradient, in one call (three small launches, fixed summation order: reproducible):
 *   mask   mask_loss 0: MSELoss(mean)(rendered, seg) | 1: BCELoss (log clamped at -100 as torch) | 2: 0.001 * MSELoss(sum)
 *   iou    1 - mean_b( I_b / (S_b + R_b - I_b) ),  I = sum seg * rendered, S = sum seg, R = sum rendered per image
 *   scale  sum_b |log((S_b - I_b) / (R_b - I_b))| * f_b / (sum_b f_b + 1e-9),  f_b = ratio > 5 or ratio < 0.2 (no gradient)
 *   align  mean over (b, k) of || kp3d - kp3d_int ||_2
 *   loss = w_mask * mask + w_iou * iou + w_scale * scale + w_align * align        (terms[0..4] = loss, mask, iou, scale, align)
 * Gradients (optional pointers) are those of `loss`; a term whose weight is 0 contributes none (torch would propagate 0 * inf
 * of a degenerate ratio); || . || = 0 has gradient 0 as in torch.  `seg` carries no gradient (the trainer detaches it). */
typedef struct hrp_sim2real_loss_desc {
  const float* rendered;   /* [B, HW] soft silhouettes in [0, 1]                                  */
  const float* seg;        /* [B, HW] segmentation probabilities                                   */
  const float* kp3d;       /* [B, K, 3] key-points of the kinematic chain (pred_keypoints3d)       */
  const float* kp3d_int;   /* [B, K, 3] key-points of the integral head (pred_keypoints3d_int)     */
  int32_t B, HW, K, mask_loss;
  float w_mask, w_iou, w_scale, w_align;
  float* terms;            /* [5]                                                                  */
  float* d_rendered;       /* optional [B, HW]                                                     */
  float* d_kp3d;           /* optional [B, K, 3]                                                   */
  float* d_kp3d_int;       /* optional [B, K, 3]                                                   */
  float* workspace;        /* [8 * B] floats                                                       */
} hrp_sim2real_loss_desc;
int hrp_sim2real_loss(const hrp_sim2real_loss_desc* d, void* stream);

/* nn.Dropout of the regression heads (lib/models/full_net.py:98-99, 132-133; p = args.p_dropout, lib/config.py default
 * 0.5), inverted scaling: mask[r,c] = (u < keep) / keep with u from Philox4x32-10 keyed by state_dev[0] (seed) at counter
 * (element / 4, salt, state_dev[1] = step); y = x * mask.  `mask` ([rows, cols] dense fp32) is what the backward multiplies
 * by (hrp_mul_f32).  hrp_rng_advance increments state_dev[1]: one launch per forward, so a captured HIP graph draws a new
 * mask at every replay, on the stream the consumer runs on. */
int hrp_rng_advance(uint64_t* state_dev, void* stream);
int hrp_dropout_f32(const float* x, int x_pitch, float* y, int y_pitch, float* mask, int rows, int cols, float keep,
                    const uint64_t* state_dev, uint32_t salt, void* stream);
/* All dropout masks of one forward in ONE launch: masks[i] = (u_i < keep) / keep, n dense fp32 values (16-byte aligned), the
 * generator and counter layout of hrp_dropout_f32 (counter = (i / 4, salt, step)).  The fused regressor chain below multiplies by
 * slices of this buffer in its staging path and its epilogue (full_net.py:98-99, 132-133: drop1 / drop2 inside the loop). */
int hrp_dropout_masks(float* masks, int64_t n, float keep, const uint64_t* state_dev, uint32_t salt, void* stream);

/* The iterative regressors of the full network (lib/models/full_net.py:318-331 joint angles, :365-378 rotation):
 *     p_{i+1} = p_i + dec(drop(fc2(drop(fc1(cat(xf, p_i))))))      n_iter times, no non-linearity between the three nn.Linear
 * as a chain of launches of ONE kernel, several problems (the two heads) per launch.  One step of one problem computes, all fp32,
 * every sum in a fixed order (bit-reproducible; exact fp32 products on v_mfma_f32_16x16x4_f32):
 *   1. state    u[m][p]  = u_prev[m][p] + u_bias[p] + sum_{k < z_len} z[m][k] * zw[k * zw_sk + p * zw_sp]
 *               (z NULL: no sum; P == 0: no state).  Every workgroup computes the u of its rows; u_out (optional) receives it.
 *   2. operand  a'[m][k] = a_mask[m][k] * (a[m][k] + sum_p u[m][p] * v[k * v_sk + p * v_sp])
 *               (a NULL: 0; a_mask NULL: 1; v NULL: no update).  a_out (dense [M][K]; required when there is a mask or an update: the
 *               product reads a' from it) receives a'.
 *   3. product  val[m][n] = out_mask[m][n] * (bias[n] + sum_k a'[m][k] * w[n * w_sn + k * w_sk] + sum_k a2[m][k] * w2[n * w_sn + k * w2_sk])
 *               out[m][n] (+)= val;  out_sum[m][n] (+)= val (optional).  One of w_sn / w_sk must be 1.  N == 0: step 1 only.
 * How the plan maps the reference loop onto it (hrpe_amd/plan.py PlanBuilder.regressors; F = feature width, H = 1024):
 *   hoist      a = xf, w = fc1.weight[:, :F] (w_sn = F + P), bias = fc1.bias -> A                 (full_net.py:319-320 recomputes this
 *              product in every iteration)
 *   forward i  u_prev = p_{i-1}, u_bias = dec.bias, z = d2_{i-1}, zw = dec.weight (zw_sk = 1, zw_sp = H) -> p_i;
 *              a = A, v = fc1.weight[:, F:], a_mask = drop1 mask -> d1_i;  w = fc2.weight, bias = fc2.bias, out_mask = drop2 mask -> d2_i
 *   backward i u_prev = g_{i+2}, z = gh1_{i+1}, zw = fc1.weight[:, F:] -> g_{i+1};  a = NULL, v = dec.weight^T, a_mask = drop2 mask -> gh2_i;
 *              w = fc2.weight^T (w_sn = 1, w_sk = H), out_mask = drop1 mask -> gh1_i, out_sum = gA
 *   d xf       a = gA(pose), w = fc_pose_1.weight^T, a2 = gA(rot), w2 = fc_rot_1.weight^T (w_sn = 1, w_sk = F + P)
 * Two kernels per call: steps 1 + 2 with one workgroup per row, step 3 with a workgroup per 32 rows x 16 columns.
 * Requirements: K % 4 == 0, a_out 16-byte aligned, P <= HRP_REG_MAX_P. */
#define HRP_REG_MAX_P 16
#define HRP_REG_MAX_PROBLEMS 4
typedef struct hrp_regressor_step_desc {
  int32_t M, P, K, N;             /* rows; state width; reduction length of the product; output columns                            */
  const float* u_prev;            /* [M][P] dense                                                                                   */
  const float* u_bias;            /* [P] or NULL                                                                                    */
  const float* z;                 /* [M][z_pitch] or NULL                                                                           */
  const float* zw;
  int32_t z_len, z_pitch, zw_sk, zw_sp;
  float* u_out;                   /* [M][P] dense or NULL                                                                           */
  const float* a;                 /* [M][a_pitch] or NULL                                                                           */
  const float* a_mask;            /* [M][K] dense or NULL                                                                           */
  const float* v;
  int32_t a_pitch, v_sk, v_sp, a2_pitch;
  float* a_out;                   /* [M][K] dense or NULL                                                                           */
  const float* w;
  const float* bias;              /* [N] or NULL                                                                                    */
  const float* out_mask;          /* [M][N] dense or NULL                                                                           */
  const float* a2;                /* second source [M][a2_pitch] or NULL (no mask, no update)                                       */
  const float* w2;
  int64_t w_sn, w_sk;
  int32_t out_pitch, out_accumulate, out_sum_accumulate;
  int32_t w2_sk;                  /* k stride of w2 (0: w_sk)                                                                      */
  float* out;                     /* [M][out_pitch]                                                                                 */
  float* out_sum;                 /* [M][N] dense or NULL                                                                           */
} hrp_regressor_step_desc;
int hrp_regressor_step(const hrp_regressor_step_desc* descs, int n, void* stream);

/* Weight / bias gradients of several nn.Linear layers in one launch (the end of the regressor chain: the n_iter iterations of a
 * layer are ONE product over n_iter * M stacked rows):  dw[n * dw_ld + k] (+)= sum_m dy[m][n] * x[m][k];  dbias[n] (+)= sum_m dy[m][n]
 * (dbias optional).  dw_ld: row length of the parameter dw points into (a column block of fc1.weight: dw_ld = F + P). */
#define HRP_LIN_WGRAD_MAX 8
typedef struct hrp_linear_wgrad_desc {
  const float* x;                 /* [M][x_pitch]  */
  const float* dy;                /* [M][dy_pitch] */
  float* dw;
  float* dbias;
  int32_t x_pitch, dy_pitch, dw_ld, M, K, N, accumulate, reserved;
} hrp_linear_wgrad_desc;
int hrp_linear_wgrad_batch(const hrp_linear_wgrad_desc* descs, int n, void* stream);

/* point_projection_from_3d_tensor (lib/utils/transforms.py:17-21): K [B,9], pts [B,P,3] -> uv [B,P,2] */
int hrp_project_fwd(const float* K, const float* pts, int B, int P, float* uv, void* stream);
int hrp_project_bwd(const float* K, const float* pts, const float* duv, int B, int P, float* dpts, void* stream);

/* Perspective-n-point, one 64-lane workgroup per sample (4 <= n <= 64 points), fp64 inside (csrc/pnp.hip).
 * hrp_pnp_solve replaces the per-sample host loop of cv2.solvePnP calls in BPnP.forward (lib/utils/BPnP.py:24-47, 129-151):
 *   EPnP (control points from the PCA of the 3-D points, null space of M^T M by Jacobi, N = 1, 2, 3 beta solutions refined by
 *   Gauss-Newton, the lowest mean reprojection error kept) unless ini_pose [B,6] is given (:142-145), then Levenberg-Marquardt on
 *   (angle-axis, t) minimising sum_i |x_i - pi(K, R X_i + t)|^2 with a fixed iteration cap.
 *   pts2d [B,n,2]; pts3d [B,n,3] (pts3d_stride = 3n) or shared [n,3] (0); K [B,3,3] (K_stride = 9) or shared [3,3] (0).
 *   P6d [B,6] = angle-axis (|w| <= pi) then translation.  status [B,2] = (converged, iterations) and rms [B] (reprojection error
 *   in px at the solution) are optional (NULL).
 * hrp_pnp_bwd replaces BPnP.backward (:50-111), BPnP_m3d.backward (:154-236) and, with fast = 1, BPnP_fast.backward (:280-341): the
 *   reference's formula grad = -g^T J_fy^-1 J_f(x, z, K) with f_j = sum_i coef_ij . (x_i S_i - (K [R|t] z_i)_{0:2}), coef = -2 dpi/dy
 *   (get_coefs :344-357, whose create_graph=True derivatives are kept unless fast).  grad_x [B,n,2]; grad_z [B,n,3] and grad_K [B,9]
 *   per sample; grad_z_sum [n,3] / grad_K_sum [9] (optional) their sums over the batch in sample order (shared pts3d / K).
 *   A singular J_fy gives NaN gradients for that sample and status[b] = 1 (optional [B]); the reference raises in torch.inverse. */
int hrp_pnp_solve(const float* pts2d, const float* pts3d, int pts3d_stride, const float* K, int K_stride, const float* ini_pose,
                  int B, int n, float* P6d, int* status, float* rms, void* stream);
int hrp_pnp_bwd(const float* pts2d, const float* pts3d, int pts3d_stride, const float* K, int K_stride, const float* P6d,
                const float* grad_out, int B, int n, int fast, float* grad_x, float* grad_z, float* grad_K, float* grad_z_sum,
                float* grad_K_sum, int* status, void* stream);

/* Robust PnP: what the reference's BPnP_fast gets from cv2.solvePnPRansac(reprojectionError, confidence) followed by solvePnP
 * (lib/utils/BPnP.py:267-271), as one launch, one 64-lane workgroup per sample, fp64 inside, no global scratch (csrc/pnp.hip, the
 * per-hypothesis core in csrc/pnp_minimal.h).  Unlike cv2, the minimal sets are enumerated, not drawn - all C(m, 3) triples of the m
 * usable points in lexicographic order, or, where C(m, 3) > max_hypotheses, max_hypotheses triples from a counter-based hash of
 * (seed, index) - and each is solved by P3P (Grunert), not by five-point EPnP: parity with cv2 is by objective, not by bits, and two
 * calls return the same bytes.
 *   1. lane = hypothesis, in passes of 64: P3P on the triple, every root scored against the usable points: a point is an inlier if its
 *      camera depth is positive and its reprojection error is finite and < reproj_error px.  Score = (inliers, -sum of their squared
 *      errors), ties to the lower hypothesis, then the lower root; a butterfly picks the winner.
 *   2. lane = point: hrp_pnp_solve's LM on the winner's inliers from the winner's pose, re-score, refit while the set changes (three
 *      refits at most); refine_all = 1: one more LM over all usable points from there (BPnP_fast's recipe).
 *   valid [B,n] bytes (optional): 0 marks a point unusable; a point with a non-finite coordinate is unusable too.  Unusable points
 *   are in no triple and never inliers.  Other arguments as hrp_pnp_solve; 4 <= min_inliers <= 64, 1 <= max_hypotheses <= 2^20.
 *   P6d [B,6]; inliers [B,n] bytes: the points within reproj_error of P6d; rms [B] over the points of the last fit;
 *   status [B,4] = (HRP_PNP_* flags, LM trials, inlier count, hypotheses scored).
 * If the best consensus is below min_inliers, HRP_PNP_NO_CONSENSUS is set and P6d, rms are what hrp_pnp_solve gives for the usable
 * points (EPnP + LM; the same bits where all points are usable).  HRP_PNP_FEW_POINTS: fewer than 4 usable points; no hypothesis is
 * formed, both flags are set and P6d is not meaningful.  HRP_PNP_CONVERGED: the last LM ended before its trial cap.
 * hrp_pnp_bwd_masked is hrp_pnp_bwd with mask [B,n] bytes: a point whose byte is 0 contributes nothing to J_fy, J_fz, J_fK and gets
 * zero grad_x / grad_z (the implicit-function gradient at the optimum over the inliers). */
enum { HRP_PNP_NO_CONSENSUS = 1, HRP_PNP_CONVERGED = 2, HRP_PNP_FEW_POINTS = 4 };
int hrp_pnp_solve_robust(const float* pts2d, const float* pts3d, int pts3d_stride, const float* K, int K_stride,
                         const unsigned char* valid, int B, int n, double reproj_error, int min_inliers, int max_hypotheses,
                         unsigned seed, int refine_all, float* P6d, unsigned char* inliers, int* status, float* rms, void* stream);
int hrp_pnp_bwd_masked(const float* pts2d, const float* pts3d, int pts3d_stride, const float* K, int K_stride, const float* P6d,
                       const float* grad_out, const unsigned char* mask, int B, int n, int fast, float* grad_x, float* grad_z,
                       float* grad_K, float* grad_z_sum, float* grad_K_sum, int* status, void* stream);

/* Pooled robust PnP: ONE pose from all the correspondences of a sequence (eye-to-hand calibration of a fixed camera, the multi-frame
 * PnP of DREAM).  It replaces scripts/test.py:121-122 and CtRNet.py:68-89 applied per frame - F poses of k points each, nothing
 * combining them - by one solve over the F x k points.  hrp_pnp_solve_robust's semantics with the point count untied from the
 * wavefront (4 <= n <= HRP_PNP_POOLED_MAX_N), fp64 inside, three launches ordered by the kernel boundary alone (csrc/pnp_pooled.hip):
 *   1. compact: the usable points (flag set, five finite coordinates, a finite bearing) in index order, m of them;
 *      H = min(C(m, 3), max_hypotheses) hypotheses, 0 for m < 4: every triple of ranks in lexicographic order where C(m, 3) <=
 *      max_hypotheses, otherwise the hash-drawn triples of (seed, h), as hrp_pnp_solve_robust.
 *   2. score: lane = hypothesis, grid (ceil(H / 64), B); P3P on the triple, every root scored against the m points (staged through
 *      LDS in tiles); one record (count, sum of squares, root, R, t) per hypothesis into the workspace.
 *   3. fit: one 256-thread workgroup per problem.  The winner by (count, -sum of squares, lower hypothesis, lower root), then
 *      hrp_pnp_solve's LM on the winner's inliers from the winner's pose, re-score, refit while the inlier set changes
 *      (HRP_PNP_POOLED_REFITS fits at most); refine_all = 1: one more LM over all usable points.  Sums run over a thread's points in
 *      index order, then a butterfly per wave, then the waves in order: two calls return the same bytes.
 *   pts2d [B,n,2], pts3d [B,n,3], K and K_stride, valid, reproj_error, seed as hrp_pnp_solve_robust; 4 <= min_inliers <= n,
 *   1 <= max_hypotheses <= 2^20.  workspace: hrp_pnp_pooled_workspace_bytes(B, n, max_hypotheses) bytes, 16-byte aligned, no
 *   initialisation, the only scratch memory used.
 *   P6d [B,6]; inliers [B,n] bytes: the points within reproj_error of P6d; rms [B] over the points of the last fit; status [B,4] =
 *   (HRP_PNP_* flags, LM trials, inlier count, H).  cov [B,36] (optional): s^2 (J^T J)^-1 in (w, t) at P6d over the nfit points of
 *   the last fit, s^2 = cost / (2 nfit - 6); all zeros with nfit <= 3 or a singular J^T J.
 * Below min_inliers HRP_PNP_NO_CONSENSUS is set and P6d is the LM over all usable points from the winner's pose (no EPnP here: a
 * sequence without consensus is a failed calibration).  Fewer than 4 usable points: both flags, no fit, zero P6d, rms and cov. */
enum { HRP_PNP_POOLED_MAX_N = 16384, HRP_PNP_POOLED_REFITS = 8 };
int hrp_pnp_pooled_workspace_bytes(int B, int n, int max_hypotheses, size_t* bytes);
int hrp_pnp_solve_pooled(const float* pts2d, const float* pts3d, const float* K, int K_stride, const unsigned char* valid, int B, int n,
                         double reproj_error, int min_inliers, int max_hypotheses, unsigned seed, int refine_all, void* workspace,
                         size_t workspace_bytes, float* P6d, unsigned char* inliers, int* status, float* rms, float* cov, void* stream);

/* DREAM dataset pixel work (csrc/dream.hip): the host (lib/dataset/dream.py) draws every random number and computes the geometry
 * of each sample into one hrp_dream_sample; these two launches do the per-pixel steps of a batch, bit-exact with the reference's
 * numpy / Pillow / torch CPU arithmetic.  Coordinates are in the sample's WORKING frame: the decoded frame or, under
 * process_truncation (dream.py:226-227, roboutils.py:163-195), its zero-padded copy of work_h x work_w with the decoded frame at
 * (pad_y, pad_x).
 * hrp_dream_augment replaces dream.py:229-255 up to the pointwise enhancements.  Per working-frame pixel, in the reference's
 *   order: jitter (flags & HRP_DREAM_JITTER; uint8 * fp64 jitter[c], clipped to [0, 255], truncated; :229-237), the occlusion fill
 *   (HRP_DREAM_OCCLUSION; the rectangle occ_* takes its bytes, HWC, from noise + noise_off; :239-245), ImageEnhance.Sharpness
 *   (HRP_DREAM_SHARPNESS; Image.blend(SMOOTH(im), im, enh[0]), SMOOTH rounding (8 neighbours + 5 centre + 6) / 13 with the
 *   border pixels kept).  frames: [B, H, W, 3] uint8; scratch: the working frame of sample b, [work_h, work_w, 3] uint8 at
 *   scratch + scratch_off; lsum: [B, HRP_DREAM_BANDS] uint64, the exact sums of convert("L") ((19595 r + 38470 g + 7471 b +
 *   2^15) >> 16) of the written frame over HRP_DREAM_BANDS bands of rows (ImageEnhance.Contrast's mean, reduced in band order by
 *   the crop launch).  max_h / max_w bound every work_h / work_w (the grid does not depend on the table: graph-capturable).
 * hrp_dream_crop_resize replaces resize_image (roboutils.py:128-156) + CropResizeToAspectAugmentation (augmentations.py:170-242):
 *   output pixel -> zero-padded side x side canvas (the crop box crop_* of the working frame at (off_x, off_y)) -> torch's CPU
 *   bilinear (align_corners=False, scale = (float)side / out) over the 4 canvas pixels, each taken through the pointwise tail
 *   Contrast (enh[1], mean int(sum / pixels + 0.5)), Brightness (enh[2]), Color (enh[3]) with Pillow's uint8 truncation between
 *   them; v / 255 interpolated, (x * 255) truncated.  side == out size: the canvas itself (augmentations.py:176-178).
 *   out0 [B, 3, h0, w0] and optionally out1 [B, 3, h1, w1] uint8 (the rootnet and other views when their sizes differ). */
#define HRP_DREAM_BANDS 32
enum {
  HRP_DREAM_JITTER = 1, HRP_DREAM_OCCLUSION = 2, HRP_DREAM_SHARPNESS = 4, HRP_DREAM_CONTRAST = 8, HRP_DREAM_BRIGHTNESS = 16,
  HRP_DREAM_COLOR = 32
};
typedef struct {
  double jitter[3];   /* per-channel colour-jitter factors (used when flags & HRP_DREAM_JITTER) */
  double enh[4];      /* Sharpness, Contrast, Brightness, Color factors as drawn (Image.blend takes them as float) */
  int32_t flags;      /* HRP_DREAM_* of the stages whose draw fired */
  int32_t occ_x, occ_y, occ_w, occ_h;                 /* occlusion rectangle in the working frame */
  int32_t pad_x, pad_y, work_w, work_h;               /* decoded frame's offset in the working frame; working-frame size */
  int32_t crop_x0, crop_y0, crop_x1, crop_y1;         /* resize_image's bbox (wmin, hmin, wmax, hmax) */
  int32_t off_x, off_y, side;                         /* its offsets in the square canvas, and the canvas side S */
  int32_t reserved;
  int64_t noise_off;                                  /* occ_h * occ_w * 3 noise bytes (HWC) */
  int64_t scratch_off;                                /* byte offset of the working frame in scratch */
} hrp_dream_sample;
int hrp_dream_augment(const uint8_t* frames, int B, int H, int W, const hrp_dream_sample* table_dev, const uint8_t* noise,
                      int64_t noise_bytes, int max_h, int max_w, uint8_t* scratch, int64_t scratch_bytes, uint64_t* lsum, void* stream);
int hrp_dream_crop_resize(const uint8_t* scratch, int64_t scratch_bytes, const hrp_dream_sample* table_dev, const uint64_t* lsum, int B,
                          int max_h, int max_w, uint8_t* out0, int h0, int w0, uint8_t* out1, int h1, int w1, void* stream);

/* Validation metrics of one batch in ONE launch (csrc/eval.hip): what farward_loss(train=False) derives from the predictions
 * (lib/core/function.py:137-179) - compute_metrics_batch in both call forms (lib/utils/metrics.py:36-113) and the mean geodesic
 * rotation distance - written straight into accumulators that live on the device for the whole epoch, so that nothing has to
 * reach the host before the summary.  All tensors dense fp32.  One workgroup; every sum over key-points and over samples runs in
 * index order (no atomics): bit-reproducible.  NaN where the reference's 0 / 0 gives NaN (an image, or a key-point over the
 * batch, with nothing in frame).
 * Per-image outputs are arrays of `capacity` floats, written at [offset, offset + B); per-batch outputs are row-major arrays of
 * `batch_capacity` rows, written at row batch_index.  offset + B > capacity, batch_index >= batch_capacity, B <= 0, a null
 * required pointer or rot_dim outside {4, 6}: HRP_ERR_ARG, nothing launches. */
typedef struct hrp_eval_desc {
  const float* pred_kp3d_fk;    /* [B,nkp,3] robot.get_keypoints / get_keypoints_root of the predictions   (metrics.py:27-34) */
  const float* pred_kp3d_int;   /* [B,nkp,3] pred_xyz_integral of the second call          (function.py:166; metrics.py:22-25) */
  const float* gt_kp3d;         /* [B,nkp,3] gt_keypoints3d                                    (function.py:142; metrics.py:39) */
  const float* gt_kp2d;         /* [B,nkp,2] gt_keypoints2d_original                           (function.py:143; metrics.py:40) */
  const float* K;               /* [B,9]     K_original                                    (function.py:144; metrics.py:41-43) */
  const float* pred_joint;      /* [B,dof]   pred_pose; NULL: zero joint errors            (function.py:146; metrics.py:89-91) */
  const float* gt_joint;        /* [B,dof]   gt_pose_before_mask (required with pred_joint)    (function.py:145; metrics.py:42) */
  const float* pred_rot;        /* [B,rot_dim] pred_rot                                                  (function.py:169-172) */
  const float* gt_rot;          /* [B,rot_dim] gt_rot - the BASE rotation, not the root-relative one     (function.py:169-172) */
  /* per image, FK branch (metrics.py:57, 67, 85-87, 95, 101, 110) */
  float *error3d, *error2d, *mean_jointerror, *error_depth, *batch_error_relative, *error3d_relative;
  /* per image, integral branch (metrics.py:57, 67, 95, 101, 110; its joint errors are zero by definition, :89-91) */
  float *error3d_int, *error2d_int, *error_depth_int, *batch_error_relative_int, *error3d_relative_int;
  float *dis3d, *dis2d, *dis3d_int, *dis2d_int;      /* per batch [batch_capacity, nkp] (metrics.py:71-74) */
  float* l1_jointerror;                              /* per batch [batch_capacity, dof] (metrics.py:83) */
  float* rotation_diff;                              /* per batch [batch_capacity]: mean_b acos(clamp((tr(Rp Rg^T) - 1) / 2, -1, 1))
                                                        (geometries.py:154-162; function.py:169-172) */
  int32_t B, nkp, dof;          /* nkp <= HRP_FK_MAX_KP, dof <= HRP_FK_MAX_JOINTS */
  int32_t rot_dim;              /* 6: two rows of the matrix (geometries.py:100-115); 4: quaternion w x y z (geometries.py:21-41) */
  int32_t root;                 /* reference_keypoint_id (metrics.py:94-99) */
  int32_t drop_last_joint;      /* panda: mean_jointerror leaves the last joint (the finger) out (metrics.py:84-85) */
  int32_t offset, capacity;     /* first per-image slot of this batch; length of the per-image arrays */
  int32_t batch_index, batch_capacity;
} hrp_eval_desc;
int hrp_eval_batch(const hrp_eval_desc* d, void* stream);

/* The DepthNet trainer's step after the model call in ONE launch (csrc/depth_loss.hip): scripts/train_depthnet.py:220-268 - the
 * loss, its gradient with respect to the model output, and the three per-image errors validate collects (:236-241, :289-301)
 * written straight into accumulators that live on the device for the whole epoch.  All tensors dense fp32.  The depth is divided by
 * 1000.0f (not multiplied by 1e-3f) as at :223-232, so the per-image errors are the reference's fp32 values bit for bit.
 *   plain     (xy_loss none, nk 0, W 1)   loss = L(pred / 1000, gt_root_depth), mean over B                              (:249-252)
 *   xy branch (xy_loss l1 | mse, W 3)     pred = (x, y, depth).  The depth term is L(pred[:, 2] / 1000, gt_root_depth) with the
 *             reference's shapes: a [B] prediction against a [B, 1] target, which torch broadcasts - the mean over all B * B
 *             pairs (p_j / 1000, g_i) (:223, :250).  Added to it: L_xy(pred[:, 0:2] * mask, gt_root_trans[:, 0:2] * mask), mean over
 *             all 2 B elements (masked rows count in the denominator); the xy columns are not divided by 1000        (:255-259)
 *   multi_kp  (nk > 0, W nk)              loss = L(pred / 1000, gt_kp3d[:, kp_index, 2]), mean over B * nk              (:263-266)
 * d_pred (with want_grad): gradient of the loss with respect to pred in mm - l1: sign(e) / n / 1000 with sign(0) = 0 as torch, mse:
 * 2 e / n / 1000, e = p / 1000 - g; for the xy columns the factor is mask in place of 1 / 1000.
 * errors (optional) [3, capacity]: |pred[:, root_col] / 1000 - gt_root_depth|, |x - gt_x|, |y - gt_y| per image at
 * [offset, offset + B); the last two rows receive zeros without the xy branch (:236-241).  With errors, losses[batch_index] receives
 * the loss as well.  One workgroup; every sum runs in sample order (no atomics): bit-reproducible at any B and offset.
 * B <= 0, W inconsistent with the mode, root_col >= W, nk > HRP_DEPTH_LOSS_MAX_KP, a kp_index entry >= J, offset + B > capacity,
 * batch_index >= batch_capacity, an unknown loss kind, want_grad without d_pred or a null required pointer: HRP_ERR_ARG, nothing
 * launches. */
#define HRP_DEPTH_LOSS_MAX_KP 16
enum { HRP_DEPTH_LOSS_L1 = 0, HRP_DEPTH_LOSS_MSE = 1 };
enum { HRP_XY_LOSS_NONE = 0, HRP_XY_LOSS_L1 = 1, HRP_XY_LOSS_MSE = 2 };
typedef struct hrp_depth_loss_desc {
  const float* pred;            /* [B,W] model(images, k_values), depth in mm                                        (:222-232) */
  const float* gt_root_trans;   /* [B,3] gt_keypoints3d[:, reference_keypoint_id] of the root view, or TCO's t       (:188-194) */
  const float* gt_kp3d;         /* [B,J,3] gt_keypoints3d of the root view; read with nk > 0 only                        (:197) */
  const float* mask;            /* [B]   valid_mask_crop[:, reference_keypoint_id] of the root view; xy branch only      (:247) */
  float* loss;                  /* [1] */
  float* d_pred;                /* [B,W] or NULL */
  float* errors;                /* [3,capacity] or NULL: error_depth, error_x, error_y                               (:236-241) */
  float* losses;                /* [batch_capacity]; required with errors                                                (:291) */
  int32_t B, W, J, nk;          /* nk <= HRP_DEPTH_LOSS_MAX_KP: len(kps_need_depth), 0 without multi_kp */
  int32_t kp_index[HRP_DEPTH_LOSS_MAX_KP];   /* kps_need_depth                                                            (:197) */
  int32_t depth_loss, xy_loss;  /* HRP_DEPTH_LOSS_*, HRP_XY_LOSS_*                                             (:249-254, 256-261) */
  int32_t root_col;             /* column of pred that is the root depth: 0 (W 1), 2 (xy branch),
                                   kps_need_depth.index(reference_keypoint_id) (multi_kp)                           (:223, 228-229) */
  int32_t want_grad;            /* nonzero: write d_pred */
  int32_t offset, capacity;     /* first per-image slot of this batch; row length of errors */
  int32_t batch_index, batch_capacity;
} hrp_depth_loss_desc;
int hrp_depth_loss(const hrp_depth_loss_desc* d, void* stream);

/* The bookkeeping of one step of the self-supervised trainer in ONE launch (csrc/sim2real_step.hip): the seven supervised terms
 * scripts/train_sim2real.py:313-400 computes for its logs - detached there (:396-398), so there is no gradient - and the twelve
 * values the training loop and validate hand to their AverageValueMeters (:649-660, :558-569).  All tensors dense fp32.
 * S = image_size, gt_root_depth = gt_root_trans[:, 2] (:208).
 *   loss_joint    mean (pose - gt_pose)^2                                                                    (:321-322)
 *   loss_rot      mean (rot - gt_root_rot)^2                                                                 (:330-331)
 *   loss_depth    mean |depth - gt_root_depth|                                                               (:337-338)
 *   loss_uv       mean_b ||(root_uv - gt_root_uv) / S||_2 - UNMASKED, unlike lib/core/function.py:231-235    (:350-353)
 *   loss_trans    e_b = ||trans - gt_root_trans||_2, m = mean e; m > 0.5: mean(e exp(-20 e)), else m         (:363-370)
 *   loss_error3d  mean over (b, k) of ||xyz_fk - gt_kp3d||_2                                                 (:374-377)
 *   loss_error2d  sum ||proj(K, xyz_fk) / S - gt_kp2d / S||_2 mask / sum (mask != 0), proj = (K p)[:2] / (K p)[2]
 *                 (lib/utils/transforms.py:17-21); an all-zero mask gives 0 / 0 = NaN as torch does           (:243, 381-386)
 * row[12] = loss, loss_joint, loss_rot, loss_trans, loss_uv, loss_depth, loss_error2d, loss_error3d, loss_mask, loss_scale,
 * loss_iou, loss_error3d_align.  row[0] = mask_terms[0] and row[8..11] = mask_terms[1], [3], [2], [4], mask_terms being the five
 * floats hrp_sim2real_loss wrote (loss, mask, iou, scale, align); mask_terms NULL (validation): those five are zero (:399-402).
 * meters (optional, 8-byte aligned): double sum[12] followed by int64 count; the launch adds row (widened to double, slots in
 * index order) to sum and 1 to count - a host-side memset resets them, nothing has to reach the host per step.  rows (optional)
 * [capacity, 12]: row is also written at row_index.  One workgroup; every sum runs over k within a sample, then over the samples,
 * in index order (no atomics): bit-reproducible.  B <= 0, a null required pointer, J > HRP_FK_MAX_KP, P > HRP_FK_MAX_JOINTS or
 * row_index >= capacity: HRP_ERR_ARG, nothing launches. */
typedef struct hrp_sim2real_monitor_desc {
  const float *pose, *rot, *trans, *root_uv, *depth, *xyz_fk;            /* [B,P] [B,6] [B,3] [B,2] [B,1] [B,J,3]       (:240-241) */
  const float *gt_pose, *gt_root_rot, *gt_root_trans, *gt_root_uv;      /* [B,P] [B,6] [B,3] [B,2]                     (:188-209) */
  const float *gt_kp3d, *gt_kp2d, *mask;                                /* [B,J,3] [B,J,2] [B,J] of the "other" crop   (:165-167) */
  const float* K;                                                       /* [B,9] other_K                                   (:155) */
  const float* mask_terms;                                              /* [5] of hrp_sim2real_loss, or NULL                      */
  float* row;                                                           /* [12]                                                   */
  void* meters;                                                         /* optional: double sum[12], int64 count                  */
  float* rows;                                                          /* optional [capacity, 12]                                */
  int32_t B, P, J;              /* J <= HRP_FK_MAX_KP, P <= HRP_FK_MAX_JOINTS */
  float image_size;
  int32_t row_index, capacity;
} hrp_sim2real_monitor_desc;
int hrp_sim2real_monitor(const hrp_sim2real_monitor_desc* d, void* stream);

/* Baseline JPEG decode of a batch on the device (csrc/jpeg.hip; the decoder itself is csrc/jpeg_core.h, the same functions for the
 * kernels and for a host compiler).  The host (lib/dataset/jpeg.py) parses each file's header into one hrp_jpeg_image and splits
 * its scan at the restart markers into hrp_jpeg_segment records; the device does entropy decoding, dequantisation, libjpeg's
 * "islow" inverse DCT, "fancy" chroma up-sampling and the YCbCr -> RGB step, byte-exact with libjpeg-turbo's defaults (Pillow).
 * Supported: SOF0, 8 bit, three components in one interleaved scan, luma sampling 1x1 / 2x1 / 2x2 with 1x1 chroma, down-sampled
 * chroma wider than 2 columns.  One call may mix sizes and sub-samplings.
 *   bytes    the files' bytes (at least every scan), one upload; a segment is bytes[off, off + len) and holds no marker
 *   coef     int16, 16-byte aligned: image i owns 64 * blocks(i) values at coef_off, quantised, natural order, the blocks of
 *            component 0 in raster order, then those of component 1, then 2; blocks(i) counts whole MCUs
 *   planes   uint8: the component planes of image i (padded to whole MCUs, 64 * blocks(i) bytes) at plane_off, same order
 *   frames   uint8: the [height, width, 3] RGB frame of image i at frame_off
 *   status   int32 [B]: 0, or the HRP_JPEG_ERR_* bits of what stopped a segment of the image (its remaining coefficients are zero)
 *            and HRP_JPEG_WARN_TRAILING
 * Five launches (clear, checksum, entropy, inverse DCT, colour) whatever the images hold, caller-owned buffers, no host synchronisation:
 * graph-capturable.  The kernels check every offset of every descriptor against nbytes / ncoef / nplanes / nframes and leave an
 * image whose descriptor does not fit untouched, with HRP_JPEG_ERR_DESC. */
enum {
  HRP_JPEG_ERR_DATA = 1,    /* the segment ran out of data */
  HRP_JPEG_ERR_MARKER = 2,  /* a marker inside the segment */
  HRP_JPEG_ERR_CODE = 4,    /* no Huffman code of 16 bits or fewer matches */
  HRP_JPEG_ERR_INDEX = 8,   /* a run leads past coefficient 63 */
  HRP_JPEG_ERR_DESC = 16,   /* the descriptor, a table or a segment record is inconsistent */
  HRP_JPEG_ERR_CHECKSUM = 64,   /* bytes[scan_off, scan_off + sum_len) are not the bytes the header was parsed from: their Adler-32
                                   is not scan_sum.  It ties a descriptor to its bytes on their separate ways from the loader worker
                                   to the device; damage that a file took before it was parsed is outside its reach */
  HRP_JPEG_WARN_TRAILING = 32   /* every MCU decoded, but the segment goes on: whole bytes are left, or padding bits that are not
                                   ones (a decoder that lost step with the encoder usually ends here) */
};
typedef struct hrp_jpeg_huff {
  uint8_t counts[16];       /* number of codes of length 1..16 (DHT's BITS) */
  uint8_t values[256];      /* the symbols in code order (DHT's HUFFVAL) */
} hrp_jpeg_huff;
typedef struct hrp_jpeg_image {
  int64_t scan_off, scan_len;       /* the entropy-coded bytes of the scan within `bytes`; every segment lies inside */
  int64_t coef_off;                 /* first int16 of the image in coef (a multiple of 64) */
  int64_t plane_off, frame_off;     /* first byte of the image in planes / frames */
  int32_t width, height;
  int32_t hsamp, vsamp;             /* luma sampling factors: 1x1, 2x1 or 2x2 (chroma is 1x1) */
  int32_t restart_interval;         /* MCUs per segment (DRI); 0: the whole scan is one segment */
  uint32_t scan_sum;                /* Adler-32 (zlib's) of bytes[scan_off, scan_off + sum_len), taken when the header was parsed */
  int64_t sum_len;                  /* from the first entropy-coded byte to the end of the file: sum_len >= scan_len */
  uint8_t comp_tq[4], comp_td[4], comp_ta[4];   /* per component: quantisation, DC and AC table selectors (entry 3 unused) */
  uint8_t reserved2[4];
  uint16_t quant[4][64];            /* quantisation tables, natural (row-major) order */
  hrp_jpeg_huff dc[2], ac[2];
} hrp_jpeg_image;
typedef struct hrp_jpeg_segment {
  int64_t off, len;                 /* bytes[off, off + len): one restart interval, or the whole scan */
  int32_t image, mcu0;              /* the image it belongs to and its first MCU (raster order) */
} hrp_jpeg_segment;
int hrp_jpeg_decode(const hrp_jpeg_image* images_dev, int B, const hrp_jpeg_segment* segments_dev, int nseg, const uint8_t* bytes,
                    size_t nbytes, int16_t* coef, size_t ncoef, uint8_t* planes, size_t nplanes, uint8_t* frames, size_t nframes,
                    int32_t* status, void* stream);
/* The stages on their own, for tools/bench_jpeg.py: stage 0 the clear + checksum + entropy launches, 1 the inverse DCT + colour launches.
 * lanes: segments per 64-lane wave of the entropy kernel, 1..64 (0: the default). */
int hrp_jpeg_decode_stage(int stage, int lanes, const hrp_jpeg_image* images_dev, int B, const hrp_jpeg_segment* segments_dev,
                          int nseg, const uint8_t* bytes, size_t nbytes, int16_t* coef, size_t ncoef, uint8_t* planes, size_t nplanes,
                          uint8_t* frames, size_t nframes, int32_t* status, void* stream);

/* The same decode with a second entropy stage for long segments (files without restart markers are one segment each).  A long
 * segment is cut into sub-sequences of subseq_bytes raw bytes (a power of two, 16 .. 4096) and decoded by one workgroup: every
 * lane decodes a sub-sequence from a guessed state (Huffman-coded scans fall into step after a few dozen symbols), the lanes pass
 * their exit states on in rounds until none changes - at that point every state is exact, so the number of rounds is not capped -
 * prefix sums give every sub-sequence its block number and its DC predictors, and a final pass writes the coefficients.  coef,
 * planes, frames and status end up exactly as hrp_jpeg_decode leaves them, for damaged scans too (csrc/jpeg_core.h,
 * tests/jpeg_sync_host_check.cpp).
 *   short_segments_dev [nshort]  go through hrp_jpeg_decode's one-lane kernel
 *   long_segments_dev [nlong]    one workgroup each; in ascending order of `off`, not overlapping, len > 0
 *                                either count may be 0, not both
 *   scratch  16-byte aligned, at least hrp_jpeg_sync_scratch_bytes(nbytes, nlong, subseq_bytes) =
 *            32 * (nbytes / subseq_bytes + 2 * nlong + 1) bytes (0 for a subseq_bytes that is not taken).  Every call rewrites what
 *            it reads there.  Long segment j owns the 32-byte slots from off / subseq_bytes + 2 * j on: first {uint32 rounds,
 *            uint32 sub-sequences, uint32 sub-sequences whose exit state changed after the first pass}, then one slot per
 *            sub-sequence.
 * Clear, checksum, one launch per non-empty segment list, inverse DCT, colour: a launch count fixed by the arguments, caller-owned
 * buffers, no host synchronisation, no workgroup waits for another: graph-capturable.  The kernels check every descriptor and
 * the scratch size as hrp_jpeg_decode's do. */
size_t hrp_jpeg_sync_scratch_bytes(size_t nbytes, int nlong, int subseq_bytes);
int hrp_jpeg_decode_sync(const hrp_jpeg_image* images_dev, int B, const hrp_jpeg_segment* short_segments_dev, int nshort,
                         const hrp_jpeg_segment* long_segments_dev, int nlong, int subseq_bytes, const uint8_t* bytes, size_t nbytes,
                         int16_t* coef, size_t ncoef, uint8_t* planes, size_t nplanes, uint8_t* frames, size_t nframes, void* scratch,
                         size_t nscratch, int32_t* status, void* stream);
/* Its stages on their own, for tools/bench_jpeg.py and the tests: stage 0 the entropy launches, 1 the pixel launches.  guess_unit,
 * guess_k: the state every sub-sequence but the first starts from (block within the MCU, zig-zag index; hrp_jpeg_decode_sync
 * passes 0, 0; the result does not depend on them, the number of rounds does). */
int hrp_jpeg_decode_sync_stage(int stage, int guess_unit, int guess_k, const hrp_jpeg_image* images_dev, int B,
                               const hrp_jpeg_segment* short_segments_dev, int nshort, const hrp_jpeg_segment* long_segments_dev, int nlong,
                               int subseq_bytes, const uint8_t* bytes, size_t nbytes, int16_t* coef, size_t ncoef, uint8_t* planes,
                               size_t nplanes, uint8_t* frames, size_t nframes, void* scratch, size_t nscratch, int32_t* status, void* stream);

/* Streaming pose tracker (csrc/track.hip; the arithmetic is csrc/track_core.h, the same functions for the kernels and for a host
 * compiler, tests/track_host_check.cpp): this frame's crop from the last frame's estimate, on the device.  Replaces what the
 * reference's loader computes from ANNOTATED key-points (lib/dataset/dream.py:171-216, 287-394; roboutils.py:59-156, 224-257;
 * lib/utils/geometries.py:360-395) and the k_values of the step (lib/core/function.py:43-48, 88-98), fed the key-points that the
 * model predicted for the previous frame.  process_truncation is not part of it: the tracker crops inside the frame.
 *
 * hrp_track_prepare, one launch: every workgroup derives its stream's hrp_track_geom once (float64, the loader's order of
 * operations, int() where the host truncates, no contraction) and then writes its share of the pixels of both views, reading the
 * frame directly (hrp_dream_crop_resize's arithmetic without the enhancement tail; no scratch copy of the frame).
 *   frames [B, H, W, 3] uint8; state_kp2d [B, nkp, 2] float64, the estimate in ORIGINAL-image pixels; state_have [B] int32 (0: no
 *   estimate, the whole frame is taken); K_original [B, 9] fp32 row-major pinhole intrinsics (no skew);
 *   out_root [B, 3, h0, w0] uint8; out_other [B, 3, h1, w1] uint8 or NULL when the two views have one size (the caller aliases
 *   them; K_other then equals K_root); h = min, w = max of the reference's resize_hw, whose first entry bounds x and whose second
 *   bounds y in the boxes, as there; extend_ratio: two host doubles (dream.py's extend_ratio);
 *   bbox_mode: the box and K that k_values takes (function.py:43-48): HRP_TRACK_BBOX_EXTENDED (use_extended_bbox),
 *   HRP_TRACK_BBOX_ORIGIN (use_origin_bbox) or HRP_TRACK_BBOX_STRICT;
 *   K_root, K_other [B, 9] fp32, k_values [B] fp32, geom [B] hrp_track_geom: outputs.
 * The estimate of a stream is treated as absent for this frame - whole frame, HRP_TRACK_NO_ESTIMATE | HRP_TRACK_BAD_BOX - when its
 * crop box fails the loader's check 0 <= x0 < x1 <= W, 0 <= y0 < y1 <= H (dream.py:318), when k_value is not finite and positive, or
 * when an input is not finite; HRP_TRACK_NO_ESTIMATE alone means state_have was 0.  Every float -> int conversion is range-checked
 * first, and every frame index is tested against W, H immediately before its load, whatever the record says.
 *
 * hrp_track_update, one launch: kp2d = (fx X / Z + cx, fy Y / Z + cy) in float64 of xyz_fk [B, nkp, 3] fp32 (camera frame) into
 * state_kp2d and, as fp32, kp2d_out [B, nkp, 2]; state_have = 1 iff every coordinate is finite, every Z > 0 and at least min_inside
 * key-points lie in [0, W) x [0, H), otherwise 0 and HRP_TRACK_LOST_OUT is ORed into status [B] (which the caller initialised, e.g.
 * from hrp_track_geom.status).
 * Grids depend on the host arguments only, caller-owned buffers, no host synchronisation: graph-capturable. */
enum { HRP_TRACK_NO_ESTIMATE = 1, HRP_TRACK_BAD_BOX = 2, HRP_TRACK_LOST_OUT = 4 };
enum { HRP_TRACK_BBOX_EXTENDED = 0, HRP_TRACK_BBOX_ORIGIN = 1, HRP_TRACK_BBOX_STRICT = 2 };
#define HRP_TRACK_MAX_KP 32
#define HRP_TRACK_MAX_SIZE 4096
typedef struct {
  int32_t status;                                   /* HRP_TRACK_NO_ESTIMATE | HRP_TRACK_BAD_BOX */
  int32_t crop_x0, crop_y0, crop_x1, crop_y1;       /* the crop box in the frame (get_bbox, strict) */
  int32_t side, off_x, off_y;                       /* resize_image's square canvas and the crop's offset in it */
  float bbox_strict_bounded[2][4];                  /* per view (0 root, 1 other) */
  float bbox_gt2d_extended[2][4];                   /* per view */
  float bbox_strict_bounded_original[4];
} hrp_track_geom;
int hrp_track_prepare(const uint8_t* frames, const double* state_kp2d, const int32_t* state_have, const float* K_original, int B, int H,
                      int W, int nkp, uint8_t* out_root, int h0, int w0, uint8_t* out_other, int h1, int w1, const double* extend_ratio,
                      int bbox_mode, float* K_root, float* K_other, float* k_values, hrp_track_geom* geom, void* stream);
int hrp_track_update(const float* xyz_fk, const float* K_original, int B, int nkp, int W, int H, int min_inside, double* state_kp2d,
                     int32_t* state_have, float* kp2d_out, int32_t* status, void* stream);

/* Tracker acquisition: a detector's key-points become the estimate of the streams that have none (csrc/track_core.h track_seed,
 * host and device code like track_geometry; tests/track_seed_host_check.cpp).  hrp_track_seed is one launch, one lane per stream.
 *   det_kp [B, nkp, 2] fp32 in DETECTOR pixels (x, y); inv_scale: two host doubles, frame pixels per detector pixel (x, y);
 *   mask [B, hm, wm] fp32 at detector resolution with min_prob, or NULL; ms [B, nkp, 2] (max logit, sum exp(l - max)) as
 *   hrp_kp_readout_fwd / hrp_softargmax_flat_fwd report them, with min_peak, or NULL; state_kp2d [B, nkp, 2] float64,
 *   state_have [B] int32: the tracker's state; seed_status [B] int32: output.
 * Per stream: have == 1 and force == 0 leave the state untouched (HRP_SEED_SKIPPED).  Otherwise u = (double)det_kp * inv_scale; a
 * key-point COUNTS when it is finite, lies in [0, W) x [0, H), (with a mask) the mask at the truncated detector pixel is >= min_prob
 * and (with ms) the peak probability 1 / sum-exp is >= min_peak.  If every key-point is finite and at least min_inside count, all
 * nkp points go into the state, have = 1 (HRP_SEED_TAKEN); otherwise the state is untouched (HRP_SEED_REFUSED).  Every value is
 * range-checked before every float -> int conversion.  No host synchronisation, caller-owned buffers: graph-capturable. */
enum { HRP_SEED_SKIPPED = 1, HRP_SEED_TAKEN = 2, HRP_SEED_REFUSED = 4 };
int hrp_track_seed(const float* det_kp, int B, int nkp, const double* inv_scale, const float* mask, int hm, int wm, float min_prob,
                   const float* ms, float min_peak, int min_inside, int force, int W, int H, double* state_kp2d, int32_t* state_have,
                   int32_t* seed_status, void* stream);

/* Tracker verification: the estimate of every stream is compared with the detector's foreground map of this frame, and a stream
 * whose estimate does not agree loses it (have = 0), so that the hrp_track_seed launch that follows takes the detection
 * (csrc/track_core.h track_verify, host and device code like track_seed; tests/track_verify_host_check.cpp, the float64 numpy
 * statement is tests/track_verify_oracle.py).  hrp_track_verify is ONE launch, one 256-lane workgroup per stream.
 *   state_kp2d [B, nkp, 2] float64 in frame pixels (read only), state_have [B] int32: the tracker's state;
 *   scale: detector pixels per frame pixel (x, y), two host doubles that the caller computed itself (never 1 / inv_scale on the
 *   device); mask [B, hm, wm] fp32 at detector resolution; alpha [B, hm, wm] fp32, the soft silhouette of the last prediction at
 *   the same resolution, or NULL; bones [nb][2] key-point index pairs, by value; samples S per bone; extend_ratio as in
 *   hrp_track_prepare; min_prob, min_fg, min_samples; min_support, min_coverage, min_iou: a negative value switches the criterion off;
 *   verify_status [B] int32, counts [B, 4] int32 = (h_s, n_s, n_in, n_fg), sums [B, 3] float64 = (I, S, R): outputs.
 * Per stream, in this order, float64 wherever a value is computed:
 *   0. have == 0: HRP_VERIFY_SKIPPED; counts and sums are written as zero, the state is untouched.
 *   1. a state coordinate, or its product with scale, is not finite: HRP_VERIFY_DROPPED, have = 0; counts and sums are zero.
 *   2. d_i = u_i * scale: the key-points in detector pixels.
 *   3. support: the sample points are every d_i and, for each bone (a, b) and j = 0 .. S - 1, d_a + t (d_b - d_a) with
 *      t = (j + 0.5) / S.  A sample COUNTS (n_s) when 0 <= x < wm and 0 <= y < hm (tested in double before the cast); it HITS (h_s)
 *      when mask[(int)y * wm + (int)x] >= min_prob (a NaN pixel compares false).  Samples outside the map are not counted at all.
 *   4. coverage: the box is [min x - e0 w, min y - e1 h, max x + e0 w, max y + e1 h] over all d_i, w = max x - min x,
 *      h = max y - min y, e = extend_ratio.  A pixel is foreground (n_fg) when mask >= min_prob; it is inside (n_in) when it is
 *      foreground and its centre (x + 0.5, y + 0.5) lies in the closed box.
 *   5. IoU, only with alpha: I = sum m a, S = sum m, R = sum a over the whole map, every fp32 value widened to double, products in
 *      double, sums in a fixed order; iou = I / (S + R - I) (s2r_sums_kernel's measure).  Without alpha I = R = 0 and S = sum m.
 *   6. n_fg < min_fg: HRP_VERIFY_UNDECIDED (the detector sees no robot), the state is untouched.  Otherwise every enabled criterion
 *      can fail, each comparison written !(score >= min) so that a NaN score fails: support on !(h_s / n_s >= min_support), not
 *      applied when n_s < min_samples; coverage on !(n_in / n_fg >= min_coverage); IoU on !(iou >= min_iou).  Any failure: have = 0
 *      and HRP_VERIFY_DROPPED | HRP_VERIFY_FAIL_*, one bit per failed criterion.  None: HRP_VERIFY_KEPT.
 * The key-point coordinates of the state are never written, only have.  Every value is range-checked before every float -> int
 * conversion and every mask index is tested against hm, wm immediately before its load.  The sums of one stream are taken in an
 * order that depends only on the arguments (and on the 16-byte alignment of the stream's maps): no atomics, two runs are
 * bit-equal.  The grid depends on B only, caller-owned buffers, no host synchronisation: graph-capturable.
 * Refused (HRP_ERR_ARG, nothing is launched): null required pointers, B outside 1 .. 65535, nkp outside 1 .. HRP_TRACK_MAX_KP,
 * hm / wm outside 1 .. HRP_TRACK_MAX_SIZE, nb outside 0 .. HRP_TRACK_MAX_BONES, a bone index outside [0, nkp), samples outside
 * 1 .. 64, scale or extend_ratio not finite, scale not positive, a threshold above 1 or NaN, min_iou >= 0 without alpha. */
enum {
  HRP_VERIFY_SKIPPED = 1, HRP_VERIFY_KEPT = 2, HRP_VERIFY_UNDECIDED = 4, HRP_VERIFY_DROPPED = 8,
  HRP_VERIFY_FAIL_SUPPORT = 16, HRP_VERIFY_FAIL_COVERAGE = 32, HRP_VERIFY_FAIL_IOU = 64
};
#define HRP_TRACK_MAX_BONES 32
#define HRP_TRACK_MAX_SAMPLES 64
typedef struct {
  const double* state_kp2d;
  int32_t* state_have;
  const float* mask;
  const float* alpha;                                /* or NULL */
  int32_t* verify_status;
  int32_t* counts;
  double* sums;
  int32_t B, nkp, hm, wm;
  int32_t nb, samples, min_fg, min_samples;
  int32_t bones[HRP_TRACK_MAX_BONES][2];
  double scale[2], extend_ratio[2];
  double min_support, min_coverage, min_iou;
  float min_prob;
  int32_t reserved;
} hrp_track_verify_desc;
int hrp_track_verify(const hrp_track_verify_desc* d, void* stream);

/* CtRNet key-point read-out and spatial soft-argmax, forward only (csrc/kp_readout.hip; reference
 * lib/models/ctrnet/keypoint_seg_resnet.py:29-33 KeypointUpSample.forward, 75-100 SpatialSoftArgmax.forward, 137-143):
 *   heat = conv_transpose2d(x, w, b, stride 2, padding 1) [B, k, 2 Hin, 2 Win]; p = softmax over the positions of each (b, c);
 *   kp[b, c] = (sum p xc - lim0, sum p yc - lim2) * (scale_x, scale_y), xc = linspace(-1, 1, 2 Win), yc = linspace(-1, 1, 2 Hin) in
 *   fp32 as torch computes them; order (x, y).  The logits are fp32 accumulators of the matrix cores (mfma_f32_32x32x16_bf16 for
 *   HRP_BF16 features, mfma_f32_32x32x2f32 for HRP_F32 and HRP_F32X3) and are never stored or rounded below fp32; partial sums are
 *   combined in a fixed order, so the result is bit-reproducible from run to run.
 * hrp_kp_readout_pack: weight [Cin, k, 4, 4] fp32 (nn.ConvTranspose2d's layout) -> the kernel's operand layout
 *   [parity 4][tap 4][Cin / V][32][V] in the element type of `dtype` (V = 8 bf16 / 4 fp32): 16 * Cin * 32 elements.
 * hrp_kp_readout_ws: bytes of the workspace (one softmax partial per (b, row strip of HRP_KP_STRIP_ROWS input rows, channel)).
 * hrp_kp_readout_fwd: x [B, Hin, Win, pitch] NHWC in `dtype`, 16-byte aligned, pitch a multiple of V; bias [k] fp32;
 *   kp [B, k, 2] fp32; ms [B, k, 2] = (maximum logit, sum exp(l - max)), so 1 / ms[..., 1] is the peak probability, or NULL.
 * Refused (HRP_ERR_ARG): Cin not a multiple of 32, k outside 1 .. HRP_TRACK_MAX_KP, empty maps, null pointers. */
#define HRP_KP_STRIP_ROWS 1
int hrp_kp_readout_pack(const float* weight, int Cin, int k, void* packed, int dtype, void* stream);
int64_t hrp_kp_readout_ws(int B, int Hin);
int hrp_kp_readout_fwd(const void* x, int dtype, int B, int Hin, int Win, int Cin, int pitch, const void* packed, const float* bias,
                       int k, float lim0, float lim2, float scale_x, float scale_y, float* kp, float* ms, void* ws, int64_t ws_bytes,
                       void* stream);

/* Kinematic refit: joint angles and, optionally, the camera pose from key-points by Levenberg-Marquardt (csrc/kin_core.h, host and
 * device code; csrc/kin.hip; tests/kinfit_host_check.cpp).  It replaces nothing in the reference, which never estimates the joint
 * state from image evidence at inference: scripts/test.py only has the `known_joint` switch that substitutes the ground truth.
 * hrp_kin_solve is ONE launch, one 64-lane workgroup per sample, fp64 inside.  With p = (free joints ascending, then w, t when
 * free_pose; w angle-axis) it minimises
 *   C(p) = sum_k w2d[k] |x_k - pi(K, X_k(p))|^2                 (pixels^2)
 *        + sum_k w3d[k] |Y_k - X_k(p)|^2                         (3-D targets in the camera frame, w3d in px^2 / m^2)
 *        + sum_{j free} prior_q[j] (q_j - q0_j)^2                (px^2 per rad^2 or m^2)
 *   X_k(p) = M FK_k(q),  M = [R(w) | t] for root == 0,  M = [R(w) | t] T_root(q)^-1 for root > 0 (the FK kernels' re-rooting), so a
 *   network's rot / trans at its reference key-point go in as they are.  pi(K, X) = (K X)[:2] / (K X)[2].
 * nkp and dof repeat the chain's counts (the chain lives on the device and the launch is sized on the host); the kernel uses the
 * descriptor's.  rot_dim 6: two rows of R by the FK kernels' formula on input, the first two rows of R(w) on output.
 *   LM loop      lm_refine's schedule (pnp.hip) unchanged: lambda0 = 1e-3, A = J^T J + lambda diag(J^T J), x0.1 on an accepted trial
 *                (not below 1e-12), x10 otherwise.  It stops at an accepted step with max|step| <= 1e-12 (1 + max|p|) or at
 *                lambda > 1e10 (both set HRP_KIN_CONVERGED), or after HRP_KIN_MAX_IT trials.
 *   trial        clamp(p + delta) on the joint entries, to [q_lo, q_hi] (fmin(fmax(v, lo), hi): lo > hi gives hi).  The step that is
 *                tested is the change after clamping.  A trial is accepted only if C drops; it is rejected when a used 2-D point has
 *                camera depth X_z <= 0 or the cost is not finite, and when the damped matrix has a pivot that is not positive.
 *   held joints  a free joint that sits on (or beyond) a bound while the descent direction -g_j points across it is held for the
 *                trials from that linearisation: its row and column of the damped matrix are the identity's and its step is 0, so
 *                the other parameters take the step of the problem with that joint fixed (an active set of one linearisation; without
 *                it the clamped full step no longer lowers C next to a bounded optimum and the loop stalls short of it).  It is
 *                released by the first linearisation whose gradient points back inside.
 *   usable       a point is used when its weight is > 0 and its coordinates are finite (a NaN weight is not > 0).
 *   rows         2 n2d + 3 n3d + #{free j : prior_q[j] > 0}.  With rows < npar, or npar == 0, nothing is solved:
 *                HRP_KIN_FEW_ROWS, and q, rot, trans are the start, bit for bit.
 *   bad start    a start with a used 2-D point at depth <= 0 or a cost that is not finite: HRP_KIN_BAD_START, outputs as the start.
 *   at limit     HRP_KIN_AT_LIMIT when a free joint ends exactly on a bound.
 *   rms          sqrt(sum w2d e^2 / sum w2d) over the used 2-D points at the returned parameters (0 without any).
 *   cov          s^2 (J^T J)^-1 at the solution, J^T J including the priors, in parameter order, s^2 = C / (rows - npar); all zeros
 *                when rows <= npar, on a pivot that is not positive, with HRP_KIN_AT_LIMIT, or when nothing was solved.
 *   unobservable a free joint that moves no used point and has no prior makes diag(J^T J) = 0 there, the damped matrix is singular at
 *                every lambda, every trial fails, lambda rises and the loop ends with the start: nothing undefined happens.
 * Fixed entries are copied through bit for bit (fixed joints, and rot / trans when free_pose == 0); a returned free w has |w| <= pi.
 * Inside, a fixed pose is used through its angle-axis vector like a free one (R(log R) is R to a few ulp of fp64).
 * xyz / uv are the FK key-points at the returned parameters and their projection, for every key-point.  Every sum is taken in index
 * order, so two calls return the same bytes.  dof <= HRP_FK_MAX_JOINTS and nkp <= HRP_FK_MAX_KP give npar <= 38 and at most 120
 * residual rows in LDS (the priors are added analytically), under 64 KB.  No host synchronisation, caller-owned buffers:
 * graph-capturable.
 * Refused (HRP_ERR_ARG, nothing is launched): a null descriptor or required pointer (chain, pts2d, K, rot0, trans0, rot, trans,
 * and q0, q when dof > 0), B <= 0, rot_dim not 3 or 6, nkp outside 1 .. HRP_FK_MAX_KP, dof outside 0 .. HRP_FK_MAX_JOINTS, a free_q bit at or above
 * dof, pts3d without w3d or the reverse, K_stride not 0 or 9, pose_stride / free_pose not 0 or 1, root outside [0, nkp). */
enum { HRP_KIN_CONVERGED = 1, HRP_KIN_AT_LIMIT = 2, HRP_KIN_FEW_ROWS = 4, HRP_KIN_BAD_START = 8 };
#define HRP_KIN_MAX_IT 200
typedef struct hrp_kin_desc {
  const hrp_fk_chain* chain;              /* device */
  const float *pts2d, *w2d;               /* [B,nkp,2]; [B,nkp] >= 0 or NULL (= 1) */
  const float *pts3d, *w3d;               /* [B,nkp,3], [B,nkp]; both or neither */
  const float* K; int32_t K_stride;       /* 9, or 0 = shared */
  int32_t nkp;                            /* the chain's nkp */
  const float* q0;                        /* [B,dof] start and prior mean */
  const float *rot0, *trans0;             /* [B,rot_dim], [B,3]; stride 0 = one pose for all (a calibrated camera) */
  int32_t rot_dim, pose_stride;           /* 3 angle-axis | 6 two rows of R; 1 = per sample, 0 = shared */
  const float *q_lo, *q_hi, *prior_q;     /* [dof] each, optional */
  uint32_t free_q; int32_t free_pose, root, B;
  int32_t dof, reserved;                  /* the chain's dof */
  float *q, *rot, *trans;                 /* [B,dof], [B,rot_dim], [B,3]: the solution, fixed entries copied through */
  float *xyz, *uv;                        /* optional [B,nkp,3], [B,nkp,2] */
  float* rms; int32_t* status; float* cov;/* [B]; [B,4] = (flags, LM trials, rows, npar); optional [B,npar,npar] */
} hrp_kin_desc;
int hrp_kin_solve(const hrp_kin_desc* d, void* stream);

/* Multi-view kinematic refit: the joint angles of one arm from the key-points seen by V fixed, calibrated cameras
 * (csrc/kin_views_core.h, host and device code; csrc/kin_views.hip; tests/kinviews_host_check.cpp; tests/kinviews_oracle.py is the
 * float64 statement).  hrp_kin_solve_views is ONE launch, one 64-lane workgroup per sample, fp64 inside, no atomics and no shuffles.
 * View v = 0 .. V-1, 1 <= V <= HRP_KIN_MAX_VIEWS, has intrinsics K_v, a fixed camera-from-base pose (w_v, t_v) - angle-axis, then
 * translation: the cTr of a fixed-camera calibration -, 2-D key-points x_vk and optional weights.  With p = the free joints ascending
 * it minimises
 *   C(p) = sum_v sum_k w2d[v,k] |x_vk - pi(K_v, R(w_v) FK_k(q) + t_v)|^2  +  sum_{j free} prior_q[j] (q_j - q0_j)^2
 * Everything else is hrp_kin_solve's with free_pose = 0 and root = 0, with "the used 2-D points" read as those of all views: the LM
 * loop, the trial and its clamping, the held joints and the stopping rules; usable points (a view whose points are all NaN or of
 * weight 0 contributes nothing); rows = 2 (used points over all views) + priors; HRP_KIN_FEW_ROWS, HRP_KIN_BAD_START,
 * HRP_KIN_AT_LIMIT and HRP_KIN_CONVERGED; a trial is rejected when a used point of ANY view has camera depth <= 0; cov under the same
 * conditions; fixed joints are copied through bit for bit.  Every sum is taken in a fixed order - views ascending, then
 * hrp_kin_solve's row order - so two calls return the same bytes.  The forward kinematics runs once per evaluation, whatever V is.
 * rms is taken over the used points of all views, rms_view [V] over each view's (0 for a view without any): a camera that has moved
 * since its calibration shows there.  used_view [V]: the used points per view.  xyz / uv: the camera-frame key-points of every view at
 * the returned joints and their projections.  No host synchronisation, caller-owned buffers: graph-capturable.
 * Refused (HRP_ERR_ARG, nothing is launched): a null descriptor or required pointer (chain, pts2d, K, poses, and q0, q when dof > 0),
 * B <= 0, V outside 1 .. HRP_KIN_MAX_VIEWS, nkp outside 1 .. HRP_FK_MAX_KP, dof outside 0 .. HRP_FK_MAX_JOINTS, a free_q bit at or
 * above dof, K_stride not 0 or 9, pose_stride not 0 or 1, more than 64 KB of LDS (the largest legal sizes need 61 KB). */
#define HRP_KIN_MAX_VIEWS 8
typedef struct hrp_kin_views_desc {
  const hrp_fk_chain* chain;              /* device */
  const float *pts2d, *w2d;               /* [B,V,nkp,2]; [B,V,nkp] >= 0 or NULL (= 1) */
  const float* K; int32_t K_stride;       /* [B,V,9] with 9, or [V,9] with 0 = shared over the batch */
  int32_t nkp;                            /* the chain's nkp */
  const float* q0;                        /* [B,dof] start and prior mean */
  const float* poses;                     /* [B,V,6] or [V,6]: (w_v, t_v) camera from base */
  int32_t pose_stride, V;                 /* 1 = per sample, 0 = shared over the batch */
  const float *q_lo, *q_hi, *prior_q;     /* [dof] each, optional */
  uint32_t free_q; int32_t B;
  int32_t dof, reserved;                  /* the chain's dof */
  float* q;                               /* [B,dof]: the solution, fixed joints copied through */
  float *xyz, *uv;                        /* optional [B,V,nkp,3], [B,V,nkp,2] */
  float *rms, *rms_view;                  /* [B]; [B,V] */
  int32_t *status, *used_view;            /* [B,4] = (flags, LM trials, rows, npar); [B,V] */
  float* cov;                             /* optional [B,npar,npar] */
} hrp_kin_views_desc;
int hrp_kin_solve_views(const hrp_kin_views_desc* d, void* stream);

/* Kinematic filter: hrp_kin_solve's parameters tracked over frames by an iterated extended Kalman filter in information form, with a
 * constant-velocity prior and an innovation gate (csrc/kin_filter_core.h, host and device code; csrc/kin_filter.hip;
 * tests/kinfilter_host_check.cpp; tests/kinfilter_oracle.py is the float64 statement).  hrp_kin_filter_step is ONE launch per frame, one
 * 64-lane workgroup per stream, fp64 inside, no atomics and no shuffles, every sum in index order: two calls from equal state return
 * equal bytes.  No host synchronisation and caller-owned buffers: graph-capturable.
 * State per stream, caller-owned, read and written in place: mean fp64 [B, 2n] = (p, v) with p hrp_kin_solve's parameter vector (free
 * joints ascending, then w, t when free_pose) and v its rate per second; cov fp64 [B, 2n, 2n]; valid, coast int32 [B].
 * n = npar, 1 .. HRP_KIN_FILTER_MAX_N.  Of cov the step reads the upper triangles of the (p, p) and (v, v) blocks and the whole (v, p)
 * block; it writes a symmetric matrix.
 *   start      a stream with valid == 0, or with keep[b] == 0 (keep optional), starts this frame: p from q_in / rot_in / trans_in, v = 0,
 *              P = diag(p0_var[2n]); no prediction and no gate; HRP_KF_INIT.
 *   predict    p- = p + dt v, v- = v, P- = F P F^T + Q, F = [[I, dt I], [0, I]], Q_i = q_acc[i] [[dt^4/4, dt^3/2], [dt^3/2, dt^2]]
 *              (white-noise acceleration per parameter).  A = P-_pp, B = P-_vp, C = P-_vv.  A pivot of A that is not positive, a used
 *              point at depth <= 0 at p- or a cost that is not finite there: the stream starts again from the inputs (HRP_KF_INIT).
 *              Inputs that are not usable either: HRP_KF_BAD_START, valid = 0, q / rot / trans are the inputs bit for bit, the
 *              state is left as it was.
 *   usable     a point is usable when w2d > 0 and its coordinates are finite.  w2d is an inverse variance in px^-2 (NULL = 1): the
 *              cost below has no unit.
 *   gate       gate_chi2 > 0, streams that did not start: with H_k the 2 x n Jacobian block and r_k the residual of usable point k
 *              at p-, S_k = H_k A H_k^T + I / w2d_k, d2_k = r_k^T S_k^-1 r_k; a point with d2_k > gate_chi2 is not used this frame.
 *   update     p+ minimises sum_k w2d_k |x_k - pi(K, X_k(p))|^2 + sum_{j free} w_q[j] (q_j - q_meas_j)^2 + (p - p-)^T A^-1 (p - p-)
 *              by hrp_kin_solve's loop (schedule, clamping to [q_lo, q_hi], held joints, stopping rules) from p- with its joints
 *              clamped to the bounds (the prior's mean stays p- itself, and so does a coasted state).  w_q [dof] and
 *              q_meas [B, dof] go together and are optional; only entries with w_q > 0 are read.  With M = J^T W J + diag(w_q) + A^-1
 *              at p+:  A+ = M^-1, G = B A^-1, v+ = v- + G (p+ - p-), P+ = [[A+, A+ G^T], [G A+, C - G (A - A+) G^T]].  No s^2 factor;
 *              A^-1 makes M positive definite, so the covariance is written on a joint limit too.  coast = 0.  A pivot of M that is
 *              not positive (not finite inputs): valid = 0, HRP_KF_LOST.
 *   coast      no usable point left after the gate: the state becomes the prediction (for a starting stream: the start), coast += 1,
 *              HRP_KF_COASTED; with coast > max_coast, valid = 0 and HRP_KF_LOST.  The outputs are those of the prediction.
 *   wrap       the state keeps w as the loop leaves it; only when |w| > pi it is brought back to |w| <= pi, the three rotational
 *              rates are set to 0, their rows and columns of P to 0 with p0_var's variances on the diagonal, HRP_KF_REWRAPPED.  The
 *              additive model p- = p + dt v of the pose holds away from |w| = pi.
 *   fixed      q_in supplies the fixed joints every frame, rot_in / trans_in the pose when free_pose == 0 (pose_stride 0: one
 *              calibrated camera for all streams); they are copied to the outputs bit for bit.
 * Outputs (fp32): q, rot (rot_dim 3 | 6), trans, and optionally xyz, uv (FK key-points at p+ and their projection), vel [B, n],
 * cov_p [B, n, n] (A+), xyz_next [B, nkp, 3] (FK at p+ + dt v+, the joints not clamped), d2 [B, nkp] (the gate statistics, NaN where
 * none was computed), status [B, 4] = (flags, LM trials, points used, points gated).
 * Refused (HRP_ERR_ARG, nothing is launched): what hrp_kin_solve refuses, and dt not positive or not finite, gate_chi2 NaN, n = 0 or
 * n > HRP_KIN_FILTER_MAX_N, a null state pointer (mean, cov, valid, coast) or q_acc / p0_var, max_coast < 0, w_q without q_meas
 * or the reverse. */
enum {
  HRP_KF_INIT = 1, HRP_KF_COASTED = 2, HRP_KF_LOST = 4, HRP_KF_BAD_START = 8, HRP_KF_REWRAPPED = 16, HRP_KF_CONVERGED = 32,
  HRP_KF_AT_LIMIT = 64
};
#define HRP_KIN_FILTER_MAX_N 20
typedef struct hrp_kin_filter_desc {
  const hrp_fk_chain* chain;              /* device */
  const float *pts2d, *w2d;               /* [B,nkp,2]; [B,nkp] inverse variances or NULL (= 1) */
  const float* K; int32_t K_stride;       /* 9, or 0 = shared */
  int32_t nkp;                            /* the chain's nkp */
  const float* q_in;                      /* [B,dof] start of the free joints, value of the fixed ones */
  const float *rot_in, *trans_in;         /* [B,rot_dim], [B,3]; stride 0 = one pose for all */
  int32_t rot_dim, pose_stride;
  const float *q_lo, *q_hi;               /* [dof] each, optional */
  const float *w_q, *q_meas;              /* [dof], [B,dof]: both or neither */
  const int32_t* keep;                    /* [B] optional: 0 = start this frame */
  const double *q_acc, *p0_var;           /* [n], [2n] */
  uint32_t free_q; int32_t free_pose, root, B, dof, max_coast;
  double dt, gate_chi2;                   /* seconds; <= 0 = no gate */
  double *mean, *cov; int32_t *valid, *coast;        /* the state */
  float *q, *rot, *trans;                 /* [B,dof], [B,rot_dim], [B,3] */
  float *xyz, *uv, *vel, *cov_p, *xyz_next, *d2;     /* optional */
  int32_t* status;                        /* optional [B,4] */
} hrp_kin_filter_desc;
int hrp_kin_filter_step(const hrp_kin_filter_desc* d, void* stream);

/* Kinematic smoother: a Rauch-Tung-Striebel pass over a recorded history of the filter's posteriors (csrc/kin_smooth_core.h, host and
 * device code; csrc/kin_smooth.hip; tests/kinsmooth_host_check.cpp; tests/kinsmooth_oracle.py is the float64 statement).
 *
 * hrp_kin_history_push is ONE launch that copies the filter's state after a step into slot `slot` of a ring of `cap` slots: mean
 * [cap, B, 2n] and cov [cap, B, 2n, 2n] fp64, valid and flags [cap, B] int32 (flags = status[b][0] of the step), dt [cap] fp64 (the
 * step's dt, a kernel argument), q_in [cap, B, dof] fp32 (the step's q_in).  Refused: a null pointer, B < 1, n outside
 * 1 .. HRP_KIN_FILTER_MAX_N, dof outside 0 .. HRP_FK_MAX_JOINTS, cap < 1, slot outside 0 .. cap - 1, dt not positive or not finite.
 *
 * hrp_kin_smooth reads the ring as it lies: frame t = 0 .. L-1, oldest first, is slot (first + t) % cap.  Frame t carries the
 * posterior x+_t = mean, P+_t = cov after its step, valid_t, the step's flags_t and that step's dt_t.
 *   frame      usable when valid_t == 1 and its mean and the diagonal of its cov are finite; otherwise HRP_KS_INVALID, its outputs are
 *              zeros and it belongs to no segment.
 *   link       t -> t+1 exists when both frames are usable and flags_{t+1} has none of HRP_KF_INIT, HRP_KF_BAD_START,
 *              HRP_KF_REWRAPPED (an INIT frame took its prior from the inputs, not from t; a REWRAPPED frame's state is in another
 *              chart of the rotation than the prediction from t).  COASTED frames link: their posterior is the prediction.
 *              With F = [[I, dt I], [0, I]], dt = dt_{t+1}, and Q the filter's white-noise-acceleration matrix of q_acc:
 *              x- = F x+_t, P- = F P+_t F^T + Q, G = P+_t F^T (P-)^-1 (Cholesky of P-, 2n solves).  A pivot of P- that is not
 *              positive or not finite, or a G that is not finite, cuts the link: HRP_KS_BAD_LINK on t.
 *   linked     x^s_t = x+_t + G (x^s_{t+1} - x-), P^s_t = P+_t + G (P^s_{t+1} - P-) G^T; HRP_KS_SMOOTHED.
 *   tail       a usable frame without a link (the newest, or before a cut): x^s = x+, P^s = P+, HRP_KS_TAIL; mean_s / cov_s are the
 *              history's bytes, the fp32 outputs are recomputed from the state.
 *   outputs    the recursion runs on unclamped values.  q: a free joint is x^s clamped to [q_lo, q_hi] (HRP_KS_CLAMPED when that moved
 *              it), a fixed joint is the frame's recorded q_in bit for bit.  rot / trans: from x^s when free_pose (a rotation beyond pi
 *              is wrapped for output, as the filter does), else rot_fixed / trans_fixed bit for bit.  vel [n] and cov_p [n, n] (the
 *              (p, p) block of P^s) from x^s, P^s; xyz [nkp, 3]: FK (kin_core.h's) at the output's q and pose.  No K is taken and no uv is
 *              returned: the caller projects.  status [2] = (flags, number of later frames that reached this one through links).
 *              Optional fp64 mean_s [L, B, 2n] (unclamped) and cov_s [L, B, 2n, 2n] (bit-symmetric).
 *   want_cov   0 skips the covariance recursion; cov_p and cov_s are then not written and may be NULL.  The other outputs have the
 *              same bytes either way.
 * Outputs are [L, B, ...], oldest first.  Frame t depends on frames t .. L-1 only: smoothing the newest `lag` frames gives the last `lag`
 * rows of smoothing everything, byte for byte.  Every sum runs in index order, no atomics, no shuffles, symmetric results are computed
 * on one triangle and mirrored: two calls return equal bytes and a stream's bytes do not depend on B.
 * Two launches on the caller's stream: links, grid (L, B) (P-, its factor, G and the decision into the caller's scratch gain
 * [L, B, 2n, 2n] fp64 and link [L, B] int32), then the walk t = L-1 .. 0, grid (B).  Nothing synchronises.
 * Refused (HRP_ERR_ARG, nothing is launched): a null required pointer (chain, the ring, q_acc, gain, link, rot, trans, vel, xyz,
 * status; q_in and q when dof > 0; cov_p when want_cov; rot_fixed / trans_fixed when free_pose == 0), B < 1 or B > 65535, L < 1,
 * L > cap, cap < 1, first outside 0 .. cap - 1,
 * n outside 1 .. HRP_KIN_FILTER_MAX_N, dof outside 0 .. HRP_FK_MAX_JOINTS, nkp outside 1 .. HRP_FK_MAX_KP, a free_q bit at or above dof,
 * root outside 0 .. nkp - 1, rot_dim not 3 or 6, free_pose not 0 or 1. */
enum { HRP_KS_SMOOTHED = 1, HRP_KS_TAIL = 2, HRP_KS_INVALID = 4, HRP_KS_BAD_LINK = 8, HRP_KS_CLAMPED = 16 };
typedef struct hrp_kin_history_desc {
  const double *mean, *cov;               /* the filter's state after the step: [B,2n], [B,2n,2n] */
  const int32_t *valid, *status;          /* [B]; the step's status [B,4] */
  const float* q_in;                      /* [B,dof] the step's q_in */
  double *h_mean, *h_cov;                 /* the ring */
  int32_t *h_valid, *h_flags;
  double* h_dt;
  float* h_q_in;
  int32_t B, n, dof, cap, slot, reserved;
  double dt;
} hrp_kin_history_desc;
int hrp_kin_history_push(const hrp_kin_history_desc* d, void* stream);

typedef struct hrp_kin_smooth_desc {
  const hrp_fk_chain* chain;              /* device */
  const double *mean, *cov;               /* the ring: [cap,B,2n], [cap,B,2n,2n] */
  const int32_t *valid, *flags;           /* [cap,B] */
  const double* dt;                       /* [cap] */
  const float* q_in;                      /* [cap,B,dof] */
  const float *rot_fixed, *trans_fixed;   /* [rot_dim], [3]: the pose of every frame when free_pose == 0 */
  const float *q_lo, *q_hi;               /* [dof] each, optional */
  const double* q_acc;                    /* [n] */
  double* gain; int32_t* link;            /* scratch [L,B,2n,2n], [L,B] */
  uint32_t free_q; int32_t free_pose, root, B, dof, nkp, rot_dim, cap, first, L, want_cov, reserved;
  float *q, *rot, *trans, *vel, *cov_p, *xyz;        /* [L,B,dof], [L,B,rot_dim], [L,B,3], [L,B,n], [L,B,n,n], [L,B,nkp,3] */
  int32_t* status;                        /* [L,B,2] */
  double *mean_s, *cov_s;                 /* optional [L,B,2n], [L,B,2n,2n] */
} hrp_kin_smooth_desc;
int hrp_kin_smooth(const hrp_kin_smooth_desc* d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HRP_H */
