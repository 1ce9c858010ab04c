/*
 * fnn.h - C ABI of the MI355X-native sliding-window 3D-U-Net inference engine.
 *
 * This is the drop-in boundary for the hot path of 77even/Fast-nnUNet.  The
 * reference has no native plugin interface for this path: the
 * boundary in the reference is the Python method
 *   nnUNetPredictor.predict_sliding_window_return_logits
 *     (distillation/nnunetv2/inference/predict_from_raw_data.py:634-680)
 * and the functions it drives.  Each entry point below names the reference
 * code it replaces.  Plain pointers and sizes only; no torch types.
 *
 * Conventions
 *   - every function returns 0 on success, a negative FNN_E_* code otherwise;
 *     fnn_last_error() gives the message (thread-local for fnn_create failures,
 *     per engine afterwards);
 *   - volumes / logits are channel-first contiguous [C, X, Y, Z], exactly the
 *     tensors the reference passes; pointers may be device (HIP) or host
 *     pointers, the engine detects which;
 *   - the engine never frees or mutates caller memory; outputs are
 *     caller-allocated;
 *   - one engine = one GPU; not re-entrant per engine (like the reference's
 *     predictor, which swaps fold weights in place, :486-489).
 */
#ifndef FNN_H
#define FNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FNN_MAX_STAGES 8
#define FNN_ABI_VERSION 4

enum {
    FNN_OK = 0,
    FNN_E_INVALID = -1,      /* bad argument (maps to AssertionError / ValueError)            */
    FNN_E_HIP = -2,          /* HIP runtime failure (maps to RuntimeError)                    */
    FNN_E_INF = -3,          /* 'Encountered inf in predicted array' (:622-625)               */
    FNN_E_UNSUPPORTED = -4,  /* topology the engine does not implement                        */
    FNN_E_STATE = -5         /* weights / gaussian not loaded                                 */
};

enum { FNN_NET_PLAIN = 0, FNN_NET_RESENC = 1 };
/* fnn_arch_desc.precision - the operand format of the matrix cores in the 3x3x3 stride-1 convolutions
 * (BASELINE config 5 asks for an fp8 conv path; the reference has no fp8 semantics):
 *   FNN_PREC_F16  fp16 operands everywhere (default; every parity statement in DESIGN.md is for this mode);
 *   FNN_PREC_F8   OCP e4m3 operands in those convolutions: weights quantised per output channel when they are
 *                 loaded, activations while they are staged (after InstanceNorm + LeakyReLU, x 8); fp32
 *                 accumulation; everything else (storage, statistics, strided / 1x1x1 / transposed convs, seg
 *                 head, accumulation) as in fp16.  Budget against the fp32 oracle: DESIGN.md, "fp8". */
enum { FNN_PREC_F16 = 0, FNN_PREC_F8 = 1 };
/* fnn_opts.accum - the arithmetic of the Gaussian-weighted accumulation (predict_from_raw_data.py:602-621):
 *   FNN_ACC_FP16_REFERENCE  the reference WITHOUT autocast (its CPU path, :591-593 `dummy_context`): the network's
 *                           logits are fp32, `prediction *= gaussian` is an fp32 product, `predicted_logits += prediction`
 *                           an fp32 sum rounded once to the fp16 accumulator.  Pinned by tests/golden/sliding_window.npz.
 *   FNN_ACC_FP32            fp32 accumulators (what the reference's error message recommends when fp16 overflows).
 *   FNN_ACC_FP16_AUTOCAST   the reference ON A GPU (`torch.autocast`: the network's output is fp16): the logit, every
 *                           mirror sum, the division by the number of evaluations, the product with the Gaussian and
 *                           the sum are each rounded to fp16.  Pinned by tests/golden/sliding_window_half.npz (made by
 *                           the reference's own predictor through networks that return fp16).  Served by the gather
 *                           path only (any number of classes: passes of 63 heads; FNN_E_UNSUPPORTED where that path
 *                           cannot run - a last stage of more than 32 channels, fp32 output - and for the
 *                           accumulate_* entry points). */
enum { FNN_ACC_FP16_REFERENCE = 0, FNN_ACC_FP32 = 1, FNN_ACC_FP16_AUTOCAST = 2 };
enum { FNN_OUT_F16 = 0, FNN_OUT_F32 = 1 };

/* Network topology: what the reference builds from plans.json + checkpoint
 * (PlainConvUNet / LiteNNUNetStudent: nnUNetDistillationTrainer.py:74-177,
 *  get_network_from_plans.py:9-43).  Features are already reduced for a student. */
typedef struct fnn_arch_desc {
    int32_t kind;                               /* FNN_NET_*                                  */
    int32_t n_stages;
    int32_t in_channels;
    int32_t num_heads;                          /* LabelManager.num_segmentation_heads        */
    int32_t features[FNN_MAX_STAGES];
    int32_t kernels[FNN_MAX_STAGES][3];         /* per-axis 1 or 3                            */
    int32_t strides[FNN_MAX_STAGES][3];         /* per-axis 1 or 2; stage 0 must be 1,1,1     */
    int32_t n_conv_enc[FNN_MAX_STAGES];         /* convs (plain) / residual blocks (resenc)   */
    int32_t n_conv_dec[FNN_MAX_STAGES];
    int32_t patch[3];                           /* ConfigurationManager.patch_size            */
    float eps;                                  /* InstanceNorm eps (1e-5)                    */
    float slope;                                /* LeakyReLU negative slope (0.01)            */
    int32_t spatial_dims;                       /* 0 or 3: 3-D configuration.  2: a `2d` configuration
                                                 * (Conv2d network, patch_size with two entries): patch[0],
                                                 * kernels[s][0] and strides[s][0] are 1 and EVERY slice of
                                                 * the first image axis is a tile position
                                                 * (predict_from_raw_data.py:508-524)               */
    int32_t precision;                          /* FNN_PREC_*                                  */
} fnn_arch_desc;

/* Knobs of nnUNetPredictor.__init__ (:40-65) + engine-side choices. */
typedef struct fnn_opts {
    double tile_step_size;                      /* 0 < s <= 1; a double like the reference's Python float:
                                                 * ceil((image - patch) / (patch * step)) of a float-rounded
                                                 * 0.3 or 0.7 gives another patch count (sliding_window_prediction.py:38-41) */
    int32_t use_gaussian;
    int32_t n_mirror_axes;                      /* 0 = no test-time mirroring                 */
    int32_t mirror_axes[3];                     /* spatial axes 0..2                          */
    int32_t accum;                              /* FNN_ACC_*                                  */
    int32_t out_dtype;                          /* FNN_OUT_*                                  */
    int32_t batch;                              /* patches per forward, <= max_batch          */
    void *stream;                               /* hipStream_t; NULL = the null stream        */
} fnn_opts;

typedef struct fnn_engine fnn_engine;

/* ---- lifecycle ----------------------------------------------------------- */
int fnn_abi_version(void);
const char *fnn_last_error(const fnn_engine *e);             /* e may be NULL */

/* Replaces network construction in initialize_from_trained_model_folder
 * (:104-118) / manual_initialization (:131-154).  max_batch: patches per forward the engine is planned for (the kernel
 * variants are chosen for it): 1 .. 64, or - small patches - as many as give a forward 2^27 voxels, at most 512. */
int fnn_create(const fnn_arch_desc *arch, int device, int max_batch, fnn_engine **out);
void fnn_destroy(fnn_engine *e);

/* Number of float32 values fnn_load_weights expects and the canonical order.
 * FNN_NET_PLAIN: for every encoder stage s, conv i: weight[F,Cin,kd,kh,kw], bias[F], gamma[F],
 * beta[F]; then for every decoder level d (deepest first): transpconv
 * weight[Cbelow,F,sd,sh,sw], bias[F]; its convs as above; finally the last
 * seg layer weight[heads,F0], bias[heads].
 * FNN_NET_RESENC (ResidualEncoderUNet, n_conv_enc = residual blocks per stage): the
 * stem conv (weight, bias, gamma, beta); then per stage, per block: conv1
 * (weight, bias, gamma, beta), conv2 (same), and - only when the block changes
 * the channel count - the 1x1x1 skip projection (weight[F,Cin], gamma, beta; it
 * has no bias); decoder and seg layer as above. */
int64_t fnn_weight_count(const fnn_engine *e);

/* Replaces network.load_state_dict(params) per fold (:486-489).  `blob` is
 * host memory in the order above.  Folds are kept resident on the device. */
int fnn_load_weights(fnn_engine *e, int fold, const float *blob, int64_t count);

/* The fp16 importance map of compute_gaussian (sliding_window_prediction.py:10-27),
 * patch[0]*patch[1]*patch[2] IEEE-half bit patterns, computed by the host
 * mirror with scipy exactly as the reference does. */
int fnn_set_gaussian(fnn_engine *e, const uint16_t *half_bits, int64_t count);

/* ---- the hot path -------------------------------------------------------- */
/* Replaces predict_sliding_window_return_logits (:634-680) for fold `fold`:
 * pad -> slicers -> per patch network (+mirroring) -> weighted accumulate ->
 * normalise -> un-pad.  vol: float32 [C,X,Y,Z]; out: [heads,X,Y,Z] of
 * opts->out_dtype.  FNN_E_INF if the normalised logits contain inf.
 * vol may be DEVICE memory (read in place) or HOST memory - what the reference's callers hold
 * (`data = data.to(results_device)`, :579): a host volume is uploaded in tiles (planes x rows) on a copy stream of the
 * engine's and a batch of patches starts when the tiles under its patches have landed (the patch order is
 * x-major, :532-537); pinned host memory is read by DMA directly, pageable memory through pinned staging. */
int fnn_predict_volume(fnn_engine *e, int fold, const float *vol, const int64_t shape[4],
                       const fnn_opts *opts, void *out_logits);

/* Replaces predict_logits_from_preprocessed_data (:471-504): mean over the
 * loaded folds [0, n_folds) - summed on the device instead of the reference's
 * per-fold device->host hop (:494-497). */
int fnn_predict_volume_ensemble(fnn_engine *e, int n_folds, const float *vol, const int64_t shape[4],
                                const fnn_opts *opts, void *out_logits);

/* One forward of the network on `n` patches (the `self.network(x)` call at
 * :545): x float32 [n,C,px,py,pz] -> logits float32 [n,heads,px,py,pz].
 * Used by parity tests and by callers that bring their own tiling. */
int fnn_forward_patches(fnn_engine *e, int fold, const float *x, int n, float *logits, void *stream);

/* How the label-map entry points turn logits into labels (engine state, default
 * ARGMAX / U8) - LabelManager.convert_logits_to_segmentation, label_handling.py:144-195:
 *   FNN_LABELS_ARGMAX  plain labels: argmax over heads, first maximum wins (:176-180);
 *   FNN_LABELS_REGIONS region-based training: label = 0, then for i in order
 *                      `if sigmoid(float(logit_i)) > 0.5: label = regions_class_order[i]`
 *                      (:163-170; n_regions must equal num_heads).
 * label_dtype follows export_prediction.py:45-46: uint8 when the dataset has
 * < 255 foreground labels, else uint16. */
enum { FNN_LABELS_ARGMAX = 0, FNN_LABELS_REGIONS = 1 };
enum { FNN_LABEL_U8 = 0, FNN_LABEL_U16 = 1 };
int fnn_set_label_rule(fnn_engine *e, int mode, const int32_t *regions_class_order, int n_regions, int label_dtype);

/* Label map without materialising the logits: for one fold the labels are taken
 * straight from the accumulators (divide, round to fp16, then the label rule -
 * exactly what convert_logits_to_segmentation would see); for several folds the
 * ensemble logits are formed first.  Replaces the reference's full-logit D2H
 * copy + numpy argmax (:386, label_handling.py:173-180).  labels: uint8 or
 * uint16 [X,Y,Z] per fnn_set_label_rule. */
int fnn_predict_labels(fnn_engine *e, int n_folds, const float *vol, const int64_t shape[4],
                       const fnn_opts *opts, void *labels);

/* Multi-GPU building blocks (not in the reference, whose only
 * inference parallelism is case-level -num_parts/-part_id, :918-925).
 * Accumulators are channels-last DEVICE buffers - fp32 when opts->accum is
 * FNN_ACC_FP32, fp16 otherwise - that cover a box of the
 * PADDED volume:  acc[bx][by][bz][HP],  HP = fnn_accumulator_channels(e)
 * (= num_heads + 1 rounded up to 8); channel h < num_heads holds sum(w * logit_h),
 * channel num_heads holds sum(w).  The caller zeroes them, exchanges / adds the
 * overlap regions between ranks, then normalises the part it owns.
 * fnn_accumulate_patches runs the listed patches (indices into the x-major patch
 * list of fnn_plan_volume; each must lie inside the box) and ADDS into acc.
 * fnn_normalize_box divides, un-pads and writes the un-padded box
 * [out_lo, out_hi) into `out`, the full [heads][X][Y][Z] tensor of opts->out_dtype. */
int64_t fnn_accumulator_channels(const fnn_engine *e);
int fnn_accumulate_patches(fnn_engine *e, int fold, const float *vol, const int64_t shape[4],
                           const fnn_opts *opts, const int64_t *patch_ids, int64_t n_ids,
                           const int64_t box_lo[3], const int64_t box_hi[3], void *acc);
int fnn_normalize_box(fnn_engine *e, const void *acc, const int64_t shape[4], const fnn_opts *opts,
                      const int64_t box_lo[3], const int64_t box_hi[3],
                      const int64_t out_lo[3], const int64_t out_hi[3], void *out_logits);

/* fnn_normalize_box's label-map twin: divide, round to fp16, apply the engine's label rule
 * (fnn_set_label_rule) and write the un-padded box [out_lo, out_hi) into `labels`, the full
 * [X][Y][Z] uint8 / uint16 map - what convert_logits_to_segmentation (label_handling.py:144-195)
 * would produce from that box's logits.  A rank of the sharded predictor labels the box it owns
 * and only the label slabs (not the logits) travel between the GPUs. */
int fnn_labels_box(fnn_engine *e, const void *acc, const int64_t shape[4], const fnn_opts *opts,
                   const int64_t box_lo[3], const int64_t box_hi[3],
                   const int64_t out_lo[3], const int64_t out_hi[3], void *labels);

/* The same sharding on the gather path (csrc/gather.hip; no accumulators, bit-identical to one GPU): a rank keeps the
 * last activation of the patches it ran - fnn_patch_features writes them, [n_ids][P][C] fp16 with P = patch voxels and
 * C = fnn_feature_channels(e), and their InstanceNorm rows [n_ids][2][C] float32, into DEVICE buffers of the caller -
 * receives from its neighbours the parts of THEIR patches that reach into the box it owns (caller's job: plain copies
 * of [dx][dy][dz][C] sub-blocks), and fnn_gather_box then forms every voxel of the un-padded box [out_lo, out_hi) from
 * all patches that cover it, in the reference's visiting order: slot_of_patch[pid] (HOST array over the x-major patch
 * list of fnn_plan_volume) = where patch pid's activation sits in feat / fss, or -1 where the caller knows the patch
 * does not reach the box.  Writes fp16 logits [heads][X][Y][Z] and / or labels [X][Y][Z] (either may be NULL) of the
 * full-size tensors.
 * Slots and mirroring (ABI 3): the caller's buffers hold `n_slots` patch slots per evaluation - feat
 * [n_eval][n_slots][P][C], fss [n_eval][n_slots][2][C], n_eval = 2^(opts->n_mirror_axes) in the order of
 * _internal_maybe_mirror_and_predict (predict_from_raw_data.py:541-557; 1 without mirroring); fnn_patch_features
 * writes patch patch_ids[i] into slot slot0 + i of every evaluation.  The activation of a mirrored evaluation is
 * stored in the network's (flipped) coordinates: voxel v of the patch sits at P - 1 - v along every flipped axis, which
 * is where a caller that moves sub-blocks between ranks has to put them (fast-nnunet_amd/dist.py, FeatureExchange). */
int64_t fnn_feature_channels(const fnn_engine *e);
int fnn_patch_features(fnn_engine *e, int fold, const float *vol, const int64_t shape[4], const fnn_opts *opts,
                       const int64_t *patch_ids, int64_t n_ids, void *feat, float *fss, int64_t slot0, int64_t n_slots);
int fnn_gather_box(fnn_engine *e, int fold, const void *feat, const float *fss, const int32_t *slot_of_patch,
                   int64_t n_slots, const int64_t shape[4], const fnn_opts *opts, const int64_t out_lo[3],
                   const int64_t out_hi[3], void *out_logits, void *labels);

/* The exchange between fnn_patch_features and fnn_gather_box as ONE launch per peer and direction (ABI 4; not in the
 * reference, whose only inference parallelism is case level: predict_from_raw_data.py:918-925).  A rank
 * sends each neighbour the sub-blocks of its kept activations that reach into the neighbour's owned box:
 * fnn_pack_regions copies `n` sub-blocks of feat ([n_eval][n_slots][PD][PH][PW][C] fp16, C = fnn_feature_channels) into
 * one contiguous message buffer, fnn_unpack_regions lands a received message in the slots of the foreign patches.
 * `regions`: a DEVICE table (built once per decomposition, it does not change from volume to volume of one shape) of
 * fnn_region records - evaluation, slot, the sub-block [lo, hi) in the slot's own (stored, i.e. flipped for a mirrored
 * evaluation) voxel coordinates, and where the block sits in the message in units of 16 bytes; blocks are [d][h][w][C]
 * contiguous.  Both run on `stream` without synchronising it; every pointer is device memory. */
typedef struct fnn_region {
    int32_t eval, slot;
    int32_t lo[3], hi[3];
    int32_t off16;                  /* block start in the message buffer, 16-byte units */
    int32_t reserved;
} fnn_region;
int fnn_pack_regions(fnn_engine *e, const void *feat, int64_t n_slots, const fnn_region *regions, int64_t n,
                     void *message, void *stream);
int fnn_unpack_regions(fnn_engine *e, void *feat, int64_t n_slots, const fnn_region *regions, int64_t n,
                       const void *message, void *stream);

/* LabelManager.convert_logits_to_segmentation on resident logits with the
 * engine's label rule: logits [heads, n_vox] f16/f32 -> labels uint8/uint16. */
int fnn_argmax_labels(fnn_engine *e, const void *logits, int dtype, int heads, int64_t n_vox,
                      void *labels, void *stream);

/* ---- whole-volume steps around the sliding window ----
 * DefaultPreprocessor.run_case_npy WITHOUT its resampling call
 * (preprocessing/preprocessors/default_preprocessor.py:45-93): float32 image
 * [C][s0][s1][s2] -> transpose_forward -> crop to the bounding box of the non-zero
 * region (preprocessing/cropping/cropping.py:7-39) -> per-channel intensity
 * normalisation (preprocessing/normalization/default_normalization_schemes.py).
 * Device pointers only.  Resampling to the target spacing is fnn_resample. */
enum { FNN_NORM_NONE = 0,        /* NoNormalization                                   :70-74 */
       FNN_NORM_ZSCORE = 1,      /* ZScoreNormalization, whole-image branch            :45-49 */
       FNN_NORM_CT = 2,          /* CTNormalization: clip, - mean, / max(std, 1e-8)    :53-67 */
       FNN_NORM_RESCALE01 = 3,   /* RescaleTo01Normalization                           :77-84 */
       FNN_NORM_RGB01 = 4 };     /* RGBTo01Normalization                               :87-98 */
typedef struct fnn_norm_desc {
    int32_t scheme;              /* FNN_NORM_*                                                 */
    float mean, std;             /* CT: intensityproperties['mean'], ['std']                   */
    float lower, upper;          /* CT: ['percentile_00_5'], ['percentile_99_5']               */
    int32_t use_mask;            /* ZScore: use_mask_for_norm - statistics and normalisation only inside
                                  * binary_fill_holes(non-zero mask) (cropping.py:7-39, schemes :36-44)   */
} fnn_norm_desc;

/* bbox[2a], bbox[2a+1] = [lo, hi) along TRANSPOSED axis a of the voxels where any
 * channel is non-zero (the full extent for an all-zero image): properties
 * ['bbox_used_for_cropping'] of the reference. */
int fnn_nonzero_bbox(const float *raw, const int64_t shape[4], const int32_t transpose_forward[3],
                     int64_t bbox[6], void *stream);
/* out: float32 [C][bbox extents] = normalise(crop(transpose(raw))); norm[C].
 * ZScore: mean and std from float64 sums in two passes, each rounded to float32 once.  NaN and inf go where numpy sends
 * them: a NaN voxel makes a RescaleTo01 or ZScore channel NaN throughout, an inf voxel a ZScore channel (its std is NaN,
 * and max(NaN, 1e-8) is NaN).  use_mask: the filled mask is found by sweeps repeated until nothing changes. */
int fnn_preprocess(const float *raw, const int64_t shape[4], const int32_t transpose_forward[3],
                   const int64_t bbox[6], const fnn_norm_desc *norm, float *out, void *stream);
/* The label half of convert_predicted_logits_to_segmentation_with_correct_shape
 * (inference/export_prediction.py:43-53): seg [bbox extents] (FNN_LABEL_U8 / U16)
 * -> zeros of shape_before_cropping with seg inserted at bbox -> transpose_backward.
 * out: [shape_before_cropping[transpose_backward[j]] for j in 0..2]. */
int fnn_revert_labels(const void *seg, int label_dtype, const int64_t bbox[6],
                      const int64_t shape_before_cropping[3], const int32_t transpose_backward[3],
                      void *out, void *stream);

/* convert_predicted_logits_to_segmentation_with_correct_shape(..., return_probabilities=True)
 * after its resampling step (inference/export_prediction.py:36-70): logits [heads][bbox
 * extents] (FNN_OUT_F16 / FNN_OUT_F32) -> apply_inference_nonlin (fp32 softmax over the heads;
 * sigmoid when regions_class_order != NULL, label_handling.py:125-139), the label rule on the
 * probabilities (:163-181), revert_cropping_on_probabilities (:197-221: background probability
 * 1 outside the box for plain labels, 0 for regions), both transposes back.
 * probs: float32 [heads][shape_before_cropping[transpose_backward[j]]]; labels: the same grid. */
int fnn_export_probabilities(const void *logits, int logits_dtype, int heads,
                             const int32_t *regions_class_order, const int64_t bbox[6],
                             const int64_t shape_before_cropping[3], const int32_t transpose_backward[3],
                             float *probs, void *labels, int label_dtype, void *stream);

/* resample_data_or_seg(..., is_seg=False) of the reference
 * (preprocessing/resampling/default_resampling.py:113-196): per channel
 * skimage.transform.resize(order, mode='edge', anti_aliasing=False) - evaluated as
 * scipy.ndimage.zoom(float64, out/in, order, mode='nearest', grid_mode=True) + clip
 * to the input range - or, with separate_axis >= 0, that resize per 2-D slice and
 * an order-0 pass along the axis (:147-188).  in / out: [C][...] of `dtype`
 * (FNN_OUT_F32 for images, FNN_OUT_F16 for fp16 logits), device pointers.
 * The caller decides separate_axis (determine_do_sep_z_and_axis, :34-71). */
typedef struct fnn_resample_desc {
    int32_t order;               /* 0, 1 or 3 (resampling_fn_*_kwargs['order'])               */
    int32_t separate_axis;       /* -1, or the anisotropic axis                                */
    int32_t order_z;             /* 0 (the only value the reference's plans use)               */
    int32_t dtype;               /* FNN_OUT_F16 / FNN_OUT_F32                                  */
} fnn_resample_desc;
int fnn_resample(const void *in, const int64_t shape[4], const int64_t new_shape[3],
                 const fnn_resample_desc *desc, void *out, void *stream);

/* resample_torch_fornnunet of the reference (preprocessing/resampling/resample_torch.py:96-154; additive in ABI 4), the
 * resampling family its `resample_with_torch` planners write into plans.json: per channel
 * torch.nn.functional.interpolate(x.float(), new_shape, mode='trilinear', antialias=False) - align_corners=False, all
 * float32 - or, with separate_axis >= 0, bilinear in the plane and the 'nearest-exact' slice along the axis.  (The
 * reference's own separate-z branch raises a TypeError before it computes anything; this is what the branch states.)
 * One fused pass, no scratch memory, asynchronous on `stream`.  in / out: [C][...] of `dtype` (fp16 input is widened
 * exactly, fp16 output is the float32 result rounded once), device pointers.  An axis with in == out is the identity.
 * fnn_resample_torch_seg: int16 labels -> int16 labels by resample_torch_simple(is_seg=True) (:51-85): the label whose
 * (seg == u) * 1000 interpolated and rounded to fp16 is largest, the smallest label on ties; with `memefficient` the
 * label whose float32 interpolated (seg == u) exceeds 0.5, else 0.  `dtype` is ignored.
 * FNN_E_UNSUPPORTED for a mode other than linear / an aniso_axis_mode other than nearest-exact. */
enum { FNN_INTERP_LINEAR = 0, FNN_INTERP_NEAREST_EXACT = 1, FNN_INTERP_OTHER = 2 };
typedef struct fnn_resample_torch_desc {
    int32_t dtype;               /* FNN_OUT_F16 / FNN_OUT_F32                                  */
    int32_t separate_axis;       /* -1, or the anisotropic axis                                */
    int32_t memefficient;        /* segmentations: memefficient_seg_resampling                 */
    int32_t mode;                /* FNN_INTERP_LINEAR (kwargs['mode'] = 'linear')              */
    int32_t aniso_axis_mode;     /* FNN_INTERP_NEAREST_EXACT (kwargs['aniso_axis_mode'])       */
} fnn_resample_torch_desc;
int fnn_resample_torch(const void *in, const int64_t shape[4], const int64_t new_shape[3],
                       const fnn_resample_torch_desc *desc, void *out, void *stream);
int fnn_resample_torch_seg(const int16_t *in, const int64_t shape[4], const int64_t new_shape[3],
                           const fnn_resample_torch_desc *desc, int16_t *out, void *stream);

/* resample + label rule in one pass (additive in ABI 4): logits [heads][in] (FNN_OUT_F16 / FNN_OUT_F32) on the network
 * grid -> labels [new_shape] (FNN_LABEL_U8 / U16), bit for bit the labels of fnn_resample (order 1, order_z 0) or
 * fnn_resample_torch followed by fnn_argmax_labels - without the resampled tensor [heads][new_shape] in between.
 * family: FNN_RESAMPLE_DEFAULT (resample_data_or_seg_to_shape, order 1, order_z 0) or FNN_RESAMPLE_TORCH
 * (resample_torch_fornnunet, linear / nearest-exact).  separate_axis -1 or 0..2.  regions_class_order NULL = argmax
 * rule (first maximum, first NaN); else n_regions = heads entries IN DEVICE MEMORY, the region rule painted in that
 * order.  Any number of heads.  Device pointers, one launch, no allocation, no synchronisation. */
enum { FNN_RESAMPLE_DEFAULT = 0, FNN_RESAMPLE_TORCH = 1 };
int fnn_resample_labels(const void *logits, int dtype, const int64_t shape[4], const int64_t new_shape[3],
                        int family, int separate_axis, const int32_t *regions_class_order, int n_regions,
                        void *labels, int label_dtype, void *stream);

/* remove_all_but_largest_component_from_segmentation (postprocessing/remove_connected_components.py:21-33) for
 * disjoint label sets at once (additive in ABI 4): labels [X][Y][Z] (FNN_LABEL_U8 / U16, device pointer) is changed in
 * place.  group_of_label[v] (host, n_table entries) is the set of label value v, or -1; labels >= n_table are in no
 * set.  Two 26-neighbours belong to one component iff their labels map to the same set.  Per set, every component
 * whose size equals the set's largest is kept (ties keep all of them); every other voxel of the set becomes
 * background_label.  removed (optional host [n_groups]) receives the voxels changed per set.  A zero-size volume
 * returns 0; more than 2^31 - 1 voxels give FNN_E_UNSUPPORTED.  Scratch: 8 B per voxel, allocated inside the call. */
int fnn_keep_largest_components(void *labels, int label_dtype, const int64_t shape[3],
                                const int32_t *group_of_label, int n_table, int n_groups,
                                int background_label, int64_t *removed, void *stream);

/* Small-region filtering for disjoint label sets at once (additive in ABI 4); the reference names the step in its inference
 * front end and ships no source for it, the definition is scipy's ndimage.label + bincount.  labels, label_dtype, shape,
 * group_of_label, n_table, n_groups, background_label, removed, the limits and the scratch: as
 * fnn_keep_largest_components.  connectivity: 26 (a voxel's full neighbourhood, scipy's generate_binary_structure(3, 3)) or
 * 6 (face neighbours, (3, 1)); any other value is FNN_E_UNSUPPORTED before any launch.  Two neighbours belong to one component
 * iff their labels map to the same set.  min_size (host, n_groups entries): every component of set g with fewer than
 * min_size[g] voxels becomes background_label, one of exactly min_size[g] is kept; min_size[g] <= 1 changes nothing for that
 * set.  All sets are labelled in one pass. */
int fnn_remove_small_components(void *labels, int label_dtype, const int64_t shape[3],
                                const int32_t *group_of_label, int n_table, int n_groups,
                                int background_label, const int64_t *min_size, int connectivity,
                                int64_t *removed, void *stream);

/* Hole filling for one label set S (additive in ABI 4); no source in the reference either, the definition is scipy's:
 * holes = ndimage.binary_fill_holes(in_S) & ~in_S with the default (cross) structure.  labels [X][Y][Z] (FNN_LABEL_U8 / U16,
 * device pointer) is changed in place.  group_of_label[v] (host, n_table entries) is 0 where label value v belongs to S and
 * -1 where not; labels >= n_table are outside S.  A hole is a 6-connected component of the complement of S that reaches no
 * face of the volume along an axis of border_axes (bit a set: the two faces of axis a are borders; 1..7).  Hole voxels whose
 * value equals background_label become fill_label; another label inside a hole stays.  A 3-D map passes border_axes 7; a 2-D
 * map is the volume [1][Y][Z] with border_axes 6 (with bit 0 set every voxel of it lies on a border and nothing is filled,
 * as scipy does for an array of shape (1, Y, Z)).  filled (optional, host) receives the number of voxels changed.
 * FNN_E_INVALID before any launch: a label outside the dtype, fill_label equal to background_label, border_axes outside
 * 1..7, a table entry outside [-1, 0]; sizes as fnn_keep_largest_components.  Launches: one pass for the bounding box of S,
 * read by the host (an empty S, or S filling its box, ends the call there); then the complement is labelled inside the box
 * only.  Scratch, allocated inside the call: 8 B per voxel of the box.  Synchronises the stream. */
int fnn_fill_holes(void *labels, int label_dtype, const int64_t shape[3], const int32_t *group_of_label, int n_table,
                   int background_label, int fill_label, int border_axes, int64_t *filled, void *stream);

/* Binary morphology of one label set S (additive in ABI 4): the last of the "morphological operations" the reference's
 * inference front end names without source; the definition is scipy's.  With M = in_S, R is ndimage.binary_dilation,
 * binary_erosion, binary_opening or binary_closing of M (op) with structure = generate_binary_structure(ndim, rank),
 * iterations = iterations, border_value = border_value and every other argument at its default.  connectivity 6, 18 or 26 is
 * rank 1, 2 or 3 (on a 2-D map 18 and 26 both give the full 3 x 3, 6 the cross).  iterations: 1..1024 (scipy's "below 1: until
 * nothing changes" is refused).  The label rule:
 *   - dilation and closing only add: voxels of R & ~M whose value equals background_label become fill_label, any other
 *     label there stays, no voxel of M changes (with border_value 0 scipy's closing loses voxels of M at the volume's border:
 *     they stay);
 *   - erosion and opening only remove: voxels of M & ~R become background_label, no voxel outside M changes (with
 *     border_value 1 scipy's opening gains voxels at the border: they are not added); fill_label is not read.
 * labels, label_dtype, shape, group_of_label (0 = in S, -1 = not), n_table and the size limits: as fnn_fill_holes.  axes is a
 * bit mask of the axes the structure spans (bit 0 x, 1 y, 2 z): 7 for a 3-D map, 6 for a 2-D map carried as [1][Y][Z]; with 7
 * on [1][Y][Z] the x-neighbours lie outside the map and count as border_value, as scipy does for a (1, Y, Z) array.  changed
 * (optional, host) receives the number of voxels written.  FNN_E_INVALID before any launch and before any device memory is
 * asked for: op outside 0..3, connectivity not 6 / 18 / 26, iterations outside 1..1024, border_value not 0 / 1, a label outside
 * the dtype, fill_label equal to background_label for an adding op, axes outside 1..7, a table entry outside [-1, 0].  A
 * zero-size volume returns 0; more than 2^31 - 1 voxels give FNN_E_UNSUPPORTED.  Launches: with border_value 0 the box pass of
 * fnn_fill_holes, read by the host (an empty S ends the call), and the work stays inside S's box (grown by iterations for the
 * adding ops); the mask is packed to bit planes, every iteration is one launch on them, one pass applies the label rule.
 * Scratch, allocated inside the call: 2 bits per voxel of the box.  Synchronises the stream. */
enum { FNN_MORPH_DILATE = 0, FNN_MORPH_ERODE = 1, FNN_MORPH_OPEN = 2, FNN_MORPH_CLOSE = 3 };
int fnn_binary_morphology(void *labels, int label_dtype, const int64_t shape[3], const int32_t *group_of_label, int n_table,
                          int op, int connectivity, int iterations, int border_value, int background_label, int fill_label,
                          int axes, int64_t *changed, void *stream);

/* Cross-configuration ensembling (additive in ABI 4): average_probabilities + merge_files without the image writer
 * (ensembling/ensemble.py:16-44), in one pass from the members' logits.  member_logits[m] (device, host array of
 * n_members pointers, 1..16) are [heads][bbox extents] of dtype member_dtype[m] (FNN_OUT_F16 / FNN_OUT_F32; members may
 * differ), the resampled logits fnn_export_probabilities takes.  Member m's probabilities are bit for bit what
 * fnn_export_probabilities writes for it; the average is p_0 += p_1 ... in member order, then / (float)n_members
 * (numpy's float32 average_probabilities, bit for bit).  The label rule is convert_logits_to_segmentation of the
 * average (label_handling.py:183-195): argmax, first maximum wins; for regions sigmoid(average) > 0.5 painted in
 * regions_class_order - the reference applies the sigmoid a second time, and so does this.
 * avg_probs (nullable): float32 [heads][shape_before_cropping[transpose_backward[j]]]; labels: the same grid
 * (FNN_LABEL_U8 / U16).  Synchronises the stream. */
int fnn_ensemble_export(const void *const *member_logits, const int32_t *member_dtype, int n_members, int heads,
                        const int32_t *regions_class_order, const int64_t bbox[6], const int64_t shape_before_cropping[3],
                        const int32_t transpose_backward[3], float *avg_probs, void *labels, int label_dtype, void *stream);
/* The .npz route (additive in ABI 4): the same average and label rule on member_probs[m], float32 [heads][n_vox] device
 * buffers on the raw grid.  avg_probs (nullable): float32 [heads][n_vox]; labels [n_vox]. */
int fnn_average_probabilities(const float *const *member_probs, int n_members, int heads,
                              const int32_t *regions_class_order, int64_t n_vox, float *avg_probs, void *labels,
                              int label_dtype, void *stream);
/* fnn_ensemble_export straight from the members' network grids (additive in ABI 4): member m's logits are
 * [heads][shape] (device, transposed axes) and are resampled to the bbox extents inside the pass, each value formed
 * and rounded to the member's dtype exactly as fnn_resample (family FNN_RESAMPLE_DEFAULT: order 1, order_z 0, that
 * separate axis) or fnn_resample_torch (FNN_RESAMPLE_TORCH) would have stored it; a member whose shape equals the
 * extents is taken as it is, whatever its family.  avg_probs and labels are bit for bit those of the per-member
 * resampling calls followed by fnn_ensemble_export, without the resampled tensors.  1..16 members, any mix of dtypes,
 * families and grids; at most 640 heads (the running sums of a voxel live in LDS; more: FNN_E_UNSUPPORTED).
 * regions_class_order: host, heads entries, or NULL.  Allocates nothing proportional to the volume; synchronises the
 * stream. */
typedef struct fnn_ensemble_member {
    const void *logits;        /* device, [heads][shape[0]][shape[1]][shape[2]]: the member's network grid, transposed axes */
    int64_t shape[3];
    int32_t dtype;             /* FNN_OUT_F16 / FNN_OUT_F32 */
    int32_t family;            /* FNN_RESAMPLE_DEFAULT (order 1, order_z 0) / FNN_RESAMPLE_TORCH */
    int32_t separate_axis;     /* -1 or 0..2 */
} fnn_ensemble_member;
int fnn_ensemble_resample_export(const fnn_ensemble_member *members, int n_members, int heads,
                                 const int32_t *regions_class_order, const int64_t bbox[6],
                                 const int64_t shape_before_cropping[3], const int32_t transpose_backward[3],
                                 float *avg_probs, void *labels, int label_dtype, void *stream);

/* Confusion counts of a reference label map against 1..4 predicted maps of the same voxel count (additive in ABI 4), for
 * compute_tp_fp_fn_tn (evaluation/evaluate_predictions.py:76-85) of every label at once.  ref and pred[p] (device,
 * 16-byte aligned; pred a host array of n_pred pointers) hold n_vox labels of label_dtype (FNN_LABEL_U8 / U16).
 * class_of_value[v] (host, n_table entries) is the class index of label value v (0..n_classes-1, n_classes <= 255);
 * values >= n_table or mapped to -1 fall in class n_classes ("other").  Reference voxels whose value equals
 * ignore_value (-1: none) are not counted.  counts (host) receives int64 [n_pred][n_classes+1][n_classes+1], indexed
 * [pred map][reference class][predicted class].  Exact integers; n_vox is not limited to 2^31; zero voxels give all
 * zeros.  The (other, other) bin is derived from the number of counted voxels.  Synchronises the stream. */
int fnn_confusion_counts(const void *ref, const void *const *pred, int n_pred, int label_dtype, int64_t n_vox,
                         const int32_t *class_of_value, int n_table, int n_classes, int ignore_value,
                         int64_t *counts, void *stream);

/* Surface distances between a reference and a predicted label map (additive in ABI 4), for the boundary metrics HD, HD95,
 * ASSD and NSD of every label or region of a case; the reference has no such function, the definitions are medpy's.
 * ref, pred: device label maps [shape[0]][shape[1]][shape[2]] = (z, y, x) of label_dtype (FNN_LABEL_U8 / U16), aligned to
 * their element.  member (host, [n_regions][n_table]): member[r][v] != 0 - label value v belongs to region r; values >=
 * n_table belong to nothing; 1..1024 regions.  The mask of a region is the union of its values; its surface S is the mask
 * minus its erosion with the 6-neighbourhood, everything outside the volume counting as background.
 * fnn_surface_count: n_surface (host [n_regions][2]) receives |S(ref_r)| and |S(pred_r)|, boxes (host [n_regions][6]) the
 * [lo, hi) box of ref_r | pred_r per axis as lo_z, hi_z, lo_y, hi_y, lo_x, hi_x - all zero when both are empty.
 * fnn_surface_distances: sq_dist (device, 8-byte aligned, room for cap doubles) receives, region after region, for every
 * voxel a of S(pred_r) in raster order min over b in S(ref_r) of ((sz dz)^2 + (sy dy)^2) + (sx dx)^2 with spacing = (sz,
 * sy, sx) - float64, evaluated in that order, the minimum taken over the evaluated values - and then the same for every
 * voxel of S(ref_r) against S(pred_r).  A region with an empty side contributes nothing.  cap below the total
 * (sum of n_surface[r][0] + n_surface[r][1] over the regions with two non-empty sides) is FNN_E_INVALID and writes nothing.
 * Nothing is read outside the two maps, nothing is written outside sq_dist[0, total); the same input gives the same bytes.
 * Both synchronise the stream.  FNN_E_INVALID before any launch, with a message: NULL or host pointers, an unknown label
 * dtype, n_regions outside 1..1024, negative n_table, a negative extent, misaligned maps or sq_dist, a spacing that is not
 * finite and positive, a negative cap; FNN_E_UNSUPPORTED: more than 2^31 - 1 voxels.  A volume without voxels gives zeros.
 * Scratch, allocated inside the call: 16 B + 24 B per region and 8 B per table value and 64 regions; fnn_surface_distances
 * also 12 B per voxel of the largest region box (8 B for the transform's y-pass values and 4 B for its z-pass voxel counts:
 * the passes are out of place so that a line longer than the LDS tile can be walked in pieces) + 4 B per 1024 box voxels
 * for the compaction's scan. */
int fnn_surface_count(const void *ref, const void *pred, int label_dtype, const int64_t shape[3], const uint8_t *member,
                      int n_table, int n_regions, int64_t *n_surface, int64_t *boxes, void *stream);
int fnn_surface_distances(const void *ref, const void *pred, int label_dtype, const int64_t shape[3], const uint8_t *member,
                          int n_table, int n_regions, const double spacing[3], double *sq_dist, int64_t cap, void *stream);

/* The connected components of a reference and a predicted label map and their overlaps (additive in ABI 4), for the
 * lesion-wise metrics of every label or region of a case (detection F1, false-positive / false-negative lesion volume,
 * panoptic quality); the reference has no such function.  ref, pred: device label maps [shape[0]][shape[1]][shape[2]] of
 * label_dtype (FNN_LABEL_U8 / U16), aligned to their element.  group_of_label, n_table, n_groups: as
 * fnn_keep_largest_components - two 26-neighbours are one component iff their values map to the same set; 1..1024 sets;
 * everything outside the volume is background.  A piece is a 26-connected component of the joint map J[v] = g + 1 where
 * the values of both maps at v belong to set g, else 0; every piece lies in exactly one component of each map, so the
 * overlap of a (pred component, ref component) pair is the sum of its pieces.
 * n_out (host) always receives {ref components, pred components, pieces}.  records (device, 4-byte aligned, room for cap
 * records of three int32) is written only when cap >= n_out[0] + n_out[1] + n_out[2]; otherwise nothing is written and the
 * call still returns 0 - the caller compares and calls again.  In this order: the ref components, then the pred components,
 * each as (set, root, size), root being the linear index of the component's first voxel in raster order, ascending in root;
 * then the pieces as (root of their pred component, root of their ref component, size), ascending in the piece's own first
 * voxel.  No atomic output cursor: the same input gives the same bytes.  Synchronises the stream.
 * FNN_E_INVALID before any launch, with a message: NULL or host pointers for the maps or records, an unknown label dtype,
 * n_groups outside 1..1024, a negative n_table, a table entry outside -1 .. n_groups - 1, a negative extent, a misaligned
 * pointer, a negative cap, a NULL n_out; FNN_E_UNSUPPORTED: more than 2^31 - 1 voxels.  A volume without voxels gives zeros.
 * Scratch, allocated inside the call: 16 B per voxel (the parents of the three labellings and one size array they use in
 * turn) + 12 B per 1024 voxels (the compaction's scan) + 12 B + 4 B per table value. */
int fnn_instance_overlaps(const void *ref, const void *pred, int label_dtype, const int64_t shape[3],
                          const int32_t *group_of_label, int n_table, int n_groups, int32_t *records, int64_t cap,
                          int64_t n_out[3], void *stream);

/* The surface of every region of a label map as triangles (additive in ABI 4), for a coloured 3-D model of a
 * segmentation: what the reference's VTKModelGenerator is called for (its source is not part of the reference; the
 * definition below is this project's own).  seg: device label map [shape[0]][shape[1]][shape[2]] = (z, y, x) of label_dtype
 * (FNN_LABEL_U8 / U16), aligned to its element.  member, n_table, n_regions: as fnn_surface_count - 1..1024 regions, each a
 * set of label values; everything outside the volume belongs to no region.
 * Faces: every pair of 6-neighbours (v, n) with v in region r and n not in r (n may lie outside the volume) is one square
 * face on the voxel boundary between them.  The faces of a region are ordered by the raster index of v, and inside one v by
 * direction -z, +z, -y, +y, -x, +x.  Every face is two triangles.
 * Vertices: the corners (cz, cy, cx) of the (Z+1)(Y+1)(X+1) corner grid whose 8 surrounding voxels are neither all in r nor
 * all outside r, ordered by the raster index of the corner; every region has its own vertices, and the triangles index the
 * concatenation of all regions' vertices.  The index-space position of a corner is (x, y, z) = (cx - 0.5, cy - 0.5,
 * cz - 0.5) in float32.
 * Triangles: with q0 < q1 < q2 < q3 the face's corners in raster order, the face is (q0, q1, q3), (q0, q3, q2) for the
 * directions +z, -y, +x and (q0, q3, q1), (q0, q2, q3) for -z, +y, -x: (b - a) x (c - a) points out of the region when
 * (x, y, z) is a right-handed triple.  When the determinant of the affine's 3x3 part is negative, the second and third
 * index of every triangle are swapped, so that the same holds in world coordinates.
 * Smoothing: smoothing_pairs times a pass with f = 0.5 and a pass with f = -0.53 (Taubin).  Two vertices of r are
 * neighbours iff they are the ends of a lattice edge whose 4 surrounding voxels are neither all in r nor all outside r.
 * A pass computes p' = p + f * (m - p) for every vertex from the positions before the pass, m = (0 + the present
 * neighbours added in the order -x, +x, -y, +y, -z, +z) * float32(1 / their number); float32, every operation rounded
 * on its own.  Regions do not see each other.
 * World coordinates: row r of the point is ((A[r][0] * x + A[r][1] * y) + A[r][2] * z) + A[r][3] in float64, evaluated in
 * that order without fused multiply-adds and rounded once to float32; affine = A, 16 doubles in row-major order, host.
 * fnn_mesh_count: counts (host [n_regions][2]) receives the vertices and the faces of every region, boxes (host
 * [n_regions][6]) the [lo, hi) box of its voxels as lo_z, hi_z, lo_y, hi_y, lo_x, hi_x - all zero for an empty region.
 * fnn_mesh_emit writes region after region.  layout 0: points float32 [n][3], cells int32 [t][3], cell_region uint16 [t]
 * (the index of the triangle's region).  layout 1: the same values big-endian and cells as [t][4] with a leading 3 - the
 * payload of the POINTS and POLYGONS sections of a legacy-VTK binary file.  n is the sum of the vertices, t twice the sum
 * of the faces; cap_points counts points and cap_cells triangles, and a cap below n or t writes nothing and is
 * FNN_E_INVALID with the number needed in the message.  points: device, 4-byte aligned; cells: device, 4-byte (layout 0)
 * or 16-byte (layout 1) aligned; cell_region: device, 2-byte aligned.  Nothing is read outside the map, nothing is written
 * outside points[0, n), cells[0, t) and cell_region[0, t); no atomic cursor places anything: the same input gives the
 * same bytes.  Both synchronise the stream.
 * FNN_E_INVALID before any launch, with a message: NULL or host pointers, an unknown label dtype, n_regions outside
 * 1..1024, a negative n_table, a negative extent, an affine that is not finite, negative smoothing_pairs, a layout other
 * than 0 and 1, a negative cap, misaligned pointers; FNN_E_UNSUPPORTED: more than 2^31 - 1 voxels, vertices or triangles.
 * A volume without voxels and regions without voxels give zeros and launch nothing for them.
 * Scratch, allocated inside the call: 8 B + 24 B per region and 8 B per table value and 64 regions; per region with faces
 * 36 B + 8 B; 196 B per 1024 corners of the regions' boxes (one bit per corner, a 4-byte prefix per 64 corners and per
 * 1024 corners) + 4 B per 1024 voxels of the boxes (the faces' scan); fnn_mesh_emit also 12 B per vertex, and 48 B per
 * vertex when it smooths (two position buffers for the Jacobi passes and six neighbour indices). */
int fnn_mesh_count(const void *seg, int label_dtype, const int64_t shape[3], const uint8_t *member, int n_table,
                   int n_regions, int64_t *counts, int64_t *boxes, void *stream);
int fnn_mesh_emit(const void *seg, int label_dtype, const int64_t shape[3], const uint8_t *member, int n_table,
                  int n_regions, const double affine[16], int smoothing_pairs, int layout, void *points,
                  int64_t cap_points, void *cells, int64_t cap_cells, void *cell_region, void *stream);

/* Fewer triangles for such a model (additive in ABI 4): data-parallel rounds of quadric-error edge collapse, what the
 * reference's callers ask of VTKModelGenerator with decimation_factor = 0.2.  As with the surface, the rule below is this
 * project's own; tests/mesh_decimate_ref.py restates it in numpy and the kernels are held to it bit for bit.
 * Input: the layout-0 result of fnn_mesh_emit on the device - points float32 [n][3], cells int32 [t][3], cell_region
 * uint16 [t] - and point_offsets (host [n_regions + 1], rising from 0 to n): region r owns the points [point_offsets[r],
 * point_offsets[r + 1]).  Every cell must name three different points below n and a region below n_regions.  Nothing in
 * the rule looks at regions: regions never share a point, so no edge crosses them.
 * Target: target = ceil((1 - d) * t) in float64, d = decimation_factor in [0, 1).  d == 0 with layout 0 returns the input
 * byte for byte by three device copies and launches nothing; d == 0 with layout 1 runs the output step alone.
 * Quadrics: one symmetric 4x4 matrix per point as 10 float64 (xx xy xz xw yy yz yw zz zw ww).  For a triangle (a, b, c):
 * n = (b - a) x (c - a) with n.x = uy vz - uz vy, n.y = uz vx - ux vz, n.z = ux vy - uy vx (u = b - a, v = c - a),
 * k = -((n.x a.x + n.y a.y) + n.z a.z), K = (n, k); Q[p] = 0 + the 10 products K_i K_j of p's triangles in ascending
 * triangle index.  From the input mesh, once; float64, every operation rounded on its own (no fused multiply-add), as
 * everything below.  When b merges into a, Q[a] = Q[a] + Q[b].
 * A round, numbered from 0.  valence(w) is the number of live triangles that hold w.  The undirected edge (a, b), a < b, is
 * a candidate iff all of these hold:
 *   valence(a) <= 32 and valence(b) <= 32 (the bound on the work of one candidate; part of the rule);
 *   exactly one live triangle runs a -> b (it is (a, b, c1) up to rotation) and exactly one runs b -> a ((b, a, c2)) - so
 *   exactly two triangles hold both ends, and an edge with four faces, where voxels touch along an edge only, is never
 *   collapsed;
 *   c1 != c2, valence(c1) > 3 and valence(c2) > 3;
 *   no vertex other than c1 and c2 is a neighbour (shares a live triangle) of both a and b (the link condition);
 *   with p the chosen position, every live triangle that holds exactly one of a, b has ((n0.x n1.x + n0.y n1.y) + n0.z n1.z)
 *   > 0, n0 its normal as above from the current float32 positions and n1 the same with the end replaced by p.
 * Position and cost: Qs = Q[a] + Q[b]; cost(p) = float32(max(c, 0)) with, for (x, y, z) = p in float64,
 *   r0 = ((Qs.xx x + Qs.xy y) + Qs.xz z) + Qs.xw, r1 = ((Qs.xy x + Qs.yy y) + Qs.yz z) + Qs.yw,
 *   r2 = ((Qs.xz x + Qs.yz y) + Qs.zz z) + Qs.zw, r3 = ((Qs.xw x + Qs.yw y) + Qs.zw z) + Qs.ww,
 *   c = ((x r0 + y r1) + z r2) + r3 (a c that is not > 0 counts as 0).
 * p is the midpoint (p[a] + p[b]) * 0.5f in float32, then p[a], then p[b]: a later one replaces an earlier one only when
 * its cost is smaller.
 * Key, a total order: (the bits of cost(p) as uint32, hash32(a, b, round), a, b), compared left to right;
 *   hash32: x = (a * 0x9E3779B1) ^ (b * 0x85EBCA77) ^ (round * 0xC2B2AE3D); x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13;
 *   x *= 0xC2B2AE35; x ^= x >> 16, all in uint32.
 * Selection: best1[w] is the smallest key among the candidates with the end w, best2[w] the smallest best1 over w and its
 * neighbours; an edge is selected iff its key equals best2 at both ends.  Selected edges share no vertex and no triangle.
 * If the live triangles minus twice the selected edges would fall below target, only the ceil((live - target) / 2) selected
 * edges with the smallest keys are applied.  Applying (a, b): p[a] = p, Q[a] = Q[a] + Q[b], every b in a triangle becomes
 * a, and the two triangles that held both are dropped; the other triangles keep their order.
 * End: the rounds stop when the live triangles are at most target (t_out is target or target - 1), or with exhausted = 1
 * when a round has no candidate or 128 rounds have been applied.
 * Output: the surviving triangles in their order, the points they name in their order, renumbered; winding untouched;
 * every region's points and triangles stay contiguous.  layout 0 and 1 as fnn_mesh_emit defines them; out_points 4-byte,
 * out_cells 4-byte (layout 0) or 16-byte (layout 1), out_cell_region 2-byte aligned, all device.  cap_points counts points
 * and cap_cells triangles; a cap below the result writes nothing and is FNN_E_INVALID with the number needed in the
 * message (n and t always suffice).  counts (host [n_regions][2]): the points and the triangles of every region.
 * status: n_out, t_out, the rounds applied, exhausted.  Nothing is written outside out_*[0, result).  Two things are placed
 * by an atomic cursor and neither decides a byte: the entries of a point's triangle list (sorted before the quadrics read
 * them in order; everything else takes counts, minima and existence from them) and the keys of the selected edges, which
 * the host reads only to cut the last round.  The same input gives the same bytes.  The stream is synchronised.
 * FNN_E_INVALID before any launch, with a message: NULL point_offsets, counts or status, a negative n or t, n_regions
 * outside 0..1024, a decimation_factor outside [0, 1) or not finite, a layout other than 0 and 1, a negative cap,
 * point_offsets that do not rise from 0 to n, triangles without a region, misaligned pointers, NULL or host pointers for
 * the model or the result; FNN_E_UNSUPPORTED: more than 2^31 - 1 points or triangle corners.  t == 0 gives zeros and
 * launches nothing.  A cell that breaks the input's rule is FNN_E_INVALID after one checking kernel.
 * Scratch, allocated inside the call: 144 B per point (position, quadric, list start, cursor, merge target, four key words,
 * selected keys) + 95 B per triangle (two copies of the cells and regions, the lists, two key words and a choice per
 * half-edge, the compaction's flags) + 4 B per 1024 of the larger + 40 B + 24 B per region. */
int fnn_mesh_decimate(const float *points, int64_t n, const int32_t *cells, const uint16_t *cell_region, int64_t t,
                      const int64_t *point_offsets, int n_regions, double decimation_factor, int layout, void *out_points,
                      int64_t cap_points, void *out_cells, int64_t cap_cells, void *out_cell_region, int64_t *counts,
                      int64_t status[4], void *stream);

/* The voxels of an image file as the file holds them -> float32 (additive in ABI 4): what the reference's
 * NibabelIO.read_images ends with (imageio/nibabel_reader_writer.py:56 and :89 - get_fdata() in float64, then
 * np.vstack(..., dtype=float32, casting='unsafe')) for one file, without the host cast.  raw: device pointer to the first
 * voxel, 16-byte aligned (FNN_E_INVALID otherwise), n_vox elements of nifti_datatype: 2 uint8, 256 int8, 4 int16,
 * 512 uint16, 8 int32, 768 uint32, 16 float32, 64 float64; any other code (complex, RGB, 64-bit integers, ...) is
 * FNN_E_UNSUPPORTED.  byteswap != 0: the bytes of every element are reversed before it is interpreted.  out: float32
 * on the device, 4-byte aligned (channel c of a [C, ...] tensor starts c * n_vox floats in, whatever n_vox is).
 * scale == 0: out = (float)v, one rounding to nearest even.  scale != 0: out = (float)((double)v * slope + inter), the
 * product and the sum each rounded to float64 (no fused multiply-add), the multiply skipped when slope == 1 and the add
 * when inter == 0.  One pass, no scratch memory, asynchronous on `stream`; n_vox == 0 returns 0. */
int fnn_decode_voxels(const void *raw, int nifti_datatype, int byteswap, int64_t n_vox, int scale, double slope,
                      double inter, float *out, void *stream);

/* The voxels of a label file as the file holds them -> a label map (additive in ABI 4): what the reference's read_seg
 * value is compared against with ==, as integers the counting and labelling kernels take, without the float32 tensor
 * and the cast behind it.  raw, nifti_datatype, byteswap, n_vox, scale, slope, inter: as fnn_decode_voxels.  The value
 * judged for a voxel is exactly the float32 fnn_decode_voxels stores for it (an integer datatype without scaling is
 * judged as the integer it is, which says the same).  out_bytes: 1 (uint8) or 2 (the bits of uint16); out: device
 * pointer aligned to the element only (a slice of a larger tensor).  A voxel whose value is integral and lies in
 * [0, 255] (out_bytes 1) or [0, 65535] (out_bytes 2) is valid and is stored as that integer.  Every other voxel stores 0
 * and raises a flag: 1 not integral or not finite, 2 negative, 4 above the output type's maximum.  status: two int32
 * on the device - [0] the flags of all voxels OR-ed, [1] the largest valid label (0 when there is none); the call zeroes
 * them on `stream` before the launch, and after the stream is synchronised both are exact and the same on every run.
 * FNN_E_INVALID before any launch: NULL or host pointers, raw not 16-byte aligned, out or status not aligned to their
 * element, out_bytes other than 1 or 2, negative n_vox; FNN_E_UNSUPPORTED: any other datatype code, more voxels than one
 * launch addresses.  n_vox == 0 zeroes status and launches nothing.  Nothing is read outside raw[0, n_vox * sizeof(T))
 * or written outside out[0, n_vox * out_bytes) and status[0..1].  One pass, no scratch memory, asynchronous on `stream`. */
#define FNN_LABEL_FLAG_NOT_INTEGRAL 1
#define FNN_LABEL_FLAG_NEGATIVE 2
#define FNN_LABEL_FLAG_TOO_LARGE 4
int fnn_decode_labels(const void *raw, int nifti_datatype, int byteswap, int64_t n_vox, int scale, double slope,
                      double inter, int out_bytes, void *out, int32_t *status, void *stream);

/* Flip and permute the axes of a C-order 3-D array on the device (additive in ABI 4): what the reference's
 * NibabelIOWithReorient does with numpy on the host (as_reoriented on read, and again on the label map on write).
 * in: shape_in[0..2] elements of elem_bytes bytes (1, 2 or 4: uint8 / uint16 labels, float32 images; anything else is
 * FNN_E_UNSUPPORTED).  out has the shape shape_in[src_axis[0]], shape_in[src_axis[1]], shape_in[src_axis[2]] and
 *   out[i0, i1, i2] = in[j],  j[src_axis[d]] = flip[d] ? shape_in[src_axis[d]] - 1 - i_d : i_d
 * - numpy's flip and transpose, bit for bit.  Both pointers are device pointers aligned to the element only (channel c of
 * an odd-sized [C, z, y, x] tensor); nothing is read or written outside the two arrays.  FNN_E_INVALID before any launch:
 * NULL or host pointers, pointers not aligned to the element, a src_axis that is no permutation of 0, 1, 2, a negative
 * extent, overlapping in and out ranges; FNN_E_UNSUPPORTED: more elements than one launch addresses.  An extent of 0
 * (no elements) returns 0 with nothing launched.  src_axis[2] == 2 is a row copy (reversed rows when flip[2]), anything
 * else a tiled transpose through LDS.  One pass, no scratch memory, asynchronous on `stream`. */
int fnn_reorient(const void *in, int elem_bytes, const int64_t shape_in[3], const int32_t src_axis[3],
                 const int32_t flip[3], void *out, void *stream);

/* A label map on the device -> the deflate bytes of its voxels in a .nii.gz file (additive in ABI 4; no counterpart in the
 * reference, whose nibabel writer compresses on the host).  in: n_elems little-endian labels of in_elem_bytes (1 or 2)
 * bytes, device pointer, 16-byte aligned.  narrow_if_fits != 0: a 2-byte map whose maximum - found here - is below 255 is
 * written as uint8, as the host writer does; *file_elem_bytes says which (1 for no elements).  out (device, any alignment,
 * out_cap >= fnn_deflate_bound(n_elems * in_elem_bytes) bytes) receives *out_bytes bytes: a fragment of a raw deflate
 * stream (RFC 1951) that leaves its reader byte aligned and not at the end - independent chunks of 16 KiB of file bytes,
 * each one non-final fixed-Huffman block followed by an empty stored block; a match has the distance of one element and
 * lies inside one 256-byte segment of its chunk.  A stream is closed behind it with the final empty fixed block 03 00.
 * *crc32: zlib's CRC-32 of the file bytes.  The bytes depend on the input alone: the same on every run.
 * Synchronises the stream (it reports sizes).  n_elems == 0: 0 bytes, CRC 0, nothing launched.  FNN_E_INVALID before any
 * launch: NULL or host pointers, a misaligned `in`, an element size other than 1 or 2, an out_cap below the bound;
 * FNN_E_UNSUPPORTED: more than 2^31 - 1 chunks (32 TiB).  Nothing is written outside out[0, *out_bytes).  Scratch,
 * allocated inside the call: 2 B per 256 file bytes and 16 B per chunk.
 * fnn_deflate_bound (host only): a capacity that always suffices - every byte a 9-bit literal, 6 bytes per chunk. */
int64_t fnn_deflate_bound(int64_t n_bytes);
int fnn_deflate_labels(const void *in, int in_elem_bytes, int64_t n_elems, int narrow_if_fits, void *out, int64_t out_cap,
                       int64_t *out_bytes, int *file_elem_bytes, uint32_t *crc32, void *stream);

/* fnn_deflate_labels with per-chunk dynamic Huffman tables (additive in ABI 4): the same arguments, contract, refusals and
 * bound, and the same chain of independent byte-aligned chunks of 16 KiB of file bytes that each end behind 00 00 FF FF.
 * The stream rule: tokens are fnn_deflate_labels' (matches at the distance of one element inside 256-byte segments).  A
 * chunk's block is BTYPE 10 with the chunk's own tables where that takes fewer bits than the fixed code, else (a tie
 * included) fnn_deflate_labels' BTYPE 01 block; so no chunk is longer than fnn_deflate_labels'.  Own tables: literal /
 * length frequencies from the chunk's tokens and one for 256.  Code lengths (limit 15): a Huffman tree from two queues - the
 * used symbols ascending by (frequency, index), and the merged nodes in the order they are made; the smaller head is taken,
 * the merged node on a tie.  Leaf depths above the limit count as the limit; while the Kraft sum exceeds 1, the deepest leaf
 * above the last level moves one level down and a leaf of the last level becomes its brother (2^-limit off the sum).  The
 * lengths are handed out longest first to the symbols in ascending (frequency, index) order; one used symbol gets length
 * 1.  The result is complete but not claimed to be the optimal length-limited code.  Canonical codes (RFC 1951 3.2.2); a
 * constant distance code of two 1-bit symbols (HDIST = 2, complete); HLIT from the last used symbol, at least 257; the
 * HLIT + 2 lengths as one sequence (a run may cross into the distance lengths), coded greedily from the left - at a run of
 * r equal values v: v = 0 and r >= 11 -> 18 with min(r, 138), v = 0 and r >= 3 -> 17 with r, v > 0 behind a v and r >= 3
 * -> 16 with min(r, 6), else v itself - under a code-length code made by the same construction with limit 7; HCLEN
 * trimmed along the permuted order, at least 4.
 * csrc/deflate_dyn_core.h states the rule in full.  *dynamic_chunks (may be NULL): the chunks that took their own tables.
 * fnn_inflate_segments refuses such a fragment with FNN_INFLATE_DYNAMIC; fnn_inflate_segments_dyn and zlib read it.  The
 * bytes depend on the input alone.  Synchronises the stream.  Scratch, allocated inside the call: fnn_deflate_labels' and 420 B per chunk. */
int fnn_deflate_labels_dyn(const void *in, int in_elem_bytes, int64_t n_elems, int narrow_if_fits, void *out, int64_t out_cap,
                           int64_t *out_bytes, int *file_elem_bytes, uint32_t *crc32, int64_t *dynamic_chunks, void *stream);

/* One label map on the device -> one deflate fragment per requested label, of the uint8 mask m[i] = (in[i] == label): the
 * voxel bytes of the per-label mask files of JHU_inference.py's export (<case>/predictions/<label_name>.nii.gz), in one
 * pass over the map per phase (additive in ABI 4).  Stateless, in two phases, because no useful capacity is known before
 * the sizes are: fnn_deflate_masks_count reports them, fnn_deflate_masks_emit writes the fragments.
 * in: n_elems little-endian labels of in_elem_bytes (1 or 2) bytes, device pointer, 16-byte aligned; a 2-byte label is
 * compared in all 16 bits.  labels: n_labels host values in [0, 65535] in any order; a value the map cannot hold (300 on a
 * 1-byte map) gives the all-zero mask; a value named twice is FNN_E_INVALID (so n_labels <= 65536, which is also what the
 * launch geometry addresses: one workgroup per label in the scan).
 * A fragment is fnn_deflate_labels' stream of the mask bytes - independent 16 KiB chunks, each a non-final fixed-Huffman
 * block and an empty stored block, matches at distance 1 inside 256-byte segments - with one change: a full chunk in which
 * the label does not occur is the constant "zero chunk" of 112 bytes (block header, literal 0, 63 matches of 258 and one
 * of 129 at distance 1, end-of-block, the empty stored block).  A chunk in which it occurs, and a last partial chunk
 * always, is tokenised by segments as before.  Closed with 03 00 a fragment inflates to the mask; it is never longer than
 * fnn_deflate_labels' fragment of the mask; the bytes depend on the input alone.
 * work: a device buffer, 16-byte aligned, of at least fnn_deflate_masks_work_bytes(n_elems, n_labels) bytes (host only;
 * 0 for arguments the calls refuse).  With C = ceil(n_elems / 16384) chunks, L = n_labels and r16 = rounding up to 16:
 *   384 + r16(4 L) + r16(8 (L + 1)) + r16(8 L) + r16(4 L) + 8 L C + r16(2 L C)
 * - the CRC field's powers and the zero chunk (384 B), the labels, the fragments' offsets in `out`, their sizes and CRCs,
 * and per (label, chunk) 8 B (the chunk's CRC, then its offset in the fragment) and 2 B (its size; 0 = the zero chunk,
 * which is also how presence is kept).  Nothing is kept per segment.
 * fnn_deflate_masks_count fills work, synchronises the stream and reports, per label in the order given, the fragment's
 * size and zlib's CRC-32 of the mask bytes (frag_bytes, crc32: host arrays of n_labels).
 * fnn_deflate_masks_emit takes the same in, n_elems and labels and the work count filled (anything else is
 * FNN_E_INVALID where it can be told: the labels are compared with those in work) and writes fragment k at offset
 * sum(frag_bytes[:k]) of out (device, any alignment); out_cap must be at least the sum of all sizes, and nothing is
 * written outside out[0, sum).  It reads the sum back from work (waiting for what the stream held before), then launches
 * asynchronously on `stream`.
 * n_elems == 0: sizes 0, CRC 0, nothing launched.  FNN_E_INVALID before any launch, with a message: NULL or host pointers
 * (in, work, out), a misaligned in or work, an element size other than 1 or 2, a negative n_elems, n_labels < 1, a label
 * outside [0, 65535], a duplicate label, a work_cap or out_cap that is too small.  FNN_E_UNSUPPORTED: more than 2^31 - 1
 * chunks. */
int64_t fnn_deflate_masks_work_bytes(int64_t n_elems, int n_labels);
int fnn_deflate_masks_count(const void *in, int in_elem_bytes, int64_t n_elems, const int32_t *labels, int n_labels,
                            void *work, int64_t work_cap, int64_t *frag_bytes, uint32_t *crc32, void *stream);
int fnn_deflate_masks_emit(const void *in, int in_elem_bytes, int64_t n_elems, const int32_t *labels, int n_labels,
                           const void *work, void *out, int64_t out_cap, void *stream);

/* A raw deflate stream on the device that is a chain of byte-aligned segments -> its bytes (additive in ABI 4; no
 * counterpart in the reference, which inflates with zlib on the host).  A single decoder cannot inflate a general deflate stream in
 * parallel - a speculative one can, and fnn_inflate_stream below is one; this entry serves the streams that need no
 * speculation: the fragments of fnn_deflate_labels and fnn_deflate_masks_emit, and what zlib writes with Z_FIXED between
 * Z_FULL_FLUSH points.  A segment starts at a byte and is a run of non-final blocks, stored (LEN / NLEN checked) or
 * fixed Huffman, up to and including the first empty stored block (.. 00 00 FF FF), behind which it ends on a byte; no
 * match reaches back past its own first output byte, it makes at most FNN_INFLATE_SEGMENT_MAX output bytes and takes at
 * most 18480 input bytes (csrc/inflate_core.h derives the number).
 * in: in_bytes bytes, device pointer, 16-byte aligned, claimed to be a chain of segments from byte 0 to byte in_bytes.
 * starts: n_starts HOST positions where a segment may start, strictly ascending, starts[0] == 0, all below in_bytes;
 * positions that start no segment are allowed (the caller finds candidates by the marker 00 00 FF FF, which also occurs
 * inside data).  out: device pointer, 16-byte aligned, of exactly out_bytes bytes.  *crc32, *status: host words.
 * Count pass: one wave per candidate decodes from starts[i] and records where the segment ended, the bytes it made and
 * why it stopped.  Chain, on the host: from candidate 0 on, the end of a member must be in_bytes (the chain is closed) or
 * a candidate (the next member).  Emit pass, launched only for a closed chain whose sizes sum to out_bytes: one wave per
 * member decodes again into LDS, stores its bytes at the member's offset in `out` (whole aligned 16-byte vectors, the ends
 * singly) and leaves their CRC-32; the host folds these in chain order into *crc32.
 * Returns 0 with *status == FNN_INFLATE_OK: out[0, out_bytes) holds the inflated bytes and *crc32 zlib's CRC-32 of them;
 * the bytes are the same on every run.  Returns 0 with *status != 0: the stream is not served - the reason of the first
 * member of the chain that was refused, FNN_INFLATE_CHAIN, or FNN_INFLATE_SIZE - and out's contents are unspecified;
 * nothing is launched past the point of knowing.  Candidates off the chain are ignored, whatever they decoded to.  In
 * every case nothing is read outside in[0, in_bytes) or written outside out[0, out_bytes), and every loop of the decoder
 * is bounded by the two budgets of a segment, whatever the input holds.  n_starts == 0 or in_bytes == 0: nothing is
 * launched, CRC 0, status FNN_INFLATE_OK when out_bytes == 0 too and FNN_INFLATE_SIZE otherwise.
 * Synchronises the stream (it reports status).  FNN_E_INVALID before any launch, with a message: NULL arguments, negative
 * sizes, a misaligned in or out, starts that do not begin at 0, do not ascend or reach in_bytes, host pointers for in or
 * out; FNN_E_UNSUPPORTED: more than 2^31 - 1 candidates.  Scratch, allocated inside the call: 48 B per candidate. */
#define FNN_INFLATE_SEGMENT_MAX 16384
#define FNN_INFLATE_OK 0
#define FNN_INFLATE_DYNAMIC 1   /* a block with dynamic tables (BTYPE 2): not served                                      */
#define FNN_INFLATE_BTYPE3 2    /* BTYPE 3                                                                              */
#define FNN_INFLATE_FINAL 3     /* a block with BFINAL set inside the chain                                             */
#define FNN_INFLATE_SYMBOL 4    /* literal / length symbol 286 or 287, distance symbol 30 or 31                         */
#define FNN_INFLATE_NLEN 5      /* a stored block whose NLEN is not the complement of LEN                               */
#define FNN_INFLATE_DISTANCE 6  /* a match that reaches back past the segment's first output byte                       */
#define FNN_INFLATE_OUTPUT 7    /* a segment of more than FNN_INFLATE_SEGMENT_MAX output bytes                          */
#define FNN_INFLATE_INPUT 8     /* a segment of more input bytes than its budget                                        */
#define FNN_INFLATE_END 9       /* the input ended inside a segment                                                     */
#define FNN_INFLATE_CHAIN 10    /* a member ended short of in_bytes at a position that is no candidate                  */
#define FNN_INFLATE_SIZE 11     /* the members' sizes do not sum to out_bytes                                           */
int fnn_inflate_segments(const void *in, int64_t in_bytes, const int64_t *starts, int64_t n_starts, void *out,
                         int64_t out_bytes, uint32_t *crc32, int32_t *status, void *stream);

/* fnn_inflate_segments for chains whose segments may hold dynamic-Huffman blocks too (additive in ABI 4): the fragments of
 * fnn_deflate_labels_dyn, and what zlib writes with any strategy between Z_FULL_FLUSH points at most 16384 bytes apart.
 * The same arguments, contract, chain rule, refusals before launch and scratch; the segment rule differs in one point: a
 * BTYPE 10 block is decoded.  Its table header is accepted exactly where zlib's inflate accepts it - HLIT <= 286 and
 * HDIST <= 30; a complete code-length code; the HLIT + HDIST lengths as one sequence, no 16 at position 0 and no run past
 * the end; a code for symbol 256; literal / length and distance sets that are not over-subscribed and incomplete only with
 * no code longer than 1 bit (a distance set of all zeros serves a block of literals only) - and refused with
 * FNN_INFLATE_TABLES otherwise; a bit pattern that belongs to no symbol of an accepted incomplete set is
 * FNN_INFLATE_SYMBOL.  FNN_INFLATE_DYNAMIC is never reported.  The two budgets of a segment are unchanged
 * (csrc/inflate_dyn_core.h states the rule in full and the order of its checks).  On a stream without dynamic blocks the
 * bytes, the CRC and the status are those of fnn_inflate_segments.  The kernels (csrc/inflate_dyn.hip) build each block's
 * three canonical codes with the wave, in LDS. */
#define FNN_INFLATE_TABLES 12   /* a dynamic block's table header that zlib's inflate would refuse (fnn_inflate_segments_dyn) */
int fnn_inflate_segments_dyn(const void *in, int64_t in_bytes, const int64_t *starts, int64_t n_starts, void *out,
                             int64_t out_bytes, uint32_t *crc32, int32_t *status, void *stream);

/* Any raw deflate stream on the device -> its bytes, speculatively and block-parallel (additive in ABI 4): what zlib, and so
 * nibabel, SimpleITK and nnU-Net, write.  csrc/inflate_any_core.h states the rule in full.
 * A CANDIDATE is a bit position where a decode may begin: bit 0, and every bit position at which BFINAL 0, BTYPE 10 stand
 * in front of a table header that passes the checks of fnn_inflate_segments_dyn (exactly zlib's accepted set) and ends
 * inside the input.  A true non-final dynamic block start is always one; zlib cuts a block every 16 K symbols at the most.
 * fnn_inflate_find_blocks: all candidates of in[0, in_bytes), ascending.  positions: DEVICE array of cap int64 (may be
 * NULL with cap == 0); *n (host): how many there are - the first min(*n, cap) are written.  Synchronises.
 * fnn_inflate_stream: in (device, 16-byte aligned) inflates to exactly out_bytes bytes at out (device, 16-byte aligned).
 *   find    the candidates (a cheap test of 74 bits per bit position and lane, the survivors by the full rule; compacted
 *           in ascending order by count, scan and write)
 *   count   one wave per candidate decodes its MEMBER - block after block, stored and fixed ones included, until a
 *           non-final block ends at a candidate or a final block ends at the input's last byte - keeping nothing, and
 *           records the end bit, the 64-bit length, the reason and how far before its own first byte its matches reach
 *   chain   on the host: member 0 starts at bit 0, a member's end is the stream's end or the next member; a member that
 *           was refused gives its reason, one that reaches back before output byte 0 FNN_INFLATE_DISTANCE, sizes that do
 *           not sum to out_bytes FNN_INFLATE_SIZE; a member that would pass out_bytes is FNN_INFLATE_OUTPUT.  Candidates
 *           off the chain are ignored.  For a valid stream the chain always closes.
 *   emit    one wave per member decodes again into 16-bit entries: a byte as 0 .. 255, a match source before the member's
 *           first byte as 0x8000 | its index in the 32 KiB of output in front of the member
 *   window  one workgroup walks the members in order and makes each one's 32 KiB window of resolved bytes
 *   resolve parallel over the output: entries and windows -> bytes, and their CRC-32 per 16 KiB, folded on the host
 * There is no limit on a member's output or input here; every loop is bounded by the input's bits.  The contract is
 * fnn_inflate_segments': returns 0 with a status word; with FNN_INFLATE_OK out holds the bytes and *crc32 zlib's CRC-32 of
 * them, the same on every run; on any other status out's contents are unspecified and nothing was launched past the point
 * of knowing; nothing is read outside in[0, in_bytes) or written outside out[0, out_bytes); it synchronises.  The reasons
 * are those above but FNN_INFLATE_DYNAMIC and FNN_INFLATE_INPUT; FNN_INFLATE_FINAL: bytes follow the final block.
 * in_bytes == 0: nothing is launched, FNN_INFLATE_OK when out_bytes == 0 too and FNN_INFLATE_SIZE otherwise.
 * FNN_E_INVALID before any launch: NULL arguments, negative sizes, a misaligned in or out, host pointers.
 * Scratch, allocated inside the call: in_bytes + 12 B per 2 KiB of input (the finder's masks), 32 B per candidate,
 * 32 B + 4 B + a 32 KiB window per member, 2 B per output byte and 4 B per 16 KiB of output.  A stream of few blocks has few
 * members and so little parallelism: one stored or fixed-only stream is decoded by one wave. */
int fnn_inflate_find_blocks(const void *in, int64_t in_bytes, int64_t *positions, int64_t cap, int64_t *n, void *stream);
int fnn_inflate_stream(const void *in, int64_t in_bytes, void *out, int64_t out_bytes, uint32_t *crc32, int32_t *status,
                       void *stream);

/* ---- host-side integer logic (no GPU needed) ------------------------------ */
/* compute_steps_for_sliding_window (sliding_window_prediction.py:30-54) for one
 * axis; returns the number of steps written (<= cap) or a negative error. */
int fnn_compute_steps(int64_t image_size, int64_t patch_size, double step, int64_t *steps, int cap);

/* Padded shape, low-side pad, number of patches and (optionally) the patch
 * origins [n][3] in the reference's visit order - x slowest, z fastest - for a
 * volume (pad_nd_image use at :657-659 and the slicer loop :525-537). */
/* patch[0] == 0 denotes a 2-D configuration (patch = {0, py, pz}): every slice of the first axis. */
int fnn_plan_volume(const int32_t patch[3], const int64_t shape_sp[3], double step, int64_t padded[3],
                    int64_t pad_lo[3], int64_t *n_patches, int32_t *origins, int64_t origins_cap);

/* The weight quantiser of FNN_PREC_F8: float32 -> OCP e4m3 ("fn": +-448 saturating, 0x7f = NaN), round to nearest
 * even - the encoding v_mfma_f32_16x16x32_fp8_fp8 reads on gfx950 (not MI300's fnuz).  Exposed so that the host-side
 * packing can be checked against another implementation without a GPU. */
int fnn_fp8_e4m3_encode(const float *in, int64_t n, uint8_t *out);

/* ---- timing / introspection ----------------------------------------------- */
/* Per-kernel-family device time of the last fnn_predict_volume call, measured
 * with HIP events on the launch stream when profiling is enabled. */
typedef struct fnn_profile {
    double total_ms;
    double conv_ms, stem_ms, tconv_ms, head_ms, finalize_ms;
    int64_t conv_launches;
    double conv_flops;                           /* algorithmic 2*MACs of the timed convs     */
    int64_t n_patches;
    double conv_bytes;                           /* algorithmic HBM bytes of the timed convs: every input
                                                  * element read once, every output element written once */
} fnn_profile;
int fnn_set_profiling(fnn_engine *e, int enabled);
int fnn_get_profile(const fnn_engine *e, fnn_profile *out);
/* Which kernel variant served every launch of the last call made while profiling was on (one line per launch, in launch
 * order: "conv3d_zr_kernel<2,8>", "conv_row_kernel<6,1,0>", ...).  A conv layer's kernel is chosen once, when the engine
 * is created, from the layer shape and the planned batch: its line is the last column of fnn_layer_table, and
 * fnn_plan_table shows the choice without a GPU.  Returns the bytes needed (with the terminating 0); writes at most
 * `cap`.  No counterpart in the reference. */
int64_t fnn_kernel_log(const fnn_engine *e, char *buf, int64_t cap);

/* Per-launch rows of the same profiled call (measurement aid of bench.py --plan / tools/plan_sweep.py; additive in ABI 4,
 * no counterpart in the reference): one line per timed launch, tab-separated -
 *   layer index (-1: seg head / gather / finalize), family (conv | stem | tconv | head | finalize), milliseconds between
 *   the launch's two HIP events, algorithmic 2*MACs, algorithmic HBM bytes, kernel variant(s) as in fnn_kernel_log.
 * fnn_layer_table describes the layers those indices name: index, type, input channels, output channels, kernel, stride,
 * input dims, output dims, 2*MACs per patch, algorithmic bytes per patch, 1 = computed inside its consumer / 2 = a
 * consumer that recomputes its producer / 0, the kernel chosen for a conv layer as fnn_kernel_log names it (- for other
 * layers).  Both return the bytes needed and write at most `cap`.
 * fnn_plan_table: the fnn_layer_table rows of an engine that fnn_create(arch, any device, max_batch) would plan - without
 * a GPU (additive in ABI 4); a negative FNN_E_* code when that engine could not be created. */
int64_t fnn_profile_launches(const fnn_engine *e, char *buf, int64_t cap);
int64_t fnn_layer_table(const fnn_engine *e, char *buf, int64_t cap);
int64_t fnn_plan_table(const fnn_arch_desc *arch, int max_batch, char *buf, int64_t cap);

/* Algorithmic work of one patch forward: 2*MACs of convs, transposed convs and
 * the seg head; ideal fp16 activation bytes (each activation written once and
 * read once).  SURVEY.md 8d. */
int fnn_patch_work(const fnn_engine *e, double *flops, double *act_bytes);

/* ---- single-op entry points (parity tests call the kernels through these) -- */
/* Host float32 NCDHW in / out; the library converts to its device layout
 * (fp16, channels-last), runs the HIP kernel, converts back.
 * Input transform fused into the kernel's load path: when gammaK != NULL the
 * input K is treated as a RAW conv output: InstanceNorm3d(eps=1e-5, affine)
 * with these gamma/beta is applied (statistics of the fp16-rounded input,
 * computed by the wrapper the way a producer kernel's epilogue would), then
 * LeakyReLU(slopeK).  gammaK == NULL = identity.  A second input (x2 != NULL)
 * is the concat-free replacement of torch.cat((x, x2), 1).
 * stats_out (may be NULL): per (n, cout) sum and sum of squares of the
 * fp16-rounded outputs, doubles [n][cout][2].
 * FNN_OP_F8=1 (honoured next to FNN_KNOBS=1, read per call): OCP e4m3
 * operands where an FNN_PREC_F8 engine would give them (3x3x3 stride-1 layers
 * the fp8 depth-shift kernel takes; other layers run their fp16 kernel), with
 * the weights, output scales and activation multiplier the engine uses. */
int fnn_op_conv3d(int device, int n, const int dims[3],
                  const float *x, int cin, const float *gamma1, const float *beta1, float slope1,
                  const float *x2, int cin2, const float *gamma2, const float *beta2, float slope2,
                  const float *w, const float *bias, int cout, const int k[3], const int stride[3],
                  float *y, double *stats_out);
int fnn_op_conv_transpose3d(int device, int n, const int dims[3],
                            const float *x, int cin, const float *gamma1, const float *beta1, float slope1,
                            const float *w, const float *bias, int cout, const int stride[3], float *y);

/* ---- single-op entry points of the kernels between the convs (additive in ABI 4) ----
 * The same conventions: host float32 NCDHW in / out, operands rounded to fp16 once by the library, gamma != NULL = the
 * operand is a raw conv output whose InstanceNorm (statistics of the fp16-rounded values) is applied on load; here the
 * LeakyReLU slope of an operand applies with or without a norm (1 = none).  Each call goes through the launcher the
 * engine calls.  The layout of every device tensor is an ARGUMENT (x_chunk_major etc.: 0 = channels-last,
 * 1 = [C / 16][voxels][16]), because the kernels take either on each operand and output separately.
 *
 * fnn_op_avgpool: AvgPool3d(stride, stride) of the transformed x (the skip path of a strided residual block),
 *   y [n][c][D / s0][H / s1][W / s2].
 * fnn_op_combine: y = LeakyReLU(T_a(a) + T_b(b), slope), the closing add of a residual block.  pool_stride != NULL:
 *   the launch also writes AvgPool3d(pool_stride) of the fp16-rounded y into `pooled` (FNN_E_UNSUPPORTED for strides or
 *   sizes the fused kernel does not take: the planner sends those through the pooling kernel). */
int fnn_op_avgpool(int device, int n, const int dims[3], const float *x, int c,
                   const float *gamma, const float *beta, float slope, const int stride[3],
                   int x_chunk_major, int y_chunk_major, float *y);
int fnn_op_combine(int device, int n, const int dims[3], int c,
                   const float *a, const float *gamma_a, const float *beta_a, float slope_a,
                   const float *b, const float *gamma_b, const float *beta_b, float slope_b,
                   float slope, const int pool_stride[3],
                   int a_chunk_major, int b_chunk_major, int y_chunk_major, int pooled_chunk_major,
                   float *y, float *pooled);
/* fnn_op_seg_head: the 1x1x1 seg head of batch item `item` of the features x [n][c][PD][PH][PW] (norm on load as above),
 *   weights w [heads][c] and bias [heads] (NULL = 0) packed as the engine packs them, weight-sum row included.
 *   mode 0: logits * gaussian accumulated into the box acc [box0][box1][box2][HP] (HP = round_up(heads + 1, 8); fp16 bits
 *     or float32 by acc_fp32; in / out) at `origin`; gauss = fp16 bits [PD * PH * PW] or NULL (weight 1); channel `heads`
 *     accumulates the weight.  first_visit (NULL = read every voxel): the thresholds of HeadParams - voxels with
 *     d >= first_visit[0] && h >= [1] && w >= [2] are written as 0 + contribution without being read.  Only the
 *     one-k-step kernels know them: *first_visit_honoured (may be NULL) says whether this call's kernel does, and
 *     thresholds other than INT_MAX are FNN_E_UNSUPPORTED when it does not.
 *   mode 1 / 2: patch_buf [heads][PD * PH * PW] float32 (in / out) = / += the logits, un-mirrored by `flips`.
 * fnn_op_patch_acc: the mean of n_div mirrored evaluations (patch_buf / n_div) * gaussian accumulated into acc, as above.
 * fnn_op_patch_input: patch windows of the volumes vol [n_vol][c][X][Y][Z] (n_vol = 1: one volume for every item, or
 *   n_vol = n) at origins [n][3], mirrored by `flips` -> the fp16 bits of the network input, out [n][cpad][PD][PH][PW]
 *   (the padding channels included). */
int fnn_op_seg_head(int device, int n, int c, const int patch[3], const float *x,
                    const float *gamma, const float *beta, float slope,
                    int heads, const float *w, const float *bias,
                    int item, int mode, const int flips[3], const unsigned short *gauss,
                    void *acc, int acc_fp32, const long long box[3], const int origin[3], const int first_visit[3],
                    float *patch_buf, int *first_visit_honoured);
int fnn_op_patch_acc(int device, const float *patch_buf, int heads, const int patch[3], int n_div,
                     const unsigned short *gauss, void *acc, int acc_fp32, const long long box[3], const int origin[3]);
int fnn_op_patch_input(int device, const float *vol, int n_vol, int c, const long long vdim[3],
                       int n, const int *origins, const int flips[3], const int patch[3], int cpad, int chunk_major,
                       unsigned short *out);
/* fnn_op_stem: the network's first conv on patch windows of the fp32 volumes vol [n_vol][c][X][Y][Z] (n_vol = 1 or n) at
 *   origins [n][3], mirrored by `flips` (the output is not mirrored back), zero padding at the PATCH border; weights
 *   w [cout][c][kd][kh][kw], bias [cout] (NULL = 0), packed as the engine packs them; the launcher picks the kernel.
 *   -> y [n][cout][PD][PH][PW] and, with stats_out, [n][cout][2] = (sum, sum of squares) of the rounded outputs summed over
 *   the slot rows.
 * fnn_op_conv_fused: a 16-channel stride-1 conv (weights w, bias, kernel k) that recomputes its producer while it stages, as
 *   the engine runs the pair.  dims = the consumer's (input = output) size.
 *   mode 1 (stem): the producer is the one-channel stem (pw [16][1][k], pbias) of the windows of vol [n_vol][1][X][Y][Z] at
 *     origins / flips, with InstanceNorm (pgamma, pbeta) and LeakyReLU pslope; w [16][16][k].  Runs the stem's statistics pass,
 *     their finalisation, then the consumer.  low / tstride / skip* are not read.
 *   mode 2 (transposed conv): the producer is ConvTranspose3d (kernel = stride = tstride; pw [low_c][16][taps], pbias) of
 *     low [n][low_c][dims / tstride] normalised on load with (pgamma, pbeta, pslope; NULL = identity); the consumer reads its
 *     output ("up", channels 0 .. 15) next to skip [n][16][dims] with its own (skip_gamma, skip_beta, skip_slope);
 *     w [16][32][1][3][3].  vol / vdim / origins / flips are not read.
 *   -> y [n][16][dims] and, with stats_out, the consumer's statistics [n][16][2].  FNN_E_UNSUPPORTED: no kernel fuses the pair. */
int fnn_op_stem(int device, const float *vol, int n_vol, int c, const long long vdim[3],
                int n, const int *origins, const int flips[3], const int patch[3],
                const float *w, const float *bias, int cout, const int k[3], float *y, double *stats_out);
int fnn_op_conv_fused(int device, int mode, int n, const int dims[3],
                      const float *vol, int n_vol, const long long vdim[3], const int *origins, const int flips[3],
                      const float *low, int low_c, const int tstride[3],
                      const float *skip, const float *skip_gamma, const float *skip_beta, float skip_slope,
                      const float *pw, const float *pbias, const float *pgamma, const float *pbeta, float pslope,
                      const float *w, const float *bias, const int k[3], float *y, double *stats_out);

/* The kernel variants the last fnn_op_* call of this thread launched, one per line (the
 * launchers pick a variant from the layer's shape; the op tests pin which one a case exercises).  Returns the size needed. */
int fnn_op_last_kernels(char *buf, int cap);

/* The shader clock the device holds while other work runs (measurement aid, no counterpart in the reference; additive in
 * ABI 4): fnn_clock_probe_start launches ONE wave on a stream of its own that sleeps between reads of the shader-clock
 * counter (s_memtime) and the constant 100 MHz counter (s_memrealtime) until max_seconds have passed on the latter or
 * fnn_clock_probe_stop raises a flag in mapped host memory; stop waits for it and returns elapsed shader cycles / elapsed
 * time in GHz.  (A device-wide synchronisation waits for the probe like for any kernel: give it less time than the
 * region it samples.)  bench.py runs one extra, untimed step beside it: under sustained MFMA load the chip lowers its
 * clock, and a roofline fraction priced at 2.4 GHz does not say how much of what the clock allows a
 * kernel uses.  The probe is not free: next to it per-launch durations stretch by ~4 %, and with HIP's default of four
 * hardware queues it can share a queue with a caller's stream, whose work then waits for it (bench.py runs it from a process of its own). */
int fnn_clock_probe_start(int device, double max_seconds, void **probe);
int fnn_clock_probe_stop(void *probe, double *ghz, double *seconds);

/* Self-check of the closing division of the seg-head gather (predicted_logits /= n_predictions,
 * predict_from_raw_data.py:619): runs the kernel's shared-reciprocal quotient over every fp16 value a and every fp16
 * b with a clear sign bit and counts the pairs whose fp16 result differs from IEEE fp32 division rounded to fp16
 * (counts[0], must be 0), the pairs that took the fast route at all (counts[1]) and one differing pair as
 * a_bits | b_bits << 16 (counts[2], 0 when there is none). */
int fnn_op_quotient_check(int device, unsigned long long counts[3]);

#ifdef __cplusplus
}
#endif
#endif /* FNN_H */
