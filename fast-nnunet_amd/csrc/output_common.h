// output_common.h - the rules of the engine's output side, once: what head.hip (the accumulate path's seg head),
// finalize.hip (accumulators -> logits / labels) and gather.hip (all of it in one pass, sums in registers) must agree
// on bit for bit.  A site that keeps its own text of one of these says why (profiles/r13_output_side.txt).
#pragma once
#include "fnn_device.h"

// ---- accumulation (predict_from_raw_data.py:611-614): `pred *= gaussian; acc += pred` - the product is rounded before
// the sum.  With the multiply next to the add hipcc contracts the pair into an fma (even through __fmul_rn / __fadd_rn):
// contraction is switched off for these blocks.
static __device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
static __device__ __forceinline__ float acc_add_product(float a, float t, float g) {
#pragma clang fp contract(off)
    const float c = t * g;
    return a + c;
}

// ---- where a voxel's accumulator line starts.  Layout: acc[AX][Y][Z][HP], channels-last (head.hip); the results are
// voxel indices, an element is voxel * HP + channel.
// Voxel (d, h, w) of the patch a HeadParams / PatchAccParams places at (ox, oy, oz):
template <class P>
static __device__ __forceinline__ size_t acc_voxel_of_patch(const P &p, int d, int h, int w) {
    return ((size_t)(p.ox + d) * p.Y + (p.oy + h)) * p.Z + (p.oz + w);
}
// Voxel (x, y, z) of the output box of a FinalizeParams:
template <class TX, class TY, class TZ>
static __device__ __forceinline__ size_t acc_voxel_of_output(const FinalizeParams &p, TX x, TY y, TZ z) {
    return ((size_t)(x + p.lo_x) * p.Y + (y + p.lo_y)) * p.Z + (z + p.lo_z);
}

// ---- the seg head's MFMA operands: head block hb's packed A fragment of k-step ks (fnn_load_weights: [block][k-step][lane][8])
// and this lane's four biases.  A kernel that always multiplies four blocks asks for blocks the head does not have: those
// re-read the last one (valid memory, the same cache lines) and their rows are dropped.
static __device__ __forceinline__ int head_block(int hb, int hblocks) { return hb < hblocks ? hb : hblocks - 1; }
static __device__ __forceinline__ f16x8 head_frag(const f16 *wpk, int hbc, int ksteps, int ks, int lane) {
    return *(const f16x8 *)(wpk + (((size_t)hbc * ksteps + ks) * 64 + lane) * 8);
}
static __device__ __forceinline__ f32x4 head_bias(const float *bias, int hbc, int q) { return *(const f32x4 *)(bias + hbc * 16 + q * 4); }

// ---- labels.  LabelManager.convert_logits_to_segmentation on one voxel's logits (label_handling.py:163-181):
//   plain labels: numpy argmax - the first maximum wins, the first NaN wins;
//   regions     : label 0, then for i in order: if sigmoid(float(logit_i)) > 0.5: label = regions_class_order[i].
// torch's fp32 sigmoid exceeds 0.5 exactly for x > 1.5 * 2^-24 (probed over every fp32 around the threshold and every
// fp16 value, tests/test_oracle_golden.py) - "logit > 0" would differ for the two smallest positive fp16 values.
#define FNN_SIGMOID_HALF_THRESHOLD (1.5f * 0x1p-24f)
// Both rules are maxima under a total order, so a pick over some heads is a value that merges:
//   argmax : the lowest-index NaN first; else the largest value, the lowest index among equals;
//   regions: the highest index above the threshold.
struct LabelPick {
    float best = 0.f; int arg = -1;                            // the argmax rule's winner so far (arg < 0: no head yet)
    int hit = -1;                                              // the regions rule's
    // the next head, in ASCENDING order: a strict compare keeps the first maximum, a NaN is kept for good
    __device__ __forceinline__ void feed(int h, float v) {
        if (v > FNN_SIGMOID_HALF_THRESHOLD) hit = h;
        if (arg < 0 || (best == best && (v > best || v != v))) { best = v; arg = h; }
    }
    // a pick over other heads, in any order
    __device__ __forceinline__ void merge(const LabelPick &o) {
        const bool n = best != best, on = o.best != o.best;
        bool take;                                             // is the other pick the better one?
        if (arg < 0 || o.arg < 0) take = arg < 0;
        else if (n || on) take = on && (!n || o.arg < arg);
        else take = o.best > best || (o.best == best && o.arg < arg);
        if (take) { best = o.best; arg = o.arg; }
        hit = hit > o.hit ? hit : o.hit;
    }
    // the pick of the lane m away (a butterfly step of a cross-lane merge)
    __device__ __forceinline__ LabelPick across(int m) const {
        LabelPick o;
        o.best = __shfl_xor(best, m, 64); o.arg = __shfl_xor(arg, m, 64); o.hit = __shfl_xor(hit, m, 64);
        return o;
    }
    __device__ __forceinline__ int label(const int *order) const { return order ? (hit >= 0 ? order[hit] : 0) : arg; }
};

// labels are uint8, or uint16 for more than 255 classes (export_prediction.py:45-46)
static __device__ __forceinline__ void store_label(void *labels, int label_u16, size_t i, int lab) {
    if (label_u16) ((uint16_t *)labels)[i] = (uint16_t)lab; else ((uint8_t *)labels)[i] = (uint8_t)lab;
}
