// ensemble_common.h - what ensemble.hip (members on the cropped grid) and ensemble_resample.hip (members on their network
// grids) must agree on bit for bit: the number of members and the rule that turns a voxel's averaged heads into its label.
#pragma once
#include "fnn_device.h"
#include <cmath>

constexpr int ENS_MAX_MEMBERS = 16;

// The merge rule on the averaged value of head h (ensemble.py:42 -> label_handling.py:183-195), heads in ascending order
// from best = -1.f, label = 0.  Regions: the reference hands the averaged PROBABILITIES to
// convert_logits_to_segmentation, which applies the sigmoid a second time before `> 0.5`; this is mirrored on purpose.
// Plain labels: argmax, the first maximum wins.
static __device__ __forceinline__ void ensemble_merge_rule(const int *order, int h, float v, float &best, int &label) {
#pragma clang fp contract(off)
    if (order) {
        if (1.f / (1.f + expf(-v)) > 0.5f) label = order[h];
    } else if (v > best) {
        best = v; label = h;
    }
}
