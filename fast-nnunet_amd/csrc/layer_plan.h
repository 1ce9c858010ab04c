// layer_plan.h - what the network is, as a value: the layer list derived from fnn_arch_desc (what the reference builds in
// PlainConvEncoder / UNetDecoder, nnUNetDistillationTrainer.py:141-173), the kernel chosen per conv layer, the fusions,
// the activation layouts, every offset into the weight, parameter, statistics and activation buffers, the weight-blob map
// and the FLOP and byte counts.  plan_layers() is its one constructor; the engine holds the result and only reads it.
// Host code only: no kernel, no __device__ function, no HIP runtime call (layer_plan.hip).
#pragma once
#include "fnn_device.h"

#include <string>
#include <vector>

struct Layer {
    enum Type { STEM, CONV, TCONV, POOL, COMBINE, GATHER } type;   // GATHER: the patches' input windows as an fp16 tensor (stem on the conv kernels)
    int n_src = 1;
    int cin_real[2] = {0, 0}, cin_pad[2] = {0, 0};
    int cout_real = 0, cout_pad = 0;
    int k[3] = {1, 1, 1}, s[3] = {1, 1, 1};
    int in_dims[3], out_dims[3];
    int src_layer[2] = {-1, -1};      // producing layer (-1 = the volume)
    bool has_norm = true;             // a conv's output is normalised by its consumers; a tconv's / pool's / block's is not
    bool act = true;                  // LeakyReLU after the norm (false: conv2 and the skip projection of a residual block)
    bool has_bias = true;             // the skip projection of a residual block has no bias
    // offsets
    size_t w_off = 0;                 // halves, packed weights (STEM: floats in fparam)
    size_t bias_off = 0, gamma_off = 0, beta_off = 0;   // floats
    size_t stats_off = 0;             // doubles
    size_t ss_off = 0;                // float2 (scale, shift) per channel
    size_t out_off = 0;               // halves, activation arena (for batch = 1)
    int64_t blob_w = 0, blob_b = 0, blob_g = 0, blob_beta = 0;
    int ksteps = 0;                   // TCONV: k-steps of its packed weights
    int stats_slots = FNN_STAT_REPL;  // rows per item in the stats buffer: atomics' replicas, or one row per tile
    ConvChoice cc;                    // CONV: the kernel chosen when the engine was planned (conv_choose); its weights are packed
                                      // for it, and stats_slots above is its
    // conv3d_thin.hip: the stem as one MFMA per 16 voxels (w_off2 = its weight fragment in wpk); a CONV that recomputes
    // its producer while staging (fuse = FUSE_STEM / FUSE_TCONV); a producer whose output is never written (virtual)
    bool mfma_stem = false, virtual_out = false;
    int pool_layer = -1;              // COMBINE: the POOL layer (the next stage's skip path) whose output this launch writes too; that POOL has pool_fused
    bool pool_fused = false;
    bool chunk_major = false;         // output stored [C / 16][voxels][16] (fnn_device.h, SrcDesc): convs / transposed convs whose consumers are convs
    bool fp8 = false;                 // conv3d_zr8_kernel: e4m3 operands; oscale_off = per-cout output scales (floats)
    size_t oscale_off = 0;
    int fuse = 0;
    size_t w_off2 = 0;
    double flops = 0;                 // 2*MACs per patch
    double bytes = 0;                 // algorithmic HBM bytes per patch: every input read once + the output written once (fp16)
};

// Every switch a plan depends on (fnn_knob: honoured next to FNN_KNOBS=1 only), read once where a plan is made
struct PlanSwitches {
    bool fuse_enabled = true;         // FNN_NO_FUSE keeps every layer a kernel of its own
    // FNN_FUSE_STEM = 0 | 1.  The transposed-conv fusion is always on (+1.2 % on the benchmark).  The stem
    // fusion is on where the row-streaming kernels take both halves (conv_row_stem_kernel + stem_row_kernel's statistics
    // pass, conv3d_row.hip); in tile form (FNN_FUSE_STEM=1 forces it) it is built and tested but slower than two kernels:
    // its consumer is instruction-bound (one MFMA per 16 halo voxels needs ~45 instructions around it), 1020 + 340 us
    // per batch against 575 + 756 us unfused.
    int fuse_stem = -1;               // -1: where the row kernels run it
    bool stem_direct = false;         // FNN_STEM_DIRECT: a multi-channel or 2-D stem on the generic stem kernel (A-B aid / its tests)
    bool no_pool_fuse = false;        // FNN_NO_POOL_FUSE: the skip path's pooling as a launch of its own
    bool no_chunk_major = false;      // FNN_NO_CHUNK_MAJOR: every activation channels-last
    int cm_min = 16;                  // FNN_CM_MIN (A-B aid): chunk-major above this many channels
    ConvOverrides ov;                 // the test switches of the conv kernels' choice
    static PlanSwitches from_env();
};

// A layer's output layout as SrcDesc::vs / cs: chunk-major (16, 16 x voxels), or channels-last - (0, 0), which the launch
// parameters' out_vs / out_cs read as (C, 16)
struct Layout { int vs; long long cs; };

struct LayerPlan {
    fnn_arch_desc arch;                     // eps <= 0 replaced by the default 1e-5
    int max_batch = 1;
    PlanSwitches switches;
    std::vector<Layer> layers;
    int head_src = -1;                      // layer feeding the seg head
    int hblocks = 0, head_ksteps = 0;
    size_t head_w_off = 0, head_bias_off = 0;
    int n_gpass = 1;                        // gather passes of <= 63 heads (GatherParams::n_pass); > 1: their own packs below
    size_t gpass_w_off = 0, gpass_bias_off = 0;
    int64_t blob_head_w = 0, blob_head_b = 0;
    int64_t blob_count = 0;
    size_t wpk_halves = 0, fparam_floats = 0, stats_doubles = 0, act_halves = 0, ss_count = 0;
    double head_flops = 0, patch_flops = 0, patch_act_bytes = 0;

    // An arena's buffers in bytes - activations, statistics, scale / shift rows; returns their sum
    size_t arena_bytes(size_t b[3]) const;
    // The shape facts of a conv layer that its kernel's choice looks at (conv_choose); forward_batch launches the layer from
    // them.  fuse / T: recomputing its producer T
    ThinParams conv_shape(const Layer &L, int fuse = 0, const Layer *T = nullptr) const;
    static Layout layout(const Layer &L) {
        return L.chunk_major ? Layout{16, 16LL * L.out_dims[0] * L.out_dims[1] * L.out_dims[2]} : Layout{0, 0};
    }
};

// The plan of `arch` for up to max_batch patches per forward.  0, or an FNN_E_* status with its message in err (out is
// then half-made and must not be used)
int plan_layers(const fnn_arch_desc &arch, int max_batch, const PlanSwitches &sw, LayerPlan &out, std::string &err);

// A fold's weight blob (LayerPlan::blob_count floats in the plan's blob order) as the two host images of the device
// buffers: wpk (fp16 MFMA fragments, LayerPlan::wpk_halves) and fparam (floats, LayerPlan::fparam_floats)
void pack_fold_weights(const LayerPlan &plan, const float *blob, std::vector<uint16_t> &wpk, std::vector<float> &fparam);

// One tab-separated row per layer (fnn_layer_table, fnn_plan_table)
std::string layer_table_text(const LayerPlan &plan);
