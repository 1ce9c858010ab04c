// layer_plan.hip - host side only: fnn_arch_desc + switches -> LayerPlan (plan_layers), a fold's weight blob -> the host
// images of its device buffers (pack_fold_weights), and the layer table's text.  No kernel and no HIP runtime call: a
// plan can be made, and is tested, without a GPU (fnn_plan_table).
#include "layer_plan.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>

PlanSwitches PlanSwitches::from_env() {
    PlanSwitches s;
    s.fuse_enabled = fnn_knob("FNN_NO_FUSE") == nullptr;
    if (const char *v = fnn_knob("FNN_FUSE_STEM")) s.fuse_stem = atoi(v) != 0 ? 1 : 0;
    s.stem_direct = fnn_knob("FNN_STEM_DIRECT") != nullptr;
    s.no_pool_fuse = fnn_knob("FNN_NO_POOL_FUSE") != nullptr;
    s.no_chunk_major = fnn_knob("FNN_NO_CHUNK_MAJOR") != nullptr;
    if (const char *v = fnn_knob("FNN_CM_MIN")) s.cm_min = atoi(v);
    s.ov = ConvOverrides::from_env();
    return s;
}

size_t LayerPlan::arena_bytes(size_t b[3]) const {
    b[0] = act_halves * max_batch * sizeof(f16);
    b[1] = stats_doubles * max_batch * sizeof(double);
    b[2] = (ss_count * max_batch * 3 + 8) * sizeof(float);           // fp32 rows, then the fp16 rows (ssh_rows)
    return b[0] + b[1] + b[2];
}

ThinParams LayerPlan::conv_shape(const Layer &L, int fuse, const Layer *T) const {
    ThinParams tp{};
    ConvParams &q = tp.c;
    q.plan_N = max_batch; q.N = max_batch; q.Cout = L.cout_pad; q.fp8 = L.fp8;
    q.n_src = L.n_src; q.chunks = (L.cin_pad[0] + (L.n_src > 1 ? L.cin_pad[1] : 0)) / 16;
    q.src[0].C = L.cin_pad[0]; q.src[1].C = L.n_src > 1 ? L.cin_pad[1] : 0;
    q.Di = L.in_dims[0]; q.Hi = L.in_dims[1]; q.Wi = L.in_dims[2];
    q.Do = L.out_dims[0]; q.Ho = L.out_dims[1]; q.Wo = L.out_dims[2];
    q.kd = L.k[0]; q.kh = L.k[1]; q.kw = L.k[2]; q.sd = L.s[0]; q.sh = L.s[1]; q.sw = L.s[2];
    tp.fuse = fuse;
    if (T) {
        tp.low.C = T->cin_pad[0];
        tp.Dl = T->in_dims[0]; tp.Hl = T->in_dims[1]; tp.Wl = T->in_dims[2];
        tp.tsd = T->s[0]; tp.tsh = T->s[1]; tp.tsw = T->s[2];
    } else { tp.tsd = tp.tsh = tp.tsw = 1; }
    return tp;
}

namespace {

inline int pad16(int c) { return (c + 15) / 16 * 16; }

int refuse(std::string &err, int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
int refuse(std::string &err, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    err = buf;
    return code;
}

// What the steps of plan_layers hand on next to the plan: every stage's spatial size, and its last encoder layer (the skip)
struct Stages {
    int dims[FNN_MAX_STAGES][3];
    int enc_last[FNN_MAX_STAGES];
};

// ---- validate: the batch bound, the descriptor's ranges, and every stage's size
int validate(const fnn_arch_desc &a, int max_batch, Stages &S, std::string &err) {
    // up to 64 patches per forward, or - small patches (a 40 x 56 x 40 plan, a 2-D slice) - as many as give a forward 2^27 voxels
    // (64 patches of 128^3), at most 512: the deep layers of a small patch have too few voxels per item to fill the chip
    const long long pv = (long long)a.patch[0] * a.patch[1] * a.patch[2];
    const long long cap = pv > 0 ? std::max<long long>(64, std::min<long long>(512, (1ll << 27) / pv)) : 64;
    if (max_batch < 1 || max_batch > cap) return refuse(err, FNN_E_INVALID, "max_batch must be 1..%lld for this patch size", cap);
    if (a.kind != FNN_NET_PLAIN && a.kind != FNN_NET_RESENC) return refuse(err, FNN_E_UNSUPPORTED, "unknown network kind %d", a.kind);
    if (a.n_stages < 2 || a.n_stages > FNN_MAX_STAGES) return refuse(err, FNN_E_INVALID, "n_stages out of range");
    if (a.in_channels < 1 || a.in_channels > 4096) return refuse(err, FNN_E_UNSUPPORTED, "in_channels must be 1..4096");
    if (a.num_heads < 1 || a.num_heads > 256) return refuse(err, FNN_E_UNSUPPORTED, "num_heads must be 1..256");
    for (int s = 0; s < a.n_stages; ++s)
        for (int d = 0; d < 3; ++d) {
            if (a.kernels[s][d] != 1 && a.kernels[s][d] != 3) return refuse(err, FNN_E_UNSUPPORTED, "kernel sizes must be 1 or 3");
            if (a.strides[s][d] != 1 && a.strides[s][d] != 2) return refuse(err, FNN_E_UNSUPPORTED, "strides must be 1 or 2");
            if (s == 0 && a.strides[s][d] != 1) return refuse(err, FNN_E_UNSUPPORTED, "stage 0 must have stride 1");
        }
    if (a.spatial_dims != 0 && a.spatial_dims != 2 && a.spatial_dims != 3) return refuse(err, FNN_E_INVALID, "spatial_dims must be 2 or 3");
    if (a.spatial_dims == 2) {
        if (a.patch[0] != 1) return refuse(err, FNN_E_INVALID, "a 2-D configuration has patch[0] == 1");
        for (int s = 0; s < a.n_stages; ++s)
            if (a.kernels[s][0] != 1 || a.strides[s][0] != 1)
                return refuse(err, FNN_E_INVALID, "a 2-D configuration has kernel and stride 1 along the first axis");
    }
    for (int d = 0; d < 3; ++d) S.dims[0][d] = a.patch[d];
    for (int s = 1; s < a.n_stages; ++s)
        for (int d = 0; d < 3; ++d) {
            const int k = a.kernels[s][d], st = a.strides[s][d], pad = (k - 1) / 2;
            S.dims[s][d] = (S.dims[s - 1][d] + 2 * pad - k) / st + 1;
            if (S.dims[s][d] * st != S.dims[s - 1][d])
                return refuse(err, FNN_E_INVALID, "patch size %d is not divisible by the pooling of axis %d", a.patch[d], d);
        }
    return 0;
}

// ---- the encoder / decoder layer list, with the weight-blob map and the per-layer FLOP and byte counts
int list_layers(LayerPlan &p, Stages &S, std::string &err) {
    const fnn_arch_desc &a = p.arch;
    const auto &dims = S.dims;
    int64_t blob = 0;
    bool next_has_bias = true, next_act = true;
    auto add_conv = [&](Layer::Type type, int nsrc, const int cin[2], const int src[2], int cout, const int32_t *k,
                        const int32_t *s, const int *in_d, const int *out_d) {
        Layer L;
        L.type = type; L.n_src = nsrc; L.has_bias = next_has_bias; L.act = next_act;
        int cin_tot = 0;
        for (int i = 0; i < nsrc; ++i) {
            L.cin_real[i] = cin[i]; L.cin_pad[i] = (type == Layer::STEM) ? cin[i] : pad16(cin[i]);
            L.src_layer[i] = src[i]; cin_tot += cin[i];
        }
        L.cout_real = cout; L.cout_pad = pad16(cout);
        for (int d = 0; d < 3; ++d) { L.k[d] = k[d]; L.s[d] = s[d]; L.in_dims[d] = in_d[d]; L.out_dims[d] = out_d[d]; }
        const int T = k[0] * k[1] * k[2];
        L.blob_w = blob; blob += (int64_t)cout * cin_tot * T;
        L.blob_b = blob; if (L.has_bias) blob += cout;
        L.blob_g = blob; blob += cout;
        L.blob_beta = blob; blob += cout;
        L.flops = 2.0 * cout * cin_tot * T * out_d[0] * out_d[1] * out_d[2];
        L.bytes = 2.0 * ((double)cin_tot * in_d[0] * in_d[1] * in_d[2] * (type == Layer::STEM ? 2 : 1)     // fp32 volume
                         + (double)cout * out_d[0] * out_d[1] * out_d[2]);
        p.layers.push_back(L);
        return (int)p.layers.size() - 1;
    };
    const int32_t one[3] = {1, 1, 1};
    int prev = -1, prev_c = a.in_channels;
    auto add_aux = [&](Layer::Type type, int src0, int src1, int channels, const int32_t *st, const int *in_d, const int *out_d) {
        Layer L;
        L.type = type; L.n_src = src1 >= 0 ? 2 : 1; L.has_norm = false;
        L.src_layer[0] = src0; L.src_layer[1] = src1;
        L.cin_real[0] = channels; L.cin_pad[0] = pad16(channels);
        L.cout_real = channels; L.cout_pad = pad16(channels);
        for (int d = 0; d < 3; ++d) { L.s[d] = st[d]; L.in_dims[d] = in_d[d]; L.out_dims[d] = out_d[d]; }
        p.layers.push_back(L);
        return (int)p.layers.size() - 1;
    };
    // The first conv of the network.  One input channel in 3-D: the stem kernels (conv3d_thin.hip / conv3d_row.hip: the window
    // of the fp32 volume in LDS, one MFMA per 16 voxels).  More channels (multi-modal MR, a cascade's one-hot channels) or a
    // `2d` configuration (depth-1 tiles: a sixteenth of that kernel's tile): the patches' windows are first written as an fp16
    // tensor with the channels padded to 16 (patch_input_kernel, body.hip) and the stem is an ordinary conv layer on the MFMA
    // conv kernels - plan sweep, round 6: the generic multi-channel stem took 17 % (4 channels) to 55 % (14) of a forward.
    auto add_stem = [&](int cin, int cout, const int32_t *k, const int *d) {
        const bool via_conv = (cin >= 2 || a.spatial_dims == 2) && !p.switches.stem_direct;
        const int c[2] = {cin, 0};
        if (!via_conv) {
            const int src[2] = {-1, -1};
            return add_conv(Layer::STEM, 1, c, src, cout, k, one, d, d);
        }
        Layer G;
        G.type = Layer::GATHER; G.n_src = 1; G.has_norm = false;
        G.cin_real[0] = cin; G.cin_pad[0] = pad16(cin); G.cout_real = cin; G.cout_pad = pad16(cin);
        for (int q = 0; q < 3; ++q) { G.in_dims[q] = d[q]; G.out_dims[q] = d[q]; }
        p.layers.push_back(G);
        const int src[2] = {(int)p.layers.size() - 1, -1};
        const int li = add_conv(Layer::CONV, 1, c, src, cout, k, one, d, d);
        p.layers[li].bytes += 2.0 * cin * (double)d[0] * d[1] * d[2];                  // the network input is fp32 in HBM
        return li;
    };
    if (a.kind == FNN_NET_PLAIN) {
        for (int s = 0; s < a.n_stages; ++s) {
            if (a.n_conv_enc[s] < 1) return refuse(err, FNN_E_INVALID, "n_conv_per_stage must be >= 1");
            for (int i = 0; i < a.n_conv_enc[s]; ++i) {
                const int cin[2] = {prev_c, 0}, src[2] = {prev, -1};
                const bool first = (s == 0 && i == 0);
                const int *in_d = (i == 0 && s > 0) ? dims[s - 1] : dims[s];
                prev = first ? add_stem(prev_c, a.features[s], a.kernels[s], dims[s])
                             : add_conv(Layer::CONV, 1, cin, src, a.features[s], a.kernels[s], i == 0 ? a.strides[s] : one, in_d, dims[s]);
                prev_c = a.features[s];
            }
            S.enc_last[s] = prev;
        }
    } else {
        // ResidualEncoderUNet: stem conv, then per stage n_conv_enc[s] BasicBlockD blocks
        //   y = LeakyReLU(norm(conv2(act(norm(conv1(x))))) + skip(x)),  skip = [AvgPool(stride)] [1x1x1 conv (no bias) + norm]
        {
            prev = add_stem(a.in_channels, a.features[0], a.kernels[0], dims[0]);
            prev_c = a.features[0];
        }
        for (int s = 0; s < a.n_stages; ++s) {
            if (a.n_conv_enc[s] < 1) return refuse(err, FNN_E_INVALID, "n_blocks_per_stage must be >= 1");
            for (int b = 0; b < a.n_conv_enc[s]; ++b) {
                const int32_t *st = b == 0 ? a.strides[s] : one;
                const int *in_d = (b == 0 && s > 0) ? dims[s - 1] : dims[s];
                const bool strided = st[0] != 1 || st[1] != 1 || st[2] != 1;
                const int F = a.features[s];
                const int cin1[2] = {prev_c, 0}, src1[2] = {prev, -1};
                const int c1 = add_conv(Layer::CONV, 1, cin1, src1, F, a.kernels[s], st, in_d, dims[s]);
                const int cin2[2] = {F, 0}, src2[2] = {c1, -1};
                next_act = false;
                const int c2 = add_conv(Layer::CONV, 1, cin2, src2, F, a.kernels[s], one, dims[s], dims[s]);
                next_act = true;
                int skip = prev;
                if (strided) skip = add_aux(Layer::POOL, prev, -1, prev_c, st, in_d, dims[s]);
                if (prev_c != F) {
                    const int cinp[2] = {prev_c, 0}, srcp[2] = {skip, -1};
                    next_has_bias = false; next_act = false;
                    skip = add_conv(Layer::CONV, 1, cinp, srcp, F, one, one, dims[s], dims[s]);
                    next_has_bias = true; next_act = true;
                }
                prev = add_aux(Layer::COMBINE, c2, skip, F, one, dims[s], dims[s]);
                prev_c = F;
            }
            S.enc_last[s] = prev;
        }
    }
    for (int d = 0; d < a.n_stages - 1; ++d) {
        const int lvl = a.n_stages - 2 - d;           // encoder stage whose skip is consumed
        const int below = prev_c, skip = a.features[lvl];
        const int32_t *st = a.strides[lvl + 1];
        Layer T;
        T.type = Layer::TCONV; T.n_src = 1; T.has_norm = false;
        T.cin_real[0] = below; T.cin_pad[0] = pad16(below); T.src_layer[0] = prev;
        T.cout_real = skip; T.cout_pad = pad16(skip);
        for (int q = 0; q < 3; ++q) { T.k[q] = st[q]; T.s[q] = st[q]; T.in_dims[q] = dims[lvl + 1][q]; T.out_dims[q] = dims[lvl][q]; }
        const int taps = st[0] * st[1] * st[2];
        T.blob_w = blob; blob += (int64_t)below * skip * taps;
        T.blob_b = blob; blob += skip;
        T.flops = 2.0 * below * skip * (double)dims[lvl][0] * dims[lvl][1] * dims[lvl][2];
        p.layers.push_back(T);
        const int tl = (int)p.layers.size() - 1;
        if (a.n_conv_dec[d] < 1) return refuse(err, FNN_E_INVALID, "n_conv_per_stage_decoder must be >= 1");
        for (int i = 0; i < a.n_conv_dec[d]; ++i) {
            if (i == 0) {
                const int cin[2] = {skip, skip}, src[2] = {tl, S.enc_last[lvl]};
                prev = add_conv(Layer::CONV, 2, cin, src, skip, a.kernels[lvl], one, dims[lvl], dims[lvl]);
            } else {
                const int cin[2] = {skip, 0}, src[2] = {prev, -1};
                prev = add_conv(Layer::CONV, 1, cin, src, skip, a.kernels[lvl], one, dims[lvl], dims[lvl]);
            }
        }
        prev_c = skip;
    }
    p.head_src = prev;
    p.blob_head_w = blob; blob += (int64_t)a.num_heads * a.features[0];
    p.blob_head_b = blob; blob += a.num_heads;
    p.blob_count = blob;

    for (Layer &L : p.layers)
        if (L.type == Layer::STEM) {
            if (!stem_mfma_ok(L.cin_real[0], L.k[0], L.k[1], L.k[2], L.cout_pad)) return refuse(err, FNN_E_UNSUPPORTED, "stem conv shape");
            L.mfma_stem = true;
        }
    return 0;
}

// ---- fusions: launches that do a neighbour's work too
void fuse_layers(LayerPlan &p) {
    const PlanSwitches &sw = p.switches;
    if (!sw.fuse_enabled) return;
    // a residual stage's pooled skip tensor is written by the launch that forms the block output it pools (combine_pool_kernel)
    for (size_t li = 0; li < p.layers.size() && !sw.no_pool_fuse; ++li) {
        Layer &L = p.layers[li];
        if (L.type != Layer::POOL) continue;
        Layer &Cb = p.layers[L.src_layer[0]];
        if (Cb.type == Layer::COMBINE && combine_pool_ok(L.in_dims[0], L.in_dims[1], L.in_dims[2], L.s[0], L.s[1], L.s[2])) {
            Cb.pool_layer = (int)li; L.pool_fused = true;
        }
    }
    // producers recomputed inside their consumer's staging (conv3d_thin.hip, conv3d_row.hip): where a kernel takes the fused layer
    if (p.arch.spatial_dims == 2) return;
    std::vector<int> consumers(p.layers.size(), 0);
    for (const Layer &L : p.layers)
        for (int i = 0; i < L.n_src; ++i) if (L.src_layer[i] >= 0) consumers[L.src_layer[i]]++;
    for (Layer &L : p.layers) {
        if (L.type != Layer::CONV || L.src_layer[0] < 0) continue;
        Layer &P = p.layers[L.src_layer[0]];
        if (consumers[L.src_layer[0]] != 1 || P.cout_pad != 16) continue;
        ConvChoice c;
        if (sw.fuse_stem != 0 && L.n_src == 1 && P.type == Layer::STEM && P.mfma_stem && P.cin_real[0] == 1 && P.k[0] == L.k[0] &&
            conv_choose(p.conv_shape(L, FUSE_STEM), sw.ov, c)) {
            // by default only where the row kernels take both halves: conv_row_stem_kernel + stem_row_kernel (statistics)
            StemParams sp{};
            sp.C = P.cin_real[0]; sp.kd = P.k[0]; sp.kh = P.k[1]; sp.kw = P.k[2]; sp.Cout = P.cout_pad;
            sp.PD = P.out_dims[0]; sp.PH = P.out_dims[1]; sp.PW = P.out_dims[2];
            if (sw.fuse_stem == 1 || (c.kernel == CK_ROW_STEM && stem_row_ok(sp))) { L.fuse = FUSE_STEM; L.cc = c; P.virtual_out = true; }
        } else if (L.n_src == 2 && P.type == Layer::TCONV && conv_choose(p.conv_shape(L, FUSE_TCONV, &P), sw.ov, c)) {
            L.fuse = FUSE_TCONV; L.cc = c; P.virtual_out = true;
        }
    }
}

// ---- activation layouts: a tensor of more than 16 channels that only conv / transposed-conv kernels read is stored
// chunk-major, so that a consumer's 16-channel chunk is whole cache lines instead of 32 bytes of every record
void choose_layouts(LayerPlan &p) {
    if (p.switches.no_chunk_major) return;
    std::vector<int> ok(p.layers.size(), 1);
    for (const Layer &L : p.layers)
        for (int i = 0; i < L.n_src; ++i)
            if (L.src_layer[i] >= 0 && L.type != Layer::CONV && L.type != Layer::TCONV && L.type != Layer::POOL &&
                L.type != Layer::COMBINE) ok[L.src_layer[i]] = 0;
    for (size_t li = 0; li < p.layers.size(); ++li) {
        Layer &L = p.layers[li];
        L.chunk_major = ok[li] && (int)li != p.head_src &&
                        (L.type == Layer::CONV || L.type == Layer::TCONV || L.type == Layer::POOL || L.type == Layer::COMBINE) &&
                        L.cout_pad > p.switches.cm_min && p.arch.spatial_dims != 2;
    }
}

// ---- device offsets and totals; an unfused conv layer gets its kernel here, because the kernel sizes its packed weights
// and its statistics rows
int place_layers(LayerPlan &p, const Stages &S, std::string &err) {
    const fnn_arch_desc &a = p.arch;
    const ConvOverrides &ov = p.switches.ov;
    size_t wpk = 0, fp = 0, st = 0, act = 0, ssn = 0;
    double flops = 0, bytes = 0;
    for (Layer &L : p.layers) {
        const size_t ovox = (size_t)L.out_dims[0] * L.out_dims[1] * L.out_dims[2];
        if (L.type == Layer::STEM) {
            const int T = L.k[0] * L.k[1] * L.k[2];
            L.w_off = fp; fp += (size_t)L.cin_real[0] * T * L.cout_pad;
            if (L.mfma_stem) { L.w_off2 = wpk; wpk += (size_t)(L.cout_pad / 16) * stem_mfma_ksteps(L.cin_real[0], L.k[0] * L.k[1] * L.k[2]) * 512; }
        } else if (L.type == Layer::CONV) {
            if (!L.fuse) {
                ThinParams tp = p.conv_shape(L);
                // e4m3 operands where conv_choose_fp8 lets them stick (the stride-1 3x3x3 layers the fp8 ZR kernel takes)
                tp.c.fp8 = a.precision == FNN_PREC_F8 &&
                           !(L.src_layer[0] >= 0 && p.layers[L.src_layer[0]].type == Layer::GATHER);   // (the network input keeps fp16: the stem was never an fp8 layer)
                if (tp.c.fp8 && ov.fp8_levels >= 0) {
                    // sensitivity studies (tools/fp8_sensitivity.py): e4m3 operands only at the resolution levels of the bit mask
                    // (level = how many times the patch's voxel count was divided by ~8 on the way to this layer's output)
                    const double P = (double)a.patch[0] * a.patch[1] * a.patch[2];
                    const int level = (int)std::lround(std::log2(P / (double)ovox) / 3.0);
                    tp.c.fp8 = ((ov.fp8_levels >> level) & 1) != 0;
                }
                const bool ok = conv_choose_fp8(tp, ov, L.cc);
                if (!ok) return refuse(err, FNN_E_UNSUPPORTED, "no conv kernel takes layer %zu (%dx%dx%d, stride %dx%dx%d, %d -> %d channels)",
                                       (size_t)(&L - p.layers.data()), L.k[0], L.k[1], L.k[2], L.s[0], L.s[1], L.s[2], tp.c.chunks * 16, L.cout_pad);
                L.fp8 = tp.c.fp8 != 0;
            }
            L.w_off = wpk; wpk += conv_packed_halves(L.cc, L.cout_pad);
        } else if (L.type == Layer::TCONV) {
            const int taps = L.s[0] * L.s[1] * L.s[2];
            L.ksteps = (L.cin_pad[0] + 31) / 32;
            L.w_off = wpk; wpk += (size_t)taps * (L.cout_pad / 16) * L.ksteps * 512;
        }
        L.bias_off = fp; fp += L.cout_pad;
        if (L.fp8) { L.oscale_off = fp; fp += L.cout_pad; }
        if (L.has_norm) { L.gamma_off = fp; fp += L.cout_pad; L.beta_off = fp; fp += L.cout_pad; }
        L.stats_slots = FNN_STAT_REPL;
        if (L.type == Layer::STEM) L.stats_slots = stem_mfma_stats_slots(L.out_dims[0], L.out_dims[1], L.out_dims[2]);
        else if (L.type == Layer::CONV) L.stats_slots = L.cc.stats_slots;
        L.stats_off = st; if (L.has_norm) st += (size_t)L.stats_slots * L.cout_pad * 2;
        L.ss_off = ssn; if (L.has_norm) ssn += L.cout_pad;
        L.out_off = act; act += ovox * L.cout_pad;
        flops += L.flops;
        bytes += 2.0 * ovox * L.cout_real * 2.0;            // written once + read once, fp16
    }
    p.hblocks = (a.num_heads + 1 + 15) / 16;                // + the weight-sum channel (zero weights, bias 1: its "logit" is 1)
    p.head_ksteps = (pad16(a.features[0]) + 31) / 32;
    p.head_w_off = wpk; wpk += (size_t)p.hblocks * p.head_ksteps * 512;
    p.head_bias_off = fp; fp += (size_t)p.hblocks * 16;
    p.n_gpass = (a.num_heads + 62) / 63;
    if (p.n_gpass > 1) {
        p.gpass_w_off = wpk; wpk += (size_t)p.n_gpass * 4 * 512;
        p.gpass_bias_off = fp; fp += (size_t)p.n_gpass * 64;
    }
    const double P = (double)a.patch[0] * a.patch[1] * a.patch[2];
    p.head_flops = 2.0 * a.num_heads * a.features[0] * P;
    p.patch_flops = flops + p.head_flops;
    // skips are read twice (next encoder stage and decoder); network input read once
    for (int s = 0; s < a.n_stages - 1; ++s) {
        const Layer &L = p.layers[S.enc_last[s]];
        bytes += (double)L.out_dims[0] * L.out_dims[1] * L.out_dims[2] * L.cout_real * 2.0;
    }
    p.patch_act_bytes = bytes;
    p.wpk_halves = wpk; p.fparam_floats = fp; p.stats_doubles = st; p.act_halves = act; p.ss_count = ssn;
    return 0;
}

}  // namespace

int plan_layers(const fnn_arch_desc &arch, int max_batch, const PlanSwitches &sw, LayerPlan &out, std::string &err) {
    out = LayerPlan{};
    out.arch = arch; out.max_batch = max_batch; out.switches = sw;
    if (out.arch.eps <= 0) out.arch.eps = 1e-5f;
    Stages S;
    if (int rc = validate(out.arch, max_batch, S, err)) return rc;
    if (int rc = list_layers(out, S, err)) return rc;
    fuse_layers(out);
    choose_layouts(out);
    return place_layers(out, S, err);
}

// ---------------------------------------------------------------------------
// weight packing (host)
// ---------------------------------------------------------------------------
// (declared in fnn_device.h: the single-op entry points pack a head the same way)
void pack_head(int heads, int cin, int hblocks, int ksteps, const float *W, unsigned short *dst) {
    for (int hb = 0; hb < hblocks; ++hb)
        for (int ks = 0; ks < ksteps; ++ks)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int ci = ks * 32 + 8 * (lane >> 4) + j, h = hb * 16 + (lane & 15);
                    float v = 0.f;
                    if (ci < cin && h < heads) v = W[(size_t)h * cin + ci];
                    dst[(((size_t)hb * ksteps + ks) * 64 + lane) * 8 + j] = fnn_half_bits(v);
                }
}

// bias row of the head kernels, [hblocks * 16]: the heads' biases, then the weight-sum channel (zero weights in pack_head,
// bias 1: its "logit" is 1 and 1 * gaussian is the weight itself), zeros behind it
void pack_head_bias(int heads, int hblocks, const float *bias, float *dst) {
    for (int h = 0; h < hblocks * 16; ++h) dst[h] = h < heads ? (bias ? bias[h] : 0.f) : (h == heads ? 1.f : 0.f);
}

void pack_fold_weights(const LayerPlan &p, const float *blob, std::vector<uint16_t> &wpk, std::vector<float> &fp) {
    wpk.assign(p.wpk_halves, 0);
    fp.assign(p.fparam_floats, 0.f);
    for (const Layer &L : p.layers) {
        if (L.type == Layer::POOL || L.type == Layer::COMBINE || L.type == Layer::GATHER) continue;
        const float *W = blob + L.blob_w;
        if (L.type == Layer::STEM) {
            const int T = L.k[0] * L.k[1] * L.k[2], C = L.cin_real[0];
            for (int c = 0; c < C; ++c)
                for (int t = 0; t < T; ++t)
                    for (int co = 0; co < L.cout_real; ++co)
                        fp[L.w_off + ((size_t)c * T + t) * L.cout_pad + co] = W[((size_t)co * C + c) * T + t];
            if (L.mfma_stem) stem_mfma_pack(W, C, T, L.cout_real, L.cout_pad, wpk.data() + L.w_off2);
        } else if (L.type == Layer::CONV) {
            conv_pack_weights(p.conv_shape(L).c, L.cc, L.cout_real, L.cin_real, W, wpk.data() + L.w_off,
                              L.fp8 ? fp.data() + L.oscale_off : nullptr);
        } else {
            tconv_pack_weights(W, L.cin_real[0], L.cout_real, L.cout_pad, L.s[0] * L.s[1] * L.s[2], L.ksteps, wpk.data() + L.w_off);
        }
        for (int c = 0; c < L.cout_real; ++c) {
            // A conv bias in front of an InstanceNorm cancels exactly (the norm removes the channel mean), so it is
            // dropped: the raw conv outputs are stored in fp16, and a large bias would only cost them resolution
            // (|bias| = 10 in front of a unit-variance channel: 2^-7 instead of 2^-11 of sigma).
            fp[L.bias_off + c] = (L.has_bias && !L.has_norm) ? blob[L.blob_b + c] : 0.f;
            if (L.has_norm) { fp[L.gamma_off + c] = blob[L.blob_g + c]; fp[L.beta_off + c] = blob[L.blob_beta + c]; }
        }
    }
    const int heads = p.arch.num_heads, cin = p.arch.features[0];
    pack_head(heads, cin, p.hblocks, p.head_ksteps, blob + p.blob_head_w, wpk.data() + p.head_w_off);
    pack_head_bias(heads, p.hblocks, blob + p.blob_head_b, fp.data() + p.head_bias_off);
    for (int k = 0; k < (p.n_gpass > 1 ? p.n_gpass : 0); ++k) {        // gather passes: heads 63 k .. + cnt - 1, then the weight-sum row
        const int h0 = 63 * k, cnt = std::min(63, heads - h0);
        pack_head(cnt, cin, 4, 1, blob + p.blob_head_w + (size_t)h0 * cin, wpk.data() + p.gpass_w_off + (size_t)k * 4 * 512);
        for (int h = 0; h < cnt; ++h) fp[p.gpass_bias_off + (size_t)k * 64 + h] = blob[p.blob_head_b + h0 + h];
        fp[p.gpass_bias_off + (size_t)k * 64 + cnt] = 1.f;
    }
}

std::string layer_table_text(const LayerPlan &p) {
    static const char *const ty[] = {"stem", "conv", "tconv", "pool", "combine", "input"};
    std::string all;
    for (size_t li = 0; li < p.layers.size(); ++li) {
        const Layer &L = p.layers[li];
        char row[320];
        snprintf(row, sizeof row, "%zu\t%s\t%d\t%d\t%dx%dx%d\t%dx%dx%d\t%dx%dx%d\t%dx%dx%d\t%.6g\t%.6g\t%d\t%s\n", li, ty[L.type],
                 L.cin_real[0] + (L.n_src > 1 ? L.cin_real[1] : 0), L.cout_real, L.k[0], L.k[1], L.k[2], L.s[0], L.s[1], L.s[2],
                 L.in_dims[0], L.in_dims[1], L.in_dims[2], L.out_dims[0], L.out_dims[1], L.out_dims[2], L.flops, L.bytes,
                 L.virtual_out ? 1 : (L.fuse ? 2 : 0), L.type == Layer::CONV ? L.cc.name : "-");
        all += row;
    }
    return all;
}
