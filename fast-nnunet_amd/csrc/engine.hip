// engine.hip - host side of the C ABI in include/fnn.h.
//
// Owns what runs: the activation / statistics / accumulator arenas in HBM, the
// folds' packed weights, the streams, and the sliding-window driver that replaces
// predict_from_raw_data.py:560-680 (x-major patch order, Gaussian weighting,
// accumulate, normalise, un-pad; mirroring; fold ensembling).  What the network
// is - the layer list, the kernel per conv layer, every offset - is the
// LayerPlan (layer_plan.h) that fnn_create makes once and everything here reads.
#include "fnn_device.h"
#include "layer_plan.h"
#include "host_upload.h"
#include "../../include/fnn.h"

#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <algorithm>
#include <climits>
#include <memory>
#include <vector>
#include <variant>

namespace {

thread_local std::string g_err;

struct FoldWeights {
    DevBuf wpk, fparam;                // f16 fragments; floats
    bool loaded = false;
};

// What one batch in flight writes: every layer's activations, the InstanceNorm statistics, and the (scale, shift) rows -
// fp32 [layer][max_batch][2][C], followed by the same rows in fp16 (ssh_rows)
struct Arena {
    DevBuf act, stats, ss;             // f16; double; float
};

// z pitch of the volume accumulators: rows start 16-byte aligned for the vectorised read-modify-write
inline long long zpitch(long long z) { return (z + 7) / 8 * 8; }

}  // namespace

struct fnn_engine {
    const LayerPlan plan;                   // what the network is: made by fnn_create before the engine, fixed for its life
    explicit fnn_engine(LayerPlan &&p) : plan(std::move(p)) {}
    int device = 0;
    std::string err;
    std::vector<FoldWeights> folds;
    // Batches in flight (fnn_accumulate / predict): one arena and one internal stream per batch in flight
    // (four by default since round 6, FNN_PIPES = 2..8; measured 2 -> 3: +1.5 %, 3 -> 4: +0.3 ... +0.9 %, beyond: nothing).  The network alternates between
    // HBM-bound (thin full-resolution convs, seg head) and MFMA-bound kernels; with the following batches' forwards on
    // the other streams they overlap.  The heads stay ordered (events), so the accumulation order - and with it every
    // rounding - is the reference's.  288 GB of HBM make the extra arenas free.
    static constexpr int MAXP = 8;
    struct Pipe { Arena arena; Stream st; Event head, done; };
    Pipe pipe[MAXP];                        // arena [0]: fnn_create's, the one a single stream uses; [k > 0]: add_pipes
    int n_pipe = 0;                         // streams allocated (0 until the first multi-batch run); arenas 1 .. n_pipe - 1 with them
    Event ev_start;
    // Every buffer below is made where it is first needed and only ever grows (DevBuf::reserve)
    DevBuf gauss;                           // f16
    DevBuf ones;                            // f16: weight map of use_gaussian = 0 (the kernels load the map unconditionally)
    DevBuf inf_flag;                        // int
    // label rule of the label-map entry points (fnn_set_label_rule)
    int label_mode = FNN_LABELS_ARGMAX, label_u16 = 0;
    DevBuf label_order;                     // int: regions_class_order[num_heads]
    IntTable origins;                       // the patches' origins, [n][3]
    DevBuf acc;
    DevBuf vol_tmp;                         // float: a host caller's volume / patches
    HostUpload up;                          // a volume that arrives in host memory, on its way into vol_tmp (host_upload.h)
    DevBuf vol_pad;                         // float
    DevBuf out_tmp;
    DevBuf patch_buf;                       // float
    // gather path (gather.hip): the last conv's raw output and InstanceNorm of every patch of the volume
    DevBuf feat, featss;
    DevBuf featssh;                         // the same rows in fp16, staging layout (GatherParams::fssh)
    IntTable steps;                         // the tile-start / slot tables
    std::vector<std::string> klog;          // kernel variants of the last profiled call, one entry per launch (fnn_kernel_log)
    bool gather_enabled = true;             // FNN_NO_GATHER (read when the engine is created): always accumulate in HBM
    // profiling
    bool profiling = false;
    struct Ev { Event a, b; int family; double flops, bytes; int layer; size_t klog_lo, klog_hi; };
    std::vector<Ev> evs; size_t ev_used = 0;
    int cur_layer = -1;                     // layer index of the launches being issued (-1: head / gather / finalize)
    std::vector<std::string> launch_rows;   // fnn_profile_launches: one row per timed launch of the last profiled call
    fnn_profile prof{};
};

// what the entry points that have no engine handle share (fnn_device.h)
void fnn_set_global_error(const char *msg) { g_err = msg ? msg : ""; }
int fnn_fail(int code, const char *msg) { fnn_set_global_error(msg); return code; }
bool fnn_dev_ptr(const void *p) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

namespace {

int fail(fnn_engine *e, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    if (e) e->err = buf;
    return code;
}

#define HIPCHK(e, call)                                                                              \
    do {                                                                                             \
        hipError_t _r = (call);                                                                      \
        if (_r != hipSuccess) return fail(e, FNN_E_HIP, "%s failed: %s", #call, hipGetErrorString(_r)); \
    } while (0)

int arena_alloc(fnn_engine *e, Arena &A) {
    size_t b[3];
    e->plan.arena_bytes(b);
    DevBuf *const buf[3] = {&A.act, &A.stats, &A.ss};
    static const char *const name[3] = {"activations", "stats", "scale/shift"};
    for (int i = 0; i < 3; ++i)
        if (hipError_t r = buf[i]->reserve(b[i])) { A = Arena{}; return fail(e, FNN_E_HIP, "hipMalloc(%s) failed: %s", name[i], hipGetErrorString(r)); }
    return 0;
}

// ---------------------------------------------------------------------------
// profiling helpers
// ---------------------------------------------------------------------------
enum { FAM_CONV = 0, FAM_STEM, FAM_TCONV, FAM_HEAD, FAM_FINAL };

struct Scope {
    fnn_engine *e; hipStream_t st; int idx = -1;
    Scope(fnn_engine *e_, hipStream_t st_, int family, double flops, double bytes = 0) : e(e_), st(st_) {
        fnn_klog_target(e->profiling ? &e->klog : nullptr);  // the launchers inside this scope note their kernel variant
        if (!e->profiling) return;
        if (e->ev_used == e->evs.size()) {
            fnn_engine::Ev ev{};
            if (ev.a.create(hipEventDefault) != hipSuccess || ev.b.create(hipEventDefault) != hipSuccess) return;
            e->evs.push_back(std::move(ev));
        }
        idx = (int)e->ev_used++;
        e->evs[idx].family = family; e->evs[idx].flops = flops; e->evs[idx].bytes = bytes;
        e->evs[idx].layer = e->cur_layer; e->evs[idx].klog_lo = e->evs[idx].klog_hi = e->klog.size();
        (void)hipEventRecord(e->evs[idx].a, st);
    }
    ~Scope() { if (idx >= 0) { (void)hipEventRecord(e->evs[idx].b, st); e->evs[idx].klog_hi = e->klog.size(); } }
};

void collect_profile(fnn_engine *e, int64_t n_patches) {
    fnn_profile &p = e->prof;
    p = fnn_profile{};
    p.n_patches = n_patches;
    e->launch_rows.clear();
    for (size_t i = 0; i < e->ev_used; ++i) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, e->evs[i].a, e->evs[i].b) != hipSuccess) continue;
        p.total_ms += ms;
        {
            static const char *const fam[] = {"conv", "stem", "tconv", "head", "finalize"};
            const fnn_engine::Ev &v = e->evs[i];
            char row[320];
            std::string names;
            for (size_t k = v.klog_lo; k < v.klog_hi && k < e->klog.size(); ++k) { if (!names.empty()) names += " + "; names += e->klog[k]; }
            snprintf(row, sizeof row, "%d\t%s\t%.6f\t%.6g\t%.6g\t%s", v.layer, fam[v.family >= 0 && v.family <= 4 ? v.family : 4],
                     (double)ms, v.flops, v.bytes, names.c_str());
            e->launch_rows.push_back(row);
        }
        switch (e->evs[i].family) {
            case FAM_CONV: p.conv_ms += ms; p.conv_launches++; p.conv_flops += e->evs[i].flops; p.conv_bytes += e->evs[i].bytes; break;
            case FAM_STEM: p.stem_ms += ms; break;
            case FAM_TCONV: p.tconv_ms += ms; break;
            case FAM_HEAD: p.head_ms += ms; break;
            default: p.finalize_ms += ms; break;
        }
    }
    e->ev_used = 0;
}

// ---------------------------------------------------------------------------
// one network forward for `nb` patches (activations only; the head is separate)
// ---------------------------------------------------------------------------
// the fp16 scale / shift rows (SrcDesc::ssh) live behind the fp32 rows of the same arena: [ss_count * max_batch * 2 + 4] floats,
// then ss_count * max_batch * 2 halves
unsigned short *ssh_rows(const fnn_engine *e, const Arena &A) { return (unsigned short *)(A.ss.as<float>() + e->plan.ss_count * e->plan.max_batch * 2 + 4); }


SrcDesc make_src(const fnn_engine *e, const Arena &A, int layer) {
    const Layer &L = e->plan.layers[layer];
    SrcDesc s{};
    s.ptr = A.act.as<f16>() + L.out_off * e->plan.max_batch;
    s.C = L.cout_pad;
    const Layout lay = LayerPlan::layout(L);
    s.vs = lay.vs ? lay.vs : L.cout_pad; s.cs = lay.vs ? lay.cs : 16;   // (spelled out: a one-source conv's src[1] is a copy with C = 0)
    if (L.has_norm) {
        s.ss = A.ss.as<float>() + L.ss_off * e->plan.max_batch * 2;
        s.ssh = ssh_rows(e, A) + L.ss_off * e->plan.max_batch * 2;        // halves: [N][C / 8][16] = 2 C per item
        s.slope = L.act ? e->plan.arch.slope : 1.f;
    } else {
        s.ss = nullptr; s.ssh = nullptr; s.slope = 1.f;
    }
    return s;
}

// One batch's forward in arena A.  head_out / head_ss: where the network's last layer writes its raw output and its
// (scale, shift) rows instead of the arena (the gather path keeps them per patch)
int forward_batch(fnn_engine *e, int fold, const Arena &A, const float *vol, long long vol_batch_stride, const long long vdim[3],
                  const int *origins_dev, int nb, const int flip[3], hipStream_t st, f16 *head_out = nullptr,
                  float *head_ss = nullptr, unsigned short *head_ssh = nullptr) {
    f16 *const wpk = e->folds[fold].wpk.as<f16>(), *const act = A.act.as<f16>();
    float *const fparam = e->folds[fold].fparam.as<float>(), *const ss = A.ss.as<float>();
    const LayerPlan &plan = e->plan;
    double *const stats = A.stats.as<double>();
    HIPCHK(e, hipMemsetAsync(stats, 0, plan.stats_doubles * plan.max_batch * sizeof(double), st));
    struct LayerMark { fnn_engine *e; ~LayerMark() { e->cur_layer = -1; } } mark{e};
    for (size_t li = 0; li < plan.layers.size(); ++li) {
        const Layer &L = plan.layers[li];
        e->cur_layer = (int)li;
        f16 *out = act + L.out_off * plan.max_batch;
        if (head_out && (int)li == plan.head_src) out = head_out;
        const Layout lay = LayerPlan::layout(L);
        double *stats_out = L.has_norm ? stats + L.stats_off * plan.max_batch : nullptr;
        int rc = 0;
        if (L.type == Layer::STEM) {
            StemParams p{};
            p.vol = vol; p.vol_batch_stride = vol_batch_stride; p.C = L.cin_real[0];
            p.X = vdim[0]; p.Y = vdim[1]; p.Z = vdim[2];
            p.origins = origins_dev;
            p.flip_d = flip[0]; p.flip_h = flip[1]; p.flip_w = flip[2];
            p.PD = L.out_dims[0]; p.PH = L.out_dims[1]; p.PW = L.out_dims[2];
            p.kd = L.k[0]; p.kh = L.k[1]; p.kw = L.k[2];
            p.Cout = L.cout_pad;
            p.w = fparam + L.w_off; p.bias = fparam + L.bias_off;
            p.out = out; p.stats_out = stats_out;
            Scope sc(e, st, FAM_STEM, L.flops * nb, L.bytes * nb);
            if (L.virtual_out) p.out = nullptr;                       // statistics only: the consumer recomputes the values
            rc = launch_stem_mfma(p, wpk + L.w_off2, nb, st);
        } else if (L.type == Layer::CONV) {
            const Layer *P = L.fuse ? &plan.layers[L.src_layer[0]] : nullptr;        // the producer a fused layer recomputes
            ThinParams tp = plan.conv_shape(L, L.fuse, L.fuse == FUSE_TCONV ? P : nullptr);
            ConvParams &p = tp.c;
            p.N = nb;
            for (int i = 0; i < L.n_src; ++i) p.src[i] = make_src(e, A, L.src_layer[i]);
            if (L.n_src == 1) { p.src[1] = p.src[0]; p.src[1].C = 0; }
            p.pd = (L.k[0] - 1) / 2; p.ph = (L.k[1] - 1) / 2; p.pw = (L.k[2] - 1) / 2;
            p.wpk = wpk + L.w_off; p.bias = fparam + L.bias_off;
            p.out = out; p.stats_out = stats_out;
            p.out_vs = lay.vs; p.out_cs = lay.cs;
            p.oscale = L.fp8 ? fparam + L.oscale_off : nullptr; p.act_mult = FNN_FP8_ACT_MULT;
            Scope sc(e, st, FAM_CONV, L.flops * nb, L.bytes * nb);
            if (L.fuse) {
                tp.fbias = fparam + P->bias_off;
                if (L.fuse == FUSE_STEM) {
                    tp.fw = wpk + P->w_off2;
                    tp.vol = vol; tp.vol_batch_stride = vol_batch_stride; tp.Y = vdim[1]; tp.Z = vdim[2];
                    tp.origins = origins_dev; tp.flip_d = flip[0]; tp.flip_h = flip[1]; tp.flip_w = flip[2];
                    tp.fss = ss + P->ss_off * plan.max_batch * 2; tp.fslope = plan.arch.slope;
                } else {
                    tp.fw = wpk + P->w_off;
                    tp.low = make_src(e, A, P->src_layer[0]);
                }
            }
            rc = launch_conv(tp, L.cc, st);
        } else if (L.type == Layer::GATHER) {
            PatchInputParams p{};
            p.vol = vol; p.vol_batch_stride = vol_batch_stride; p.C = L.cin_real[0]; p.Cpad = L.cout_pad;
            p.X = vdim[0]; p.Y = vdim[1]; p.Z = vdim[2];
            p.origins = origins_dev;
            p.flip_d = flip[0]; p.flip_h = flip[1]; p.flip_w = flip[2];
            p.PD = L.out_dims[0]; p.PH = L.out_dims[1]; p.PW = L.out_dims[2]; p.N = nb;
            p.out = out; p.out_vs = lay.vs; p.out_cs = lay.cs;
            Scope sc(e, st, FAM_STEM, 0, 2.0 * nb * (2.0 * L.cin_real[0] + L.cout_pad) * L.out_dims[0] * L.out_dims[1] * L.out_dims[2]);
            rc = launch_patch_input(p, st);
        } else if (L.type == Layer::POOL) {
            if (L.pool_fused) continue;                               // written by the COMBINE launch of its source
            PoolParams p{};
            p.src = make_src(e, A, L.src_layer[0]);
            p.N = nb; p.Di = L.in_dims[0]; p.Hi = L.in_dims[1]; p.Wi = L.in_dims[2];
            p.sd = L.s[0]; p.sh = L.s[1]; p.sw = L.s[2];
            p.out = out; p.out_vs = lay.vs; p.out_cs = lay.cs;
            Scope sc(e, st, FAM_TCONV, 0);
            rc = launch_avgpool(p, st);
        } else if (L.type == Layer::COMBINE) {
            CombineParams p{};
            p.a = make_src(e, A, L.src_layer[0]);
            p.b = make_src(e, A, L.src_layer[1]);
            p.vox = (long long)L.out_dims[0] * L.out_dims[1] * L.out_dims[2];
            p.N = nb; p.slope = plan.arch.slope; p.out = out; p.out_vs = lay.vs; p.out_cs = lay.cs;
            if (L.pool_layer >= 0) {
                const Layer &P = plan.layers[L.pool_layer];
                const Layout pool = LayerPlan::layout(P);
                p.pool_out = act + P.out_off * plan.max_batch;
                p.D = L.out_dims[0]; p.H = L.out_dims[1]; p.W = L.out_dims[2];
                p.psd = P.s[0]; p.psh = P.s[1]; p.psw = P.s[2];
                p.pool_vs = pool.vs; p.pool_cs = pool.cs;
            }
            Scope sc(e, st, FAM_TCONV, 0);
            rc = launch_combine(p, st);
        } else {
            TconvParams p{};
            p.src = make_src(e, A, L.src_layer[0]);
            p.N = nb; p.Di = L.in_dims[0]; p.Hi = L.in_dims[1]; p.Wi = L.in_dims[2];
            p.sd = L.s[0]; p.sh = L.s[1]; p.sw = L.s[2];
            p.Cout = L.cout_pad; p.wpk = wpk + L.w_off; p.bias = fparam + L.bias_off;
            p.out = out; p.out_vs = lay.vs; p.out_cs = lay.cs; p.ksteps = L.ksteps; p.nblk = L.cout_pad / 16;
            if (L.virtual_out) continue;                              // computed inside its consumer (conv3d_thin.hip)
            Scope sc(e, st, FAM_TCONV, L.flops * nb);
            rc = launch_tconv(p, st);
        }
        if (rc != 0) return fail(e, rc == -1 ? FNN_E_UNSUPPORTED : FNN_E_HIP, "kernel launch failed at layer %zu (rc=%d)", li, rc);
        if (L.has_norm) {
            StatsFinalizeParams q{};
            q.stats = stats_out; q.gamma = fparam + L.gamma_off; q.beta = fparam + L.beta_off;
            q.ss = ss + L.ss_off * plan.max_batch * 2; q.C = L.cout_pad; q.nrep = L.stats_slots;
            q.ssh = ssh_rows(e, A) + L.ss_off * plan.max_batch * 2;
            if (head_ss && (int)li == plan.head_src) q.ss = head_ss;
            if (head_ssh && (int)li == plan.head_src) q.ssh = head_ssh;
            q.inv_count = 1.f / ((float)L.out_dims[0] * L.out_dims[1] * L.out_dims[2]); q.eps = plan.arch.eps;
            if (launch_stats_finalize(q, nb, st) != 0) return fail(e, FNN_E_HIP, "stats finalize launch failed");
        }
    }
    return 0;
}

HeadParams make_head(const fnn_engine *e, const Arena &A, int fold, int b) {
    const fnn_arch_desc &a = e->plan.arch;
    const FoldWeights &fw = e->folds[fold];
    HeadParams h{};
    h.src = make_src(e, A, e->plan.head_src);
    h.b = b; h.PD = a.patch[0]; h.PH = a.patch[1]; h.PW = a.patch[2];
    h.heads = a.num_heads; h.hblocks = e->plan.hblocks; h.ksteps = e->plan.head_ksteps;
    h.wpk = fw.wpk.as<f16>() + e->plan.head_w_off; h.bias = fw.fparam.as<float>() + e->plan.head_bias_off;
    h.fx = h.fy = h.fz = INT_MAX;                           // every voxel is read unless run_patches knows better
    return h;
}

int steps_1d(int64_t image, int64_t patch, double step, std::vector<int64_t> &out) {
    // compute_steps_for_sliding_window (sliding_window_prediction.py:30-54), one axis
    if (!(step > 0 && step <= 1) || patch <= 0 || image < patch) return -1;
    const double target = (double)patch * step;
    const int64_t n = (int64_t)std::ceil((double)(image - patch) / target) + 1;
    out.clear();
    if (n > 1) {
        const double actual = (double)(image - patch) / (double)(n - 1);
        for (int64_t i = 0; i < n; ++i) out.push_back((int64_t)std::nearbyint(actual * (double)i));   // half-to-even
    } else {
        out.push_back(0);
    }
    return 0;
}

struct VolPlan {
    int64_t padded[3], lo[3];
    std::vector<int64_t> steps[3];
    std::vector<int> origins;          // [n][3], x-major (predict_from_raw_data.py:532-537)
    int64_t n_patches = 0;
};

// _internal_get_sliding_window_slicers (:506-538): padding to >= patch, tile starts per axis, x-major order.
// two_d: the `2d` branch (:508-524) - the first axis is not tiled, every slice is visited once.
int plan_volume_p(const int32_t patch[3], const int64_t sp[3], double step, bool two_d, VolPlan &vp) {
    for (int d = 0; d < 3; ++d) {
        if (two_d && d == 0) {
            if (sp[0] < 1) return -1;
            vp.padded[0] = sp[0]; vp.lo[0] = 0;
            vp.steps[0].clear();
            for (int64_t i = 0; i < sp[0]; ++i) vp.steps[0].push_back(i);
            continue;
        }
        if (sp[d] < 1 || patch[d] < 1) return -1;
        const int64_t target = sp[d] > patch[d] ? sp[d] : patch[d];
        const int64_t diff = target - sp[d];
        vp.padded[d] = target; vp.lo[d] = diff / 2;        // the odd voxel goes to the high side
        if (steps_1d(target, patch[d], step, vp.steps[d]) != 0) return -1;
    }
    vp.origins.clear();
    for (int64_t x : vp.steps[0])
        for (int64_t y : vp.steps[1])
            for (int64_t z : vp.steps[2]) { vp.origins.push_back((int)x); vp.origins.push_back((int)y); vp.origins.push_back((int)z); }
    vp.n_patches = (int64_t)vp.origins.size() / 3;
    return 0;
}

// The plan of a call's volume (shape [C][X][Y][Z]); the call fails when the shape and the step size make none
int plan_volume(fnn_engine *e, const int64_t shape[4], const fnn_opts &o, VolPlan &vp) {
    if (plan_volume_p(e->plan.arch.patch, shape + 1, o.tile_step_size, e->plan.arch.spatial_dims == 2, vp) != 0)
        return fail(e, FNN_E_INVALID, "invalid volume shape / step size");
    return 0;
}

// mirror-axis subsets in the reference's order: by size, then lexicographic (:551-553)
std::vector<std::vector<int>> mirror_combos(const fnn_opts &o) {
    std::vector<std::vector<int>> out;
    const int n = o.n_mirror_axes;
    // enumerate combinations of positions in lexicographic order
    for (int size = 1; size <= n; ++size) {
        std::vector<int> idx(size);
        for (int i = 0; i < size; ++i) idx[i] = i;
        while (true) {
            std::vector<int> c;
            for (int i : idx) c.push_back(o.mirror_axes[i]);
            out.push_back(c);
            int i = size - 1;
            while (i >= 0 && idx[i] == n - size + i) --i;
            if (i < 0) break;
            ++idx[i];
            for (int j = i + 1; j < size; ++j) idx[j] = idx[j - 1] + 1;
        }
    }
    return out;
}

int check_ready(fnn_engine *e, int fold, const fnn_opts *o) {
    if (!e) return FNN_E_INVALID;
    if (!o) return fail(e, FNN_E_INVALID, "opts is NULL");
    if (fold < 0 || fold >= (int)e->folds.size() || !e->folds[fold].loaded) return fail(e, FNN_E_STATE, "weights of fold %d are not loaded", fold);
    if (!(o->tile_step_size > 0 && o->tile_step_size <= 1)) return fail(e, FNN_E_INVALID, "step_size must be larger than 0 and smaller or equal to 1");
    if (o->use_gaussian && !e->gauss.p) return fail(e, FNN_E_STATE, "use_gaussian is set but fnn_set_gaussian was not called");
    if (o->n_mirror_axes < 0 || o->n_mirror_axes > 3) return fail(e, FNN_E_INVALID, "n_mirror_axes out of range");
    for (int i = 0; i < o->n_mirror_axes; ++i)
        if (o->mirror_axes[i] < 0 || o->mirror_axes[i] > 2) return fail(e, FNN_E_INVALID, "mirror_axes does not match the dimension of the input!");
    if (o->accum < FNN_ACC_FP16_REFERENCE || o->accum > FNN_ACC_FP16_AUTOCAST) return fail(e, FNN_E_INVALID, "accum is not a FNN_ACC_* value");
    return 0;
}

// the entry points on accumulator buffers (multi-GPU accumulate mode, > 63 classes) only know the two buffer arithmetics
inline int no_autocast(fnn_engine *e, const fnn_opts *o, const char *who) {
    return o->accum == FNN_ACC_FP16_AUTOCAST ? fail(e, FNN_E_UNSUPPORTED, "%s: FNN_ACC_FP16_AUTOCAST is served by the gather path only", who) : 0;
}

struct Box { int64_t lo[3], hi[3]; };

std::vector<int64_t> id_range(int64_t first, int64_t n) {
    std::vector<int64_t> ids(n);
    for (int64_t i = 0; i < n; ++i) ids[i] = first + i;
    return ids;
}

// ---- argument checks the entry points share.  out_lo / out_hi: the box of the un-padded volume a call writes; `acc`:
// the accumulator box (padded volume) it reads, or nullptr
int check_out_box(fnn_engine *e, const VolPlan &vp, const int64_t shape[4], const int64_t out_lo[3], const int64_t out_hi[3],
                  const Box *acc) {
    for (int d = 0; d < 3; ++d) {
        if (out_lo[d] < 0 || out_hi[d] > shape[1 + d] || out_lo[d] >= out_hi[d]) return fail(e, FNN_E_INVALID, "output box out of bounds");
        if (acc && (out_lo[d] + vp.lo[d] < acc->lo[d] || out_hi[d] + vp.lo[d] > acc->hi[d]))
            return fail(e, FNN_E_INVALID, "output box is not covered by the accumulator box");
    }
    return 0;
}

// labels of `classes` classes by argmax in the engine's label dtype (fnn_set_label_rule checks the region rule's)
const char *const U16_HINT = ": fnn_set_label_rule(..., FNN_LABEL_U16)";
int check_u8_labels(fnn_engine *e, int classes, const char *hint) {
    if (e->label_u16 || e->label_mode != FNN_LABELS_ARGMAX || classes <= 256) return 0;
    return fail(e, FNN_E_INVALID, "%d classes do not fit uint8 labels%s", classes, hint);
}

// Reads back the inf flag of the launches on `st` (synchronising it) and fails like the reference when one was set
int check_inf(fnn_engine *e, hipStream_t st, const char *msg = "Encountered inf in predicted array.") {
    int flag = 0;
    HIPCHK(e, hipMemcpyAsync(&flag, e->inf_flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    return flag ? fail(e, FNN_E_INF, "%s", msg) : 0;
}

inline int acc_hp(const fnn_arch_desc &a) { return (a.num_heads + 1 + 7) / 8 * 8; }

// What run_patches makes of its patches.  AccBox: the seg head accumulates them into `acc`, which covers `box` of the padded volume ([bx][by][bz][HP],
// channels-last, channel num_heads = weight sum).  `fresh`: the patches are the volume's whole list in visiting order and
// `acc` holds nothing yet (it need not even be zeroed): voxels no earlier patch has touched are then written without
// being read (HeadParams::fx).
struct AccBox { void *acc; Box box; int acc_fp32; bool fresh; };
// FeatSlots (gather path): no head; every evaluation of patch ids[i] leaves the last layer's raw output and InstanceNorm
// rows in slot slot0 + i, item f * n_slots + slot for evaluation f.  fssh: the same rows in fp16 (the engine's slots; a
// caller's rows are converted by fnn_gather_box), or nullptr.
struct FeatSlots { void *feat; float *fss; unsigned short *fssh; int64_t slot0, n_slots; };
using Target = std::variant<AccBox, FeatSlots>;

// Where the patch at origin `oo` lands in an accumulator box, weighted how (HeadParams, PatchAccParams)
template <class Params> void place_patch(Params &p, const fnn_engine *e, const fnn_opts &o, const AccBox &t, const int *oo) {
    const Box &box = t.box;
    p.gauss = (o.use_gaussian ? e->gauss : e->ones).as<f16>();
    p.acc = t.acc; p.AX = box.hi[0] - box.lo[0]; p.Y = box.hi[1] - box.lo[1]; p.Z = box.hi[2] - box.lo[2];
    p.HP = acc_hp(e->plan.arch); p.acc_fp32 = t.acc_fp32;
    p.ox = oo[0] - (int)box.lo[0]; p.oy = oo[1] - (int)box.lo[1]; p.oz = oo[2] - (int)box.lo[2];
}

// Arenas and streams for `want` batches in flight (2 .. MAXP); *np: how many there are.  The arenas take at most half of
// the device's memory (a full-width teacher's is 29 GB at batch 32, the 160^3 ResEnc student's 45 GB) and never what is
// not free: fewer batches in flight then, not a failed call.
int add_pipes(fnn_engine *e, int want, int *np) {
    int NP = std::clamp(want, 2, (int)fnn_engine::MAXP);
    if (e->n_pipe < NP) {
        size_t b[3], free_b = 0, total_b = 0;
        const size_t arena = e->plan.arena_bytes(b);
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && arena > 0) {
            const long long by_total = (long long)(total_b / 2 / arena), by_free = (long long)(free_b * 8 / 10 / arena) + e->n_pipe;
            const long long cap = std::max<long long>(2, std::min(by_total, by_free));
            if (NP > cap) NP = (int)std::max<long long>(cap, e->n_pipe);
        }
    }
    HIPCHK(e, e->ev_start.create());
    for (int k = e->n_pipe; k < NP; ++k) {
        fnn_engine::Pipe &p = e->pipe[k];
        if (k > 0 && !p.arena.act.p) if (int rc = arena_alloc(e, p.arena)) return rc;
        HIPCHK(e, p.st.create());
        HIPCHK(e, p.head.create());
        HIPCHK(e, p.done.create());
        e->n_pipe = k + 1;
    }
    *np = NP;
    return 0;
}

// Runs the listed patches (their origins already on the device) in balanced batches and hands every evaluation
// (mirroring) to the target.  Several batches in flight (see fnn_engine::pipe): batch i runs on arena and stream
// i % NP, its heads wait for the previous batch's; otherwise arena 0 on the caller's stream.  A volume still arriving
// from the host is waited for tile by tile under each batch (HostUpload::need).
int run_patches(fnn_engine *e, int fold, const float *vol_dev, const VolPlan &vp, const fnn_opts &o,
                const std::vector<int64_t> &ids, const int *ids_origins_dev, const Target &t, hipStream_t st) {
    const fnn_arch_desc &a = e->plan.arch;
    const AccBox *ab = std::get_if<AccBox>(&t);
    const FeatSlots *fs = std::get_if<FeatSlots>(&t);
    const long long vdim[3] = {(long long)vp.padded[0], (long long)vp.padded[1], (long long)vp.padded[2]};
    int B = o.batch > 0 ? o.batch : e->plan.max_batch;
    if (B > e->plan.max_batch) B = e->plan.max_batch;
    const auto combos = mirror_combos(o);
    const bool tta = !combos.empty();
    const size_t P = (size_t)a.patch[0] * a.patch[1] * a.patch[2];
    if (tta && ab)
        HIPCHK(e, e->patch_buf.reserve((size_t)B * a.num_heads * P * sizeof(float)));
    const int64_t np = (int64_t)ids.size();
    if (np > B) {                                           // balanced batches: 75 patches run as 19+19+19+18, not 24+24+24+3
        const int64_t nbat = (np + B - 1) / B;
        B = (int)((np + nbat - 1) / nbat);
    }
    for (int64_t i = 0; i < np && ab; ++i) {
        const int *oo = &vp.origins[ids[i] * 3];
        for (int d = 0; d < 3; ++d)
            if (oo[d] < ab->box.lo[d] || oo[d] + a.patch[d] > ab->box.hi[d])
                return fail(e, FNN_E_INVALID, "patch %lld lies outside the accumulator box", (long long)ids[i]);
    }
    const size_t featC = fs ? (size_t)e->plan.layers[e->plan.head_src].cout_pad : 0;
    static const bool no_pipe = fnn_knob("FNN_NO_PIPELINE") != nullptr;                // A-B aid
    static const int want_pipes = fnn_knob("FNN_PIPES") ? atoi(fnn_knob("FNN_PIPES")) : 4;   // round 6: four beat three by 0.3-0.9 % on C1 / C2 / C4 / C5 (profiles/r06_pipes_sweep.txt); beyond four: nothing
    const bool pipelined = !no_pipe && (!tta || fs) && !e->profiling && np > B;
    int NP = 1;
    if (pipelined) {
        if (int rc = add_pipes(e, want_pipes, &NP)) return rc;
        HIPCHK(e, hipEventRecord(e->ev_start, st));
        for (int k = 0; k < NP; ++k) HIPCHK(e, hipStreamWaitEvent(e->pipe[k].st, e->ev_start, 0));
    }
    const bool fresh = ab && ab->fresh;
    std::vector<int> uniq[3];                             // distinct patch positions per axis (fresh: overlap with the previous one)
    if (fresh) {
        for (int d = 0; d < 3; ++d) {
            for (int64_t i = 0; i < vp.n_patches; ++i) uniq[d].push_back(vp.origins[i * 3 + d]);
            std::sort(uniq[d].begin(), uniq[d].end());
            uniq[d].erase(std::unique(uniq[d].begin(), uniq[d].end()), uniq[d].end());
        }
    }
    auto first_visit = [&](const int *oo, int d) -> int {
        if (!fresh) return INT_MAX;
        const auto it = std::lower_bound(uniq[d].begin(), uniq[d].end(), oo[d]);
        if (it == uniq[d].begin()) return 0;
        const int ov = *(it - 1) + a.patch[d] - oo[d];
        return ov > 0 ? ov : 0;
    };
    int64_t bi = 0;
    for (int64_t p0 = 0; p0 < np; p0 += B, ++bi) {
        const int nb = (int)((np - p0 < B) ? np - p0 : B);
        const int *org = ids_origins_dev + p0 * 3;
        const int k = (int)(bi % NP);
        const Arena &A = e->pipe[k].arena;
        hipStream_t bst = pipelined ? (hipStream_t)e->pipe[k].st : st;
        if (e->up.active) {                                   // a volume still arriving from the host: the box this batch's patches read
            int64_t lo[2] = {INT64_MAX, INT64_MAX}, hi[2] = {0, 0};   // (un-padded volume: padded == shape along every axis here)
            for (int b = 0; b < nb; ++b)
                for (int d = 0; d < 2; ++d) {
                    const int64_t o0 = vp.origins[ids[p0 + b] * 3 + d];
                    lo[d] = std::min(lo[d], o0); hi[d] = std::max(hi[d], o0 + a.patch[d]);
                }
            HIPCHK(e, e->up.need(lo[0], hi[0], lo[1], hi[1], bst));
        }
        for (size_t ci = 0; ci <= (tta ? combos.size() : 0); ++ci) {
            int flip[3] = {0, 0, 0};
            if (ci > 0) for (int ax : combos[ci - 1]) flip[ax] = 1;
            if (fs) {                                         // [evaluation][slot]: the batch's items stay contiguous
                const size_t item = (size_t)ci * fs->n_slots + fs->slot0 + p0;
                if (int rc = forward_batch(e, fold, A, vol_dev, 0, vdim, org, nb, flip, bst, (f16 *)fs->feat + item * P * featC,
                                           fs->fss + item * 2 * featC, fs->fssh ? fs->fssh + item * 2 * featC : nullptr)) return rc;
                continue;
            }
            if (int rc = forward_batch(e, fold, A, vol_dev, 0, vdim, org, nb, flip, bst)) return rc;
            if (pipelined && bi > 0) HIPCHK(e, hipStreamWaitEvent(bst, e->pipe[(bi - 1) % NP].head, 0));   // heads in patch order
            for (int b = 0; b < nb; ++b) {
                HeadParams h = make_head(e, A, fold, b);
                const int *oo = &vp.origins[ids[p0 + b] * 3];
                place_patch(h, e, o, *ab, oo);
                h.flip_d = flip[0]; h.flip_h = flip[1]; h.flip_w = flip[2];
                h.fx = first_visit(oo, 0); h.fy = first_visit(oo, 1); h.fz = first_visit(oo, 2);
                if (tta) { h.mode = ci == 0 ? 1 : 2; h.patch_buf = e->patch_buf.as<float>() + (size_t)b * a.num_heads * P; }
                Scope sc(e, bst, FAM_HEAD, e->plan.head_flops);
                if (launch_head(h, bst) != 0) return fail(e, FNN_E_HIP, "seg head launch failed");
            }
            if (pipelined) HIPCHK(e, hipEventRecord(e->pipe[k].head, bst));
        }
        if (tta && ab) {
            for (int b = 0; b < nb; ++b) {
                PatchAccParams q{};
                place_patch(q, e, o, *ab, &vp.origins[ids[p0 + b] * 3]);
                q.patch_buf = e->patch_buf.as<float>() + (size_t)b * a.num_heads * P;
                q.n_div = (int)combos.size() + 1;
                q.PD = a.patch[0]; q.PH = a.patch[1]; q.PW = a.patch[2]; q.heads = a.num_heads;
                Scope sc(e, bst, FAM_HEAD, 0);
                if (launch_patch_acc(q, bst) != 0) return fail(e, FNN_E_HIP, "patch accumulate launch failed");
            }
        }
    }
    if (pipelined) {
        for (int k = 0; k < NP; ++k) {
            HIPCHK(e, hipEventRecord(e->pipe[k].done, e->pipe[k].st));
            HIPCHK(e, hipStreamWaitEvent(st, e->pipe[k].done, 0));
        }
    }
    return 0;
}

// Brings the input volume onto the device and pads it when smaller than the patch.  `slabbed`: the caller's batches call
// e->up.need() for the box their patches read (run_patches); otherwise the whole volume is waited for here.
int stage_volume(fnn_engine *e, const float *vol, const int64_t shape[4], const VolPlan &vp, hipStream_t st,
                 const float **vol_dev, bool slabbed = false) {
    const size_t nin = (size_t)shape[0] * shape[1] * shape[2] * shape[3];
    const float *src = vol;
    const bool need_pad = vp.padded[0] != shape[1] || vp.padded[1] != shape[2] || vp.padded[2] != shape[3];
    if (!fnn_dev_ptr(vol)) {
        HIPCHK(e, e->vol_tmp.reserve(nin * sizeof(float)));
        src = e->vol_tmp.as<float>();
        HIPCHK(e, e->up.begin(vol, e->vol_tmp.as<float>(), (int)shape[0], shape[1], shape[2], shape[3], st));
        if (!slabbed || need_pad) { HIPCHK(e, e->up.need(0, shape[1], 0, shape[2], st)); e->up.active = false; }
    }
    if (need_pad) {
        const size_t npad = (size_t)shape[0] * vp.padded[0] * vp.padded[1] * vp.padded[2];
        HIPCHK(e, e->vol_pad.reserve(npad * sizeof(float)));
        const long long s[3] = {(long long)shape[1], (long long)shape[2], (long long)shape[3]};
        const long long d[3] = {(long long)vp.padded[0], (long long)vp.padded[1], (long long)vp.padded[2]};
        const long long lo[3] = {(long long)vp.lo[0], (long long)vp.lo[1], (long long)vp.lo[2]};
        if (launch_pad_volume(src, e->vol_pad.as<float>(), (int)shape[0], s, d, lo, st) != 0) return fail(e, FNN_E_HIP, "pad launch failed");
        src = e->vol_pad.as<float>();
    }
    *vol_dev = src;
    return 0;
}

// Ends a call's host-volume upload (stage_volume) however the call returns: HostUpload::finish
struct UploadGuard {
    fnn_engine *e;
    bool ok = false;
    ~UploadGuard() { (void)e->up.finish(ok); }
};

// Origins of the listed patches -> device (the stem conv reads them).
int upload_origins(fnn_engine *e, const VolPlan &vp, const std::vector<int64_t> &ids, hipStream_t st) {
    std::vector<int> host(ids.size() * 3);
    for (size_t i = 0; i < ids.size(); ++i)
        for (int d = 0; d < 3; ++d) host[i * 3 + d] = vp.origins[ids[i] * 3 + d];
    HIPCHK(e, e->origins.upload(host.data(), host.size(), st));
    return 0;
}

FinalizeParams make_finalize(fnn_engine *e, const void *acc, const Box &box, const int64_t out_lo[3],
                             const int64_t out_hi[3], const VolPlan &vp, const int64_t shape[4], const fnn_opts &o,
                             int acc_fp32, int mode, void *out) {
    // out_lo / out_hi: box of the UN-PADDED volume that is written
    FinalizeParams f{};
    f.acc = acc;
    f.AX = box.hi[0] - box.lo[0]; f.Y = box.hi[1] - box.lo[1]; f.Z = box.hi[2] - box.lo[2];
    f.HP = acc_hp(e->plan.arch);
    f.lo_x = (int)(out_lo[0] + vp.lo[0] - box.lo[0]); f.lo_y = (int)(out_lo[1] + vp.lo[1] - box.lo[1]);
    f.lo_z = (int)(out_lo[2] + vp.lo[2] - box.lo[2]);
    f.OX = out_hi[0] - out_lo[0]; f.OY = out_hi[1] - out_lo[1]; f.OZ = out_hi[2] - out_lo[2];
    f.out_X = shape[1]; f.out_Y = shape[2]; f.out_Z = shape[3];
    f.out_x = out_lo[0]; f.out_y = out_lo[1]; f.out_z = out_lo[2];
    f.heads = e->plan.arch.num_heads; f.acc_fp32 = acc_fp32; f.out_fp32 = o.out_dtype == FNN_OUT_F32;
    f.mode = mode; f.out = out; f.inf_flag = e->inf_flag.as<int>();
    return f;
}

int accumulate_whole_volume(fnn_engine *e, int fold, const float *vol_dev, const VolPlan &vp, const fnn_opts &o,
                            Box &box, hipStream_t st) {
    const fnn_arch_desc &a = e->plan.arch;
    const int acc_fp32 = o.accum == FNN_ACC_FP32;
    const size_t esz = acc_fp32 ? 4 : 2;
    const size_t nvox = (size_t)vp.padded[0] * vp.padded[1] * vp.padded[2];
    const size_t bytes = nvox * acc_hp(a) * esz;
    HIPCHK(e, e->acc.reserve(bytes));
    // The whole list in visiting order: the seg head writes every voxel's first visit without reading it, so the
    // 17 GB zero fill (and an eighth of the accumulator reads) is skipped.  Mirroring accumulates through the patch
    // buffer and the generic head kernel: those keep the zero fill.
    static const bool no_fv = fnn_knob("FNN_NO_FIRST_VISIT") != nullptr;            // A-B aid
    const bool fresh = !no_fv && o.n_mirror_axes == 0 && launch_head_first_visit_ok(make_head(e, e->pipe[0].arena, fold, 0));
    if (!fresh) HIPCHK(e, hipMemsetAsync(e->acc.p, 0, bytes, st));
    for (int d = 0; d < 3; ++d) { box.lo[d] = 0; box.hi[d] = vp.padded[d]; }
    return run_patches(e, fold, vol_dev, vp, o, id_range(0, vp.n_patches), e->origins.data(), AccBox{e->acc.p, box, acc_fp32, fresh}, st);
}

// The gather kernel's integer tables for a volume: tile starts (+ window bases of axes with more than 64 positions,
// gather.hip gather_tile_windows).  false: an axis has more than 64 tiles over one voxel.
bool gather_tables(const fnn_arch_desc &a, const VolPlan &vp, std::vector<int> *tab, int off[3]) {
    const long long *st[3] = {(const long long *)vp.steps[0].data(), (const long long *)vp.steps[1].data(), (const long long *)vp.steps[2].data()};
    const int n[3] = {(int)vp.steps[0].size(), (int)vp.steps[1].size(), (int)vp.steps[2].size()};
    const int ext[3] = {a.patch[0], a.patch[1], a.patch[2]};
    const long long pad[3] = {(long long)vp.padded[0], (long long)vp.padded[1], (long long)vp.padded[2]};
    size_t count = 0;
    if (!gather_tile_windows(st, n, ext, pad, nullptr, off, &count)) return false;
    if (tab) { tab->assign(count, 0); (void)gather_tile_windows(st, n, ext, pad, tab->data(), off, &count); }
    return true;
}
void gather_set_tables(GatherParams &g, const int *dev, const int off[3]) {
    g.steps = dev;
    g.base_x = off[0] >= 0 ? dev + off[0] : nullptr; g.base_y = off[1] >= 0 ? dev + off[1] : nullptr; g.base_z = off[2] >= 0 ? dev + off[2] : nullptr;
    g.windowed = 1;
}

// The gather kernel's parameters that follow from the engine, the fold, the volume's plan and shape, and the options.
// Its callers add the feature buffers with their slots or ring, the tables, the output box and what is written.
GatherParams gather_params(const fnn_engine *e, int fold, const VolPlan &vp, const int64_t shape[4], const fnn_opts &o) {
    const fnn_arch_desc &a = e->plan.arch;
    const Layer &H = e->plan.layers[e->plan.head_src];
    const FoldWeights &fw = e->folds[fold];
    GatherParams g{};
    g.heads = a.num_heads; g.hblocks = e->plan.hblocks; g.C = H.cout_pad; g.slope = H.act ? a.slope : 1.f;
    g.PD = a.patch[0]; g.PH = a.patch[1]; g.PW = a.patch[2];
    g.nx = (int)vp.steps[0].size(); g.ny = (int)vp.steps[1].size(); g.nz = (int)vp.steps[2].size();
    { int off[3]; g.windowed = gather_tables(a, vp, nullptr, off) ? 1 : 0; }
    const auto combos = mirror_combos(o);
    g.n_eval = 1 + (int)combos.size();
    for (size_t ci = 0; ci < combos.size() && ci + 1 < 8; ++ci)    // (flipmask[0] = 0: the plain evaluation)
        for (int ax : combos[ci]) g.flipmask[ci + 1] |= 1 << ax;
    g.wpk = fw.wpk.as<f16>() + e->plan.head_w_off; g.bias = fw.fparam.as<float>() + e->plan.head_bias_off;
    g.n_pass = e->plan.n_gpass; g.pass_wpk = fw.wpk.as<f16>() + e->plan.gpass_w_off; g.pass_bias = fw.fparam.as<float>() + e->plan.gpass_bias_off;
    g.gauss = (o.use_gaussian ? e->gauss : e->ones).as<f16>();
    g.lo_x = (int)vp.lo[0]; g.lo_y = (int)vp.lo[1]; g.lo_z = (int)vp.lo[2];
    g.OX = shape[1]; g.OY = shape[2]; g.OZ = shape[3];
    g.acc_mode = o.accum; g.inf_flag = e->inf_flag.as<int>();
    g.label_u16 = e->label_u16; g.order = e->label_mode == FNN_LABELS_REGIONS ? e->label_order.as<int>() : nullptr;
    return g;
}

// Plan of the gather path (gather.hip) for a volume: how many x layers of patches are kept at a time.
struct GatherPlan { bool ok = false; int n_eval = 1, ring = 0, cover = 1; size_t layer_items = 0, feat_bytes = 0; const char *why = ""; };

// No gather when the head does not fit the kernel's registers or when not even the layers that cover one output slab fit
// next to what is already allocated; otherwise the whole volume's patches when they fit (one launch at the end), else
// a ring of `cover` layers with one launch per output slab.
GatherPlan gather_plan(fnn_engine *e, int fold, const VolPlan &vp, const int64_t shape[4], const fnn_opts &o, size_t pending_bytes) {
    GatherPlan gp;
    gp.why = "FNN_NO_GATHER is set or the output is not fp16";
    if (!e->gather_enabled || o.out_dtype != FNN_OUT_F16) return gp;
    const Layer &H = e->plan.layers[e->plan.head_src];
    const GatherParams g = gather_params(e, fold, vp, shape, o);
    gp.n_eval = g.n_eval;
    gp.why = "the network's head does not fit the gather kernel (a normalised last layer of <= 32 channels, <= 8 evaluations per patch, <= 64 tiles of one axis over a voxel)";
    if (!H.has_norm || e->plan.head_ksteps != 1 || !gather_ok(g)) return gp;
    gp.why = "not enough free HBM for the patch activations that cover one output slab";
    const auto &sx = vp.steps[0];
    const int nx = (int)sx.size();
    gp.cover = 1;
    for (int i = 0; i < nx; ++i) {                            // layers still needed when layer i has just been produced
        int c = 0;
        for (int j = 0; j <= i; ++j) c += sx[j] + g.PD > sx[i];
        gp.cover = std::max(gp.cover, c);
    }
    const size_t P = (size_t)g.PD * g.PH * g.PW;
    gp.layer_items = (size_t)vp.steps[1].size() * vp.steps[2].size();
    const size_t layer_bytes = gp.layer_items * gp.n_eval * P * H.cout_pad * sizeof(f16);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return gp;
    const double frac = fnn_knob("FNN_GATHER_MEM_FRACTION") ? atof(fnn_knob("FNN_GATHER_MEM_FRACTION")) : 0.6;
    const int force_ring = fnn_knob("FNN_GATHER_RING") ? atoi(fnn_knob("FNN_GATHER_RING")) : 0;     // tests: a ring although all fits
    // (the accumulators are not needed then; `pending_bytes`: what the caller still allocates after this plan - output / label staging)
    const double budget = frac * ((double)(free_b + e->feat.bytes + e->acc.bytes) - (double)pending_bytes);
    if (!force_ring && (double)layer_bytes * nx <= budget) gp.ring = nx;
    else if ((double)layer_bytes * gp.cover <= budget) gp.ring = std::min(nx, std::max(gp.cover, force_ring));
    else return gp;
    gp.feat_bytes = layer_bytes * gp.ring;
    gp.ok = true;
    return gp;
}

int gather_whole_volume(fnn_engine *e, int fold, const float *vol_dev, const VolPlan &vp, const int64_t shape[4],
                        const fnn_opts &o, const GatherPlan &gp, int mode, void *out, void *labels, hipStream_t st) {
    const Layer &H = e->plan.layers[e->plan.head_src];
    if (gp.feat_bytes > e->feat.bytes) e->acc.free();
    HIPCHK(e, e->feat.reserve(gp.feat_bytes));
    const int64_t n_slots = (int64_t)gp.layer_items * gp.ring;
    HIPCHK(e, e->featss.reserve((size_t)n_slots * gp.n_eval * 2 * H.cout_pad * sizeof(float)));
    HIPCHK(e, e->featssh.reserve((size_t)n_slots * gp.n_eval * 2 * H.cout_pad * sizeof(f16)));
    std::vector<int> steps;
    int win_off[3];
    if (!gather_tables(e->plan.arch, vp, &steps, win_off)) return fail(e, FNN_E_UNSUPPORTED, "more than 64 tiles of one axis over a voxel");
    HIPCHK(e, e->steps.upload(steps.data(), steps.size(), st));
    GatherParams g = gather_params(e, fold, vp, shape, o);
    g.feat = e->feat.as<f16>(); g.fss = e->featss.as<float>(); g.fssh = e->featssh.as<unsigned short>();
    g.n_slots = (int)n_slots; g.ring = gp.ring;
    gather_set_tables(g, e->steps.data(), win_off);
    g.y_lo = 0; g.y_hi = (int)shape[2]; g.z_lo = 0; g.z_hi = (int)shape[3];
    g.out_vec = out && shape[3] % 8 == 0 && ((size_t)out % 16) == 0;
    g.mode = mode; g.out = out; g.labels = labels;
    auto launch = [&](int x_lo, int x_hi, double n_patches) {
        g.x_lo = x_lo; g.x_hi = x_hi;
        Scope sc(e, st, FAM_HEAD, e->plan.head_flops * n_patches * gp.n_eval);
        return launch_gather(g, st) == 0 ? 0 : fail(e, FNN_E_HIP, "gather launch failed");
    };
    const FeatSlots slots{e->feat.p, e->featss.as<float>(), e->featssh.as<unsigned short>(), 0, n_slots};
    if (gp.ring == g.nx) {                                     // every patch of the volume is kept: one pass at the end
        if (int rc = run_patches(e, fold, vol_dev, vp, o, id_range(0, vp.n_patches), e->origins.data(), slots, st)) return rc;
        return launch(0, (int)shape[1], (double)vp.n_patches);
    }
    // ring: after x layer ix the output slab up to the next layer's first voxel is complete (padded coordinates
    // [steps[ix], steps[ix + 1]); the un-padded range is clamped); the next layer then overwrites the oldest slot
    const int64_t L = (int64_t)gp.layer_items;
    for (int ix = 0; ix < g.nx; ++ix) {
        FeatSlots layer = slots;
        layer.slot0 = (ix % gp.ring) * L;
        if (int rc = run_patches(e, fold, vol_dev, vp, o, id_range(ix * L, L), e->origins.data() + ix * L * 3, layer, st)) return rc;
        const int64_t p_lo = ix == 0 ? 0 : vp.steps[0][ix], p_hi = ix + 1 < g.nx ? vp.steps[0][ix + 1] : vp.padded[0];
        const int x_lo = (int)std::max<int64_t>(0, p_lo - vp.lo[0]), x_hi = (int)std::min<int64_t>(shape[1], p_hi - vp.lo[0]);
        if (x_hi > x_lo) if (int rc = launch(x_lo, x_hi, (double)L)) return rc;
    }
    return 0;
}

int predict_impl(fnn_engine *e, int fold0, int n_folds, const float *vol, const int64_t shape[4], const fnn_opts *o,
                 void *out, void *labels) {
    for (int f = fold0; f < fold0 + n_folds; ++f)
        if (int rc = check_ready(e, f, o)) return rc;
    if (!vol || (!out && !labels) || !shape) return fail(e, FNN_E_INVALID, "NULL argument");
    const fnn_arch_desc &a = e->plan.arch;
    if (shape[0] != a.in_channels) return fail(e, FNN_E_INVALID, "input has %lld channels, the network expects %d", (long long)shape[0], a.in_channels);
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)o->stream;
    VolPlan vp;
    if (int rc = plan_volume(e, shape, *o, vp)) return rc;
    const float *vol_dev = nullptr;
    UploadGuard upload{e};
    if (int rc = stage_volume(e, vol, shape, vp, st, &vol_dev, true)) return rc;
    if (int rc = upload_origins(e, vp, id_range(0, vp.n_patches), st)) return rc;
    const size_t nvox_out = (size_t)shape[1] * shape[2] * shape[3];
    const size_t nout = (size_t)a.num_heads * nvox_out;
    const size_t osz = o->out_dtype == FNN_OUT_F32 ? 4 : 2;
    const bool want_logits = out != nullptr;
    const bool out_on_dev = out && fnn_dev_ptr(out);
    const bool lab_on_dev = labels && fnn_dev_ptr(labels);
    const size_t lab_bytes = nvox_out * (e->label_u16 ? 2 : 1);
    // (the plan first: nothing is allocated yet when it refuses the request, and it decides how labels are formed; the
    // staging buffers that ARE allocated afterwards - fp16 / fp32 logits when the caller's are on the host or the labels
    // come from materialised logits, the label map of a host caller - come out of its budget)
    size_t pending = 0;
    {
        const bool maybe_direct = labels && !want_logits && n_folds == 1 && e->plan.n_gpass == 1;
        if (!maybe_direct && !out_on_dev && nout * osz > e->out_tmp.bytes) pending += nout * osz - e->out_tmp.bytes;
        if (labels && !lab_on_dev) pending += lab_bytes;
    }
    const GatherPlan gp = gather_plan(e, fold0, vp, shape, *o, pending);
    if (!gp.ok && o->accum == FNN_ACC_FP16_AUTOCAST)
        return fail(e, FNN_E_UNSUPPORTED, "FNN_ACC_FP16_AUTOCAST needs the gather path: %s", gp.why);
    // argmax straight from the accumulators / the gather kernel's registers; with more than 63 classes the gather kernel
    // runs in passes over the heads, so the labels come from its logits
    // (accumulate path: labels_from_acc_coop_kernel covers up to 32 lanes of 8 channels per voxel - 254 classes; beyond, the
    // labels come from the logits like an ensemble's)
    const bool labels_direct = labels && !want_logits && n_folds == 1 && !(gp.ok && e->plan.n_gpass > 1) && (gp.ok || acc_hp(a) <= 256);
    void *out_dev = out;
    if (!labels_direct && !out_on_dev) {
        HIPCHK(e, e->out_tmp.reserve(nout * osz));
        out_dev = e->out_tmp.p;
    }
    void *lab_dev = labels;
    DevBuf lab_tmp;
    const int *lab_order = e->label_mode == FNN_LABELS_REGIONS ? e->label_order.as<int>() : nullptr;
    if (labels) if (int rc = check_u8_labels(e, a.num_heads, U16_HINT)) return rc;
    if (labels && !lab_on_dev) { HIPCHK(e, lab_tmp.reserve(lab_bytes)); lab_dev = lab_tmp.p; }
    HIPCHK(e, hipMemsetAsync(e->inf_flag.p, 0, sizeof(int), st));
    e->ev_used = 0; e->klog.clear();
    const int acc_fp32 = o->accum == FNN_ACC_FP32;
    const int64_t zero3[3] = {0, 0, 0}, full3[3] = {shape[1], shape[2], shape[3]};
    int rc = 0;
    for (int f = 0; f < n_folds && rc == 0; ++f) {
        if (gp.ok) {
            rc = gather_whole_volume(e, fold0 + f, vol_dev, vp, shape, *o, gp, f > 0 ? 1 : 0, labels_direct ? nullptr : out_dev,
                                     labels_direct ? lab_dev : nullptr, st);
            continue;
        }
        Box box;
        rc = accumulate_whole_volume(e, fold0 + f, vol_dev, vp, *o, box, st);
        if (rc) break;
        FinalizeParams fp = make_finalize(e, e->acc.p, box, zero3, full3, vp, shape, *o, acc_fp32, f > 0 ? 1 : 0, out_dev);
        Scope sc(e, st, FAM_FINAL, 0);
        if (labels_direct) { if (launch_labels_from_acc(fp, lab_dev, e->label_u16, lab_order, st) != 0) rc = fail(e, FNN_E_HIP, "labels launch failed"); }
        else if (launch_finalize(fp, st) != 0) rc = fail(e, FNN_E_HIP, "finalize launch failed");
    }
    if (rc == 0 && !labels_direct && n_folds > 1)
        if (launch_scale_output(out_dev, o->out_dtype == FNN_OUT_F32, (long long)nout, n_folds, e->inf_flag.as<int>(), st) != 0)
            rc = fail(e, FNN_E_HIP, "scale launch failed");
    if (rc == 0 && labels && !labels_direct)
        if (launch_argmax(out_dev, o->out_dtype == FNN_OUT_F32, a.num_heads, (long long)nvox_out, lab_dev, e->label_u16, lab_order, st) != 0)
            rc = fail(e, FNN_E_HIP, "argmax launch failed");
    if (rc == 0) {
        hipError_t r1 = hipSuccess;
        if (want_logits && !out_on_dev) r1 = hipMemcpyAsync(out, out_dev, nout * osz, hipMemcpyDeviceToHost, st);
        if (r1 == hipSuccess && labels && !lab_on_dev) r1 = hipMemcpyAsync(labels, lab_dev, lab_bytes, hipMemcpyDeviceToHost, st);
        if (r1 != hipSuccess) rc = fail(e, FNN_E_HIP, "copy back failed: %s", hipGetErrorString(r1));
    }
    if (rc == 0)
        rc = check_inf(e, st, "Encountered inf in predicted array. Aborting... If this problem persists, reduce "
                              "value_scaling_factor in compute_gaussian or increase the dtype of predicted_logits to fp32");
    if (e->profiling && (rc == 0 || rc == FNN_E_INF)) collect_profile(e, vp.n_patches * n_folds);
    upload.ok = rc == 0;
    return rc;
}

// The patch entry points' common part (fnn_accumulate_patches, fnn_patch_features): the caller's patches of the volume
// -> the target
int run_listed_patches(fnn_engine *e, int fold, const float *vol, const int64_t shape[4], const fnn_opts &o, const VolPlan &vp,
                       const int64_t *patch_ids, int64_t n_ids, const Target &t) {
    const std::vector<int64_t> ids(patch_ids, patch_ids + n_ids);
    for (int64_t id : ids) if (id < 0 || id >= vp.n_patches) return fail(e, FNN_E_INVALID, "patch id out of range");
    if (ids.empty()) return 0;
    hipStream_t st = (hipStream_t)o.stream;
    const float *vol_dev = nullptr;
    UploadGuard upload{e};
    if (int rc = stage_volume(e, vol, shape, vp, st, &vol_dev)) return rc;
    if (int rc = upload_origins(e, vp, ids, st)) return rc;
    e->ev_used = 0; e->klog.clear();
    if (int rc = run_patches(e, fold, vol_dev, vp, o, ids, e->origins.data(), t, st)) return rc;
    if (e->profiling) { HIPCHK(e, hipStreamSynchronize(st)); collect_profile(e, n_ids); }
    upload.ok = true;
    return 0;
}

// fnn_normalize_box (out) and fnn_labels_box (labels): an output box from an accumulator box
int finalize_box(fnn_engine *e, const char *who, const void *acc, const int64_t shape[4], const fnn_opts *opts,
                 const int64_t box_lo[3], const int64_t box_hi[3], const int64_t out_lo[3], const int64_t out_hi[3],
                 void *out, void *labels) {
    if (!e || !opts) return FNN_E_INVALID;
    if (int rc = no_autocast(e, opts, who)) return rc;
    void *dst = out ? out : labels;
    if (!acc || !dst || !box_lo || !box_hi || !out_lo || !out_hi) return fail(e, FNN_E_INVALID, "NULL argument");
    if (!fnn_dev_ptr(acc) || !fnn_dev_ptr(dst)) return fail(e, FNN_E_INVALID, "%s needs device pointers", who);
    if (labels && acc_hp(e->plan.arch) > 256)
        return fail(e, FNN_E_UNSUPPORTED, "fnn_labels_box serves up to 254 classes (%d here): take the logits (fnn_normalize_box) and fnn_argmax_labels", e->plan.arch.num_heads);
    if (labels) if (int rc = check_u8_labels(e, e->plan.arch.num_heads, U16_HINT)) return rc;
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)opts->stream;
    VolPlan vp;
    if (int rc = plan_volume(e, shape, *opts, vp)) return rc;
    Box box;
    for (int d = 0; d < 3; ++d) { box.lo[d] = box_lo[d]; box.hi[d] = box_hi[d]; }
    if (int rc = check_out_box(e, vp, shape, out_lo, out_hi, &box)) return rc;
    HIPCHK(e, hipMemsetAsync(e->inf_flag.p, 0, sizeof(int), st));
    const FinalizeParams f = make_finalize(e, acc, box, out_lo, out_hi, vp, shape, *opts, opts->accum == FNN_ACC_FP32, 0, out);
    const int *order = e->label_mode == FNN_LABELS_REGIONS ? e->label_order.as<int>() : nullptr;
    if (out && launch_finalize(f, st) != 0) return fail(e, FNN_E_HIP, "finalize launch failed");
    if (labels && launch_labels_from_acc(f, labels, e->label_u16, order, st) != 0) return fail(e, FNN_E_HIP, "labels launch failed");
    return check_inf(e, st);
}

}  // namespace

// ===========================================================================
// C ABI
// ===========================================================================
extern "C" {

int fnn_abi_version(void) { return FNN_ABI_VERSION; }

const char *fnn_last_error(const fnn_engine *e) { return e ? e->err.c_str() : g_err.c_str(); }

// The layer plan (layer_plan.h: host only, no HIP call) under the switches the environment holds now; a refusal is
// the call's error
static int make_plan(const fnn_arch_desc *arch, int max_batch, LayerPlan &plan) {
    std::string err;
    const int rc = plan_layers(*arch, max_batch, PlanSwitches::from_env(), plan, err);
    return rc ? fail(nullptr, rc, "%s", err.c_str()) : 0;
}

// text -> the caller's buffer (cut to cap - 1 characters, 0-terminated); returns the size that holds all of it
static int64_t copy_text(const std::string &all, char *buf, int64_t cap) {
    if (buf && cap > 0) {
        const size_t n = std::min((size_t)cap - 1, all.size());
        memcpy(buf, all.data(), n);
        buf[n] = 0;
    }
    return (int64_t)all.size() + 1;
}
static std::string lines(const std::vector<std::string> &rows) {
    std::string all;
    for (const std::string &r : rows) { all += r; all += '\n'; }
    return all;
}

// The plan is made before a device is looked for: a descriptor or batch size that cannot be planned is refused as such
int fnn_create(const fnn_arch_desc *arch, int device, int max_batch, fnn_engine **out) {
    if (!arch || !out) return fail(nullptr, FNN_E_INVALID, "NULL argument");
    LayerPlan plan;
    if (int rc = make_plan(arch, max_batch, plan)) return rc;
    std::unique_ptr<fnn_engine> e(new fnn_engine(std::move(plan)));
    e->gather_enabled = fnn_knob("FNN_NO_GATHER") == nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(nullptr, FNN_E_HIP, "no HIP device is available: the MI355X engine has no CPU fallback");
    if (device < 0 || device >= ndev) return fail(nullptr, FNN_E_INVALID, "device %d out of range (%d visible)", device, ndev);
    e->device = device;
    HIPCHK(nullptr, hipSetDevice(device));
    if (int rc = arena_alloc(e.get(), e->pipe[0].arena)) return rc;
    HIPCHK(nullptr, e->inf_flag.reserve(sizeof(int)));
    {
        const size_t P = (size_t)arch->patch[0] * arch->patch[1] * arch->patch[2];
        std::vector<uint16_t> one(P, 0x3c00);                                       // fp16 1.0
        HIPCHK(nullptr, e->ones.reserve(P * 2));
        HIPCHK(nullptr, hipMemcpy(e->ones.p, one.data(), P * 2, hipMemcpyHostToDevice));
    }
    *out = e.release();
    return 0;
}

// Every resource is a member that frees itself (owned.h): their order in fnn_engine carries no meaning, because the device
// is idle before the first of them goes.
void fnn_destroy(fnn_engine *e) {
    if (!e) return;
    (void)hipSetDevice(e->device);
    (void)hipDeviceSynchronize();
    delete e;
}

int64_t fnn_weight_count(const fnn_engine *e) { return e ? e->plan.blob_count : -1; }

int fnn_load_weights(fnn_engine *e, int fold, const float *blob, int64_t count) {
    if (!e) return FNN_E_INVALID;
    if (!blob) return fail(e, FNN_E_INVALID, "NULL blob");
    if (count != e->plan.blob_count) return fail(e, FNN_E_INVALID, "weight blob has %lld values, expected %lld", (long long)count, (long long)e->plan.blob_count);
    if (fold < 0 || fold >= 64) return fail(e, FNN_E_INVALID, "fold index out of range");
    HIPCHK(e, hipSetDevice(e->device));
    if ((int)e->folds.size() <= fold) e->folds.resize(fold + 1);
    FoldWeights &fw = e->folds[fold];
    std::vector<uint16_t> wpk;
    std::vector<float> fp;
    pack_fold_weights(e->plan, blob, wpk, fp);
    HIPCHK(e, fw.wpk.reserve(fnn_weight_alloc_bytes(wpk.size())));
    HIPCHK(e, fw.fparam.reserve(fp.size() * 4));
    HIPCHK(e, hipMemcpy(fw.wpk.p, wpk.data(), wpk.size() * 2, hipMemcpyHostToDevice));
    HIPCHK(e, hipMemcpy(fw.fparam.p, fp.data(), fp.size() * 4, hipMemcpyHostToDevice));
    fw.loaded = true;
    return 0;
}

int fnn_set_gaussian(fnn_engine *e, const uint16_t *half_bits, int64_t count) {
    if (!e) return FNN_E_INVALID;
    const int64_t P = (int64_t)e->plan.arch.patch[0] * e->plan.arch.patch[1] * e->plan.arch.patch[2];
    if (!half_bits || count != P) return fail(e, FNN_E_INVALID, "gaussian must have %lld values", (long long)P);
    HIPCHK(e, hipSetDevice(e->device));
    HIPCHK(e, e->gauss.reserve(P * 2));
    HIPCHK(e, hipMemcpy(e->gauss.p, half_bits, P * 2, hipMemcpyHostToDevice));
    return 0;
}

int fnn_predict_volume(fnn_engine *e, int fold, const float *vol, const int64_t shape[4], const fnn_opts *opts, void *out) {
    if (!e) return FNN_E_INVALID;
    return predict_impl(e, fold, 1, vol, shape, opts, out, nullptr);
}

int fnn_predict_volume_ensemble(fnn_engine *e, int n_folds, const float *vol, const int64_t shape[4], const fnn_opts *opts, void *out) {
    if (!e) return FNN_E_INVALID;
    if (n_folds < 1) return fail(e, FNN_E_INVALID, "n_folds must be >= 1");
    return predict_impl(e, 0, n_folds, vol, shape, opts, out, nullptr);
}

int fnn_predict_labels(fnn_engine *e, int n_folds, const float *vol, const int64_t shape[4], const fnn_opts *opts, void *labels) {
    if (!e) return FNN_E_INVALID;
    if (n_folds < 1) return fail(e, FNN_E_INVALID, "n_folds must be >= 1");
    if (!labels) return fail(e, FNN_E_INVALID, "NULL labels");
    return predict_impl(e, 0, n_folds, vol, shape, opts, nullptr, labels);
}

int64_t fnn_accumulator_channels(const fnn_engine *e) { return e ? acc_hp(e->plan.arch) : -1; }

int fnn_accumulate_patches(fnn_engine *e, int fold, const float *vol, const int64_t shape[4], const fnn_opts *opts,
                           const int64_t *patch_ids, int64_t n_ids, const int64_t box_lo[3], const int64_t box_hi[3],
                           void *acc) {
    if (int rc = check_ready(e, fold, opts)) return rc;
    if (int rc = no_autocast(e, opts, "fnn_accumulate_patches")) return rc;
    if (!vol || !acc || !box_lo || !box_hi || (n_ids > 0 && !patch_ids)) return fail(e, FNN_E_INVALID, "NULL argument");
    if (!fnn_dev_ptr(acc)) return fail(e, FNN_E_INVALID, "accumulators must be device memory");
    HIPCHK(e, hipSetDevice(e->device));
    VolPlan vp;
    if (int rc = plan_volume(e, shape, *opts, vp)) return rc;
    Box box;
    for (int d = 0; d < 3; ++d) {
        box.lo[d] = box_lo[d]; box.hi[d] = box_hi[d];
        if (box.lo[d] < 0 || box.hi[d] > vp.padded[d] || box.lo[d] >= box.hi[d]) return fail(e, FNN_E_INVALID, "box out of bounds");
    }
    return run_listed_patches(e, fold, vol, shape, *opts, vp, patch_ids, n_ids, AccBox{acc, box, opts->accum == FNN_ACC_FP32, false});
}

int fnn_normalize_box(fnn_engine *e, const void *acc, const int64_t shape[4], const fnn_opts *opts,
                      const int64_t box_lo[3], const int64_t box_hi[3], const int64_t out_lo[3], const int64_t out_hi[3],
                      void *out) {
    return finalize_box(e, "fnn_normalize_box", acc, shape, opts, box_lo, box_hi, out_lo, out_hi, out, nullptr);
}

int fnn_labels_box(fnn_engine *e, const void *acc, const int64_t shape[4], const fnn_opts *opts,
                   const int64_t box_lo[3], const int64_t box_hi[3], const int64_t out_lo[3], const int64_t out_hi[3],
                   void *labels) {
    return finalize_box(e, "fnn_labels_box", acc, shape, opts, box_lo, box_hi, out_lo, out_hi, nullptr, labels);
}

int64_t fnn_feature_channels(const fnn_engine *e) { return e ? e->plan.layers[e->plan.head_src].cout_pad : -1; }

int fnn_patch_features(fnn_engine *e, int fold, const float *vol, const int64_t shape[4], const fnn_opts *opts,
                       const int64_t *patch_ids, int64_t n_ids, void *feat, float *fss, int64_t slot0, int64_t n_slots) {
    if (int rc = check_ready(e, fold, opts)) return rc;
    if (!vol || !feat || !fss || (n_ids > 0 && !patch_ids)) return fail(e, FNN_E_INVALID, "NULL argument");
    if (!fnn_dev_ptr(feat) || !fnn_dev_ptr(fss)) return fail(e, FNN_E_INVALID, "feature buffers must be device memory");
    if (slot0 < 0 || n_slots < slot0 + n_ids) return fail(e, FNN_E_INVALID, "slots [%lld, %lld) do not fit %lld slots", (long long)slot0, (long long)(slot0 + n_ids), (long long)n_slots);
    if (1 + (int)mirror_combos(*opts).size() > 8) return fail(e, FNN_E_UNSUPPORTED, "more than 8 evaluations per patch");
    if (!e->plan.layers[e->plan.head_src].has_norm) return fail(e, FNN_E_UNSUPPORTED, "the network's last layer has no InstanceNorm");
    HIPCHK(e, hipSetDevice(e->device));
    VolPlan vp;
    if (int rc = plan_volume(e, shape, *opts, vp)) return rc;
    return run_listed_patches(e, fold, vol, shape, *opts, vp, patch_ids, n_ids, FeatSlots{feat, fss, nullptr, slot0, n_slots});
}

int fnn_gather_box(fnn_engine *e, int fold, const void *feat, const float *fss, const int32_t *slot_of_patch,
                   int64_t n_slots, const int64_t shape[4], const fnn_opts *opts, const int64_t out_lo[3], const int64_t out_hi[3],
                   void *out_logits, void *labels) {
    if (int rc = check_ready(e, fold, opts)) return rc;
    if (!feat || !fss || !slot_of_patch || !out_lo || !out_hi || (!out_logits && !labels)) return fail(e, FNN_E_INVALID, "NULL argument");
    if (!fnn_dev_ptr(feat) || !fnn_dev_ptr(fss) || (out_logits && !fnn_dev_ptr(out_logits)) || (labels && !fnn_dev_ptr(labels)))
        return fail(e, FNN_E_INVALID, "fnn_gather_box needs device pointers");
    if (opts->out_dtype != FNN_OUT_F16) return fail(e, FNN_E_UNSUPPORTED, "fnn_gather_box: fp16 logits");
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)opts->stream;
    VolPlan vp;
    if (int rc = plan_volume(e, shape, *opts, vp)) return rc;
    if (int rc = check_out_box(e, vp, shape, out_lo, out_hi, nullptr)) return rc;
    const Layer &H = e->plan.layers[e->plan.head_src];
    GatherParams g = gather_params(e, fold, vp, shape, *opts);
    std::vector<int> tab;
    int win_off[3];
    (void)gather_tables(e->plan.arch, vp, &tab, win_off);          // (g.windowed: whether it could)
    // (labels of more than 256 classes end here too: the uint8 limit needs no check of its own)
    if (labels && e->plan.n_gpass > 1)
        return fail(e, FNN_E_UNSUPPORTED, "fnn_gather_box writes labels for <= 63 classes; with %d take the logits and fnn_argmax_labels", e->plan.arch.num_heads);
    if (!H.has_norm || e->plan.head_ksteps != 1 || !gather_ok(g)) return fail(e, FNN_E_UNSUPPORTED, "this network's head does not fit the gather kernel");
    for (int64_t i = 0; i < vp.n_patches; ++i)
        if (slot_of_patch[i] >= n_slots) return fail(e, FNN_E_INVALID, "slot %d of patch %lld is beyond the %lld slots", slot_of_patch[i], (long long)i, (long long)n_slots);
    // tile starts (+ window bases), then the slot table, in one device buffer
    const size_t n_steps = tab.size();
    for (int64_t i = 0; i < vp.n_patches; ++i) tab.push_back(slot_of_patch[i]);
    HIPCHK(e, e->steps.upload(tab.data(), tab.size(), st));
    HIPCHK(e, hipMemsetAsync(e->inf_flag.p, 0, sizeof(int), st));
    {   // the kernel reads the InstanceNorm rows in the conv kernels' fp16 staging layout: converted from the caller's fp32 rows
        const size_t items = (size_t)n_slots * g.n_eval;
        HIPCHK(e, e->featssh.reserve(items * 2 * H.cout_pad * sizeof(f16)));
        if (launch_fss_to_ssh(fss, e->featssh.as<unsigned short>(), (long long)items, H.cout_pad, st) != 0) return fail(e, FNN_E_HIP, "row conversion launch failed");
    }
    g.feat = (const f16 *)feat; g.fss = fss; g.fssh = e->featssh.as<unsigned short>();
    g.n_slots = (int)n_slots; g.ring = 1;                       // evaluation f of slot s: item f * n_slots + s (fnn_patch_features)
    gather_set_tables(g, e->steps.data(), win_off);
    g.slot_tab = e->steps.data() + n_steps;
    g.x_lo = (int)out_lo[0]; g.x_hi = (int)out_hi[0]; g.y_lo = (int)out_lo[1]; g.y_hi = (int)out_hi[1];
    g.z_lo = (int)out_lo[2]; g.z_hi = (int)out_hi[2];
    e->ev_used = 0; e->klog.clear();
    if (out_logits) {
        g.out = out_logits; g.labels = nullptr;
        g.out_vec = shape[3] % 8 == 0 && ((size_t)out_logits % 16) == 0;
        Scope sc(e, st, FAM_HEAD, 0);
        if (launch_gather(g, st) != 0) return fail(e, FNN_E_HIP, "gather launch failed");
    }
    if (labels) {
        g.out = nullptr; g.labels = labels; g.out_vec = 0;
        Scope sc(e, st, FAM_HEAD, 0);
        if (launch_gather(g, st) != 0) return fail(e, FNN_E_HIP, "gather launch failed");
    }
    return check_inf(e, st);
}

static int region_copy(fnn_engine *e, void *feat, int64_t n_slots, const fnn_region *regions, int64_t n, void *message,
                       void *stream, bool pack) {
    if (!e) return FNN_E_INVALID;
    if (n == 0) return 0;
    if (!feat || !regions || !message || n < 0 || n_slots < 1) return fail(e, FNN_E_INVALID, "bad argument");
    if (!fnn_dev_ptr(feat) || !fnn_dev_ptr(regions) || !fnn_dev_ptr(message))
        return fail(e, FNN_E_INVALID, "fnn_pack_regions / fnn_unpack_regions need device pointers (the region table too)");
    if (n > 65535) return fail(e, FNN_E_INVALID, "more than 65535 regions in one message");
    static_assert(sizeof(fnn_region) == 40, "fnn_region is ten 32-bit words");
    HIPCHK(e, hipSetDevice(e->device));
    const fnn_arch_desc &a = e->plan.arch;
    if (launch_region_copy(feat, n_slots, (const int *)regions, (int)n, message, a.patch[0], a.patch[1], a.patch[2],
                           e->plan.layers[e->plan.head_src].cout_pad, pack, (hipStream_t)stream) != 0)
        return fail(e, FNN_E_HIP, "region copy launch failed");
    return 0;
}

int fnn_pack_regions(fnn_engine *e, const void *feat, int64_t n_slots, const fnn_region *regions, int64_t n, void *message, void *stream) {
    return region_copy(e, const_cast<void *>(feat), n_slots, regions, n, message, stream, true);
}

int fnn_unpack_regions(fnn_engine *e, void *feat, int64_t n_slots, const fnn_region *regions, int64_t n, const void *message, void *stream) {
    return region_copy(e, feat, n_slots, regions, n, const_cast<void *>(message), stream, false);
}

int fnn_forward_patches(fnn_engine *e, int fold, const float *x, int n, float *logits, void *stream) {
    if (!e) return FNN_E_INVALID;
    if (fold < 0 || fold >= (int)e->folds.size() || !e->folds[fold].loaded) return fail(e, FNN_E_STATE, "weights of fold %d are not loaded", fold);
    if (!x || !logits || n < 1) return fail(e, FNN_E_INVALID, "bad argument");
    HIPCHK(e, hipSetDevice(e->device));
    hipStream_t st = (hipStream_t)stream;
    const fnn_arch_desc &a = e->plan.arch;
    const size_t P = (size_t)a.patch[0] * a.patch[1] * a.patch[2];
    const size_t nin = (size_t)n * a.in_channels * P, nout = (size_t)n * a.num_heads * P;
    const float *xd = x;
    if (!fnn_dev_ptr(x)) {
        HIPCHK(e, e->vol_tmp.reserve(nin * 4));
        HIPCHK(e, hipMemcpyAsync(e->vol_tmp.p, x, nin * 4, hipMemcpyHostToDevice, st));
        xd = e->vol_tmp.as<float>();
    }
    float *od = logits;
    const bool out_dev = fnn_dev_ptr(logits);
    if (!out_dev) {
        HIPCHK(e, e->out_tmp.reserve(nout * 4));
        od = e->out_tmp.as<float>();
    }
    std::vector<int> zeros((size_t)e->plan.max_batch * 3, 0);
    HIPCHK(e, e->origins.upload(zeros.data(), zeros.size(), st));
    HIPCHK(e, hipStreamSynchronize(st));
    const long long vdim[3] = {a.patch[0], a.patch[1], a.patch[2]};
    const int flip[3] = {0, 0, 0};
    e->ev_used = 0; e->klog.clear();
    for (int p0 = 0; p0 < n; p0 += e->plan.max_batch) {
        const int nb = (n - p0 < e->plan.max_batch) ? n - p0 : e->plan.max_batch;
        if (int rc = forward_batch(e, fold, e->pipe[0].arena, xd + (size_t)p0 * a.in_channels * P, (long long)(a.in_channels * P), vdim,
                                   e->origins.data(), nb, flip, st)) return rc;
        for (int b = 0; b < nb; ++b) {
            HeadParams h = make_head(e, e->pipe[0].arena, fold, b);
            h.mode = 1; h.patch_buf = od + (size_t)(p0 + b) * a.num_heads * P;
            h.acc_fp32 = 1;
            Scope sc(e, st, FAM_HEAD, e->plan.head_flops);
            if (launch_head(h, st) != 0) return fail(e, FNN_E_HIP, "seg head launch failed");
        }
    }
    if (!out_dev) HIPCHK(e, hipMemcpyAsync(logits, od, nout * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    if (e->profiling) collect_profile(e, n);
    return 0;
}

int fnn_set_label_rule(fnn_engine *e, int mode, const int32_t *regions_class_order, int n_regions, int label_dtype) {
    if (!e) return FNN_E_INVALID;
    if ((mode != FNN_LABELS_ARGMAX && mode != FNN_LABELS_REGIONS) || (label_dtype != FNN_LABEL_U8 && label_dtype != FNN_LABEL_U16))
        return fail(e, FNN_E_INVALID, "unknown label mode / dtype");
    if (mode == FNN_LABELS_REGIONS) {
        if (!regions_class_order || n_regions != e->plan.arch.num_heads)
            return fail(e, FNN_E_INVALID, "regions_class_order needs one entry per segmentation head (%d), got %d", e->plan.arch.num_heads, n_regions);
        const int limit = label_dtype == FNN_LABEL_U16 ? 65535 : 255;
        for (int i = 0; i < n_regions; ++i)
            if (regions_class_order[i] < 0 || regions_class_order[i] > limit)
                return fail(e, FNN_E_INVALID, "regions_class_order[%d] = %d does not fit the label dtype", i, regions_class_order[i]);
        HIPCHK(e, hipSetDevice(e->device));
        HIPCHK(e, e->label_order.reserve(sizeof(int) * (size_t)e->plan.arch.num_heads));
        HIPCHK(e, hipMemcpy(e->label_order.p, regions_class_order, sizeof(int) * (size_t)n_regions, hipMemcpyHostToDevice));
    }
    e->label_mode = mode;
    e->label_u16 = label_dtype == FNN_LABEL_U16;
    return FNN_OK;
}

int fnn_argmax_labels(fnn_engine *e, const void *logits, int dtype, int heads, int64_t n_vox, void *labels, void *stream) {
    if (!e) return FNN_E_INVALID;
    if (!logits || !labels || heads < 1) return fail(e, FNN_E_INVALID, "bad argument");
    const bool regions = e->label_mode == FNN_LABELS_REGIONS;
    if (regions && heads != e->plan.arch.num_heads) return fail(e, FNN_E_INVALID, "the region rule was set for %d heads, got %d", e->plan.arch.num_heads, heads);
    if (int rc = check_u8_labels(e, heads, "")) return rc;
    if (!fnn_dev_ptr(logits) || !fnn_dev_ptr(labels)) return fail(e, FNN_E_INVALID, "fnn_argmax_labels needs device pointers");
    HIPCHK(e, hipSetDevice(e->device));
    if (launch_argmax(logits, dtype == FNN_OUT_F32, heads, n_vox, labels, e->label_u16, regions ? e->label_order.as<int>() : nullptr,
                      (hipStream_t)stream) != 0)
        return fail(e, FNN_E_HIP, "argmax launch failed");
    return 0;
}

int fnn_compute_steps(int64_t image_size, int64_t patch_size, double step, int64_t *steps, int cap) {
    std::vector<int64_t> s;
    if (steps_1d(image_size, patch_size, step, s) != 0) return fail(nullptr, FNN_E_INVALID, "image size must be as large or larger than patch_size, 0 < step <= 1");
    if ((int)s.size() > cap) return fail(nullptr, FNN_E_INVALID, "steps buffer too small (%zu needed)", s.size());
    for (size_t i = 0; i < s.size(); ++i) steps[i] = s[i];
    return (int)s.size();
}

int fnn_plan_volume(const int32_t patch[3], const int64_t shape_sp[3], double step, int64_t padded[3], int64_t pad_lo[3],
                    int64_t *n_patches, int32_t *origins, int64_t origins_cap) {
    if (!patch || !shape_sp) return fail(nullptr, FNN_E_INVALID, "NULL argument");
    VolPlan vp;
    const bool two_d = patch[0] == 0;
    const int32_t pp[3] = {two_d ? 1 : patch[0], patch[1], patch[2]};
    if (plan_volume_p(pp, shape_sp, step, two_d, vp) != 0) return fail(nullptr, FNN_E_INVALID, "invalid volume shape / patch / step size");
    for (int d = 0; d < 3; ++d) { if (padded) padded[d] = vp.padded[d]; if (pad_lo) pad_lo[d] = vp.lo[d]; }
    if (n_patches) *n_patches = vp.n_patches;
    if (origins) {
        if (origins_cap < vp.n_patches) return fail(nullptr, FNN_E_INVALID, "origins buffer too small");
        for (size_t i = 0; i < vp.origins.size(); ++i) origins[i] = vp.origins[i];
    }
    return 0;
}

int fnn_fp8_e4m3_encode(const float *in, int64_t n, uint8_t *out) {
    if (!in || !out || n < 0) return fail(nullptr, FNN_E_INVALID, "NULL argument");
    for (int64_t i = 0; i < n; ++i) out[i] = f2e4m3(in[i]);
    return 0;
}

int fnn_set_profiling(fnn_engine *e, int enabled) { if (!e) return FNN_E_INVALID; e->profiling = enabled != 0; return 0; }

int fnn_get_profile(const fnn_engine *e, fnn_profile *out) { if (!e || !out) return FNN_E_INVALID; *out = e->prof; return 0; }

int64_t fnn_kernel_log(const fnn_engine *e, char *buf, int64_t cap) { return e ? copy_text(lines(e->klog), buf, cap) : FNN_E_INVALID; }

int64_t fnn_profile_launches(const fnn_engine *e, char *buf, int64_t cap) { return e ? copy_text(lines(e->launch_rows), buf, cap) : FNN_E_INVALID; }

int64_t fnn_layer_table(const fnn_engine *e, char *buf, int64_t cap) { return e ? copy_text(layer_table_text(e->plan), buf, cap) : FNN_E_INVALID; }

int64_t fnn_plan_table(const fnn_arch_desc *arch, int max_batch, char *buf, int64_t cap) {
    if (!arch) return fail(nullptr, FNN_E_INVALID, "NULL argument");
    LayerPlan plan;
    if (int rc = make_plan(arch, max_batch, plan)) return rc;
    return copy_text(layer_table_text(plan), buf, cap);
}

int fnn_patch_work(const fnn_engine *e, double *flops, double *act_bytes) {
    if (!e) return FNN_E_INVALID;
    if (flops) *flops = e->plan.patch_flops;
    if (act_bytes) *act_bytes = e->plan.patch_act_bytes;
    return 0;
}

}  // extern "C"
