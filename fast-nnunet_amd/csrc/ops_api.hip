// ops_api.hip - single-op entry points of include/fnn.h (fnn_op_*).
//
// Parity tests drive the HIP kernels one at a time through these: host float32
// NCDHW tensors in, host float32 out.  The wrapper does what the engine does
// around a kernel: convert to fp16 channels-last with padded channels, pack the
// weights into MFMA fragment order, provide the producer-side InstanceNorm
// statistics, launch, convert back.
#include "host_call.h"

#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace {

inline int pad16(int c) { return (c + 15) / 16 * 16; }
inline float h2f_bits(uint16_t b) { f16 h; memcpy(&h, &b, 2); return (float)h; }

// Element (batch item b, channel ch, voxel v) of a device tensor of cp (padded) channels: channels-last [n][vox][cp], or
// chunk-major [n][cp / 16][vox][16] (fnn_device.h, SrcDesc)
inline size_t layout_index(bool chunk_major, int b, int ch, size_t v, int cp, size_t vox) {
    return chunk_major ? ((size_t)b * cp / 16 + ch / 16) * vox * 16 + v * 16 + ch % 16 : ((size_t)b * vox + v) * cp + ch;
}

// NCDHW fp32 -> NDHWC fp16 with channel padding; also the per-(n,c) statistics of the rounded values
// FNN_OP_CHUNK_MAJOR=1 (next to FNN_KNOBS=1; read per call): tensors of more than 16 channels travel chunk-major
// ([C / 16][voxels][16]; fnn_device.h, SrcDesc) through the conv / transposed-conv ops, as in the engine
bool op_chunk_major(int cp) { const char *v = fnn_knob("FNN_OP_CHUNK_MAJOR"); return v && v[0] != '0' && cp > 16; }
// FNN_OP_F8=1 (next to FNN_KNOBS=1; read per call): e4m3 operands on the layers the engine's FNN_PREC_F8 plan gives them
// (conv_choose_fp8), weights and output scales packed as the engine packs them
bool op_fp8() { const char *v = fnn_knob("FNN_OP_F8"); return v && v[0] != '0'; }

void to_ndhwc(const float *x, int n, int c, int cp, size_t vox, std::vector<uint16_t> &out, std::vector<double> *stats, bool cm = false) {
    out.assign((size_t)n * vox * cp, 0);
    if (stats) stats->assign((size_t)n * FNN_STAT_REPL * cp * 2, 0.0);
    for (int b = 0; b < n; ++b)
        for (int ch = 0; ch < c; ++ch) {
            double s1 = 0, s2 = 0;
            const float *src = x + ((size_t)b * c + ch) * vox;
            for (size_t v = 0; v < vox; ++v) {
                const uint16_t hb = fnn_half_bits(src[v]);
                out[layout_index(cm, b, ch, v, cp, vox)] = hb;
                const double f = h2f_bits(hb);
                s1 += f; s2 += f * f;
            }
            if (stats) {
                // spread over two replicas to exercise the replica sum
                double *st = stats->data() + ((size_t)b * FNN_STAT_REPL * cp + ch) * 2;
                st[0] = s1 * 0.25; st[1] = s2 * 0.25;
                st[(size_t)3 * cp * 2] = s1 * 0.75; st[(size_t)3 * cp * 2 + 1] = s2 * 0.75;
            }
        }
}

struct SrcHolder {
    DevBuf act, stats, gamma, beta, ss, ssh;
    SrcDesc d{};
};

bool make_src(SrcHolder &h, const float *x, int n, int c, size_t vox, const float *gamma, const float *beta, float slope,
              bool layout_aware = false, int layout = -1) {
    // layout: -1 = the FNN_OP_CHUNK_MAJOR knob decides (conv ops), 0 = channels-last, 1 = chunk-major (an argument of the body ops)
    const int cp = pad16(c);
    std::vector<uint16_t> a;
    std::vector<double> st;
    const bool cm = layout < 0 ? layout_aware && op_chunk_major(cp) : layout != 0;
    to_ndhwc(x, n, c, cp, vox, a, gamma ? &st : nullptr, cm);
    if (!h.act.alloc(a.size() * 2)) return false;
    if (hipMemcpy(h.act.p, a.data(), a.size() * 2, hipMemcpyHostToDevice) != hipSuccess) return false;
    h.d.ptr = h.act.as<f16>(); h.d.C = cp; h.d.slope = 1.f;
    if (cm) { h.d.vs = 16; h.d.cs = 16LL * (long long)vox; }
    if (gamma) {
        std::vector<float> g(cp, 0.f), b(cp, 0.f);
        for (int i = 0; i < c; ++i) { g[i] = gamma[i]; b[i] = beta ? beta[i] : 0.f; }
        if (!h.stats.alloc(st.size() * 8) || !h.gamma.alloc(cp * 4) || !h.beta.alloc(cp * 4)) return false;
        (void)hipMemcpy(h.stats.p, st.data(), st.size() * 8, hipMemcpyHostToDevice);
        (void)hipMemcpy(h.gamma.p, g.data(), cp * 4, hipMemcpyHostToDevice);
        (void)hipMemcpy(h.beta.p, b.data(), cp * 4, hipMemcpyHostToDevice);
        // what the engine does between producer and consumer: statistics -> (scale, shift)
        if (!h.ss.alloc((size_t)n * cp * 8) || !h.ssh.alloc((size_t)n * cp * 4)) return false;
        StatsFinalizeParams q{};
        q.stats = h.stats.as<double>(); q.gamma = h.gamma.as<float>(); q.beta = h.beta.as<float>();
        q.ss = h.ss.as<float>(); q.ssh = h.ssh.as<unsigned short>(); q.C = cp; q.nrep = FNN_STAT_REPL; q.inv_count = 1.f / (float)vox; q.eps = 1e-5f;
        if (launch_stats_finalize(q, n, 0) != 0) return false;
        h.d.ss = h.ss.as<float>();
        h.d.ssh = h.ssh.as<unsigned short>();
        h.d.slope = slope;
    }
    return true;
}

}  // namespace


namespace {

// device tensor [n][vox][cp] (channels-last) or [n][cp / 16][vox][16] (chunk-major), fp16 -> host float32 [n][c][vox]
void from_device_layout(const std::vector<uint16_t> &ho, int n, int c, int cp, size_t vox, bool cm, float *y) {
    for (int b = 0; b < n; ++b)
        for (int ch = 0; ch < c; ++ch)
            for (size_t v = 0; v < vox; ++v)
                y[((size_t)b * c + ch) * vox + v] = h2f_bits(ho[layout_index(cm, b, ch, v, cp, vox)]);
}

// a body-op operand: make_src with the layout as an argument and the slope applied with or without a norm, as the kernels do
bool make_body_src(SrcHolder &h, const float *x, int n, int c, size_t vox, const float *gamma, const float *beta, float slope, int cm) {
    if (!make_src(h, x, n, c, vox, gamma, beta, slope, false, cm ? 1 : 0)) return false;
    h.d.slope = slope;
    return true;
}

bool upload(DevBuf &d, const void *src, size_t bytes) {
    return d.alloc(bytes) && hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice) == hipSuccess;
}

// Where a patch lands in an accumulator box: shared by the head and patch-accumulate ops
struct AccArgs { void *acc; int acc_fp32; const long long *box; const int *origin; };
bool acc_args_ok(const AccArgs &a, const int patch[3], int heads) {
    if (!a.acc || !a.box || !a.origin || heads < 1) return false;
    for (int i = 0; i < 3; ++i)
        if (patch[i] < 1 || a.origin[i] < 0 || a.box[i] < 1 || (long long)a.origin[i] + patch[i] > a.box[i]) return false;
    return true;
}

}  // namespace

// kernel variants of the last fnn_op_* call of this thread (fnn_note_kernel at the launch sites): fnn_op_last_kernels
static thread_local std::vector<std::string> g_op_kernels;
// (FnnOpKlog, fnn_device.h, holds it for a scope - here and in the entry points outside this file)
void fnn_op_klog_begin() { g_op_kernels.clear(); fnn_klog_target(&g_op_kernels); }
void fnn_op_klog_end() { fnn_klog_target(nullptr); }

extern "C" {

int fnn_op_conv3d(int device, int n, const int dims[3],
                  const float *x, int cin, const float *gamma1, const float *beta1, float slope1,
                  const float *x2, int cin2, const float *gamma2, const float *beta2, float slope2,
                  const float *w, const float *bias, int cout, const int k[3], const int stride[3],
                  float *y, double *stats_out) {
    if (!x || !w || !y || !dims || !k || !stride || n < 1 || cin < 1 || cout < 1) return FNN_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return FNN_E_HIP;
    FnnOpKlog klog;
    const size_t vox = (size_t)dims[0] * dims[1] * dims[2];
    const int nsrc = x2 ? 2 : 1;
    SrcHolder s1, s2;
    if (!make_src(s1, x, n, cin, vox, gamma1, beta1, slope1, true)) return FNN_E_HIP;
    if (x2 && !make_src(s2, x2, n, cin2, vox, gamma2, beta2, slope2, true)) return FNN_E_HIP;
    const int cp1 = pad16(cin), cp2 = x2 ? pad16(cin2) : 0, cop = pad16(cout);
    ConvParams p{};
    p.n_src = nsrc; p.src[0] = s1.d;
    if (x2) p.src[1] = s2.d; else { p.src[1] = s1.d; p.src[1].C = 0; }
    p.N = n; p.Di = dims[0]; p.Hi = dims[1]; p.Wi = dims[2];
    p.kd = k[0]; p.kh = k[1]; p.kw = k[2]; p.sd = stride[0]; p.sh = stride[1]; p.sw = stride[2];
    p.pd = (k[0] - 1) / 2; p.ph = (k[1] - 1) / 2; p.pw = (k[2] - 1) / 2;
    p.Do = (p.Di + 2 * p.pd - p.kd) / p.sd + 1; p.Ho = (p.Hi + 2 * p.ph - p.kh) / p.sh + 1; p.Wo = (p.Wi + 2 * p.pw - p.kw) / p.sw + 1;
    p.Cout = cop; p.chunks = (cp1 + cp2) / 16;
    p.fp8 = op_fp8();
    ThinParams tp{};
    tp.c = p;
    ConvChoice cc;                                  // chosen per call, for this call's N (the engine chooses for its planned batch)
    if (!conv_choose_fp8(tp, ConvOverrides::from_env(), cc)) return FNN_E_UNSUPPORTED;
    p.fp8 = tp.c.fp8;
    auto launch = [&]() { tp.c = p; return launch_conv(tp, cc, 0); };
    const size_t slots = (size_t)cc.stats_slots;
    std::vector<uint16_t> wp(conv_packed_halves(cc, cop), 0);
    std::vector<float> scales(p.fp8 ? cop : 0, 0.f);
    const int cin_real[2] = {cin, x2 ? cin2 : 0};
    conv_pack_weights(p, cc, cout, cin_real, w, wp.data(), p.fp8 ? scales.data() : nullptr);
    std::vector<float> bp(cop, 0.f);
    if (bias) for (int i = 0; i < cout; ++i) bp[i] = bias[i];
    const size_t ovox = (size_t)p.Do * p.Ho * p.Wo;
    DevBuf dw, db, dsc, dout, dst;
    if (!dw.alloc(fnn_weight_alloc_bytes(wp.size())) || !db.alloc(cop * 4) || !dout.alloc((size_t)n * ovox * cop * 2) ||
        !dst.alloc((size_t)n * slots * cop * 16) || (p.fp8 && !dsc.alloc(cop * 4))) return FNN_E_HIP;
    (void)hipMemcpy(dw.p, wp.data(), wp.size() * 2, hipMemcpyHostToDevice);
    (void)hipMemcpy(db.p, bp.data(), cop * 4, hipMemcpyHostToDevice);
    if (p.fp8) (void)hipMemcpy(dsc.p, scales.data(), cop * 4, hipMemcpyHostToDevice);
    (void)hipMemset(dst.p, 0, (size_t)n * slots * cop * 16);
    (void)hipMemset(dout.p, 0, (size_t)n * ovox * cop * 2);
    p.wpk = dw.as<f16>(); p.bias = db.as<float>(); p.out = dout.as<f16>(); p.stats_out = dst.as<double>();
    p.oscale = p.fp8 ? dsc.as<float>() : nullptr; p.act_mult = FNN_FP8_ACT_MULT;
    const bool ocm = op_chunk_major(cop);
    if (ocm) { p.out_vs = 16; p.out_cs = 16LL * (long long)ovox; }
#ifdef FNN_STAMPS
    DevBuf ddbg;
    const size_t dbg_n = (size_t)1 << 20;
    if (!ddbg.alloc(dbg_n * 8)) return FNN_E_HIP;
    (void)hipMemset(ddbg.p, 0, dbg_n * 8);
    p.dbg = ddbg.as<unsigned long long>();
    (void)launch();                      // warm-up
    (void)hipDeviceSynchronize();
    (void)hipMemset(dst.p, 0, (size_t)n * slots * cop * 16);
#endif
    if (fnn_knob("FNN_OP_TIME")) {                    // diagnostic: mean duration of 30 launches of this layer (after 2 warm-ups)
        Event e0, e1;
        (void)e0.create(hipEventDefault); (void)e1.create(hipEventDefault);
        for (int i = 0; i < 2; ++i) (void)launch();
        (void)hipEventRecord(e0, 0);
        for (int i = 0; i < 30; ++i) (void)launch();
        (void)hipEventRecord(e1, 0);
        (void)hipDeviceSynchronize();
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e0, e1);
        fprintf(stderr, "[op time] conv3d %d+%d -> %d at %dx%dx%d, N = %d: %.1f us per launch\n", cin, cin2, cout, p.Di, p.Hi, p.Wi, n, ms * (1000.f / 30.f));
        (void)hipMemset(dst.p, 0, (size_t)n * slots * cop * 16);
    }
#ifdef FNN_STAMPS
    Event ev0, ev1;
    (void)ev0.create(hipEventDefault); (void)ev1.create(hipEventDefault);
    (void)hipEventRecord(ev0, 0);
#endif
    const int rc = launch();
    if (rc != 0) return rc == -1 ? FNN_E_UNSUPPORTED : FNN_E_HIP;
#ifdef FNN_STAMPS
    (void)hipEventRecord(ev1, 0);
#endif
    if (hipDeviceSynchronize() != hipSuccess) return FNN_E_HIP;
#ifdef FNN_STAMPS
    {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ev0, ev1);
        fprintf(stderr, "[stamps] launch %.1f us; ", ms * 1000.f);
        std::vector<unsigned long long> h(dbg_n);
        (void)hipMemcpy(h.data(), ddbg.p, dbg_n * 8, hipMemcpyDeviceToHost);
        double sum[12] = {0}; long cnt = 0;
        unsigned long long tmin = ~0ull, tmax = 0;
        for (size_t w = 0; w * 12 + 11 < dbg_n; ++w) {
            if (h[w * 12] == 0) continue;
            ++cnt;
            int last = 0;
            for (int i = 1; i < 12; ++i) if (h[w * 12 + i]) { sum[i] += (double)(h[w * 12 + i] - h[w * 12 + i - 1]); last = i; }
            if (h[w * 12] < tmin) tmin = h[w * 12];
            if (h[w * 12 + last] > tmax) tmax = h[w * 12 + last];
        }
        fprintf(stderr, "[stamps] %ld workgroups, kernel span %.0f ticks; mean ticks per segment:", cnt, (double)(tmax - tmin));
        for (int i = 1; i < 12; ++i) fprintf(stderr, " %d:%.0f", i, cnt ? sum[i] / cnt : 0.0);
        fprintf(stderr, "\n");
    }
#endif
    std::vector<uint16_t> ho((size_t)n * ovox * cop);
    std::vector<double> hs((size_t)n * slots * cop * 2);
    (void)hipMemcpy(ho.data(), dout.p, ho.size() * 2, hipMemcpyDeviceToHost);
    (void)hipMemcpy(hs.data(), dst.p, hs.size() * 8, hipMemcpyDeviceToHost);
    for (int b = 0; b < n; ++b)
        for (int co = 0; co < cout; ++co) {
            for (size_t v = 0; v < ovox; ++v)
                y[((size_t)b * cout + co) * ovox + v] = h2f_bits(ho[layout_index(ocm, b, co, v, cop, ovox)]);
            if (stats_out) {
                double a = 0, q = 0;
                for (size_t r = 0; r < slots; ++r) {
                    a += hs[(((size_t)b * slots + r) * cop + co) * 2];
                    q += hs[(((size_t)b * slots + r) * cop + co) * 2 + 1];
                }
                stats_out[((size_t)b * cout + co) * 2] = a;
                stats_out[((size_t)b * cout + co) * 2 + 1] = q;
            }
        }
    return 0;
}

int fnn_op_conv_transpose3d(int device, int n, const int dims[3],
                            const float *x, int cin, const float *gamma1, const float *beta1, float slope1,
                            const float *w, const float *bias, int cout, const int stride[3], float *y) {
    if (!x || !w || !y || !dims || !stride || n < 1 || cin < 1 || cout < 1) return FNN_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return FNN_E_HIP;
    FnnOpKlog klog;
    const size_t vox = (size_t)dims[0] * dims[1] * dims[2];
    SrcHolder s1;
    if (!make_src(s1, x, n, cin, vox, gamma1, beta1, slope1, true)) return FNN_E_HIP;
    const int cp = pad16(cin), cop = pad16(cout);
    const int taps = stride[0] * stride[1] * stride[2];
    TconvParams p{};
    p.src = s1.d; p.N = n; p.Di = dims[0]; p.Hi = dims[1]; p.Wi = dims[2];
    p.sd = stride[0]; p.sh = stride[1]; p.sw = stride[2];
    p.Cout = cop; p.nblk = cop / 16; p.ksteps = (cp + 31) / 32;
    std::vector<uint16_t> wp((size_t)taps * p.nblk * p.ksteps * 512, 0);
    tconv_pack_weights(w, cin, cout, cop, taps, p.ksteps, wp.data());
    std::vector<float> bp(cop, 0.f);
    if (bias) for (int i = 0; i < cout; ++i) bp[i] = bias[i];
    const size_t ovox = vox * taps;
    DevBuf dw, db, dout;
    if (!dw.alloc(wp.size() * 2) || !db.alloc(cop * 4) || !dout.alloc((size_t)n * ovox * cop * 2)) return FNN_E_HIP;
    (void)hipMemcpy(dw.p, wp.data(), wp.size() * 2, hipMemcpyHostToDevice);
    (void)hipMemcpy(db.p, bp.data(), cop * 4, hipMemcpyHostToDevice);
    (void)hipMemset(dout.p, 0, (size_t)n * ovox * cop * 2);
    p.wpk = dw.as<f16>(); p.bias = db.as<float>(); p.out = dout.as<f16>();
    const bool ocm = op_chunk_major(cop);
    if (ocm) { p.out_vs = 16; p.out_cs = 16LL * (long long)ovox; }
    if (launch_tconv(p, 0) != 0) return FNN_E_HIP;
    if (hipDeviceSynchronize() != hipSuccess) return FNN_E_HIP;
    std::vector<uint16_t> ho((size_t)n * ovox * cop);
    (void)hipMemcpy(ho.data(), dout.p, ho.size() * 2, hipMemcpyDeviceToHost);
    from_device_layout(ho, n, cout, cop, ovox, ocm, y);
    return 0;
}

int fnn_op_avgpool(int device, int n, const int dims[3], const float *x, int c,
                   const float *gamma, const float *beta, float slope, const int stride[3],
                   int x_chunk_major, int y_chunk_major, float *y) {
    if (!x || !y || !dims || !stride || n < 1 || c < 1) return FNN_E_INVALID;
    for (int i = 0; i < 3; ++i) if (stride[i] < 1 || dims[i] < stride[i]) return FNN_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return FNN_E_HIP;
    FnnOpKlog klog;
    const size_t vox = (size_t)dims[0] * dims[1] * dims[2];
    const int cp = pad16(c);
    SrcHolder s;
    if (!make_body_src(s, x, n, c, vox, gamma, beta, slope, x_chunk_major)) return FNN_E_HIP;
    PoolParams p{};
    p.src = s.d; p.N = n; p.Di = dims[0]; p.Hi = dims[1]; p.Wi = dims[2];
    p.sd = stride[0]; p.sh = stride[1]; p.sw = stride[2];
    const size_t ovox = (size_t)(dims[0] / stride[0]) * (dims[1] / stride[1]) * (dims[2] / stride[2]);
    DevBuf dout;
    if (!dout.alloc((size_t)n * ovox * cp * 2)) return FNN_E_HIP;
    (void)hipMemset(dout.p, 0, (size_t)n * ovox * cp * 2);
    p.out = dout.as<f16>();
    if (y_chunk_major) { p.out_vs = 16; p.out_cs = 16LL * (long long)ovox; }
    if (launch_avgpool(p, 0) != 0) return FNN_E_HIP;
    if (hipDeviceSynchronize() != hipSuccess) return FNN_E_HIP;
    std::vector<uint16_t> ho((size_t)n * ovox * cp);
    (void)hipMemcpy(ho.data(), dout.p, ho.size() * 2, hipMemcpyDeviceToHost);
    from_device_layout(ho, n, c, cp, ovox, y_chunk_major != 0, y);
    return 0;
}

int fnn_op_combine(int device, int n, const int dims[3], int c,
                   const float *a, const float *gamma_a, const float *beta_a, float slope_a,
                   const float *b, const float *gamma_b, const float *beta_b, float slope_b,
                   float slope, const int pool_stride[3],
                   int a_chunk_major, int b_chunk_major, int y_chunk_major, int pooled_chunk_major,
                   float *y, float *pooled) {
    if (!a || !b || !y || !dims || n < 1 || c < 1 || (pool_stride && !pooled)) return FNN_E_INVALID;
    for (int i = 0; i < 3; ++i) if (dims[i] < 1) return FNN_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return FNN_E_HIP;
    FnnOpKlog klog;
    const size_t vox = (size_t)dims[0] * dims[1] * dims[2];
    const int cp = pad16(c);
    SrcHolder sa, sb;
    if (!make_body_src(sa, a, n, c, vox, gamma_a, beta_a, slope_a, a_chunk_major)) return FNN_E_HIP;
    if (!make_body_src(sb, b, n, c, vox, gamma_b, beta_b, slope_b, b_chunk_major)) return FNN_E_HIP;
    CombineParams p{};
    p.a = sa.d; p.b = sb.d; p.vox = (long long)vox; p.N = n; p.slope = slope;
    DevBuf dout, dpool;
    if (!dout.alloc((size_t)n * vox * cp * 2)) return FNN_E_HIP;
    (void)hipMemset(dout.p, 0, (size_t)n * vox * cp * 2);
    p.out = dout.as<f16>();
    if (y_chunk_major) { p.out_vs = 16; p.out_cs = 16LL * (long long)vox; }
    size_t pvox = 0;
    if (pool_stride) {
        // the launcher takes the strides combine_pool_kernel serves and sizes that are multiples of them; anything else is
        // the caller's to send through fnn_op_avgpool, as the planner does
        if (!combine_pool_ok(dims[0], dims[1], dims[2], pool_stride[0], pool_stride[1], pool_stride[2])) return FNN_E_UNSUPPORTED;
        pvox = (size_t)(dims[0] / pool_stride[0]) * (dims[1] / pool_stride[1]) * (dims[2] / pool_stride[2]);
        if (!dpool.alloc((size_t)n * pvox * cp * 2)) return FNN_E_HIP;
        (void)hipMemset(dpool.p, 0, (size_t)n * pvox * cp * 2);
        p.pool_out = dpool.as<f16>();
        p.D = dims[0]; p.H = dims[1]; p.W = dims[2];
        p.psd = pool_stride[0]; p.psh = pool_stride[1]; p.psw = pool_stride[2];
        if (pooled_chunk_major) { p.pool_vs = 16; p.pool_cs = 16LL * (long long)pvox; }
    }
    const int rc = launch_combine(p, 0);
    if (rc != 0) return rc == -1 ? FNN_E_UNSUPPORTED : FNN_E_HIP;
    if (hipDeviceSynchronize() != hipSuccess) return FNN_E_HIP;
    std::vector<uint16_t> ho((size_t)n * vox * cp);
    (void)hipMemcpy(ho.data(), dout.p, ho.size() * 2, hipMemcpyDeviceToHost);
    from_device_layout(ho, n, c, cp, vox, y_chunk_major != 0, y);
    if (pool_stride) {
        ho.resize((size_t)n * pvox * cp);
        (void)hipMemcpy(ho.data(), dpool.p, ho.size() * 2, hipMemcpyDeviceToHost);
        from_device_layout(ho, n, c, cp, pvox, pooled_chunk_major != 0, pooled);
    }
    return 0;
}

int fnn_op_seg_head(int device, int n, int c, const int patch[3], const float *x,
                    const float *gamma, const float *beta, float slope,
                    int heads, const float *w, const float *bias,
                    int item, int mode, const int flips[3], const unsigned short *gauss,
                    void *acc, int acc_fp32, const long long box[3], const int origin[3], const int first_visit[3],
                    float *patch_buf, int *first_visit_honoured) {
    if (!x || !w || !patch || !flips || n < 1 || c < 1 || heads < 1 || item < 0 || item >= n || mode < 0 || mode > 2) return FNN_E_INVALID;
    for (int i = 0; i < 3; ++i) if (patch[i] < 1) return FNN_E_INVALID;
    const AccArgs aa{acc, acc_fp32, box, origin};
    if (mode == 0 ? !acc_args_ok(aa, patch, heads) : !patch_buf) return FNN_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return FNN_E_HIP;
    FnnOpKlog klog;
    const size_t P = (size_t)patch[0] * patch[1] * patch[2];
    const int cp = pad16(c);
    SrcHolder s;                                    // the head kernels read channels-last features
    if (!make_body_src(s, x, n, c, P, gamma, beta, slope, 0)) return FNN_E_HIP;
    HeadParams h{};
    h.src = s.d; h.b = item; h.PD = patch[0]; h.PH = patch[1]; h.PW = patch[2];
    h.heads = heads; h.hblocks = (heads + 1 + 15) / 16; h.ksteps = (cp + 31) / 32;      // as the engine plans them
    h.HP = (heads + 1 + 7) / 8 * 8;
    h.flip_d = flips[0]; h.flip_h = flips[1]; h.flip_w = flips[2];
    h.mode = mode; h.acc_fp32 = acc_fp32;
    h.fx = h.fy = h.fz = 0x7fffffff;
    std::vector<uint16_t> wp((size_t)h.hblocks * h.ksteps * 512);
    std::vector<float> bp((size_t)h.hblocks * 16);
    pack_head(heads, c, h.hblocks, h.ksteps, w, wp.data());
    pack_head_bias(heads, h.hblocks, bias, bp.data());
    DevBuf dw, db, dg, dacc, dpb;
    if (!upload(dw, wp.data(), wp.size() * 2) || !upload(db, bp.data(), bp.size() * 4)) return FNN_E_HIP;
    h.wpk = dw.as<f16>(); h.bias = db.as<float>();
    size_t acc_bytes = 0;
    if (mode == 0) {
        // the weight map: the caller's, or the all-ones map the engine keeps for use_gaussian = 0
        std::vector<uint16_t> ones;
        if (!gauss) ones.assign(P, fnn_half_bits(1.f));
        if (!upload(dg, gauss ? gauss : ones.data(), P * 2)) return FNN_E_HIP;
        h.gauss = dg.as<f16>();
        h.AX = box[0]; h.Y = box[1]; h.Z = box[2];
        h.ox = origin[0]; h.oy = origin[1]; h.oz = origin[2];
        acc_bytes = (size_t)box[0] * box[1] * box[2] * h.HP * (acc_fp32 ? 4 : 2);
        if (!upload(dacc, acc, acc_bytes)) return FNN_E_HIP;
        h.acc = dacc.p;
    } else {
        if (!upload(dpb, patch_buf, (size_t)heads * P * 4)) return FNN_E_HIP;
        h.patch_buf = dpb.as<float>();
    }
    const bool fv_ok = launch_head_first_visit_ok(h);
    if (first_visit_honoured) *first_visit_honoured = fv_ok ? 1 : 0;
    if (first_visit) {
        const bool all_read = first_visit[0] == 0x7fffffff && first_visit[1] == 0x7fffffff && first_visit[2] == 0x7fffffff;
        if (!fv_ok && !all_read) return FNN_E_UNSUPPORTED;
        h.fx = first_visit[0]; h.fy = first_visit[1]; h.fz = first_visit[2];
    }
    if (launch_head(h, 0) != 0) return FNN_E_HIP;
    if (hipDeviceSynchronize() != hipSuccess) return FNN_E_HIP;
    if (mode == 0) (void)hipMemcpy(acc, dacc.p, acc_bytes, hipMemcpyDeviceToHost);
    else (void)hipMemcpy(patch_buf, dpb.p, (size_t)heads * P * 4, hipMemcpyDeviceToHost);
    return 0;
}

int fnn_op_patch_acc(int device, const float *patch_buf, int heads, const int patch[3], int n_div,
                     const unsigned short *gauss, void *acc, int acc_fp32, const long long box[3], const int origin[3]) {
    const AccArgs aa{acc, acc_fp32, box, origin};
    if (!patch_buf || !patch || n_div < 1 || !acc_args_ok(aa, patch, heads)) return FNN_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return FNN_E_HIP;
    FnnOpKlog klog;
    const size_t P = (size_t)patch[0] * patch[1] * patch[2];
    PatchAccParams q{};
    q.n_div = n_div; q.PD = patch[0]; q.PH = patch[1]; q.PW = patch[2]; q.heads = heads;
    q.AX = box[0]; q.Y = box[1]; q.Z = box[2]; q.HP = (heads + 1 + 7) / 8 * 8;
    q.ox = origin[0]; q.oy = origin[1]; q.oz = origin[2]; q.acc_fp32 = acc_fp32;
    const size_t acc_bytes = (size_t)box[0] * box[1] * box[2] * q.HP * (acc_fp32 ? 4 : 2);
    DevBuf dpb, dg, dacc;
    if (!upload(dpb, patch_buf, (size_t)heads * P * 4) || !upload(dacc, acc, acc_bytes)) return FNN_E_HIP;
    if (gauss && !upload(dg, gauss, P * 2)) return FNN_E_HIP;
    q.patch_buf = dpb.as<float>(); q.gauss = gauss ? dg.as<f16>() : nullptr; q.acc = dacc.p;
    if (launch_patch_acc(q, 0) != 0) return FNN_E_HIP;
    if (hipDeviceSynchronize() != hipSuccess) return FNN_E_HIP;
    (void)hipMemcpy(acc, dacc.p, acc_bytes, hipMemcpyDeviceToHost);
    return 0;
}

int fnn_op_patch_input(int device, const float *vol, int n_vol, int c, const long long vdim[3],
                       int n, const int *origins, const int flips[3], const int patch[3], int cpad, int chunk_major,
                       unsigned short *out) {
    if (!vol || !vdim || !origins || !flips || !patch || !out || n < 1 || c < 1 || cpad < c || cpad % 16 != 0) return FNN_E_INVALID;
    if (n_vol != 1 && n_vol != n) return FNN_E_INVALID;
    for (int b = 0; b < n; ++b)
        for (int i = 0; i < 3; ++i)
            if (patch[i] < 1 || origins[b * 3 + i] < 0 || (long long)origins[b * 3 + i] + patch[i] > vdim[i]) return FNN_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return FNN_E_HIP;
    FnnOpKlog klog;
    const size_t P = (size_t)patch[0] * patch[1] * patch[2];
    const size_t vvox = (size_t)vdim[0] * vdim[1] * vdim[2];
    PatchInputParams p{};
    DevBuf dvol, dorg, dout;
    if (!upload(dvol, vol, (size_t)n_vol * c * vvox * 4) || !upload(dorg, origins, (size_t)n * 3 * 4)) return FNN_E_HIP;
    if (!dout.alloc((size_t)n * P * cpad * 2)) return FNN_E_HIP;
    (void)hipMemset(dout.p, 0xff, (size_t)n * P * cpad * 2);               // (NaN bits: the kernel writes the padding channels)
    p.vol = dvol.as<float>(); p.vol_batch_stride = n_vol == 1 ? 0 : (long long)c * (long long)vvox;
    p.C = c; p.Cpad = cpad; p.X = vdim[0]; p.Y = vdim[1]; p.Z = vdim[2];
    p.origins = dorg.as<int>();
    p.flip_d = flips[0]; p.flip_h = flips[1]; p.flip_w = flips[2];
    p.PD = patch[0]; p.PH = patch[1]; p.PW = patch[2]; p.N = n;
    p.out = dout.as<f16>();
    if (chunk_major) { p.out_vs = 16; p.out_cs = 16LL * (long long)P; }
    if (launch_patch_input(p, 0) != 0) return FNN_E_HIP;
    if (hipDeviceSynchronize() != hipSuccess) return FNN_E_HIP;
    std::vector<uint16_t> ho((size_t)n * P * cpad);
    (void)hipMemcpy(ho.data(), dout.p, ho.size() * 2, hipMemcpyDeviceToHost);
    for (int b = 0; b < n; ++b)
        for (int ch = 0; ch < cpad; ++ch)
            for (size_t v = 0; v < P; ++v)
                out[((size_t)b * cpad + ch) * P + v] = ho[layout_index(chunk_major != 0, b, ch, v, cpad, P)];
    return 0;
}

}  // extern "C"

namespace {

// The stem of a batch of patch windows as forward_batch launches it: the fp32 volumes, the origins, StemParams with p.w in
// [C][taps][Cout] and the stem_mfma_pack fragments, one zeroed statistics row per slot
struct StemHolder {
    DevBuf vol, org, w, bias, frag, stats;
    StemParams p{};
    int cop = 0, slots = 0;
    size_t P = 0;
};

int make_stem(StemHolder &h, const float *vol, int n_vol, int c, const long long vdim[3], int n, const int *origins, const int flips[3],
              const int patch[3], const float *w, const float *bias, int cout, const int k[3]) {
    if (!vol || !vdim || !origins || !flips || !patch || !w || !k || n < 1 || c < 1 || cout < 1) return FNN_E_INVALID;
    if (n_vol != 1 && n_vol != n) return FNN_E_INVALID;
    for (int b = 0; b < n; ++b)
        for (int i = 0; i < 3; ++i)
            if (patch[i] < 1 || origins[b * 3 + i] < 0 || (long long)origins[b * 3 + i] + patch[i] > vdim[i]) return FNN_E_INVALID;
    h.cop = pad16(cout);
    if (!stem_mfma_ok(c, k[0], k[1], k[2], h.cop)) return FNN_E_UNSUPPORTED;
    const int T = k[0] * k[1] * k[2];
    const size_t vvox = (size_t)vdim[0] * vdim[1] * vdim[2];
    h.P = (size_t)patch[0] * patch[1] * patch[2];
    h.slots = stem_mfma_stats_slots(patch[0], patch[1], patch[2]);
    std::vector<float> wt((size_t)c * T * h.cop, 0.f), bp(h.cop, 0.f);
    for (int ci = 0; ci < c; ++ci)
        for (int t = 0; t < T; ++t)
            for (int co = 0; co < cout; ++co) wt[((size_t)ci * T + t) * h.cop + co] = w[((size_t)co * c + ci) * T + t];
    if (bias) for (int i = 0; i < cout; ++i) bp[i] = bias[i];
    std::vector<uint16_t> frag((size_t)(h.cop / 16) * stem_mfma_ksteps(c, T) * 512, 0);
    stem_mfma_pack(w, c, T, cout, h.cop, frag.data());
    const size_t stat_bytes = (size_t)n * h.slots * h.cop * 16;
    if (!upload(h.vol, vol, (size_t)n_vol * c * vvox * 4) || !upload(h.org, origins, (size_t)n * 3 * 4) || !upload(h.w, wt.data(), wt.size() * 4) ||
        !upload(h.bias, bp.data(), bp.size() * 4) || !upload(h.frag, frag.data(), frag.size() * 2) || !h.stats.alloc(stat_bytes)) return FNN_E_HIP;
    (void)hipMemset(h.stats.p, 0, stat_bytes);
    StemParams &p = h.p;
    p.vol = h.vol.as<float>(); p.vol_batch_stride = n_vol == 1 ? 0 : (long long)c * (long long)vvox; p.C = c;
    p.X = vdim[0]; p.Y = vdim[1]; p.Z = vdim[2];
    p.origins = h.org.as<int>();
    p.flip_d = flips[0]; p.flip_h = flips[1]; p.flip_w = flips[2];
    p.PD = patch[0]; p.PH = patch[1]; p.PW = patch[2];
    p.kd = k[0]; p.kh = k[1]; p.kw = k[2];
    p.Cout = h.cop;
    p.w = h.w.as<float>(); p.bias = h.bias.as<float>();
    p.stats_out = h.stats.as<double>();
    return FNN_OK;
}

// statistics rows [n][slots][cop][2] on the device -> host [n][cout][2], summed over the slot rows
void sum_stat_rows(const DevBuf &dst, int n, size_t slots, int cout, int cop, double *stats_out) {
    std::vector<double> hs((size_t)n * slots * cop * 2);
    (void)hipMemcpy(hs.data(), dst.p, hs.size() * 8, hipMemcpyDeviceToHost);
    for (int b = 0; b < n; ++b)
        for (int co = 0; co < cout; ++co) {
            double a = 0, q = 0;
            for (size_t r = 0; r < slots; ++r) {
                a += hs[(((size_t)b * slots + r) * cop + co) * 2];
                q += hs[(((size_t)b * slots + r) * cop + co) * 2 + 1];
            }
            stats_out[((size_t)b * cout + co) * 2] = a;
            stats_out[((size_t)b * cout + co) * 2 + 1] = q;
        }
}

}  // namespace

extern "C" {

int fnn_op_stem(int device, const float *vol, int n_vol, int c, const long long vdim[3],
                int n, const int *origins, const int flips[3], const int patch[3],
                const float *w, const float *bias, int cout, const int k[3], float *y, double *stats_out) {
    if (!y) return FNN_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return FNN_E_HIP;
    FnnOpKlog klog;
    StemHolder s;
    if (const int rc = make_stem(s, vol, n_vol, c, vdim, n, origins, flips, patch, w, bias, cout, k)) return rc;
    DevBuf dout;
    if (!dout.alloc((size_t)n * s.P * s.cop * 2)) return FNN_E_HIP;
    (void)hipMemset(dout.p, 0, (size_t)n * s.P * s.cop * 2);
    s.p.out = dout.as<f16>();
    const int rc = launch_stem_mfma(s.p, s.frag.as<f16>(), n, 0);
    if (rc != 0) return rc == -1 ? FNN_E_UNSUPPORTED : FNN_E_HIP;
    if (hipDeviceSynchronize() != hipSuccess) return FNN_E_HIP;
    std::vector<uint16_t> ho((size_t)n * s.P * s.cop);
    (void)hipMemcpy(ho.data(), dout.p, ho.size() * 2, hipMemcpyDeviceToHost);
    from_device_layout(ho, n, cout, s.cop, s.P, false, y);
    if (stats_out) sum_stat_rows(s.stats, n, (size_t)s.slots, cout, s.cop, stats_out);
    return 0;
}

int fnn_op_conv_fused(int device, int mode, int n, const int dims[3],
                      const float *vol, int n_vol, const long long vdim[3], const int *origins, const int flips[3],
                      const float *low, int low_c, const int tstride[3],
                      const float *skip, const float *skip_gamma, const float *skip_beta, float skip_slope,
                      const float *pw, const float *pbias, const float *pgamma, const float *pbeta, float pslope,
                      const float *w, const float *bias, const int k[3], float *y, double *stats_out) {
    if ((mode != FUSE_STEM && mode != FUSE_TCONV) || !dims || !pw || !w || !k || !y || n < 1) return FNN_E_INVALID;
    for (int i = 0; i < 3; ++i) if (dims[i] < 1 || (k[i] != 1 && k[i] != 3)) return FNN_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return FNN_E_HIP;
    FnnOpKlog klog;
    const size_t vox = (size_t)dims[0] * dims[1] * dims[2];
    const int cop = 16;
    DevBuf dout, dst;
    if (!dout.alloc((size_t)n * vox * cop * 2)) return FNN_E_HIP;
    (void)hipMemset(dout.p, 0, (size_t)n * vox * cop * 2);
    ThinParams tp{};
    ConvParams &p = tp.c;
    tp.fuse = mode;
    p.N = n; p.Di = p.Do = dims[0]; p.Hi = p.Ho = dims[1]; p.Wi = p.Wo = dims[2];
    p.kd = k[0]; p.kh = k[1]; p.kw = k[2]; p.sd = p.sh = p.sw = 1;
    p.pd = (k[0] - 1) / 2; p.ph = (k[1] - 1) / 2; p.pw = (k[2] - 1) / 2;
    p.Cout = cop;
    tp.tsd = tp.tsh = tp.tsw = 1;
    StemHolder s;
    SrcHolder slow, sskip;
    DevBuf dg, db, dss, dssh, dfw, dfb;
    int cin_real[2] = {16, 0};
    if (mode == FUSE_STEM) {
        // the stem's statistics pass, their (scale, shift) rows, then the consumer that recomputes the stem while it stages
        if (!pgamma || !pbeta) return FNN_E_INVALID;
        if (const int rc = make_stem(s, vol, n_vol, 1, vdim, n, origins, flips, dims, pw, pbias, 16, k)) return rc;
        s.p.out = nullptr;
        const int rc = launch_stem_mfma(s.p, s.frag.as<f16>(), n, 0);
        if (rc != 0) return rc == -1 ? FNN_E_UNSUPPORTED : FNN_E_HIP;
        if (!upload(dg, pgamma, 16 * 4) || !upload(db, pbeta, 16 * 4) || !dss.alloc((size_t)n * 16 * 8) || !dssh.alloc((size_t)n * 16 * 4)) return FNN_E_HIP;
        StatsFinalizeParams q{};
        q.stats = s.stats.as<double>(); q.gamma = dg.as<float>(); q.beta = db.as<float>();
        q.ss = dss.as<float>(); q.ssh = dssh.as<unsigned short>(); q.C = 16; q.nrep = s.slots; q.inv_count = 1.f / (float)vox; q.eps = 1e-5f;
        if (launch_stats_finalize(q, n, 0) != 0) return FNN_E_HIP;
        p.n_src = 1; p.chunks = 1;
        p.src[0].ptr = dout.as<f16>();                                // the stem's output is virtual: never read
        p.src[0].C = 16; p.src[0].ss = dss.as<float>(); p.src[0].ssh = dssh.as<unsigned short>(); p.src[0].slope = pslope;
        p.src[1] = p.src[0]; p.src[1].C = 0;
        tp.fw = s.frag.as<f16>(); tp.fbias = s.p.bias;
        tp.vol = s.p.vol; tp.vol_batch_stride = s.p.vol_batch_stride; tp.Y = s.p.Y; tp.Z = s.p.Z;
        tp.origins = s.p.origins; tp.flip_d = s.p.flip_d; tp.flip_h = s.p.flip_h; tp.flip_w = s.p.flip_w;
        tp.fss = dss.as<float>(); tp.fslope = pslope;
    } else {
        if (!low || !skip || !tstride || (low_c != 16 && low_c != 32)) return FNN_E_INVALID;
        for (int i = 0; i < 3; ++i) if (tstride[i] < 1 || tstride[i] > 2 || dims[i] % tstride[i]) return FNN_E_INVALID;
        tp.tsd = tstride[0]; tp.tsh = tstride[1]; tp.tsw = tstride[2];
        tp.Dl = dims[0] / tp.tsd; tp.Hl = dims[1] / tp.tsh; tp.Wl = dims[2] / tp.tsw;
        const int taps = tp.tsd * tp.tsh * tp.tsw, ksteps = (low_c + 31) / 32;
        if (!make_src(slow, low, n, low_c, (size_t)tp.Dl * tp.Hl * tp.Wl, pgamma, pbeta, pslope, true)) return FNN_E_HIP;
        if (!make_src(sskip, skip, n, 16, vox, skip_gamma, skip_beta, skip_slope, true)) return FNN_E_HIP;
        std::vector<uint16_t> fw((size_t)taps * ksteps * 512, 0);
        tconv_pack_weights(pw, low_c, 16, 16, taps, ksteps, fw.data());
        std::vector<float> fb(16, 0.f);
        if (pbias) for (int i = 0; i < 16; ++i) fb[i] = pbias[i];
        if (!upload(dfw, fw.data(), fw.size() * 2) || !upload(dfb, fb.data(), 16 * 4)) return FNN_E_HIP;
        p.n_src = 2; p.chunks = 2;
        p.src[0] = sskip.d; p.src[1] = sskip.d;                       // src[0], the transposed conv's output, is virtual: never read
        tp.low = slow.d;
        tp.fw = dfw.as<f16>(); tp.fbias = dfb.as<float>();
        cin_real[1] = 16;
    }
    ConvChoice cc;
    if (!conv_choose(tp, ConvOverrides::from_env(), cc)) return FNN_E_UNSUPPORTED;
    const size_t slots = (size_t)cc.stats_slots;
    std::vector<uint16_t> wp(conv_packed_halves(cc, cop), 0);
    conv_pack_weights(p, cc, 16, cin_real, w, wp.data(), nullptr);
    std::vector<float> bp(cop, 0.f);
    if (bias) for (int i = 0; i < 16; ++i) bp[i] = bias[i];
    DevBuf dw, dbias;
    if (!dw.alloc(fnn_weight_alloc_bytes(wp.size())) || !upload(dbias, bp.data(), cop * 4) || !dst.alloc((size_t)n * slots * cop * 16)) return FNN_E_HIP;
    (void)hipMemcpy(dw.p, wp.data(), wp.size() * 2, hipMemcpyHostToDevice);
    (void)hipMemset(dst.p, 0, (size_t)n * slots * cop * 16);
    p.wpk = dw.as<f16>(); p.bias = dbias.as<float>(); p.out = dout.as<f16>(); p.stats_out = dst.as<double>();
    const int rc = launch_conv(tp, cc, 0);
    if (rc != 0) return rc == -1 ? FNN_E_UNSUPPORTED : FNN_E_HIP;
    if (hipDeviceSynchronize() != hipSuccess) return FNN_E_HIP;
    std::vector<uint16_t> ho((size_t)n * vox * cop);
    (void)hipMemcpy(ho.data(), dout.p, ho.size() * 2, hipMemcpyDeviceToHost);
    from_device_layout(ho, n, 16, cop, vox, false, y);
    if (stats_out) sum_stat_rows(dst, n, slots, 16, cop, stats_out);
    return 0;
}

int fnn_op_last_kernels(char *buf, int cap) {
    std::string all;
    for (const std::string &k : g_op_kernels) { all += k; all += '\n'; }
    if (buf && cap > 0) { strncpy(buf, all.c_str(), (size_t)cap - 1); buf[cap - 1] = 0; }
    return (int)all.size() + 1;
}

int fnn_op_quotient_check(int device, unsigned long long counts[3]) {
    if (!counts) return FNN_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return FNN_E_HIP;
    DevBuf d;
    if (!d.alloc(24)) return FNN_E_HIP;
    (void)hipMemset(d.p, 0, 24);
    if (launch_quotient_check(d.as<unsigned long long>(), 0) != 0) return FNN_E_HIP;
    if (hipDeviceSynchronize() != hipSuccess) return FNN_E_HIP;
    (void)hipMemcpy(counts, d.p, 24, hipMemcpyDeviceToHost);
    return 0;
}

}  // extern "C"

// ----------------------------------------------------------------------------
// fnn_clock_probe_*: the shader clock under load (include/fnn.h)
// ----------------------------------------------------------------------------
namespace {
__global__ void clock_probe_kernel(unsigned long long *out, const int *flag, unsigned long long max_ticks) {
    if (threadIdx.x) return;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    unsigned long long i = 0;
    for (;; ++i) {                                            // ~16 us per turn
        __builtin_amdgcn_s_sleep(127); __builtin_amdgcn_s_sleep(127); __builtin_amdgcn_s_sleep(127); __builtin_amdgcn_s_sleep(127);
        if (__builtin_amdgcn_s_memrealtime() - r0 >= max_ticks) break;
        if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) break;
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    out[0] = t1 - t0; out[1] = r1 - r0; out[2] = i;
}
struct ClockProbe {
    int device = 0;
    Stream st;
    DevBuf out;                                               // 4 x u64
    PinnedBuf flag;                                           // one int in mapped host memory
};
}  // namespace

int fnn_clock_probe_start(int device, double max_seconds, void **probe) {
    if (!probe || !(max_seconds > 0) || max_seconds > 60) return FNN_E_INVALID;
    *probe = nullptr;
    if (hipSetDevice(device) != hipSuccess) return FNN_E_HIP;
    std::unique_ptr<ClockProbe> c(new ClockProbe);
    c->device = device;
    int *dflag = nullptr;
    if (c->st.create() != hipSuccess || !c->out.alloc(32) || c->flag.reserve(sizeof(int), hipHostMallocMapped) != hipSuccess ||
        hipHostGetDevicePointer((void **)&dflag, c->flag.p, 0) != hipSuccess)
        return FNN_E_HIP;
    *c->flag.as<int>() = 0;
    (void)hipMemsetAsync(c->out.p, 0, 32, c->st);
    hipLaunchKernelGGL(clock_probe_kernel, dim3(1), dim3(64), 0, c->st, c->out.as<unsigned long long>(), dflag, (unsigned long long)(max_seconds * 1e8));
    if (hipGetLastError() != hipSuccess) return FNN_E_HIP;
    *probe = c.release();
    return FNN_OK;
}

int fnn_clock_probe_stop(void *probe, double *ghz, double *seconds) {
    std::unique_ptr<ClockProbe> c((ClockProbe *)probe);
    if (!c) return FNN_E_INVALID;
    (void)hipSetDevice(c->device);
    __atomic_store_n(c->flag.as<int>(), 1, __ATOMIC_RELEASE);
    unsigned long long h[4] = {0, 0, 0, 0};
    const bool ok = hipStreamSynchronize(c->st) == hipSuccess && hipMemcpy(h, c->out.p, 32, hipMemcpyDeviceToHost) == hipSuccess;
    c.reset();
    if (!ok || h[1] == 0) return FNN_E_HIP;
    if (ghz) *ghz = (double)h[0] / (double)h[1] * 0.1;        // s_memrealtime: 100 MHz
    if (seconds) *seconds = (double)h[1] * 1e-8;
    return FNN_OK;
}
