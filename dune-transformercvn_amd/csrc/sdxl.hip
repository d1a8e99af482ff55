// SDXL-style embedder engine (reference: transformercvn/network/layers/sdxl_net.py:7-42 = diffusers' VAE Encoder with
// block_out_channels [d,d,2d,2d,4d,4d,8d,8d,out], norm_num_groups 1, then Flatten + Linear(out,out); selected by
// networks/neutrino_full_sdxl_network.py:6-20 / train.py --sdxl).  PARITY UNPINNED: diffusers is not vendored, pinned or
// installed; the block definitions this schedule follows are restated and cited in oracle/sdxl_oracle.py.
//
// The network is held as a TAPE of two operator kinds over NHWC activation buffers in the caller's workspace:
//   CONV  out = conv(in; w, b, kernel, stride, top-left pad) [+ residual buffer]        (sdxl_kernels.hip, implicit GEMM)
//   GN    out = silu?(groupnorm_1group(in; gamma, beta, eps 1e-6))                        (two-phase reduction)
// forward walks the tape, backward walks it in reverse: every buffer has a gradient buffer, the first contribution
// writes it and later ones accumulate.  The mid-block attention runs over the H*W tokens of the final map; the plan requires
// that map to be 1x1 (as the reference's Flatten + Linear(out,out) does), where softmax == 1 and the block reduces to
// x + to_out(to_v(groupnorm(x))); to_q / to_k keep their slots and receive zero gradients.
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/tcvn_hip.h"
#include "densenet_plan.h"      // Slot
#include "sdxl_ops.h"
#include "tcvn_ops.h"           // scatter_pixels, pack_weights, unpack_wgrads

using namespace tcvn;

static_assert(SCONV_GENERIC == TCVN_SCONV_GENERIC && SCONV_C64 == TCVN_SCONV_C64 && SCONV_G == TCVN_SCONV_G && SCONV_S2 == TCVN_SCONV_S2 &&
              SCONV_IN == TCVN_SCONV_IN, "tcvn_sdxl_conv_kernels returns SConvKernel values under the C names");

namespace {
#ifdef TCVN_DEBUG_KNOBS
int g_backward_stop = -1;                   // tcvn_debug_sdxl_backward_stop: backward() processes the ops last .. stop only; -1 = all
int g_forward_stop = -1;                    // tcvn_debug_sdxl_forward_stop: forward() processes the ops 0 .. stop only; -1 = all
#endif
constexpr float kGnEps = 1e-6f;
enum { OP_CONV = 0, OP_GN = 1 };
struct SBuf { int H, W, C; };
// stats_gn (CONV): the GroupNorm (gn_id) whose statistics this convolution's output feeds, or -1;  stats_given (GN): the producing
// convolution delivers this GroupNorm's statistics, so it runs no statistics pass of its own
struct SOp { int kind, in, out, res, w, b, ks, stride, pad, act, conv_id, gn_id, final_f32, stats_gn, stats_given; };
struct Bump {
    long off = 0;
    long take(long bytes) { long o = off; off += round_up(bytes, 256); return o; }
};
struct SLayout {
    std::vector<long> act, grad;            // per buffer (act[0] = image); grad[0] unused
    std::vector<long> wk, wkt, gwk;         // per conv
    long stats, bstats, zero_begin, zero_end, slab, total;
};
// a descriptor table on the device; its rows hold workspace addresses, so it is rebuilt when the workspace moves
struct DevTable {
    char* d = nullptr; size_t cap = 0; const char* ws = nullptr; long total = 0; int n = 0;
    std::vector<char> host;                 // source of the asynchronous copy
    bool stale(const char* ws_, long total_) const { return ws != ws_ || total != total_; }
    template <typename D>
    int upload(const std::vector<D>& rows, const char* ws_, long total_, hipStream_t st) {
        const size_t bytes = rows.size() * sizeof(D);
        if (bytes > cap) { if (d) TCVN_CHECK(hipFree(d)); d = nullptr; cap = 0; TCVN_CHECK(hipMalloc(&d, bytes)); cap = bytes; }
        host.assign(reinterpret_cast<const char*>(rows.data()), reinterpret_cast<const char*>(rows.data()) + bytes);
        TCVN_CHECK(hipMemcpyAsync(d, host.data(), bytes, hipMemcpyHostToDevice, st));
        n = (int)rows.size(); ws = ws_; total = total_;
        return 0;
    }
};
}  // namespace

struct tcvn_sdxl {
    tcvn_sdxl_cfg cfg;
    int esz;
    std::vector<Slot> slots;
    std::vector<float*> data, grad;
    std::vector<SBuf> bufs;
    std::vector<SOp> ops;
    std::vector<std::pair<std::string, int>> taps;                 // tcvn_sdxl_tap: name -> buffer, recorded as the tape is built
    int n_conv = 0, n_gn = 0;
    bool bound = false;
    int last_n = 0;
    const int32_t* last_coords = nullptr; long last_nnz = 0;       // COO list of the last forward (conv_in weight gradient)
    DevTable pack, unpack;
#ifdef TCVN_DEBUG_KNOBS
    std::vector<long> dbg_goff;                                    // tcvn_debug_sdxl_goff: gradient region and written flag of every buffer
    std::vector<char> dbg_written;                                 // when the last backward returned
#endif

    explicit tcvn_sdxl(const tcvn_sdxl_cfg& c);
    ~tcvn_sdxl() { if (pack.d) (void)hipFree(pack.d); if (unpack.d) (void)hipFree(unpack.d); }
    // slots `p.weight`, `p.bias` (the bias slot follows the weight slot) -> the weight slot
    int wb(const std::string& p, long w_numel, long b_numel) {
        slots.push_back({p + ".weight", w_numel, TCVN_SLOT_PARAM});
        slots.push_back({p + ".bias", b_numel, TCVN_SLOT_PARAM});
        return (int)slots.size() - 2;
    }
    int new_buf(int H, int W, int C) { bufs.push_back({H, W, C}); return (int)bufs.size() - 1; }
    // the one op constructor of each kind; w >= 0: slots reserved earlier (registration order differs from execution order)
    int conv(const std::string& p, int in, int cout, int ks, int stride, int pad, int res, int w = -1);
    int gn(const std::string& p, int in, int act, int w = -1);
    int resnet(const std::string& p, int in, int cout);
    void layout(int n, bool bwd, SLayout& L) const;
    int Kp(const SOp& o) const { return (int)round_up((long)o.ks * o.ks * bufs[o.in].C, 32); }
    int Kpt(const SOp& o) const { return (int)round_up((long)o.ks * o.ks * bufs[o.out].C, 32); }
    SConv geom(const SOp& o, int n) const;
    SConv bwd_geom(const SOp& o, int n, char* ws, const SLayout& L, const int32_t* hits, long nnz) const;
    GnArgs gn_args(const SOp& o, int n, char* ws, const SLayout& L) const;
    SConvFwd fwd_call(const SOp& o, int n, char* ws, const SLayout& L, float* out, long out_ld) const;
    SConvDgrad dgrad_call(const SOp& o, const SConv& g, char* ws, const SLayout& L, const char* dO, char* dI, int accumulate) const;
    SConvWgrad wgrad_call(const SOp& o, const SConv& g, char* ws, const SLayout& L, const char* dO) const;
    int forward(int n, const int32_t* coords, const float* values, long nnz, int log_pixels, float noise_std, float* out, long out_ld,
                char* ws, long ws_bytes, int train, uint64_t seed, hipStream_t st);
    int backward(int n, const float* d_out, long d_out_ld, char* ws, long ws_bytes, hipStream_t st);
};

int tcvn_sdxl::conv(const std::string& p, int in, int cout, int ks, int stride, int pad, int res, int w) {
    SOp o{};
    o.kind = OP_CONV; o.in = in; o.res = res; o.ks = ks; o.stride = stride; o.pad = pad; o.conv_id = n_conv++; o.stats_gn = -1;
    o.w = w >= 0 ? w : wb(p, (long)cout * bufs[in].C * ks * ks, cout);
    o.b = o.w + 1;
    // taps beyond the map read zero: behind a stride-2 convolution (pad 0) that is the row and column of diffusers' F.pad(0,1,0,1)
    const int far = stride == 2 ? 1 : pad;
    o.out = new_buf((bufs[in].H + pad + far - ks) / stride + 1, (bufs[in].W + pad + far - ks) / stride + 1, cout);
    ops.push_back(o);
    return o.out;
}
int tcvn_sdxl::gn(const std::string& p, int in, int act, int w) {
    SOp o{};
    o.kind = OP_GN; o.in = in; o.res = -1; o.act = act; o.gn_id = n_gn++;
    o.w = w >= 0 ? w : wb(p, bufs[in].C, bufs[in].C);
    o.b = o.w + 1;
    o.out = new_buf(bufs[in].H, bufs[in].W, bufs[in].C);
    ops.push_back(o);
    return o.out;
}
// ResnetBlock2D: x + conv2(silu(gn2(conv1(silu(gn1(x)))))), x through a 1x1 conv_shortcut when the width changes.
// Slot order = module registration order: norm1, conv1, norm2, conv2, conv_shortcut.
int tcvn_sdxl::resnet(const std::string& p, int in, int cout) {
    const int a1 = gn(p + ".norm1", in, 1);
    const int h1 = conv(p + ".conv1", a1, cout, 3, 1, 1, -1);
    const int a2 = gn(p + ".norm2", h1, 1);
    if (bufs[in].C == cout) return conv(p + ".conv2", a2, cout, 3, 1, 1, in);
    // conv2 is registered before conv_shortcut but runs after it (the shortcut's output is its residual): reserve its slots first
    const int w2 = wb(p + ".conv2", (long)cout * cout * 9, cout);
    const int sc = conv(p + ".conv_shortcut", in, cout, 1, 1, 0, -1);
    return conv(p + ".conv2", a2, cout, 3, 1, 1, sc, w2);
}

tcvn_sdxl::tcvn_sdxl(const tcvn_sdxl_cfg& c) : cfg(c) {
    esz = cfg.mode == MODE_F32 ? 4 : 2;
    std::vector<int> chans;
    int d = cfg.init_ch;
    for (int b = 0; b < cfg.num_blocks; ++b) { for (int r = 0; r < cfg.repeat; ++r) chans.push_back(d); d *= 2; }
    chans.push_back(cfg.out_dim);
    const std::string e = "encoder";
    int h = new_buf(cfg.H, cfg.W, cfg.in_ch);                                     // buffer 0: the scattered pixel map
    taps.push_back({"img", h});
    h = conv(e + ".conv_in", h, chans[0], 3, 1, 1, -1);
    taps.push_back({"conv_in", h});
    for (size_t i = 0; i < chans.size(); ++i) {
        const std::string p = e + ".down_blocks." + std::to_string(i);
        for (int j = 0; j < 2; ++j) h = resnet(p + ".resnets." + std::to_string(j), h, chans[i]);
        taps.push_back({"block" + std::to_string(i), h});                         // in front of the block's down-sampler
        if (i + 1 != chans.size()) h = conv(p + ".downsamplers.0.conv", h, chans[i], 3, 2, 0, -1);      // F.pad(0,1,0,1) + 3x3 stride 2, padding 0
    }
    const int C = chans.back();
    // mid block.  Registration order in diffusers: attentions, then resnets; execution: resnet0, attention, resnet1.
    const std::string m = e + ".mid_block", at = m + ".attentions.0";
    const int s_gn = wb(at + ".group_norm", C, C);
    wb(at + ".to_q", (long)C * C, C);
    wb(at + ".to_k", (long)C * C, C);
    const int s_v = wb(at + ".to_v", (long)C * C, C), s_o = wb(at + ".to_out.0", (long)C * C, C);
    h = resnet(m + ".resnets.0", h, C);
    const int t = gn(at + ".group_norm", h, 0, s_gn);                             // one token: x + to_out(to_v(gn(x)))
    const int v = conv(at + ".to_v", t, C, 1, 1, 0, -1, s_v);
    h = conv(at + ".to_out.0", v, C, 1, 1, 0, h, s_o);
    h = resnet(m + ".resnets.1", h, C);
    taps.push_back({"mid", h});
    h = conv(e + ".conv_out", gn(e + ".conv_norm_out", h, 1), cfg.out_dim, 3, 1, 1, -1);
    h = conv("output_layer.1", h, cfg.out_dim, 1, 1, 0, -1);
    ops.back().final_f32 = 1;
    // a buffer read by exactly one GroupNorm and produced by a convolution gets its statistics from that convolution
    for (auto& q : ops) {
        if (q.kind != OP_GN) continue;
        int readers = 0;
        for (const auto& o : ops) readers += o.kind == OP_GN && o.in == q.in;
        for (auto& o : ops)
            if (o.kind == OP_CONV && o.out == q.in && !o.final_f32 && readers == 1) { o.stats_gn = q.gn_id; q.stats_given = 1; }
    }
    data.assign(slots.size(), nullptr);
    grad.assign(slots.size(), nullptr);
}

void tcvn_sdxl::layout(int n, bool bwd, SLayout& L) const {
    Bump b;
    L.act.assign(bufs.size(), -1); L.grad.assign(bufs.size(), -1);
    for (size_t i = 0; i + 1 < bufs.size(); ++i) L.act[i] = b.take((long)n * bufs[i].H * bufs[i].W * bufs[i].C * esz);
    L.wk.assign(n_conv, -1); L.wkt.assign(n_conv, -1); L.gwk.assign(n_conv, -1);
    for (const auto& o : ops)
        if (o.kind == OP_CONV) {
            L.wk[o.conv_id] = b.take((long)bufs[o.out].C * Kp(o) * esz);
            if (o.in != 0) L.wkt[o.conv_id] = b.take((long)bufs[o.in].C * Kpt(o) * esz);
        }
    L.zero_begin = b.off;
    L.stats = b.take((long)n_gn * n * 16);
    if (bwd) {
        L.bstats = b.take((long)n_gn * n * 16);
        for (const auto& o : ops)
            if (o.kind == OP_CONV) L.gwk[o.conv_id] = b.take((long)bufs[o.out].C * Kp(o) * 4);
    } else L.bstats = -1;
    L.zero_end = b.off;
    L.slab = bwd ? b.take(kSconvSlabBytes) : -1;
    if (bwd)
        for (size_t i = 1; i < bufs.size(); ++i) L.grad[i] = b.take((long)n * bufs[i].H * bufs[i].W * bufs[i].C * esz);
    L.total = b.off;
}

SConv tcvn_sdxl::geom(const SOp& o, int n) const {
    SConv g{};
    g.mode = cfg.mode; g.n = n; g.Hin = bufs[o.in].H; g.Win = bufs[o.in].W; g.Cin = bufs[o.in].C; g.lda = g.Cin;
    g.Ho = bufs[o.out].H; g.Wo = bufs[o.out].W; g.Cout = bufs[o.out].C; g.ks = o.ks; g.stride = o.stride; g.pad = o.pad;
    g.Kp = Kp(o); g.Kpt = Kpt(o);
    return g;
}
// backward geometry: plus the weight-gradient slab and, for conv_in, the hit list of the forward
SConv tcvn_sdxl::bwd_geom(const SOp& o, int n, char* ws, const SLayout& L, const int32_t* hits, long nnz) const {
    SConv g = geom(o, n);
    g.slab = reinterpret_cast<float*>(ws + L.slab); g.slab_bytes = kSconvSlabBytes;
    if (o.in == 0) { g.hits = hits; g.nnz = nnz; }
    return g;
}
GnArgs tcvn_sdxl::gn_args(const SOp& o, int n, char* ws, const SLayout& L) const {
    return GnArgs{cfg.mode, ws + L.act[o.in], bufs[o.in].C, n, bufs[o.in].H * bufs[o.in].W, bufs[o.in].C, data[o.w], data[o.b], kGnEps, o.act,
                  reinterpret_cast<double*>(ws + L.stats) + (long)o.gn_id * n * 2};
}
// the last convolution writes the caller's fp32 output, every other one its activation buffer
SConvFwd tcvn_sdxl::fwd_call(const SOp& o, int n, char* ws, const SLayout& L, float* out, long out_ld) const {
    SConvFwd c{};
    c.g = geom(o, n);
    if (o.stats_gn >= 0) c.g.stats = reinterpret_cast<double*>(ws + L.stats) + (long)o.stats_gn * n * 2;
    c.In = ws + L.act[o.in]; c.Wk = ws + L.wk[o.conv_id]; c.bias = data[o.b];
    if (o.res >= 0) { c.Res = ws + L.act[o.res]; c.ldres = bufs[o.res].C; }
    c.Out = o.final_f32 ? reinterpret_cast<void*>(out) : reinterpret_cast<void*>(ws + L.act[o.out]);
    c.ldo = o.final_f32 ? out_ld : c.g.Cout;
    c.out_f32 = o.final_f32;
    return c;
}
SConvDgrad tcvn_sdxl::dgrad_call(const SOp& o, const SConv& g, char* ws, const SLayout& L, const char* dO, char* dI, int accumulate) const {
    return SConvDgrad{g, dO, g.Cout, ws + L.wkt[o.conv_id], dI, g.Cin, accumulate};
}
SConvWgrad tcvn_sdxl::wgrad_call(const SOp& o, const SConv& g, char* ws, const SLayout& L, const char* dO) const {
    return SConvWgrad{g, ws + L.act[o.in], dO, g.Cout, reinterpret_cast<float*>(ws + L.gwk[o.conv_id]), grad[o.b]};
}

int tcvn_sdxl::forward(int n, const int32_t* coords, const float* values, long nnz, int log_pixels, float noise_std, float* out,
                       long out_ld, char* ws, long ws_bytes, int train, uint64_t seed, hipStream_t st) {
    if (!bound) return -11;
    if (n <= 0) return 0;
    const SBuf& last = bufs.back();
    if (last.H != 1 || last.W != 1) {
        fprintf(stderr, "tcvn: SDXL embedder needs a 1x1 final map (Flatten + Linear(out,out)); %dx%d maps end at %dx%d\n", cfg.H, cfg.W, last.H, last.W);
        return -22;
    }
    SLayout L;
    layout(n, train != 0, L);
    if (ws_bytes < L.total) { fprintf(stderr, "tcvn: sdxl workspace too small (%ld < %ld)\n", ws_bytes, L.total); return -12; }
    int rc;
    if (pack.stale(ws, L.total)) {                                      // weight packing descriptors depend on the workspace address
        std::vector<PackDesc> pd;
        for (const auto& o : ops)
            if (o.kind == OP_CONV) {
                const int cin = bufs[o.in].C, cout = bufs[o.out].C;
                pd.push_back(PackDesc{data[o.w], ws + L.wk[o.conv_id], cout, cin, o.ks * o.ks, Kp(o), 0, 0});
                if (o.in != 0) pd.push_back(PackDesc{data[o.w], ws + L.wkt[o.conv_id], cout, cin, o.ks * o.ks, Kpt(o), 1, 0});
            }
        if ((rc = pack.upload(pd, ws, L.total, st))) return rc;
    }
    if ((rc = pack_weights(reinterpret_cast<const PackDesc*>(pack.d), pack.n, cfg.mode, st))) return rc;
    TCVN_CHECK(hipMemsetAsync(ws + L.act[0], 0, (size_t)n * cfg.H * cfg.W * cfg.in_ch * esz, st));
    TCVN_CHECK(hipMemsetAsync(ws + L.stats, 0, (size_t)n_gn * n * 16, st));
    {
        ScatterArgs a{cfg.mode, coords, values, nnz, n, ws + L.act[0], cfg.H, cfg.W, cfg.in_ch, log_pixels, train ? noise_std : 0.f, seed};
        if ((rc = scatter_pixels(a, st))) return rc;
    }
    for (const auto& o : ops) {
#ifdef TCVN_DEBUG_KNOBS
        if (g_forward_stop >= 0 && &o - ops.data() > g_forward_stop) break;
#endif
        if (o.kind == OP_GN) {
            const GnArgs a = gn_args(o, n, ws, L);
            if (!o.stats_given && (rc = gn_stats(a, st))) return rc;
            if ((rc = gn_act(a, ws + L.act[o.out], bufs[o.out].C, st))) return rc;
        } else if ((rc = sconv_fwd(fwd_call(o, n, ws, L, out, out_ld), st))) return rc;
    }
    last_n = n; last_coords = coords; last_nnz = nnz;
    return 0;
}

int tcvn_sdxl::backward(int n, const float* d_out, long d_out_ld, char* ws, long ws_bytes, hipStream_t st) {
    if (!bound) return -11;
    if (n <= 0) return 0;
    if (n != last_n) { fprintf(stderr, "tcvn: sdxl backward without matching forward\n"); return -13; }
    for (size_t i = 0; i < slots.size(); ++i)
        if (grad[i] == nullptr) { fprintf(stderr, "tcvn: grad of %s unbound\n", slots[i].name.c_str()); return -14; }
    SLayout L;
    layout(n, true, L);
    if (ws_bytes < L.total) return -12;
    int rc;
    if (unpack.stale(ws, L.total)) {
        std::vector<UnpackDesc> ud;
        for (const auto& o : ops)
            if (o.kind == OP_CONV)
                ud.push_back(UnpackDesc{reinterpret_cast<const float*>(ws + L.gwk[o.conv_id]), grad[o.w], bufs[o.out].C, bufs[o.in].C,
                                        o.ks * o.ks, Kp(o), 0});
        if ((rc = unpack.upload(ud, ws, L.total, st))) return rc;
    }
    // zero: backward GroupNorm sums and the kernel-layout weight gradients (forward statistics sit in front of them and stay)
    TCVN_CHECK(hipMemsetAsync(ws + L.bstats, 0, (size_t)(L.zero_end - L.bstats), st));
    std::vector<char> written(bufs.size(), 0);
    // gradient region of every buffer for THIS call: a residual input that has no contribution yet simply TAKES OVER the region of the output
    // gradient (same shape; dead once its producer has been processed) instead of receiving a copy of it (round 5: ten device-to-device copies of
    // up to 2 GB, 3.1 ms per step)
    std::vector<long> goff(L.grad.begin(), L.grad.end());
    const int last = (int)bufs.size() - 1;
    // the last buffer is the caller's fp32 output; its gradient arrives as fp32 too
    if ((rc = cast_f32_to(cfg.mode, d_out, d_out_ld, ws + goff[last], bufs[last].C, n, bufs[last].C, st))) return rc;
    written[last] = 1;
    for (int oi = (int)ops.size() - 1; oi >= 0; --oi) {
#ifdef TCVN_DEBUG_KNOBS
        if (g_backward_stop >= 0 && oi < g_backward_stop) break;
#endif
        const SOp& o = ops[oi];
        if (!written[o.out]) { fprintf(stderr, "tcvn: sdxl backward: gradient of buffer %d never produced\n", o.out); return -15; }
        const char* dO = ws + goff[o.out];
        if (o.kind == OP_GN) {
            const GnArgs a = gn_args(o, n, ws, L);
            double* bs = reinterpret_cast<double*>(ws + L.bstats) + (long)o.gn_id * n * 2;
            if ((rc = gn_bwd_reduce(a, dO, bufs[o.out].C, bs, grad[o.w], grad[o.b], st))) return rc;
            if ((rc = gn_bwd_apply(a, dO, bufs[o.out].C, bs, ws + goff[o.in], bufs[o.in].C, written[o.in], st))) return rc;
            written[o.in] = 1;
        } else {
            const SConv g = bwd_geom(o, n, ws, L, last_coords, last_nnz);
            if ((rc = sconv_wgrad(wgrad_call(o, g, ws, L, dO), st))) return rc;
            if (o.in != 0) {
                if ((rc = sconv_dgrad(dgrad_call(o, g, ws, L, dO, ws + goff[o.in], written[o.in]), st))) return rc;
                written[o.in] = 1;
            }
            if (o.res >= 0) {                                            // out = conv(...) + res: the residual receives dOut as is
                const long rows = (long)n * bufs[o.res].H * bufs[o.res].W;
                if (written[o.res]) { if ((rc = add_into(cfg.mode, ws + goff[o.res], bufs[o.res].C, dO, g.Cout, rows, g.Cout, st))) return rc; }
                else if (bufs[o.res].C == g.Cout && rows == (long)n * bufs[o.out].H * bufs[o.out].W) std::swap(goff[o.res], goff[o.out]);      // stream order: this op's kernels read dO first
                else TCVN_CHECK(hipMemcpyAsync(ws + goff[o.res], dO, (size_t)rows * g.Cout * esz, hipMemcpyDeviceToDevice, st));
                written[o.res] = 1;
            }
        }
    }
#ifdef TCVN_DEBUG_KNOBS
    dbg_goff = goff; dbg_written = written;
#endif
    return unpack_wgrads(reinterpret_cast<const UnpackDesc*>(unpack.d), unpack.n, st);
}

// ---------------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------------
extern "C" {

int tcvn_sdxl_create(const tcvn_sdxl_cfg* cfg, tcvn_sdxl** out) {
    if (!cfg || !out || cfg->num_blocks < 1 || cfg->num_blocks > 6 || cfg->repeat < 1 || cfg->repeat > 4 || cfg->init_ch < 1) return -1;
    if (cfg->mode != TCVN_MODE_F32 && cfg->mode != TCVN_MODE_BF16) return -1;
    *out = new tcvn_sdxl(*cfg);
    return 0;
}
void tcvn_sdxl_destroy(tcvn_sdxl* p) { delete p; }
int tcvn_sdxl_num_slots(const tcvn_sdxl* p) { return (int)p->slots.size(); }
int tcvn_sdxl_slot(const tcvn_sdxl* p, int i, char* name, int cap, int64_t* numel, int* kind) {
    if (i < 0 || i >= (int)p->slots.size()) return -1;
    const auto& s = p->slots[i];
    if (name && cap > 0) { strncpy(name, s.name.c_str(), cap - 1); name[cap - 1] = 0; }
    if (numel) *numel = s.numel;
    if (kind) *kind = s.kind;
    return 0;
}
int tcvn_sdxl_bind(tcvn_sdxl* p, void* const* d, void* const* g) {
    for (size_t i = 0; i < p->slots.size(); ++i) {
        p->data[i] = reinterpret_cast<float*>(d[i]);
        p->grad[i] = g ? reinterpret_cast<float*>(g[i]) : nullptr;
        if (p->data[i] == nullptr) { fprintf(stderr, "tcvn: slot %s unbound\n", p->slots[i].name.c_str()); return -10; }
    }
    p->bound = true; p->pack.ws = nullptr; p->unpack.ws = nullptr;
    return 0;
}
int64_t tcvn_sdxl_workspace_bytes(const tcvn_sdxl* p, int n_img, int with_backward) {
    SLayout L;
    p->layout(n_img, with_backward != 0, L);
    return L.total;
}
int tcvn_sdxl_forward(tcvn_sdxl* p, int n_img, const int32_t* coords, const float* values, int64_t nnz, int log_pixels, float noise_std,
                      float* out, int64_t out_ld, void* ws, int64_t ws_bytes, int train, uint64_t seed, void* stream) {
    return p->forward(n_img, coords, values, nnz, log_pixels, noise_std, out, out_ld, reinterpret_cast<char*>(ws), ws_bytes, train, seed,
                      reinterpret_cast<hipStream_t>(stream));
}
int tcvn_sdxl_backward(tcvn_sdxl* p, int n_img, const float* d_out, int64_t d_out_ld, void* ws, int64_t ws_bytes, void* stream) {
    return p->backward(n_img, d_out, d_out_ld, reinterpret_cast<char*>(ws), ws_bytes, reinterpret_cast<hipStream_t>(stream));
}
/* tap: "img", "conv_in", "block<i>" (output of down block i before its downsampler), "mid" -> byte offset + NHWC shape */
int tcvn_sdxl_tap(const tcvn_sdxl* p, int n_img, const char* name, int64_t* byte_off, int* n, int* h, int* w, int* c, int* ld,
                  int* elem_bytes) {
    for (const auto& t : p->taps)
        if (t.first == name) {
            SLayout L;
            p->layout(n_img, false, L);
            const SBuf& b = p->bufs[t.second];
            *byte_off = L.act[t.second]; *n = n_img; *h = b.H; *w = b.W; *c = b.C; *ld = b.C; *elem_bytes = p->esz;
            return 0;
        }
    return -1;
}
int tcvn_sdxl_num_convs(const tcvn_sdxl* p) { return p->n_conv; }
/* The choosers' answers for one convolution of a training step.  Operand addresses enter the choice through their alignment only, so
 * any 256-byte aligned workspace base stands for the caller's; no HIP call is made. */
int tcvn_sdxl_conv_kernels(const tcvn_sdxl* p, int n_img, int conv_index, int* fwd, int* dgrad, int* wgrad) {
    if (conv_index < 0 || conv_index >= p->n_conv || n_img <= 0) return -1;
    const SOp* o = nullptr;
    for (const auto& q : p->ops)
        if (q.kind == OP_CONV && q.conv_id == conv_index) o = &q;
    SLayout L;
    p->layout(n_img, true, L);
    char* ws = reinterpret_cast<char*>(uintptr_t(1) << 20);
    static const int32_t some_hit[3] = {0, 0, 0};
    const SConv g = p->bwd_geom(*o, n_img, ws, L, some_hit, 1);
    *fwd = sconv_fwd_kernel(p->fwd_call(*o, n_img, ws, L, reinterpret_cast<float*>(ws), g.Cout));
    *dgrad = o->in == 0 ? -1 : sconv_dgrad_kernel(p->dgrad_call(*o, g, ws, L, ws + L.grad[o->out], ws + L.grad[o->in], 0));
    *wgrad = sconv_wgrad_kernel(p->wgrad_call(*o, g, ws, L, ws + L.grad[o->out]));
    return 0;
}
int tcvn_sdxl_num_ops(const tcvn_sdxl* p) { return (int)p->ops.size(); }
/* One op of the tape, in execution order.  Fields that do not apply to the op's kind are -1 (res without a residual; ks, stride, pad,
 * conv_id, stats_gn and final_f32 of a GroupNorm; act, gn_id and stats_given of a convolution). */
int tcvn_sdxl_op(const tcvn_sdxl* p, int i, int* fields, int n_fields) {
    if (i < 0 || i >= (int)p->ops.size() || !fields || n_fields < TCVN_SDXL_OP_FIELDS) return -1;
    const SOp& o = p->ops[i];
    const bool cv = o.kind == OP_CONV;
    fields[TCVN_SDXL_OP_KIND] = o.kind; fields[TCVN_SDXL_OP_IN] = o.in; fields[TCVN_SDXL_OP_OUT] = o.out; fields[TCVN_SDXL_OP_RES] = o.res;
    fields[TCVN_SDXL_OP_W] = o.w;
    fields[TCVN_SDXL_OP_KS] = cv ? o.ks : -1; fields[TCVN_SDXL_OP_STRIDE] = cv ? o.stride : -1; fields[TCVN_SDXL_OP_PAD] = cv ? o.pad : -1;
    fields[TCVN_SDXL_OP_ACT] = cv ? -1 : o.act;
    fields[TCVN_SDXL_OP_CONV_ID] = cv ? o.conv_id : -1; fields[TCVN_SDXL_OP_GN_ID] = cv ? -1 : o.gn_id;
    fields[TCVN_SDXL_OP_STATS_GN] = cv ? o.stats_gn : -1; fields[TCVN_SDXL_OP_STATS_GIVEN] = cv ? -1 : o.stats_given;
    fields[TCVN_SDXL_OP_FINAL_F32] = cv ? o.final_f32 : -1;
    return 0;
}
/* Where a piece of the engine's state lies in a workspace of n_img maps: byte offset, shape (ndim <= 4 extents, row-major, dense) and
 * element size.  -1: no such region in this layout (the last buffer is the caller's output; conv_in has no transposed pack; gradients,
 * gwk and bstats exist only with_backward).  No HIP call. */
int tcvn_sdxl_region(const tcvn_sdxl* p, int n_img, int with_backward, int what, int index, int64_t* byte_off, int64_t* shape, int* ndim,
                     int* elem_bytes) {
    if (n_img <= 0 || !byte_off || !shape || !ndim || !elem_bytes) return -1;
    SLayout L;
    p->layout(n_img, with_backward != 0, L);
    long off = -1;
    auto set = [&](long o, int es, int nd, long a, long b, long c, long d) {
        off = o; *elem_bytes = es; *ndim = nd; shape[0] = a; shape[1] = b; shape[2] = c; shape[3] = d;
    };
    const SOp* cv = nullptr;
    if (what == TCVN_SDXL_REGION_WK || what == TCVN_SDXL_REGION_WKT || what == TCVN_SDXL_REGION_GWK) {
        for (const auto& q : p->ops)
            if (q.kind == OP_CONV && q.conv_id == index) cv = &q;
        if (!cv) return -1;
    }
    switch (what) {
    case TCVN_SDXL_REGION_ACT: case TCVN_SDXL_REGION_GRAD: {
        if (index < 0 || index >= (int)p->bufs.size()) return -1;
        const SBuf& b = p->bufs[index];
        set(what == TCVN_SDXL_REGION_ACT ? L.act[index] : L.grad[index], p->esz, 4, n_img, b.H, b.W, b.C);
        break;
    }
    case TCVN_SDXL_REGION_WK: set(L.wk[index], p->esz, 2, p->bufs[cv->out].C, p->Kp(*cv), 1, 1); break;
    case TCVN_SDXL_REGION_WKT: set(L.wkt[index], p->esz, 2, p->bufs[cv->in].C, p->Kpt(*cv), 1, 1); break;
    case TCVN_SDXL_REGION_GWK: set(L.gwk[index], 4, 2, p->bufs[cv->out].C, p->Kp(*cv), 1, 1); break;
    case TCVN_SDXL_REGION_STATS: set(L.stats, 8, 3, p->n_gn, n_img, 2, 1); break;
    case TCVN_SDXL_REGION_BSTATS: set(L.bstats, 8, 3, p->n_gn, n_img, 2, 1); break;
    default: return -1;
    }
    if (off < 0) return -1;
    *byte_off = off;
    return 0;
}

}  // extern "C"

#ifdef TCVN_DEBUG_KNOBS
// Validation build only.  A process-wide stop point for tcvn_sdxl_backward: it processes the ops last .. op of the tape (op = number of ops:
// only the cast of d_out), runs the weight-gradient unpack and returns; -1 switches it off.
extern "C" void tcvn_debug_sdxl_backward_stop(int op) { g_backward_stop = op; }
// The same for tcvn_sdxl_forward: it scatters the pixels and processes the ops 0 .. op of the tape, so that a test can see what one op wrote
// outside its own buffer before a later op overwrites it; -1 switches it off.
extern "C" void tcvn_debug_sdxl_forward_stop(int op) { g_forward_stop = op; }
// Where buffer `buf`'s gradient lay (byte offset in the workspace; a residual input may have taken over its output's region) and whether it had
// been written when the last tcvn_sdxl_backward of this plan returned.
extern "C" int tcvn_debug_sdxl_goff(const tcvn_sdxl* p, int buf, int64_t* off, int* written) {
    if (buf < 0 || buf >= (int)p->dbg_goff.size()) return -1;
    *off = p->dbg_goff[buf]; *written = p->dbg_written[buf];
    return 0;
}
#endif
