// DenseNet embedder engine: owns the layer schedule of layers/dense_net.py:97-167 (reference) and drives the gfx950
// kernels on one stream.  Data layout in HBM (per call, inside the caller's workspace):
//   img    [n,H,W,in_ch]                dense pixel map, NHWC
//   c0     [n,H/2,W/2,init]             conv0 output (pre-BN)
//   D[b]   [n,Hb,Wb,ld_b]               concat buffer of dense block b; layer l writes channels [C0_b+l*g, +g) in place
//   Y[b,l] [n,Hb,Wb,bn_size*g]          bottleneck (1x1 conv) output, kept for backward
//   bstat  (mean, biased var) per produced channel, fp64; BN (scale, shift) tables per BatchNorm layer, fp32
// Activations are fp32 (TCVN_MODE_F32) or bf16 (TCVN_MODE_BF16); statistics and tables are always fp64/fp32.
#include <string>
#include <vector>
#include <cstring>

#include "tcvn_rows.h"
#include <cstdlib>
#include "densenet_plan.h"

using namespace tcvn;

namespace {
constexpr float kEps = 1e-5f, kMom = 0.1f;
}

// ---------------------------------------------------------------------------------------------------------------------
// plan construction
// ---------------------------------------------------------------------------------------------------------------------
int DenseNetPlan::add_slot(const std::string& name, long numel, int kind) {
    slots.push_back({name, numel, kind});
    return (int)slots.size() - 1;
}
BnSlots DenseNetPlan::add_bn(const std::string& p, int c) {
    BnSlots s;
    s.w = add_slot(p + ".weight", c, TCVN_SLOT_PARAM);
    s.b = add_slot(p + ".bias", c, TCVN_SLOT_PARAM);
    s.rm = add_slot(p + ".running_mean", c, TCVN_SLOT_BUFFER);
    s.rv = add_slot(p + ".running_var", c, TCVN_SLOT_BUFFER);
    s.nbt = add_slot(p + ".num_batches_tracked", 1, TCVN_SLOT_COUNTER);
    s.C = c;
    s.id = n_bn++;
    return s;
}

DenseNetPlan::DenseNetPlan(const tcvn_densenet_cfg& c) : cfg(c) {
    esz = cfg.mode == MODE_F32 ? 4 : 2;
    const int g = cfg.growth, mid = cfg.bn_size * cfg.growth;
    Hc = (cfg.H + 6 - 7) / 2 + 1; Wc = (cfg.W + 6 - 7) / 2 + 1;
    int h = (Hc - 3) / 2 + 1, w = (Wc - 3) / 2 + 1;
    int ch = cfg.init_ch;
    const std::string f = "features";
    s_w0 = add_slot(f + ".conv0.weight", (long)ch * cfg.in_ch * 49, TCVN_SLOT_PARAM);
    s_b0 = add_slot(f + ".conv0.bias", ch, TCVN_SLOT_PARAM);
    n0 = add_bn(f + ".norm0", ch);
    s_a0 = add_slot(f + ".relu0.weight", ch, TCVN_SLOT_PARAM);
    for (int b = 0; b < cfg.n_blocks; ++b) {
        BlockGeom bg;
        bg.H = h; bg.W = w; bg.C0 = ch; bg.L = cfg.layers[b]; bg.Ctot = ch + bg.L * g; bg.ldp = (int)round_up(bg.Ctot, 8);
        // bf16 rows start on 128-B lines: the kernels read and write channel PREFIXES of these rows (1x1 input, its gradient's
        // read-modify-write); with a 320-B pitch (160 channels) every second prefix straddles one line more than it has to
        bg.ld = cfg.mode == MODE_BF16 ? (int)round_up(bg.Ctot, 64) : bg.ldp;
        for (int l = 0; l < bg.L; ++l) {
            LayerSlots ls;
            const int cin = ch + l * g;
            const std::string p = f + ".dense" + std::to_string(b + 1) + ".layers." + std::to_string(l);
            ls.n1 = add_bn(p + ".bottleneck_block.norm1", cin);
            ls.a1 = add_slot(p + ".bottleneck_block.relu1.weight", cin, TCVN_SLOT_PARAM);
            ls.w1 = add_slot(p + ".bottleneck_block.conv1.weight", (long)mid * cin, TCVN_SLOT_PARAM);
            ls.b1 = add_slot(p + ".bottleneck_block.conv1.bias", mid, TCVN_SLOT_PARAM);
            ls.n2 = add_bn(p + ".output_block.norm2", mid);
            ls.a2 = add_slot(p + ".output_block.relu2.weight", mid, TCVN_SLOT_PARAM);
            ls.w2 = add_slot(p + ".output_block.conv2.weight", (long)g * mid * 9, TCVN_SLOT_PARAM);
            ls.b2 = add_slot(p + ".output_block.conv2.bias", g, TCVN_SLOT_PARAM);
            ls.cin = cin;
            bg.layers.push_back(ls);
        }
        ch = bg.Ctot;
        if (b != cfg.n_blocks - 1) {
            const std::string p = f + ".transition" + std::to_string(b + 1);
            bg.has_trans = true;
            bg.tn = add_bn(p + ".norm", ch);
            bg.ta = add_slot(p + ".relu.weight", ch, TCVN_SLOT_PARAM);
            bg.tw = add_slot(p + ".conv.weight", (long)(ch / 2) * ch, TCVN_SLOT_PARAM);
            bg.tb = add_slot(p + ".conv.bias", ch / 2, TCVN_SLOT_PARAM);
            ch = ch / 2; h = h / 2; w = w / 2;
        }
        blocks.push_back(bg);
    }
    Cf = ch;
    nf = add_bn(f + ".final_norm", ch);
    s_af = add_slot(f + ".final_relu.weight", ch, TCVN_SLOT_PARAM);
    s_wl = add_slot("output_block.linear.weight", (long)cfg.out_dim * ch, TCVN_SLOT_PARAM);
    nl = add_bn("output_block.norm", cfg.out_dim);
    s_al = add_slot("output_block.relu.weight", cfg.out_dim, TCVN_SLOT_PARAM);
    data.assign(slots.size(), nullptr);
    grad.assign(slots.size(), nullptr);
    for (const auto& bg : blocks) path.emplace_back(bg.L);
}

DenseNetPlan::~DenseNetPlan() {
    if (d_desc) (void)hipFree(d_desc);
    if (d_undesc) (void)hipFree(d_undesc);
    if (side_st) {
        (void)hipStreamSynchronize(side_st);
        (void)hipStreamDestroy(side_st);
        (void)hipEventDestroy(ev_fork_a); (void)hipEventDestroy(ev_fork_b); (void)hipEventDestroy(ev_done[0]);
        (void)hipEventDestroy(ev_done[1]); (void)hipEventDestroy(ev_drain);
    }
}
int DenseNetPlan::ensure_side() {
    if (side_st) return 0;
    TCVN_CHECK(hipStreamCreateWithFlags(&side_st, hipStreamNonBlocking));
    hipEvent_t* evs[5] = {&ev_fork_a, &ev_fork_b, &ev_done[0], &ev_done[1], &ev_drain};
    for (hipEvent_t* e : evs) TCVN_CHECK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// workspace layout
// ---------------------------------------------------------------------------------------------------------------------
namespace {
struct Bump {
    long off = 0;
    long take(long bytes) { long o = off; off += round_up(bytes, 256); return o; }
};
}  // namespace

void DenseNetPlan::layout(int n, bool bwd, Layout& L) const {
    Bump b;
    const int mid = cfg.bn_size * cfg.growth;
    L.img = b.take((long)n * cfg.H * cfg.W * cfg.in_ch * esz);
    L.own = b.take(pixel_owners_bytes((long)n * cfg.H * cfg.W));      // directly behind img: one memset clears the map and the record's bitmaps
    L.c0 = b.take((long)n * Hc * Wc * cfg.init_ch * esz);
    L.D.clear(); L.Y.clear(); L.bstatD.clear(); L.bstatY.clear(); L.YA.clear(); L.XA.clear(); L.XP.clear(); L.KM.clear();
    L.zeros = b.take(1024);
    // link-free statistics accumulators: contiguous with the zero page, so that ONE memset per forward clears both
    L.isumD.clear(); L.isumY.clear(); L.isum_bytes = 0;
    if (cfg.mode == MODE_BF16) {
        const long i0 = b.off;
        for (const auto& bg : blocks) {
            L.isumD.push_back(b.take((long)LF_REP * bg.ld * 16));             // LF_REP replicas of [ld][2]
            std::vector<long> ys;
            for (int l = 0; l < bg.L; ++l) ys.push_back(b.take((long)LF_REP * mid * 16));
            L.isumY.push_back(ys);
        }
        L.isum_bytes = b.off - i0;
    }
    L.sact = (cfg.mode == MODE_BF16 && cfg.init_ch == 64) ? b.take((long)n * Hc * stem_act_words(Wc) * 4) : -1;
    L.sidx = sparse_stem_possible() ? b.take(stem_sparse_index_bytes(n, cfg.H, cfg.W)) : -1;
    long max_part = (long)pool0_grid(n, blocks[0].H, blocks[0].W) * cfg.init_ch * 16;
    max_part = std::max(max_part, 1024L * cfg.init_ch * 16);      // sparse stem passes: <= 1024 workgroups
    max_part = std::max(max_part, 512L * cfg.init_ch * 16);
    long maxY = 0;
    for (const auto& bg : blocks) {
        const long M = (long)n * bg.H * bg.W;
        L.D.push_back(b.take(M * bg.ld * esz));
        std::vector<long> ys, bs;
        for (int l = 0; l < bg.L; ++l) { ys.push_back(b.take(M * mid * esz)); bs.push_back(b.take(mid * 16)); }
        L.Y.push_back(ys); L.bstatY.push_back(bs);
        std::vector<long> yas;
        if (cfg.mode == MODE_BF16)
            for (int l = 0; l < bg.L; ++l) yas.push_back(b.take(M * mid * esz));
        L.YA.push_back(yas);
        std::vector<long> kms;
        if (cfg.mode == MODE_BF16 && cfg.dropout > 0.f)
            for (int l = 0; l < bg.L; ++l) kms.push_back(b.take(M * 4));
        L.KM.push_back(kms);
        std::vector<long> xas;
        for (int l = 0; l < bg.L; ++l) {
            const int cin = bg.C0 + l * cfg.growth;
            xas.push_back(fast1_ok(cin) ? b.take(M * round_up(cin, 8) * esz) : -1);     // >= 0 marks the bf16 GEMM path
        }
        L.XA.push_back(xas);
        const bool tfast = bg.has_trans && fastt_ok(bg.Ctot);
        // fp32 mode (round 4): the same materialised operand feeds the generic forward / weight-gradient kernels of the transition
        const bool tmat32 = bg.has_trans && cfg.mode == MODE_F32 && conv3x3_tile_enabled() && (bg.ld & 3) == 0;
        L.XP.push_back((tfast || tmat32) ? b.take((long)n * (bg.H / 2) * (bg.W / 2) * bg.ldp * esz) : -1);   // row stride bg.ldp, zero padded
        L.bstatD.push_back(b.take((long)bg.ld * 16));
        max_part = std::max(max_part, 512L * std::max(mid, bg.Ctot) * 16);   // the conv launchers use <= 512 workgroups ...
        max_part = std::max(max_part, 768L * mid * 16);                      // ... but the fused 1x1 forward up to 768 (fwd1x1_fused_nblk: three per CU)
        maxY = std::max(maxY, M * mid);
    }
    L.bstat0 = b.take((long)cfg.init_ch * 16);
    L.part = b.take(max_part * 2);                     // x2: backward partials carry 3 doubles per channel
    L.tabs = b.take((long)tab_floats() * 4);
    L.F = b.take((long)n * Cf * 4);
    L.Z = b.take((long)n * cfg.out_dim * 4);
    L.head_stat = b.take((long)cfg.out_dim * 8);
    L.wk = b.take(wk_bytes());
    L.fwd_end = b.off;
    if (bwd) layout_bwd(n, b.off, maxY, L);
    else L.total = b.off;
}

long DenseNetPlan::tab_floats() const { return tab_off(nf) + 2 * round_up(nf.C, 8); }      // (scale, shift) per BN layer, channel count rounded to 8; final_norm is the last

// offsets (in floats) of the table of BN layer `s` inside the tabs region: sc at off, sh at off + round_up(C, 8)
long DenseNetPlan::tab_off(const BnSlots& s) const {
    long t = 0;
    bool found = false;
    auto add = [&](const BnSlots& q) {
        if (found) return;
        if (q.id == s.id) { found = true; return; }
        t += 2 * round_up(q.C, 8);
    };
    add(n0);
    for (const auto& bg : blocks) {
        for (const auto& ls : bg.layers) { add(ls.n1); add(ls.n2); }
        if (bg.has_trans) add(bg.tn);
    }
    add(nf);
    return t;
}

long DenseNetPlan::wk_bytes() const {
    long t = 0;
    for (const auto& w : wk_list()) t += round_up(round_up(w.rows, 32) * w.Kp * esz, 256);
    return t;
}

// bf16 GEMM paths for the 1x1 convolutions: operands are materialised with row strides rounded up to 8 channels (zero
// padded), so any channel count works as long as the K extent fits the NT kernel's register-resident weights (<= 640).
bool DenseNetPlan::fast1_ok(int cin) const {
    const int mid = cfg.bn_size * cfg.growth;
    return cfg.mode == MODE_BF16 && conv3x3_tile_enabled() && mid % 8 == 0 && mid <= 256 && round_up(cin, 32) <= 640;
}
bool DenseNetPlan::sparse_stem_possible() const {
    return cfg.mode == MODE_BF16 && cfg.in_ch >= 1 && cfg.in_ch <= 3 && cfg.init_ch == 64 && !blocks.empty() && (blocks[0].ld & 7) == 0;
}
bool DenseNetPlan::fastt_ok(int Ctot) const {
    return cfg.mode == MODE_BF16 && conv3x3_tile_enabled() && round_up(Ctot, 32) <= 640 && Ctot / 2 <= 512;
}

// every conv weight in kernel layout; the order defines the offsets in the wk region
std::vector<WkEntry> DenseNetPlan::wk_list() const {
    std::vector<WkEntry> v;
    const int mid = cfg.bn_size * cfg.growth, g = cfg.growth;
    long off = 0;
    auto add = [&](int slot, int N, int Cin, int taps, int transpose, int frag = 0) {
        WkEntry e;
        e.slot = slot; e.N = N; e.Cin = Cin; e.taps = taps; e.transpose = transpose; e.frag = frag;
        e.rows = transpose ? Cin : N;
        e.Kp = (int)round_up((long)taps * (transpose ? N : Cin), 32);
        e.off = off;
        off += round_up(round_up(e.rows, 32) * e.Kp * esz, 256);
        v.push_back(e);
    };
    const bool frag = cfg.mode == MODE_BF16;      // bf16 fast paths read weights in MFMA fragment order
    add(s_w0, cfg.init_ch, cfg.in_ch, 49, 0);
    for (const auto& bg : blocks) {
        for (const auto& ls : bg.layers) {
            add(ls.w1, mid, ls.cin, 1, 0);
            add(ls.w2, g, mid, 9, 0);
            add(ls.w1, mid, ls.cin, 1, 1);     // dgrad layouts
            add(ls.w2, g, mid, 9, 1);
            if (frag) {
                add(ls.w2, g, mid, 9, 0, 1); add(ls.w2, g, mid, 9, 1, 1);
                add(ls.w1, mid, ls.cin, 1, 0, 1); add(ls.w1, mid, ls.cin, 1, 1, 1);
            }
        }
        if (bg.has_trans) {
            add(bg.tw, bg.Ctot / 2, bg.Ctot, 1, 0); add(bg.tw, bg.Ctot / 2, bg.Ctot, 1, 1);
            if (frag) { add(bg.tw, bg.Ctot / 2, bg.Ctot, 1, 0, 1); add(bg.tw, bg.Ctot / 2, bg.Ctot, 1, 1, 1); }
        }
    }
    return v;
}

const void* DenseNetPlan::wk_frag(const char* ws, const Layout& L, int slot, int transpose) const {
    for (const auto& e : wk_cache)
        if (e.slot == slot && e.transpose == transpose && e.frag == 1) return ws + L.wk + e.off;
    return nullptr;
}

const WkEntry& DenseNetPlan::wk_find(int slot, int transpose, int frag) const {
    for (const auto& e : wk_cache)
        if (e.slot == slot && e.transpose == transpose && e.frag == frag) return e;
    fprintf(stderr, "tcvn: wk_find miss\n");
    abort();
}

int DenseNetPlan::bind(void* const* d, void* const* g) {
    for (size_t i = 0; i < slots.size(); ++i) {
        data[i] = reinterpret_cast<float*>(d[i]);
        grad[i] = g ? reinterpret_cast<float*>(g[i]) : nullptr;
        if (slots[i].kind != TCVN_SLOT_COUNTER && data[i] == nullptr) {
            fprintf(stderr, "tcvn: slot %s unbound\n", slots[i].name.c_str());
            return -10;
        }
    }
    wk_cache = wk_list();
    fast3x3 = cfg.mode == MODE_BF16 && cfg.bn_size * cfg.growth == 128 && cfg.growth <= 32 && conv3x3_tile_enabled();
    bound = true;
    desc_ws = nullptr;   // device descriptor tables are rebuilt on the next forward
    undesc_ws = nullptr;
    last_ws = nullptr;   // ... and nothing packed from the old bindings is resumed from
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------------
int DenseNetPlan::upload_descs(char* ws, const Layout& L, hipStream_t st) {
    // Pack descriptors (weights -> kernel layout) and eval-mode BN descriptors live in a small device table that
    // depends on the workspace address; rebuilt only when the workspace base or the bindings change.
    if (desc_ws == ws && desc_total == L.total) return 0;
    std::vector<PackDesc> pd;
    for (const auto& e : wk_cache) {
        PackDesc d;
        d.src = data[e.slot]; d.dst = ws + L.wk + e.off; d.N = e.N; d.Cin = e.Cin; d.taps = e.taps; d.Kp = e.Kp;
        d.transpose = e.transpose; d.frag = e.frag;
        pd.push_back(d);
    }
    std::vector<BnEvalDesc> bd;
    auto addbn = [&](const BnSlots& s) {
        BnEvalDesc d;
        d.gamma = data[s.w]; d.beta = data[s.b]; d.rm = data[s.rm]; d.rv = data[s.rv];
        const Tab t = tab(ws, L, s);
        d.sc = t.sc; d.sh = t.sh; d.C = s.C;
        bd.push_back(d);
    };
    addbn(n0);
    for (const auto& bg : blocks) {
        for (const auto& ls : bg.layers) { addbn(ls.n1); addbn(ls.n2); }
        if (bg.has_trans) addbn(bg.tn);
    }
    addbn(nf);
    n_pack = (int)pd.size(); n_bneval = (int)bd.size();
    const size_t bytes = pd.size() * sizeof(PackDesc) + bd.size() * sizeof(BnEvalDesc);
    if (bytes > desc_cap) {
        if (d_desc) TCVN_CHECK(hipFree(d_desc));
        TCVN_CHECK(hipMalloc(&d_desc, bytes));
        desc_cap = bytes;
    }
    h_desc.resize(bytes);
    memcpy(h_desc.data(), pd.data(), pd.size() * sizeof(PackDesc));
    memcpy(h_desc.data() + pd.size() * sizeof(PackDesc), bd.data(), bd.size() * sizeof(BnEvalDesc));
    TCVN_CHECK(hipMemcpyAsync(d_desc, h_desc.data(), bytes, hipMemcpyHostToDevice, st));
    desc_ws = ws; desc_total = L.total;
    return 0;
}

Tab DenseNetPlan::tab(char* ws, const Layout& L, const BnSlots& bn) const {
    float* sc = reinterpret_cast<float*>(ws + L.tabs) + tab_off(bn);
    return Tab{sc, sc + round_up(bn.C, 8)};
}

ConvFwdArgs DenseNetPlan::conv0_args(const Step& s) const {
    const WkEntry& e = wk_find(s_w0, 0);
    ConvFwdArgs a{};
    a.mode = cfg.mode; a.amode = A_STEM; a.A = s.ws + s.L.img; a.lda = cfg.in_ch; a.M = s.n * Hc * Wc; a.N = cfg.init_ch;
    a.K = 49 * cfg.in_ch; a.Kp = e.Kp; a.C = cfg.in_ch; a.H = Hc; a.W = Wc; a.Hin = cfg.H; a.Win = cfg.W;
    a.Wk = s.ws + s.L.wk + e.off; a.bias = data[s_b0]; a.Out = s.ws + s.L.c0; a.ldo = cfg.init_ch; a.n_off = 0;
    return a;
}

ConvFwdArgs DenseNetPlan::conv1_args(const Step& s, int bi, int l) const {      // D[:, 0:cin] -> Y
    const BlockGeom& bg = blocks[bi];
    const LayerSlots& ls = bg.layers[l];
    const WkEntry& e = wk_find(ls.w1, 0);
    const Tab t = tab(s.ws, s.L, ls.n1);
    ConvFwdArgs a{};
    a.mode = cfg.mode; a.amode = A_1X1; a.A = s.ws + s.L.D[bi]; a.lda = bg.ld; a.M = s.n * bg.H * bg.W; a.N = cfg.bn_size * cfg.growth;
    a.K = ls.cin; a.Kp = e.Kp; a.C = ls.cin; a.H = bg.H; a.W = bg.W; a.sc = t.sc; a.sh = t.sh; a.sl = data[ls.a1];
    a.Wk = s.ws + s.L.wk + e.off; a.bias = data[ls.b1]; a.Out = s.ws + s.L.Y[bi][l]; a.ldo = a.N; a.n_off = 0;
    return a;
}

ConvFwdArgs DenseNetPlan::conv3_args(const Step& s, int bi, int l) const {      // Y -> D[:, cin:cin+g]
    const BlockGeom& bg = blocks[bi];
    const LayerSlots& ls = bg.layers[l];
    const WkEntry& e = wk_find(ls.w2, 0);
    const Tab t = tab(s.ws, s.L, ls.n2);
    const int mid = cfg.bn_size * cfg.growth;
    ConvFwdArgs a{};
    a.mode = cfg.mode; a.amode = A_3X3; a.A = s.ws + s.L.Y[bi][l]; a.lda = mid; a.M = s.n * bg.H * bg.W; a.N = cfg.growth; a.K = 9 * mid;
    a.Kp = e.Kp; a.C = mid; a.H = bg.H; a.W = bg.W; a.sc = t.sc; a.sh = t.sh; a.sl = data[ls.a2];
    a.Wk = s.ws + s.L.wk + e.off; a.bias = data[ls.b2]; a.Out = s.ws + s.L.D[bi]; a.ldo = bg.ld; a.n_off = ls.cin;
    a.Wfrag = wk_frag(s.ws, s.L, ls.w2, 0);
    if (cfg.mode == MODE_BF16) { a.zeros = s.ws + s.L.zeros; a.Aact = a.A; }
    return a;
}

ConvFwdArgs DenseNetPlan::trans_args(const Step& s, int bi) const {      // D[bi] -> first channels of D[bi + 1]
    const BlockGeom &bg = blocks[bi], &nb = blocks[bi + 1];
    const WkEntry& e = wk_find(bg.tw, 0);
    ConvFwdArgs a{};
    a.mode = cfg.mode; a.M = s.n * nb.H * nb.W; a.N = bg.Ctot / 2; a.Kp = e.Kp; a.H = nb.H; a.W = nb.W; a.Hin = bg.H; a.Win = bg.W;
    if (s.L.XP[bi] >= 0 && cfg.mode == MODE_F32) {      // the pooled + activated operand is materialised: a plain 1x1 convolution over it (K padded to ldp: zero columns x zero weights)
        a.amode = A_1X1; a.A = s.ws + s.L.XP[bi]; a.lda = bg.ldp; a.K = bg.ldp; a.C = bg.ldp;
    } else {
        const Tab t = tab(s.ws, s.L, bg.tn);
        a.amode = A_1X1_POOL; a.A = s.ws + s.L.D[bi]; a.lda = bg.ld; a.K = bg.Ctot; a.C = bg.Ctot; a.sc = t.sc; a.sh = t.sh; a.sl = data[bg.ta];
    }
    a.Wk = s.ws + s.L.wk + e.off; a.bias = data[bg.tb]; a.Out = s.ws + s.L.D[bi + 1]; a.ldo = nb.ld; a.n_off = 0;
    return a;
}

// index, weights, geometry and BatchNorm0 table of the sparse-aware stem; Out / part (forward) and e / P0 / Q0 / slab / dWk (backward) are the caller's
StemSparseArgs DenseNetPlan::stem_sparse_args(const Step& s, const int32_t* coords, const float* values, long nnz, int value_mode, float noise_std) const {
    const WkEntry& e = wk_find(s_w0, 0);
    const Tab t = tab(s.ws, s.L, n0);
    StemSparseArgs sa{};
    sa.coords = coords; sa.values = values; sa.nnz = nnz; sa.n_img = s.n; sa.H = cfg.H; sa.W = cfg.W; sa.Cpix = cfg.in_ch;
    sa.value_mode = value_mode; sa.noise_std = noise_std; sa.seed = s.seed;
    stem_sparse_carve(sa, s.ws + s.L.sidx);
    sa.Wk = s.ws + s.L.wk + e.off; sa.Kp = e.Kp; sa.bias = data[s_b0];
    sa.Hc = Hc; sa.Wc = Wc; sa.Ho = blocks[0].H; sa.Wo = blocks[0].W;
    sa.sc = t.sc; sa.sh = t.sh; sa.sl = data[s_a0];
    return sa;
}

int DenseNetPlan::link(const Step& s, const BnSlots& bn, int nblk, int part_ld, int c_new0, int n_new, double* bstat, long count,
                       const long long* isum, long isum_stride) const {
    if (!s.train) return 0;
    BnLinkArgs a{};
    a.isum = isum; a.isum_stride = isum_stride;                  // window sums in fixed-point accumulators (a link-free producer) instead of partial rows
    a.part = s.part; a.nblk = nblk; a.part_ld = part_ld; a.c_new0 = c_new0; a.n_new = n_new; a.bstat = bstat;
    a.count = count; a.C = bn.C; a.gamma = data[bn.w]; a.beta = data[bn.b];
    a.running_mean = data[bn.rm]; a.running_var = data[bn.rv];
    const Tab t = tab(s.ws, s.L, bn); a.sc = t.sc; a.sh = t.sh; a.train = 1; a.eps = kEps; a.momentum = kMom;
    return bn_link(a, s.st);
}

// the table of a BatchNorm over block bi's concat buffer by the link kernel (window sums from the partial rows or from the block's accumulators)
int DenseNetPlan::link_fresh(const Step& s, const BnSlots& bn, int bi, const FreshStats& fr) const {
    const BlockGeom& bg = blocks[bi];
    const long long* isum = fr.isum ? reinterpret_cast<const long long*>(s.ws + s.L.isumD[bi]) + 2 * fr.c0 : nullptr;      // [ld][2], indexed by channel
    return link(s, bn, fr.nblk, fr.ld, fr.c0, fr.n, reinterpret_cast<double*>(s.ws + s.L.bstatD[bi]), (long)s.n * bg.H * bg.W, isum, 2L * bg.ld);
}

LfLink DenseNetPlan::lf_link(const Step& s, const BnSlots& bn, const long long* isum, long rep_stride, int c_new0, int n_new, double* bstat, long count) const {
    LfLink k{};
    k.isum = isum; k.rep_stride = rep_stride; k.c_new0 = c_new0; k.n_new = n_new; k.bstat = bstat; k.inv_count = 1.0 / (double)count; k.count = count;
    k.gamma = data[bn.w]; k.beta = data[bn.b]; k.running_mean = data[bn.rm]; k.running_var = data[bn.rv];
    const Tab t = tab(s.ws, s.L, bn); k.sc_out = t.sc; k.sh_out = t.sh; k.eps = kEps; k.momentum = kMom;
    return k;
}

// draw (eval pass only): Monte-Carlo dropout, the dropout sites draw from `seed` and nothing else changes.  resume (with draw): the call
// starts at dense block 1, layer 0, on what the last eval-kind forward of the same inputs left in this workspace -- no dropout site lies
// in front of the first 3x3 convolution, and the eval layout gives the stem's channels of D[0], the packed weights (wk) and the BatchNorm
// tables (tabs) regions that no later launch of an eval pass writes (link() returns at once, lf_link needs lf_on).
int DenseNetPlan::forward(int n, const int32_t* coords, const float* values, long nnz, int log_pixels, float noise_std,
                          float* out, long out_ld, char* ws, long ws_bytes, int train, uint64_t seed, hipStream_t st, bool draw, bool resume,
                          bool frozen) {
    if (!bound) return -11;
    if (frozen && (train || draw || resume)) return -1;
    if (frozen && log_pixels == 3) { fprintf(stderr, "tcvn: densenet forward_frozen: one-hot pixels are class indices and have no gradient\n"); return -22; }
    if (n <= 0) return 0;
    Layout L;
    layout(n, train != 0 || frozen, L);
    if (ws_bytes < L.total) { fprintf(stderr, "tcvn: densenet workspace too small (%ld < %ld)\n", ws_bytes, L.total); return -12; }
    if (resume && !(last_ws == ws && last_eval && !last_frozen && last_n == n && last_coords == coords && last_nnz == nnz && last_values == values &&
                    last_value_mode == log_pixels)) {
        fprintf(stderr, "tcvn: densenet forward_mc cannot resume: the last call on this workspace was not an eval-mode forward of these inputs\n");
        return -18;
    }
    int rc;
    if (!resume) {
        last_ws = nullptr;       // until this call has come through
        last_frozen = false;
        if ((rc = upload_descs(ws, L, st))) return rc;
        // weights -> kernel layout (fp32 -> T); eval: all BN tables from the running statistics in one launch
        if ((rc = pack_weights(reinterpret_cast<const PackDesc*>(d_desc), n_pack, cfg.mode, st))) return rc;
        if (!train && (rc = bn_eval_tables(reinterpret_cast<const BnEvalDesc*>(d_desc + n_pack * sizeof(PackDesc)), n_bneval, kEps, st))) return rc;
    }
    // Round 5, link-free BatchNorm statistics (bn_lf.h): the fused 1x1 kernels and the 3x3 pair kernel ADD their per-workgroup sums to
    // fixed-point accumulators and derive their input BatchNorm's table in their own prologue -- no k_bn_link launch between them (120 of
    // the 132 per step and embedder).  TCVN_NO_LF (validation build): the link kernels of rounds 1-4.
    static const bool no_lf = TCVN_KNOB_SET("TCVN_NO_LF");
    const bool lf_on = train && !no_lf && cfg.mode == MODE_BF16 && L.isum_bytes > 0;
    TCVN_CHECK(hipMemsetAsync(ws + L.zeros, 0, 1024 + (lf_on ? L.isum_bytes : 0), st));
    const Step s{ws, L, st, n, train != 0, seed, reinterpret_cast<double*>(ws + L.part), lf_on, false, 0, false, draw && !train, frozen};
    FreshStats fr{};                  // statistics of the newest channels of the block being built (read by train-mode links only)
    if (!resume && (rc = fwd_stem(s, coords, values, nnz, log_pixels, noise_std, fr))) return rc;
    for (int bi = 0; bi < (int)blocks.size(); ++bi) {
        for (int l = 0; l < blocks[bi].L; ++l)
            if ((rc = fwd_layer(s, bi, l, fr))) return rc;
        if ((rc = fwd_transition(s, bi, fr))) return rc;
    }
    if ((rc = fwd_output(s, out, out_ld))) return rc;
    last_seed = seed; last_n = n; last_coords = coords; last_nnz = nnz; last_ws = ws; last_eval = !train; last_frozen = frozen;
    return 0;
}

// ---- stem: conv0 - BN0 - PReLU0 - AvgPool(3, 2) -> the first channels of block 1 ----
int DenseNetPlan::fwd_stem(const Step& s, const int32_t* coords, const float* values, long nnz, int log_pixels, float noise_std, FreshStats& fr) {
    const Layout& L = s.L;
    const BlockGeom& b0 = blocks[0];
    const int mode = cfg.mode, n = s.n;
    const long M0 = (long)n * Hc * Wc;
    const float noise = s.train ? noise_std : 0.f;
    double* bstat0 = reinterpret_cast<double*>(s.ws + L.bstat0);
    int rc;
    // Sparse-aware stem (bf16, 3 -> 64 channels, the hit list fits the index): conv0 + BN0 + PReLU0 + AvgPool straight from the COO
    // list, neither the dense map nor the conv0 output is materialised (stem_sparse.hip).  Otherwise: scatter + dense kernels.
    // Measured on MI355X (256 prong maps / 32 event maps, round 3): inference -- index + pooled pass 0.60 / 0.27 ms against 0.97 / 0.12 ms
    // for the dense conv0 + pooling kernels, so eval-mode forwards take the sparse stem.  Training -- the statistics pass adds 0.34 / 0.16 ms
    // (forward at parity with the dense kernels) and the sparse backward passes (0.87 + 4.3 ms) lose clearly to the dense backward
    // (0.40 + 0.50 ms: its weight gradient already walks the hit list), so train-mode steps keep the dense stem.  The validation build
    // can force either (TCVN_DENSE_STEM / TCVN_SPARSE_STEM_TRAIN) for the parity tests of all four sparse passes.
    static const bool dense_stem_knob = TCVN_KNOB_SET("TCVN_DENSE_STEM");
    static const bool sparse_train_knob = TCVN_KNOB_SET("TCVN_SPARSE_STEM_TRAIN");
    // Round 4: the maps are mostly empty, so most conv0 outputs are exactly bf16(bias) (a sum of zeros plus the bias).  stem_mark builds a bitmap
    // of the output positions some hit reaches (~16 % of a prong map's 28 000 at 20-800 hits); the pooling BACKWARD kernel reads one shared row for
    // every other position and does not store their gradient rows (only the hit-list weight gradient reads that tensor).  Bit-identical results.
    // Measured and NOT kept: the same bitmap in conv0 (stores skipped) and in the forward pooling kernel -- the forward pooling got slower
    // (prong embedder 271 -> 345 us: its nine loads per pixel turn into a mix of L2 hits and isolated 128-B HBM lines, which DRAM serves far
    // below its streaming rate), the backward gained 10 %, the step did not move (19.65-19.76 against 19.74-19.86 ms).
    static const bool no_stem_skip = TCVN_KNOB_SET("TCVN_NO_STEM_SKIP") || TCVN_KNOB_SET("TCVN_POOL0_BWD_FLAT");   // (the flat backward kernel reads every row)
    stem_path = StemPath{};
    // A frozen pass takes the dense stem: its backward needs the conv0 map behind the pooling backward (DU0), and the duplicate record.
    // The activity bitmap stays off with it (act_skip asks for train), so the pooling backward stores EVERY row of DU0 -- a hit gathers from
    // the <= 16 conv0 outputs whose window holds it, and all of them are stored rows whatever the other hits are.
    stem_path.sparse = !s.frozen && !dense_stem_knob && (!s.train || sparse_train_knob) && L.sidx >= 0 &&
                       stem_sparse_ok(mode, cfg.in_ch, cfg.init_ch, cfg.H, cfg.W, log_pixels, nnz, n, b0.ld);
    last_values = values; last_value_mode = log_pixels; last_noise = noise;
    fr = FreshStats{0, b0.C0, 0, cfg.init_ch, false};
    if (stem_path.sparse) {
        StemSparseArgs sa = stem_sparse_args(s, coords, values, nnz, log_pixels, noise);
        if ((rc = stem_sparse_index(sa, s.st))) return rc;
        if (s.train) {
            sa.part = s.part;
            if ((rc = stem_sparse_stats(sa, s.st))) return rc;
            if ((rc = link(s, n0, stem_sparse_plan(sa, StemPass::Stats).grid, cfg.init_ch, 0, cfg.init_ch, bstat0, M0))) return rc;
        }
        sa.Out = s.ws + L.D[0]; sa.ldo = b0.ld; sa.part = s.train ? s.part : nullptr;
        if ((rc = stem_sparse_pool(sa, s.st))) return rc;
        fr.nblk = stem_sparse_plan(sa, StemPass::Pool).grid;
        return 0;
    }
    TCVN_CHECK(hipMemsetAsync(s.ws + L.img, 0, (size_t)(L.own - L.img + pixel_owners_zero_bytes((long)n * cfg.H * cfg.W)), s.st));
    ScatterArgs sc{mode, coords, values, nnz, n, s.ws + L.img, cfg.H, cfg.W, cfg.in_ch, log_pixels, noise, s.seed,
                   PixelOwners{reinterpret_cast<uint32_t*>(s.ws + L.own), (long)n * cfg.H * cfg.W}};
    if ((rc = scatter_pixels(sc, s.st))) return rc;
    ConvFwdArgs a = conv0_args(s);
    stem_path.act_skip = !no_stem_skip && s.train && L.sact >= 0 && stem_fwd_ok(a) && (b0.ld & 7) == 0 && coords != nullptr;
    if (stem_path.act_skip &&      // (the shared row: the zero page is 1 KB; DMA sources use its first 256 B)
        (rc = stem_mark(coords, nnz, n, cfg.H, cfg.W, Hc, Wc, reinterpret_cast<uint32_t*>(s.ws + L.sact), data[s_b0], s.ws + L.zeros + 512, s.st))) return rc;
    a.part = s.train ? s.part : nullptr; a.nblk = conv_fwd_nblk(a);
    if ((rc = conv_fwd(a, s.st))) return rc;
    if ((rc = link(s, n0, a.nblk, cfg.init_ch, 0, cfg.init_ch, bstat0, M0))) return rc;
    const Tab t = tab(s.ws, L, n0);
    Pool0Args p{mode, s.ws + L.c0, n, Hc, Wc, cfg.init_ch, t.sc, t.sh, data[s_a0], s.ws + L.D[0], b0.ld, b0.H, b0.W,
                s.train ? s.part : nullptr, pool0_grid(n, b0.H, b0.W)};
    if ((rc = pool0_fwd(p, s.st))) return rc;
    fr.nblk = p.nblk;
    return 0;
}

// The path of dense layer (bi, l) in this call, decided from the layer's 3x3 arguments `c3` (conv3_args) before its first launch.  When the
// fused 1x1 kernel takes the layer (raw1x1), `f1` holds its arguments (lf / isum_out left to the caller).
LayerPath DenseNetPlan::layer_path(const Step& s, int bi, int l, const ConvFwdArgs& c3, Fwd1x1Args& f1) const {
    const Layout& L = s.L;
    const BlockGeom& bg = blocks[bi];
    const LayerSlots& ls = bg.layers[l];
    const long M = (long)s.n * bg.H * bg.W;
    const bool bf16 = cfg.mode == MODE_BF16, fast1 = L.XA[bi][l] >= 0;
    const Conv3x3Fwd k3 = bf16 ? conv3x3_fwd_kernel(c3) : CONV3X3_FWD_NONE;
    LayerPath p;
    // Eval mode (running statistics: no batch reduction between the 1x1 output and its BatchNorm): the 1x1 GEMM's epilogue
    // applies norm2 + PReLU and writes the activated map the 3x3 tile kernel stages -- the raw bottleneck output Y and the
    // k_act_bf16 pass over it (512 B per pixel and layer, one launch) do not exist.  Train mode needs Y for the statistics.
    p.fuse_ya = !s.train && !s.frozen && fast1 && k3 != CONV3X3_FWD_NONE;      // (a frozen pass keeps Y: its backward reads it)
    // Round 4: norm2 + PReLU are applied INSIDE the 3x3 kernel (and inside the layer's weight-gradient kernel): the raw
    // bottleneck map is staged by LDS-DMA and the wave that fetched a row activates it in LDS once -- the activated copy YA
    // (256 B written + 256 B read per pixel and layer) and the k_act_bf16 launch over Y do not exist.  Bit-identical images.
    p.act_fused = bf16 && !p.fuse_ya && conv3x3_act_fusable(c3);
    // Train mode (round 4): the 1x1 runs on the RAW concat buffer, norm1 + PReLU1 applied to the landed LDS tiles (fwd1x1_fused.hip);
    // the fused 1x1 backward kernel rebuilds that activation from x, so the activated copy XA is neither written nor read.
    static const bool no_fuse1 = TCVN_KNOB_SET("TCVN_NO_FWD1_FUSE") || TCVN_KNOB_SET("TCVN_NO_BWD1_FUSE");
    const bool keep = s.train || s.frozen;      // a backward follows: the layer keeps what it needs
    if ((keep || p.fuse_ya) && fast1 && !no_fuse1 && cfg.bn_size * cfg.growth == 128 && bf16) {
        const WkEntry& e = wk_find(ls.w1, 0, 1);
        const Tab t1 = tab(s.ws, L, ls.n1);
        f1 = Fwd1x1Args{};
        f1.Xin = s.ws + L.D[bi]; f1.ldx = bg.ld; f1.cin = ls.cin; f1.sc = t1.sc; f1.sh = t1.sh; f1.sl = data[ls.a1]; f1.M = M;
        f1.Wfrag = s.ws + L.wk + e.off; f1.Kp = e.Kp; f1.bias = data[ls.b1]; f1.Out = s.ws + L.Y[bi][l]; f1.zeros = s.ws + L.zeros;
        f1.part = s.train ? s.part : nullptr; f1.nblk = fwd1x1_fused_nblk(f1);
        if (!keep) {                   // eval: norm2 + PReLU2 in the epilogue, the activated map is the only output (as k_gemm_nt_bf16<.., XF = 2>)
            f1.osc = c3.sc; f1.osh = c3.sh; f1.osl = c3.sl; f1.Out = s.ws + L.YA[bi][l];
        }
        // train mode: the activated copy XA is only dropped when the backward's fused 1x1 kernel will accept this layer (it rebuilds
        // the activation from x); otherwise the step would die in backward after the forward has already run
        Bwd1x1Args b1;
        p.raw1x1 = fwd1x1_fused_ok(f1) && (!keep || bwd1x1_fill(bi, l, M, s.ws, L, b1));
    }
    const bool pair = k3 == CONV3X3_FWD_PAIR;            // the kernel that honours lf / isum_out and fills keep_out
    // norm2's consumer: the 3x3 pair kernel with the activation in LDS derives the table itself; anything else takes the link kernel
    p.lf2 = p.raw1x1 && s.lf_on && p.act_fused && pair;
    p.out_isum = s.lf_on && pair && cfg.growth <= 32;    // link-free producer of the new channels' statistics
    p.keep_stored = s.train && !L.KM[bi].empty() && pair;
    return p;
}

// ---- one dense layer: BN1 - PReLU1 - 1x1 conv -> Y; BN2 - PReLU2 - 3x3 conv - dropout -> D[:, cin:cin+g] ----
int DenseNetPlan::fwd_layer(const Step& s, int bi, int l, FreshStats& fr) {
    const Layout& L = s.L;
    const BlockGeom& bg = blocks[bi];
    const LayerSlots& ls = bg.layers[l];
    const long M = (long)s.n * bg.H * bg.W;
    const int mid = cfg.bn_size * cfg.growth, g = cfg.growth;
    char* D = s.ws + L.D[bi];
    char* Y = s.ws + L.Y[bi][l];
    double* bstatD = reinterpret_cast<double*>(s.ws + L.bstatD[bi]);
    double* bstatY = reinterpret_cast<double*>(s.ws + L.bstatY[bi][l]);
    long long* isumD = s.lf_on ? reinterpret_cast<long long*>(s.ws + L.isumD[bi]) : nullptr;      // [ld][2], indexed by channel
    long long* isumY = s.lf_on ? reinterpret_cast<long long*>(s.ws + L.isumY[bi][l]) : nullptr;
    int rc;
    ConvFwdArgs a = conv3_args(s, bi, l);
    Fwd1x1Args f1;
    const LayerPath p = path[bi][l] = layer_path(s, bi, l, a, f1);
    if (p.raw1x1) {
        // link-free consumer of norm1: the fresh window was added to isumD by the previous layer's 3x3 kernel (the block's first
        // layer follows a transition / the stem, whose statistics still leave as partial rows: link kernel)
        if (s.lf_on && fr.isum) f1.lf = lf_link(s, ls.n1, isumD + 2 * fr.c0, 2L * bg.ld, fr.c0, fr.n, bstatD, M);
        else if ((rc = link_fresh(s, ls.n1, bi, fr))) return rc;
        f1.isum_out = isumY; f1.isum_stride = 2L * mid;       // link-free producer of norm2's statistics
        if ((rc = fwd1x1_fused(f1, s.st))) return rc;
        if (!p.lf2 && (rc = link(s, ls.n2, f1.nblk, mid, 0, mid, bstatY, M, isumY, 2L * mid))) return rc;
    } else {
        if ((rc = link_fresh(s, ls.n1, bi, fr))) return rc;
        int nblk;
        if (L.XA[bi][l] >= 0) {
            // activated copy of the 1x1 input: operand of the bf16 GEMMs (forward, weight gradient); bottleneck 1x1 on the NT GEMM: XA x W1^T -> Y
            const int cin8 = (int)round_up(ls.cin, 8);
            const Tab t1 = tab(s.ws, L, ls.n1);
            ActArgs act{D, bg.ld, M, ls.cin, t1.sc, t1.sh, data[ls.a1], s.ws + L.XA[bi][l], cin8};
            if ((rc = act_bf16(act, s.st))) return rc;
            const WkEntry& e = wk_find(ls.w1, 0, 1);
            GemmNtArgs ga{};
            ga.epi = EPI_FWD; ga.A = s.ws + L.XA[bi][l]; ga.lda = cin8; ga.K = cin8; ga.M = M; ga.N = mid;
            ga.Wfrag = s.ws + L.wk + e.off; ga.Kp = e.Kp; ga.zeros = s.ws + L.zeros; ga.bias = data[ls.b1];
            ga.Out = Y; ga.ldo = mid; ga.n_off = 0; ga.part = s.train ? s.part : nullptr; ga.nblk = gemm_nt_nblk(ga);
            if (p.fuse_ya) {               // eval: norm2 + PReLU in the GEMM epilogue, the activated map is the only output
                ga.osc = a.sc; ga.osh = a.sh; ga.osl = a.sl; ga.Out = s.ws + L.YA[bi][l];
            }
            if ((rc = gemm_nt_bf16(ga, "k_gemm_nt_bf16<fwd1x1>", s.st))) return rc;
            nblk = ga.nblk;
        } else {
            ConvFwdArgs c1 = conv1_args(s, bi, l);
            c1.part = s.train ? s.part : nullptr; c1.nblk = conv_fwd_nblk(c1);
            if ((rc = conv_fwd(c1, s.st))) return rc;
            nblk = c1.nblk;
        }
        if ((rc = link(s, ls.n2, nblk, mid, 0, mid, bstatY, M))) return rc;
    }
    if (p.act_fused) a.act_fused = 1;
    else if (cfg.mode == MODE_BF16) {      // materialise prelu(bn(Y)) once (unless the 1x1 epilogue did); the tile kernel stages it by LDS-DMA
        if (!p.fuse_ya) {
            ActArgs act{Y, mid, M, mid, a.sc, a.sh, a.sl, s.ws + L.YA[bi][l], mid};
            if ((rc = act_bf16(act, s.st))) return rc;
        }
        a.Aact = s.ws + L.YA[bi][l];
    }
    a.part = s.train ? s.part : nullptr;
    a.drop_p = s.drop_p(cfg.dropout); a.seed = s.seed; a.stream_id = (uint32_t)(bi * 64 + l + 1);
    a.nblk = conv_fwd_nblk(a);
    if (p.lf2) {
        if (!a.act_fused) { fprintf(stderr, "tcvn: link-free norm2 without the in-LDS activation\n"); return -17; }
        a.lf = lf_link(s, ls.n2, isumY, 2L * mid, 0, mid, bstatY, M);
    }
    if (p.out_isum) { a.isum_out = isumD + 2 * ls.cin; a.isum_stride = 2L * bg.ld; }
    if (s.train && !L.KM[bi].empty()) a.keep_out = reinterpret_cast<uint32_t*>(s.ws + L.KM[bi][l]);      // the pair kernel leaves the keep flags it drew for the backward kernels
    if ((rc = conv_fwd(a, s.st))) return rc;
    fr = FreshStats{ls.cin, g, a.nblk, g, p.out_isum};
    return 0;
}

// ---- transition: BN - PReLU - 1x1 conv - AvgPool(2) (pool commuted in front of the conv) -> the first channels of block bi + 1;
//      last block: final_norm - PReLU - global average -> F ----
int DenseNetPlan::fwd_transition(const Step& s, int bi, FreshStats& fr) {
    const Layout& L = s.L;
    const BlockGeom& bg = blocks[bi];
    char* D = s.ws + L.D[bi];
    int rc;
    if ((rc = link_fresh(s, bg.has_trans ? bg.tn : nf, bi, fr))) return rc;
    if (!bg.has_trans) {
        const Tab t = tab(s.ws, L, nf);
        HeadPoolArgs a{cfg.mode, D, bg.ld, s.n, bg.H * bg.W, Cf, t.sc, t.sh, data[s_af], reinterpret_cast<float*>(s.ws + L.F)};
        return head_pool_fwd(a, s.st);
    }
    const BlockGeom& nb = blocks[bi + 1];
    fr = FreshStats{0, nb.C0, 0, bg.Ctot / 2, false};
    if (L.XP[bi] >= 0) {
        const Tab t = tab(s.ws, L, bg.tn);
        ActPoolArgs ap{D, bg.ld, s.n, bg.H, bg.W, bg.Ctot, t.sc, t.sh, data[bg.ta], s.ws + L.XP[bi], bg.ldp};
        if ((rc = cfg.mode == MODE_BF16 ? act_pool_bf16(ap, s.st) : act_pool_f32(ap, s.st))) return rc;
    }
    if (L.XP[bi] >= 0 && cfg.mode == MODE_BF16) {
        const WkEntry& ef = wk_find(bg.tw, 0, 1);
        GemmNtArgs ga{};
        ga.epi = EPI_FWD; ga.A = s.ws + L.XP[bi]; ga.lda = bg.ldp; ga.K = bg.ldp; ga.M = (long)s.n * nb.H * nb.W; ga.N = bg.Ctot / 2;
        ga.Wfrag = s.ws + L.wk + ef.off; ga.Kp = ef.Kp; ga.zeros = s.ws + L.zeros; ga.bias = data[bg.tb];
        ga.Out = s.ws + L.D[bi + 1]; ga.ldo = nb.ld; ga.n_off = 0; ga.part = s.train ? s.part : nullptr; ga.nblk = gemm_nt_nblk(ga);
        if ((rc = gemm_nt_bf16(ga, "k_gemm_nt_bf16<fwdtrans>", s.st))) return rc;
        fr.nblk = ga.nblk;
        return 0;
    }
    ConvFwdArgs a = trans_args(s, bi);
    a.part = s.train ? s.part : nullptr; a.nblk = conv_fwd_nblk(a);
    if ((rc = conv_fwd(a, s.st))) return rc;
    fr.nblk = a.nblk;
    return 0;
}

// ---- output block: Linear(no bias) - BatchNorm1d - PReLU - Dropout (layers/dense_net.py:157-162) ----
int DenseNetPlan::fwd_output(const Step& s, float* out, long out_ld) const {
    float* F = reinterpret_cast<float*>(s.ws + s.L.F);
    float* Z = reinterpret_cast<float*>(s.ws + s.L.Z);
    int rc;
    if ((rc = linear_fwd(F, Cf, data[s_wl], nullptr, Z, cfg.out_dim, s.n, cfg.out_dim, Cf, s.st))) return rc;
    float* hs = reinterpret_cast<float*>(s.ws + s.L.head_stat);
    RowsBnArgs r{};
    r.X = Z; r.ldx = cfg.out_dim; r.R = s.n; r.C = cfg.out_dim; r.gamma = data[nl.w]; r.beta = data[nl.b]; r.slope = data[s_al];
    r.running_mean = data[nl.rm]; r.running_var = data[nl.rv]; r.Y = out; r.ldy = out_ld;
    r.save_mean = hs; r.save_rstd = hs + cfg.out_dim; r.train = s.train; r.eps = kEps; r.momentum = kMom;
    r.drop_p = s.drop_p(cfg.dropout); r.seed = s.seed; r.stream_id = 0x4000u;
    return rows_bn_fwd(r, s.st);
}

int DenseNetPlan::tap(int n, const char* name, long* off, int* tn, int* th, int* tw, int* tc, int* tld, int* tes) const {
    Layout L;
    layout(n, false, L);
    std::string s(name);
    *tn = n; *tes = esz;
    if ((s == "img" || s == "conv0") && stem_path.sparse && n == last_n) return -1;      // the sparse stem materialises neither
    if (s == "img") { *off = L.img; *th = cfg.H; *tw = cfg.W; *tc = cfg.in_ch; *tld = cfg.in_ch; return 0; }
    if (s == "conv0") { *off = L.c0; *th = Hc; *tw = Wc; *tc = cfg.init_ch; *tld = cfg.init_ch; return 0; }
    if (s == "condense") { *off = L.F; *th = 1; *tw = 1; *tc = Cf; *tld = Cf; *tes = 4; return 0; }
    if (s == "raw:wk") { *tn = *th = *tw = 1; *off = L.wk; *tc = *tld = (int)(wk_bytes() / esz); return 0; }
    if (s == "raw:tabs") { *tn = *th = *tw = 1; *off = L.tabs; *tc = *tld = (int)tab_floats(); *tes = 4; return 0; }
    if (s.rfind("raw:ystat", 0) == 0) {                          // (mean, biased var) of a bottleneck map: "raw:ystat<block>.<layer>"
        int b = 0, l = 0;
        if (sscanf(s.c_str(), "raw:ystat%d.%d", &b, &l) != 2) return -1;
        b -= 1;
        if (b < 0 || b >= (int)blocks.size() || l < 0 || l >= blocks[b].L) return -1;
        *tn = *th = *tw = 1; *off = L.bstatY[b][l]; *tc = *tld = 2 * cfg.bn_size * cfg.growth; *tes = 8; return 0;
    }
    if (s.rfind("raw:isumy", 0) == 0) {                          // fixed-point accumulators of a bottleneck map whose norm2 the last forward derived link-free (LayerPath::lf2); else no such tap
        int b = 0, l = 0;
        if (sscanf(s.c_str(), "raw:isumy%d.%d", &b, &l) != 2) return -1;
        b -= 1;
        if (b < 0 || b >= (int)blocks.size() || l < 0 || l >= blocks[b].L || L.isumY.empty() || n != last_n || !path[b][l].lf2) return -1;
        *tn = *th = *tw = 1; *off = L.isumY[b][l]; *tc = *tld = LF_REP * 2 * cfg.bn_size * cfg.growth; *tes = 8; return 0;
    }
    if (s.rfind("raw:bstat", 0) == 0) {
        const int b = atoi(s.c_str() + 9) - 1;
        if (s == "raw:bstat0") { *tn = *th = *tw = 1; *off = L.bstat0; *tc = *tld = cfg.init_ch * 2; *tes = 8; return 0; }      // norm0's rows (conv0 output)
        if (b < 0 || b >= (int)blocks.size()) return -1;
        *tn = *th = *tw = 1; *off = L.bstatD[b]; *tc = *tld = blocks[b].ld * 2; *tes = 8; return 0;
    }
    // output block: the rows its BatchNorm1d normalises (Linear output, fp32) and, after a train-mode forward, the (mean, 1 / sqrt(var + eps)) rows it saved
    if (s == "output_linear") { *off = L.Z; *th = 1; *tw = 1; *tc = *tld = cfg.out_dim; *tes = 4; return 0; }
    // after a backward pass (read-only offsets into the backward layout)
    if (s.rfind("raw:grad", 0) == 0) {      // the gradient accumulator of block b's concat buffer ("raw:grad1": what reaches the stem)
        const int b = atoi(s.c_str() + 8) - 1;
        if (b < 0 || b >= (int)blocks.size()) return -1;
        Layout Lb;
        layout(n, true, Lb);
        *off = Lb.G[b]; *th = blocks[b].H; *tw = blocks[b].W; *tc = blocks[b].Ctot; *tld = blocks[b].ld; return 0;
    }
    // the stem's own backward state (checked by tests/stem_reference.py): "raw:du0" = DU0 = sc0 prelu0'(u) dz over the conv0 map (with the
    // activity bitmap on, rows no hit reaches are never stored), "raw:pq0" = BatchNorm0's [2][init_ch] fp32 (P0, Q0) rows
    if (s == "raw:du0" || s == "raw:pq0") {
        Layout Lb;
        layout(n, true, Lb);
        if (s == "raw:du0") { *off = Lb.du0; *th = Hc; *tw = Wc; *tc = *tld = cfg.init_ch; return 0; }
        *tn = *th = *tw = 1; *off = Lb.pq0; *tc = *tld = 2 * cfg.init_ch; *tes = 4; return 0;
    }
    if (s.rfind("raw:pq", 0) == 0) {        // the [2][ld] fp32 (P, Q) rows of block b's channels
        const int b = atoi(s.c_str() + 6) - 1;
        if (b < 0 || b >= (int)blocks.size()) return -1;
        Layout Lb;
        layout(n, true, Lb);
        *tn = *th = *tw = 1; *off = Lb.pqD[b]; *tc = *tld = 2 * blocks[b].ld; *tes = 4; return 0;
    }
    if (s == "raw:dcondense") {             // fp32 [n][Cf]: the gradient with respect to "condense" (what the head pooling backward spreads over the last block)
        Layout Lb;
        layout(n, true, Lb);
        *off = Lb.dF; *th = 1; *tw = 1; *tc = *tld = Cf; *tes = 4; return 0;
    }
    if (s.rfind("raw:du", 0) == 0) {        // "raw:du<b>": the bottleneck-sized scratch DU in block b's geometry -- every dense layer overwrites it, so
        const int b = atoi(s.c_str() + 6) - 1;      // it holds the 3x3 data gradient of the layer that ran last (layer 0 of the lowest block run)
        if (b < 0 || b >= (int)blocks.size()) return -1;
        Layout Lb;
        layout(n, true, Lb);
        *off = Lb.du; *th = blocks[b].H; *tw = blocks[b].W; *tc = *tld = cfg.bn_size * cfg.growth; return 0;
    }
    if (s.rfind("raw:ey", 0) == 0) {        // "raw:ey<b>.<l>": the eff rows [pixels][32] of the layer's 3x3 output gradient; the buffer exists in bf16 mode with growth 32,
        int b = 0, l = 0;                   // and only the consecutive-tile data-gradient kernel fills it (the caller knows which kernel ran)
        if (sscanf(s.c_str(), "raw:ey%d.%d", &b, &l) != 2) return -1;
        b -= 1;
        Layout Lb;
        layout(n, true, Lb);
        if (b < 0 || b >= (int)blocks.size() || l < 0 || l >= blocks[b].L || Lb.EY3[b].empty()) return -1;
        *off = Lb.EY3[b][l]; *th = blocks[b].H; *tw = blocks[b].W; *tc = *tld = 32; return 0;
    }
    if (s == "raw:head_stat") { *tn = *th = *tw = 1; *off = L.head_stat; *tc = *tld = 2 * cfg.out_dim; *tes = 4; return 0; }
    if (s.rfind("dense", 0) == 0) {
        const int b = atoi(s.c_str() + 5) - 1;
        if (b < 0 || b >= (int)blocks.size()) return -1;
        *off = L.D[b]; *th = blocks[b].H; *tw = blocks[b].W; *tc = blocks[b].Ctot; *tld = blocks[b].ld;
        return 0;
    }
    if (s.rfind("bottleneck", 0) == 0) {
        int b = 0, l = 0;
        if (sscanf(s.c_str(), "bottleneck%d.%d", &b, &l) != 2) return -1;
        b -= 1;
        if (b < 0 || b >= (int)blocks.size() || l < 0 || l >= blocks[b].L) return -1;
        for (const auto& pb : path)                              // eval pass with the activation in some GEMM epilogue: no raw Y exists
            for (const LayerPath& p : pb) if (n == last_n && p.fuse_ya) return -1;
        *off = L.Y[b][l]; *th = blocks[b].H; *tw = blocks[b].W; *tc = cfg.bn_size * cfg.growth; *tld = *tc;
        return 0;
    }
    if (s.rfind("xa", 0) == 0 || s.rfind("ya", 0) == 0) {      // bf16 mode: materialised activations (1x1 / 3x3 operands)
        int b = 0, l = 0;
        if (sscanf(s.c_str() + 2, "%d.%d", &b, &l) != 2) return -1;
        b -= 1;
        if (b < 0 || b >= (int)blocks.size() || l < 0 || l >= blocks[b].L) return -1;
        const bool xa = s[0] == 'x';
        if ((xa && (L.XA[b].empty() || L.XA[b][l] < 0)) || (!xa && L.YA[b].empty())) return -1;
        if (n == last_n && (xa ? path[b][l].raw1x1 : path[b][l].act_fused)) return -1;      // the 1x1 ran on the raw buffer / the map was activated in LDS only
        *off = xa ? L.XA[b][l] : L.YA[b][l]; *th = blocks[b].H; *tw = blocks[b].W;
        *tc = xa ? blocks[b].layers[l].cin : cfg.bn_size * cfg.growth; *tld = xa ? (int)round_up(*tc, 8) : *tc;
        return 0;
    }
    return -1;
}

// ---------------------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------------------
struct tcvn_densenet { DenseNetPlan plan; explicit tcvn_densenet(const tcvn_densenet_cfg& c) : plan(c) {} };

extern "C" {

int tcvn_version(void) { return 1; }
void tcvn_backward_overlap(int on) { tcvn::set_backward_overlap(on); }

int tcvn_densenet_create(const tcvn_densenet_cfg* cfg, tcvn_densenet** out) {
    if (!cfg || !out || cfg->n_blocks < 1 || cfg->n_blocks > 8) return -1;
    if (cfg->mode != TCVN_MODE_F32 && cfg->mode != TCVN_MODE_BF16) return -1;
    *out = new tcvn_densenet(*cfg);
    return 0;
}
void tcvn_densenet_destroy(tcvn_densenet* p) { delete p; }
int tcvn_densenet_num_slots(const tcvn_densenet* p) { return (int)p->plan.slots.size(); }
int tcvn_densenet_slot(const tcvn_densenet* p, int i, char* name, int cap, int64_t* numel, int* kind) {
    if (i < 0 || i >= (int)p->plan.slots.size()) return -1;
    const auto& s = p->plan.slots[i];
    if (name && cap > 0) { strncpy(name, s.name.c_str(), cap - 1); name[cap - 1] = 0; }
    if (numel) *numel = s.numel;
    if (kind) *kind = s.kind;
    return 0;
}
int tcvn_densenet_bind(tcvn_densenet* p, void* const* data, void* const* grad) { return p->plan.bind(data, grad); }
int64_t tcvn_densenet_workspace_bytes(const tcvn_densenet* p, int n_img, int with_backward) {
    Layout L;
    p->plan.layout(n_img, with_backward != 0, L);
    return L.total;
}
int tcvn_densenet_forward(tcvn_densenet* p, int n_img, const int32_t* coords, const float* values, int64_t nnz, int log_pixels,
                          float noise_std, float* out, int64_t out_ld, void* ws, int64_t ws_bytes, int train, uint64_t seed,
                          void* stream) {
    return p->plan.forward(n_img, coords, values, nnz, log_pixels, noise_std, out, out_ld, reinterpret_cast<char*>(ws), ws_bytes,
                           train, seed, reinterpret_cast<hipStream_t>(stream));
}
int tcvn_densenet_forward_mc(tcvn_densenet* p, int n_img, const int32_t* coords, const float* values, int64_t nnz, int log_pixels,
                             float* out, int64_t out_ld, void* ws, int64_t ws_bytes, uint64_t seed, int resume, void* stream) {
    return p->plan.forward(n_img, coords, values, nnz, log_pixels, 0.f, out, out_ld, reinterpret_cast<char*>(ws), ws_bytes, 0, seed,
                           reinterpret_cast<hipStream_t>(stream), true, resume != 0);
}
int tcvn_densenet_forward_frozen(tcvn_densenet* p, int n_img, const int32_t* coords, const float* values, int64_t nnz, int log_pixels,
                                 float* out, int64_t out_ld, void* ws, int64_t ws_bytes, void* stream) {
    return p->plan.forward(n_img, coords, values, nnz, log_pixels, 0.f, out, out_ld, reinterpret_cast<char*>(ws), ws_bytes, 0, 0,
                           reinterpret_cast<hipStream_t>(stream), false, false, true);
}
int tcvn_densenet_input_gradient(tcvn_densenet* p, int n_img, const float* d_out, int64_t d_out_ld, float* d_values, void* ws,
                                 int64_t ws_bytes, void* stream) {
    return p->plan.input_gradient(n_img, d_out, d_out_ld, d_values, reinterpret_cast<char*>(ws), ws_bytes, reinterpret_cast<hipStream_t>(stream));
}
int tcvn_densenet_backward(tcvn_densenet* p, int n_img, const float* d_out, int64_t d_out_ld, void* ws, int64_t ws_bytes,
                           void* stream) {
    return p->plan.backward(n_img, d_out, d_out_ld, reinterpret_cast<char*>(ws), ws_bytes, reinterpret_cast<hipStream_t>(stream));
}
int tcvn_densenet_num_blocks(const tcvn_densenet* p) { return (int)p->plan.blocks.size(); }
int tcvn_densenet_backward_blocks(tcvn_densenet* p, int n_img, const float* d_out, int64_t d_out_ld, void* ws, int64_t ws_bytes,
                                  int block_hi, int block_lo, void* stream) {
    return p->plan.backward(n_img, d_out, d_out_ld, reinterpret_cast<char*>(ws), ws_bytes, reinterpret_cast<hipStream_t>(stream), block_hi,
                            block_lo);
}
int tcvn_densenet_tap(const tcvn_densenet* p, int n_img, const char* name, int64_t* byte_off, int* n, int* h, int* w, int* c,
                      int* ld, int* elem_bytes) {
    long off = 0;
    int rc = p->plan.tap(n_img, name, &off, n, h, w, c, ld, elem_bytes);
    *byte_off = off;
    return rc;
}

}  // extern "C"
