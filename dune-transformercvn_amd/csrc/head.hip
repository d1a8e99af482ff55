// Token path engine: combined embedding (LinearBlock), transformer encoder, event / prong decoders and the softmax
// focal loss; forward, loss and backward on one stream.  Reference call chain:
//   networks/neutrino_full_base_network.py:113-125 (combined embedding, pad), :184-188 (encoder, decoders)
//   layers/prong_custom_bert_encoder.py:57-75, layers/prong_decoder.py:15-16, layers/prong_target_decoder.py:34-41
//   trainers/neutrino_full_base_trainer.py:148-177 (loss)
// All arithmetic fp32 (this path is < 0.03 % of the FLOPs).
#include <string>
#include <vector>
#include <cstring>

#include "../../include/tcvn_hip.h"
#include "head_plan.h"
#include "tcvn_rows.h"
#include "tcvn_encoder.h"
#include "tcvn_input_grad.h"

using namespace tcvn;

namespace {
constexpr float kEps = 1e-5f, kMom = 0.1f;
// Dropout stream ids: forward draws and backward replays the mask of (seed, stream id, element)
constexpr uint32_t kSidCombined = 0x5000u;
constexpr uint32_t sid_enc(int l, int k) { return 0x6000u + l * 8 + k; }     // encoder layer l; k = 0 attention probabilities, 1 attention branch, 2 activation, 3 feed-forward branch
constexpr uint32_t sid_dec(int i) { return 0x7000u + (uint32_t)i; }           // prong decoder layer i

__global__ void k_combine_loss(const float* oe, const float* op, float ew, float* losses, float* accs) {
    losses[0] = ew * oe[0] + (1.f - ew) * op[0];
    losses[1] = oe[0]; losses[2] = op[0];
    accs[0] = oe[1]; accs[1] = op[1];
}
}  // namespace

int HeadPlan::add_slot(const std::string& name, long numel, int kind) {
    slots.push_back({name, numel, kind});
    return (int)slots.size() - 1;
}
HBn HeadPlan::add_bn(const std::string& p, int c) {
    HBn s;
    s.w = add_slot(p + ".weight", c, TCVN_SLOT_PARAM);
    s.b = add_slot(p + ".bias", c, TCVN_SLOT_PARAM);
    s.rm = add_slot(p + ".running_mean", c, TCVN_SLOT_BUFFER);
    s.rv = add_slot(p + ".running_var", c, TCVN_SLOT_BUFFER);
    add_slot(p + ".num_batches_tracked", 1, TCVN_SLOT_COUNTER);
    return s;
}

HeadPlan::HeadPlan(const tcvn_head_cfg& c) : cfg(c) {
    const int D = cfg.hidden_dim;
    const std::string ce = "prong_embedding.combined_embedding";
    // LinearBlock (layers/prong_feature_embedding.py:7-33): Linear(bias = not linear_batch_norm) - BatchNorm1d | Identity - PReLU | ReLU - Dropout
    const bool bn = !cfg.no_linear_bn, prelu_act = !cfg.linear_relu;
    comb.in = cfg.in_dim; comb.out = D; comb.sid = kSidCombined; comb.drop = true;
    comb.w = add_slot(ce + ".linear.weight", (long)D * cfg.in_dim, TCVN_SLOT_PARAM);
    if (!bn) comb.b = add_slot(ce + ".linear.bias", D, TCVN_SLOT_PARAM);
    if (bn) comb.n = add_bn(ce + ".norm", D);
    if (prelu_act) comb.a = add_slot(ce + ".activation.weight", D, TCVN_SLOT_PARAM);
    for (int l = 0; l < cfg.n_layers; ++l) {
        const std::string p = "encoder.encoder.layers." + std::to_string(l);
        HLayer L;
        L.win = add_slot(p + ".self_attn.in_proj_weight", 3L * D * D, TCVN_SLOT_PARAM);
        L.bin = add_slot(p + ".self_attn.in_proj_bias", 3 * D, TCVN_SLOT_PARAM);
        L.wo = add_slot(p + ".self_attn.out_proj.weight", (long)D * D, TCVN_SLOT_PARAM);
        L.bo = add_slot(p + ".self_attn.out_proj.bias", D, TCVN_SLOT_PARAM);
        L.w1 = add_slot(p + ".linear1.weight", (long)D * D, TCVN_SLOT_PARAM);
        L.b1 = add_slot(p + ".linear1.bias", D, TCVN_SLOT_PARAM);
        L.w2 = add_slot(p + ".linear2.weight", (long)D * D, TCVN_SLOT_PARAM);
        L.b2 = add_slot(p + ".linear2.bias", D, TCVN_SLOT_PARAM);
        L.g1 = add_slot(p + ".norm1.weight", D, TCVN_SLOT_PARAM);
        L.be1 = add_slot(p + ".norm1.bias", D, TCVN_SLOT_PARAM);
        L.g2 = add_slot(p + ".norm2.weight", D, TCVN_SLOT_PARAM);
        L.be2 = add_slot(p + ".norm2.bias", D, TCVN_SLOT_PARAM);
        layers.push_back(L);
    }
    ew = add_slot("event_decoder.hidden_layer.weight", (long)cfg.event_classes * D, TCVN_SLOT_PARAM);
    eb = add_slot("event_decoder.hidden_layer.bias", cfg.event_classes, TCVN_SLOT_PARAM);
    int idx = 0, in = D;
    for (int i = 0; i < cfg.n_dec; ++i) {
        const std::string p = "prong_decoder.hidden_layers.";
        HDec d;
        d.in = in; d.out = cfg.dec_dims[i]; d.sid = sid_dec(i); d.drop = cfg.dropout_modules != 0;
        // create_linear_block (layers/encoder.py:10-24): [Linear, BatchNorm1d?, PReLU | ReLU, Dropout?] -- the Sequential indices follow
        d.w = add_slot(p + std::to_string(idx) + ".weight", (long)d.out * d.in, TCVN_SLOT_PARAM);
        d.b = add_slot(p + std::to_string(idx) + ".bias", d.out, TCVN_SLOT_PARAM);
        if (bn) d.n = add_bn(p + std::to_string(idx + 1), d.out);
        if (prelu_act) d.a = add_slot(p + std::to_string(idx + 1 + (bn ? 1 : 0)) + ".weight", d.out, TCVN_SLOT_PARAM);
        idx += 2 + (bn ? 1 : 0) + (cfg.dropout_modules ? 1 : 0);
        in = d.out;
        dec.push_back(d);
    }
    dec_width = in;
    ow = add_slot("prong_decoder.output_layer.weight", (long)cfg.prong_classes * cfg.dec_out_in, TCVN_SLOT_PARAM);
    ob = add_slot("prong_decoder.output_layer.bias", cfg.prong_classes, TCVN_SLOT_PARAM);
    data.assign(slots.size(), nullptr);
    grad.assign(slots.size(), nullptr);
}

int HeadPlan::bind(void* const* d, void* const* g) {
    for (size_t i = 0; i < slots.size(); ++i) {
        data[i] = reinterpret_cast<float*>(d[i]);
        grad[i] = g ? reinterpret_cast<float*>(g[i]) : nullptr;
        if (slots[i].kind != TCVN_SLOT_COUNTER && data[i] == nullptr) return -10;
    }
    bound = true;
    return 0;
}

void HeadPlan::layout(int B, int P, int nP, HLayout& L) const {
    Bump b;
    const int D = cfg.hidden_dim, S = 1 + P, T = S * B, R = B + nP, TP = P * B, H = cfg.heads;
    const long td = (long)T * D * 4;
    L.Zc = b.take((long)R * D * 4); L.C = b.take((long)R * D * 4); L.cstat = b.take(2L * D * 4);
    L.X.clear(); L.lay.clear();
    for (int l = 0; l <= cfg.n_layers; ++l) L.X.push_back(b.take(td));
    for (int l = 0; l < cfg.n_layers; ++l) {
        HLayBuf q;
        q.qkv = b.take(3 * td); q.probs = b.take((long)B * H * S * S * 4); q.ctx = b.take(td); q.ao = b.take(td);
        q.xh1 = b.take(td); q.rstd1 = b.take((long)T * 4); q.x1 = b.take(td); q.hpre = b.take(td); q.hact = b.take(td);
        q.f = b.take(td); q.xh2 = b.take(td); q.rstd2 = b.take((long)T * 4);
        q.h1 = cfg.norm_first ? b.take(td) : -1; q.h2 = cfg.norm_first ? b.take(td) : -1;
        L.lay.push_back(q);
    }
    L.HID = b.take(td);
    L.Zd.clear(); L.Ad.clear(); L.dstat.clear();
    for (const auto& d : dec) {
        L.Zd.push_back(b.take((long)TP * d.out * 4)); L.Ad.push_back(b.take((long)TP * d.out * 4));
        L.dstat.push_back(b.take(2L * d.out * 4));
    }
    L.LG = b.take((long)TP * cfg.prong_classes * 4);
    L.dEv = b.take((long)B * cfg.event_classes * 4); L.dPr = b.take((long)B * P * cfg.prong_classes * 4);
    L.lossbuf = b.take(64);
    // backward scratch
    L.dLG = b.take((long)TP * cfg.prong_classes * 4);
    L.t0 = b.take(3 * td); L.t1 = b.take(3 * td); L.t2 = b.take(td); L.t3 = b.take(td); L.dHID = b.take(td);
    L.dC = b.take((long)R * D * 4); L.dZc = b.take((long)R * D * 4);
    // fused encoder backward: per-layer weight-gradient operands and per-event LayerNorm sums
    for (int l = 0; l < cfg.n_layers; ++l) {
        HLayBuf& q = L.lay[l];
        q.g_dqkv = b.take(3 * td); q.g_dao = b.take(td); q.g_dhp = b.take(td); q.g_df = b.take(td);
    }
    L.lnp = b.take((long)B * cfg.n_layers * 4 * D * 4);
    L.total = b.off;
}

// ---- the step: what check() was, plus every size constant the drivers derive from (B, P, nP) ---------------------------------
int HeadPlan::step(int B, int P, int nP, void* ws, long ws_bytes, int train, uint64_t seed, hipStream_t st, HeadStep& s, bool draw, bool keep_note) const {
    if (!keep_note) last_frozen_ws = nullptr;
    if (!bound) return -11;
    if (cfg.dec_out_in != dec_width) { fprintf(stderr, "tcvn: prong decoder width mismatch (reference would fail too)\n"); return -21; }
    if (B <= 0 || P < 0 || nP < 0 || 1 + P > 64) return -1;          // attention kernel: sequences up to 64 tokens
    s.B = B; s.P = P; s.nP = nP; s.S = 1 + P; s.T = s.S * B; s.R = B + nP; s.TP = P * B;
    s.ws = reinterpret_cast<char*>(ws); s.train = train; s.seed = seed; s.draw = draw && !train; s.st = st;
    s.dp = train || s.draw ? cfg.dropout : 0.f;
    layout(B, P, nP, s.L);
    return ws_bytes < s.L.total ? -12 : 0;
}

// The ONE place that chooses the encoder's kernels: encode() and backward() switch on it
EncPath HeadPlan::enc_path(int S) const {
    if (fused_encoder && encoder_fused_ok(S, cfg.hidden_dim, cfg.heads, cfg.n_layers, cfg.norm_first)) return EncPath::FUSED;
    return cfg.norm_first ? EncPath::PRE_NORM : EncPath::POST_NORM;
}

// ---- launch arguments shared by forward and backward ----------------------------------------------------------------------
EncLayerW HeadPlan::enc_w(int l) const {
    const HLayer& W = layers[l];
    return EncLayerW{data[W.win], data[W.bin], data[W.wo], data[W.bo], data[W.w1], data[W.b1], data[W.w2], data[W.b2],
                     data[W.g1], data[W.be1], data[W.g2], data[W.be2]};
}
EncLayerBuf HeadPlan::enc_buf(const HeadStep& s, int l) const {
    const HLayBuf& q = s.L.lay[l];
    return EncLayerBuf{s.F(q.qkv), s.F(q.probs), s.F(q.ctx), s.F(q.xh1), s.F(q.rstd1), s.F(q.x1), s.F(q.hpre), s.F(q.hact), s.F(q.xh2),
                       s.F(q.rstd2), s.F(s.L.X[l + 1])};
}
// LinearBlock behind its Linear: X [rows][d.out] -> Y, batch statistics kept at stat; the backward takes dY back to dX
RowsBnArgs HeadPlan::block_fwd(const HDec& d, const HeadStep& s, long X, long Y, long stat, int rows) const {
    RowsBnArgs r{};
    r.X = s.F(X); r.ldx = d.out; r.R = rows; r.C = d.out; r.slope = d.a >= 0 ? data[d.a] : nullptr; r.no_norm = cfg.no_linear_bn;
    if (!r.no_norm) { r.gamma = data[d.n.w]; r.beta = data[d.n.b]; r.running_mean = data[d.n.rm]; r.running_var = data[d.n.rv]; }
    r.Y = s.F(Y); r.ldy = d.out;
    r.save_mean = s.F(stat); r.save_rstd = s.F(stat) + d.out; r.train = s.train; r.eps = kEps; r.momentum = kMom;
    r.drop_p = d.drop ? s.dp : 0.f; r.seed = s.seed; r.stream_id = d.sid;
    return r;
}
RowsBnBwdArgs HeadPlan::block_bwd(const HDec& d, const HeadStep& s, long X, long dY, long stat, long dX, int rows) const {
    RowsBnBwdArgs r{};
    r.X = s.F(X); r.ldx = d.out; r.dY = s.F(dY); r.lddy = d.out; r.R = rows; r.C = d.out;
    r.no_norm = cfg.no_linear_bn; r.slope = d.a >= 0 ? data[d.a] : nullptr; r.dslope = d.a >= 0 ? grad[d.a] : nullptr;
    if (!r.no_norm) { r.gamma = data[d.n.w]; r.beta = data[d.n.b]; r.dgamma = grad[d.n.w]; r.dbeta = grad[d.n.b]; }
    r.save_mean = s.F(stat); r.save_rstd = s.F(stat) + d.out;
    r.dX = s.F(dX); r.lddx = d.out;
    r.drop_p = d.drop ? s.dp : 0.f; r.seed = s.seed; r.stream_id = d.sid;
    return r;
}
// The block's backward: on batch statistics with its parameter gradients, or (frozen) the running-statistics form for the data alone
int HeadPlan::block_bwd_run(const HDec& d, const HeadStep& s, long X, long dY, long stat, long dX, int rows) const {
    if (!s.frozen) return rows_bn_bwd(block_bwd(d, s, X, dY, stat, dX, rows), s.st);
    RowsBnFrozenBwdArgs r{};
    r.X = s.F(X); r.ldx = d.out; r.dY = s.F(dY); r.lddy = d.out; r.R = rows; r.C = d.out; r.no_norm = cfg.no_linear_bn;
    r.slope = d.a >= 0 ? data[d.a] : nullptr; r.eps = kEps; r.dX = s.F(dX); r.lddx = d.out;
    if (!r.no_norm) { r.gamma = data[d.n.w]; r.beta = data[d.n.b]; r.running_mean = data[d.n.rm]; r.running_var = data[d.n.rv]; }
    return rows_bn_bwd_frozen(r, s.st);
}
// The prong decoder chain: layer i (i == n_dec: the output layer) reads the prong tokens of HID (i == 0) or the block before it, and
// its input gradient goes to the prong rows of dHID or to the scratch t0 that the block before reads as its dY.
DecIn HeadPlan::dec_in(const HeadStep& s, int i) const {
    const long hid_prongs = (long)s.B * cfg.hidden_dim;
    if (i == 0) return DecIn{s.F(s.L.HID) + hid_prongs, s.F(s.L.dHID) + hid_prongs, cfg.hidden_dim};
    return DecIn{s.F(s.L.Ad[i - 1]), s.F(s.L.t0), dec[i - 1].out};
}

// ---- stage 1: combined embedding (LinearBlock over event + packed prong rows) and the token gather -> L.X[0] ------------
int HeadPlan::embed(const HeadStep& s, const float* rows, const int32_t* tok_row) const {
    const HLayout& L = s.L;
    const int D = cfg.hidden_dim;
    if (int rc = linear_fwd(rows, cfg.in_dim, data[comb.w], comb.b >= 0 ? data[comb.b] : nullptr, s.F(L.Zc), D, s.R, D, cfg.in_dim, s.st)) return rc;
    if (int rc = rows_bn_fwd(block_fwd(comb, s, L.Zc, L.C, L.cstat, s.R), s.st)) return rc;
    return gather_tokens(s.F(L.C), tok_row, s.F(L.X[0]), s.B, s.S, D, s.st);
}

// ---- stage 2: transformer encoder, L.X[0] (sequence-major tokens, padding rows zero) -> L.HID (masked) ------------------
int HeadPlan::encode(const HeadStep& s, const int32_t* tok_row) const {
    switch (enc_path(s.S)) {
    case EncPath::FUSED: {                                      // one launch for the whole stack (+ mask)
        EncFusedArgs a{};
        a.X0 = s.F(s.L.X[0]); a.tok_row = tok_row; a.HID = s.F(s.L.HID); a.B = s.B; a.S = s.S; a.H = cfg.heads; a.L = cfg.n_layers;
        a.gelu = cfg.gelu; a.save = 1; a.eps = kEps; a.drop_p = s.dp; a.seed = s.seed;
        for (int l = 0; l < cfg.n_layers; ++l) { a.w[l] = enc_w(l); a.buf[l] = enc_buf(s, l); }
        return encoder_fused_fwd(a, s.st);
    }
    case EncPath::POST_NORM: return encode_post(s, tok_row);
    case EncPath::PRE_NORM: return encode_pre(s, tok_row);
    }
    return -1;
}
int HeadPlan::encode_post(const HeadStep& s, const int32_t* tok_row) const {
    const HLayout& L = s.L;
    const int D = cfg.hidden_dim, T = s.T, H = cfg.heads, hd = D / H;
    for (int l = 0; l < cfg.n_layers; ++l) {
        const HLayer& W = layers[l];
        const HLayBuf& q = L.lay[l];
        if (int rc = linear_fwd(s.F(L.X[l]), D, data[W.win], data[W.bin], s.F(q.qkv), 3 * D, T, 3 * D, D, s.st)) return rc;
        AttnArgs a{s.F(q.qkv), tok_row, s.F(q.probs), s.F(q.ctx), s.B, s.S, H, hd, s.dp, s.seed, sid_enc(l, 0)};
        if (int rc = attn_fwd(a, s.st)) return rc;
        if (int rc = linear_fwd(s.F(q.ctx), D, data[W.wo], data[W.bo], s.F(q.ao), D, T, D, D, s.st)) return rc;
        AddLnArgs n1{s.F(L.X[l]), s.F(q.ao), data[W.g1], data[W.be1], s.F(q.x1), s.F(q.xh1), s.F(q.rstd1), T, D, kEps, s.dp, s.seed, sid_enc(l, 1)};
        if (int rc = add_ln_fwd(n1, s.st)) return rc;
        if (int rc = linear_fwd(s.F(q.x1), D, data[W.w1], data[W.b1], s.F(q.hpre), D, T, D, D, s.st)) return rc;
        if (int rc = act_fwd(s.F(q.hpre), s.F(q.hact), (long)T * D, cfg.gelu, s.dp, s.seed, sid_enc(l, 2), s.st)) return rc;
        if (int rc = linear_fwd(s.F(q.hact), D, data[W.w2], data[W.b2], s.F(q.f), D, T, D, D, s.st)) return rc;
        AddLnArgs n2{s.F(q.x1), s.F(q.f), data[W.g2], data[W.be2], s.F(L.X[l + 1]), s.F(q.xh2), s.F(q.rstd2), T, D, kEps, s.dp, s.seed, sid_enc(l, 3)};
        if (int rc = add_ln_fwd(n2, s.st)) return rc;
    }
    return mask_rows(s.F(L.X[cfg.n_layers]), tok_row, s.F(L.HID), s.B, s.S, D, s.st);
}
// pre-norm variant (prong_custom_bert_encoder.py:45-52 with transformer_norm_first): x += drop(sa(LN1(x))); x += drop(ff(LN2(x))).
// LN(x) is add_ln_fwd with a zero residual branch (t0 is scratch of the backward pass, free here).
int HeadPlan::encode_pre(const HeadStep& s, const int32_t* tok_row) const {
    const HLayout& L = s.L;
    const int D = cfg.hidden_dim, T = s.T, H = cfg.heads, hd = D / H;
    float* zero = s.F(L.t0);
    TCVN_CHECK(hipMemsetAsync(zero, 0, (size_t)T * D * 4, s.st));
    for (int l = 0; l < cfg.n_layers; ++l) {
        const HLayer& W = layers[l];
        const HLayBuf& q = L.lay[l];
        AddLnArgs n1{s.F(L.X[l]), zero, data[W.g1], data[W.be1], s.F(q.h1), s.F(q.xh1), s.F(q.rstd1), T, D, kEps, 0.f, s.seed, sid_enc(l, 1)};
        if (int rc = add_ln_fwd(n1, s.st)) return rc;
        if (int rc = linear_fwd(s.F(q.h1), D, data[W.win], data[W.bin], s.F(q.qkv), 3 * D, T, 3 * D, D, s.st)) return rc;
        AttnArgs a{s.F(q.qkv), tok_row, s.F(q.probs), s.F(q.ctx), s.B, s.S, H, hd, s.dp, s.seed, sid_enc(l, 0)};
        if (int rc = attn_fwd(a, s.st)) return rc;
        if (int rc = linear_fwd(s.F(q.ctx), D, data[W.wo], data[W.bo], s.F(q.ao), D, T, D, D, s.st)) return rc;
        if (int rc = add_drop(s.F(L.X[l]), s.F(q.ao), s.F(q.x1), (long)T * D, s.dp, s.seed, sid_enc(l, 1), s.st)) return rc;
        AddLnArgs n2{s.F(q.x1), zero, data[W.g2], data[W.be2], s.F(q.h2), s.F(q.xh2), s.F(q.rstd2), T, D, kEps, 0.f, s.seed, sid_enc(l, 3)};
        if (int rc = add_ln_fwd(n2, s.st)) return rc;
        if (int rc = linear_fwd(s.F(q.h2), D, data[W.w1], data[W.b1], s.F(q.hpre), D, T, D, D, s.st)) return rc;
        if (int rc = act_fwd(s.F(q.hpre), s.F(q.hact), (long)T * D, cfg.gelu, s.dp, s.seed, sid_enc(l, 2), s.st)) return rc;
        if (int rc = linear_fwd(s.F(q.hact), D, data[W.w2], data[W.b2], s.F(q.f), D, T, D, D, s.st)) return rc;
        if (int rc = add_drop(s.F(q.x1), s.F(q.f), s.F(L.X[l + 1]), (long)T * D, s.dp, s.seed, sid_enc(l, 3), s.st)) return rc;
    }
    return mask_rows(s.F(L.X[cfg.n_layers]), tok_row, s.F(L.HID), s.B, s.S, D, s.st);
}

// ---- stage 3: event decoder on token 0, prong decoder on tokens 1..P of L.HID -------------------------------------------
int HeadPlan::decode(const HeadStep& s, float* ev_logits, float* pr_logits) const {
    const HLayout& L = s.L;
    const int D = cfg.hidden_dim, TP = s.TP, n_dec = (int)dec.size();
    if (ev_logits)
        if (int rc = linear_fwd(s.F(L.HID), D, data[ew], data[eb], ev_logits, cfg.event_classes, s.B, cfg.event_classes, D, s.st)) return rc;
    if (!pr_logits || TP == 0) return 0;
    for (int i = 0; i < n_dec; ++i) {
        const HDec& d = dec[i];
        const DecIn in = dec_in(s, i);
        if (int rc = linear_fwd(in.x, in.w, data[d.w], data[d.b], s.F(L.Zd[i]), d.out, TP, d.out, d.in, s.st)) return rc;
        if (int rc = rows_bn_fwd(block_fwd(d, s, L.Zd[i], L.Ad[i], L.dstat[i], TP), s.st)) return rc;
    }
    const DecIn in = dec_in(s, n_dec);
    if (int rc = linear_fwd(in.x, in.w, data[ow], data[ob], s.F(L.LG), cfg.prong_classes, TP, cfg.prong_classes, cfg.dec_out_in, s.st)) return rc;
    return permute_rows(s.F(L.LG), pr_logits, s.B, s.P, cfg.prong_classes, 1, s.st);
}

int HeadPlan::forward(int B, int P, int nP, const float* rows, const int32_t* tok_row, float* ev_logits, float* pr_logits,
                      void* ws, long ws_bytes, int train, uint64_t seed, hipStream_t st, bool draw) {
    HeadStep s;
    if (int rc = step(B, P, nP, ws, ws_bytes, train, seed, st, s, draw)) return rc;
    if (int rc = embed(s, rows, tok_row)) return rc;
    if (int rc = encode(s, tok_row)) return rc;
    if (int rc = decode(s, ev_logits, pr_logits)) return rc;
    last_seed = seed;
    return 0;
}

// Frozen pass (hit gradients).  The token path keeps its backward state in every forward (one layout, the fused encoder always saves), so
// the frozen forward IS the eval forward -- running statistics, dropout 0 -- plus the note that input_gradient may follow on this workspace.
int HeadPlan::forward_frozen(int B, int P, int nP, const float* rows, const int32_t* tok_row, float* ev_logits, float* pr_logits,
                             void* ws, long ws_bytes, hipStream_t st) {
    if (int rc = forward(B, P, nP, rows, tok_row, ev_logits, pr_logits, ws, ws_bytes, 0, 0, st)) return rc;
    last_frozen_ws = ws; last_frozen_shape[0] = B; last_frozen_shape[1] = P; last_frozen_shape[2] = nP;
    return 0;
}

// Data-only backward of the last frozen forward: the reverse schedule of backward() with dropout probability 0 at every site (not the replay
// of cfg.dropout), the running-statistics rows backward in every LinearBlock, and no parameter gradient -- every dW / db / LayerNorm
// gradient launch is left out (gp() gives null), the bound grad pointers are not read and may be null.
int HeadPlan::input_gradient(int B, int P, int nP, const float* rows, const int32_t* tok_row, const float* dEv, const float* dPr,
                             float* d_rows, void* ws, long ws_bytes, hipStream_t st) {
    if (bound && (last_frozen_ws == nullptr || last_frozen_ws != ws || last_frozen_shape[0] != B || last_frozen_shape[1] != P || last_frozen_shape[2] != nP)) {
        fprintf(stderr, "tcvn: head input_gradient: the last forward of this plan on this workspace was not a frozen forward of this batch\n");
        return -21;
    }
    HeadStep s;
    if (int rc = step(B, P, nP, ws, ws_bytes, 0, 0, st, s, false, true)) return rc;      // (the note stays: other seeds may follow on the same forward)
    s.frozen = true;
    return backward_chain(s, rows, tok_row, dEv, dPr, d_rows);
}

int HeadPlan::loss(int B, int P, const float* ev_logits, const float* pr_logits, const int64_t* et, const int8_t* pt, float* losses,
                   float* accs, float* dEv, float* dPr, hipStream_t st) {
    float* lb = accs + 2;                       // accs has room for 2 + 4 floats (scratch behind the two accuracies)
    if (int rc = focal_i64(ev_logits, et, B, cfg.event_classes, cfg.gamma, cfg.event_weight, dEv, lb, st)) return rc;
    if (int rc = focal_i8(pr_logits, pt, B * P, cfg.prong_classes, cfg.gamma, 1.f - cfg.event_weight, dPr, lb + 2, st)) return rc;
    hipLaunchKernelGGL(k_combine_loss, dim3(1), dim3(1), 0, st, lb, lb + 2, cfg.event_weight, losses, accs);
    TCVN_LAUNCH_CHECK();
    return 0;
}

// ---- backward: decoders -> dHID, mask, encoder (one of three paths) -> d X[0], combined embedding -> d_rows ----------------
int HeadPlan::backward(int B, int P, int nP, const float* rows, const int32_t* tok_row, const float* dEv, const float* dPr,
                       float* d_rows, void* ws, long ws_bytes, hipStream_t st) {
    if (bound)                                   // an unbound plan is the step's -11, which comes first
        for (size_t i = 0; i < slots.size(); ++i)
            if (slots[i].kind == TCVN_SLOT_PARAM && grad[i] == nullptr) return -14;
    // train = 1 always: backward replays the masks of cfg.dropout whatever the forward's train flag was (the backward of an
    // eval-mode forward is not supported; callers run it after train-mode forwards only)
    if (bound && last_frozen_ws == ws) { fprintf(stderr, "tcvn: head backward after a frozen forward: only tcvn_head_input_gradient is defined there\n"); return -20; }
    HeadStep s;
    if (int rc = step(B, P, nP, ws, ws_bytes, 1, last_seed, st, s)) return rc;
    return backward_chain(s, rows, tok_row, dEv, dPr, d_rows);
}
int HeadPlan::backward_chain(const HeadStep& s, const float* rows, const int32_t* tok_row, const float* dEv, const float* dPr, float* d_rows) const {
    if (int rc = decoders_bwd(s, dEv, dPr)) return rc;
    float* dX = s.F(s.L.t2);
    if (int rc = mask_rows(s.F(s.L.dHID), tok_row, dX, s.B, s.S, cfg.hidden_dim, s.st)) return rc;
    int rc = 0;
    switch (enc_path(s.S)) {
    case EncPath::FUSED: rc = encoder_bwd_fused(s, dX, s.F(s.L.t3)); dX = s.F(s.L.t3); break;
    case EncPath::POST_NORM: rc = encoder_bwd_post(s, dX); break;
    case EncPath::PRE_NORM: rc = encoder_bwd_pre(s, dX); break;
    }
    return rc ? rc : embed_bwd(s, dX, rows, tok_row, d_rows);
}

// prong decoder (output layer, then the blocks last to first) and event decoder -> dHID
int HeadPlan::decoders_bwd(const HeadStep& s, const float* dEv, const float* dPr) const {
    const HLayout& L = s.L;
    const int D = cfg.hidden_dim, TP = s.TP, Ce = cfg.event_classes, Cp = cfg.prong_classes, n_dec = (int)dec.size();
    if (int rc = permute_rows(dPr, s.F(L.dLG), s.B, s.P, Cp, 0, s.st)) return rc;
    const DecIn last = dec_in(s, n_dec);
    if (int rc = linear_bwd_dw(s.F(L.dLG), Cp, last.x, last.w, gp(s, ow), gp(s, ob), TP, Cp, last.w, s.st)) return rc;
    if (int rc = linear_bwd_dx(s.F(L.dLG), Cp, data[ow], last.dx, last.w, TP, Cp, last.w, 0, s.st)) return rc;
    float* dZ = s.F(L.t1);
    for (int i = n_dec - 1; i >= 0; --i) {
        const HDec& d = dec[i];
        const DecIn in = dec_in(s, i);
        if (int rc = block_bwd_run(d, s, L.Zd[i], L.t0, L.dstat[i], L.t1, TP)) return rc;       // dY: what layer i + 1 left in t0
        if (int rc = linear_bwd_dw(dZ, d.out, in.x, in.w, gp(s, d.w), gp(s, d.b), TP, d.out, d.in, s.st)) return rc;
        if (int rc = linear_bwd_dx(dZ, d.out, data[d.w], in.dx, in.w, TP, d.out, d.in, 0, s.st)) return rc;
    }
    if (int rc = linear_bwd_dw(dEv, Ce, s.F(L.HID), D, gp(s, ew), gp(s, eb), s.B, Ce, D, s.st)) return rc;
    return linear_bwd_dx(dEv, Ce, data[ew], s.F(L.dHID), D, s.B, Ce, D, 0, s.st);
}

// chain kernel (one workgroup per event) + grouped weight-gradient launch: dY = d HID (masked) -> dX = d X[0]
int HeadPlan::encoder_bwd_fused(const HeadStep& s, const float* dY, float* dX) const {
    const HLayout& L = s.L;
    const int D = cfg.hidden_dim;
    EncFusedBwdArgs a{};
    a.dY = dY; a.dX = dX; a.lnp = s.F(L.lnp); a.B = s.B; a.S = s.S; a.H = cfg.heads; a.L = cfg.n_layers; a.gelu = cfg.gelu;
    a.drop_p = s.dp; a.seed = s.seed;
    EncWgradArgs w{};
    w.T = s.T; w.B = s.B; w.L = cfg.n_layers; w.lnp = s.F(L.lnp);
    int nj = 0, nt = 0;
    for (int l = 0; l < cfg.n_layers; ++l) {
        const HLayer& W = layers[l];
        const HLayBuf& q = L.lay[l];
        a.w[l] = enc_w(l); a.buf[l] = enc_buf(s, l);
        a.g[l] = EncLayerGrad{s.F(q.g_dqkv), s.F(q.g_dao), s.F(q.g_dhp), s.F(q.g_df)};
        w.job[nj++] = EncWgradJob{s.F(q.g_dqkv), 3 * D, s.F(L.X[l]), gp(s, W.win), gp(s, W.bin), 3 * D / 32};
        w.job[nj++] = EncWgradJob{s.F(q.g_dao), D, s.F(q.ctx), gp(s, W.wo), gp(s, W.bo), D / 32};
        w.job[nj++] = EncWgradJob{s.F(q.g_dhp), D, s.F(q.x1), gp(s, W.w1), gp(s, W.b1), D / 32};
        w.job[nj++] = EncWgradJob{s.F(q.g_df), D, s.F(q.hact), gp(s, W.w2), gp(s, W.b2), D / 32};
        nt += 3 * D / 32 + 3 * (D / 32);
        w.ln_dst[l][0] = gp(s, W.g1); w.ln_dst[l][1] = gp(s, W.be1); w.ln_dst[l][2] = gp(s, W.g2); w.ln_dst[l][3] = gp(s, W.be2);
    }
    w.n_jobs = nj; w.n_tiles = nt;
    if (s.frozen) { w.n_jobs = 0; w.n_tiles = 0; }      // the chain kernel alone: its weight-gradient operands and LayerNorm sums stay in the workspace
    return encoder_fused_bwd(a, w, s.st);
}

// post-norm layers, last to first: dX = d x_{l+1} on entry, d x_l on exit (in place)
int HeadPlan::encoder_bwd_post(const HeadStep& s, float* dX) const {
    const HLayout& L = s.L;
    const int D = cfg.hidden_dim, T = s.T, H = cfg.heads, hd = D / H;
    float *d1 = s.F(L.t3), *dR = s.F(L.t0), *dT = s.F(L.t1);
    for (int l = cfg.n_layers - 1; l >= 0; --l) {
        const HLayer& W = layers[l];
        const HLayBuf& q = L.lay[l];
        AddLnBwdArgs n2{dX, s.F(q.xh2), s.F(q.rstd2), data[W.g2], d1, dR, gp(s, W.g2), gp(s, W.be2), T, D, s.dp, s.seed, sid_enc(l, 3)};
        if (int rc = add_ln_bwd(n2, s.st)) return rc;                                   // d1 = d(x1) residual, dR = d(f)
        if (int rc = linear_bwd_dw(dR, D, s.F(q.hact), D, gp(s, W.w2), gp(s, W.b2), T, D, D, s.st)) return rc;
        if (int rc = linear_bwd_dx(dR, D, data[W.w2], dT, D, T, D, D, 0, s.st)) return rc;      // dT = d(hact)
        if (int rc = act_bwd(s.F(q.hpre), dT, dR, (long)T * D, cfg.gelu, s.dp, s.seed, sid_enc(l, 2), s.st)) return rc;   // dR = d(hpre)
        if (int rc = linear_bwd_dw(dR, D, s.F(q.x1), D, gp(s, W.w1), gp(s, W.b1), T, D, D, s.st)) return rc;
        if (int rc = linear_bwd_dx(dR, D, data[W.w1], d1, D, T, D, D, 1, s.st)) return rc;      // d1 += through FFN
        AddLnBwdArgs n1{d1, s.F(q.xh1), s.F(q.rstd1), data[W.g1], dX, dR, gp(s, W.g1), gp(s, W.be1), T, D, s.dp, s.seed, sid_enc(l, 1)};
        if (int rc = add_ln_bwd(n1, s.st)) return rc;                                   // dX = d(x_l) residual, dR = d(ao)
        if (int rc = linear_bwd_dw(dR, D, s.F(q.ctx), D, gp(s, W.wo), gp(s, W.bo), T, D, D, s.st)) return rc;
        if (int rc = linear_bwd_dx(dR, D, data[W.wo], dT, D, T, D, D, 0, s.st)) return rc;      // dT = d(ctx)
        AttnBwdArgs ab{s.F(q.qkv), s.F(q.probs), dT, dR, s.B, s.S, H, hd, s.dp, s.seed, sid_enc(l, 0)};       // dR = d(qkv) [T, 3D]
        if (int rc = attn_bwd(ab, s.st)) return rc;
        if (int rc = linear_bwd_dw(dR, 3 * D, s.F(L.X[l]), D, gp(s, W.win), gp(s, W.bin), T, 3 * D, D, s.st)) return rc;
        if (int rc = linear_bwd_dx(dR, 3 * D, data[W.win], dX, D, T, 3 * D, D, 1, s.st)) return rc;
    }
    return 0;
}

// pre-norm layers, last to first, dX in place: d x1 = dX + LN2'(d h2); d x_l = d x1 + LN1'(d h1); the dropped branches carry
// drop * gradient
int HeadPlan::encoder_bwd_pre(const HeadStep& s, float* dX) const {
    const HLayout& L = s.L;
    const int D = cfg.hidden_dim, T = s.T, H = cfg.heads, hd = D / H;
    const long n = (long)T * D;
    float *d1 = s.F(L.t3), *dR = s.F(L.t0), *dT = s.F(L.t1);
    float* dS = s.F(L.dHID);                                   // LayerNorm input gradients (dHID is consumed by now)
    for (int l = cfg.n_layers - 1; l >= 0; --l) {
        const HLayer& W = layers[l];
        const HLayBuf& q = L.lay[l];
        if (int rc = mul_drop(dX, dR, n, s.dp, s.seed, sid_enc(l, 3), s.st)) return rc;                         // dR = d f
        if (int rc = linear_bwd_dw(dR, D, s.F(q.hact), D, gp(s, W.w2), gp(s, W.b2), T, D, D, s.st)) return rc;
        if (int rc = linear_bwd_dx(dR, D, data[W.w2], dT, D, T, D, D, 0, s.st)) return rc;                  // dT = d hact
        if (int rc = act_bwd(s.F(q.hpre), dT, dR, n, cfg.gelu, s.dp, s.seed, sid_enc(l, 2), s.st)) return rc;   // dR = d hpre
        if (int rc = linear_bwd_dw(dR, D, s.F(q.h2), D, gp(s, W.w1), gp(s, W.b1), T, D, D, s.st)) return rc;
        if (int rc = linear_bwd_dx(dR, D, data[W.w1], dT, D, T, D, D, 0, s.st)) return rc;                  // dT = d h2
        AddLnBwdArgs n2{dT, s.F(q.xh2), s.F(q.rstd2), data[W.g2], dS, d1, gp(s, W.g2), gp(s, W.be2), T, D, 0.f, s.seed, sid_enc(l, 3)};
        if (int rc = add_ln_bwd(n2, s.st)) return rc;                                                       // dS = LN2 input gradient
        if (int rc = add_inplace(dX, dS, n, s.st)) return rc;                                               // dX = d x1
        if (int rc = mul_drop(dX, dR, n, s.dp, s.seed, sid_enc(l, 1), s.st)) return rc;                         // dR = d ao
        if (int rc = linear_bwd_dw(dR, D, s.F(q.ctx), D, gp(s, W.wo), gp(s, W.bo), T, D, D, s.st)) return rc;
        if (int rc = linear_bwd_dx(dR, D, data[W.wo], dT, D, T, D, D, 0, s.st)) return rc;                  // dT = d ctx
        AttnBwdArgs ab{s.F(q.qkv), s.F(q.probs), dT, dR, s.B, s.S, H, hd, s.dp, s.seed, sid_enc(l, 0)};     // dR = d qkv [T, 3D]
        if (int rc = attn_bwd(ab, s.st)) return rc;
        if (int rc = linear_bwd_dw(dR, 3 * D, s.F(q.h1), D, gp(s, W.win), gp(s, W.bin), T, 3 * D, D, s.st)) return rc;
        if (int rc = linear_bwd_dx(dR, 3 * D, data[W.win], dT, D, T, 3 * D, D, 0, s.st)) return rc;         // dT = d h1
        AddLnBwdArgs n1{dT, s.F(q.xh1), s.F(q.rstd1), data[W.g1], dS, d1, gp(s, W.g1), gp(s, W.be1), T, D, 0.f, s.seed, sid_enc(l, 1)};
        if (int rc = add_ln_bwd(n1, s.st)) return rc;
        if (int rc = add_inplace(dX, dS, n, s.st)) return rc;                                               // dX = d x_l
    }
    return 0;
}

// combined embedding: d X[0] -> token scatter -> LinearBlock -> Linear -> d_rows
int HeadPlan::embed_bwd(const HeadStep& s, const float* dX0, const float* rows, const int32_t* tok_row, float* d_rows) const {
    const HLayout& L = s.L;
    const int D = cfg.hidden_dim;
    if (int rc = scatter_tokens_bwd(dX0, tok_row, s.F(L.dC), s.B, s.S, D, s.st)) return rc;
    if (int rc = block_bwd_run(comb, s, L.Zc, L.dC, L.cstat, L.dZc, s.R)) return rc;
    if (int rc = linear_bwd_dw(s.F(L.dZc), D, rows, cfg.in_dim, gp(s, comb.w), gp(s, comb.b), s.R, D, cfg.in_dim, s.st)) return rc;
    return linear_bwd_dx(s.F(L.dZc), D, data[comb.w], d_rows, cfg.in_dim, s.R, D, cfg.in_dim, 0, s.st);
}

extern "C" {
int tcvn_head_create(const tcvn_head_cfg* cfg, tcvn_head** out) {
    if (!cfg || !out || cfg->n_dec < 0 || cfg->n_dec > 8 || cfg->hidden_dim % cfg->heads != 0) return -1;
    *out = new tcvn_head(*cfg);
    return 0;
}
void tcvn_head_destroy(tcvn_head* p) { delete p; }
int tcvn_head_num_slots(const tcvn_head* p) { return (int)p->plan.slots.size(); }
int tcvn_head_slot(const tcvn_head* p, int i, char* name, int cap, int64_t* numel, int* kind) {
    if (i < 0 || i >= (int)p->plan.slots.size()) return -1;
    const auto& s = p->plan.slots[i];
    if (name && cap > 0) { strncpy(name, s.name.c_str(), cap - 1); name[cap - 1] = 0; }
    if (numel) *numel = s.numel;
    if (kind) *kind = s.kind;
    return 0;
}
int tcvn_head_bind(tcvn_head* p, void* const* data, void* const* grad) { return p->plan.bind(data, grad); }
void tcvn_head_set_fused_encoder(tcvn_head* p, int on) { p->plan.fused_encoder = on != 0; }
int64_t tcvn_head_workspace_bytes(const tcvn_head* p, int batch, int max_prongs, int n_prongs) {
    HLayout L;
    p->plan.layout(batch, max_prongs, n_prongs, L);
    return L.total;
}
int tcvn_head_forward(tcvn_head* p, int batch, int max_prongs, int n_prongs, const float* rows, const int32_t* tok_row,
                      float* event_logits, float* prong_logits, void* ws, int64_t ws_bytes, int train, uint64_t seed, void* stream) {
    p->last_np = n_prongs; p->last_b = batch; p->last_p = max_prongs;
    return p->plan.forward(batch, max_prongs, n_prongs, rows, tok_row, event_logits, prong_logits, ws, ws_bytes, train, seed,
                           reinterpret_cast<hipStream_t>(stream));
}
int tcvn_head_forward_mc(tcvn_head* p, int batch, int max_prongs, int n_prongs, const float* rows, const int32_t* tok_row,
                         float* event_logits, float* prong_logits, void* ws, int64_t ws_bytes, uint64_t seed, void* stream) {
    p->last_np = n_prongs; p->last_b = batch; p->last_p = max_prongs;
    return p->plan.forward(batch, max_prongs, n_prongs, rows, tok_row, event_logits, prong_logits, ws, ws_bytes, 0, seed,
                           reinterpret_cast<hipStream_t>(stream), true);
}
/* stage entry points (forward only): see include/tcvn_hip.h */
int tcvn_head_embed(tcvn_head* p, int batch, int max_prongs, int n_prongs, const float* rows, const int32_t* tok_row, float* tokens,
                    void* ws, int64_t ws_bytes, int train, uint64_t seed, void* stream) {
    HeadStep s;
    if (int rc = p->plan.step(batch, max_prongs, n_prongs, ws, ws_bytes, train, seed, reinterpret_cast<hipStream_t>(stream), s)) return rc;
    if (int rc = p->plan.embed(s, rows, tok_row)) return rc;
    return permute_rows(s.F(s.L.X[0]), tokens, batch, s.S, p->plan.cfg.hidden_dim, 1, s.st);
}
int tcvn_head_encode(tcvn_head* p, int batch, int max_prongs, const float* tokens, const int32_t* tok_row, float* hidden, void* ws,
                     int64_t ws_bytes, int train, uint64_t seed, void* stream) {
    HeadStep s;
    if (int rc = p->plan.step(batch, max_prongs, 0, ws, ws_bytes, train, seed, reinterpret_cast<hipStream_t>(stream), s)) return rc;
    const int D = p->plan.cfg.hidden_dim;
    float* X0 = s.F(s.L.X[0]);
    if (int rc = permute_rows(tokens, X0, batch, s.S, D, 0, s.st)) return rc;          // [B,S,D] -> sequence-major rows
    if (int rc = mask_rows(X0, tok_row, X0, batch, s.S, D, s.st)) return rc;           // embeddings * sequence_mask (:69)
    if (int rc = p->plan.encode(s, tok_row)) return rc;
    p->last_np = 0; p->last_b = batch; p->last_p = max_prongs;
    TCVN_CHECK(hipMemcpyAsync(hidden, s.F(s.L.HID), (size_t)s.T * D * 4, hipMemcpyDeviceToDevice, s.st));
    return 0;
}
int tcvn_head_decode(tcvn_head* p, int batch, int max_prongs, const float* hidden, float* event_logits, float* prong_logits,
                     void* ws, int64_t ws_bytes, int train, uint64_t seed, void* stream) {
    HeadStep s;
    if (int rc = p->plan.step(batch, max_prongs, 0, ws, ws_bytes, train, seed, reinterpret_cast<hipStream_t>(stream), s)) return rc;
    TCVN_CHECK(hipMemcpyAsync(s.F(s.L.HID), hidden, (size_t)s.T * p->plan.cfg.hidden_dim * 4, hipMemcpyDeviceToDevice, s.st));
    return p->plan.decode(s, event_logits, prong_logits);
}

int tcvn_head_loss(tcvn_head* p, int batch, int max_prongs, const float* event_logits, const float* prong_logits,
                   const int64_t* event_targets, const int8_t* prong_targets, float* losses, float* accs, float* d_event_logits,
                   float* d_prong_logits, void* stream) {
    return p->plan.loss(batch, max_prongs, event_logits, prong_logits, event_targets, prong_targets, losses, accs, d_event_logits,
                        d_prong_logits, reinterpret_cast<hipStream_t>(stream));
}
int tcvn_head_forward_frozen(tcvn_head* p, int batch, int max_prongs, int n_prongs, const float* rows, const int32_t* tok_row,
                             float* event_logits, float* prong_logits, void* ws, int64_t ws_bytes, void* stream) {
    p->last_np = n_prongs; p->last_b = batch; p->last_p = max_prongs;
    return p->plan.forward_frozen(batch, max_prongs, n_prongs, rows, tok_row, event_logits, prong_logits, ws, ws_bytes,
                                  reinterpret_cast<hipStream_t>(stream));
}
int tcvn_head_input_gradient(tcvn_head* p, int batch, int max_prongs, int n_prongs, const float* rows, const int32_t* tok_row,
                             const float* d_event_logits, const float* d_prong_logits, float* d_rows, void* ws, int64_t ws_bytes,
                             void* stream) {
    return p->plan.input_gradient(batch, max_prongs, n_prongs, rows, tok_row, d_event_logits, d_prong_logits, d_rows, ws, ws_bytes,
                                  reinterpret_cast<hipStream_t>(stream));
}
int tcvn_head_backward(tcvn_head* p, int batch, int max_prongs, int n_prongs, const float* rows, const int32_t* tok_row,
                       const float* d_event_logits, const float* d_prong_logits, float* d_rows, void* ws, int64_t ws_bytes,
                       void* stream) {
    return p->plan.backward(batch, max_prongs, n_prongs, rows, tok_row, d_event_logits, d_prong_logits, d_rows, ws, ws_bytes,
                            reinterpret_cast<hipStream_t>(stream));
}
}

// Stand-alone row operators behind the holder modules' own forward() (LinearBlock, ProngDecoder, ProngTargetDecoder,
// DenseNet.output_block): forward only, fp32, caller-owned tensors.
extern "C" int tcvn_linear_forward(const float* x, int64_t ldx, const float* weight, const float* bias, float* y, int64_t ldy,
                                   int rows, int n_out, int n_in, void* stream) {
    if (!x || !weight || !y || rows < 0 || n_out <= 0 || n_in <= 0) return -1;
    if (rows == 0) return 0;
    return linear_fwd(x, ldx, weight, bias, y, ldy, rows, n_out, n_in, reinterpret_cast<hipStream_t>(stream));
}
// train: batch statistics and their running-stat update; draw: dropout is applied (a training call draws, an eval call does not, the
// Monte-Carlo dropout call runs on running statistics and draws).  save_mean_rstd may be NULL only where the caller says so (mc: an
// eval pass saves nothing)
static int rows_bn_prelu_forward(const float* x, int64_t ldx, int rows, int channels, const float* gamma, const float* beta,
                                 const float* slope, float* running_mean, float* running_var, float* y, int64_t ldy,
                                 float* save_mean_rstd, int train, bool draw, float drop_p, uint64_t seed, uint32_t stream_id, void* stream,
                                 bool need_save = true) {
    const bool no_norm = !gamma && !beta && !running_mean && !running_var;      // LinearBlock without BatchNorm1d (norm = Identity)
    if (!x || !y || rows <= 0 || channels <= 0) return -1;
    if (!no_norm && (!gamma || !beta || !running_mean || !running_var || (need_save && !save_mean_rstd))) return -1;
    RowsBnArgs r{};
    r.no_norm = no_norm ? 1 : 0;
    r.X = x; r.ldx = ldx; r.R = rows; r.C = channels; r.gamma = gamma; r.beta = beta; r.slope = slope;      // slope NULL: ReLU
    r.running_mean = running_mean; r.running_var = running_var; r.Y = y; r.ldy = ldy;
    r.save_mean = save_mean_rstd; r.save_rstd = save_mean_rstd ? save_mean_rstd + channels : nullptr; r.train = train; r.eps = kEps; r.momentum = kMom;
    r.drop_p = draw ? drop_p : 0.f; r.seed = seed; r.stream_id = stream_id;
    return rows_bn_fwd(r, reinterpret_cast<hipStream_t>(stream));
}
extern "C" int tcvn_rows_bn_prelu_forward(const float* x, int64_t ldx, int rows, int channels, const float* gamma, const float* beta,
                                          const float* slope, float* running_mean, float* running_var, float* y, int64_t ldy,
                                          float* save_mean_rstd, int train, float drop_p, uint64_t seed, uint32_t stream_id,
                                          void* stream) {
    return rows_bn_prelu_forward(x, ldx, rows, channels, gamma, beta, slope, running_mean, running_var, y, ldy, save_mean_rstd, train,
                                 train != 0, drop_p, seed, stream_id, stream);
}
extern "C" int tcvn_rows_bn_prelu_forward_mc(const float* x, int64_t ldx, int rows, int channels, const float* gamma, const float* beta,
                                             const float* slope, const float* running_mean, const float* running_var, float* y,
                                             int64_t ldy, float drop_p, uint64_t seed, uint32_t stream_id, void* stream) {
    if (!(drop_p >= 0.f && drop_p < 1.f)) { fprintf(stderr, "tcvn: rows_bn_prelu_forward_mc: drop_p %g outside [0, 1)\n", (double)drop_p); return -1; }
    return rows_bn_prelu_forward(x, ldx, rows, channels, gamma, beta, slope, const_cast<float*>(running_mean),
                                 const_cast<float*>(running_var), y, ldy, nullptr, 0, true, drop_p, seed, stream_id, stream, false);
}

// Backward of the two row operators (smart-feature MLP, layers/prong_feature_embedding.py:36-78: the only LinearBlocks outside the head plan)
extern "C" int tcvn_linear_backward(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* weight, float* dx, int64_t lddx,
                                    float* dweight, float* dbias, int rows, int n_out, int n_in, void* stream) {
    if (!dy || !x || !weight || rows <= 0 || n_out <= 0 || n_in <= 0) return -1;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    int rc;
    if ((dweight || dbias) && (rc = linear_bwd_dw(dy, lddy, x, ldx, dweight, dbias, rows, n_out, n_in, st))) return rc;
    if (dx && (rc = linear_bwd_dx(dy, lddy, weight, dx, lddx, rows, n_out, n_in, 0, st))) return rc;
    return 0;
}
extern "C" int tcvn_rows_bn_prelu_backward(const float* x, int64_t ldx, const float* dy, int64_t lddy, int rows, int channels,
                                           const float* gamma, const float* beta, const float* slope, const float* save_mean_rstd,
                                           float* dx, int64_t lddx, float* dgamma, float* dbeta, float* dslope, float drop_p,
                                           uint64_t seed, uint32_t stream_id, void* stream) {
    const bool no_norm = !gamma && !beta && !dgamma && !dbeta;                  // LinearBlock without BatchNorm1d
    if (!x || !dy || !dx || rows <= 0 || channels <= 0 || (slope != nullptr) != (dslope != nullptr)) return -1;
    if (!no_norm && (!gamma || !beta || !save_mean_rstd || !dgamma || !dbeta)) return -1;
    RowsBnBwdArgs r{};
    r.no_norm = no_norm ? 1 : 0;
    r.X = x; r.ldx = ldx; r.dY = dy; r.lddy = lddy; r.R = rows; r.C = channels; r.gamma = gamma; r.beta = beta; r.slope = slope;
    r.save_mean = save_mean_rstd; r.save_rstd = save_mean_rstd ? save_mean_rstd + channels : nullptr; r.dX = dx; r.lddx = lddx;
    r.dgamma = dgamma; r.dbeta = dbeta; r.dslope = dslope; r.drop_p = drop_p; r.seed = seed; r.stream_id = stream_id;
    return rows_bn_bwd(r, reinterpret_cast<hipStream_t>(stream));
}

// Stand-alone softmax focal loss of one logit matrix (reference: NeutrinoFullBaseTrainer.loss, :148-160)
extern "C" int tcvn_focal_loss(const float* logits, const int64_t* targets, int rows, int classes, float gamma, float weight,
                               float* d_logits, float* out2, void* stream) {
    return focal_i64(logits, targets, rows, classes, gamma, weight, d_logits, out2, reinterpret_cast<hipStream_t>(stream));
}
