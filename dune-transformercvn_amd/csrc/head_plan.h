// Token-path plan: slot table, workspace layout, forward / loss / backward drivers.
#pragma once
#include <string>
#include <vector>

#include "../../include/tcvn_hip.h"
#include "tcvn_common.h"
#include "tcvn_rows.h"
#include "tcvn_encoder.h"

namespace tcvn {

struct HBn { int w = -1, b = -1, rm = -1, rv = -1; };
struct HLayer { int win, bin, wo, bo, w1, b1, w2, b2, g1, be1, g2, be2; };
// One LinearBlock (Linear - BatchNorm1d | Identity - PReLU | ReLU - Dropout): the combined embedding and every prong decoder layer.
// b = -1: Linear without bias; a = -1: ReLU; n.w = -1: no BatchNorm1d.  sid / drop: dropout stream id, and whether the block has a Dropout.
struct HDec { int w, b = -1, a = -1, in, out; HBn n; uint32_t sid = 0; bool drop = false; };
struct HLayBuf { long qkv, probs, ctx, ao, xh1, rstd1, x1, hpre, hact, f, xh2, rstd2, g_dqkv, g_dao, g_dhp, g_df,
                 h1, h2; };     // h1 / h2: LayerNorm outputs of the pre-norm variant (transformer_norm_first)
struct HLayout {
    long Zc, C, cstat, HID, LG, dEv, dPr, lossbuf, dLG, t0, t1, t2, t3, dHID, dC, dZc, lnp, total;
    std::vector<long> X, Zd, Ad, dstat;
    std::vector<HLayBuf> lay;
};

// Everything one call works on, built once by HeadPlan::step: shape, workspace, dropout and stream.
struct HeadStep {
    int B, P, nP, S, T, R, TP;       // S = 1 + P tokens a sequence, T = S * B token rows, R = B + nP embedding rows, TP = P * B prong rows
    char* ws; HLayout L;
    int train; uint64_t seed; float dp; hipStream_t st;      // dp: the effective dropout probability (0 in eval mode, unless the call draws)
    bool draw = false;               // train == 0: the dropout sites draw their masks (Monte-Carlo dropout); everything else is the eval pass
    bool frozen = false;             // backward of a frozen forward (hit gradients): dp = 0, running-statistics LinearBlock backward, no parameter gradient
    float* F(long off) const { return reinterpret_cast<float*>(ws + off); }
};
enum class EncPath { FUSED, POST_NORM, PRE_NORM };
struct DecIn { const float* x; float* dx; int w; };         // input rows of a decoder layer, where their gradient goes, and their width

// Workspace offsets handed out in order, each rounded up to 256 bytes
struct Bump {
    long off = 0;
    long take(long bytes) { long o = off; off += round_up(bytes, 256); return o; }
};

struct HeadPlan {
    tcvn_head_cfg cfg;
    std::vector<Slot> slots;
    std::vector<float*> data, grad;
    HDec comb;                      // combined embedding: in_dim -> hidden_dim, over the event rows and the packed prong rows
    int ew, eb, ow, ob, dec_width;
    std::vector<HLayer> layers;
    std::vector<HDec> dec;
    bool bound = false;
    bool fused_encoder = true;     // encoder_fused.hip when the shape allows (tcvn_head_set_fused_encoder(p, 0): unfused kernels, for A/B tests)
    uint64_t last_seed = 0;
    // workspace and (B, P, nP) of the last forward when it was a frozen one, else null: step() drops the note before anything writes a
    // workspace (a forward that fails midway, a stage entry, a scan), forward_frozen sets it when it has come through
    mutable const void* last_frozen_ws = nullptr; int last_frozen_shape[3] = {0, 0, 0};

    explicit HeadPlan(const tcvn_head_cfg& c);
    int add_slot(const std::string& name, long numel, int kind);
    HBn add_bn(const std::string& p, int c);
    int bind(void* const* d, void* const* g);
    void layout(int B, int P, int nP, HLayout& L) const;
    int step(int B, int P, int nP, void* ws, long ws_bytes, int train, uint64_t seed, hipStream_t st, HeadStep& s, bool draw = false,
             bool keep_note = false) const;
    EncPath enc_path(int S) const;
    // launch arguments that forward and backward must agree on
    EncLayerW enc_w(int l) const;  EncLayerBuf enc_buf(const HeadStep& s, int l) const;
    RowsBnArgs block_fwd(const HDec& d, const HeadStep& s, long X, long Y, long stat, int rows) const;
    RowsBnBwdArgs block_bwd(const HDec& d, const HeadStep& s, long X, long dY, long stat, long dX, int rows) const;
    int block_bwd_run(const HDec& d, const HeadStep& s, long X, long dY, long stat, long dX, int rows) const;
    float* gp(const HeadStep& s, int slot) const { return s.frozen || slot < 0 ? nullptr : grad[slot]; }      // where a parameter gradient goes (frozen: nowhere)
    DecIn dec_in(const HeadStep& s, int i) const;
    int embed(const HeadStep& s, const float* rows, const int32_t* tok_row) const;
    int encode(const HeadStep& s, const int32_t* tok_row) const, encode_post(const HeadStep& s, const int32_t* tok_row) const,
        encode_pre(const HeadStep& s, const int32_t* tok_row) const;
    int decode(const HeadStep& s, float* ev_logits, float* pr_logits) const;
    int forward(int B, int P, int nP, const float* rows, const int32_t* tok_row, float* ev_logits, float* pr_logits, void* ws,
                long ws_bytes, int train, uint64_t seed, hipStream_t st, bool draw = false);
    int loss(int B, int P, const float* ev_logits, const float* pr_logits, const int64_t* et, const int8_t* pt, float* losses,
             float* accs, float* dEv, float* dPr, hipStream_t st);
    int backward(int B, int P, int nP, const float* rows, const int32_t* tok_row, const float* dEv, const float* dPr, float* d_rows,
                 void* ws, long ws_bytes, hipStream_t st);
    int forward_frozen(int B, int P, int nP, const float* rows, const int32_t* tok_row, float* ev_logits, float* pr_logits, void* ws,
                       long ws_bytes, hipStream_t st);
    int input_gradient(int B, int P, int nP, const float* rows, const int32_t* tok_row, const float* dEv, const float* dPr, float* d_rows,
                       void* ws, long ws_bytes, hipStream_t st);
    int backward_chain(const HeadStep& s, const float* rows, const int32_t* tok_row, const float* dEv, const float* dPr, float* d_rows) const;
    int decoders_bwd(const HeadStep& s, const float* dEv, const float* dPr) const;
    int encoder_bwd_fused(const HeadStep& s, const float* dY, float* dX) const;      // d HID (masked) -> d X[0]
    int encoder_bwd_post(const HeadStep& s, float* dX) const, encoder_bwd_pre(const HeadStep& s, float* dX) const;      // in place
    int embed_bwd(const HeadStep& s, const float* dX0, const float* rows, const int32_t* tok_row, float* d_rows) const;
};

}  // namespace tcvn

// The handle of the C ABI (head.hip: plan, stages, loss, backward; head_explain.hip: the explanation scans)
struct tcvn_head {
    tcvn::HeadPlan plan;
    int last_np = 0, last_b = 0, last_p = -1;      // shape of the last forward / encode: what tcvn_head_attention may export
    explicit tcvn_head(const tcvn_head_cfg& c) : plan(c) {}
};
