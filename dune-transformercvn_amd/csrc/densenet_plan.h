// DenseNet plan: slot table, geometry, workspace layout, forward/backward drivers.
#pragma once
#include <string>
#include <vector>

#include "../../include/tcvn_hip.h"
#include "tcvn_ops.h"

namespace tcvn {

struct BnSlots { int w = -1, b = -1, rm = -1, rv = -1, nbt = -1, C = 0, id = -1; };
struct LayerSlots { BnSlots n1, n2; int a1, w1, b1, a2, w2, b2, cin; };
struct BlockGeom {
    int H, W, C0, L, Ctot, ld;        // ld: channel pitch of the concat / gradient buffers (bf16: a multiple of 64 = whole 128-B lines per row)
    int ldp;                          // channel pitch of the pooled transition input XP (Ctot rounded up to 8: also its GEMM's K extent)
    std::vector<LayerSlots> layers;
    bool has_trans = false;
    BnSlots tn; int ta = -1, tw = -1, tb = -1;
};
struct WkEntry { int slot, N, Cin, taps, transpose, rows, Kp, frag; long off; };

struct Layout {
    long img, c0, bstat0, part, tabs, F, Z, head_stat, wk, fwd_end, total;
    std::vector<long> D, bstatD;
    std::vector<std::vector<long>> Y, bstatY, YA;     // YA: activated bf16 copies of Y (bf16 mode)
    std::vector<std::vector<long>> EY3;               // bf16 mode: [pixels][32] eff rows of a layer's 3x3 output gradient (data gradient -> weight gradient)
    std::vector<std::vector<long>> KM;                // bf16 mode with dropout: one keep word per pixel and dense layer (3x3 output dropout)
    long zeros, ey, ey2, slab;
    long isum_bytes = 0;                 // link-free BatchNorm statistics (bn_lf.h): fixed-point accumulators, directly behind the zero page
    std::vector<long> isumD;             //   per dense block: [ld][2] int64 (sum, sum of squares) of the concat buffer's channels
    std::vector<std::vector<long>> isumY;    //   per dense layer: [128][2] of the bottleneck map
    long slab1;                          // bf16 mode: slabs of the fused 1x1 backward kernel (main stream; `slab` may be in use by the 3x3 weight gradient
                                         // on the side stream when tcvn_backward_overlap is on)
    long sact;                           // bf16 dense stem: activity bitmap of the conv0 output (stem_mark), -1 when unused
    long sidx;                           // sparse-stem bucket index (stem_sparse.hip), -1 when the plan cannot use it
    long own;                            // dense stem: duplicate-coordinate record (PixelOwners: scatter_pixels writes it, the hit-list weight gradient reads it)
    std::vector<std::vector<long>> XA;   // activated bf16 copies of the 1x1-conv inputs (per layer, -1 if absent)
    std::vector<long> XP;                // pooled activated transition inputs (-1 if absent)
    // backward
    long du, du0, pq0, pqY, gwk, bpart, dF, dZ, zero_end;
    std::vector<long> G, pqD;
};

// What the last forward did with one dense layer / with the stem.  DenseNetPlan::layer_path decides a layer's record before the layer's first
// launch; the forward launches, the backward and tap() read it and never re-derive it.
struct LayerPath {
    bool fuse_ya = false;      // eval pass: the 1x1 GEMM's epilogue wrote the activated bottleneck map YA only (no raw Y exists)
    bool raw1x1 = false;       // the fused 1x1 kernel ran on the raw concat buffer: no activated copy XA of the layer's input exists, backward must
                               // take the fused 1x1 kernel (which rebuilds it from x)
    bool act_fused = false;    // the 3x3 pair kernel ran on the RAW bottleneck map (activation applied in LDS, ConvFwdArgs::act_fused): no activated
                               // copy YA exists, the weight gradient does the same
    bool lf2 = false;          // the 3x3 pair kernel derived norm2's table itself (no link launch in front of it)
    bool out_isum = false;     // the 3x3 pair kernel added the new channels' statistics to the block's fixed-point accumulators (link-free producer)
    bool keep_stored = false;  // train mode: the 3x3 pair kernel stored the dropout keep words it drew (Layout::KM) for the backward kernels
};
struct StemPath {
    bool sparse = false;       // the sparse-aware stem ran: no dense map / conv0 output exists (backward must match)
    bool act_skip = false;     // the dense stem skipped the conv0-output rows no hit reaches (backward must use the same bitmap)
};
struct Tab { float* sc; float* sh; };      // (scale, shift) table of one BatchNorm layer
// Channels [c0, c0 + n) of a concat buffer whose statistics no BatchNorm table covers yet: `nblk` partial rows of `ld` channels, or (isum) in the block's accumulators
struct FreshStats { int c0, n, nblk, ld; bool isum; };
struct Step {                  // values shared by the pieces of one forward or backward call
    char* ws; const Layout& L; hipStream_t st; int n; bool train; uint64_t seed;
    double* part; bool lf_on;  // statistics partials (Layout::part forward, Layout::bpart backward); forward: link-free BatchNorm statistics (bn_lf.h)
    bool side_on; int seq; bool side_busy;      // backward: weight gradients on the side stream; parity of the EY buffer / tail half (reset by drain);
                                                // work on the side stream that `st` has not waited for
    bool draw = false;         // forward, train == false: the dropout sites draw their masks (Monte-Carlo dropout); everything else is the eval pass
    // Frozen pass (hit gradients): the eval pass -- running statistics, no dropout, no noise -- in a workspace laid out with backward and on
    // the layer paths that keep what a backward needs (dense stem, raw bottleneck maps).  Its backward (input_gradient) is the data-gradient
    // chain alone: no BatchNorm link (P = Q = 0), no weight gradient, dropout probability 0, nothing added to a bound grad pointer.
    bool frozen = false;
    float drop_p(float cfg_p) const { return (train || draw) && !frozen ? cfg_p : 0.f; }      // the effective dropout probability of this call
};

bool backward_overlap_enabled();
void set_backward_overlap(int on);

struct DenseNetPlan {
    tcvn_densenet_cfg cfg;
    int esz, Hc, Wc, Cf, n_bn = 0;
    std::vector<Slot> slots;
    std::vector<float*> data, grad;
    std::vector<BlockGeom> blocks;
    int s_w0, s_b0, s_a0, s_af, s_wl, s_al;
    BnSlots n0, nf, nl;
    std::vector<WkEntry> wk_cache;
    bool bound = false;
    bool fast1_ok(int cin) const;    // 1x1 bottleneck conv on the bf16 NT/TN GEMMs
    bool fastt_ok(int Ctot) const;   // transition conv on the bf16 NT/TN GEMMs
    bool fast3x3 = false;            // bf16 padded-tile 3x3 kernels in use (decided at bind time)
    // device descriptor table (pack + eval BN descriptors)
    char* d_desc = nullptr; size_t desc_cap = 0; std::vector<char> h_desc;
    char* desc_ws = nullptr; long desc_total = 0; int n_pack = 0, n_bneval = 0;
    uint64_t last_seed = 0; int last_n = 0;
    const int32_t* last_coords = nullptr; long last_nnz = 0;     // COO list of the last forward (sparse stem weight gradient)
    const float* last_values = nullptr; int last_value_mode = 0; float last_noise = 0.f;
    const char* last_ws = nullptr; bool last_eval = false;       // workspace of the last forward, and whether it ran on running statistics: what a
                                                                 // Monte-Carlo dropout sample may resume from (null: nothing)
    bool last_frozen = false;                                    // the last forward was a frozen one: input_gradient may follow, backward and a
                                                                 // Monte-Carlo resume may not
    std::vector<std::vector<LayerPath>> path;    // [block][layer] of the last forward
    StemPath stem_path;
    bool sparse_stem_possible() const;   // plan-level condition (bf16, 3 -> 64 channels); the hit count decides per call
    // weight-gradient side stream of backward (3x3 and 1x1 weight gradients run beside the data-gradient chain)
    hipStream_t side_st = nullptr; hipEvent_t ev_fork_a = nullptr, ev_fork_b = nullptr, ev_done[2] = {nullptr, nullptr}, ev_drain = nullptr;
    int ensure_side();
    char* d_undesc = nullptr; std::vector<char> h_undesc; char* undesc_ws = nullptr; long undesc_total = 0; int n_unpack = 0;

    explicit DenseNetPlan(const tcvn_densenet_cfg& c);
    ~DenseNetPlan();
    int add_slot(const std::string& name, long numel, int kind);
    BnSlots add_bn(const std::string& p, int c);
    void layout(int n, bool bwd, Layout& L) const;
    void layout_bwd(int n, long start, long maxY, Layout& L) const;
    long tab_floats() const;
    long tab_off(const BnSlots& s) const;
    long wk_bytes() const;
    std::vector<WkEntry> wk_list() const;
    const WkEntry& wk_find(int slot, int transpose, int frag = 0) const;
    const void* wk_frag(const char* ws, const Layout& L, int slot, int transpose) const;   // null when absent
    int bind(void* const* d, void* const* g);
    int upload_descs(char* ws, const Layout& L, hipStream_t st);
    int forward(int n, const int32_t* coords, const float* values, long nnz, int log_pixels, float noise_std, float* out,
                long out_ld, char* ws, long ws_bytes, int train, uint64_t seed, hipStream_t st, bool draw = false, bool resume = false,
                bool frozen = false);
    int backward(int n, const float* d_out, long d_out_ld, char* ws, long ws_bytes, hipStream_t st, int bi_hi = -1, int bi_lo = 0);
    // data-only backward of the last frozen forward: d_out -> d_values [nnz][in_ch] at the hits of that forward's list
    int input_gradient(int n, const float* d_out, long d_out_ld, float* d_values, char* ws, long ws_bytes, hipStream_t st);
    // the pieces of forward and of backward, each in launch order
    int fwd_stem(const Step& s, const int32_t* coords, const float* values, long nnz, int log_pixels, float noise_std, FreshStats& fr);
    int fwd_layer(const Step& s, int bi, int l, FreshStats& fr);
    int fwd_transition(const Step& s, int bi, FreshStats& fr);      // the last block: final_norm + global average instead
    int fwd_output(const Step& s, float* out, long out_ld) const;
    LayerPath layer_path(const Step& s, int bi, int l, const ConvFwdArgs& c3, Fwd1x1Args& f1) const;
    int link(const Step& s, const BnSlots& bn, int nblk, int part_ld, int c_new0, int n_new, double* bstat, long count,
             const long long* isum = nullptr, long isum_stride = 0) const;
    int link_fresh(const Step& s, const BnSlots& bn, int bi, const FreshStats& fr) const;
    LfLink lf_link(const Step& s, const BnSlots& bn, const long long* isum, long rep_stride, int c_new0, int n_new, double* bstat, long count) const;
    int bwd_output(const Step& s, const float* d_out, long d_out_ld) const;
    int bwd_transition(Step& s, int bi) const;                      // the last block: final_norm + global average instead
    int bwd_layer(Step& s, int bi, int l) const;
    int bwd_stem(const Step& s) const;
    int bwd_link(const Step& s, const BnSlots& bn, int nblk, const double* bstat, long count, float* P, float* Q, int acc, int a_slot) const;
    int drain(Step& s) const;                                       // `st` waits for everything enqueued on the side stream
    float* gw_of(const Step& s, int slot) const;                    // kernel-layout weight gradient of a conv weight slot
    // One argument builder per launch kind: every site that launches the kernel, asks a predicate about the launch or regenerates its operand in
    // backward (ConvWgradArgs::fa) starts from these; per-step fields (part, nblk, dropout, seed, act_fused / Aact, lf, isum_out, keep_out) are the caller's
    Tab tab(char* ws, const Layout& L, const BnSlots& bn) const;
    ConvFwdArgs conv0_args(const Step& s) const, trans_args(const Step& s, int bi) const;
    ConvFwdArgs conv1_args(const Step& s, int bi, int l) const, conv3_args(const Step& s, int bi, int l) const;   // 1x1 on the generic kernels; 3x3 (bf16: Aact = raw map Y)
    StemSparseArgs stem_sparse_args(const Step& s, const int32_t* coords, const float* values, long nnz, int value_mode, float noise_std) const;
    // Arguments of the fused 1x1 backward kernel for block bi, layer l (PY / QY / part left to the caller) -- the ONE place that decides whether a
    // layer's backward can take it: the forward asks before it drops the activated copy XA, the backward fills its launch from the same function
    bool bwd1x1_fill(int bi, int l, long M, char* ws, const Layout& L, Bwd1x1Args& fa) const;
    std::vector<int> unpack_first;   // first unpack descriptor of every block (+ total): partial backward calls unpack their own blocks
    int tap(int n, const char* name, long* off, int* tn, int* th, int* tw, int* tc, int* tld, int* tes) const;
};

}  // namespace tcvn
