// Token-path explanation scans (forward only): attention export, leave-one-prong-out, prong Shapley values and the token-path pass of
// the occlusion scan.  Every scan sends passes of variant sequences through HeadPlan::encode / decode with eval arithmetic, in a head
// workspace of its own: what the last forward left for backward() and tcvn_head_attention stays as it is.
#include <vector>

#include "../../include/tcvn_hip.h"
#include "head_plan.h"
#include "tcvn_explain.h"
#include "tcvn_occlude.h"
#include "tcvn_shapley.h"

using namespace tcvn;

namespace {
// What every scan's workspace ends in: vrow [cap][1 + P] and the head workspace of cap sequences
struct PassLayout { long vrow, head; };
PassLayout take_pass(Bump& b, const HeadPlan& plan, long cap, int P) {
    PassLayout o;
    o.vrow = b.take(cap * (1 + P) * 4);
    HLayout L;
    plan.layout((int)cap, P, 0, L);
    o.head = b.take(L.total);
    return o;
}
// One pass of n variant sequences in the workspace w: gather(X0 [S*n][D], vrow [n][S]) fills the tokens and their validity, then the
// encoder and the decoders run on them (a NULL logits pointer skips that decoder).
template <class Gather>
int run_pass(const HeadPlan& plan, int n, int P, char* w, long ws_bytes, const PassLayout& at, hipStream_t st, Gather gather,
             float* ev_logits, float* pr_logits) {
    HeadStep s;
    if (int rc = plan.step(n, P, 0, w + at.head, ws_bytes - at.head, 0, 0, st, s)) return rc;
    int* vrow = reinterpret_cast<int*>(w + at.vrow);
    if (int rc = gather(s.F(s.L.X[0]), vrow)) return rc;
    if (int rc = plan.encode(s, vrow)) return rc;
    return plan.decode(s, ev_logits, pr_logits);
}
// The variant list of a scan over prongs depends on the mask: tok_row [B][S] comes back to the host (a few KB, one synchronisation)
int read_tok_row(const int32_t* tok_row, int B, int S, hipStream_t st, std::vector<int32_t>& tr) {
    tr.assign((size_t)B * S, 0);
    TCVN_CHECK(hipMemcpyAsync(tr.data(), tok_row, tr.size() * 4, hipMemcpyDeviceToHost, st));
    TCVN_CHECK(hipStreamSynchronize(st));
    return 0;
}

// Workspace of the leave-one-prong-out scan: job list, slot -> job map, the logits of every job, and one pass (at most
// TCVN_LOO_MAX_PASS sequences).
struct LooLayout { long jobs, src, lg, total; PassLayout pass; int cap; };
void loo_layout(const HeadPlan& plan, int B, int P, LooLayout& o) {
    Bump b;
    const long slots = (long)B * (1 + P);
    o.cap = (int)(slots < TCVN_LOO_MAX_PASS ? slots : TCVN_LOO_MAX_PASS);
    o.jobs = b.take(slots * 4); o.src = b.take(slots * 4); o.lg = b.take(slots * plan.cfg.event_classes * 4);
    o.pass = take_pass(b, plan, o.cap, P);
    o.total = b.off;
}
// Prong Shapley scan.  The per-event table (ShapTable, tcvn_shapley.h) as the host builds it from tok_row: event b has n[b] valid prong
// slots (vmask), runs exactly when n <= max_exact, and owns the coalitions offsets[b] .. offsets[b+1]-1: 2^n of them, or empty + full +
// the M (n-1) proper prefixes of its permutations.
struct ShapHost { std::vector<int64_t> offsets, vmask; std::vector<int32_t> n, exact; };
bool shap_shape_ok(int batch, int max_prongs, int max_exact, int samples) {
    return batch > 0 && batch <= 65535 && max_prongs >= 0 && max_prongs <= 63 && max_exact >= 0 && max_exact <= TCVN_SHAP_MAX_EXACT &&
           samples >= 1;
}
long shap_jobs(int n, int max_exact, int M) { return n <= max_exact ? 1L << n : 2 + (long)M * (n - 1); }
int shap_read_table(const int32_t* tok_row, int B, int S, int max_exact, int M, hipStream_t st, ShapHost& h) {
    std::vector<int32_t> tr;
    if (int rc = read_tok_row(tok_row, B, S, st, tr)) return rc;
    h.offsets.assign(B + 1, 0); h.vmask.assign(B, 0); h.n.assign(B, 0); h.exact.assign(B, 0);
    for (int b = 0; b < B; ++b) {
        for (int s = 1; s < S; ++s)
            if (tr[(size_t)b * S + s] >= 0) { h.vmask[b] |= (int64_t)1 << (s - 1); ++h.n[b]; }
        h.exact[b] = h.n[b] <= max_exact;
        h.offsets[b + 1] = h.offsets[b] + shap_jobs(h.n[b], max_exact, M);
    }
    return 0;
}
// Workspace: the table's n / vmask, the inverse permutations, the fp64 values of as many coalitions as any mask of this shape can have
// (the size is asked for before the mask is known), and one pass (at most TCVN_SHAP_MAX_PASS sequences).
struct ShapLayout { long n, vmask, pos, values, total; PassLayout pass; long cap; };
void shap_layout(const HeadPlan& plan, int B, int P, int max_exact, int M, ShapLayout& o) {
    Bump b;
    long per_event = 1L << (P < max_exact ? P : max_exact);
    if (P > max_exact && shap_jobs(P, max_exact, M) > per_event) per_event = shap_jobs(P, max_exact, M);
    const long jmax = per_event * B;
    o.cap = jmax < TCVN_SHAP_MAX_PASS ? jmax : TCVN_SHAP_MAX_PASS;
    o.n = b.take((long)B * 4); o.vmask = b.take((long)B * 8); o.pos = b.take((long)B * M * (P > 0 ? P : 1) * 4);
    o.values = b.take(jmax * plan.cfg.event_classes * 8);
    o.pass = take_pass(b, plan, o.cap, P);
    o.total = b.off;
}
// Workspace of one pass of the occlusion scan (at most TCVN_OCC_MAX_PASS variants): variant rows, their combined embedding as one-token
// sequences (E: the Zc / C / cstat / X[0] part of a head layout) and the pass of the variant sequences.
struct OccHeadLayout { long vrows, ident, total; HLayout E; PassLayout pass; };
void occ_head_layout(const HeadPlan& plan, int P, OccHeadLayout& o) {
    Bump b;
    const long cap = TCVN_OCC_MAX_PASS, D = plan.cfg.hidden_dim;
    o.vrows = b.take(cap * plan.cfg.in_dim * 4); o.ident = b.take(cap * 4);
    o.E.Zc = b.take(cap * D * 4); o.E.C = b.take(cap * D * 4); o.E.cstat = b.take(2 * D * 4);
    o.E.X.assign(1, b.take(cap * D * 4));
    o.pass = take_pass(b, plan, cap, P);
    o.total = b.off;
}
}  // namespace

extern "C" {
/* see include/tcvn_hip.h */
int tcvn_head_attention(tcvn_head* p, int batch, int max_prongs, const int32_t* tok_row, const void* ws, int64_t ws_bytes,
                        float* weights, void* stream) {
    if (!p || !tok_row || !ws || !weights || batch <= 0 || max_prongs < 0 || 1 + max_prongs > 64) {
        fprintf(stderr, "tcvn: head_attention: bad argument (NULL pointer, batch < 1 or more than 64 tokens)\n");
        return -1;
    }
    if (batch != p->last_b || max_prongs != p->last_p) {
        fprintf(stderr, "tcvn: head_attention: no forward / encode of shape (batch %d, max_prongs %d) precedes this call\n", batch, max_prongs);
        return -15;
    }
    HLayout L;
    p->plan.layout(batch, max_prongs, p->last_np, L);
    if (ws_bytes < L.total) {
        fprintf(stderr, "tcvn: head_attention: workspace of %lld bytes, the forward's has %ld\n", (long long)ws_bytes, L.total);
        return -12;
    }
    const int nl = p->plan.cfg.n_layers;
    if (nl < 1) { fprintf(stderr, "tcvn: head_attention: the encoder has no layer\n"); return -1; }
    const long stride = nl > 1 ? L.lay[1].probs - L.lay[0].probs : 0;       // every layer takes the same buffers: constant stride
    for (int l = 1; l < nl; ++l)
        if (L.lay[l].probs - L.lay[l - 1].probs != stride) return -16;
    return attn_export(reinterpret_cast<const char*>(ws), L.lay[0].probs, stride, tok_row, weights, nl, batch, p->plan.cfg.heads,
                       1 + max_prongs, reinterpret_cast<hipStream_t>(stream));
}
int64_t tcvn_head_leave_one_out_workspace_bytes(const tcvn_head* p, int batch, int max_prongs) {
    if (!p || batch <= 0 || max_prongs < 0 || 1 + max_prongs > 64) return -1;
    LooLayout o;
    loo_layout(p->plan, batch, max_prongs, o);
    return o.total;
}
int tcvn_head_leave_one_out(tcvn_head* p, int batch, int max_prongs, const float* tokens, const int32_t* tok_row, float* event_logits,
                            float* loo, void* ws, int64_t ws_bytes, void* stream) {
    if (!p || !tokens || !tok_row || !event_logits || !ws || (max_prongs > 0 && !loo) || batch <= 0 || max_prongs < 0 ||
        1 + max_prongs > 64) {
        fprintf(stderr, "tcvn: head_leave_one_out: bad argument (NULL pointer, batch < 1 or more than 64 tokens)\n");
        return -1;
    }
    LooLayout o;
    loo_layout(p->plan, batch, max_prongs, o);
    if (ws_bytes < o.total) {
        fprintf(stderr, "tcvn: head_leave_one_out: workspace of %lld bytes, %ld needed\n", (long long)ws_bytes, o.total);
        return -12;
    }
    if (!p->plan.bound) { fprintf(stderr, "tcvn: head_leave_one_out: parameters are not bound\n"); return -11; }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int B = batch, P = max_prongs, S = 1 + P, D = p->plan.cfg.hidden_dim, Ce = p->plan.cfg.event_classes;
    char* w = reinterpret_cast<char*>(ws);
    std::vector<int32_t> tr, jobs, src((size_t)B * S);
    if (int rc = read_tok_row(tok_row, B, S, st, tr)) return rc;
    for (int b = 0; b < B; ++b) { jobs.push_back(b * S); src[(size_t)b * S] = b; }          // jobs 0 .. B-1: the unablated events
    for (int b = 0; b < B; ++b)
        for (int s = 1; s < S; ++s) {
            const bool valid = tr[(size_t)b * S + s] >= 0;
            src[(size_t)b * S + s] = valid ? (int32_t)jobs.size() : b;
            if (valid) jobs.push_back(b * S + s);
        }
    const int J = (int)jobs.size();
    int* d_jobs = reinterpret_cast<int*>(w + o.jobs);
    int* d_src = reinterpret_cast<int*>(w + o.src);
    float* lg = reinterpret_cast<float*>(w + o.lg);
    TCVN_CHECK(hipMemcpyAsync(d_jobs, jobs.data(), (size_t)J * 4, hipMemcpyHostToDevice, st));
    TCVN_CHECK(hipMemcpyAsync(d_src, src.data(), src.size() * 4, hipMemcpyHostToDevice, st));
    TCVN_CHECK(hipStreamSynchronize(st));                                                   // the host vectors are pageable
    for (int off = 0; off < J; off += o.cap) {
        const int n = J - off < o.cap ? J - off : o.cap;
        auto gather = [&](float* X0, int* vrow) { return loo_gather(tokens, tok_row, d_jobs + off, X0, vrow, n, S, D, st); };
        if (int rc = run_pass(p->plan, n, P, w, ws_bytes, o.pass, st, gather, lg + (long)off * Ce, nullptr)) return rc;
    }
    return loo_scatter(lg, d_src, event_logits, loo, B, S, Ce, st);
}

int64_t tcvn_head_shapley_workspace_bytes(const tcvn_head* p, int batch, int max_prongs, int max_exact, int samples) {
    if (!p || !shap_shape_ok(batch, max_prongs, max_exact, samples)) return -1;
    ShapLayout o;
    shap_layout(p->plan, batch, max_prongs, max_exact, samples, o);
    return o.total;
}
int64_t tcvn_head_shapley_count(int batch, int max_prongs, const int32_t* tok_row, int max_exact, int samples, void* stream) {
    if (!tok_row || !shap_shape_ok(batch, max_prongs, max_exact, samples)) {
        fprintf(stderr, "tcvn: head_shapley_count: bad argument (NULL pointer, batch outside 1..65535, max_prongs outside 0..63, max_exact outside 0..%d or samples < 1)\n",
                TCVN_SHAP_MAX_EXACT);
        return -1;
    }
    ShapHost h;
    if (shap_read_table(tok_row, batch, 1 + max_prongs, max_exact, samples, reinterpret_cast<hipStream_t>(stream), h)) return -2;
    return h.offsets[batch];
}
int tcvn_head_shapley(tcvn_head* p, int batch, int max_prongs, const float* tokens, const int32_t* tok_row, int max_exact, int samples,
                      uint64_t seed, int value_kind, float* event_logits, float* phi, float* std_error, float* interaction,
                      int32_t* exact, int64_t* offsets, int64_t* masks, int32_t* event, float* coalition_logits, int64_t n_coalitions,
                      int32_t* permutations, void* ws, int64_t ws_bytes, void* stream) {
    const bool prongs = max_prongs > 0;
    if (!p || !tokens || !tok_row || !event_logits || !exact || !offsets || !masks || !event || !coalition_logits || !ws ||
        (prongs && (!phi || !std_error || !interaction || !permutations)) || !shap_shape_ok(batch, max_prongs, max_exact, samples) ||
        (value_kind != TCVN_SHAP_VALUE_PROB && value_kind != TCVN_SHAP_VALUE_LOGIT) || n_coalitions < batch) {
        fprintf(stderr, "tcvn: head_shapley: bad argument (NULL pointer, batch outside 1..65535, max_prongs outside 0..63, max_exact outside 0..%d, samples < 1, unknown value kind or fewer coalitions than events)\n",
                TCVN_SHAP_MAX_EXACT);
        return -1;
    }
    ShapLayout o;
    shap_layout(p->plan, batch, max_prongs, max_exact, samples, o);
    if (ws_bytes < o.total) {
        fprintf(stderr, "tcvn: head_shapley: workspace of %lld bytes, %ld needed\n", (long long)ws_bytes, o.total);
        return -12;
    }
    if (!p->plan.bound) { fprintf(stderr, "tcvn: head_shapley: parameters are not bound\n"); return -11; }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int B = batch, P = max_prongs, S = 1 + P, M = samples, D = p->plan.cfg.hidden_dim, Ce = p->plan.cfg.event_classes;
    char* w = reinterpret_cast<char*>(ws);
    ShapHost h;
    if (int rc = shap_read_table(tok_row, B, S, max_exact, M, st, h)) return rc;
    const long J = h.offsets[B];
    if (J != n_coalitions) {
        fprintf(stderr, "tcvn: head_shapley: outputs sized for %lld coalitions, this mask has %ld (tcvn_head_shapley_count)\n",
                (long long)n_coalitions, J);
        return -13;
    }
    int32_t* d_n = reinterpret_cast<int32_t*>(w + o.n);
    int64_t* d_vmask = reinterpret_cast<int64_t*>(w + o.vmask);
    double* values = reinterpret_cast<double*>(w + o.values);
    TCVN_CHECK(hipMemcpyAsync(offsets, h.offsets.data(), (size_t)(B + 1) * 8, hipMemcpyHostToDevice, st));      // outputs that double as
    TCVN_CHECK(hipMemcpyAsync(exact, h.exact.data(), (size_t)B * 4, hipMemcpyHostToDevice, st));                // the device's table
    TCVN_CHECK(hipMemcpyAsync(d_n, h.n.data(), (size_t)B * 4, hipMemcpyHostToDevice, st));
    TCVN_CHECK(hipMemcpyAsync(d_vmask, h.vmask.data(), (size_t)B * 8, hipMemcpyHostToDevice, st));
    TCVN_CHECK(hipStreamSynchronize(st));                                                   // the host vectors are pageable
    const ShapTable t{offsets, d_n, d_vmask, exact};
    int32_t* d_pos = reinterpret_cast<int32_t*>(w + o.pos);
    if (int rc = shap_perm(tok_row, permutations, d_pos, B, M, P, seed, st)) return rc;
    for (long off = 0; off < J; off += o.cap) {
        const int n = (int)(J - off < o.cap ? J - off : o.cap);
        auto gather = [&](float* X0, int* vrow) {
            return shap_gather(tokens, tok_row, t, permutations, off, n, B, M, S, D, X0, vrow, masks, event, st);
        };
        if (int rc = run_pass(p->plan, n, P, w, ws_bytes, o.pass, st, gather, coalition_logits + off * Ce, nullptr)) return rc;
    }
    if (int rc = shap_full_rows(coalition_logits, t, event_logits, B, Ce, st)) return rc;
    if (int rc = shap_values(coalition_logits, values, J, Ce, value_kind == TCVN_SHAP_VALUE_PROB, st)) return rc;
    if (int rc = shap_exact(values, t, phi, std_error, B, P, Ce, st)) return rc;
    if (int rc = shap_pairs(values, t, interaction, B, P, Ce, st)) return rc;
    return shap_sampled(values, t, d_pos, phi, std_error, B, M, P, Ce, st);
}

int64_t tcvn_head_occlusion_workspace_bytes(const tcvn_head* p, int max_prongs) {
    if (!p || max_prongs < 0 || 1 + max_prongs > 64) return -1;
    OccHeadLayout o;
    occ_head_layout(p->plan, max_prongs, o);
    return o.total;
}
int tcvn_head_occlusion(tcvn_head* p, int batch, int max_prongs, int n_prongs, const float* rows, const float* tokens,
                        const int32_t* tok_row, int n, const int32_t* vimg, const int32_t* index, int row_base, const float* emb,
                        int64_t emb_ld, int col0, int width, float* occluded_event_logits, float* occluded_prong_logits, void* ws,
                        int64_t ws_bytes, void* stream) {
    if (!p || !rows || !tokens || !tok_row || !vimg || !index || !emb || !occluded_event_logits || !ws ||
        (max_prongs > 0 && !occluded_prong_logits) || batch <= 0 || max_prongs < 0 || 1 + max_prongs > 64 || n_prongs < 0 || n < 1 ||
        n > TCVN_OCC_MAX_PASS || row_base < 0 || row_base > batch + n_prongs || col0 < 0 || width < 1 ||
        col0 + width > p->plan.cfg.in_dim || emb_ld < width) {
        fprintf(stderr, "tcvn: head_occlusion: bad argument (NULL pointer, batch < 1, more than 64 tokens, n outside 1..%d or columns outside the row)\n",
                TCVN_OCC_MAX_PASS);
        return -1;
    }
    OccHeadLayout o{};
    occ_head_layout(p->plan, max_prongs, o);
    if (ws_bytes < o.total) {
        fprintf(stderr, "tcvn: head_occlusion: workspace of %lld bytes, %ld needed\n", (long long)ws_bytes, o.total);
        return -12;
    }
    if (!p->plan.bound) { fprintf(stderr, "tcvn: head_occlusion: parameters are not bound\n"); return -11; }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int P = max_prongs, S = 1 + P, D = p->plan.cfg.hidden_dim;
    char* w = reinterpret_cast<char*>(ws);
    float* vrows = reinterpret_cast<float*>(w + o.vrows);
    int* ident = reinterpret_cast<int*>(w + o.ident);
    if (int rc = occ_rows(rows, vimg, row_base, emb, emb_ld, col0, width, vrows, ident, n, p->plan.cfg.in_dim, batch + n_prongs, st)) return rc;
    HeadStep e;                         // n one-token sequences embedded in the scan's own buffers
    if (int rc = p->plan.step(n, 0, 0, w, ws_bytes, 0, 0, st, e)) return rc;
    e.L = o.E;
    if (int rc = p->plan.embed(e, vrows, ident)) return rc;                                   // -> E.X[0] [n][D]
    auto gather = [&](float* X0, int* vrow) { return occ_gather(tokens, tok_row, index, e.F(o.E.X[0]), X0, vrow, n, batch, S, D, st); };
    return run_pass(p->plan, n, P, w, ws_bytes, o.pass, st, gather, occluded_event_logits, occluded_prong_logits);
}
}
