/* tcvn_hip.h -- C ABI of libtcvn_hip.so: the MI355X (gfx950) implementation of the TransformerCVN hot path.
 *
 * The reference (ayankele/dune-transformercvn) has no native interface of its own: its hot path is the Python call
 * chain NeutrinoFullDenseTrainer.forward -> NeutrinoDenseNetwork.forward -> torch ATen ops
 * (transformercvn/network/trainers/neutrino_full_base_trainer.py:90-116, networks/neutrino_full_base_network.py:87-125,
 * :166-188, layers/dense_net.py:8-167).  This header is the boundary a maintainer binds instead of those ATen calls
 * (see INTEGRATION.md for the ctypes stub).  Plain pointers and sizes only; every pointer is a DEVICE pointer unless
 * named h_*; every function enqueues work on `stream` (a hipStream_t passed as void*) and returns 0 on success or a
 * non-zero hipError_t / negative argument-error code.  No function allocates per call or synchronises the device;
 * workspaces are supplied by the caller.
 */
#ifndef TCVN_HIP_H
#define TCVN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TCVN_MODE_F32 0  /* fp32 activations, v_mfma_f32_32x32x2_f32 : parity mode (1e-3 logit gate)      */
#define TCVN_MODE_BF16 1 /* bf16 activations/weights, v_mfma_f32_32x32x16_bf16, fp32 accumulate/statistics */

#define TCVN_SLOT_PARAM 0   /* float tensor with gradient            */
#define TCVN_SLOT_BUFFER 1  /* float tensor without gradient (BN running statistics) */
#define TCVN_SLOT_COUNTER 2 /* int64 scalar (num_batches_tracked); kept by the host, never read on the device */

int tcvn_version(void);

/* ---------------------------------------------------------------------------------------------------------------
 * DenseNet embedder (replaces transformercvn/network/layers/dense_net.py:97-167 DenseNet.forward and its autograd)
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct tcvn_densenet_cfg {
    int in_ch;          /* pixel channels (3)                                   */
    int out_dim;        /* embedding width (256 prong / 288 event)              */
    int init_ch;        /* options.initial_pixel_dim                            */
    int growth;         /* options.densenet_growth_rate                         */
    int bn_size;        /* options.densenet_batch_norm_size                     */
    int n_blocks;       /* len(options.densenet_structure) (<= 8)               */
    int layers[8];      /* options.densenet_structure                           */
    int H, W;           /* pixel map shape (400, 280)                           */
    float dropout;      /* options.dropout                                      */
    int mode;           /* TCVN_MODE_*                                          */
} tcvn_densenet_cfg;

typedef struct tcvn_densenet tcvn_densenet; /* opaque plan */

int tcvn_densenet_create(const tcvn_densenet_cfg* cfg, tcvn_densenet** out);
void tcvn_densenet_destroy(tcvn_densenet* p);

/* Parameter slots in reference state_dict order; names are relative to the DenseNet module
 * ("features.conv0.weight", ..., "output_block.relu.weight"). */
int tcvn_densenet_num_slots(const tcvn_densenet* p);
int tcvn_densenet_slot(const tcvn_densenet* p, int i, char* name, int name_cap, int64_t* numel, int* kind);
/* data[i]: device pointer of slot i (fp32, reference layout: conv OIHW); grad[i]: fp32 gradient of the same shape
 * (ignored for buffers/counters; may be NULL for inference-only use). */
int tcvn_densenet_bind(tcvn_densenet* p, void* const* data, void* const* grad);

int64_t tcvn_densenet_workspace_bytes(const tcvn_densenet* p, int n_img, int with_backward);

/* Forward over n_img sparse pixel maps.
 *   coords [nnz,3] int32 (image, y, x), values [nnz, in_ch] fp32 raw pixel values (reference:
 *   trainers/neutrino_full_dense_trainer.py:15-24,46-67: v/255 or log(v+1), optional multiplicative noise, COO->dense).
 *   out [n_img, out_dim] fp32 with row stride out_ld.
 *   train != 0: batch statistics, running-stat update, dropout (seed) -- and the workspace keeps what backward needs;
 *   `coords` must stay valid until tcvn_densenet_backward has run (the stem weight gradient walks the hit list). */
int tcvn_densenet_forward(tcvn_densenet* p, int n_img, const int32_t* coords, const float* values, int64_t nnz,
                          int log_pixels, float noise_std, float* out, int64_t out_ld, void* workspace,
                          int64_t workspace_bytes, int train, uint64_t seed, void* stream);
/* log_pixels: 0 = v/255, 1 = log(v+1), 2 = values are final, 3 = one_hot_pixels (reference :47-52): values [nnz, in_ch/256] hold
 * integers 0..255, pixel channel f*256 + v is set to 1 (no scaling, no noise); conv0 then has in_ch = 256 * value channels. */

/* Backward of the last train-mode forward on the same workspace: d_out [n_img, out_dim] fp32 -> parameter gradients
 * are ACCUMULATED into the bound grad pointers (zero them first). */
int tcvn_densenet_backward(tcvn_densenet* p, int n_img, const float* d_out, int64_t d_out_ld, void* workspace,
                           int64_t workspace_bytes, void* stream);

/* The same backward in slices: dense blocks block_hi ... block_lo (0-based, walked downwards).  block_hi = n_blocks-1 also runs the
 * output block, block_lo = 0 also the stem; the parameter gradients of a slice are final when its call returns (in stream order), so
 * a data-parallel caller can start their all-reduce under the remaining slices.  Slices must be issued from the last block to the
 * first and cover every block exactly once. */
int tcvn_densenet_num_blocks(const tcvn_densenet* p);
int tcvn_densenet_backward_blocks(tcvn_densenet* p, int n_img, const float* d_out, int64_t d_out_ld, void* workspace,
                                  int64_t workspace_bytes, int block_hi, int block_lo, void* stream);

/* Debug/validation taps into the workspace of the last forward: name in {"img","conv0","dense<b>","bottleneck<b>.<l>","condense"},
 * "output_linear" (the fp32 rows the output block's BatchNorm1d normalises), in bf16 mode also the materialised operands
 * "xa<b>.<l>" / "ya<b>.<l>", and the raw regions "raw:wk","raw:tabs","raw:bstat<b>" (b = 0: norm0),"raw:ystat<b>.<l>","raw:head_stat",
 * "raw:isumy<b>.<l>" (exists only where the last forward derived norm2 link-free);
 * after a backward pass also "raw:grad<b>" (gradient accumulator of block b's concat buffer), "raw:pq<b>" (its [2][ld] fp32 (P, Q) rows),
 * "raw:du<b>" (the 3x3 data-gradient scratch in block b's geometry: it holds the layer that ran last) and "raw:ey<b>.<l>" (the eff rows
 * [pixels][32] of a layer's 3x3 output gradient, bf16 mode with growth 32; filled only by the consecutive-tile data-gradient kernel)
 * and "raw:dcondense" (fp32 [n][C]: the gradient with respect to "condense"), and the stem's own backward state (b = 0): "raw:du0"
 * (DU0 over the conv0 map, [n][Hc][Wc][init_ch]; with the activity bitmap on, rows no hit reaches are never stored) and "raw:pq0"
 * (BatchNorm0's [2][init_ch] fp32 (P0, Q0) rows) -- what tests/stem_reference.py checks per element;
 * returns the byte offset into the workspace and the logical NHWC shape + channel stride + element size. */
int tcvn_densenet_tap(const tcvn_densenet* p, int n_img, const char* name, int64_t* byte_off, int* n, int* h, int* w,
                      int* c, int* ld, int* elem_bytes);

/* ---------------------------------------------------------------------------------------------------------------
 * SDXL-style embedder (replaces transformercvn/network/layers/sdxl_net.py:7-42 SDXLNet.forward and its autograd: the
 * diffusers VAE Encoder with block_out_channels [d,d,2d,2d,4d,4d,8d,8d,out], GroupNorm with one group, SiLU, stride-2
 * downsampling with (0,1,0,1) padding, one-token mid-block attention, then Flatten + Linear(out,out); selected by
 * networks/neutrino_full_sdxl_network.py:6-20).  Same calling convention as the DenseNet embedder.  Parity is UNPINNED:
 * diffusers is neither vendored nor pinned by the reference; oracle/sdxl_oracle.py restates the definitions.
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct tcvn_sdxl_cfg {
    int in_ch;          /* pixel channels (3)                                                   */
    int out_dim;        /* embedding width (256 prong / 288 event) = last block's channel count */
    int init_ch;        /* options.initial_pixel_dim (64)                                       */
    int repeat;         /* repeat_block_dim (2)                                                 */
    int num_blocks;     /* num_blocks (4): widths d, 2d, 4d, 8d, each `repeat` times            */
    int H, W;           /* pixel map shape (400, 280); must reduce to 1x1                       */
    int mode;           /* TCVN_MODE_*                                                          */
} tcvn_sdxl_cfg;
typedef struct tcvn_sdxl tcvn_sdxl;
int tcvn_sdxl_create(const tcvn_sdxl_cfg* cfg, tcvn_sdxl** out);
void tcvn_sdxl_destroy(tcvn_sdxl* p);
/* slots in state_dict order, names relative to the SDXLNet module ("encoder.conv_in.weight", ..., "output_layer.1.bias") */
int tcvn_sdxl_num_slots(const tcvn_sdxl* p);
int tcvn_sdxl_slot(const tcvn_sdxl* p, int i, char* name, int name_cap, int64_t* numel, int* kind);
int tcvn_sdxl_bind(tcvn_sdxl* p, void* const* data, void* const* grad);
int64_t tcvn_sdxl_workspace_bytes(const tcvn_sdxl* p, int n_img, int with_backward);
/* Same calling convention as tcvn_densenet_forward / _backward; `coords` must stay valid until tcvn_sdxl_backward has run (the
 * conv_in weight gradient walks the hit list). */
int tcvn_sdxl_forward(tcvn_sdxl* p, int n_img, const int32_t* coords, const float* values, int64_t nnz, int log_pixels,
                      float noise_std, float* out, int64_t out_ld, void* workspace, int64_t workspace_bytes, int train,
                      uint64_t seed, void* stream);
int tcvn_sdxl_backward(tcvn_sdxl* p, int n_img, const float* d_out, int64_t d_out_ld, void* workspace, int64_t workspace_bytes,
                       void* stream);
/* taps: "img", "conv_in", "block<i>" (output of down block i in front of its downsampler), "mid" */
int tcvn_sdxl_tap(const tcvn_sdxl* p, int n_img, const char* name, int64_t* byte_off, int* n, int* h, int* w, int* c, int* ld,
                  int* elem_bytes);
/* Which kernel family convolution `conv_index` (tape order, 0 .. tcvn_sdxl_num_convs - 1) of a training step on n_img maps runs in each
 * direction: TCVN_SCONV_*; *dgrad = -1 for conv_in, which has no data gradient.  Assumes a workspace at a 256-byte aligned address
 * with the weight-gradient slab and a hit list present.  Makes no GPU call. */
enum { TCVN_SCONV_GENERIC = 0, TCVN_SCONV_C64 = 1, TCVN_SCONV_G = 2, TCVN_SCONV_S2 = 3, TCVN_SCONV_IN = 4 };
int tcvn_sdxl_num_convs(const tcvn_sdxl* p);
int tcvn_sdxl_conv_kernels(const tcvn_sdxl* p, int n_img, int conv_index, int* fwd, int* dgrad, int* wgrad);
/* The tape, op by op in execution order (validation): fields[TCVN_SDXL_OP_*], n_fields >= TCVN_SDXL_OP_FIELDS.  kind 0 = convolution
 * (out = conv(in; slot w, bias slot w + 1) [+ res]), 1 = GroupNorm (+ SiLU when act).  in / out / res are buffer indices (0 = the pixel
 * map), w a slot index, conv_id the row of tcvn_sdxl_conv_kernels, stats_gn the GroupNorm (gn_id) a convolution delivers the statistics
 * of, stats_given whether a GroupNorm receives them, final_f32 the convolution that writes the caller's fp32 output.  A field that does
 * not apply to the op's kind is -1.  Makes no GPU call. */
enum { TCVN_SDXL_OP_KIND = 0, TCVN_SDXL_OP_IN, TCVN_SDXL_OP_OUT, TCVN_SDXL_OP_RES, TCVN_SDXL_OP_W, TCVN_SDXL_OP_KS, TCVN_SDXL_OP_STRIDE,
       TCVN_SDXL_OP_PAD, TCVN_SDXL_OP_ACT, TCVN_SDXL_OP_CONV_ID, TCVN_SDXL_OP_GN_ID, TCVN_SDXL_OP_STATS_GN, TCVN_SDXL_OP_STATS_GIVEN,
       TCVN_SDXL_OP_FINAL_F32, TCVN_SDXL_OP_FIELDS };
int tcvn_sdxl_num_ops(const tcvn_sdxl* p);
int tcvn_sdxl_op(const tcvn_sdxl* p, int i, int* fields, int n_fields);
/* Where the engine keeps a piece of its state in a workspace of n_img maps (validation): byte offset, up to four extents (dense,
 * row-major) and the element size.  ACT / GRAD: buffer `index`, [n, H, W, C] in the mode's element type (GRAD: the nominal gradient
 * region; a residual input may take over its output's region during a backward).  WK / WKT / GWK: convolution `index` (conv_id), the
 * packed weights [Cout][Kp], k = tap * Cin + c, the transposed pack [Cin][Kpt], k = tap * Cout + n, and the fp32 kernel-layout weight
 * gradient [Cout][Kp].  STATS / BSTATS: [n_gn][n][2] doubles, (sum, sum of squares) of every GroupNorm input and the backward sums
 * (sum gamma dU, sum gamma dU xhat); index ignored.  Returns non-zero where the layout has no such region.  Makes no GPU call. */
enum { TCVN_SDXL_REGION_ACT = 0, TCVN_SDXL_REGION_GRAD, TCVN_SDXL_REGION_WK, TCVN_SDXL_REGION_WKT, TCVN_SDXL_REGION_GWK,
       TCVN_SDXL_REGION_STATS, TCVN_SDXL_REGION_BSTATS };
int tcvn_sdxl_region(const tcvn_sdxl* p, int n_img, int with_backward, int what, int index, int64_t* byte_off, int64_t* shape, int* ndim,
                     int* elem_bytes);

/* ---------------------------------------------------------------------------------------------------------------
 * Token path: combined embedding, transformer encoder, decoders, focal loss
 * (networks/neutrino_full_base_network.py:99-125,184-188; layers/prong_custom_bert_encoder.py:57-75;
 *  layers/prong_decoder.py:15-16; layers/prong_target_decoder.py:34-41; trainers/neutrino_full_base_trainer.py:148-177)
 * --------------------------------------------------------------------------------------------------------------- */
typedef struct tcvn_head_cfg {
    int hidden_dim, heads, n_layers;       /* encoder: d_model, heads, layers; FFN width == hidden_dim (reference quirk) */
    int in_dim;                            /* combined embedding input width (feat + pix + pos = 320)              */
    int event_classes, prong_classes;
    int n_dec; int dec_dims[8];            /* prong decoder widths after each hidden block (64,32,16,8)           */
    int dec_out_in;                        /* in_features of prong_decoder.output_layer (reference quirk value)   */
    int gelu;                              /* 1 = gelu, 0 = relu                                                   */
    int norm_first;
    int dropout_modules;                   /* 1 when options.dropout > 0 (shifts prong_decoder.hidden_layers idx)  */
    float dropout; float gamma; float event_weight;
    int no_linear_bn;                      /* 1 = options.linear_batch_norm False: LinearBlock = Linear(bias)-act-Dropout, decoder blocks without
                                              BatchNorm1d (prong_feature_embedding.py:11-16, encoder.py:13-14); 0 = the shipped option files   */
    int linear_relu;                       /* 1 = options.linear_prelu_activation False: ReLU instead of PReLU (:18-21, :16-19), no slope slots  */
} tcvn_head_cfg;

typedef struct tcvn_head tcvn_head;
int tcvn_head_create(const tcvn_head_cfg* cfg, tcvn_head** out);
void tcvn_head_destroy(tcvn_head* p);
int tcvn_head_num_slots(const tcvn_head* p);
int tcvn_head_slot(const tcvn_head* p, int i, char* name, int name_cap, int64_t* numel, int* kind);
int tcvn_head_bind(tcvn_head* p, void* const* data, void* const* grad);
int64_t tcvn_head_workspace_bytes(const tcvn_head* p, int batch, int max_prongs, int n_prongs);
/* The encoder stack runs as ONE launch forward (one workgroup per event, csrc/encoder_fused.hip) and TWO launches backward (the
 * data-gradient chain + a grouped weight-gradient GEMM) when hidden_dim == 128, heads in {4,8}, 1 + max_prongs <= 22 and <= 8
 * layers; otherwise, or after tcvn_head_set_fused_encoder(p, 0), layer by layer on the row kernels.  Both forwards fill the same
 * workspace buffers, so either backward follows either forward.  On by default. */
void tcvn_head_set_fused_encoder(tcvn_head* p, int on);

/* rows [batch + n_prongs, in_dim] fp32: event rows first, then packed prong rows (already concatenated with the
 * feature / position embeddings).  tok_row [batch, 1+max_prongs] int32: row index of each token or -1 for padding.
 * Outputs: event_logits [batch, event_classes], prong_logits [batch, max_prongs, prong_classes]. */
int tcvn_head_forward(tcvn_head* p, int batch, int max_prongs, int n_prongs, const float* rows, const int32_t* tok_row,
                      float* event_logits, float* prong_logits, void* workspace, int64_t workspace_bytes, int train,
                      uint64_t seed, void* stream);
/* The three stages of tcvn_head_forward as separate forward-only entry points -- what the reference's sub-modules compute when
 * called on their own (CreateCompiled.ipynb cells 7-8 call network.prong_embedding / .encoder / .event_decoder / .prong_decoder):
 *   embed   rows, tok_row -> tokens [batch, 1+max_prongs, hidden] (batch-major, padding rows zero): the combined LinearBlock +
 *           masked pad of BaseProngEmbedding.forward (networks/neutrino_full_base_network.py:113-125);
 *   encode  tokens [batch, S, hidden], tok_row (only its sign is read: < 0 = padding) -> hidden [S, batch, hidden] (sequence-major,
 *           masked): ProngCustomBertEncoder.forward (layers/prong_custom_bert_encoder.py:57-75);
 *   decode  hidden [S, batch, hidden] -> event_logits [batch, Ce] from token 0 (layers/prong_decoder.py:15-16) and prong_logits
 *           [batch, max_prongs, Cp] from tokens 1.. (layers/prong_target_decoder.py:34-41); either output may be NULL.
 * Workspace: tcvn_head_workspace_bytes(batch, max_prongs, n_prongs) (n_prongs = 0 for encode / decode).  No backward: training
 * goes through tcvn_head_forward / tcvn_head_backward. */
int tcvn_head_embed(tcvn_head* p, int batch, int max_prongs, int n_prongs, const float* rows, const int32_t* tok_row, float* tokens,
                    void* workspace, int64_t workspace_bytes, int train, uint64_t seed, void* stream);
int tcvn_head_encode(tcvn_head* p, int batch, int max_prongs, const float* tokens, const int32_t* tok_row, float* hidden,
                     void* workspace, int64_t workspace_bytes, int train, uint64_t seed, void* stream);
int tcvn_head_decode(tcvn_head* p, int batch, int max_prongs, const float* hidden, float* event_logits, float* prong_logits,
                     void* workspace, int64_t workspace_bytes, int train, uint64_t seed, void* stream);

/* Explaining a prediction (forward only; nothing here changes a forward, a backward or a parameter).
 *   attention   weights [layers, batch, heads, S, S] fp32, S = 1 + max_prongs: the probability with which token i attends to token j
 *               (softmax over j of q_i.k_j / sqrt(head_dim), padded keys excluded, BEFORE attention dropout) -- what
 *               nn.MultiheadAttention(need_weights=True, average_attn_weights=False) returns inside the reference's encoder layers.
 *               Token 0 is the event, token 1 + p prong slot p.  Columns of padded keys and rows of padded queries are exactly 0.
 *               Exports what the last tcvn_head_forward / tcvn_head_encode (train or eval, either encoder path) left in `workspace`;
 *               batch / max_prongs must be that call's.  The workspace is read, never written: a backward may still follow.
 *   rollout     [batch, S, S] = A^_{L-1} ... A^_0 with A^_l = rownorm(0.5 fuse_h(weights[l]) + 0.5 I_valid) (Abnar & Zuidema 2020);
 *               I_valid has ones at valid tokens only, so padded tokens have zero rows and columns.  rollout[b, 0, 1 + p] is the
 *               relevance of prong slot p for the event token.  One workgroup per event, S <= 64.
 *   leave one out   event_logits [batch, Ce] and loo_event_logits [batch, max_prongs, Ce]: row [b, p] is event_logits[b] recomputed
 *               with prong slot p masked out (token zeroed, key padded; the encoder has no positional encoding, so this IS the event
 *               without that prong); rows of padded slots are copies of event_logits[b].  Eval arithmetic (no dropout).  tokens
 *               [batch, S, hidden] as tcvn_head_embed returns them.  The variants (one sequence per valid prong) run through the
 *               encoder and the event decoder in passes of at most TCVN_LOO_MAX_PASS sequences; workspace:
 *               tcvn_head_leave_one_out_workspace_bytes.  The call reads tok_row back to build the variant list, so it
 *               synchronises with `stream` (not capturable into a graph).
 * Argument errors (NULL, S > 64, layers < 1, unknown fusion, workspace too small or of another shape) return non-zero before any
 * device call and print one "tcvn:" line. */
#define TCVN_FUSE_MEAN 0
#define TCVN_FUSE_MAX 1
#define TCVN_LOO_MAX_PASS 256
int tcvn_head_attention(tcvn_head* p, int batch, int max_prongs, const int32_t* tok_row, const void* workspace,
                        int64_t workspace_bytes, float* weights, void* stream);
int tcvn_attention_rollout(const float* weights, const int32_t* tok_row, int layers, int batch, int heads, int seq, int head_fusion,
                           float* rollout, void* stream);
int64_t tcvn_head_leave_one_out_workspace_bytes(const tcvn_head* p, int batch, int max_prongs);
int tcvn_head_leave_one_out(tcvn_head* p, int batch, int max_prongs, const float* tokens, const int32_t* tok_row,
                            float* event_logits, float* loo_event_logits, void* workspace, int64_t workspace_bytes, void* stream);

/* Prong Shapley values (forward only, eval arithmetic): the event's class score shared among its prongs.
 *   coalition   a subset C of the valid prong slots N_b of event b (n = |N_b|, max_prongs <= 63), stored as an int64 mask: bit p set =
 *               slot p present.  Its sequence is event b's tokens [batch, S, hidden] (tcvn_head_embed) with every absent or padded
 *               prong token zeroed and padded as a key; token 0, the event's own map, is present whenever tok_row says so.  Its value
 *               v_c(C) per event class c is the softmax probability (TCVN_SHAP_VALUE_PROB, formed in double precision) or the raw logit
 *               (TCVN_SHAP_VALUE_LOGIT) of the event decoder on that sequence.
 *   exact       events with n <= max_exact (0..TCVN_SHAP_MAX_EXACT) run all 2^n coalitions, ordered by the compact index k: bit i of k
 *               stands for the i-th valid slot in ascending slot order (k = 0 empty, k = 2^n - 1 full; n = 0: one coalition).
 *               phi[b, p, c] = sum over C in N\{p} of |C|! (n-|C|-1)! / n! (v_c(C + p) - v_c(C)).  interaction[b, p, q, c], p != q: half
 *               the Shapley interaction index, 1/2 sum over C in N\{p,q} of |C|! (n-|C|-2)! / (n-1)! (v(C+p+q) - v(C+p) - v(C+q) + v(C));
 *               p = q: phi[b, p] - sum_{q != p} interaction[b, p, q] (the SHAP convention: symmetric, row p sums to phi[b, p]).
 *               std_error is 0.
 *   sampled     events with n > max_exact: permutations[b, m] (m < samples) is N_b sorted by (key, slot), key = word 0 of the library's
 *               Philox-4x32-10 with counter (slot, m, b, 0x53484150) and the 64-bit seed as key, followed by -1 up to max_prongs
 *               entries (drawn for every event, used by the sampled ones).  The event's coalitions: empty, full, then for every m the
 *               prefixes of length 1 .. n-1 of permutation m.  phi[b, p, c] is the mean over m of v_c(prefix with p) - v_c(prefix
 *               before p), std_error the sample standard deviation of those contributions / sqrt(samples) (0 with samples = 1);
 *               interaction is NaN.
 *   both        rows and columns of padded slots are exactly 0 in phi, std_error and interaction, and sum_p phi[b, p, c] =
 *               v_c(full) - v_c(empty).  Values are double precision, every sum is taken in a fixed order without atomics (two runs
 *               agree bit for bit) and rounded to fp32 once.
 *   outputs     event_logits [batch, Ce] (the full coalition's row), phi / std_error [batch, max_prongs, Ce], interaction [batch,
 *               max_prongs, max_prongs, Ce], exact [batch] (1 / 0), offsets [batch + 1] (event b owns coalitions offsets[b] ..
 *               offsets[b+1]-1), masks [J], event [J], coalition_logits [J, Ce], permutations [batch, samples, max_prongs]; all device
 *               memory.  J = n_coalitions must be what tcvn_head_shapley_count returns for the same tok_row, max_exact and samples
 *               (sum over events of 2^n or 2 + samples (n-1)).  With max_prongs = 0 the prong-shaped outputs may be NULL.
 *   passes      the coalitions run through the encoder and the event decoder in passes of at most TCVN_SHAP_MAX_PASS sequences; job ->
 *               (event, mask) is resolved on the device from a per-event table.  Both calls read tok_row back, so they synchronise
 *               with `stream` (not capturable into a graph).  Workspace: tcvn_head_shapley_workspace_bytes, asked for
 *               before the mask is known and therefore sized for the most coalitions a mask of this shape can have (double-precision values of
 *               batch x max(2^min(max_prongs, max_exact), 2 + samples (max_prongs - 1)) coalitions, plus one pass): it grows with max_exact.
 * Argument errors (NULL, batch outside 1..65535, max_prongs > 63, max_exact outside 0..16, samples < 1, unknown value kind, workspace
 * too small, parameters not bound, n_coalitions not the mask's count) return non-zero before any kernel and print one "tcvn:" line. */
#define TCVN_SHAP_MAX_PASS 1024
#define TCVN_SHAP_MAX_EXACT 16
#define TCVN_SHAP_VALUE_PROB 0
#define TCVN_SHAP_VALUE_LOGIT 1
int64_t tcvn_head_shapley_workspace_bytes(const tcvn_head* p, int batch, int max_prongs, int max_exact, int samples);
int64_t tcvn_head_shapley_count(int batch, int max_prongs, const int32_t* tok_row, int max_exact, int samples, void* stream);
int tcvn_head_shapley(tcvn_head* p, int batch, int max_prongs, const float* tokens, const int32_t* tok_row, int max_exact, int samples,
                      uint64_t seed, int value_kind, float* event_logits, float* phi, float* std_error, float* interaction,
                      int32_t* exact, int64_t* offsets, int64_t* masks, int32_t* event, float* coalition_logits, int64_t n_coalitions,
                      int32_t* permutations, void* workspace, int64_t workspace_bytes, void* stream);

/* Occlusion maps (forward only, eval arithmetic): which regions of which pixel maps a prediction rests on.
 *   tile        (tile_h, tile_w) >= 1, need not divide the map: grid_h = ceil(height / tile_h), grid_w = ceil(width / tile_w); the hit
 *               (y, x) lies in tile (y / tile_h, x / tile_w); the last row / column of tiles may be ragged.
 *   variant     (b, s, ty, tx): event b, token slot s (0 = the event's own map, 1 + p = the map of valid prong slot p) and a tile of
 *               that map that holds at least one hit.  Its input is the same event with every hit of that tile removed from that one
 *               map, all other hits in their original order (duplicate coordinates: the highest index wins, as in the embedders).  A
 *               tile without hits is no variant: removing nothing changes nothing.  A variant may be an empty map; its token then
 *               carries the embedding of an image without hits (this is not leave-one-out: the token stays in the sequence).
 *   variants    one hit list (coords [nnz, 3] = (image, y, x), sorted by image, every hit inside the map) -> the V variants of its
 *               n_img images ordered by (image, ty, tx): vimg [V] the image, index [V, 4] = (img_bs[image][0], img_bs[image][1], ty,
 *               tx) with img_bs [n_img, 2] the caller's (b, s) of every image.  vimg and index need room for n_img * grid_h * grid_w
 *               rows.  host_out (host memory, 4 + ceil(n_img * grid_h * grid_w / max_pass) + 1 words): [0] = V, [1] != 0: the list
 *               is not sorted by image, [2] != 0: some hit lies outside the images / the map (in both cases nothing else is valid:
 *               drop those hits, sort stably by image and call again), [3] = hits of all variants together, [4 + k] = first row of
 *               pass k in the hit lists of the variants (pass k = variants k * max_pass ...; entry ceil(V / max_pass) is the end of
 *               the last pass).  Occupancy counts are integer atomics: deterministic.  The call synchronises with `stream` once.
 *   build_pass  writes the hit lists of variants first .. first + count - 1 (count <= max_pass, one pass): out_coords [rows, 3] with
 *               the image index rewritten to the variant's index inside the pass, out_values [rows, channels] copied untouched;
 *               rows = host_out[4 + k + 1] - host_out[4 + k]; nothing is written beyond out_rows.  The result goes through
 *               tcvn_densenet_forward / tcvn_sdxl_forward (train = 0) as `count` images; rows = 0 is a pass of empty maps.
 *   head_occlusion  one pass through the token path: variant j takes row row_base + vimg[j] of `rows` (the rows of the forward being
 *               explained) with columns [col0, col0 + width) replaced by emb[j] (the embedder output of the pass, row stride emb_ld),
 *               goes through the combined embedding as a one-token sequence and replaces token index[j][1] of event index[j][0] in
 *               `tokens` [batch, S, hidden] (tcvn_head_embed of the same forward); encoder and both decoders then give
 *               occluded_event_logits [n, Ce] and occluded_prong_logits [n, max_prongs, Cp] (rows of padded slots as
 *               tcvn_head_decode leaves them).  n <= TCVN_OCC_MAX_PASS; workspace of its own (tcvn_head_occlusion_workspace_bytes), so
 *               the forward's workspace keeps its attention probabilities.
 *   heatmap     [batch, 1 + max_prongs, grid_h, grid_w] = softmax(base)[c] - softmax(occluded)[c] at every variant's position,
 *               exactly 0 elsewhere.  TCVN_OCC_TARGET_EVENT: event logits, c = classes[b] or (classes == NULL) the predicted class of
 *               event b.  TCVN_OCC_TARGET_PRONG: for s >= 1 the prong logits of slot s - 1 and that slot's predicted class; row s = 0
 *               stays 0.
 * Argument errors (NULL, tile < 1, max_pass outside 1..TCVN_OCC_MAX_PASS, S > 64, workspace too small) return non-zero before any
 * device call and print one "tcvn:" line. */
#define TCVN_OCC_MAX_PASS 256
#define TCVN_OCC_TARGET_EVENT 0
#define TCVN_OCC_TARGET_PRONG 1
int64_t tcvn_occlusion_workspace_bytes(int n_img, int height, int width, int tile_h, int tile_w, int max_pass);
int tcvn_occlusion_variants(const int32_t* coords, int64_t nnz, int n_img, int height, int width, int tile_h, int tile_w,
                            const int32_t* img_bs, int max_pass, int32_t* vimg, int32_t* index, void* workspace,
                            int64_t workspace_bytes, int64_t* host_out, int64_t host_cap, void* stream);
int tcvn_occlusion_build_pass(const int32_t* coords, const float* values, int64_t nnz, int channels, int n_img, int height, int width,
                              int tile_h, int tile_w, int max_pass, const int32_t* vimg, const void* workspace, int64_t workspace_bytes,
                              int first, int count, int32_t* out_coords, float* out_values, int64_t out_rows, void* stream);
int64_t tcvn_head_occlusion_workspace_bytes(const tcvn_head* p, int max_prongs);
int tcvn_head_occlusion(tcvn_head* p, int batch, int max_prongs, int n_prongs, const float* rows, const float* tokens,
                        const int32_t* tok_row, int n, const int32_t* vimg, const int32_t* index, int row_base, const float* emb,
                        int64_t emb_ld, int col0, int width, float* occluded_event_logits, float* occluded_prong_logits,
                        void* workspace, int64_t workspace_bytes, void* stream);
int tcvn_occlusion_heatmap(const float* event_logits, const float* prong_logits, const float* occluded_event_logits,
                           const float* occluded_prong_logits, const int32_t* index, int64_t n_variants, int batch, int max_prongs,
                           int event_classes, int prong_classes, int grid_h, int grid_w, int target, const int32_t* classes,
                           float* heatmap, void* stream);

/* Coarse-to-fine occlusion maps: level l uses tiles (tile_h >> l, tile_w >> l) and evaluates only the children of the variants of
 * level l - 1 that were selected.  Level 0 is the flat scan above.
 *   select      heat [batch, 1 + max_prongs, grid_h, grid_w] (tcvn_occlusion_heatmap of one level) and that level's index [V, 4] ->
 *               keep_map uint8 of the same shape: 1 at the variants to refine, 0 everywhere else.  score = |h| at the variant's
 *               position; m = the largest score of the variant's group (TCVN_OCC_GROUP_EVENT: all variants of event b;
 *               TCVN_OCC_GROUP_MAP: those of the map (b, s)); selected iff score >= keep * m (float32, one multiplication) and
 *               (keep == 0 or score > 0).  keep in [0, 1]; keep == 0 selects every variant.  group_max: batch * (1 + max_prongs)
 *               words of scratch (the maxima, as float bit patterns, taken with an integer atomicMax: order-independent).
 *   refine_variants  tcvn_occlusion_variants at the child tile (tile_h, tile_w), restricted by the parent level's keep_map
 *               [batch, 1 + max_prongs, parent_grid_h, parent_grid_w] (the grid of tiles (2 tile_h, 2 tile_w), checked): a hit counts
 *               towards its tile only if keep_map[b][s][y / (2 tile_h)][x / (2 tile_w)] != 0 with (b, s) = img_bs[image].  The variants
 *               are therefore the children (2 ty + i, 2 tx + j) of the selected tiles that hold a hit, ordered by (image, ty, tx).
 *               Same outputs, workspace layout (tcvn_occlusion_workspace_bytes at the child tile) and host_out as
 *               tcvn_occlusion_variants; tcvn_occlusion_build_pass serves the list unchanged: a variant's hits are still the whole
 *               image minus that one tile.
 *   mark        evaluated uint8 [batch, 1 + max_prongs, grid_h, grid_w]: 1 at the positions of index [V, 4], 0 elsewhere.
 *   occupancy   sets occupied[b][s][y / tile_h][x / tile_w] = 1 for every hit inside the map ((b, s) = img_bs[image]); the caller
 *               clears the map first and may call once per hit list.
 *   paint       out [batch, 1 + max_prongs, gh, gw] on the grid of the last of `levels` levels (host arrays heat[l], evaluated[l],
 *               grid_h[l], grid_w[l]; grid l = ceil(last grid / 2^(levels - 1 - l)), checked): a cell with occupied != 0 takes the
 *               stored heat value of the deepest level whose evaluated tile contains it, every other cell exactly 0.
 * Argument errors return non-zero before any device call and print one "tcvn:" line. */
#define TCVN_OCC_GROUP_EVENT 0
#define TCVN_OCC_GROUP_MAP 1
#define TCVN_OCC_MAX_LEVELS 16
int tcvn_occlusion_select(const float* heat, const int32_t* index, int64_t n_variants, int batch, int max_prongs, int grid_h,
                          int grid_w, int group, float keep, uint32_t* group_max, uint8_t* keep_map, void* stream);
int tcvn_occlusion_refine_variants(const int32_t* coords, int64_t nnz, int n_img, int height, int width, int tile_h, int tile_w,
                                   const int32_t* img_bs, const uint8_t* keep_map, int batch, int max_prongs, int parent_grid_h,
                                   int parent_grid_w, int max_pass, int32_t* vimg, int32_t* index, void* workspace,
                                   int64_t workspace_bytes, int64_t* host_out, int64_t host_cap, void* stream);
int tcvn_occlusion_mark(const int32_t* index, int64_t n_variants, int batch, int max_prongs, int grid_h, int grid_w, uint8_t* evaluated,
                        void* stream);
int tcvn_occlusion_occupancy(const int32_t* coords, int64_t nnz, int n_img, int height, int width, int tile_h, int tile_w,
                             const int32_t* img_bs, int batch, int max_prongs, uint8_t* occupied, void* stream);
int tcvn_occlusion_paint(int levels, const float* const* heat, const uint8_t* const* evaluated, const int32_t* grid_h,
                         const int32_t* grid_w, const uint8_t* occupied, int batch, int max_prongs, float* out, void* stream);

/* Deletion / insertion curves (forward only, eval arithmetic): how faithful a relevance map [batch, 1 + max_prongs, grid_h, grid_w] is.
 * Per map: the n tiles that hold a hit are ranked by relevance, descending, ties by the tile index ty * grid_w + tx, ascending (-0.0
 * counts as +0.0; the values are expected to be finite).  Step k = 0..steps uses m_k = (k * n + steps - 1) / steps tiles (integers):
 * the deletion variant k is the map without the hits of its m_k first tiles, the insertion variant k the map with only those hits;
 * all other hits keep their order.  A map with at least one hit gives exactly steps + 1 variants, a map without hits none.
 *   curve_variants  the hit list of tcvn_occlusion_variants and relevance -> the V variants ordered by (image, k): vimg [V] the image,
 *               index [V, 4] = (img_bs[image][0], img_bs[image][1], k, m_k); both need room for n_img * (steps + 1) rows.  rank
 *               [batch, 1 + max_prongs, grid_h, grid_w]: the rank of every occupied tile of this list's maps is written at (b, s) =
 *               img_bs[image]; the caller fills it with -1 first and may call once per hit list.  One workgroup per map sorts 64-bit
 *               keys (descending-orderable float pattern, tile index) in LDS: grid_h * grid_w <= TCVN_CURVE_MAX_TILES.  host_out
 *               (4 + ceil(n_img * (steps + 1) / max_pass) + 1 words), the two flags, the pass boundaries and the one synchronisation
 *               are those of tcvn_occlusion_variants.
 *   curve_build_pass  tcvn_occlusion_build_pass for these variants: a hit survives iff (rank of its tile < m_k) != (mode is deletion).
 *               The result goes through the embedder and tcvn_head_occlusion unchanged (the latter reads index[j][0:2] only).
 *   curve       curve [batch, 1 + max_prongs, steps + 1]: the softmax probability (double precision, as the heat map) of the target
 *               class at every step, from step_event_logits [V, Ce] / step_prong_logits [V, max_prongs, Cp]; auc [batch, 1 +
 *               max_prongs] = (p_0 / 2 + p_1 + ... + p_{steps-1} + p_steps / 2) / steps, summed in that order.  target and classes as
 *               in tcvn_occlusion_heatmap.  Rows without variants are NaN in both (and row s = 0 with TCVN_OCC_TARGET_PRONG).
 * Argument errors (NULL, tile < 1, steps outside 1..TCVN_CURVE_MAX_STEPS, more than TCVN_CURVE_MAX_TILES tiles per map, unknown mode,
 * max_pass outside 1..TCVN_OCC_MAX_PASS, workspace too small) return non-zero before any device call and print one "tcvn:" line. */
#define TCVN_CURVE_MAX_STEPS 64
#define TCVN_CURVE_MAX_TILES 4096
#define TCVN_CURVE_DELETION 0
#define TCVN_CURVE_INSERTION 1
int64_t tcvn_occlusion_curve_workspace_bytes(int n_img, int height, int width, int tile_h, int tile_w, int steps, int max_pass);
int tcvn_occlusion_curve_variants(const int32_t* coords, int64_t nnz, int n_img, int height, int width, int tile_h, int tile_w,
                                  const int32_t* img_bs, const float* relevance, int batch, int max_prongs, int steps, int mode,
                                  int32_t* rank, int max_pass, int32_t* vimg, int32_t* index, void* workspace,
                                  int64_t workspace_bytes, int64_t* host_out, int64_t host_cap, void* stream);
int tcvn_occlusion_curve_build_pass(const int32_t* coords, const float* values, int64_t nnz, int channels, int n_img, int height,
                                    int width, int tile_h, int tile_w, int steps, int mode, int max_pass, const int32_t* vimg,
                                    const void* workspace, int64_t workspace_bytes, int first, int count, int32_t* out_coords,
                                    float* out_values, int64_t out_rows, void* stream);
int tcvn_occlusion_curve(const float* event_logits, const float* prong_logits, const float* step_event_logits,
                         const float* step_prong_logits, const int32_t* index, int64_t n_variants, int batch, int max_prongs,
                         int event_classes, int prong_classes, int steps, int target, const int32_t* classes, float* curve, float* auc,
                         void* stream);

/* Tile Shapley values (forward only, eval arithmetic): the class score of a pixel map shared among its tiles.  For a scanned map (b, s)
 * the players are its n tiles that hold at least one hit inside the map, tile index t = ty * grid_w + tx.  A coalition C is the map with
 * only the hits of the tiles in C (all other hits removed, the survivors keep their order); every other token of event b stays as in the
 * forward being explained, the replacement tcvn_occlusion_build_pass makes.  v(C) is the softmax probability (TCVN_SHAP_VALUE_PROB, double
 * precision) or the raw logit (TCVN_SHAP_VALUE_LOGIT) of the target class under that variant; v(all) is taken from the logits of the
 * forward itself, v(empty) is one variant per map.
 *   exact    1 <= n <= max_exact (0..TCVN_TSHAP_MAX_EXACT): all coalitions but the full one are variants, numbered k = 0 .. 2^n - 2, bit i
 *            of k being the i-th occupied tile in ascending tile index.  phi[t] = sum over C without t of |C|! (n-|C|-1)! / n! *
 *            (v(C + t) - v(C)), stderr = 0.
 *   sampled  n > max_exact: `samples` (1..TCVN_TSHAP_MAX_SAMPLES) permutations.  Permutation m of map (b, s) is its occupied tiles sorted
 *            by (key, t), key = word 0 of the Philox-4x32-10 of the dropout masks at counter (t, m, b * (1 + max_prongs) + s, 0x54534850)
 *            under (seed & 0xffffffff, seed >> 32).  Variants: the empty map, then for every m the prefixes of length 1 .. n - 1.
 *            phi[t] = mean over m of v(prefix up to and including t) - v(prefix before t); stderr[t] = the sample standard deviation of
 *            those contributions / sqrt(samples), 0 for samples = 1.
 * A map contributes 2^n - 1 (exact) or 1 + samples * (n - 1) (sampled) variants, a map without hits none.  In both modes sum_t phi[t] =
 * v(all) - v(empty): it telescopes per permutation.
 *   shapley_variants  the hit list of tcvn_occlusion_variants -> the V variants ordered by (image, m, k): vimg [V] the image, index [V, 4] =
 *            (img_bs[image][0], img_bs[image][1], m, k): exact maps m = 0 and k the coalition number; sampled maps (0, 0) the empty map and
 *            (m, k), k >= 1, prefix k of permutation m.  Both need room for n_img * max(2^max_exact - 1, 1 + samples * (grid_h * grid_w - 1))
 *            rows; host_out has 4 + ceil(that / max_pass) + 1 words with the meaning, the two flags and the one synchronisation of
 *            tcvn_occlusion_variants.  At (b, s) = img_bs[image] the call writes permutations [batch, 1 + max_prongs, samples, grid_h *
 *            grid_w] (the n tiles of permutation m in front, -1 behind; drawn for every map that holds a hit, whichever its mode), n_tiles
 *            [batch, 1 + max_prongs] = n and exact [batch, 1 + max_prongs] = (1 <= n <= max_exact).  The caller fills them with -1, -1 and
 *            0 first and may call once per hit list.  One workgroup per (map, m) sorts the 64-bit words (key << 32 | t) in LDS: grid_h *
 *            grid_w <= TCVN_TSHAP_MAX_TILES.  The workspace holds the rank of every tile in every permutation (n_img x samples x tiles
 *            16-bit words) and the hit counts of every prefix.
 *   shapley_build  tcvn_occlusion_build_pass for these variants: a hit survives iff its tile's bit is set in k (exact) or its tile stands
 *            in front of position k of permutation m (sampled).  The result goes through the embedder and tcvn_head_occlusion unchanged.
 *   shapley_values  the base logits, the variants' logits coalition_event_logits [V, Ce] / coalition_prong_logits [V, max_prongs, Cp], index
 *            (ordered by map; the lists of several calls merged), exact, n_tiles and permutations -> phi and std_err float32 [batch, 1 +
 *            max_prongs, grid_h, grid_w], full = v(all) and empty = v(empty) float64 [batch, 1 + max_prongs].  target and classes as in
 *            tcvn_occlusion_heatmap.  phi and std_err are 0 at tiles without hits of scanned maps (a map with n = 0 is all 0, and its empty
 *            = full); all four are NaN where n_tiles < 0 (padded slots, maps not scanned) and in row s = 0 with TCVN_OCC_TARGET_PRONG.
 *            The exact weights are an fp64 table, every sum is taken in double in a fixed order and rounded to float32 once; there is no
 *            floating-point atomic.  scratch: 8 * (batch * (1 + max_prongs) + n_variants) bytes.
 * Argument errors (NULL, tile < 1, samples, max_exact or the tiles per map out of range, max_pass outside 1..TCVN_OCC_MAX_PASS, workspace
 * or scratch too small) return non-zero before any device call and print one "tcvn:" line. */
#define TCVN_TSHAP_MAX_TILES 1024
#define TCVN_TSHAP_MAX_SAMPLES 256
#define TCVN_TSHAP_MAX_EXACT 10
int64_t tcvn_occlusion_shapley_workspace_bytes(int n_img, int height, int width, int tile_h, int tile_w, int samples, int max_exact,
                                               int max_pass);
int tcvn_occlusion_shapley_variants(const int32_t* coords, int64_t nnz, int n_img, int height, int width, int tile_h, int tile_w,
                                    const int32_t* img_bs, int batch, int max_prongs, int samples, int max_exact, uint64_t seed,
                                    int32_t* permutations, int32_t* n_tiles, int32_t* exact, int max_pass, int32_t* vimg, int32_t* index,
                                    void* workspace, int64_t workspace_bytes, int64_t* host_out, int64_t host_cap, void* stream);
int tcvn_occlusion_shapley_build(const int32_t* coords, const float* values, int64_t nnz, int channels, int n_img, int height, int width,
                                 int tile_h, int tile_w, int samples, int max_exact, int max_pass, const int32_t* vimg,
                                 const void* workspace, int64_t workspace_bytes, int first, int count, int32_t* out_coords,
                                 float* out_values, int64_t out_rows, void* stream);
int tcvn_occlusion_shapley_values(const float* event_logits, const float* prong_logits, const float* coalition_event_logits,
                                  const float* coalition_prong_logits, const int32_t* index, int64_t n_variants, const int32_t* exact,
                                  const int32_t* n_tiles, const int32_t* permutations, int batch, int max_prongs, int event_classes,
                                  int prong_classes, int grid_h, int grid_w, int samples, int target, const int32_t* classes, int value,
                                  float* phi, float* std_err, double* full, double* empty, void* scratch, int64_t scratch_bytes,
                                  void* stream);

/* Detector-effect scans (forward only, eval arithmetic): how a prediction moves when the hits are not those of the detector the training
 * sample assumed.  A variant is a map whose hits went through one effect; unlike the occlusion variants it transforms coordinates and
 * values.  One effect acts on every hit (y, x, v[0..channels)) of the map (b, s) = img_bs[image] in this order -- the detector acts, then
 * the window moves --:
 *   1. drop       u = (philox4(y * width + x, b, s, 0x44455453, seed & 0xffffffff, seed >> 32).x >> 8) * 2^-24 (the Philox-4x32-10 of
 *                 the dropout masks); the hit is removed iff drop > 0 and u < drop.  The draw belongs to the original pixel of the map:
 *                 two hits on one pixel share it, and neither the hit's position in the list nor the pass enters.
 *   2. dead       removed iff dead_y0 <= y < dead_y1 or dead_x0 <= x < dead_x1 (original coordinates; the empty range 0, 0 is "none").
 *   3. scale      v[c] = v[c] * scale, one fp32 multiplication on the raw list value (before the embedder's log_pixels transform).
 *   4. threshold  only if threshold > 0: every v[c] < threshold becomes 0, and a hit whose channels are all 0 afterwards is removed.
 *   5. shift      y += shift_y, x += shift_x; a hit that leaves [0, height) x [0, width) is removed.
 * The hits that survive keep their order (duplicate coordinates: the highest index wins, as in the embedders).
 *   detector_variants  the hit list of tcvn_occlusion_variants and n_effects effects (host array, copied into the launch arguments: it is
 *               not read after the call returns) -> rows (image, k), a row being a variant iff its image holds a hit inside the map (a
 *               variant may be an empty map).  The V variants are ordered by (image, k): vimg [V] the image, index [V, 4] =
 *               (img_bs[image][0], img_bs[image][1], k, surviving hits); both need room for n_img * n_effects rows.  The surviving hits
 *               are counted by one thread per hit looping over the effects (integer atomics: deterministic).  host_out (4 +
 *               ceil(n_img * n_effects / max_pass) + 1 words), the two flags, the pass boundaries and the one synchronisation are
 *               those of tcvn_occlusion_variants.  The effects are kept in the workspace for the build passes.
 *   detector_build_pass  the hit lists of variants first .. first + count - 1: out_coords [rows, 3] = (variant's index inside the pass,
 *               y + shift_y, x + shift_x), out_values [rows, channels] the transformed values.  The count and the build evaluate the
 *               same device function per hit and effect.  The result goes through the embedder and (one token replaced)
 *               tcvn_head_occlusion unchanged; the latter reads index[j][0:2] only.
 *   detector_response  prob = softmax(varied)[c], delta = prob - softmax(base)[c] (double precision, stored as fp32) and flipped uint8 =
 *               (arg max of the varied row != arg max of the base row); target and classes as in tcvn_occlusion_heatmap.
 *               TCVN_DET_SCOPE_MAP: varied_event_logits [V, Ce], varied_prong_logits [V, max_prongs, Cp] and index [V, 4] as above;
 *               outputs [n_effects, batch, 1 + max_prongs], written at (k, b, s) of every variant.  TCVN_DET_SCOPE_EVENT: varied_event_logits
 *               [n_effects, batch, Ce], varied_prong_logits [n_effects, batch, max_prongs, Cp], index unused; outputs [n_effects, batch]
 *               with TCVN_OCC_TARGET_EVENT, [n_effects, batch, max_prongs] with TCVN_OCC_TARGET_PRONG: every slot p with
 *               valid[b * (1 + max_prongs) + 1 + p] >= 0 against its own predicted class.  Every other entry is NaN (flipped 0).  No
 *               atomics: one thread per entry.
 * Argument errors (NULL, n_effects outside 1..TCVN_DET_MAX_EFFECTS, an effect with a negative or non-finite scale / threshold, drop
 * outside [0, 1], a dead range outside 0 <= lo <= hi <= dimension or |shift| > 32767, max_pass outside 1..TCVN_OCC_MAX_PASS, unknown
 * scope or target, workspace too small) return non-zero before any device call and print one "tcvn:" line. */
#define TCVN_DET_MAX_EFFECTS 64
#define TCVN_DET_SCOPE_EVENT 0
#define TCVN_DET_SCOPE_MAP 1
typedef struct tcvn_detector_effect {
    float scale, threshold, drop;
    int32_t dead_y0, dead_y1, dead_x0, dead_x1, shift_y, shift_x;
    uint64_t seed;
} tcvn_detector_effect;
int64_t tcvn_detector_workspace_bytes(int n_img, int n_effects, int max_pass);
int tcvn_detector_variants(const int32_t* coords, int64_t nnz, int n_img, int height, int width, int channels, const float* values,
                           const int32_t* img_bs, const tcvn_detector_effect* effects, int n_effects, int max_pass, int32_t* vimg,
                           int32_t* index, void* workspace, int64_t workspace_bytes, int64_t* host_out, int64_t host_cap, void* stream);
int tcvn_detector_build_pass(const int32_t* coords, const float* values, int64_t nnz, int channels, int n_img, int height, int width,
                             const int32_t* img_bs, int n_effects, int max_pass, const int32_t* vimg, const void* workspace,
                             int64_t workspace_bytes, int first, int count, int32_t* out_coords, float* out_values, int64_t out_rows,
                             void* stream);
int tcvn_detector_response(const float* event_logits, const float* prong_logits, const float* varied_event_logits,
                           const float* varied_prong_logits, const int32_t* index, int64_t n_variants, const int32_t* valid, int batch,
                           int max_prongs, int event_classes, int prong_classes, int n_effects, int scope, int target,
                           const int32_t* classes, float* prob, float* delta, uint8_t* flipped, void* stream);

/* Predictive uncertainty: Monte-Carlo dropout (forward only; nothing here changes a parameter, a buffer or a running statistic).
 * A third run mode beside "train" and "eval": EVAL statistics, dropout DRAWN.  An _mc forward is the train = 0 forward of the same
 * plan (BatchNorm on running statistics, no pixel noise, no statistics partials, no keep-flag output, no running-stat update, the same
 * kernel choices) except that every dropout site applies the mask of (seed, stream id, element) with the plan's dropout probability --
 * the masks tcvn_dropout_keep reports.  It counts as an eval-mode forward for what follows: taps work, tcvn_head_attention may export
 * it, a backward is not defined after it.  With dropout = 0 it is the eval forward, bit for bit.
 *   densenet_forward_mc   workspace: tcvn_densenet_workspace_bytes(p, n_img, 0).  resume = 0: a whole forward.  resume != 0: starts at
 *               dense block 1, layer 0, on what the last forward left in `workspace` (no dropout site lies in front of the first 3x3
 *               convolution; the stem's output channels, the packed weights and the BatchNorm tables are written by no later launch of
 *               an eval pass).  Accepted only if the plan's last forward ran on this workspace with train = 0 (plain or _mc) and the
 *               same n_img, coords, values, nnz and log_pixels, and no tcvn_densenet_bind came between; otherwise one "tcvn:" line,
 *               non-zero, no launch.  The caller must not have changed the bound parameters or the hit list in between.
 *   head_forward_mc       tcvn_head_forward in this mode, on either encoder path.
 *   rows_bn_prelu_forward_mc   tcvn_rows_bn_prelu_forward on running statistics (never written) with dropout drop_p in [0, 1) drawn.
 *   mc_dropout_stats      sample_logits [n_samples, rows, classes] fp32 -> per row, with p_t = softmax(sample t) in double precision
 *               (max-subtracted), natural logarithms and 0 ln 0 = 0:
 *                 mean_prob[c] = 1/T sum_t p_t[c];  std_prob[c] = sqrt(sum_t (p_t[c] - mean_prob[c])^2 / (T - 1)), 0 at T = 1;
 *                 entropy = -sum_c mean_prob[c] ln mean_prob[c];  expected_entropy = 1/T sum_t H(p_t);
 *                 mutual_info = max(entropy - expected_entropy, 0);  votes[c] = the share of samples whose arg max is c (ties: the
 *                 lowest class).
 *               mean_prob, std_prob, votes [rows, classes]; entropy, expected_entropy, mutual_info [rows].  valid [rows] int32 or NULL:
 *               rows with valid[r] < 0 (padded prong slots) are NaN in every output.  One wave per row, its lanes stride over the
 *               samples; sums in a fixed order without atomics (two runs agree bit for bit), rounded to fp32 once.
 *               Argument errors (NULL other than valid, n_samples < 1, classes outside 1..TCVN_MC_MAX_CLASSES) return non-zero before
 *               any launch and print one "tcvn:" line. */
#define TCVN_MC_MAX_CLASSES 256
int tcvn_densenet_forward_mc(tcvn_densenet* p, int n_img, const int32_t* coords, const float* values, int64_t nnz, int log_pixels,
                             float* out, int64_t out_ld, void* workspace, int64_t workspace_bytes, uint64_t seed, int resume,
                             void* stream);
int tcvn_head_forward_mc(tcvn_head* p, int batch, int max_prongs, int n_prongs, const float* rows, const int32_t* tok_row,
                         float* event_logits, float* prong_logits, void* workspace, int64_t workspace_bytes, uint64_t seed,
                         void* stream);
int tcvn_rows_bn_prelu_forward_mc(const float* x, int64_t ldx, int rows, int channels, const float* gamma, const float* beta,
                                  const float* slope, const float* running_mean, const float* running_var, float* y, int64_t ldy,
                                  float drop_p, uint64_t seed, uint32_t stream_id, void* stream);
int tcvn_mc_dropout_stats(const float* sample_logits, const int32_t* valid, int n_samples, int rows, int classes, float* mean_prob,
                          float* std_prob, float* entropy, float* expected_entropy, float* mutual_info, float* votes, void* stream);

/* Hit gradients: the gradient of an embedder output with respect to the raw values of the hits, through the eval-mode model.
 * With running statistics a BatchNorm is a per-channel affine map, so its data gradient dx = sc*dU + P*x + Q loses the batch terms
 * (P = Q = 0) and the backward of the eval pass is the training backward's data-gradient chain with the links left out.
 *   densenet_forward_frozen   the eval forward (running statistics, no dropout whatever cfg.dropout is, no pixel noise, no running-stat
 *               update, nothing added to num_batches_tracked) in a workspace of tcvn_densenet_workspace_bytes(p, n_img, 1), on the
 *               dense stem and the layer paths that keep what a backward reads.  Same `out` as tcvn_densenet_forward with train = 0
 *               up to the kernel choice (bit-identical in fp32 mode).  log_pixels = 3 (one-hot: class indices have no gradient) is
 *               refused.  `coords` and `values` must stay valid and unchanged until input_gradient has run.
 *   densenet_input_gradient   d_out [n_img, out_dim] -> d_values [nnz, in_ch] fp32 = d <d_out, out> / d values of that forward's list.
 *               Every entry is written exactly once, without atomics: an entry outside the maps and an entry that does not own its
 *               pixel (duplicate coordinates: the highest list index owns it) get exactly 0; two calls agree bit for bit.  No
 *               parameter gradient is formed or delivered: the bound grad pointers are not touched and may be NULL.  Accepted only
 *               if the plan's last forward was a frozen one of n_img maps on this workspace; tcvn_densenet_backward and a
 *               tcvn_densenet_forward_mc resume are refused after a frozen forward.  Refusals: one "tcvn:" line, non-zero, no launch.
 *   head_forward_frozen   tcvn_head_forward with train = 0 (the token path keeps its backward state in every forward), noted as the
 *               forward that head_input_gradient may follow on this workspace.
 *   head_input_gradient   the logit seeds -> d_rows [batch + n_prongs, in_dim], as tcvn_head_backward returns it, through the reverse
 *               schedule with dropout probability 0 at every site, the running-statistics form of every LinearBlock's BatchNorm1d and no
 *               parameter gradient (no dW / db / LayerNorm-gradient launch; grad pointers may be NULL), on whichever encoder path the
 *               forward took.  Accepted only while the plan's last call that writes a workspace was a head_forward_frozen of the same
 *               shape on this workspace that came through (any forward, stage entry or scan of the plan drops the note before its first
 *               launch; further head_input_gradient calls with other seeds keep it); tcvn_head_backward on that workspace is refused
 *               until then.
 *   hit_gradient_gather   the last stage alone: e0 [n_img, Hc, Wc, init_ch] (mode: TCVN_MODE_F32 / _BF16 elements, row pitch lde), the
 *               gradient with respect to the conv0 output (7x7, stride 2, pad 3; Hc = (height - 1) / 2 + 1), and conv0_weight
 *               [init_ch, in_ch, 7, 7] fp32 ->
 *                 d_values[h, c] = pre'(v[h, c]) * sum over the <= 16 outputs (oy, ox) whose window holds the hit, and over co, of
 *                                  e0[img, oy, ox, co] * conv0_weight[co, c, y + 3 - 2 oy, x + 3 - 2 ox],
 *               pre' = 1/255 (value_mode 0), 1/(v + 1) (1), 1 (2); sums in double, rounded to fp32 once.  in_ch <= 4.  The workspace
 *               (hit_gradient_workspace_bytes) holds the duplicate record, built as a forward builds it.
 *   ig_scale / ig_accumulate / ig_finish   integrated gradients along alpha * v: out = alpha * v; acc (double) += weight * grad;
 *               attr = (float)(acc * v).  Element-wise over `count` values. */
int tcvn_densenet_forward_frozen(tcvn_densenet* p, int n_img, const int32_t* coords, const float* values, int64_t nnz, int log_pixels,
                                 float* out, int64_t out_ld, void* workspace, int64_t workspace_bytes, void* stream);
int tcvn_densenet_input_gradient(tcvn_densenet* p, int n_img, const float* d_out, int64_t d_out_ld, float* d_values, void* workspace,
                                 int64_t workspace_bytes, void* stream);
int tcvn_head_forward_frozen(tcvn_head* p, int batch, int max_prongs, int n_prongs, const float* rows, const int32_t* tok_row,
                             float* event_logits, float* prong_logits, void* workspace, int64_t workspace_bytes, void* stream);
int tcvn_head_input_gradient(tcvn_head* p, int batch, int max_prongs, int n_prongs, const float* rows, const int32_t* tok_row,
                             const float* d_event_logits, const float* d_prong_logits, float* d_rows, void* workspace,
                             int64_t workspace_bytes, void* stream);
int64_t tcvn_hit_gradient_workspace_bytes(int n_img, int height, int width, int in_ch);
int tcvn_hit_gradient_gather(int mode, const int32_t* coords, const float* values, int64_t nnz, int n_img, int height, int width,
                             int in_ch, int value_mode, const void* e0, int64_t lde, int init_ch, const float* conv0_weight,
                             float* d_values, void* workspace, int64_t workspace_bytes, void* stream);
/* seed [rows, n_classes] = d score / d logits for the score of class classes[r] of every row: value_kind 1 (TCVN_SHAP_VALUE_LOGIT) the logit
 * (a one-hot row), 0 (TCVN_SHAP_VALUE_PROB) its softmax probability (the Jacobian row p_t (delta_ct - p_c), formed in double precision,
 * max-subtracted).  classes[r] < 0, a padded slot, gives a zero row. */
int tcvn_hit_gradient_seed(const float* logits, const int32_t* classes, int rows, int n_classes, int value_kind, float* seed, void* stream);
int tcvn_ig_scale(const float* values, float alpha, float* out, int64_t count, void* stream);
int tcvn_ig_accumulate(double* acc, const float* grad, double weight, int64_t count, void* stream);
int tcvn_ig_finish(const double* acc, const float* values, float* attr, int64_t count, void* stream);
/* Noise-averaged hit gradients (SmoothGrad, SmoothGrad^2, VarGrad; csrc/noise_tunnel.hip): T noisy copies of a hit list, R of them per
 * frozen pass as one list over R * n_img images, and the running statistics of their gradients.  img_bs [n_img, 2] int32 = (event b, token
 * slot s) of every image of the list, s = 0 the event's own map and 1 + p prong slot p; an image whose pair lies outside
 * [batch, 1 + max_prongs] is left alone.  Entries outside the maps (tcvn hit rule: image, y or x out of range) are ignored by noise_sigma and
 * copied unperturbed by noise_replicate.
 *   noise_sigma      sigma[b * (1 + max_prongs) + s] = (float)(noise * ((double)max(0, max v) + (double)max(0, -min v))), max and min over
 *               every value channel of every entry inside that map (a NaN value moves neither); a map without hits gets 0.  Slots that no
 *               image names are not written: the caller pre-fills them.  Integer atomics on the sign-split values: exact and deterministic.
 *               The workspace (noise_workspace_bytes) holds the two bounds per image.
 *   noise_replicate  samples t0 .. t0 + reps - 1: coords_out[r * nnz + i] = (img + r * n_img, y, x) -- an image index outside 0 .. n_img - 1
 *               is written as -1, so that it stays outside in every sample -- and values_out[r * nnz + i][c] =
 *               (float)max((double)v + (double)sigma * z, 0) with z the draw of (sample t0 + r, pixel q = y * width + x, map m =
 *               b * (1 + max_prongs) + s, channel c): Philox-4x32-10 with counters (q, m, t, 0x4e54554e + (c >> 2)) and key (seed lo, seed hi)
 *               yields w0..w3; channel pair (c & 3) >> 1 takes (wa, wb) = (w0, w1) or (w2, w3); u1 = (wa + 1) 2^-32, u2 = wb 2^-32;
 *               z = sqrt(-2 ln u1) cos(2 pi u2) for even c, sin for odd c, all in double.  Where sigma is 0 (noise 0, an empty range) or the
 *               entry lies outside the maps the values are copied bit for bit, negative ones included.  The draw depends on nothing but
 *               (t, q, m, c, seed): duplicates share it and every split into calls gives the same bits.  in_ch <= 16.
 *   noise_accumulate folds grads [reps, count] and the matching perturbed values [reps, count] (count = nnz * in_ch) of samples
 *               t0 .. t0 + reps - 1 into acc [4, count] doubles = (gradient mean, gradient M2, attribution mean, attribution M2), the
 *               attribution being gradient x value (exact in double), by Welford's update in ascending t; t0 = 0 starts from zero whatever
 *               acc holds.  One thread per element, no atomics; a call split at any t0 gives the bits of one call.
 *   noise_finish     acc after `samples` samples -> stats [6, count] fp32 = (mean, unbiased variance M2 / (samples - 1), mean square
 *               mean^2 + M2 / samples) of the gradient, then of the attribution; the variance is NaN at samples = 1. */
int64_t tcvn_noise_workspace_bytes(int n_img);
int tcvn_noise_sigma(const int32_t* coords, const float* values, int64_t nnz, int in_ch, int n_img, int height, int width,
                     const int32_t* img_bs, int batch, int max_prongs, double noise, float* sigma, void* workspace,
                     int64_t workspace_bytes, void* stream);
int tcvn_noise_replicate(const int32_t* coords, const float* values, int64_t nnz, int in_ch, int n_img, int height, int width,
                         const int32_t* img_bs, int batch, int max_prongs, const float* sigma, uint64_t seed, int t0, int reps,
                         int32_t* coords_out, float* values_out, void* stream);
int tcvn_noise_accumulate(double* acc, const float* grads, const float* values, int64_t count, int t0, int reps, void* stream);
int tcvn_noise_finish(const double* acc, int64_t count, int samples, float* stats, void* stream);

/* Row operators behind the holder modules' own forward() (forward only, fp32):
 *   y = x W^T + b (torch.nn.Linear layout; bias may be NULL)                      -- layers/prong_decoder.py:15-16
 *   y = dropout(prelu(batchnorm1d(x)))  with batch statistics + running-stat update when train != 0, running statistics
 *   otherwise; save_mean_rstd: 2*channels floats of scratch                        -- layers/prong_feature_embedding.py:25-33
 *   Option variants of the block (:11-21): gamma == beta == running_mean == running_var == NULL -> no BatchNorm1d (norm = Identity,
 *   options.linear_batch_norm False); slope == NULL -> ReLU (options.linear_prelu_activation False).  Same rules in the backward. */
int tcvn_linear_forward(const float* x, int64_t ldx, const float* weight, const float* bias, float* y, int64_t ldy, int rows,
                        int n_out, int n_in, void* stream);
int tcvn_rows_bn_prelu_forward(const float* x, int64_t ldx, int rows, int channels, const float* gamma, const float* beta,
                               const float* slope, float* running_mean, float* running_var, float* y, int64_t ldy,
                               float* save_mean_rstd, int train, float drop_p, uint64_t seed, uint32_t stream_id, void* stream);

/* Backward of the two row operators (used by the smart-feature MLP, layers/prong_feature_embedding.py:36-78, the only LinearBlocks
 * outside the head plan): dx = dy W (NULL to skip), dweight += dy^T x, dbias += colsum(dy) (either may be NULL);
 * BatchNorm1d(train statistics kept in save_mean_rstd by the forward) + PReLU + dropout backward, parameter gradients accumulated. */
int tcvn_linear_backward(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* weight, float* dx, int64_t lddx,
                         float* dweight, float* dbias, int rows, int n_out, int n_in, void* stream);
int tcvn_rows_bn_prelu_backward(const float* x, int64_t ldx, const float* dy, int64_t lddy, int rows, int channels, const float* gamma,
                                const float* beta, const float* slope, const float* save_mean_rstd, float* dx, int64_t lddx,
                                float* dgamma, float* dbeta, float* dslope, float drop_p, uint64_t seed, uint32_t stream_id, void* stream);

/* Softmax focal loss and its gradient w.r.t. the logits (trainers/neutrino_full_base_trainer.py:148-177):
 * event_targets [batch] int64, prong_targets [batch, max_prongs] int8 (-1 = padding).
 * losses[3] (device, fp32) = {total, event, prong}; accs[6]: {event accuracy, prong accuracy} + 4 floats of scratch;
 * d_event_logits [batch, event_classes], d_prong_logits [batch, max_prongs, prong_classes] = d(total)/d(logits). */
int tcvn_head_loss(tcvn_head* p, int batch, int max_prongs, const float* event_logits, const float* prong_logits,
                   const int64_t* event_targets, const int8_t* prong_targets, float* losses, float* accs,
                   float* d_event_logits, float* d_prong_logits, void* stream);
/* Backward of the last train-mode forward on the same workspace: logit gradients -> d_rows [batch + n_prongs, in_dim];
 * parameter gradients are ACCUMULATED into the bound grad pointers. */
int tcvn_head_backward(tcvn_head* p, int batch, int max_prongs, int n_prongs, const float* rows, const int32_t* tok_row,
                       const float* d_event_logits, const float* d_prong_logits, float* d_rows, void* workspace,
                       int64_t workspace_bytes, void* stream);

/* Stand-alone softmax focal loss of one logit matrix [rows, classes] (targets int64, < 0 = ignore):
 * out2 = {mean loss, accuracy}; d_logits = weight * d(mean loss)/d(logits). Single workgroup; rows up to a few thousand. */
int tcvn_focal_loss(const float* logits, const int64_t* targets, int rows, int classes, float gamma, float weight,
                    float* d_logits, float* out2, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Fused optimizer step over flat arenas (replaces torch.optim.AdamW.step over 782 tensors + clip_grad_norm_:
 * trainers/neutrino_base.py:88-152, train.py:140).  All pointers are device pointers of `n` fp32 elements.
 * --------------------------------------------------------------------------------------------------------------- */
/* out[0] = sum of squares of x (fp64 accumulation; partials: scratch of n_partials doubles, n_partials <= 1024 used). */
int tcvn_grad_sumsq(const float* x, int64_t n, double* partials, int n_partials, float* out, void* stream);
/* One AdamW step (decoupled weight decay).  weight_decay[i] < 0 freezes element i (parameter the reference's optimizer never
 * touches).  grad_sumsq (device, may be NULL) and clip > 0 apply the global-norm clip coefficient min(1, clip/(norm+1e-6))
 * to the gradient on the fly (the gradient arena itself is left as is).  step is 1-based. */
int tcvn_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, const float* weight_decay, int64_t n,
                    float lr, float beta1, float beta2, float eps, int64_t step, const float* grad_sumsq, float clip, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Validation aid: the dropout keep-scale (0 or 1/(1-p)) the kernels apply at one site, as a [rows, cols] fp32 tensor.
 * Masks are never stored: forward and backward recompute them from (seed, stream id, element).  kind 0: sites indexed by the
 * row-major element number (output block 0x4000, combined embedding 0x5000, encoder layer l 0x6000+8l+{0 attention
 * probabilities [B,H,S,S], 1 attention output, 2 FFN activation, 3 FFN output} [T,D], prong decoder 0x7000+i); kind 1: the
 * 3x3 convolution outputs of dense block b, layer l (stream id 64 b + l + 1; rows = pixels n*H*W, cols = growth).
 * The reference draws its masks from torch's global generator (layers/dense_net.py:29-40 via nn.Dropout); only the
 * distribution is comparable, so tests feed these masks to the CPU oracle.
 * --------------------------------------------------------------------------------------------------------------- */
int tcvn_dropout_keep(int kind, float p, uint64_t seed, uint32_t stream_id, int64_t rows, int cols, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------------------------
 * Measurement aid (bench.py roofline leg): when enabled, every convolution launch is bracketed by a HIP event pair on
 * its own stream.  tcvn_profile_get blocks on the record's end event; name is the kernel's label, flops the algorithmic
 * 2*M*N*K of that launch and bytes its algorithmic HBM traffic (operands once, results once).  Off by default; with a
 * filter set only the matching launches pay for their two events, which is cheap enough for the timed region.
 * --------------------------------------------------------------------------------------------------------------- */
/* tcvn_backward_overlap(1): backward runs the 3x3 weight-gradient kernels of the bf16 DenseNet (and the TN GEMMs of 1x1 layers the fused
 * backward kernel does not serve) on a plan-owned side stream beside the data-gradient chain (double-buffered EY, event-released).
 * OFF by default since round 4 (with the 1x1 backward fused into one kernel on the caller's stream the overlap no longer pays: same-box A/B
 * 19.55 against 19.55-19.60 ms/step); on by default in rounds 2-3 (-1.2 % then). */
void tcvn_backward_overlap(int on);
void tcvn_profile_enable(int on);
void tcvn_profile_filter(const char* label_substring); /* NULL or "" = every launch; else only matching kernel labels */
void tcvn_profile_reset(void);
int tcvn_profile_count(void);
int tcvn_profile_get(int i, char* name, int name_cap, float* ms, double* flops, double* bytes);

#ifdef __cplusplus
}
#endif
#endif /* TCVN_HIP_H */
