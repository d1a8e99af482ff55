// DenseNet backward driver: reverse schedule of densenet.hip::forward on the same workspace.
// Extra HBM state: G[b] (gradient accumulators shaped like the concat buffers), (P,Q) per channel, one bottleneck-sized
// scratch DU, a conv0-sized scratch DU0, fp32 kernel-layout weight gradients (converted to OIHW at the end).
#include <cstring>
#include <vector>

#include <cstdlib>
#include "densenet_plan.h"
#include "tcvn_rows.h"
#include "tcvn_input_grad.h"

using namespace tcvn;

// tcvn_backward_overlap(): the 3x3 weight gradients on a side stream beside the data-gradient chain.  ON by default in rounds 2-3 (26.0-26.1 ms
// against 26.4 ms when the side stream also carried the 1x1 TN GEMMs).  OFF by default since round 4: with the fused 1x1 backward kernel on the
// main stream only the 3x3 weight gradient is left to overlap, and the same-box A/B reads 19.55 ms/step serial against 19.55-19.60 with the side
// stream (19.8 when the fused kernel's slab reductions also went there) -- nothing to gain, and serial kernel timings are what profiles show.
static int g_backward_overlap = 0;
bool tcvn::backward_overlap_enabled() { return g_backward_overlap != 0; }
void tcvn::set_backward_overlap(int on) { g_backward_overlap = on; }

#ifdef TCVN_DEBUG_KNOBS
// Validation build: the (PY, QY) rows of dense layer (block, layer) -- one buffer that every layer of the backward pass overwrites -- are
// copied to `dst` ([2][bn_size * growth] floats on the device) on the backward's stream once that layer's norm2 link has been issued;
// dst == nullptr switches the tap off (tests/test_backward_link_rider_gpu.py).
static struct { int block, layer; float* dst; } g_pq_tap = {0, 0, nullptr};
extern "C" void tcvn_debug_pq_tap(int block, int layer, float* dst) { g_pq_tap = {block, layer, dst}; }
// Validation build: snapshots of the backward state around dense layer (block, layer), or around the block's transition / the head
// (layer == -1), for tests/test_densenet_layers_float64_gpu.py.  The buffers involved are reused layer after layer, so armed layers are
// copied device to device on the backward's stream into a caller-owned buffer: in front of the first launch G[block] and the block's
// (P, Q) rows; behind the last launch G[block] and (P, Q) again, DU, (PY, QY) and the layer's eff rows EY3 (where the layout has them).
// Sections in that order, each starting at a multiple of 256 bytes (tcvn_debug_layer_snapshot_report gives the total); a buffer that is
// too small is refused.  The report also says which 3x3 data-gradient kernel ran (Conv3x3Dgrad), whether the fused 1x1 backward ran and
// whether the data-gradient kernel filled EY3; tcvn_debug_layer_snapshot_grid gives the fused 1x1 backward's grid (row workgroups, 128-column
// slices; 0 row workgroups where it did not run).  The backward-overlap side stream must be off (the default).
struct LayerSnap { int block, layer; char* dst; long cap, bytes; int dgrad_kernel, fused1, ey_valid, nblk1, slices1; };
static std::vector<LayerSnap> g_snaps;
static struct { int dgrad_kernel, fused1, ey_valid, nblk1, slices1; } g_snap_path = {0, 0, 0, 0, 0};
extern "C" void tcvn_debug_layer_snapshot_clear(void) { g_snaps.clear(); }
extern "C" int tcvn_debug_layer_snapshot(int block, int layer, void* dst, int64_t cap) {
    if (!dst || cap <= 0) return -1;
    g_snaps.push_back(LayerSnap{block, layer, reinterpret_cast<char*>(dst), (long)cap, 0, 0, 0, 0, 0, 0});
    return (int)g_snaps.size() - 1;
}
extern "C" int tcvn_debug_layer_snapshot_report(int i, int* dgrad_kernel, int* fused1, int* ey_valid, int64_t* bytes) {
    if (i < 0 || i >= (int)g_snaps.size()) return -1;
    *dgrad_kernel = g_snaps[i].dgrad_kernel; *fused1 = g_snaps[i].fused1; *ey_valid = g_snaps[i].ey_valid; *bytes = g_snaps[i].bytes;
    return 0;
}
extern "C" int tcvn_debug_layer_snapshot_grid(int i, int* nblk, int* slices) {
    if (i < 0 || i >= (int)g_snaps.size()) return -1;
    *nblk = g_snaps[i].nblk1; *slices = g_snaps[i].slices1;
    return 0;
}
static int layer_snapshot(const DenseNetPlan& pl, const Step& s, int bi, int l, bool after) {
    for (LayerSnap& sn : g_snaps) {
        if (sn.block != bi || sn.layer != l) continue;
        const BlockGeom& bg = pl.blocks[bi];
        const int mid = pl.cfg.bn_size * pl.cfg.growth;
        const long M = (long)s.n * bg.H * bg.W;
        const long gb = round_up(M * bg.ld * pl.esz, 256), pb = round_up((long)bg.ld * 8, 256), db = round_up(M * mid * pl.esz, 256),
                   yb = round_up((long)mid * 8, 256), eb = round_up(M * 32 * pl.esz, 256);
        const bool ey = l >= 0 && !s.L.EY3[bi].empty();
        sn.bytes = 2 * (gb + pb) + db + yb + (ey ? eb : 0);
        if (sn.bytes > sn.cap) { fprintf(stderr, "tcvn: layer snapshot buffer too small (%ld < %ld)\n", sn.cap, sn.bytes); return -18; }
        char* d = sn.dst + (after ? gb + pb : 0);
        TCVN_CHECK(hipMemcpyAsync(d, s.ws + s.L.G[bi], (size_t)(M * bg.ld * pl.esz), hipMemcpyDeviceToDevice, s.st));
        TCVN_CHECK(hipMemcpyAsync(d + gb, s.ws + s.L.pqD[bi], (size_t)bg.ld * 8, hipMemcpyDeviceToDevice, s.st));
        if (!after || l < 0) continue;
        d = sn.dst + 2 * (gb + pb);
        TCVN_CHECK(hipMemcpyAsync(d, s.ws + s.L.du, (size_t)(M * mid * pl.esz), hipMemcpyDeviceToDevice, s.st));
        TCVN_CHECK(hipMemcpyAsync(d + db, s.ws + s.L.pqY, (size_t)mid * 8, hipMemcpyDeviceToDevice, s.st));
        if (ey) TCVN_CHECK(hipMemcpyAsync(d + db + yb, s.ws + s.L.EY3[bi][l], (size_t)(M * 32 * pl.esz), hipMemcpyDeviceToDevice, s.st));
        sn.dgrad_kernel = g_snap_path.dgrad_kernel; sn.fused1 = g_snap_path.fused1; sn.ey_valid = g_snap_path.ey_valid;
        sn.nblk1 = g_snap_path.nblk1; sn.slices1 = g_snap_path.slices1;
    }
    return 0;
}
#endif

namespace {
constexpr float kEps = 1e-5f;
constexpr long kSlabBytes = 48L << 20;      // per-workgroup partial weight gradients (<= 256 x 147 KB) and column sums
constexpr long kSlab1GemmBytes = 64L << 20; // fused 1x1 backward: per-workgroup [128][ldc] fp32 weight-gradient tiles, bias column sums behind them
constexpr long kSlab1Bytes = 68L << 20;
constexpr long kSlabGemmBytes = 44L << 20;  // GEMM slabs; the tail [44 MB, 48 MB) holds the bias column-sum partials (<= 1024 x 512 floats)
struct Bump {
    long off;
    long take(long bytes) { long o = off; off += round_up(bytes, 256); return o; }
};
}  // namespace

void DenseNetPlan::layout_bwd(int n, long start, long maxY, Layout& L) const {
    Bump b{start};
    const int mid = cfg.bn_size * cfg.growth;
    L.G.clear(); L.pqD.clear();
    // --- zeroed at the start of every backward: G, pqD, gwk (contiguous) ---
    long bpart = (long)std::max(pool0_bwd_grid(n, Hc, Wc), pool0_bwd_vec_grid(n, Hc, Wc)) * cfg.init_ch * 24;
    bpart = std::max(bpart, 1024L * cfg.init_ch * 24);              // sparse stem backward: <= 1024 workgroups
    bpart = std::max(bpart, (long)head_pool_bwd_grid(n) * Cf * 24);
    for (const auto& bg : blocks) {
        const long M = (long)n * bg.H * bg.W;
        L.G.push_back(b.take(M * bg.ld * esz));
        bpart = std::max(bpart, 512L * std::max(mid, bg.Ctot) * 24);
    }
    for (const auto& bg : blocks) L.pqD.push_back(b.take((long)bg.ld * 8));
    long gw = 0;
    for (const auto& e : wk_list())
        if (!e.transpose && !e.frag) gw += round_up((long)e.N * e.Kp * 4, 256);
    L.gwk = b.take(gw);
    L.zero_end = b.off;
    L.du = b.take(maxY * esz);
    L.ey = b.take(maxY * esz);
    L.ey2 = b.take(maxY * esz);                    // second EY buffer: the weight-gradient stream may still read the previous one
    L.slab = b.take(kSlabBytes);
    L.slab1 = cfg.mode == MODE_BF16 ? b.take(kSlab1Bytes) : -1;
    L.pqY = b.take((long)mid * 8);
    L.du0 = b.take((long)n * Hc * Wc * cfg.init_ch * esz);
    L.pq0 = b.take((long)cfg.init_ch * 8);
    L.bpart = b.take(bpart);
    L.dF = b.take((long)n * Cf * 4);
    L.dZ = b.take((long)n * cfg.out_dim * 4);
    L.EY3.clear();                                 // per dense layer: the 3x3 output gradient's eff rows, data gradient -> weight gradient
    for (const auto& bg : blocks) {
        std::vector<long> eys;
        if (cfg.mode == MODE_BF16 && cfg.growth == 32)
            for (int l = 0; l < bg.L; ++l) eys.push_back(b.take((long)n * bg.H * bg.W * 32 * esz));
        L.EY3.push_back(eys);
    }
    L.total = b.off;
}

bool DenseNetPlan::bwd1x1_fill(int bi, int l, long M, char* ws, const Layout& L, Bwd1x1Args& fa) const {
    static const bool no_fuse1 = TCVN_KNOB_SET("TCVN_NO_BWD1_FUSE");      // validation build: the three-kernel 1x1 backward (eff copy, TN GEMM, NT GEMM)
    const BlockGeom& bg = blocks[bi];
    const LayerSlots& ls = bg.layers[l];
    const int mid = cfg.bn_size * cfg.growth;
    if (no_fuse1 || L.XA[bi][l] < 0 || mid != 128 || L.slab1 < 0 || cfg.mode != MODE_BF16) return false;
    const Tab t1 = tab(ws, L, ls.n1);
    const WkEntry& etf = wk_find(ls.w1, 1, 1);
    fa = Bwd1x1Args{};
    fa.DU = ws + L.du; fa.Y = ws + L.Y[bi][l]; fa.PY = reinterpret_cast<float*>(ws + L.pqY); fa.QY = fa.PY + mid; fa.M = M;
    fa.Xin = ws + L.D[bi]; fa.ldx = bg.ld; fa.cin = ls.cin;
    fa.sc = t1.sc; fa.sh = t1.sh; fa.sl = data[ls.a1]; fa.Gout = ws + L.G[bi]; fa.ldg = bg.ld;
    fa.Wfrag = ws + L.wk + etf.off; fa.Kp = etf.Kp; fa.zeros = ws + L.zeros; fa.part = reinterpret_cast<double*>(ws + L.bpart);
    fa.slab = reinterpret_cast<float*>(ws + L.slab1); fa.slab_bytes = kSlab1GemmBytes; fa.ldc = wk_find(ls.w1, 0).Kp;
    fa.tail = reinterpret_cast<float*>(ws + L.slab1 + kSlab1GemmBytes);
    fa.nblk = bwd1x1_fused_nblk(fa);
    return bwd1x1_fused_ok(fa);
}

float* DenseNetPlan::gw_of(const Step& s, int slot) const {      // kernel-layout gradient offsets follow wk_list order (non-transposed entries only)
    long o = 0;
    for (const WkEntry& e : wk_cache) {
        if (e.transpose || e.frag) continue;
        if (e.slot == slot) return reinterpret_cast<float*>(s.ws + s.L.gwk + o);
        o += round_up((long)e.N * e.Kp * 4, 256);
    }
    return nullptr;
}

int DenseNetPlan::bwd_link(const Step& s, const BnSlots& bn, int nblk, const double* bstat, long count, float* P, float* Q, int acc, int a_slot) const {
    if (s.frozen) return 0;      // running statistics: the BatchNorm is a per-channel affine map, P = Q = 0 (zeroed by input_gradient) and no parameter gradient
    BnBwdLinkArgs a{s.part, nblk, bn.C, bstat, count, kEps, data[bn.w], grad[bn.w], grad[bn.b], grad[a_slot], P, Q, acc};
    return bn_bwd_link(a, s.st);
}

int DenseNetPlan::drain(Step& s) const {
    if (s.side_on && s.side_busy) {
        TCVN_CHECK(hipEventRecord(ev_drain, side_st));
        TCVN_CHECK(hipStreamWaitEvent(s.st, ev_drain, 0));
        s.side_busy = false;
    }
    s.seq = 0;
    return 0;
}

// Blocks [bi_lo, bi_hi] of the backward pass (bi_hi == last block: also the output block; bi_lo == 0: also the stem).  A caller that
// wants each block's parameter gradients as soon as they are final (data-parallel exchange overlapped with the rest of backward)
// walks the blocks from the last to the first; one call with (n_blocks - 1, 0) is the whole backward.
int DenseNetPlan::backward(int n, const float* d_out, long d_out_ld, char* ws, long ws_bytes, hipStream_t st, int bi_hi, int bi_lo) {
    if (!bound) return -11;
    if (bi_hi < 0) bi_hi = (int)blocks.size() - 1;
    if (bi_lo < 0 || bi_lo > bi_hi || bi_hi >= (int)blocks.size()) return -1;
    const bool first_part = bi_hi == (int)blocks.size() - 1, last_part = bi_lo == 0;
    if (n <= 0) return 0;
    if (n != last_n) { fprintf(stderr, "tcvn: densenet backward without matching forward\n"); return -13; }
    if (last_frozen) { fprintf(stderr, "tcvn: densenet backward after a frozen forward: only tcvn_densenet_input_gradient is defined there\n"); return -20; }
    for (size_t i = 0; i < slots.size(); ++i)
        if (slots[i].kind == TCVN_SLOT_PARAM && grad[i] == nullptr) { fprintf(stderr, "tcvn: grad of %s unbound\n", slots[i].name.c_str()); return -14; }
    Layout L;
    layout(n, true, L);
    if (ws_bytes < L.total) return -12;
    int rc;
    // Weight gradients (3x3 and 1x1, with their slab reductions) do not feed the data-gradient chain: in bf16 mode they run on a
    // side stream beside it.  Shared state: the slab (side stream only between drains), EY (double buffered, released by
    // ev_done), the bias column-sum partials (two halves of the slab tail).  tcvn_backward_overlap(0), the default, keeps everything on `st`.
    const bool side_on = fast3x3 && backward_overlap_enabled();
    if (side_on && (rc = ensure_side())) return rc;
    Step s{ws, L, st, n, true, last_seed, reinterpret_cast<double*>(ws + L.bpart), false, side_on, 0, false};

    // device table of unpack descriptors (depends on ws)
    if (undesc_ws != ws || undesc_total != L.total) {
        std::vector<UnpackDesc> ud;
        unpack_first.assign(blocks.size() + 1, 0);            // descriptors are in wk_list order: conv0, then block by block
        long o = 0;                                           // (as gw_of)
        for (const WkEntry& e : wk_cache) {
            if (e.transpose || e.frag) continue;
            for (size_t bi = 0; bi < blocks.size(); ++bi) {   // first descriptor of block bi = its first layer's conv1
                if (!blocks[bi].layers.empty() && e.slot == blocks[bi].layers[0].w1) unpack_first[bi] = (int)ud.size();
            }
            UnpackDesc d{reinterpret_cast<const float*>(ws + L.gwk + o), grad[e.slot], e.N, e.Cin, e.taps, e.Kp,
                         (fast3x3 && e.taps == 9) ? 1 : 0};
            ud.push_back(d);
            o += round_up((long)e.N * e.Kp * 4, 256);
        }
        n_unpack = (int)ud.size();
        unpack_first[blocks.size()] = n_unpack;
        if (!d_undesc) TCVN_CHECK(hipMalloc(&d_undesc, ud.size() * sizeof(UnpackDesc)));
        h_undesc.assign(reinterpret_cast<char*>(ud.data()), reinterpret_cast<char*>(ud.data()) + ud.size() * sizeof(UnpackDesc));
        TCVN_CHECK(hipMemcpyAsync(d_undesc, h_undesc.data(), h_undesc.size(), hipMemcpyHostToDevice, st));
        undesc_ws = ws; undesc_total = L.total;
    }

    if (first_part) {
        // Zeroed per backward: the (P, Q) tables and the kernel-layout weight gradients (one contiguous range behind the G buffers),
        // and those gradient buffers G[b] whose first contribution accumulates.  In the bf16 fast path the first writer of G[b] -- the
        // transition's pooled data gradient, or the head for the last block -- writes instead (g_write), which saves a 0.9 GB memset and
        // the read of it at B = 32 x 8 prongs; only the pixels no 2x2 window covers (odd map sizes) are zeroed explicitly.
        TCVN_CHECK(hipMemsetAsync(ws + L.pqD[0], 0, (size_t)(L.zero_end - L.pqD[0]), st));
        for (size_t bi = 0; bi + 1 < blocks.size(); ++bi) {
            const long bytes = (long)n * blocks[bi].H * blocks[bi].W * blocks[bi].ld * esz;
            if (L.XP[bi] >= 0 && cfg.mode == MODE_BF16) {
                if ((rc = zero_pool_remainder(ws + L.G[bi], blocks[bi].ld, n, blocks[bi].H, blocks[bi].W, blocks[bi + 1].H, blocks[bi + 1].W, st))) return rc;
            } else TCVN_CHECK(hipMemsetAsync(ws + L.G[bi], 0, (size_t)bytes, st));
        }
        if ((rc = bwd_output(s, d_out, d_out_ld))) return rc;
    }
    for (int bi = bi_hi; bi >= bi_lo; --bi) {
#ifdef TCVN_DEBUG_KNOBS
        if ((rc = layer_snapshot(*this, s, bi, -1, false))) return rc;
#endif
        if ((rc = bwd_transition(s, bi))) return rc;
#ifdef TCVN_DEBUG_KNOBS
        if ((rc = layer_snapshot(*this, s, bi, -1, true))) return rc;
#endif
        for (int l = blocks[bi].L - 1; l >= 0; --l) {
#ifdef TCVN_DEBUG_KNOBS
            if ((rc = layer_snapshot(*this, s, bi, l, false))) return rc;
#endif
            if ((rc = bwd_layer(s, bi, l))) return rc;
#ifdef TCVN_DEBUG_KNOBS
            if ((rc = layer_snapshot(*this, s, bi, l, true))) return rc;
#endif
        }
    }
    if ((rc = drain(s))) return rc;                // the stem weight gradient uses the slab; k_unpack reads every weight gradient
    if (last_part && (rc = bwd_stem(s))) return rc;
    // kernel-layout weight gradients of the blocks just finished -> reference OIHW gradients (conv0 rides with block 0)
    const int u0 = last_part ? 0 : unpack_first[bi_lo], u1 = unpack_first[bi_hi + 1];
    return unpack_wgrads(reinterpret_cast<const UnpackDesc*>(d_undesc) + u0, u1 - u0, st);
}

// Data-only backward of the last frozen forward (hit gradients).  With running statistics every BatchNorm is a per-channel affine map, so
// its data gradient dx = sc*dU + Px*x + Qx (bn_link.h) loses the two terms that come from batch statistics: the reverse schedule above runs
// with P = Q = 0 everywhere, without a link (launched or riding), with dropout probability 0 in every EffSrc, and without any launch or
// reduction that delivers a parameter gradient -- no 3x3 / 1x1 / stem weight gradient, no TN GEMM, no bias column sum, no k_unpack; the bound
// grad pointers are neither read nor written and may be null.  Where the weight gradient is part of a data-gradient kernel (the fused 1x1
// backward) it stays in that kernel's slabs.  The chain ends in DU0 = sc0 * prelu0'(u) * dz over the whole conv0 map (dense stem, no activity
// bitmap), which k_hit_gradient (input_grad.hip) takes through conv0 at the hits.
int DenseNetPlan::input_gradient(int n, const float* d_out, long d_out_ld, float* d_values, char* ws, long ws_bytes, hipStream_t st) {
    if (!bound) return -11;
    if (n <= 0) return 0;
    if (!last_frozen || last_ws != ws || n != last_n) {
        fprintf(stderr, "tcvn: densenet input_gradient: the last forward of this plan on this workspace was not a frozen forward of %d maps\n", n);
        return -21;
    }
    if (stem_path.sparse || stem_path.act_skip || last_coords == nullptr) return -16;
    Layout L;
    layout(n, true, L);
    if (ws_bytes < L.total) return -12;
    int rc;
    Step s{ws, L, st, n, true, last_seed, reinterpret_cast<double*>(ws + L.bpart), false, false, 0, false, false, true};
    // (P, Q) of every block (not the kernel-layout weight gradients behind them: nothing is delivered), (PY, QY) and (P0, Q0) -- the links
    // write the last two with acc = 0 in a training backward, so the per-backward memset does not cover them
    TCVN_CHECK(hipMemsetAsync(ws + L.pqD[0], 0, (size_t)(L.gwk - L.pqD[0]), st));
    TCVN_CHECK(hipMemsetAsync(ws + L.pqY, 0, (size_t)cfg.bn_size * cfg.growth * 8, st));
    TCVN_CHECK(hipMemsetAsync(ws + L.pq0, 0, (size_t)cfg.init_ch * 8, st));
    for (size_t bi = 0; bi + 1 < blocks.size(); ++bi) {      // G buffers whose first contribution accumulates: as backward()
        const long bytes = (long)n * blocks[bi].H * blocks[bi].W * blocks[bi].ld * esz;
        if (L.XP[bi] >= 0 && cfg.mode == MODE_BF16) {
            if ((rc = zero_pool_remainder(ws + L.G[bi], blocks[bi].ld, n, blocks[bi].H, blocks[bi].W, blocks[bi + 1].H, blocks[bi + 1].W, st))) return rc;
        } else TCVN_CHECK(hipMemsetAsync(ws + L.G[bi], 0, (size_t)bytes, st));
    }
    if ((rc = bwd_output(s, d_out, d_out_ld))) return rc;
    for (int bi = (int)blocks.size() - 1; bi >= 0; --bi) {
#ifdef TCVN_DEBUG_KNOBS
        if ((rc = layer_snapshot(*this, s, bi, -1, false))) return rc;
#endif
        if ((rc = bwd_transition(s, bi))) return rc;
#ifdef TCVN_DEBUG_KNOBS
        if ((rc = layer_snapshot(*this, s, bi, -1, true))) return rc;
#endif
        for (int l = blocks[bi].L - 1; l >= 0; --l) {
#ifdef TCVN_DEBUG_KNOBS
            if ((rc = layer_snapshot(*this, s, bi, l, false))) return rc;
#endif
            if ((rc = bwd_layer(s, bi, l))) return rc;
#ifdef TCVN_DEBUG_KNOBS
            if ((rc = layer_snapshot(*this, s, bi, l, true))) return rc;
#endif
        }
    }
    if ((rc = bwd_stem(s))) return rc;
    HitGradArgs h{};
    h.mode = cfg.mode; h.coords = last_coords; h.values = last_values; h.nnz = last_nnz; h.n_img = n; h.H = cfg.H; h.W = cfg.W; h.Cpix = cfg.in_ch;
    h.value_mode = last_value_mode; h.E0 = ws + L.du0; h.lde = cfg.init_ch; h.Hc = Hc; h.Wc = Wc; h.N = cfg.init_ch; h.W0 = data[s_w0];
    h.o = PixelOwners{reinterpret_cast<uint32_t*>(ws + L.own), (long)n * cfg.H * cfg.W};
    h.d_values = d_values;
    return hit_gradient(h, st);
}

// ---- output block backward: Dropout - PReLU - BatchNorm1d - Linear ----
int DenseNetPlan::bwd_output(const Step& s, const float* d_out, long d_out_ld) const {
    const Layout& L = s.L;
    float* F = reinterpret_cast<float*>(s.ws + L.F);
    float* Z = reinterpret_cast<float*>(s.ws + L.Z);
    float* dF = reinterpret_cast<float*>(s.ws + L.dF);
    float* dZ = reinterpret_cast<float*>(s.ws + L.dZ);
    float* hs = reinterpret_cast<float*>(s.ws + L.head_stat);
    int rc;
    if (s.frozen) {
        RowsBnFrozenBwdArgs f{Z, cfg.out_dim, d_out, d_out_ld, s.n, cfg.out_dim, data[nl.w], data[nl.b], data[s_al], data[nl.rm], data[nl.rv], kEps,
                              dZ, cfg.out_dim, 0};
        if ((rc = rows_bn_bwd_frozen(f, s.st))) return rc;
        return linear_bwd_dx(dZ, cfg.out_dim, data[s_wl], dF, Cf, s.n, cfg.out_dim, Cf, 0, s.st);
    }
    RowsBnBwdArgs r{};
    r.X = Z; r.ldx = cfg.out_dim; r.dY = d_out; r.lddy = d_out_ld; r.R = s.n; r.C = cfg.out_dim;
    r.gamma = data[nl.w]; r.beta = data[nl.b]; r.slope = data[s_al]; r.save_mean = hs; r.save_rstd = hs + cfg.out_dim;
    r.dX = dZ; r.lddx = cfg.out_dim; r.dgamma = grad[nl.w]; r.dbeta = grad[nl.b]; r.dslope = grad[s_al];
    r.drop_p = cfg.dropout; r.seed = s.seed; r.stream_id = 0x4000u;
    if ((rc = rows_bn_bwd(r, s.st))) return rc;
    if ((rc = linear_bwd_dw(dZ, cfg.out_dim, F, Cf, grad[s_wl], nullptr, s.n, cfg.out_dim, Cf, s.st))) return rc;
    return linear_bwd_dx(dZ, cfg.out_dim, data[s_wl], dF, Cf, s.n, cfg.out_dim, Cf, 0, s.st);
}

// ---- transition: BN - PReLU - (pool commuted) - 1x1 conv, output = first channels of block bi+1; last block: final_norm + global average ----
int DenseNetPlan::bwd_transition(Step& s, int bi) const {
    const Layout& L = s.L;
    const BlockGeom& bg = blocks[bi];
    const int mode = cfg.mode;
    const long M = (long)s.n * bg.H * bg.W;
    char* D = s.ws + L.D[bi];
    char* G = s.ws + L.G[bi];
    float* P = reinterpret_cast<float*>(s.ws + L.pqD[bi]);
    float* Q = P + bg.ld;
    const double* bstatD = reinterpret_cast<const double*>(s.ws + L.bstatD[bi]);
    int rc;
    if (!bg.has_trans) {
        const Tab t = tab(s.ws, L, nf);
        HeadPoolBwdArgs a{mode, D, bg.ld, s.n, bg.H * bg.W, Cf, t.sc, t.sh, data[s_af], reinterpret_cast<float*>(s.ws + L.dF), G, bg.ld, s.part,
                          head_pool_bwd_grid(s.n)};
        if ((rc = head_pool_bwd(a, s.st))) return rc;
        return bwd_link(s, nf, a.nblk, bstatD, M, P, Q, 1, s_af);
    }
    const BlockGeom& nb = blocks[bi + 1];
    const long Mn = (long)s.n * nb.H * nb.W;
    const int Nt = bg.Ctot / 2;
    float* Pn = reinterpret_cast<float*>(s.ws + L.pqD[bi + 1]);
    float* Qn = Pn + nb.ld;
    const EffSrc e{s.ws + L.G[bi + 1], nb.ld, s.ws + L.D[bi + 1], nb.ld, 0, Nt, Pn, Qn, 0.f, 0, 0};
    const Tab t = tab(s.ws, L, bg.tn);
    const WkEntry& ef = wk_find(bg.tw, 0);
    if ((rc = drain(s))) return rc;            // the transition uses EY and the slab on `st`
    if (L.XP[bi] >= 0 && mode == MODE_BF16) {
        // materialise the output gradient once (+ bias gradient), then dW = ET^T x XP on the TN GEMM
        const int Nt8 = (int)round_up(Nt, 8);
        SlabJob bias_job{};
        EffMatArgs em{e, Mn, s.ws + L.ey, Nt8, s.frozen ? nullptr : grad[bg.tb], reinterpret_cast<float*>(s.ws + L.slab + kSlabGemmBytes), &bias_job};
        if ((rc = eff_materialize_bf16(em, s.st))) return rc;
        GemmTnArgs gt{s.ws + L.ey, Nt8, Nt8, s.ws + L.XP[bi], bg.ldp, bg.ldp, Mn, gw_of(s, bg.tw), ef.Kp, s.ws + L.zeros,
                      reinterpret_cast<float*>(s.ws + L.slab), kSlabGemmBytes, Nt, bias_job};
        if (!s.frozen && (rc = gemm_tn_bf16(gt, "k_gemm_tn_bf16<transition>", s.st))) return rc;
        const WkEntry& etf = wk_find(bg.tw, 1, 1);
        GemmNtArgs ga{};
        ga.epi = EPI_DGRAD_POOL; ga.A = s.ws + L.ey; ga.lda = Nt8; ga.K = Nt8; ga.M = Mn; ga.N = bg.Ctot;
        ga.Wfrag = s.ws + L.wk + etf.off; ga.Kp = etf.Kp; ga.zeros = s.ws + L.zeros;
        ga.Xin = D; ga.ldxin = bg.ld; ga.sc = t.sc; ga.sh = t.sh; ga.sl = data[bg.ta];
        ga.Gout = G; ga.ldgo = bg.ld; ga.g_write = 1; ga.H = nb.H; ga.W = nb.W; ga.Hin = bg.H; ga.Win = bg.W;
        ga.part = s.part; ga.nblk = gemm_nt_nblk(ga);
        if ((rc = gemm_nt_bf16(ga, "k_gemm_nt_bf16<dgradtrans>", s.st))) return rc;
        return bwd_link(s, bg.tn, ga.nblk, bstatD, M, P, Q, 1, bg.ta);
    }
    ConvWgradArgs w{};
    w.mode = mode; w.e = e; w.dWk = gw_of(s, bg.tw); w.dbias = grad[bg.tb];
    w.fa = trans_args(s, bi);               // fp32 with the pooled activation of the forward materialised: that is the weight gradient's operand
    if (L.XP[bi] >= 0) { w.slab = reinterpret_cast<float*>(s.ws + L.slab); w.slab_bytes = kSlabBytes; }      // split-K slabs of k_gemm_tn_f32 (the stream was drained above)
    if (!s.frozen && (rc = conv_wgrad(w, s.st))) return rc;
    const WkEntry& et = wk_find(bg.tw, 1);
    ConvDgradArgs d{};
    d.mode = mode; d.dmode = DG_1X1_POOL; d.e = e; d.M = (int)Mn; d.N = bg.Ctot; d.Kp = et.Kp;
    d.H = nb.H; d.W = nb.W; d.Hin = bg.H; d.Win = bg.W; d.Wt = s.ws + L.wk + et.off;
    d.Xin = D; d.ldxin = bg.ld; d.sc = t.sc; d.sh = t.sh; d.sl = data[bg.ta];
    d.Gout = G; d.ldgo = bg.ld; d.accumulate = 1; d.part = s.part; d.nblk = conv_dgrad_nblk(d);
    if ((rc = conv_dgrad(d, s.st))) return rc;
    return bwd_link(s, bg.tn, d.nblk, bstatD, M, P, Q, 1, bg.ta);
}

// ---- one dense layer: 3x3 data gradient -> DU, 3x3 weight gradient, 1x1 backward -> G[:, 0:cin] ----
int DenseNetPlan::bwd_layer(Step& s, int bi, int l) const {
    const Layout& L = s.L;
    const BlockGeom& bg = blocks[bi];
    const LayerSlots& ls = bg.layers[l];
    const LayerPath& p = path[bi][l];
    const int mode = cfg.mode, g = cfg.growth, mid = cfg.bn_size * cfg.growth;
    const long M = (long)s.n * bg.H * bg.W;
    hipStream_t st = s.st;
    char* D = s.ws + L.D[bi];
    char* G = s.ws + L.G[bi];
    float* P = reinterpret_cast<float*>(s.ws + L.pqD[bi]);
    float* Q = P + bg.ld;
    const double* bstatD = reinterpret_cast<const double*>(s.ws + L.bstatD[bi]);
    char* Y = s.ws + L.Y[bi][l];
    char* DU = s.ws + L.du;
    float* PY = reinterpret_cast<float*>(s.ws + L.pqY);
    float* QY = PY + mid;
    int rc;
    ConvWgradArgs w3{};                    // conv2 (3x3) weight gradient; its operand arguments serve the data gradient's table too
    w3.fa = conv3_args(s, bi, l);
    // gradient of this layer's output slice D[:, cin:cin+g]
    EffSrc e2{G, bg.ld, D, bg.ld, ls.cin, g, P + ls.cin, Q + ls.cin, s.frozen ? 0.f : cfg.dropout, s.seed, (uint32_t)(bi * 64 + l + 1)};
    if (p.keep_stored) e2.keep = reinterpret_cast<const uint32_t*>(s.ws + L.KM[bi][l]);      // keep words of this layer's forward (else: the hash)
    bool ey_valid = false;
    BnBwdLinkArgs link2{};                 // norm2 backward link (partials of the data gradient below -> PY / QY, which only the 1x1 backward reads)
    {   // conv2 data gradient -> DU (= sc2 * dU2) + norm2 partials (+ the eff rows for the weight gradient below)
        const WkEntry& et = wk_find(ls.w2, 1);
        ConvDgradArgs d{};
        d.mode = mode; d.dmode = DG_3X3; d.e = e2; d.M = (int)M; d.N = mid; d.Kp = et.Kp; d.H = bg.H; d.W = bg.W;
        d.Wt = s.ws + L.wk + et.off; d.Xin = Y; d.ldxin = mid; d.sc = w3.fa.sc; d.sh = w3.fa.sh; d.sl = w3.fa.sl;
        d.Gout = DU; d.ldgo = mid; d.accumulate = 0; d.part = s.part;
        d.Wfrag = wk_frag(s.ws, L, ls.w2, 1); d.zeros = s.ws + L.zeros;
        ey_valid = fast3x3 && !L.EY3[bi].empty() && conv3x3_dgrad_kernel(d) == CONV3X3_DGRAD_CONSEC;      // the kernel that fills ey_out
        if (ey_valid) d.ey_out = s.ws + L.EY3[bi][l];
#ifdef TCVN_DEBUG_KNOBS
        g_snap_path.dgrad_kernel = (int)conv3x3_dgrad_kernel(d); g_snap_path.ey_valid = ey_valid ? 1 : 0;
#endif
        d.nblk = conv_dgrad_nblk(d);
        if ((rc = conv_dgrad(d, st))) return rc;
        link2 = BnBwdLinkArgs{s.part, d.nblk, ls.n2.C, reinterpret_cast<const double*>(s.ws + L.bstatY[bi][l]), M, kEps, data[ls.n2.w],
                              grad[ls.n2.w], grad[ls.n2.b], grad[ls.a2], PY, QY, 0};
    }
    // Fused 1x1 backward (round 4, bwd1x1_fused.hip): effective gradient formed in LDS, bias / data / weight gradient and the norm1
    // backward epilogue in one pass -- no EY in HBM, no read of the activated copy XA, one launch instead of three.  It writes G, so it
    // runs on `st`; its slabs are its own (L.slab belongs to the 3x3 weight gradient, which may be on the side stream).
    // Every width takes the fused kernel.  A/B on MI355X (B = 32 x 8 prongs, validation build): fused for cin <= 256 only 19.76 ms/step, <= 384
    // 19.39, all layers 19.16 -- although a launch with three or four 128-column slices (block 3: every slice re-reads DU / Y and rebuilds EY)
    // takes longer than k_eff_mat + k_gemm_nt did (105 against ~58 us at four slices), the step is shorter without the two extra launches
    // per layer on the main stream and the TN GEMM competing on the side stream.
    Bwd1x1Args fa{};
    const bool fuse1 = bwd1x1_fill(bi, l, M, s.ws, L, fa);       // (the same function the forward asked before it dropped the activated copy)
#ifdef TCVN_DEBUG_KNOBS
    g_snap_path.fused1 = fuse1 ? 1 : 0; g_snap_path.nblk1 = fuse1 ? fa.nblk : 0; g_snap_path.slices1 = cdiv(ls.cin, 128);
#endif
    SlabJob w3jobs[2] = {};        // the 3x3 weight gradient's slab reductions, folded into the fused kernel's reduction launch (same stream only)
    bool w3_deferred = false;
    if (!s.frozen) {   // conv2 (3x3) weight gradient: beside the rest of this layer's data-gradient chain (frozen: neither it nor the norm2 link, PY = QY = 0)
        w3.mode = mode; w3.e = e2; w3.dWk = gw_of(s, ls.w2); w3.dbias = grad[ls.b2];
        if (ey_valid) w3.e.ey = s.ws + L.EY3[bi][l];
        if (fast3x3) {
            w3.nfast = 1; w3.fa.act_fused = p.act_fused ? 1 : 0;
            if (!p.act_fused) w3.fa.Aact = s.ws + L.YA[bi][l];
            w3.slab = reinterpret_cast<float*>(s.ws + L.slab); w3.slab_bytes = kSlabBytes;
        }
        const bool par = s.side_on && L.XA[bi][l] >= 0;
        // The norm2 link rides in the weight-gradient launch when that is the tile kernel on `st` (the kernel reads neither the partials nor
        // PY / QY, and everything that does follows it on `st`): 60 launches fewer on the chain per step.  Otherwise -- side stream, generic
        // kernels, fp32 -- it stays a launch of its own in front of the weight gradient.  TCVN_LINK_LAUNCH (validation build): always.
        static const bool link_launch = TCVN_KNOB_SET("TCVN_LINK_LAUNCH");
        const bool tile3 = fast3x3 && conv3x3_wgrad_tile_ok(w3);
        if (!par && tile3 && !link_launch) w3.link = link2;
        else if ((rc = bn_bwd_link(link2, st))) return rc;
        if (par) {                    // G slice, its (P, Q), the materialised YA and the eff rows are final: fork
            TCVN_CHECK(hipEventRecord(ev_fork_a, st));
            TCVN_CHECK(hipStreamWaitEvent(side_st, ev_fork_a, 0));
            s.side_busy = true;
        }
        if (!par && fuse1 && tile3) { w3.deferred = w3jobs; w3_deferred = true; }
        if ((rc = conv_wgrad(w3, par ? side_st : st))) return rc;
#ifdef TCVN_DEBUG_KNOBS
        if (g_pq_tap.dst != nullptr && g_pq_tap.block == bi && g_pq_tap.layer == l)
            TCVN_CHECK(hipMemcpyAsync(g_pq_tap.dst, PY, (size_t)2 * mid * sizeof(float), hipMemcpyDeviceToDevice, st));
#endif
    }
    if (fuse1) {
        // The slab reductions stay on `st` behind the launch (on the side stream, with double-buffered slabs, the step was 0.25 ms LONGER);
        // one launch reduces this kernel's slabs and the 3x3 weight gradient's.
        if ((rc = bwd1x1_fused_launch(fa, st))) return rc;
        // frozen: the kernel's weight-gradient tiles and bias column sums stay in its slabs (workspace scratch): no reduction into a gradient, no link
        if (s.frozen) return 0;
        // Round 5: the norm1 link rides in the reduction launch (the workgroups behind the last job of k_slab_reduce_link's 1-D grid): both are ~5 us latency-floor
        // launches on the critical chain and independent of each other -- 60 launches fewer per step
        const BnSlots& s1 = ls.n1;
        BnBwdLinkArgs la{s.part, fa.nblk, s1.C, bstatD, M, kEps, data[s1.w], grad[s1.w], grad[s1.b], grad[ls.a1], P, Q, 1};
        return bwd1x1_fused_reduce(fa, gw_of(s, ls.w1), grad[ls.b1], w3_deferred ? w3jobs : nullptr, st, &la);
    }
    if (p.raw1x1) {
        fprintf(stderr, "tcvn: the forward skipped the activated 1x1 input of block %d layer %d but the fused 1x1 backward cannot run\n", bi, l);
        return -15;
    }
    const Tab t1 = tab(s.ws, L, ls.n1);
    const EffSrc e1{DU, mid, Y, mid, 0, mid, PY, QY, 0.f, 0, 0};
    if (L.XA[bi][l] < 0) {      // generic kernels: conv1 (1x1) weight gradient; data gradient -> G[:, 0:cin] += sc1 * dU1, norm1 partials
        ConvWgradArgs w{};
        w.mode = mode; w.e = e1; w.dWk = gw_of(s, ls.w1); w.dbias = grad[ls.b1];
        w.fa = conv1_args(s, bi, l);
        if (mode == MODE_F32) { w.slab = reinterpret_cast<float*>(s.ws + L.slab); w.slab_bytes = kSlabBytes; }     // k_gemm_tn_f32 (cin % 4 != 0); same stream as every other user
        if (!s.frozen && (rc = conv_wgrad(w, st))) return rc;
        const WkEntry& et = wk_find(ls.w1, 1);
        ConvDgradArgs d{};
        d.mode = mode; d.dmode = DG_1X1; d.e = e1; d.M = (int)M; d.N = ls.cin; d.Kp = et.Kp; d.H = bg.H; d.W = bg.W;
        d.Wt = s.ws + L.wk + et.off; d.Xin = D; d.ldxin = bg.ld; d.sc = t1.sc; d.sh = t1.sh; d.sl = data[ls.a1];
        d.Gout = G; d.ldgo = bg.ld; d.accumulate = 1; d.part = s.part; d.nblk = conv_dgrad_nblk(d);
        if ((rc = conv_dgrad(d, st))) return rc;
        return bwd_link(s, ls.n1, d.nblk, bstatD, M, P, Q, 1, ls.a1);
    }
    // bf16 GEMMs: EY = the materialised gradient (+ bias gradient), conv1 weight gradient dW = EY^T x XA on the TN GEMM, data gradient on the NT GEMM (A = EY)
    const bool odd = s.side_on && (s.seq & 1);
    char* EY = s.ws + (odd ? L.ey2 : L.ey);
    float* tail = reinterpret_cast<float*>(s.ws + L.slab + kSlabGemmBytes + (odd ? (kSlabBytes - kSlabGemmBytes) / 2 : 0));
    if (s.side_on && s.seq >= 2) TCVN_CHECK(hipStreamWaitEvent(st, ev_done[s.seq & 1], 0));   // that EY buffer / tail half is free again
    SlabJob bias_job{};     // bias column sums: reduced together with the weight-gradient slab below
    EffMatArgs em{e1, M, EY, mid, s.frozen ? nullptr : grad[ls.b1], tail, &bias_job};
    if ((rc = eff_materialize_bf16(em, st))) return rc;
    if (s.side_on) {
        TCVN_CHECK(hipEventRecord(ev_fork_b, st));
        TCVN_CHECK(hipStreamWaitEvent(side_st, ev_fork_b, 0));
        s.side_busy = true;
    }
    const int cin8 = (int)round_up(ls.cin, 8);
    GemmTnArgs gt{EY, mid, mid, s.ws + L.XA[bi][l], cin8, cin8, M, gw_of(s, ls.w1), wk_find(ls.w1, 0).Kp, s.ws + L.zeros,
                  reinterpret_cast<float*>(s.ws + L.slab), kSlabGemmBytes, mid, bias_job};
    if (!s.frozen && (rc = gemm_tn_bf16(gt, "k_gemm_tn_bf16<conv1>", s.side_on ? side_st : st))) return rc;
    if (s.side_on) TCVN_CHECK(hipEventRecord(ev_done[s.seq & 1], side_st));
    const WkEntry& etf = wk_find(ls.w1, 1, 1);
    GemmNtArgs ga{};
    ga.epi = EPI_DGRAD; ga.A = EY; ga.lda = mid; ga.K = mid; ga.M = M; ga.N = ls.cin;
    ga.Wfrag = s.ws + L.wk + etf.off; ga.Kp = etf.Kp; ga.zeros = s.ws + L.zeros;
    ga.Xin = D; ga.ldxin = bg.ld; ga.sc = t1.sc; ga.sh = t1.sh; ga.sl = data[ls.a1];
    ga.Gout = G; ga.ldgo = bg.ld; ga.part = s.part; ga.nblk = gemm_nt_nblk(ga);
    if ((rc = gemm_nt_bf16(ga, "k_gemm_nt_bf16<dgrad1x1>", st))) return rc;
    if ((rc = bwd_link(s, ls.n1, ga.nblk, bstatD, M, P, Q, 1, ls.a1))) return rc;
    ++s.seq;
    return 0;
}

// ---- stem: AvgPool0 - PReLU0 - BN0 - conv0 ----
int DenseNetPlan::bwd_stem(const Step& s) const {
    const Layout& L = s.L;
    const BlockGeom& b0 = blocks[0];
    const int mode = cfg.mode, n = s.n;
    float* P = reinterpret_cast<float*>(s.ws + L.pqD[0]);
    float* Q = P + b0.ld;
    float* P0 = reinterpret_cast<float*>(s.ws + L.pq0);
    float* Q0 = P0 + cfg.init_ch;
    const double* bstat0 = reinterpret_cast<const double*>(s.ws + L.bstat0);
    const long M0 = (long)n * Hc * Wc;
    const EffSrc e{s.ws + L.G[0], b0.ld, s.ws + L.D[0], b0.ld, 0, cfg.init_ch, P, Q, 0.f, 0, 0};
    int rc;
    if (stem_path.sparse) {
        // stem_sparse.hip: BwdSums = pooling / PReLU0 / BN0 backward sums with the conv0 output rebuilt from the hit list per region;
        // BwdWgrad = conv0 weight gradient from the same regions with (P0, Q0) applied.  No conv0-sized tensor is read or written.
        StemSparseArgs sa = stem_sparse_args(s, last_coords, last_values, last_nnz, last_value_mode, last_noise);
        sa.e = e; sa.part = s.part;
        if ((rc = stem_sparse_bwd(sa, StemPass::BwdSums, s.st))) return rc;
        if ((rc = bwd_link(s, n0, stem_sparse_plan(sa, StemPass::BwdSums).grid, bstat0, M0, P0, Q0, 0, s_a0))) return rc;
        sa.P0 = P0; sa.Q0 = Q0; sa.slab = reinterpret_cast<float*>(s.ws + L.slab); sa.slab_bytes = kSlabBytes; sa.dWk = gw_of(s, s_w0);
        return stem_sparse_bwd(sa, StemPass::BwdWgrad, s.st);
    }
    const Tab t = tab(s.ws, L, n0);
    Pool0BwdArgs a{mode, s.ws + L.c0, n, Hc, Wc, cfg.init_ch, t.sc, t.sh, data[s_a0], e, b0.H, b0.W, s.ws + L.du0, s.part,
                   pool0_bwd_grid(n, Hc, Wc), nullptr, nullptr};
    if (stem_path.act_skip) {                // the forward skipped the conv0-output rows no hit reaches: read the shared row for them, skip their gradient rows
        a.act = reinterpret_cast<const uint32_t*>(s.ws + L.sact); a.cline = s.ws + L.zeros + 512;
    }
    const bool vec = pool0_bwd_vec_ok(a) && conv3x3_tile_enabled();
    if (stem_path.act_skip && !(vec && cfg.init_ch == 64 && mode == MODE_BF16)) { fprintf(stderr, "tcvn: stem activity bitmap without the tile kernel\n"); return -16; }
    if (vec) { a.nblk = pool0_bwd_vec_grid(n, Hc, Wc); rc = pool0_bwd_vec(a, s.st); }
    else rc = pool0_bwd(a, s.st);
    if (rc) return rc;
    if ((rc = bwd_link(s, n0, a.nblk, bstat0, M0, P0, Q0, 0, s_a0))) return rc;
    if (s.frozen) return 0;      // DU0 is the effective conv0-output gradient itself (P0 = Q0 = 0): input_gradient gathers it at the hits
    const EffSrc e0{s.ws + L.du0, cfg.init_ch, s.ws + L.c0, cfg.init_ch, 0, cfg.init_ch, P0, Q0, 0.f, 0, 0};
    if (conv3x3_tile_enabled() && cfg.in_ch <= 3 && cfg.init_ch <= 64 && last_coords != nullptr) {
        // conv0 weight gradient from the hit list (bias gradient is exactly zero in exact arithmetic: BN0 follows)
        StemWgradArgs sa{last_coords, last_nnz, s.ws + L.img, n, cfg.H, cfg.W, cfg.in_ch, e0, Hc, Wc, wk_find(s_w0, 0).Kp,
                         reinterpret_cast<float*>(s.ws + L.slab), kSlabBytes, mode,
                         PixelOwners{reinterpret_cast<uint32_t*>(s.ws + L.own), (long)n * cfg.H * cfg.W}};
        return stem_wgrad_sparse(sa, gw_of(s, s_w0), s.st);
    }
    ConvWgradArgs w{};
    w.mode = mode; w.e = e0; w.dWk = gw_of(s, s_w0); w.dbias = grad[s_b0];
    w.fa = conv0_args(s);
    return conv_wgrad(w, s.st);
}
