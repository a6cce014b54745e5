// layer.hip -- host-side sequencing of one whole BertLayer (forward: 7 launches, backward: 15) behind a
// single C-ABI call each, so the Python side pays two FFI calls per layer instead of ~22 op dispatches.
// Pure orchestration: every launch goes through the same entry points the per-op ABI exposes.
//
// Replaces BertLayer.forward and its autograd backward
//   (pytorch_pretrained_bert/modeling.py:331-341 = BertAttention :276-293 [BertSelfAttention :231-261,
//    BertSelfOutput :270-274] -> BertIntermediate :302-305 -> BertOutput :315-319).
#include "vb_rt.h"
#include "../../include/visualbert_hip.h"

namespace {

// dtype: the caller's (VB_F32 / VB_BF16 / VB_BF16X3); edt: what the non-GEMM kernels see (bf16x3 keeps every activation
// in fp32 and splits a GEMM's operands into bf16 hi | lo planes right in front of it); es: bytes per activation element
struct Dims { int B, S, H, I, nh; long M; size_t es; int dtype, edt; bool x3; };

inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

// one carve of a workspace: consecutive 256-byte-aligned slots (base == NULL: only the total is wanted)
struct Carver {
    unsigned char* base; size_t o;
    unsigned char* take(size_t bytes) { unsigned char* p = base ? base + o : nullptr; o += al(bytes); return p; }
};

// saved-for-backward workspace of one layer
struct Saved {
    unsigned char *qkv, *ctx, *z1, *a_out, *pre, *inter, *z2;
    float *lse, *mean1, *rstd1, *mean2, *rstd2;
    uint64_t* keepbits;
    int* ln_flags;      // [2] device ints written by the two LayerNorm forwards: 1 = no z was written, the backward rebuilds x-hat from y
    int *rb1, *rb2;     // = ln_flags, ln_flags + 1, or NULL (wider rows: the backward's rebuild-capable form does not pay, layernorm.hip)
    // bf16x3 only: the split (hi | lo) images of the four GEMM inputs the forward made anyway -- they are the x operands of the
    // backward's weight-gradient launch, so keeping them saves four split passes per layer (19 % of the mode's split traffic)
    unsigned char *sp_hin, *sp_ctx, *sp_aout, *sp_inter;
    size_t total;
};

Saved carve_saved(unsigned char* base, const Dims& d, bool attn_dropout) {
    Saved s;
    Carver c{base, 0};
    s.qkv = c.take((size_t)d.M * 3 * d.H * d.es);
    s.ctx = c.take(d.x3 ? 0 : (size_t)d.M * d.H * d.es);    // split-operand mode: the context and the FFN activation exist only as
                                                              // their images (sp_ctx, sp_inter below): only GEMMs read them
    s.z1 = c.take((size_t)d.M * d.H * d.es);
    s.a_out = c.take((size_t)d.M * d.H * d.es);
    s.pre = c.take((size_t)d.M * d.I * d.es);
    s.inter = c.take(d.x3 ? 0 : (size_t)d.M * d.I * d.es);
    s.z2 = c.take((size_t)d.M * d.H * d.es);
    s.lse = (float*)c.take((size_t)d.B * d.nh * d.S * 4);
    s.mean1 = (float*)c.take((size_t)d.M * 4);
    s.rstd1 = (float*)c.take((size_t)d.M * 4);
    s.mean2 = (float*)c.take((size_t)d.M * 4);
    s.rstd2 = (float*)c.take((size_t)d.M * 4);
    s.keepbits = (uint64_t*)c.take(attn_dropout ? (size_t)d.B * d.nh * vb_attn_keepbits_words(d.S) * 8 : 0);
    s.ln_flags = (int*)c.take(8);
    const bool rb = d.H <= 768 && s.ln_flags;
    s.rb1 = rb ? s.ln_flags : nullptr;
    s.rb2 = rb ? s.ln_flags + 1 : nullptr;
    const size_t sh = d.x3 ? (size_t)d.M * 2 * d.H * 2 : 0, si = d.x3 ? (size_t)d.M * 2 * d.I * 2 : 0;
    s.sp_hin = c.take(sh); s.sp_ctx = c.take(sh); s.sp_aout = c.take(sh); s.sp_inter = c.take(si);
    s.total = c.o;
    return s;
}

// scratch (temporaries, reusable by every layer on the same stream)
struct Scratch {
    unsigned char *t_h0, *t_h1, *t_h2, *t_h3, *t_h4, *t_h5, *t_i, *t_3h;
    float* dsum;
    float *ln_ws, *ln_ws1;      // column partials of the output / the attention-output LayerNorm's backward (both alive to the layer's
                                // one second-stage reduction launch)
    // bf16x3 only: split (hi | lo) images of the backward's output gradients, [M, 2 x features] bf16 each, alive until the
    // grouped weight-gradient launch (the x operands' images come from the forward: Saved)
    unsigned char *sp_dfo, *sp_dpre, *sp_dao, *sp_dqkv;
    size_t total;
};
Scratch carve_scratch(unsigned char* base, const Dims& d) {
    Scratch s;
    Carver c{base, 0};
    s.t_h0 = c.take((size_t)d.M * d.H * d.es);
    s.t_h1 = c.take((size_t)d.M * d.H * d.es);
    s.t_h2 = c.take((size_t)d.M * d.H * d.es);
    s.t_h3 = c.take((size_t)d.M * d.H * d.es);
    s.t_h4 = c.take((size_t)d.M * d.H * d.es);
    s.t_h5 = c.take((size_t)d.M * d.H * d.es);
    s.t_i = c.take((size_t)d.M * d.I * d.es);
    s.t_3h = c.take((size_t)d.M * 3 * d.H * d.es);
    s.dsum = (float*)c.take((size_t)vb_attn_bwd_ws_floats((int)d.B, (int)d.S, (int)d.nh) * 4);
    s.ln_ws = (float*)c.take((size_t)vb_ln_bwd_ws_bytes((int)d.M, d.H));
    s.ln_ws1 = (float*)c.take((size_t)vb_ln_bwd_ws_bytes((int)d.M, d.H));
    const size_t sh = d.x3 ? (size_t)d.M * 2 * d.H * 2 : 0, si = d.x3 ? (size_t)d.M * 2 * d.I * 2 : 0;
    s.sp_dfo = c.take(sh); s.sp_dpre = c.take(si); s.sp_dao = c.take(sh); s.sp_dqkv = c.take(3 * sh);
    s.total = c.o;
    return s;
}

bool fill_dims(Dims& d, int dtype, int B, int S, int H, int I, int nh) {
    if (B <= 0 || S <= 0 || H <= 0 || I <= 0 || nh <= 0 || nh * 64 != H || (H % 8) || (I % 8)) return false;
    if (dtype != VB_F32 && dtype != VB_BF16 && dtype != VB_BF16X3) return false;
    if (dtype == VB_BF16X3 && ((H % 64) || (I % 64))) return false;       // split-operand GEMMs reduce over whole K tiles
    d.B = B; d.S = S; d.H = H; d.I = I; d.nh = nh; d.M = (long)B * S; d.es = dtype == VB_BF16 ? 2 : 4;
    d.dtype = dtype; d.x3 = dtype == VB_BF16X3; d.edt = d.x3 ? VB_F32 : dtype;
    return true;
}

// weights[] by name (VB_LW_* order: T for matrices read by the GEMMs, fp32 for biases / LayerNorm)
struct LayerWeights {
    const void* wqkv; const float* bqkv; const void* wo; const float* bo; const float *g1, *b1;
    const void* wi; const float* bi; const void* wo2; const float* bo2; const float *g2, *b2;
};
LayerWeights unpack_weights(const void* const* w) {
    auto f = [&](int i) { return (const float*)w[i]; };
    return {w[VB_LW_QKV_W], f(VB_LW_QKV_B), w[VB_LW_AO_W], f(VB_LW_AO_B), f(VB_LW_LN1_G), f(VB_LW_LN1_B),
            w[VB_LW_FI_W], f(VB_LW_FI_B), w[VB_LW_FO_W], f(VB_LW_FO_B), f(VB_LW_LN2_G), f(VB_LW_LN2_B)};
}

// y[m, n] = epilogue(x[m, k] W[n, k]^T): in the split-operand mode x (fp32) is split into `stage` first and W arrives split
// split_y (split-operand mode only): y is written as a split image [m, 2 n] itself (the result feeds only GEMMs)
int linear(const Dims& d, int m, const void* x, int k, unsigned char* stage, const void* w, int64_t ldw, void* y, int n,
           const float* bias, const void* addend, int act, const void* aux_in, void* aux_out, float* colsum, void* stream,
           bool split_y = false) {
    if (!d.x3)
        return vb_gemm(d.dtype, d.dtype, VB_KCONTIG, VB_KCONTIG, x, k, w, ldw, y, n, m, n, k, 1.f, nullptr, bias, addend, n, act,
                       aux_in, aux_out, n, 0, colsum, stream);
    if (stage) {                                               // nullptr: `x` already is the split image
        const int rc = vb_split_bf16((const float*)x, k, stage, 2 * k, m, k, stream);
        if (rc != VB_OK) return rc;
        x = stage;
    }
    return vb_gemm(VB_BF16X3, split_y ? VB_BF16X3 : VB_F32, VB_KCONTIG, VB_KCONTIG, x, 2 * k, w, ldw, y, split_y ? 2 * n : n, m, n, k,
                   1.f, nullptr, bias, addend, n, act, aux_in, aux_out, n, 0, colsum, stream);
}

#ifndef VB_DEFER_REDUCE
#define VB_DEFER_REDUCE 1       // 0: every second-stage reduction right behind its producer (the A/B arm of profiles/r06_small_batch_ab.txt)
#endif
#define VB_TRY(expr) do { int rc_ = (expr); if (rc_ != VB_OK) return rc_; } while (0)

// the second stages of the two LayerNorm backwards' column reductions and of the attention backward's bias gradient run as ONE
// launch at the end of the layer (vb_rt.h: VbReduceJobs): while a DeferScope lives they are collected in its list
struct DeferScope {
    explicit DeferScope(VbReduceJobs* j) { vb_reduce_defer_slot() = VB_DEFER_REDUCE ? j : nullptr; }
    ~DeferScope() { vb_reduce_defer_slot() = nullptr; }
};

// what a backward entry was called with, beyond the tensors that are its own
struct Bwd {
    Dims d;
    LayerWeights w;
    const void* const* weights_t; const int64_t* ld_t;
    const float* mask_add;
    float p_hidden, p_attn; uint64_t seed; uint32_t sid; void* stream;
    float* G[VB_LW_COUNT];              // grads[]: fp32 accumulation targets in VB_LW_* order (all required)

    bool take_grads(void* const* grads) {
        for (int i = 0; i < VB_LW_COUNT; ++i) { G[i] = (float*)grads[i]; if (!G[i]) return false; }
        return true;
    }
    // dgrad dx[m,in] = dy[m,out] W[out,in]: with W^T [in, ld>=out] both operands are K-contiguous (LDS-direct
    // loads); otherwise W is read K-strided and transposed on the fly
    // split-operand mode: dy arrives as its split image -- kept for the grouped weight-gradient launch -- and W^T arrives split
    int dgrad(int m, const void* dy, int n_out, const void* wm, int which_t, int n_in, void* dx, const void* addend,
              int act, const void* aux, float* colsum = nullptr, bool split_dx = false) const {
        const void* wt = weights_t ? weights_t[which_t] : nullptr;
        if (d.x3)
            return linear(d, m, dy, n_out, nullptr, wt, ld_t[which_t], dx, n_in, nullptr, addend, act, aux, nullptr, colsum, stream,
                          split_dx);
        if (wt)
            return vb_gemm(d.dtype, d.dtype, VB_KCONTIG, VB_KCONTIG, dy, n_out, wt, ld_t[which_t], dx, n_in, m, n_in, n_out,
                           1.f, nullptr, nullptr, addend, n_in, act, aux, nullptr, n_in, 0, colsum, stream);
        return vb_gemm(d.dtype, d.dtype, VB_KCONTIG, VB_KSTRIDED, dy, n_out, wm, n_in, dx, n_in, m, n_in, n_out, 1.f, nullptr,
                       nullptr, addend, n_in, act, aux, nullptr, n_in, 0, colsum, stream);
    }
};

// the groups of one vb_wgrad_grouped launch: dW[n_out, n_in] += dy[rows, n_out]^T x[rows, n_in] each.  The order of the add() calls
// is the order of the groups inside the launch, and with it the summation order of the atomics
struct WgradGroups {
    const void* dys[4]; int64_t ld_dy[4]; const void* xs[4]; int64_t ld_x[4]; void* dws[4]; int64_t ld_dw[4]; int n_out[4], n_in[4];
    int n = 0;
    void add(const void* dy, int64_t ldy, const void* x, int64_t ldx, void* dw, int64_t ldw, int out, int in) {
        dys[n] = dy; ld_dy[n] = ldy; xs[n] = x; ld_x[n] = ldx; dws[n] = dw; ld_dw[n] = ldw; n_out[n] = out; n_in[n] = in;
        ++n;
    }
    int launch(int dtype, int rows, void* stream) const {
        return vb_wgrad_grouped(dtype, n, dys, ld_dy, xs, ld_x, dws, ld_dw, n_out, n_in, rows, 1.f, nullptr, stream);
    }
};

// Where the row-wise front of the backward (steps 1-5: every one of them acts on one row at a time) runs: on all M rows in place,
// or on the compact rows of a row map.
struct Front {
    int m_gemm, m_ln;                   // rows the GEMMs see (whole row tiles) / rows the LayerNorms write: [m_ln, m_gemm) is zero padding
    const int64_t* rows;                // row map into d_out and the saved tensors (vb_rt.h: vb_ln_bwd_map), or NULL: row m is row m
    int dy_mapped;                      // d_out is indexed through the map (it always is [M, H]; the front's own buffers are [m_gemm, .])
    const void* d_out;
    unsigned char *dz2, *dfo, *dpre, *da, *dz1, *dao, *dctx;   // dfo / dao are used with dropout only: without it they ARE dz2 / dz1, and
                                                               // bwd_front() leaves that in these two fields for the weight gradients
    const void* gelu_grad;              // GELU'(pre) of the front's rows, [m_gemm, I]
    float *ln_ws, *ln_ws1;
    unsigned char *sp_dfo, *sp_dao;     // split-operand mode: dfo / dao leave their LayerNorm backward ONLY as hi | lo images; else NULL
    const void* dfo_op() const { return sp_dfo ? sp_dfo : dfo; }     // what the GEMMs read
    const void* dao_op() const { return sp_dao ? sp_dao : dao; }
};

int bwd_front(const Bwd& c, const Saved& sv, const void* h_out, Front& f) {
    const Dims& d = c.d;
    const int H = d.H, I = d.I;
    float* const* G = c.G;
    // the LayerNorm backwards write rows [0, m_ln) of their outputs: the padding rows of what a GEMM reads are cleared
    auto clear_pad = [&](unsigned char* p) -> int {
        if (f.m_gemm == f.m_ln) return VB_OK;
        return hipMemsetAsync(p + (size_t)f.m_ln * H * d.es, 0, (size_t)(f.m_gemm - f.m_ln) * H * d.es, (hipStream_t)c.stream) == hipSuccess
                   ? VB_OK : VB_ERR_LAUNCH;
    };
    if (!(c.p_hidden > 0.f)) { f.dfo = f.dz2; f.dao = f.dz1; }
    // 1. output LayerNorm backward (+ bias gradient of the FFN-out dense as a by-product): dz2 = d(a_out) through the residual of the
    //    output LN, dfo = d(FFN-out dense output)
    //    (split-operand mode: + the hi | lo image of dfo, the next dgrad's and the weight-gradient launch's operand)
    VB_TRY(vb_ln_bwd_map(d.edt, f.d_out, sv.z2, sv.mean2, sv.rstd2, c.w.g2, f.dz2, f.sp_dfo ? nullptr : f.dfo, G[VB_LW_LN2_G], G[VB_LW_LN2_B],
                         G[VB_LW_FO_B], f.m_ln, H, c.p_hidden, c.sid + 4, 0.f, 0, c.seed, f.ln_ws, f.sp_dfo, 2 * H, h_out, c.w.b2, sv.rb2,
                         f.rows, f.dy_mapped, c.stream));
    VB_TRY(clear_pad(f.dz2));
    if (f.dfo != f.dz2) VB_TRY(clear_pad(f.dfo));
    // 2. dgrad FFN-out with the saved GELU' folded into the epilogue: dpre = (dfo Wo2) * gelu'(pre)
    //    (+ bias gradient of FFN-in = column sums of dpre, accumulated by the same epilogue)
    //    (split-operand mode: dpre leaves the GEMM as a split image -- only the next dgrad and the wgrad launch read it)
    VB_TRY(c.dgrad(f.m_gemm, f.dfo_op(), H, c.w.wo2, VB_LWT_FO, I, f.dpre, nullptr, VB_ACT_MUL_AUX, f.gelu_grad, G[VB_LW_FI_B], d.x3));
    // 3. dgrad FFN-in + residual gradient: da = dpre Wi + dz2
    VB_TRY(c.dgrad(f.m_gemm, f.dpre, I, c.w.wi, VB_LWT_FI, H, f.da, f.dz2, VB_ACT_NONE, nullptr));
    // 4. attention-output LayerNorm backward (dy is the front's own da: never through the map)
    VB_TRY(vb_ln_bwd_map(d.edt, f.da, sv.z1, sv.mean1, sv.rstd1, c.w.g1, f.dz1, f.sp_dao ? nullptr : f.dao, G[VB_LW_LN1_G], G[VB_LW_LN1_B],
                         G[VB_LW_AO_B], f.m_ln, H, c.p_hidden, c.sid + 1, 0.f, 0, c.seed, f.ln_ws1, f.sp_dao, 2 * H, sv.a_out, c.w.b1, sv.rb1,
                         f.rows, 0, c.stream));
    VB_TRY(clear_pad(f.dao));
    // 5. dgrad attention-out: dctx = dao Wo
    return c.dgrad(f.m_gemm, f.dao_op(), H, c.w.wo, VB_LWT_AO, H, f.dctx, nullptr, VB_ACT_NONE, nullptr);
}

// The dense tail of the backward, over all M rows: the attention backward mixes rows.
// attention backward (one pass for bf16 and S <= 192, else dQ pass + dK/dV pass) + the q | k | v bias gradient (per-sample sums out of
// the one-pass kernel's accumulators; a column-sum pass over dqkv otherwise), then dgrad QKV + residual gradient: dh = dqkv Wqkv + dz1
// sp_dqkv (split-operand mode, else NULL): dqkv leaves the attention backward only as its hi | lo image
int bwd_tail(const Bwd& c, const Saved& sv, const void* dctx, const void* dz1, float* dsum, unsigned char* dqkv, unsigned char* sp_dqkv,
             void* d_in) {
    const Dims& d = c.d;
    VB_TRY(vb_attn_bwd_sp(d.dtype, sv.qkv, c.mask_add, dctx, sv.lse, sv.keepbits, dsum, dqkv, d.x3 ? nullptr : sv.ctx, c.G[VB_LW_QKV_B],
                          d.B, d.S, d.nh, 64, c.p_attn, c.seed, c.sid, sp_dqkv, 1, c.stream));
    return c.dgrad((int)d.M, sp_dqkv ? (const void*)sp_dqkv : (const void*)dqkv, 3 * d.H, c.w.wqkv, VB_LWT_QKV, d.H, d_in, dz1, VB_ACT_NONE,
                   nullptr);
}

}  // namespace

extern "C" int64_t vb_bert_layer_saved_bytes(int dtype, int B, int S, int H, int I, int nh, float p_attn) {
    Dims d;
    if (!fill_dims(d, dtype, B, S, H, I, nh)) return -1;
    return (int64_t)carve_saved(nullptr, d, p_attn > 0.f).total;
}
extern "C" int64_t vb_bert_layer_scratch_bytes(int dtype, int B, int S, int H, int I, int nh) {
    Dims d;
    if (!fill_dims(d, dtype, B, S, H, I, nh)) return -1;
    return (int64_t)carve_scratch(nullptr, d).total;
}

// weights[]: VB_LW_* order (T for matrices read by the GEMMs, fp32 for biases / LayerNorm)
extern "C" int vb_bert_layer_fwd(int dtype, const void* h_in, const float* mask_add, void* h_out,
                                 void* saved, void* scratch, const void* const* weights,
                                 int B, int S, int H, int I, int nh, float p_hidden, float p_attn, float eps,
                                 uint64_t seed, uint32_t sid, void* stream) {
    Dims d;
    if (!fill_dims(d, dtype, B, S, H, I, nh) || !h_in || !mask_add || !h_out || !saved || !scratch || !weights)
        return VB_ERR_ARG;
    Saved sv = carve_saved((unsigned char*)saved, d, p_attn > 0.f);
    Scratch sc = carve_scratch((unsigned char*)scratch, d);
    const int M = (int)d.M;
    const LayerWeights w = unpack_weights(weights);

    const int edt = d.edt;
    const int64_t wk = d.x3 ? 2 : 1;                   // leading dimension of a weight matrix per K element (split: hi | lo)
    // 1. packed Q|K|V projection
    VB_TRY(linear(d, M, h_in, H, sv.sp_hin, w.wqkv, wk * H, sv.qkv, 3 * H, w.bqkv, nullptr, VB_ACT_NONE, nullptr, nullptr, nullptr, stream));
    // 2. fused attention
    //    (split-operand mode: the kernels that PRODUCE a GEMM input write its hi | lo image themselves -- the context here, the
    //     LayerNorm output below, the three output gradients in the backward -- so the only stand-alone split pass left per layer
    //     is the one over h_in, which the previous layer / the embeddings produced)
    //    and where ONLY GEMMs read a result -- the context, and in the backward dfo / dao / dqkv -- its fp32 form is not written
    //    at all (sv.ctx, sc.t_h1 / t_h4 / t_3h stay untouched in this mode)
    VB_TRY(vb_attn_fwd_sp(d.dtype, sv.qkv, mask_add, sv.ctx, sv.lse, sv.keepbits, B, S, nh, 64, p_attn, seed, sid,
                          d.x3 ? sv.sp_ctx : nullptr, 1, stream));
    // 3 + 4. attention output projection, dropout + residual + LayerNorm
    //    (the pre-LN sum z is NOT written by the LayerNorm when the backward can rebuild x-hat from the output it reads anyway --
    //     decided in the kernel from gamma / beta and recorded in sv.ln_flags)
    //    Round 6 built the other split of this block -- the GEMM's epilogue applies dropout + residual and writes z straight into the saved
    //    slot, the LayerNorm launch reads ONE tensor -- measured it, and declined it: with dropout the mask
    //    generator in the persistent kernel's epilogue costs more than the LayerNorm saves (step 118.0 -> 118.45 ms), and even the
    //    residual-only form normalises a bf16-rounded residual stream (max |dlogit| against the reference 3.2e-3 -> 5.8e-3).  The arm
    //    stays reachable in the developer library (debug bit 29: gemm.hip vb_gemm_dropres; profiles/r06_dropres_epilogue_ab.txt).
    auto out_block = [&](const void* x, int k, const void* wm, const float* bias, const void* resid, unsigned char* tmp, unsigned char* zslot,
                         void* y, float* mean, float* rstd, const float* gam, const float* bet, uint32_t site, int* rbf,
                         void* y_split) -> int {
        if (d.dtype == VB_BF16 && vb_gemm_fuse_residual_armed()) {
            const int rc = vb_gemm_dropres(VB_BF16, VB_BF16, VB_KCONTIG, VB_KCONTIG, x, k, wm, k, zslot, H, M, H, k, 1.f, nullptr, bias, resid, H,
                                           VB_ACT_NONE, nullptr, nullptr, H, 0, nullptr, p_hidden, seed, site, stream);
            if (rc == VB_OK)                            // z is in its slot already: x = z_out = the slot (the kernel reads a row before it writes it)
                return vb_ln_fwd_sp(edt, zslot, nullptr, zslot, y, mean, rstd, gam, bet, M, H, eps, 0.f, site, 0.f, 0, seed, nullptr, 0, rbf, stream);
            if (rc != VB_ERR_UNSUPPORTED) return rc;    // (small problems: declined, nothing launched)
        }
        VB_TRY(linear(d, M, x, k, nullptr, wm, wk * k, tmp, H, bias, nullptr, VB_ACT_NONE, nullptr, nullptr, nullptr, stream));
        return vb_ln_fwd_sp(edt, tmp, resid, zslot, y, mean, rstd, gam, bet, M, H, eps, p_hidden, site, 0.f, 0, seed, y_split, 2 * H, rbf, stream);
    };
    VB_TRY(out_block(d.x3 ? (const void*)sv.sp_ctx : (const void*)sv.ctx, H, w.wo, w.bo, h_in, sc.t_h0, sv.z1, sv.a_out, sv.mean1, sv.rstd1,
                     w.g1, w.b1, sid + 1, sv.rb1, d.x3 ? sv.sp_aout : nullptr));
    // 5. FFN in + erf-GELU (GELU' kept for backward)
    //    (split-operand mode: the activation leaves the GEMM as a split image -- only GEMMs read it: FFN-out and its wgrad)
    VB_TRY(linear(d, M, d.x3 ? (const void*)sv.sp_aout : (const void*)sv.a_out, H, nullptr, w.wi, wk * H,
                  d.x3 ? (void*)sv.sp_inter : (void*)sv.inter, I, w.bi, nullptr, VB_ACT_GELU_SAVE_GRAD, nullptr, sv.pre, nullptr, stream, d.x3));
    // 6 + 7. FFN out, dropout + residual + LayerNorm (the same block: modeling.py:316-318)
    VB_TRY(out_block(d.x3 ? (const void*)sv.sp_inter : (const void*)sv.inter, I, w.wo2, w.bo2, sv.a_out, sc.t_h1, sv.z2, h_out, sv.mean2, sv.rstd2,
                     w.g2, w.b2, sid + 4, sv.rb2, nullptr));
    return VB_OK;
}

// grads[]: fp32 accumulation targets in VB_LW_* order (all required)
extern "C" int vb_bert_layer_bwd(int dtype, const void* h_in, const void* h_out, const float* mask_add, const void* d_out, void* d_in,
                                 const void* saved, void* scratch, const void* const* weights, void* const* grads,
                                 const void* const* weights_t, const int64_t* ld_t,
                                 int B, int S, int H, int I, int nh, float p_hidden, float p_attn,
                                 uint64_t seed, uint32_t sid, void* stream) {
    Dims d;
    if (!fill_dims(d, dtype, B, S, H, I, nh) || !h_in || !mask_add || !d_out || !d_in || !saved || !scratch ||
        !weights || !grads)
        return VB_ERR_ARG;
    if (H <= 768 && !h_out) return VB_ERR_ARG;               // the output LayerNorm's backward may rebuild x-hat from it
    Saved sv = carve_saved((unsigned char*)saved, d, p_attn > 0.f);
    Scratch sc = carve_scratch((unsigned char*)scratch, d);
    const int M = (int)d.M;
    Bwd c{d, unpack_weights(weights), weights_t, ld_t, mask_add, p_hidden, p_attn, seed, sid, stream, {}};
    if (!c.take_grads(grads)) return VB_ERR_ARG;
    if (d.x3 && (!weights_t || !weights_t[0] || !weights_t[1] || !weights_t[2] || !weights_t[3] || !ld_t)) return VB_ERR_UNSUPPORTED;
    float* const* G = c.G;

    // Every output gradient (dfo, dpre, dao, dqkv) stays alive to the end of the layer so that the four weight
    // gradients run as ONE grouped launch (vb_wgrad_grouped): 108 output tiles x 2 token slices fill the chip with
    // 164-K-tile items, where four separate launches had 9..36 tiles each and needed 7..28 slices (atomic traffic x4).
    VbReduceJobs tail{};
    DeferScope defer_scope(&tail);
    // 1-5. on all rows, in place
    Front f{M, M, nullptr, 0, d_out, sc.t_h0, sc.t_h1, d.x3 ? sc.sp_dpre : sc.t_i, sc.t_h2, sc.t_h5, sc.t_h4, sc.t_h3, sv.pre,
            sc.ln_ws, sc.ln_ws1, d.x3 ? sc.sp_dfo : nullptr, d.x3 ? sc.sp_dao : nullptr};
    VB_TRY(bwd_front(c, sv, h_out, f));
    // 6-9. attention backward, dgrad QKV
    unsigned char* sp_dqkv = d.x3 ? sc.sp_dqkv : nullptr;
    VB_TRY(bwd_tail(c, sv, f.dctx, f.dz1, sc.dsum, sc.t_3h, sp_dqkv, d_in));
    // 10. the four weight gradients: dW_fo[H,I] += dfo^T inter, dW_fi[I,H] += dpre^T a_out, dW_ao[H,H] += dao^T ctx,
    //     dW_qkv[3H,H] += dqkv^T h_in
    //     (split-operand mode: the dy images were split for the dgrads above; the four layer inputs' images were kept by the forward)
    const int64_t k = d.x3 ? 2 : 1;                          // columns of an operand per feature (split: hi | lo)
    WgradGroups wg;
    wg.add(f.dfo_op(), k * H, d.x3 ? sv.sp_inter : sv.inter, k * I, G[VB_LW_FO_W], I, H, I);
    wg.add(f.dpre, k * I, d.x3 ? sv.sp_aout : sv.a_out, k * H, G[VB_LW_FI_W], H, I, H);
    wg.add(f.dao_op(), k * H, d.x3 ? sv.sp_ctx : sv.ctx, k * H, G[VB_LW_AO_W], H, H, H);
    wg.add(d.x3 ? (const void*)sp_dqkv : (const void*)sc.t_3h, k * 3 * H, d.x3 ? (const void*)sv.sp_hin : h_in, k * H, G[VB_LW_QKV_W], H,
           3 * H, H);
    VB_TRY(wg.launch(dtype, M, stream));
    return vb_reduce_jobs_launch(tail, stream);
}

// ---- the backward over the rows that carry a gradient ---------------------------------------------------------------------------
// The LAST encoder layer of a model whose heads read a few rows of its output (the labelled and the [CLS] rows in pre-training: ~12 %;
// one row per sample under a pooled-only head) receives a d_out that is zero on every other row.  Steps 1-5 of the backward above and
// three of its four weight gradients act on one row at a time -- a zero row stays zero through all of them and adds exact zeros to
// every column sum and weight gradient -- so they run here on the compact rows only; the attention backward mixes rows, and from there
// on the layer is dense.
namespace {

constexpr int ROW_PAD = 256;          // compact row counts are rounded up to whole GEMM row tiles; padding rows carry a zero gradient

// scratch of the row-map backward: the dense temporaries it still needs first, the compact ones behind them
struct RowsScratch {
    unsigned char *dctx, *dz1, *t_3h;                                   // dense [M, .]: contiguous dctx | dz1 (cleared by one launch)
    float *dsum, *ln_ws, *ln_ws1;
    unsigned char *dz2_c, *dfo_c, *da_c, *dz1_c, *dao_c, *dctx_c, *aout_c, *ctx_c;      // compact [n_pad, H]
    unsigned char *pre_c, *inter_c, *dpre_c;                            // compact [n_pad, I]
    size_t total;
};
RowsScratch carve_rows_scratch(unsigned char* base, const Dims& d, long n_pad) {
    RowsScratch s;
    Carver c{base, 0};
    s.dctx = c.take((size_t)d.M * d.H * d.es);
    s.dz1 = c.take((size_t)d.M * d.H * d.es);
    s.t_3h = c.take((size_t)d.M * 3 * d.H * d.es);
    s.dsum = (float*)c.take((size_t)vb_attn_bwd_ws_floats((int)d.B, (int)d.S, (int)d.nh) * 4);
    s.ln_ws = (float*)c.take((size_t)vb_ln_bwd_ws_bytes((int)d.M, d.H));
    s.ln_ws1 = (float*)c.take((size_t)vb_ln_bwd_ws_bytes((int)d.M, d.H));
    const size_t ch = (size_t)n_pad * d.H * d.es, ci = (size_t)n_pad * d.I * d.es;
    s.dz2_c = c.take(ch); s.dfo_c = c.take(ch); s.da_c = c.take(ch); s.dz1_c = c.take(ch); s.dao_c = c.take(ch); s.dctx_c = c.take(ch);
    s.aout_c = c.take(ch); s.ctx_c = c.take(ch);
    s.pre_c = c.take(ci); s.inter_c = c.take(ci); s.dpre_c = c.take(ci);
    s.total = c.o;
    return s;
}
inline long rows_pad(int n_rows) { return ((long)n_rows + ROW_PAD - 1) / ROW_PAD * ROW_PAD; }

}  // namespace

extern "C" int64_t vb_bert_layer_bwd_rows_scratch_bytes(int dtype, int B, int S, int H, int I, int nh, int n_rows) {
    Dims d;
    if (!fill_dims(d, dtype, B, S, H, I, nh) || n_rows < 0 || n_rows > d.M) return -1;
    if (dtype != VB_BF16) return -1;
    return (int64_t)carve_rows_scratch(nullptr, d, rows_pad(n_rows)).total;
}

// rows[n_rows]: ascending int64 indices into B * S, on the device; d_out must be zero on every other row (the caller's promise: nothing
// here looks at the data).  Computes what vb_bert_layer_bwd computes from such a d_out.  bf16 only (VB_ERR_UNSUPPORTED otherwise: the
// caller takes the dense entry).  scratch: vb_bert_layer_bwd_rows_scratch_bytes() bytes.
extern "C" int vb_bert_layer_bwd_rows(int dtype, const void* h_in, const void* h_out, const float* mask_add, const void* d_out, void* d_in,
                                      const void* saved, void* scratch, const void* const* weights, void* const* grads,
                                      const void* const* weights_t, const int64_t* ld_t,
                                      int B, int S, int H, int I, int nh, float p_hidden, float p_attn,
                                      uint64_t seed, uint32_t sid, const int64_t* rows, int n_rows, void* stream) {
    Dims d;
    if (!fill_dims(d, dtype, B, S, H, I, nh) || !h_in || !mask_add || !d_out || !d_in || !saved || !scratch ||
        !weights || !grads || n_rows < 0 || n_rows > d.M || (n_rows > 0 && !rows))
        return VB_ERR_ARG;
    if (H <= 768 && !h_out) return VB_ERR_ARG;
    if (dtype != VB_BF16) return VB_ERR_UNSUPPORTED;
    Bwd c{d, unpack_weights(weights), weights_t, ld_t, mask_add, p_hidden, p_attn, seed, sid, stream, {}};
    if (!c.take_grads(grads)) return VB_ERR_ARG;
    float* const* G = c.G;
    const int M = (int)d.M;
    if (n_rows == 0) {                                      // d_out = 0: every gradient of the layer is an exact zero
        if (hipMemsetAsync(d_in, 0, (size_t)M * H * d.es, (hipStream_t)stream) != hipSuccess) return VB_ERR_LAUNCH;
        return VB_OK;
    }
    const int n_pad = (int)rows_pad(n_rows);
    Saved sv = carve_saved((unsigned char*)saved, d, p_attn > 0.f);
    RowsScratch sc = carve_rows_scratch((unsigned char*)scratch, d, n_pad);
    VbReduceJobs tail{};
    DeferScope defer_scope(&tail);
    const int hb = (int)(H * d.es), ib = (int)(I * d.es);
    // 0. the saved rows the compact GEMMs read: GELU', and the x operands of the three compact weight gradients
    {
        VbRowJobs g{{sv.pre, sv.inter, sv.a_out, sv.ctx}, {sc.pre_c, sc.inter_c, sc.aout_c, sc.ctx_c}, {ib, ib, hb, hb}, 4};
        VB_TRY(vb_rows_gather(g, rows, n_rows, n_pad, stream));
    }
    // 1-5. on the compact rows: d_out, the saved pre-LN sums / LayerNorm outputs and the statistics through the map, n_pad rows in
    //      the GEMMs
    Front f{n_pad, n_rows, rows, 1, d_out, sc.dz2_c, sc.dfo_c, sc.dpre_c, sc.da_c, sc.dz1_c, sc.dao_c, sc.dctx_c, sc.pre_c,
            sc.ln_ws, sc.ln_ws1, nullptr, nullptr};
    VB_TRY(bwd_front(c, sv, h_out, f));
    // 6. back to all rows: dctx and dz1 are zero outside the map
    VB_TRY(vb_zero(sc.dctx, (int64_t)((sc.dz1 - sc.dctx) + al((size_t)M * H * d.es)), stream));
    {
        VbRowJobs s2{{f.dctx, f.dz1}, {sc.dctx, sc.dz1}, {hb, hb}, 2};
        VB_TRY(vb_rows_scatter(s2, rows, n_rows, stream));
    }
    // 7-9. dense: attention backward, dh = dqkv Wqkv + dz1
    VB_TRY(bwd_tail(c, sv, sc.dctx, sc.dz1, sc.dsum, sc.t_3h, nullptr, d_in));
    // 10. weight gradients: FFN-out, FFN-in, attention-out over the compact rows (one launch), QKV over all rows
    WgradGroups wc;
    wc.add(f.dfo, H, sc.inter_c, I, G[VB_LW_FO_W], I, H, I);
    wc.add(f.dpre, I, sc.aout_c, H, G[VB_LW_FI_W], H, I, H);
    wc.add(f.dao, H, sc.ctx_c, H, G[VB_LW_AO_W], H, H, H);
    VB_TRY(wc.launch(dtype, n_pad, stream));
    WgradGroups wq;
    wq.add(sc.t_3h, 3 * H, h_in, H, G[VB_LW_QKV_W], H, 3 * H, H);
    VB_TRY(wq.launch(dtype, M, stream));
    return vb_reduce_jobs_launch(tail, stream);
}
