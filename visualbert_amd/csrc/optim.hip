// optim.hip -- fused multi-tensor optimizers over the flat parameter arena: BertAdam (below) and LAMB (vb_lamb_step_groups).
//
// Replaces BertAdam.step (pytorch_pretrained_bert/optimization.py:239-304), a Python loop over ~200
// tensors with ~10 small kernels each, by three launches over one contiguous fp32 arena:
//   1. per-TENSOR gradient sum of squares (the reference clips every tensor separately to
//      max_grad_norm with clip_grad_norm_, optimization.py:272-273)
//   2. update: m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2 ; u = m / (sqrt(v) + e) + wd * p ;
//      p -= lr * schedule(step) * u      -- no bias correction, eps OUTSIDE the sqrt, decoupled weight
//      decay, LR multiplier from the per-tensor step counter read BEFORE its increment (:292,297);
//      the bf16 shadow copy that the MFMA GEMMs read is refreshed in the same pass
//   3. step counters += 1
// HBM traffic per parameter: read p, g, m, v (16 B) + write p, m, v (12 B) [+ 2 B shadow] = 28-30 B.
// Everything the step needs lives on the device (chunk table, step counters, hyper-parameters): no
// host<->device traffic per step, so the step can sit in a captured graph.
// Two entries share the element loop: vb_bert_adam_step (one set of scalar hyper-parameters) and
// vb_bert_adam_step_groups (a device-resident table with one row per parameter group, :262-301).
//
// vb_lamb_step_groups -- LAMB (You et al., "Large Batch Optimization for Deep Learning", with the NVLAMB conventions: one GLOBAL
// gradient norm, optional bias correction, trust ratio per tensor) on the same arena, tables, group table (+ 2 columns), skip
// rule and norm kernels.  The trust ratio ||p|| / ||u|| of a tensor is known only after every element's update u is, so the
// element work is two passes, and u is RECOMPUTED in the second from the new moments instead of being kept in an arena-sized buffer:
//   1. per-tensor gradient sums of squares (the BertAdam kernels), then ONE wave adds them in table order: the global norm
//   2. moments: m, v updated and stored; u formed in registers; per-chunk partials of ||p||^2 and ||u||^2
//   3. per-tensor trust ratios from the partials, in table order
//   4. apply: u again from the stored m, v and the old p; p -= lr * schedule(step) * ratio * u; bf16 shadow
//   5. step counters += 1
// HBM traffic per parameter: pass 2 reads g, m, v, p (16 B) + writes m, v (8 B); pass 4 reads m, v, p (12 B) + writes p (4 B)
// [+ 2 B shadow] = 40-42 B, counted like BertAdam's 28-30 B (the norm pass adds 4 B to either).  A tensor whose ratio is 1 by rule
// (no weight decay, not always_adapt) skips the read of p in pass 2.  With bias_correction = always_adapt = 0, no weight decay and no
// clipping the result is bit for bit that of vb_bert_adam_step_groups: the element arithmetic is adam_update_chunk's, in its order.
#include "vb_rt.h"
#include "../../include/visualbert_hip.h"

namespace {

constexpr int NT = 256;

struct AdamHyper {
    float lr, b1, b2, eps, max_grad_norm, warmup, t_total, weight_decay;
    int schedule;      // 0 = none (multiplier 1), 1 = warmup_linear
};

// chunk table entry layout (int64 x 4): tensor id, arena offset of the chunk, length, number of chunks of this tensor
// tensor table entry layout (int64 x 4): arena offset, numel, shadow offset (-1: none), flags (bit0: optimise, bit1: decay)

// Squared gradient norms per tensor, DETERMINISTICALLY: a chunk's partial goes to its own slot and one thread per tensor
// adds its chunks' partials in table order.  (A float atomic per chunk made the clip coefficient differ in the last bit
// from run to run -- and between data-parallel replicas, whose weights then drift apart ulp by ulp.)
VB_DEVICE void chunk_norm2(const float* grads, const int64_t* c, float* red, float* out) {
    const long off = c[1], len = c[2];
    float s = 0.f;
    if (((off | len) & 3) == 0) {
        // 16-byte loads, four independent ones in flight per trip (the scalar rolled loop paid a memory round trip per
        // element: 145 us for 448 MB)
        const f32x4* g4 = (const f32x4*)(grads + off);
        const long n4 = len >> 2;
        long i = threadIdx.x;
        for (; i + 3 * NT < n4; i += 4 * NT) {
            const f32x4 a = g4[i], b = g4[i + NT], c2 = g4[i + 2 * NT], d = g4[i + 3 * NT];
            s += (a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + a[3] * a[3]) + (b[0] * b[0] + b[1] * b[1] + b[2] * b[2] + b[3] * b[3]) +
                 (c2[0] * c2[0] + c2[1] * c2[1] + c2[2] * c2[2] + c2[3] * c2[3]) + (d[0] * d[0] + d[1] * d[1] + d[2] * d[2] + d[3] * d[3]);
        }
        for (; i < n4; i += NT) { const f32x4 a = g4[i]; s += a[0] * a[0] + a[1] * a[1] + a[2] * a[2] + a[3] * a[3]; }
    } else {
        for (long i = threadIdx.x; i < len; i += NT) { const float g = grads[off + i]; s += g * g; }
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) *out = (red[0] + red[1]) + (red[2] + red[3]);
}
VB_KERNEL VB_LAUNCH_BOUNDS(NT) adam_norm_kernel(const float* grads, const int64_t* chunks, float* partial) {
    VB_DYN_SMEM(smem);
    chunk_norm2(grads, chunks + (long)blockIdx.x * 4, (float*)smem, partial + blockIdx.x);
}
// one wave per tensor (the workgroup of the tensor's FIRST chunk; the others leave): lane l adds the partials of chunks
// l, l + 64, ... in that order, then a fixed butterfly -- the same bits every time
VB_KERNEL VB_LAUNCH_BOUNDS(64) adam_norm_finish_kernel(const int64_t* chunks, int n_chunks, const float* partial, float* norm2) {
    const int j = blockIdx.x;
    const int64_t id = chunks[(long)j * 4];
    if (j > 0 && chunks[(long)(j - 1) * 4] == id) return;
    const int count = (int)chunks[(long)j * 4 + 3];                  // chunks of this tensor (adjacent in the table)
    float s = 0.f;
    for (int k = threadIdx.x; k < count; k += 64) s += partial[j + k];
    s = wave_sum(s);
    if (threadIdx.x == 0) norm2[id] = s;
}

VB_DEVICE float schedule_mult(const AdamHyper& h, int step) {
    if (h.schedule == 0 || h.t_total < 0.f) return 1.0f;
    // optimization.py:55-73 and :164-173, evaluated in double like the reference's Python floats
    const double progress = (double)step / (double)h.t_total;
    const double w = h.warmup > 0.f ? (double)h.warmup : 0.0;
    double r;
    if (progress < w) r = progress / w;
    else { r = (progress - 1.0) / (w - 1.0); if (r < 0.0) r = 0.0; }
    return (float)r;
}

// a tensor no backward pass has EVER written to (and whose gradient is zero): the reference's `if p.grad is None: continue`
// (optimization.py:254-255).  .grad stops being None at a parameter's first backward and zero_grad() leaves a zero tensor
// behind from then on, so the skip is sticky the other way round: once a tensor has taken a step (its counter is > 0) it
// takes every later step too (weight decay, moment decay, counter) even when this step wrote nothing to it.  Device-side,
// per step: no host-cached decision can go stale between data-parallel ranks.  The gradient norms are always computed when
// flags are given (host side below), so an unrecorded non-zero gradient is never dropped.
// ASSUMED zero_grad SEMANTICS: the reference's era (torch < 2: zero_grad() zeroes .grad in place, so .grad is None only before
// a parameter's first backward).  Under torch >= 2's default zero_grad(set_to_none=True) the REFERENCE would skip a tensor again
// in any later step that does not reach it; this library keeps the torch < 2 behaviour the reference was written and trained
// with (include/visualbert_hip.h: vb_bert_adam_step; visualbert_amd.optimization.BertAdam docstring).
VB_DEVICE bool adam_skips(const float* touched, const float* norm2, const int* steps, long tid) {
    if (!touched || touched[tid] != 0.f || steps[tid] > 0) return false;
    return !(norm2[tid] > 0.f);
}

// one chunk of one tensor, every hyper-parameter already reduced to the six floats of this tensor and step
// (4-byte accesses on purpose: a wave's load is 256 contiguous bytes per array and many of them are in flight.  The 16-byte form --
// a quarter of the memory instructions -- measured SLOWER in the step, 632 vs 554 us at B = 8 on the 3.3 GB pass; round 6, not kept)
VB_DEVICE void adam_update_chunk(float* params, const float* grads, float* m, float* v, bf16* shadow, long off, long len,
                                 long t_off, long sh_off, float lr, float b1, float b2, float eps, float wd, float clip) {
    for (long i = threadIdx.x; i < len; i += NT) {
        const long e = off + i;
        const float g = grads[e] * clip;
        const float p = params[e];
        const float mm = m[e] * b1 + (1.0f - b1) * g;
        const float vv = v[e] * b2 + (1.0f - b2) * g * g;
        float u = mm / (sqrtf(vv) + eps);
        if (wd > 0.f) u += wd * p;
        const float pn = p - lr * u;
        m[e] = mm; v[e] = vv; params[e] = pn;
        if (shadow && sh_off >= 0) shadow[sh_off + (e - t_off)] = (bf16)pn;
    }
}

VB_KERNEL VB_LAUNCH_BOUNDS(NT) adam_update_kernel(float* params, const float* grads, float* m, float* v, bf16* shadow,
                                                 const int64_t* chunks, const int64_t* tensors, const float* norm2,
                                                 const int* steps, const float* touched, AdamHyper h) {
    const int64_t* c = chunks + (long)blockIdx.x * 4;
    const long tid = c[0], off = c[1], len = c[2];
    const int64_t* te = tensors + tid * 4;
    const long t_off = te[0], sh_off = te[2], flags = te[3];
    if (!(flags & 1)) return;
    if (adam_skips(touched, norm2, steps, tid)) return;
    const float wd = (flags & 2) ? h.weight_decay : 0.0f;
    float clip = 1.0f;
    if (h.max_grad_norm > 0.f) {
        const float cc = h.max_grad_norm / (sqrtf(norm2[tid]) + 1e-6f);
        clip = cc < 1.0f ? cc : 1.0f;
    }
    const float lr = h.lr * schedule_mult(h, steps[tid]);
    adam_update_chunk(params, grads, m, v, shadow, off, len, t_off, sh_off, lr, h.b1, h.b2, h.eps, wd, clip);
}

VB_KERNEL adam_step_inc_kernel(int* steps, const int64_t* tensors, int n, const float* touched, const float* norm2) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && (tensors[(long)i * 4 + 3] & 1) && !adam_skips(touched, norm2, steps, i)) steps[i] += 1;
}

// ---- per-group hyper-parameters (vb_bert_adam_step_groups) -------------------------------------------------------------
// group table row (fp64 x GROUP_COLS): lr, b1, b2, eps, weight_decay, max_grad_norm, schedule code, warmup, t_total, cycles,
// host multiplier.  A tensor's group id is flags >> 2 of its tensor-table entry.  A chunk belongs to one tensor, so its row is
// uniform per workgroup: it is read (scalar loads) and reduced to six floats before the element loop, which is the loop of
// adam_update_kernel.
constexpr int GROUP_COLS = 11;
enum { G_LR = 0, G_B1, G_B2, G_EPS, G_WD, G_CLIP, G_SCHED, G_WARMUP, G_TTOTAL, G_CYCLES, G_HOSTMULT };
enum { SCHED_NONE = 0, SCHED_WARMUP_LINEAR, SCHED_WARMUP_CONSTANT, SCHED_WARMUP_COSINE, SCHED_COSINE_HARD_RESTARTS,
       SCHED_COSINE_WARMUP_RESTARTS, SCHED_HOST, SCHED_COUNT };

// the row of tensor `tid`, or NULL when the tensor takes no part: not optimised, or -- only reachable when the caller passed
// validate = 0 with a bad table -- a group id outside the table or an unknown schedule code (never read outside the table)
VB_DEVICE const double* adam_group_row(const int64_t* tensors, long tid, const double* groups, int n_groups,
                                       int cols = GROUP_COLS) {
    const long flags = tensors[tid * 4 + 3];
    if (!(flags & 1)) return nullptr;
    const long gid = flags >> 2;
    if (gid < 0 || gid >= n_groups) return nullptr;
    const double* row = groups + gid * cols;
    const double code = row[G_SCHED];
    if (!(code >= 0.0 && code < (double)SCHED_COUNT) || code != (double)(int)code) return nullptr;
    return row;
}

// _LRSchedule.get_lr and the get_lr_ of its six classes (optimization.py:55-73, :83-173), in double and in the reference's
// operation order (no contraction: -ffp-contract=off).  progress is never negative, so Python's float % is fmod.
VB_DEVICE double schedule_mult_group(const double* row, int step) {
    const int code = (int)row[G_SCHED];
    if (code == SCHED_HOST) return row[G_HOSTMULT];
    const double t_total = row[G_TTOTAL];
    if (code == SCHED_NONE || t_total < 0.0) return 1.0;
    const double w = row[G_WARMUP] > 0.0 ? row[G_WARMUP] : 0.0, cycles = row[G_CYCLES];
    const double pi = 3.141592653589793;
    double progress = (double)step / t_total;
    if (code == SCHED_COSINE_WARMUP_RESTARTS) progress = fmod(progress * cycles, 1.0);
    if (progress < w) return progress / w;
    if (code == SCHED_WARMUP_CONSTANT) return 1.0;
    if (code == SCHED_WARMUP_LINEAR) { const double r = (progress - 1.0) / (w - 1.0); return r < 0.0 ? 0.0 : r; }
    progress = (progress - w) / (1.0 - w);
    if (code == SCHED_WARMUP_COSINE) return 0.5 * (1.0 + cos(pi * cycles * 2.0 * progress));
    if (code == SCHED_COSINE_HARD_RESTARTS) return 0.5 * (1.0 + cos(pi * fmod(cycles * progress, 1.0)));
    return 0.5 * (1.0 + cos(pi * progress));
}

// the norm of a chunk is needed when its tensor's group clips or when the skip rule will read it (touched given); otherwise its
// slot is zeroed, so that the finish kernel still sums defined values
VB_KERNEL VB_LAUNCH_BOUNDS(NT) adam_norm_groups_kernel(const float* grads, const int64_t* chunks, const int64_t* tensors,
                                                      const double* groups, int n_groups, const float* touched, float* partial) {
    VB_DYN_SMEM(smem);
    const int64_t* c = chunks + (long)blockIdx.x * 4;
    const double* row = adam_group_row(tensors, c[0], groups, n_groups);
    if (!row || (!touched && !(row[G_CLIP] > 0.0))) {
        if (threadIdx.x == 0) partial[blockIdx.x] = 0.f;
        return;
    }
    chunk_norm2(grads, c, (float*)smem, partial + blockIdx.x);
}

VB_KERNEL VB_LAUNCH_BOUNDS(NT) adam_update_groups_kernel(float* params, const float* grads, float* m, float* v, bf16* shadow,
                                                        const int64_t* chunks, const int64_t* tensors, const float* norm2,
                                                        const int* steps, const float* touched, const double* groups,
                                                        int n_groups) {
    const int64_t* c = chunks + (long)blockIdx.x * 4;
    const long tid = c[0], off = c[1], len = c[2];
    const double* row = adam_group_row(tensors, tid, groups, n_groups);
    if (!row) return;
    if (adam_skips(touched, norm2, steps, tid)) return;
    const int64_t* te = tensors + tid * 4;
    const long t_off = te[0], sh_off = te[2];
    const float max_grad_norm = (float)row[G_CLIP];
    float clip = 1.0f;
    if (max_grad_norm > 0.f) {
        const float cc = max_grad_norm / (sqrtf(norm2[tid]) + 1e-6f);
        clip = cc < 1.0f ? cc : 1.0f;
    }
    const float lr = (float)row[G_LR] * (float)schedule_mult_group(row, steps[tid]);
    adam_update_chunk(params, grads, m, v, shadow, off, len, t_off, sh_off, lr, (float)row[G_B1], (float)row[G_B2],
                      (float)row[G_EPS], (float)row[G_WD], clip);
}

VB_KERNEL adam_step_inc_groups_kernel(int* steps, const int64_t* tensors, int n, const float* touched, const float* norm2,
                                      const double* groups, int n_groups) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && adam_group_row(tensors, i, groups, n_groups) && !adam_skips(touched, norm2, steps, i)) steps[i] += 1;
}

// argument check of the device-resident tables: they are read back (this waits for the stream), so the caller asks for it only
// when a table is new
static int adam_groups_validate(const int64_t* tensor_table, int n_tensors, const double* group_table, int n_groups,
                                hipStream_t s, int cols = GROUP_COLS) {
    int64_t* tt = (int64_t*)malloc((size_t)n_tensors * 4 * sizeof(int64_t));
    double* gt = (double*)malloc((size_t)n_groups * cols * sizeof(double));
    int rc = (tt && gt) ? VB_OK : VB_ERR_LAUNCH;
#ifdef VB_EMU
    if (rc == VB_OK) {
        memcpy(tt, tensor_table, (size_t)n_tensors * 4 * sizeof(int64_t));
        memcpy(gt, group_table, (size_t)n_groups * cols * sizeof(double));
    }
#else
    if (rc == VB_OK && (hipMemcpyAsync(tt, tensor_table, (size_t)n_tensors * 4 * sizeof(int64_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
                        hipMemcpyAsync(gt, group_table, (size_t)n_groups * cols * sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess ||
                        hipStreamSynchronize(s) != hipSuccess))
        rc = VB_ERR_LAUNCH;
#endif
    for (int i = 0; rc == VB_OK && i < n_tensors; ++i) {
        const int64_t flags = tt[(size_t)i * 4 + 3];
        if ((flags & 1) && ((flags >> 2) < 0 || (flags >> 2) >= n_groups)) rc = VB_ERR_ARG;
    }
    for (int g = 0; rc == VB_OK && g < n_groups; ++g) {
        const double code = gt[(size_t)g * cols + G_SCHED];
        if (!(code >= 0.0 && code < (double)SCHED_COUNT) || code != (double)(int)code) rc = VB_ERR_ARG;
    }
    free(tt);
    free(gt);
    return rc;
}

// ---- LAMB (vb_lamb_step_groups) ------------------------------------------------------------------------------------------
// group table row (fp64 x LAMB_COLS): the GROUP_COLS columns above in the same order, then bias_correction (0/1) and
// always_adapt (0/1).  workspace (fp32): per-tensor ||g||^2 [n_tensors] | per-tensor trust ratio [n_tensors] | global ||g||^2
// [4, one used] | per-chunk partials of ||g||^2, ||p||^2, ||u||^2 [3 x n_chunks].  Every sum is formed without atomics: a chunk's
// partial has its own slot and one wave adds a tensor's (or the table's) slots in table order -- the reason given at chunk_norm2.
constexpr int LAMB_COLS = GROUP_COLS + 2;
enum { L_BIAS_CORRECTION = GROUP_COLS, L_ALWAYS_ADAPT };

// the row of a tensor that takes this step, or NULL (not optimised, bad row under validate = 0, or skipped by adam_skips)
VB_DEVICE const double* lamb_row(const int64_t* tensors, long tid, const double* groups, int n_groups, const float* touched,
                                 const float* norm2, const int* steps) {
    const double* row = adam_group_row(tensors, tid, groups, n_groups, LAMB_COLS);
    if (!row || adam_skips(touched, norm2, steps, tid)) return nullptr;
    return row;
}

// every optimised tensor's norm is needed: the clip coefficient comes from the norm over ALL groups
VB_KERNEL VB_LAUNCH_BOUNDS(NT) lamb_norm_kernel(const float* grads, const int64_t* chunks, const int64_t* tensors,
                                               const double* groups, int n_groups, float* partial) {
    VB_DYN_SMEM(smem);
    const int64_t* c = chunks + (long)blockIdx.x * 4;
    if (!adam_group_row(tensors, c[0], groups, n_groups, LAMB_COLS)) {
        if (threadIdx.x == 0) partial[blockIdx.x] = 0.f;
        return;
    }
    chunk_norm2(grads, c, (float*)smem, partial + blockIdx.x);
}

// one wave: lane l adds the norms of tensors l, l + 64, ... that take this step, then the fixed butterfly
VB_KERNEL VB_LAUNCH_BOUNDS(64) lamb_global_norm_kernel(const int64_t* tensors, int n_tensors, const double* groups, int n_groups,
                                                      const float* touched, const float* norm2, const int* steps, float* gnorm2) {
    float s = 0.f;
    for (int t = threadIdx.x; t < n_tensors; t += 64)
        if (lamb_row(tensors, t, groups, n_groups, touched, norm2, steps)) s += norm2[t];
    s = wave_sum(s);
    if (threadIdx.x == 0) *gnorm2 = s;
}

struct LambHyper { float b1, b2, eps, wd, c1, c2; bool bias_correction; };

VB_DEVICE LambHyper lamb_hyper(const double* row, int step) {
    LambHyper h;
    h.b1 = (float)row[G_B1]; h.b2 = (float)row[G_B2]; h.eps = (float)row[G_EPS]; h.wd = (float)row[G_WD];
    h.bias_correction = row[L_BIAS_CORRECTION] != 0.0;
    h.c1 = h.c2 = 1.0f;
    if (h.bias_correction) {                         // 1 - beta^t of the fp32 betas the element loop uses, t = step + 1
        h.c1 = (float)(1.0 - pow((double)h.b1, (double)(step + 1)));
        h.c2 = (float)(1.0 - pow((double)h.b2, (double)(step + 1)));
    }
    return h;
}

// the update direction of one element from its NEW moments and its OLD parameter: adam_update_chunk's expression, with the
// moments divided by 1 - beta^t first when the group asks for bias correction.  Both element passes call this, so the u whose
// norm sets the trust ratio and the u that is applied are the same bits.
VB_DEVICE float lamb_direction(float mm, float vv, float p, const LambHyper& h) {
    if (h.bias_correction) { mm = mm / h.c1; vv = vv / h.c2; }
    float u = mm / (sqrtf(vv) + h.eps);
    if (h.wd > 0.f) u += h.wd * p;
    return u;
}

// the trust ratio is 1 by rule for a tensor without weight decay unless its group adapts always: no norm is formed for it
VB_DEVICE bool lamb_adapts(const double* row) { return (float)row[G_WD] > 0.f || row[L_ALWAYS_ADAPT] != 0.0; }

// pass 2: moments of one chunk (4-byte accesses as in adam_update_chunk) + this chunk's partials of ||p||^2 and ||u||^2
// (the four arena buffers never overlap: __restrict__ lets the loads of the next trip start before this trip's stores)
VB_KERNEL VB_LAUNCH_BOUNDS(NT) lamb_moments_kernel(const float* __restrict__ params, const float* __restrict__ grads,
                                                  float* __restrict__ m, float* __restrict__ v,
                                                  const int64_t* chunks, const int64_t* tensors, const float* norm2,
                                                  const float* gnorm2, const int* steps, const float* touched,
                                                  const double* groups, int n_groups, float* partial_p, float* partial_u) {
    VB_DYN_SMEM(smem);
    float* red = (float*)smem;                                       // [2][4]
    const int64_t* c = chunks + (long)blockIdx.x * 4;
    const long tid = c[0], off = c[1], len = c[2];
    const double* row = lamb_row(tensors, tid, groups, n_groups, touched, norm2, steps);
    if (!row) {
        if (threadIdx.x == 0) { partial_p[blockIdx.x] = 0.f; partial_u[blockIdx.x] = 0.f; }
        return;
    }
    const LambHyper h = lamb_hyper(row, steps[tid]);
    const float max_grad_norm = (float)row[G_CLIP];
    float clip = 1.0f;
    if (max_grad_norm > 0.f) {
        const float cc = max_grad_norm / (sqrtf(*gnorm2) + 1e-6f);
        clip = cc < 1.0f ? cc : 1.0f;
    }
    const bool adapts = lamb_adapts(row);
    float sp = 0.f, su = 0.f;
    for (long i = threadIdx.x; i < len; i += NT) {
        const long e = off + i;
        const float g = grads[e] * clip;
        const float mm = m[e] * h.b1 + (1.0f - h.b1) * g;
        const float vv = v[e] * h.b2 + (1.0f - h.b2) * g * g;
        m[e] = mm; v[e] = vv;
        if (adapts) {
            const float p = params[e];
            const float u = lamb_direction(mm, vv, p, h);
            sp += p * p; su += u * u;
        }
    }
    sp = wave_sum(sp); su = wave_sum(su);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6] = sp; red[4 + (threadIdx.x >> 6)] = su; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial_p[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
        partial_u[blockIdx.x] = (red[4] + red[5]) + (red[6] + red[7]);
    }
}

// pass 3: one wave per tensor, as adam_norm_finish_kernel.  A tensor that formed no norms has zero partials: ratio 1.
VB_KERNEL VB_LAUNCH_BOUNDS(64) lamb_ratio_kernel(const int64_t* chunks, int n_chunks, const float* partial_p,
                                                const float* partial_u, float* ratio) {
    const int j = blockIdx.x;
    const int64_t id = chunks[(long)j * 4];
    if (j > 0 && chunks[(long)(j - 1) * 4] == id) return;
    const int count = (int)chunks[(long)j * 4 + 3];
    float sp = 0.f, su = 0.f;
    for (int k = threadIdx.x; k < count; k += 64) { sp += partial_p[j + k]; su += partial_u[j + k]; }
    sp = wave_sum(sp); su = wave_sum(su);
    if (threadIdx.x == 0) ratio[id] = (sp > 0.f && su > 0.f) ? sqrtf(sp) / sqrtf(su) : 1.0f;
}

// pass 4: the direction again from the stored moments, applied with the tensor's ratio
VB_KERNEL VB_LAUNCH_BOUNDS(NT) lamb_apply_kernel(float* __restrict__ params, const float* __restrict__ m,
                                                const float* __restrict__ v, bf16* __restrict__ shadow,
                                                const int64_t* chunks, const int64_t* tensors, const float* norm2,
                                                const float* ratio, const int* steps, const float* touched,
                                                const double* groups, int n_groups) {
    const int64_t* c = chunks + (long)blockIdx.x * 4;
    const long tid = c[0], off = c[1], len = c[2];
    const double* row = lamb_row(tensors, tid, groups, n_groups, touched, norm2, steps);
    if (!row) return;
    const int64_t* te = tensors + tid * 4;
    const long t_off = te[0], sh_off = te[2];
    const LambHyper h = lamb_hyper(row, steps[tid]);
    const float lr = (float)row[G_LR] * (float)schedule_mult_group(row, steps[tid]) * ratio[tid];
    for (long i = threadIdx.x; i < len; i += NT) {
        const long e = off + i;
        const float p = params[e];
        const float u = lamb_direction(m[e], v[e], p, h);
        const float pn = p - lr * u;
        params[e] = pn;
        if (shadow && sh_off >= 0) shadow[sh_off + (e - t_off)] = (bf16)pn;
    }
}

VB_KERNEL lamb_step_inc_kernel(int* steps, const int64_t* tensors, int n, const float* touched, const float* norm2,
                               const double* groups, int n_groups) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && lamb_row(tensors, i, groups, n_groups, touched, norm2, steps)) steps[i] += 1;
}

VB_KERNEL VB_LAUNCH_BOUNDS(NT) shadow_refresh_kernel(const float* params, bf16* shadow, const int64_t* chunks,
                                                    const int64_t* tensors) {
    const int64_t* c = chunks + (long)blockIdx.x * 4;
    const long tid = c[0], off = c[1], len = c[2];
    const long t_off = tensors[tid * 4], sh_off = tensors[tid * 4 + 2];
    if (sh_off < 0) return;
    for (long i = threadIdx.x; i < len; i += NT) shadow[sh_off + (off + i - t_off)] = (bf16)params[off + i];
}


// multi-tensor tiled transpose of bf16 weight shadows: for every GEMM weight W [R,C] keep W^T [C, R_pad]
// so that dgrad (dx = dy W) runs as a K-contiguous x K-contiguous GEMM with LDS-direct loads.
// tensors: int64[n][5] = {src offset, R, C, dst offset, dst ld}; tiles: int64[n_tiles][3] = {tensor, tile row, tile col}
VB_KERNEL VB_LAUNCH_BOUNDS(NT) shadow_transpose_kernel(const bf16* src, bf16* dst, const int64_t* tensors,
                                                      const int64_t* tiles) {
    VB_DYN_SMEM(smem);
    bf16* tile = (bf16*)smem;                       // [64][66]
    const int64_t* tl = tiles + (long)blockIdx.x * 3;
    const int64_t* te = tensors + tl[0] * 5;
    const long soff = te[0], R = te[1], C = te[2], doff = te[3], dld = te[4];
    const long r0 = tl[1] * 64, c0 = tl[2] * 64;
    // interior tiles of 16-byte aligned tensors move whole 16-byte vectors on both sides (the element-wise form below
    // took 232 us per step for 85 M weights: 1.4 TB/s)
    const bool fast = r0 + 64 <= R && c0 + 64 <= C && (C & 7) == 0 && (dld & 7) == 0 && (soff & 7) == 0 && (doff & 7) == 0;
    if (fast) {
        for (int i = threadIdx.x; i < 64 * 8; i += NT) {
            const int r = i >> 3, cc = (i & 7) * 8;
            const u32x4 v = *(const u32x4*)(src + soff + (r0 + r) * C + c0 + cc);
            uint32_t* t32 = (uint32_t*)(tile + r * 66 + cc);
            t32[0] = v[0]; t32[1] = v[1]; t32[2] = v[2]; t32[3] = v[3];
        }
        __syncthreads();
        for (int i = threadIdx.x; i < 64 * 8; i += NT) {
            const int c = i >> 3, rr = (i & 7) * 8;      // output row = source column
            bf16x8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = tile[(rr + j) * 66 + c];
            *(bf16x8*)(dst + doff + (c0 + c) * dld + r0 + rr) = o;
        }
        return;
    }
    for (int i = threadIdx.x; i < 64 * 8; i += NT) {
        const int r = i >> 3, cc = (i & 7) * 8;
        const long gr = r0 + r, gc = c0 + cc;
        bf16 v[8];
        for (int j = 0; j < 8; ++j) v[j] = (gr < R && gc + j < C) ? src[soff + gr * C + gc + j] : (bf16)0.0f;
        for (int j = 0; j < 8; ++j) tile[r * 66 + cc + j] = v[j];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * 8; i += NT) {
        const int c = i >> 3, rr = (i & 7) * 8;      // output row = source column
        const long gc = c0 + c, gr = r0 + rr;
        if (gc >= C) continue;
        for (int j = 0; j < 8; ++j) if (gr + j < R) dst[doff + gc * dld + gr + j] = tile[(rr + j) * 66 + c];
    }
}

}  // namespace

extern "C" int vb_bert_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                                 void* bf16_shadow, const int64_t* chunk_table, int n_chunks,
                                 const int64_t* tensor_table, int n_tensors, const float* touched, float* norm2_ws,
                                 int* step_counters,
                                 float lr, float b1, float b2, float eps, float weight_decay,
                                 float max_grad_norm, float warmup, float t_total, int schedule, void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !chunk_table || !tensor_table || !norm2_ws || !step_counters)
        return VB_ERR_ARG;
    if (n_chunks <= 0 || n_tensors <= 0 || (schedule != 0 && schedule != 1)) return VB_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    AdamHyper h{lr, b1, b2, eps, max_grad_norm, warmup, t_total, weight_decay, schedule};
    if (max_grad_norm > 0.f || touched) {                   // the skip decision reads the norms too
        float* partial = norm2_ws + n_tensors;              // [n_chunks]
        VB_LAUNCH(adam_norm_kernel, dim3((unsigned)n_chunks), dim3(NT), 64, s, grads, chunk_table, partial);
        VB_LAUNCH(adam_norm_finish_kernel, dim3((unsigned)n_chunks), dim3(64), 0, s, chunk_table, n_chunks,
                  (const float*)partial, norm2_ws);
    }
    VB_LAUNCH(adam_update_kernel, dim3((unsigned)n_chunks), dim3(NT), 0, s, params, grads, exp_avg, exp_avg_sq,
              (bf16*)bf16_shadow, chunk_table, tensor_table, (const float*)norm2_ws, (const int*)step_counters, touched, h);
    VB_LAUNCH(adam_step_inc_kernel, dim3((unsigned)((n_tensors + 63) / 64)), dim3(64), 0, s, step_counters,
              tensor_table, n_tensors, touched, (const float*)norm2_ws);
    return vb_check_launch();
}

extern "C" int vb_bert_adam_step_groups(float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                                        void* bf16_shadow, const int64_t* chunk_table, int n_chunks,
                                        const int64_t* tensor_table, int n_tensors, const float* touched, float* norm2_ws,
                                        int* step_counters, const double* group_table, int n_groups, int validate,
                                        void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !chunk_table || !tensor_table || !norm2_ws || !step_counters)
        return VB_ERR_ARG;
    if (n_chunks <= 0 || n_tensors <= 0 || !group_table || n_groups <= 0) return VB_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (validate) {
        const int rc = adam_groups_validate(tensor_table, n_tensors, group_table, n_groups, s);
        if (rc != VB_OK) return rc;
    }
    // whether a group clips is in the table, on the device: the norm kernel decides per chunk (a chunk that needs no norm costs
    // one empty workgroup)
    float* partial = norm2_ws + n_tensors;                  // [n_chunks]
    VB_LAUNCH(adam_norm_groups_kernel, dim3((unsigned)n_chunks), dim3(NT), 64, s, grads, chunk_table, tensor_table,
              group_table, n_groups, touched, partial);
    VB_LAUNCH(adam_norm_finish_kernel, dim3((unsigned)n_chunks), dim3(64), 0, s, chunk_table, n_chunks,
              (const float*)partial, norm2_ws);
    VB_LAUNCH(adam_update_groups_kernel, dim3((unsigned)n_chunks), dim3(NT), 0, s, params, grads, exp_avg, exp_avg_sq,
              (bf16*)bf16_shadow, chunk_table, tensor_table, (const float*)norm2_ws, (const int*)step_counters, touched,
              group_table, n_groups);
    VB_LAUNCH(adam_step_inc_groups_kernel, dim3((unsigned)((n_tensors + 63) / 64)), dim3(64), 0, s, step_counters,
              tensor_table, n_tensors, touched, (const float*)norm2_ws, group_table, n_groups);
    return vb_check_launch();
}

extern "C" int64_t vb_lamb_ws_floats(int n_tensors, int n_chunks) {
    if (n_tensors <= 0 || n_chunks <= 0) return -1;
    return 2 * (int64_t)n_tensors + 4 + 3 * (int64_t)n_chunks;
}

extern "C" int vb_lamb_step_groups(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, void* bf16_shadow,
                                   const int64_t* chunk_table, int n_chunks, const int64_t* tensor_table, int n_tensors,
                                   const float* touched, float* ws, int* step_counters, const double* group_table,
                                   int n_groups, int validate, void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !chunk_table || !tensor_table || !ws || !step_counters)
        return VB_ERR_ARG;
    if (n_chunks <= 0 || n_tensors <= 0 || !group_table || n_groups <= 0) return VB_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (validate) {
        const int rc = adam_groups_validate(tensor_table, n_tensors, group_table, n_groups, s, LAMB_COLS);
        if (rc != VB_OK) return rc;
    }
    float* norm2 = ws;                                      // [n_tensors]
    float* ratio = norm2 + n_tensors;                       // [n_tensors]
    float* gnorm2 = ratio + n_tensors;                      // [4]
    float* partial_g = gnorm2 + 4;                          // [n_chunks] each
    float* partial_p = partial_g + n_chunks;
    float* partial_u = partial_p + n_chunks;
    const int* steps = step_counters;
    VB_LAUNCH(lamb_norm_kernel, dim3((unsigned)n_chunks), dim3(NT), 64, s, grads, chunk_table, tensor_table, group_table,
              n_groups, partial_g);
    VB_LAUNCH(adam_norm_finish_kernel, dim3((unsigned)n_chunks), dim3(64), 0, s, chunk_table, n_chunks,
              (const float*)partial_g, norm2);
    VB_LAUNCH(lamb_global_norm_kernel, dim3(1), dim3(64), 0, s, tensor_table, n_tensors, group_table, n_groups, touched,
              (const float*)norm2, steps, gnorm2);
    VB_LAUNCH(lamb_moments_kernel, dim3((unsigned)n_chunks), dim3(NT), 64, s, (const float*)params, grads, exp_avg,
              exp_avg_sq, chunk_table, tensor_table, (const float*)norm2, (const float*)gnorm2, steps, touched, group_table,
              n_groups, partial_p, partial_u);
    VB_LAUNCH(lamb_ratio_kernel, dim3((unsigned)n_chunks), dim3(64), 0, s, chunk_table, n_chunks, (const float*)partial_p,
              (const float*)partial_u, ratio);
    VB_LAUNCH(lamb_apply_kernel, dim3((unsigned)n_chunks), dim3(NT), 0, s, params, (const float*)exp_avg,
              (const float*)exp_avg_sq, (bf16*)bf16_shadow, chunk_table, tensor_table, (const float*)norm2,
              (const float*)ratio, steps, touched, group_table, n_groups);
    VB_LAUNCH(lamb_step_inc_kernel, dim3((unsigned)((n_tensors + 63) / 64)), dim3(64), 0, s, step_counters, tensor_table,
              n_tensors, touched, (const float*)norm2, group_table, n_groups);
    return vb_check_launch();
}

extern "C" int vb_refresh_bf16_shadow(const float* params, void* bf16_shadow, const int64_t* chunk_table,
                                      int n_chunks, const int64_t* tensor_table, void* stream) {
    if (!params || !bf16_shadow || !chunk_table || !tensor_table || n_chunks <= 0) return VB_ERR_ARG;
    VB_LAUNCH(shadow_refresh_kernel, dim3((unsigned)n_chunks), dim3(NT), 0, (hipStream_t)stream, params,
              (bf16*)bf16_shadow, chunk_table, tensor_table);
    return vb_check_launch();
}

extern "C" int vb_refresh_transposed_shadow(const void* bf16_shadow, void* bf16_shadow_t, const int64_t* tensor_table5,
                                            const int64_t* tile_table3, int n_tiles, void* stream) {
    if (!bf16_shadow || !bf16_shadow_t || !tensor_table5 || !tile_table3 || n_tiles <= 0) return VB_ERR_ARG;
    VB_LAUNCH(shadow_transpose_kernel, dim3((unsigned)n_tiles), dim3(NT), 64 * 66 * 2, (hipStream_t)stream,
              (const bf16*)bf16_shadow, (bf16*)bf16_shadow_t, tensor_table5, tile_table3);
    return vb_check_launch();
}
