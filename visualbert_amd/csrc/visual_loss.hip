// visual_loss.hip -- the masked-region objective of the sibling LXRT model: three per-region losses and their gradients in one
// sweep over one score matrix.
//   reference: LXRTPretraining.forward, unsupervised_visualbert/src/lxrt/modeling.py:1391-1420 (heads: BertVisualObjHead :971-996)
//     obj  / attr : CrossEntropyLoss(ignore_index=-1, reduction='none') over 1600 / 400 detector classes
//     feat        : SmoothL1Loss(reduction='none') against the region's 2048-d feature, .mean(1)
//     each        : (loss_r * mask_conf_r).mean() * weight        -- the mean runs over ALL M = B * R regions
//
// Memory plan.  scores is T [M, ld]: object logits | attribute logits | feature prediction | padding.  A row is at most 4096
// columns (16 KB of fp32), so ONE WAVE owns a row and keeps it in registers (8 x 8 floats per lane): every score is read from
// memory once, the maxima, the sums of exponentials, the label logits and the SmoothL1 sum come from wave shuffles (no LDS, no
// barrier), and the gradient is written from the registers -- which is why dscores may alias scores.  Of a row's vectors only
// those that touch a segment with a non-zero weight are loaded; a row whose three weights are all zero (label -1 or confidence 0
// for the class terms, mask 0 for the feature term: the common row, ~85 % of the feature masks are 0) takes a wave-uniform
// branch that reads nothing and zero-fills its gradient row.
//
// Reproducibility.  No float atomics: every row stores its three confidence-weighted losses into ws ([3][M]) and a second,
// single-workgroup launch adds them in a fixed order -- the four results are bit-identical from run to run and from stream to
// stream, like everything else the data-parallel replicas compare.
#include "vb_rt.h"
#include "../../include/visualbert_hip.h"

namespace {

constexpr int NT = 256;                       // four waves = four rows per workgroup
constexpr int ROWS = NT / 64;
constexpr int IT = 8;                         // vectors of 8 columns per lane
constexpr int MAXW = IT * 64 * 8;             // 4096 columns
constexpr int FIN_NT = 1024;

// exp(x) for x <= 0 to about one ulp: fast_exp alone rounds x * log2(e) to fp32 before the hardware 2^t, a relative error of up to
// |t| 2^-24 in the result; here the product's rounding residual (one fma) and the fp32 constant's own residual are put back to first order.
// Four more VALU operations per element of a kernel that waits on memory; they buy the losses their last bit (tests/test_visual_loss.py).
VB_DEVICE float exp_1ulp(float x) {
    const float L = 1.44269504088896340736f, L_LO = 1.92596299112661746e-8f;        // log2(e) = L + L_LO
    const float t = x * L;
    const float r = __builtin_fmaf(x, L, -t) + x * L_LO;
    const float p = fast_exp2(t);
    return __builtin_fmaf(p, r * 0.69314718055994530942f, p);
}

VB_DEVICE float smooth_l1(float e) {                         // beta = 1
    const float ae = fabsf(e);
    return ae < 1.f ? 0.5f * e * e : ae - 0.5f;
}

// where the 8 columns from j lie: 0 / 1 / 2 = wholly inside the object / attribute / feature segment, 3 = across a boundary or the
// row's end (handled per element), 4 = past the row
VB_DEVICE int vec_kind(int j, int o1, int o2, int o3) {
    if (j >= o3) return 4;
    if (j + 8 <= o1) return 0;
    if (j >= o1 && j + 8 <= o2) return 1;
    if (j >= o2 && j + 8 <= o3) return 2;
    return 3;
}

template <typename T, bool VEC>
VB_DEVICE void zero_row(T* drow, long from, long ldd, int lane) {
    if (VEC) {
        const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (long j = from + (long)lane * 8; j < ldd; j += 64 * 8) store8(drow + j, z);
    } else {
        for (long j = from + lane; j < ldd; j += 64) drow[j] = from_f32<T>(0.f);
    }
}

// g_obj = w_obj / M, g_attr = w_attr / M, g_feat = w_feat / (M n_feat): the gradient scales without the row's confidence.
// VEC: both pitches are multiples of 8 and both bases 16-byte aligned (the host checks); tvec: the same for 4-float reads of the target
// at the feature segment's offset.
// Four waves per SIMD: 98 - 114 VGPRs, no scratch (unbounded, the allocator takes 130 - 146 and a wave less).
template <typename T, bool VEC>
VB_KERNEL VB_LAUNCH_BOUNDS2(NT, 4) visual_loss_row_kernel(const T* scores, long ld, int n_obj, int n_attr, int n_feat,
        const int64_t* obj_label, const float* obj_conf, const int64_t* attr_label, const float* attr_conf,
        const float* feat_target, long ldt, const float* feat_conf, float g_obj, float g_attr, float g_feat,
        float* ws, T* dscores, long ldd, int M, int tvec) {
    const int lane = threadIdx.x & 63;
    const int row = vb_uniform((int)blockIdx.x * ROWS + ((int)threadIdx.x >> 6));
    if (row >= M) return;                                    // wave-uniform
    const int o1 = n_obj, o2 = n_obj + n_attr, o3 = o2 + n_feat;
    const int64_t lo = n_obj > 0 ? obj_label[row] : (int64_t)-1;
    const int64_t la = n_attr > 0 ? attr_label[row] : (int64_t)-1;
    const float co = n_obj > 0 ? obj_conf[row] : 0.f;
    const float ca = n_attr > 0 ? attr_conf[row] : 0.f;
    const float cf = n_feat > 0 ? feat_conf[row] : 0.f;
    const bool on_o = lo >= 0 && lo < n_obj && co != 0.f;
    const bool on_a = la >= 0 && la < n_attr && ca != 0.f;
    const bool on_f = n_feat > 0 && cf != 0.f;
    T* drow = dscores ? dscores + (long)row * ldd : nullptr;
    if (!(on_o || on_a || on_f)) {                           // wave-uniform: the scores of this row are never read
        if (lane == 0) { ws[row] = 0.f; ws[(long)M + row] = 0.f; ws[2 * (long)M + row] = 0.f; }
        if (drow) zero_row<T, VEC>(drow, 0, ldd, lane);
        return;
    }
    const T* x = scores + (long)row * ld;
    float v[IT][8];
#pragma unroll
    for (int k = 0; k < IT; ++k) {
        const int j = (k * 64 + lane) * 8;
        // does [j, j + 8) touch a segment whose weight is not zero?
        const bool need = (on_o && j < o1) || (on_a && j + 8 > o1 && j < o2) || (on_f && j + 8 > o2 && j < o3);
        if (VEC) {
            if (need) load8(v[k], x + j);                    // j < o3 <= ld and ld % 8 == 0: the vector ends inside the row
            else {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[k][e] = 0.f;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[k][e] = (need && j + e < o3) ? to_f32(x[j + e]) : 0.f;
        }
    }
    if (on_f) {                                              // feature columns become e = prediction - target
        const float* trow = feat_target + (long)row * ldt;
#pragma unroll
        for (int k = 0; k < IT; ++k) {
            const int j = (k * 64 + lane) * 8;
            if (j + 8 <= o2 || j >= o3) continue;
            if (tvec && j >= o2 && j + 8 <= o3) {
                float t[8];
                load8(t, trow + (j - o2));
#pragma unroll
                for (int e = 0; e < 8; ++e) v[k][e] -= t[e];
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int c = j + e;
                    if (c >= o2 && c < o3) v[k][e] -= trow[c - o2];
                }
            }
        }
    }
    // Almost every vector lies inside ONE segment (vec_kind 0 / 1 / 2): those take a branch that does that segment's arithmetic only --
    // and none at all when the segment's weight is zero, a wave-uniform test.  The per-element form is for the vectors that straddle a
    // boundary or the row's end.  (One chain of per-element selects for everything made the compiler evaluate both exponentials and the
    // SmoothL1 term for every element: the kernel was bound by the VALU, not by memory.)
    float mo = -INFINITY, ma = -INFINITY;
#pragma unroll
    for (int k = 0; k < IT; ++k) {
        const int j = (k * 64 + lane) * 8;
        const int kind = vec_kind(j, o1, o2, o3);
        if (kind == 0) {
            if (on_o) {
#pragma unroll
                for (int e = 0; e < 8; ++e) mo = fmaxf(mo, v[k][e]);
            }
        } else if (kind == 1) {
            if (on_a) {
#pragma unroll
                for (int e = 0; e < 8; ++e) ma = fmaxf(ma, v[k][e]);
            }
        } else if (kind == 3) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int c = j + e;
                if (c < o1) mo = fmaxf(mo, v[k][e]);
                else if (c < o2) ma = fmaxf(ma, v[k][e]);
            }
        }
    }
    mo = wave_max(mo);
    ma = wave_max(ma);
    float so = 0.f, sa = 0.f, xo = 0.f, xa = 0.f, sf = 0.f;
#pragma unroll
    for (int k = 0; k < IT; ++k) {
        const int j = (k * 64 + lane) * 8;
        const int kind = vec_kind(j, o1, o2, o3);
        if (kind == 0) {
            if (on_o) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    so += exp_1ulp(v[k][e] - mo);
                    if (j + e == lo) xo = v[k][e];           // the label's logit comes from the registers too (dscores may alias)
                }
            }
        } else if (kind == 1) {
            if (on_a) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    sa += exp_1ulp(v[k][e] - ma);
                    if (j + e - o1 == la) xa = v[k][e];
                }
            }
        } else if (kind == 2) {
            if (on_f) {
#pragma unroll
                for (int e = 0; e < 8; ++e) sf += smooth_l1(v[k][e]);
            }
        } else if (kind == 3) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int c = j + e;
                const float xv = v[k][e];
                if (c < o1) {
                    if (on_o) { so += exp_1ulp(xv - mo); if (c == lo) xo = xv; }
                } else if (c < o2) {
                    if (on_a) { sa += exp_1ulp(xv - ma); if (c - o1 == la) xa = xv; }
                } else if (c < o3) {
                    if (on_f) sf += smooth_l1(xv);
                }
            }
        }
    }
    so = wave_sum(so); sa = wave_sum(sa); xo = wave_sum(xo); xa = wave_sum(xa); sf = wave_sum(sf);
    const float lse_o = mo + logf(so), lse_a = ma + logf(sa);       // of a segment whose weight is zero: never used
    if (lane == 0) {
        ws[row] = on_o ? co * (lse_o - xo) : 0.f;
        ws[(long)M + row] = on_a ? ca * (lse_a - xa) : 0.f;
        ws[2 * (long)M + row] = on_f ? cf * (sf / (float)n_feat) : 0.f;
    }
    if (!drow) return;
    const float go = g_obj * co, ga = g_attr * ca, gf = g_feat * cf;
#pragma unroll
    for (int k = 0; k < IT; ++k) {
        const int j = (k * 64 + lane) * 8;
        const int kind = vec_kind(j, o1, o2, o3);
        float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (kind == 0) {
            if (on_o) {
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = (exp_1ulp(v[k][e] - lse_o) - (j + e == lo ? 1.f : 0.f)) * go;
            }
        } else if (kind == 1) {
            if (on_a) {
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = (exp_1ulp(v[k][e] - lse_a) - (j + e - o1 == la ? 1.f : 0.f)) * ga;
            }
        } else if (kind == 2) {
            if (on_f) {
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = fminf(fmaxf(v[k][e], -1.f), 1.f) * gf;
            }
        } else if (kind == 3) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int c = j + e;
                const float xv = v[k][e];
                if (c < o1) { if (on_o) o[e] = (exp_1ulp(xv - lse_o) - (c == lo ? 1.f : 0.f)) * go; }
                else if (c < o2) { if (on_a) o[e] = (exp_1ulp(xv - lse_a) - (c - o1 == la ? 1.f : 0.f)) * ga; }
                else if (c < o3) { if (on_f) o[e] = fminf(fmaxf(xv, -1.f), 1.f) * gf; }
            }
        }
        if (VEC) {
            if (j < ldd) store8(drow + j, o);                // ldd % 8 == 0: pad columns up to ldd are written as zeros
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (j + e < ldd) drow[j + e] = from_f32<T>(o[e]);
        }
    }
    if (ldd > MAXW) zero_row<T, VEC>(drow, MAXW, ldd, lane);
}

// losses[k] = w_k * (sum_r ws[k][r]) / M in a fixed order: thread t adds rows t, t + 1024, ... ascending, the 64 lanes of a wave
// combine by the same butterfly every time, thread 0 adds the 16 wave sums in order.  The sums run in fp64 (a few thousand adds in
// all): the M fp32 row terms are then rounded once, at the end.  losses[3] = obj + attr + feat.
VB_DEVICE double wave_sum_f64(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
VB_KERNEL VB_LAUNCH_BOUNDS(FIN_NT) visual_loss_finish_kernel(const float* ws, int M, float w_obj, float w_attr, float w_feat,
                                                            float* losses) {
    VB_DYN_SMEM(smem);
    double* red = (double*)smem;                             // [3][FIN_NT / 64]
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int r = threadIdx.x; r < M; r += FIN_NT) {
        a0 += (double)ws[r];
        a1 += (double)ws[(long)M + r];
        a2 += (double)ws[2 * (long)M + r];
    }
    a0 = wave_sum_f64(a0); a1 = wave_sum_f64(a1); a2 = wave_sum_f64(a2);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int NW = FIN_NT / 64;
    if (lane == 0) { red[wave] = a0; red[NW + wave] = a1; red[2 * NW + wave] = a2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (int w = 0; w < NW; ++w) { s0 += red[w]; s1 += red[NW + w]; s2 += red[2 * NW + w]; }
        const double l0 = (s0 / (double)M) * (double)w_obj, l1 = (s1 / (double)M) * (double)w_attr, l2 = (s2 / (double)M) * (double)w_feat;
        losses[0] = (float)l0; losses[1] = (float)l1; losses[2] = (float)l2;
        losses[3] = (float)((l0 + l1) + l2);
    }
}

template <typename T>
int launch_rows(const void* scores, int64_t ld, int n_obj, int n_attr, int n_feat, const int64_t* obj_label,
                const float* obj_conf, const int64_t* attr_label, const float* attr_conf, const float* feat_target,
                int64_t ldt, const float* feat_conf, float g_obj, float g_attr, float g_feat, float* ws, void* dscores,
                int64_t ldd, int M, hipStream_t s) {
    const bool vec = (ld & 7) == 0 && (!dscores || (ldd & 7) == 0) && ((((uintptr_t)scores) | ((uintptr_t)dscores)) & 15) == 0;
    const int tvec = n_feat > 0 && ((n_obj + n_attr) & 3) == 0 && (ldt & 3) == 0 && (((uintptr_t)feat_target) & 15) == 0;
    const dim3 grid((unsigned)((M + ROWS - 1) / ROWS));
    if (vec)
        VB_LAUNCH((visual_loss_row_kernel<T, true>), grid, dim3(NT), 0, s, (const T*)scores, (long)ld, n_obj, n_attr, n_feat,
                  obj_label, obj_conf, attr_label, attr_conf, feat_target, (long)ldt, feat_conf, g_obj, g_attr, g_feat, ws,
                  (T*)dscores, (long)ldd, M, tvec);
    else
        VB_LAUNCH((visual_loss_row_kernel<T, false>), grid, dim3(NT), 0, s, (const T*)scores, (long)ld, n_obj, n_attr, n_feat,
                  obj_label, obj_conf, attr_label, attr_conf, feat_target, (long)ldt, feat_conf, g_obj, g_attr, g_feat, ws,
                  (T*)dscores, (long)ldd, M, tvec);
    return VB_OK;
}

}  // namespace

extern "C" int64_t vb_visual_loss_ws_floats(int M) {
    return M > 0 ? 3 * (int64_t)M : -1;
}

extern "C" int vb_visual_loss_fwd_bwd(int dtype, const void* scores, int64_t ld_scores, int n_obj, int n_attr, int n_feat,
        const int64_t* obj_label, const float* obj_conf, const int64_t* attr_label, const float* attr_conf,
        const float* feat_target, int64_t ld_target, const float* feat_conf,
        float w_obj, float w_attr, float w_feat, float* ws, float* losses, void* dscores, int64_t ld_dscores, int M,
        void* stream) {
    if (!scores || !ws || !losses || M <= 0 || n_obj < 0 || n_attr < 0 || n_feat < 0) return VB_ERR_ARG;
    const int64_t width = (int64_t)n_obj + n_attr + n_feat;
    if (width <= 0 || ld_scores < width || (dscores && ld_dscores < width)) return VB_ERR_ARG;
    if ((n_obj > 0 && (!obj_label || !obj_conf)) || (n_attr > 0 && (!attr_label || !attr_conf))) return VB_ERR_ARG;
    if (n_feat > 0 && (!feat_target || !feat_conf || ld_target < n_feat)) return VB_ERR_ARG;
    if (width > MAXW) return VB_ERR_UNSUPPORTED;             // a row lives in one wave's registers
    hipStream_t s = (hipStream_t)stream;
    const float g_obj = w_obj / (float)M, g_attr = w_attr / (float)M;
    const float g_feat = n_feat > 0 ? w_feat / ((float)M * (float)n_feat) : 0.f;
    if (dtype == VB_BF16)
        launch_rows<bf16>(scores, ld_scores, n_obj, n_attr, n_feat, obj_label, obj_conf, attr_label, attr_conf, feat_target,
                          ld_target, feat_conf, g_obj, g_attr, g_feat, ws, dscores, ld_dscores, M, s);
    else if (dtype == VB_F32)
        launch_rows<float>(scores, ld_scores, n_obj, n_attr, n_feat, obj_label, obj_conf, attr_label, attr_conf, feat_target,
                           ld_target, feat_conf, g_obj, g_attr, g_feat, ws, dscores, ld_dscores, M, s);
    else return VB_ERR_ARG;
    VB_LAUNCH(visual_loss_finish_kernel, dim3(1), dim3(FIN_NT), 3 * (FIN_NT / 64) * sizeof(double), s, (const float*)ws, M,
              w_obj, w_attr, w_feat, losses);
    return vb_check_launch();
}
