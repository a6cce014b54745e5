// answer_head.hip -- the two kernels the sibling LXRT model's answer head needs and nothing else in the library offers.
//   reference: BertVisualAnswerHead, unsupervised_visualbert/src/lxrt/modeling.py:956-969
//                Linear(H, 2H) -> GeLU -> BertLayerNorm(2H) -> Linear(2H, num_answers)
//              the VQA / GQA fine-tuning loss on the same head, src/tasks/vqa.py:72, :106-107 (BCEWithLogitsLoss x num_answers
//              on soft targets) and the accuracy :114-117 derives from the argmax
//
//   * GELU + LayerNorm over WIDE rows (8 <= H <= 8192), forward and backward.  layernorm.hip is built for many narrow rows (half a
//     wave per row, H <= 1024); here the rows are few -- one per sample, the pooled output -- and 1536 / 2048 wide.  One 256-thread
//     workgroup owns a row: thread t holds the 8-element chunks {t, t + 256, t + 512, t + 768} in registers (16-byte accesses),
//     sums reduce inside the wave by shuffles and across the four waves through 32 bytes of LDS.  The GELU in front of the
//     LayerNorm is applied to the registers: its output never exists in memory, in either direction -- the backward recomputes it
//     (and its derivative) from the pre-activation the forward read.
//   * BCEWithLogitsLoss(mean) x V on soft targets + its gradient + the VQA score, one workgroup per row.
//
// Reproducibility.  No float atomics.  LayerNorm backward: a workgroup walks rows blockIdx, blockIdx + grid, ... with its column sums
// of dgamma / dbeta in registers, stores them as one slab of ws, and a second launch adds the slabs of a column in a fixed order.
// BCE: every row stores its loss term and its score into ws and a single workgroup adds them as a fixed tree.  The same call gives
// the same bits every time, on any stream.
#include "vb_rt.h"
#include "../../include/visualbert_hip.h"

namespace {

constexpr int NT = 256;
constexpr int NW = NT / 64;
constexpr int KC = 4;                         // chunks of 8 columns per thread
constexpr int MAXH = KC * NT * 8;             // 8192
constexpr int BWD_MAX_WG = 256;               // workgroups (= slabs of partial column sums) of the backward
constexpr int FIN_NT = 1024;

// BERT's GELU, x * 0.5 * (1 + erf(x / sqrt 2)), with the library erf: the GEMM epilogues' 1.5e-7 polynomial (vb_rt.h fast_erf) is
// several ulp of a saturated activation, and the LayerNorm behind it multiplies that by rstd * gamma.  These kernels wait on memory.
VB_DEVICE float gelu_exact(float x) { return x * 0.5f * (1.0f + erff(x * 0.70710678118654752440f)); }
VB_DEVICE void gelu_exact_and_grad(float x, float& y, float& dy) {
    const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
    const float pdf = 0.39894228040143267794f * expf(-0.5f * x * x);
    y = x * cdf;
    dy = cdf + x * pdf;
}

// sums of a and b over the workgroup, in a fixed order (wave butterfly, then the four wave sums in order); red: 2 * NW floats of LDS.
// The leading barrier lets the caller reuse red right after the previous call's result was read.
VB_DEVICE void block_sum2(float& a, float& b, float* red) {
    a = wave_sum(a);
    b = wave_sum(b);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) { red[wave] = a; red[NW + wave] = b; }
    __syncthreads();
    a = (red[0] + red[1]) + (red[2] + red[3]);
    b = (red[NW] + red[NW + 1]) + (red[NW + 2] + red[NW + 3]);
}

// One workgroup per row.  nc = H / 8 chunks; chunk c = t + 256 k of thread t covers columns [8 c, 8 c + 8).
template <typename T>
VB_KERNEL VB_LAUNCH_BOUNDS(NT) ln_wide_fwd_kernel(const T* x, int act, T* y, float* mean, float* rstd, const float* gamma,
                                                 const float* beta, int H, float eps) {
    VB_DYN_SMEM(smem);
    float* red = (float*)smem;
    const int row = blockIdx.x, nc = H >> 3, t = threadIdx.x;
    const T* xr = x + (long)row * H;
    float v[KC][8];
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const int c = t + k * NT;
        if (c < nc) load8(v[k], xr + c * 8);
        else {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[k][e] = 0.f;
        }
    }
    float s = 0.f, unused = 0.f;
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        if (t + k * NT < nc) {
            if (act) {
#pragma unroll
                for (int e = 0; e < 8; ++e) v[k][e] = gelu_exact(v[k][e]);
            }
            s += ((v[k][0] + v[k][1]) + (v[k][2] + v[k][3])) + ((v[k][4] + v[k][5]) + (v[k][6] + v[k][7]));
        }
    }
    block_sum2(s, unused, red);
    const float mu = s / (float)H;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        if (t + k * NT < nc) {
            float d[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) { d[e] = v[k][e] - mu; d[e] *= d[e]; }
            q += ((d[0] + d[1]) + (d[2] + d[3])) + ((d[4] + d[5]) + (d[6] + d[7]));
        }
    }
    block_sum2(q, unused, red);
    const float rs = 1.0f / sqrtf(q / (float)H + eps);
    if (t == 0) { mean[row] = mu; rstd[row] = rs; }
    T* yr = y + (long)row * H;
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const int c = t + k * NT;
        if (c < nc) {
            float g[8], b[8], o[8];
            load8(g, gamma + c * 8);
            load8(b, beta + c * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = g[e] * ((v[k][e] - mu) * rs) + b[e];
            store8(yr + c * 8, o);
        }
    }
}

// Workgroup b walks rows b, b + grid, ...; per row: g and x-hat from x, mean, rstd; the two row sums of the LayerNorm backward in ONE
// reduction; dx through the LayerNorm and (act) GELU'.  dx may alias dy: a thread reads its chunks of dy before it writes the same
// chunks of dx, and no other thread touches them.  The column sums of dy * x-hat and dy stay in registers across the rows and leave
// as slab b of ws ([grid][2][H]); every workgroup has at least one row (grid <= M), so every slab is written whatever ws held.
template <typename T>
VB_KERNEL VB_LAUNCH_BOUNDS(NT) ln_wide_bwd_kernel(const T* dy, const T* x, int act, const float* mean, const float* rstd,
                                                 const float* gamma, T* dx, float* ws, int M, int H) {
    VB_DYN_SMEM(smem);
    float* red = (float*)smem;
    const int nc = H >> 3, t = threadIdx.x;
    float gm[KC][8], ag[KC][8], ab[KC][8];
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const int c = t + k * NT;
        if (c < nc) load8(gm[k], gamma + c * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (c >= nc) gm[k][e] = 0.f;
            ag[k][e] = 0.f;
            ab[k][e] = 0.f;
        }
    }
    for (int row = blockIdx.x; row < M; row += gridDim.x) {
        const float mu = mean[row], rs = rstd[row];
        const T* xr = x + (long)row * H;
        const T* dr = dy + (long)row * H;
        float d[KC][8], xh[KC][8], gp[KC][8];
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            const int c = t + k * NT;
            if (c < nc) { load8(xh[k], xr + c * 8); load8(d[k], dr + c * 8); }
            else {
#pragma unroll
                for (int e = 0; e < 8; ++e) { xh[k][e] = 0.f; d[k][e] = 0.f; }
            }
        }
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            if (t + k * NT < nc) {
                float p1[8], p2[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float g = xh[k][e];
                    gp[k][e] = 1.f;
                    if (act) gelu_exact_and_grad(xh[k][e], g, gp[k][e]);
                    xh[k][e] = (g - mu) * rs;
                    ag[k][e] += d[k][e] * xh[k][e];
                    ab[k][e] += d[k][e];
                    d[k][e] *= gm[k][e];                       // from here on dy * gamma
                    p1[e] = d[k][e];
                    p2[e] = d[k][e] * xh[k][e];
                }
                s1 += ((p1[0] + p1[1]) + (p1[2] + p1[3])) + ((p1[4] + p1[5]) + (p1[6] + p1[7]));
                s2 += ((p2[0] + p2[1]) + (p2[2] + p2[3])) + ((p2[4] + p2[5]) + (p2[6] + p2[7]));
            }
        }
        block_sum2(s1, s2, red);
        const float c1 = s1 / (float)H, c2 = s2 / (float)H;
        T* or_ = dx + (long)row * H;
#pragma unroll
        for (int k = 0; k < KC; ++k) {
            const int c = t + k * NT;
            if (c < nc) {
                float o[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] = (rs * ((d[k][e] - c1) - xh[k][e] * c2)) * gp[k][e];
                store8(or_ + c * 8, o);
            }
        }
    }
    if (!ws) return;                                            // neither dgamma nor dbeta is wanted
    float* slab = ws + (long)blockIdx.x * 2 * H;
#pragma unroll
    for (int k = 0; k < KC; ++k) {
        const int c = t + k * NT;
        if (c < nc) { store8(slab + c * 8, ag[k]); store8(slab + H + c * 8, ab[k]); }
    }
}

// dst[c] += sum over the slabs p < n of ws[p][which][c]: eight running sums over p = 8 i + j, joined as a tree -- the same order every
// time.  blockIdx.y: 0 = dgamma, 1 = dbeta.
VB_KERNEL VB_LAUNCH_BOUNDS(NT) ln_wide_colsum_kernel(const float* ws, int n, int H, float* dgamma, float* dbeta) {
    float* dst = blockIdx.y == 0 ? dgamma : dbeta;
    const int c = blockIdx.x * NT + threadIdx.x;
    if (!dst || c >= H) return;
    const float* src = ws + (long)blockIdx.y * H + c;
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int p = 0;
    for (; p + 8 <= n; p += 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] += src[(long)(p + j) * 2 * H];
    }
    for (int j = 0; p + j < n; ++j) a[j] += src[(long)(p + j) * 2 * H];
    dst[c] += ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
}

// ---- BCEWithLogitsLoss x V ----------------------------------------------------------------------------------------------------
// 8 values of a row from column j; n of them (0 .. 8) lie inside the row, the others read as 0.  vec: the row pitch is a multiple of 8
// floats and the base 16-byte aligned, so a vector that starts inside the row ends inside the pitch.
VB_DEVICE void load_row8(float (&v)[8], const float* row, long j, int n, bool vec) {
    if (vec) {
        load8(v, row + j);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = e < n ? v[e] : 0.f;
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = e < n ? row[j + e] : 0.f;
    }
}

// (value, index) with the larger value, the lower index on ties
VB_DEVICE void argmax_join(float& bv, int& bi, float ov, int oi) {
    if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
}

// One workgroup per row: l_r = sum_v max(x, 0) - x t + log1p(exp(-|x|)) -> ws[row]; target[row, argmax_v x] -> ws[M + row];
// dlogits = (sigmoid(x) - t) / M with zeros in the pad columns up to ldd.  exp(-|x|) never overflows, and the sigmoid is formed from
// the same exponential: 1 / (1 + e) for x >= 0, e / (1 + e) below.
VB_KERNEL VB_LAUNCH_BOUNDS(NT) bce_row_kernel(const float* logits, long ld, const float* target, long ldt, float* ws,
                                             float* dlogits, long ldd, int M, int V, int vec_x, int vec_t, int vec_d) {
    VB_DYN_SMEM(smem);
    float* red = (float*)smem;                                   // [NW] sums, [NW] maxima, [NW] indices
    const int row = blockIdx.x, t = threadIdx.x;
    const float* xr = logits + (long)row * ld;
    const float* tr = target + (long)row * ldt;
    float* dr = dlogits ? dlogits + (long)row * ldd : nullptr;
    const long span = (dr && ldd > V) ? ldd : (long)V;
    const float fM = (float)M;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float bv = -INFINITY;
    int bi = V;
    for (long j = (long)t * 8; j < span; j += NT * 8) {
        const int n = j >= V ? 0 : (V - j >= 8 ? 8 : (int)(V - j));          // columns of this vector inside the row
        float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (n > 0) {
            float xv[8], tv[8];
            load_row8(xv, xr, j, n, vec_x != 0);
            load_row8(tv, tr, j, n, vec_t != 0);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (e < n) {
                    const float xe = xv[e], e1 = expf(-fabsf(xe));
                    acc[e] += (fmaxf(xe, 0.f) - xe * tv[e]) + log1pf(e1);
                    const float sg = (xe >= 0.f ? 1.0f : e1) / (1.0f + e1);
                    o[e] = (sg - tv[e]) / fM;
                    if (xe > bv) { bv = xe; bi = (int)j + e; }  // ascending columns: the first maximum stays
                }
            }
        }
        if (dr) {
            if (vec_d) store8(dr + j, o);                        // j < ldd and ldd % 8 == 0
            else {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (j + e < ldd) dr[j + e] = o[e];
            }
        }
    }
    float s = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    s = wave_sum(s);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ov = __shfl_xor(bv, m);
        const int oi = __shfl_xor(bi, m);
        argmax_join(bv, bi, ov, oi);
    }
    const int lane = t & 63, wave = t >> 6;
    if (lane == 0) { red[wave] = s; red[NW + wave] = bv; ((int*)red)[2 * NW + wave] = bi; }
    __syncthreads();
    if (t == 0) {
        ws[row] = (red[0] + red[1]) + (red[2] + red[3]);
        for (int w = 1; w < NW; ++w) argmax_join(bv, bi, red[NW + w], ((const int*)red)[2 * NW + w]);
        ws[(long)M + row] = (bi >= 0 && bi < V) ? tr[bi] : 0.f;
    }
}

VB_DEVICE double wave_sum_f64(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
// loss[0] = (sum_r ws[r]) / M, score[0] = (sum_r ws[M + r]) / M as a fixed tree: thread t adds rows t, t + 1024, ... ascending, the
// lanes of a wave join by the same butterfly every time, the sixteen wave sums pairwise.  The tree runs in fp64 (M adds in all), so the
// fp32 row terms are rounded once more, at the end.
VB_KERNEL VB_LAUNCH_BOUNDS(FIN_NT) bce_finish_kernel(const float* ws, int M, float* loss, float* score) {
    VB_DYN_SMEM(smem);
    double* red = (double*)smem;                                 // [2][FIN_NT / 64]
    constexpr int FW = FIN_NT / 64;
    double a = 0.0, b = 0.0;
    for (int r = threadIdx.x; r < M; r += FIN_NT) {
        a += (double)ws[r];
        b += (double)ws[(long)M + r];
    }
    a = wave_sum_f64(a);
    b = wave_sum_f64(b);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[wave] = a; red[FW + wave] = b; }
    __syncthreads();
    if (threadIdx.x < 2) {
        double* r = red + threadIdx.x * FW;
        for (int w = FW / 2; w >= 1; w >>= 1)
            for (int i = 0; i < w; ++i) r[i] += r[i + w];
        float* out = threadIdx.x == 0 ? loss : score;
        if (out) out[0] = (float)(r[0] / (double)M);
    }
}

int ln_wide_bwd_grid(int M) { return M < BWD_MAX_WG ? M : BWD_MAX_WG; }
bool ln_wide_shape_ok(int M, int H, int act) {
    return M > 0 && H >= 8 && H <= MAXH && (H & 7) == 0 && (act == VB_ACT_NONE || act == VB_ACT_GELU);
}

}  // namespace

extern "C" int vb_ln_wide_fwd(int dtype, const void* x, int act, void* y, float* mean, float* rstd, const float* gamma,
                              const float* beta, int M, int H, float eps, void* stream) {
    if (!x || !y || !mean || !rstd || !gamma || !beta || !ln_wide_shape_ok(M, H, act)) return VB_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = 2 * NW * sizeof(float);
    if (dtype == VB_BF16)
        VB_LAUNCH(ln_wide_fwd_kernel<bf16>, dim3((unsigned)M), dim3(NT), lds, s, (const bf16*)x, act, (bf16*)y, mean, rstd, gamma,
                  beta, H, eps);
    else if (dtype == VB_F32)
        VB_LAUNCH(ln_wide_fwd_kernel<float>, dim3((unsigned)M), dim3(NT), lds, s, (const float*)x, act, (float*)y, mean, rstd,
                  gamma, beta, H, eps);
    else return VB_ERR_ARG;
    return vb_check_launch();
}

extern "C" int64_t vb_ln_wide_bwd_ws_floats(int M, int H) {
    return ln_wide_shape_ok(M, H, VB_ACT_NONE) ? 2 * (int64_t)ln_wide_bwd_grid(M) * H : -1;
}

extern "C" int vb_ln_wide_bwd(int dtype, const void* dy, const void* x, int act, const float* mean, const float* rstd,
                              const float* gamma, void* dx, float* dgamma, float* dbeta, float* ws, int M, int H, void* stream) {
    if (!dy || !x || !mean || !rstd || !gamma || !dx || !ws || !ln_wide_shape_ok(M, H, act)) return VB_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const size_t lds = 2 * NW * sizeof(float);
    const int grid = ln_wide_bwd_grid(M);
    float* slabs = (dgamma || dbeta) ? ws : nullptr;
    if (dtype == VB_BF16)
        VB_LAUNCH(ln_wide_bwd_kernel<bf16>, dim3((unsigned)grid), dim3(NT), lds, s, (const bf16*)dy, (const bf16*)x, act, mean,
                  rstd, gamma, (bf16*)dx, slabs, M, H);
    else if (dtype == VB_F32)
        VB_LAUNCH(ln_wide_bwd_kernel<float>, dim3((unsigned)grid), dim3(NT), lds, s, (const float*)dy, (const float*)x, act, mean,
                  rstd, gamma, (float*)dx, slabs, M, H);
    else return VB_ERR_ARG;
    if (slabs)
        VB_LAUNCH(ln_wide_colsum_kernel, dim3((unsigned)((H + NT - 1) / NT), 2), dim3(NT), 0, s, (const float*)ws, grid, H, dgamma,
                  dbeta);
    return vb_check_launch();
}

extern "C" int64_t vb_bce_logits_ws_floats(int M) {
    return M > 0 ? 2 * (int64_t)M : -1;
}

extern "C" int vb_bce_logits_fwd_bwd(const float* logits, int64_t ld_logits, const float* target, int64_t ld_target, float* ws,
                                     float* loss, float* score, float* dlogits, int64_t ld_dlogits, int M, int V, void* stream) {
    if (!logits || !target || !ws || !loss || M <= 0 || V <= 0) return VB_ERR_ARG;
    if (ld_logits < V || ld_target < V || (dlogits && ld_dlogits < V)) return VB_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int vec_x = (ld_logits & 7) == 0 && (((uintptr_t)logits) & 15) == 0;
    const int vec_t = (ld_target & 7) == 0 && (((uintptr_t)target) & 15) == 0;
    const int vec_d = dlogits && (ld_dlogits & 7) == 0 && (((uintptr_t)dlogits) & 15) == 0;
    VB_LAUNCH(bce_row_kernel, dim3((unsigned)M), dim3(NT), 3 * NW * sizeof(float), s, logits, (long)ld_logits, target,
              (long)ld_target, ws, dlogits, (long)ld_dlogits, M, V, vec_x, vec_t, vec_d);
    VB_LAUNCH(bce_finish_kernel, dim3(1), dim3(FIN_NT), 2 * (FIN_NT / 64) * sizeof(double), s, (const float*)ws, M, loss, score);
    return vb_check_launch();
}
