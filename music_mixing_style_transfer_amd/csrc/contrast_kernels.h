// Contrastive and gain training losses (modules/loss.py of the reference: NT_Xent :24-71, RMSLoss :77-93, infoNCE :228-238) with their
// gradients.  The reference's NT-Xent broadcasts two [N, D] operands to [N, N, D]; the arithmetic is a Gram matrix of the normalised rows, a
// row-wise log-sum-exp and, backwards, one more matrix product:
//   zh_i = z_i / max(|z_i|, eps)      S_ij = zh_i . zh_j / tau      row term = -S_i,p(i) + log sum_{j != i} exp S_ij
//   G_ij = (softmax_j(S_i.) - [j = p(i)]) dloss / N      dZh = (G + G^T) Zh / tau      dz_i = (dzh_i - zh_i (zh_i . dzh_i)) / |z_i|
// (infoNCE: S = A B^T / tau, p(i) = i, no masked diagonal, dA = G B / tau, dB = G^T A / tau).
// Both products run on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain), everything that is a sum over a row or over
// the rows is float64 in a fixed order - thread-strided partials, then a fixed tree in LDS.  No atomics anywhere: the same inputs give the
// same bits in every run.  fp32 operands only: at tau = 0.1 a bf16 Gram entry's rounding (4e-3 x 10) would move the loss in its second
// digit.  Ragged N and D are predicated (zeros enter the chains, which leaves them exact); nothing of the caller's is padded.
#pragma once
#include "mst_dev.h"

constexpr int NTX_THREADS = 256;      // every kernel of this file: four waves
constexpr int NTX_TILE = 32;          // rows of a strip / contraction steps staged at once
constexpr int NTX_COLS = 128;         // columns of a workgroup: one 32 x 32 MFMA tile per wave
constexpr int NTX_LD = NTX_TILE + 1;  // LDS row stride of the 32-wide tiles: lanes on consecutive rows hit consecutive banks
constexpr int NTX_KC = 64;            // values of D the Gram kernel stages at once (41.6 KB of LDS: two workgroups per CU)
constexpr int NTX_LDK = NTX_KC + 1;
constexpr int RMS_CHUNK = 8192;       // samples of a row one workgroup of rms_rows_kernel sums

// the sum of one double per thread over the workgroup: a fixed tree (the same bits whatever the wave scheduling)
__device__ __forceinline__ double ntx_block_sum(double v, double *red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = NTX_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ float ntx_block_max(float v, float *red) {
    const int t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (int s = NTX_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = fmaxf(red[t], red[t + s]);
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

// row r of cat(a, b): zh[r] = z / max(|z|, eps) (F.normalize / CosineSimilarity), |z|^2 summed in float64.  invn[r] is the factor the
// forward used, invn[N + r] the backward's: the same, or 0 for a row below eps (its gradient is exact zeros, not dzh / eps).
__global__ __launch_bounds__(NTX_THREADS) void ntx_normalize_kernel(const float *__restrict__ a, const float *__restrict__ b, int n_a, int N, int D,
                                                                    double eps, float *__restrict__ zh, float *__restrict__ invn) {
    __shared__ double red[NTX_THREADS];
    const int r = blockIdx.x, t = threadIdx.x;
    const float *src = r < n_a ? a + (size_t)r * D : b + (size_t)(r - n_a) * D;
    double ss = 0.0;
    for (int k = t; k < D; k += NTX_THREADS) {
        const double v = (double)src[k];
        ss += v * v;
    }
    const double norm = sqrt(ntx_block_sum(ss, red));
    const float inv = (float)(1.0 / (norm > eps ? norm : eps));
    float *dst = zh + (size_t)r * D;
    for (int k = t; k < D; k += NTX_THREADS) dst[k] = src[k] * inv;
    if (t == 0) {
        invn[r] = inv;
        invn[N + r] = norm < eps ? 0.0f : inv;
    }
}

// S[i][j] = (X_i . Y_j) inv_tau for a 32-row strip and 128 columns: X [M, D], Y [Nc, D], S [M, Nc].  The strip of X and the wave's 32 rows
// of Y pass through LDS 64 values of D at a time; each entry is one fmaf chain over D in k order.
__global__ __launch_bounds__(NTX_THREADS) void ntx_gram_kernel(const float *__restrict__ X, const float *__restrict__ Y, int M, int Nc, int D,
                                                               float inv_tau, float *__restrict__ S) {
    __shared__ float xs[NTX_TILE * NTX_LDK];
    __shared__ float ys[NTX_COLS * NTX_LDK];
    const int t = threadIdx.x, w = t >> 6, l = t & 63;
    const int i0 = blockIdx.x * NTX_TILE, j0 = blockIdx.y * NTX_COLS;
    f32x16 acc;
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int k0 = 0; k0 < D; k0 += NTX_KC) {
        for (int e = t; e < NTX_TILE * NTX_KC; e += NTX_THREADS) {
            const int r = e >> 6, kk = e & 63, gi = i0 + r, gk = k0 + kk;
            xs[r * NTX_LDK + kk] = (gi < M && gk < D) ? X[(size_t)gi * D + gk] : 0.0f;
        }
        for (int e = t; e < NTX_COLS * NTX_KC; e += NTX_THREADS) {
            const int r = e >> 6, kk = e & 63, gj = j0 + r, gk = k0 + kk;
            ys[r * NTX_LDK + kk] = (gj < Nc && gk < D) ? Y[(size_t)gj * D + gk] : 0.0f;
        }
        __syncthreads();
        const float *xa = xs + (l & 31) * NTX_LDK + (l >> 5), *yb = ys + (w * 32 + (l & 31)) * NTX_LDK + (l >> 5);
#pragma unroll
        for (int kk = 0; kk < NTX_KC; kk += 2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[kk], yb[kk], acc, 0, 0, 0);
        __syncthreads();
    }
    const int gj = j0 + w * 32 + (l & 31);
    for (int r = 0; r < 16; ++r) {
        const int gi = i0 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
        if (gi < M && gj < Nc) S[(size_t)gi * Nc + gj] = acc[r] * inv_tau;
    }
}

// Row i of S [M, Nc]: the max over the row's logits (mask_diag: every j but i), sum exp(S - max) in float64, and either the row's loss term
// -S_i,p + max + log sum (dloss null) or, in place of S, G_ij = (exp(S_ij - max) / sum - [j = p]) dloss / M with G_ii = 0 where masked.
// p = i + half (mod M).  A row whose only logit is its positive (N = 2) gives exactly 0 both ways.
__global__ __launch_bounds__(NTX_THREADS) void ntx_rows_kernel(float *__restrict__ S, int M, int Nc, int mask_diag, int half,
                                                               const double *__restrict__ dloss, double *__restrict__ rowterm) {
    __shared__ double red[NTX_THREADS];
    __shared__ float redf[NTX_THREADS];
    const int i = blockIdx.x, t = threadIdx.x;
    float *row = S + (size_t)i * Nc;
    const int skip = mask_diag ? i : -1, p = (i + half) % Nc;
    float mx = -INFINITY;
    for (int j = t; j < Nc; j += NTX_THREADS)
        if (j != skip) mx = fmaxf(mx, row[j]);
    mx = ntx_block_max(mx, redf);
    double s = 0.0;
    for (int j = t; j < Nc; j += NTX_THREADS)
        if (j != skip) s += exp((double)row[j] - (double)mx);
    const double tot = ntx_block_sum(s, red);
    if (!dloss) {
        if (t == 0) rowterm[i] = ((double)mx - (double)row[p]) + log(tot);
        return;
    }
    const double scale = dloss[0] / (double)M;
    for (int j = t; j < Nc; j += NTX_THREADS) {
        const double g = j == skip ? 0.0 : exp((double)row[j] - (double)mx) / tot - (j == p ? 1.0 : 0.0);
        row[j] = (float)(g * scale);
    }
}

// loss = (1 / M) sum of the row terms, float64 in a fixed order (one workgroup)
__global__ __launch_bounds__(NTX_THREADS) void ntx_mean_kernel(const double *__restrict__ rowterm, int M, double *__restrict__ loss) {
    __shared__ double red[NTX_THREADS];
    double s = 0.0;
    for (int i = threadIdx.x; i < M; i += NTX_THREADS) s += rowterm[i];
    s = ntx_block_sum(s, red);
    if (threadIdx.x == 0) loss[0] = s / (double)M;
}

// dZh[i][d] = inv_tau sum_j P_ij Y[j][d] for a 32-row strip and 128 columns of D, P_ij = (use_g ? G[i][j] : 0) + (use_gt ? G[j][i] : 0):
// G [., ldg], Y [K, D].  Row i goes to out_a (i < n_split) or out_b, both [., D].  The contraction runs over j in order.
__global__ __launch_bounds__(NTX_THREADS) void ntx_grad_kernel(const float *__restrict__ G, int M, int K, int ldg, int use_g, int use_gt,
                                                               const float *__restrict__ Y, int D, float inv_tau, float *__restrict__ out_a,
                                                               float *__restrict__ out_b, int n_split) {
    __shared__ float ps[NTX_TILE * NTX_LD];      // G[i0 + r][j0 + c]
    __shared__ float qs[NTX_TILE * NTX_LD];      // G[j0 + r][i0 + c]
    __shared__ float ys[NTX_TILE * NTX_COLS];
    const int t = threadIdx.x, w = t >> 6, l = t & 63;
    const int i0 = blockIdx.x * NTX_TILE, d0 = blockIdx.y * NTX_COLS;
    f32x16 acc;
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
    for (int j0 = 0; j0 < K; j0 += NTX_TILE) {
        for (int e = t; e < NTX_TILE * NTX_TILE; e += NTX_THREADS) {
            const int r = e >> 5, c = e & 31;
            ps[r * NTX_LD + c] = (use_g && i0 + r < M && j0 + c < K) ? G[(size_t)(i0 + r) * ldg + j0 + c] : 0.0f;
            qs[r * NTX_LD + c] = (use_gt && j0 + r < K && i0 + c < M) ? G[(size_t)(j0 + r) * ldg + i0 + c] : 0.0f;
        }
        for (int e = t; e < NTX_TILE * NTX_COLS; e += NTX_THREADS) {
            const int r = e >> 7, c = e & 127;
            ys[e] = (j0 + r < K && d0 + c < D) ? Y[(size_t)(j0 + r) * D + d0 + c] : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < NTX_TILE; kk += 2) {
            const int kq = kk + (l >> 5);
            const float av = ps[(l & 31) * NTX_LD + kq] + qs[kq * NTX_LD + (l & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, ys[kq * NTX_COLS + w * 32 + (l & 31)], acc, 0, 0, 0);
        }
        __syncthreads();
    }
    const int gd = d0 + w * 32 + (l & 31);
    for (int r = 0; r < 16; ++r) {
        const int gi = i0 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5);
        if (gi < M && gd < D) {
            float *dst = gi < n_split ? out_a + (size_t)gi * D : out_b + (size_t)(gi - n_split) * D;
            dst[gd] = acc[r] * inv_tau;
        }
    }
}

// through the normalisation, in place: row i holds dzh_i and leaves dz_i = (dzh_i - zh_i (zh_i . dzh_i)) invn_i, the dot product in float64
// in a fixed order; a row the forward clamped (invn_i = 0) leaves exact zeros
__global__ __launch_bounds__(NTX_THREADS) void ntx_project_kernel(float *__restrict__ out_a, float *__restrict__ out_b, int n_split,
                                                                  const float *__restrict__ zh, const float *__restrict__ invn_bw, int D) {
    __shared__ double red[NTX_THREADS];
    const int i = blockIdx.x, t = threadIdx.x;
    float *g = i < n_split ? out_a + (size_t)i * D : out_b + (size_t)(i - n_split) * D;
    const float *z = zh + (size_t)i * D;
    double s = 0.0;
    for (int k = t; k < D; k += NTX_THREADS) s += (double)z[k] * (double)g[k];
    const double dot = ntx_block_sum(s, red), inv = (double)invn_bw[i];
    for (int k = t; k < D; k += NTX_THREADS) g[k] = inv == 0.0 ? 0.0f : (float)(((double)g[k] - (double)z[k] * dot) * inv);
}

// ---- RMSLoss --------------------------------------------------------------------------------------------------------------------------
// partial[(which rows + row) nchunks + chunk] = the float64 sum of squares of samples chunk RMS_CHUNK .. of row `row` of est (which = 0) or
// tgt (1), both [rows, T]: thread-strided partials, then the fixed tree
__global__ __launch_bounds__(NTX_THREADS) void rms_rows_kernel(const float *__restrict__ est, const float *__restrict__ tgt, long T, int nchunks,
                                                               double *__restrict__ partial) {
    __shared__ double red[NTX_THREADS];
    const int chunk = blockIdx.x, row = blockIdx.y, which = blockIdx.z, rows = gridDim.y;
    const float *src = (which ? tgt : est) + (size_t)row * T;
    const long lo = (long)chunk * RMS_CHUNK, hi = lo + RMS_CHUNK < T ? lo + RMS_CHUNK : T;
    double s = 0.0;
    for (long j = lo + threadIdx.x; j < hi; j += NTX_THREADS) {
        const double v = (double)src[j];
        s += v * v;
    }
    s = ntx_block_sum(s, red);
    if (threadIdx.x == 0) partial[((size_t)which * rows + row) * nchunks + chunk] = s;
}

// One workgroup: per row r the two rms values, w_r = wf max(|rms_t - rms_e|, 1 / wf) and d_r = rms_e - rms_t;
// loss = mean(w^1.5) mean(d^2) (nn.MSELoss(reduce=None) is the mean reduction).  With dloss: coef[r] = dloss d loss / d rms_e,r / (T rms_e,r),
// the factor of est[r, t] in the gradient - 0 for a row without energy, and the clamp's side |d| < 1 / wf passes no gradient through w.
__global__ __launch_bounds__(NTX_THREADS) void rms_finish_kernel(const double *__restrict__ partial, int rows, int nchunks, long T, double wf,
                                                                 const double *__restrict__ dloss, double *__restrict__ loss,
                                                                 double *__restrict__ coef, double *__restrict__ rms) {
    __shared__ double red[NTX_THREADS];
    const int t = threadIdx.x;
    double sw = 0.0, sd = 0.0;
    for (int r = t; r < rows; r += NTX_THREADS) {
        double se = 0.0, st = 0.0;
        for (int c = 0; c < nchunks; ++c) {
            se += partial[(size_t)r * nchunks + c];
            st += partial[((size_t)rows + r) * nchunks + c];
        }
        const double re = sqrt(se / (double)T), rt = sqrt(st / (double)T), d = re - rt;
        const double a = fabs(rt - re), w = (a > 1.0 / wf ? a : 1.0 / wf) * wf;
        rms[r] = re;
        rms[rows + r] = rt;
        sw += w * sqrt(w);
        sd += d * d;
    }
    const double W = ntx_block_sum(sw, red) / (double)rows, Q = ntx_block_sum(sd, red) / (double)rows;
    if (!dloss) {
        if (t == 0) loss[0] = W * Q;
        return;
    }
    const double up = dloss[0] / (double)rows;
    for (int r = t; r < rows; r += NTX_THREADS) {
        const double re = rms[r], rt = rms[rows + r], d = re - rt, a = fabs(rt - re);
        const double w = (a > 1.0 / wf ? a : 1.0 / wf) * wf;
        const double dw = a >= 1.0 / wf ? (d > 0.0 ? wf : (d < 0.0 ? -wf : 0.0)) : 0.0;
        coef[r] = re > 0.0 ? up * (1.5 * sqrt(w) * dw * Q + W * 2.0 * d) / ((double)T * re) : 0.0;
    }
}

// grad[r, t] = coef[r] est[r, t], the product in float64, rounded once
__global__ __launch_bounds__(NTX_THREADS) void rms_grad_kernel(const float *__restrict__ est, const double *__restrict__ coef, long T,
                                                               float *__restrict__ grad) {
    const int row = blockIdx.y;
    const double c = coef[row];
    const long lo = (long)blockIdx.x * RMS_CHUNK, hi = lo + RMS_CHUNK < T ? lo + RMS_CHUNK : T;
    const float *src = est + (size_t)row * T;
    float *dst = grad + (size_t)row * T;
    for (long j = lo + threadIdx.x; j < hi; j += NTX_THREADS) dst[j] = c == 0.0 ? 0.0f : (float)(c * (double)src[j]);
}
