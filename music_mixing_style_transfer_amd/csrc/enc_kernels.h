// gfx950 kernels of the FXencoder (reference networks/architectures.py:26-70; one Conv1d_layer =
// ReflectionPad1d -> Conv1d(stride) -> BatchNorm1d(eval) -> ReLU, networks/network_utils.py:28-34,47-51,74-83;
// Res_ConvBlock = conv2(conv1(x) + x), network_utils.py:116-119).
//
// One generic implicit-GEMM convolution in exact fp32 on the matrix cores (v_mfma_f32_32x32x2_f32):
//     D[co][n] = sum_k W'[co][k] * X[k][n],   k = ci*ksz + j,  n = b*Lout + to,
//     X[k][n] = x[b][ci][reflect(to*stride + j*dil - pad_l)]
// Layout: activations NCL fp32 (time contiguous) like the reference, so the MFMA B fragment (32 consecutive
// output times per half-wave) and the epilogue stores (32 consecutive times per accumulator register)
// are both coalesced.  BatchNorm is folded into W' and a per-channel shift on the host; weights are
// pre-packed per (co-tile, k-chunk) in the exact [16][MT] image the LDS wants, so staging A is a straight
// 16-byte copy.  The im2col gather (reflection + stride) happens while staging B; the (ci, tap offset) of
// every k comes from a small per-layer table instead of integer divisions.
// Workgroup = 4 waves; wave = 32 output channels x 128 columns (4 accumulator tiles).  MW waves along
// channels: tile = (32*MW) x (128 * 4/MW); MW is picked from Cout (1 for <=32, 2 for 64, 4 otherwise).
#pragma once
#include "mst_dev.h"

// the encoder's activation (Conv1d_layer, network_utils.py:76-80): ReLU (slope 0), LeakyReLU(0.01) or none (slope 1): v > 0 ? v : slope * v,
// with torch's results for non-finite values too - ReLU(-inf) = 0 (slope * v would be 0 * -inf = NaN), NaN propagates in every mode
__device__ __forceinline__ float enc_act(float v, float slope) {
    const float neg = slope == 0.0f ? (v != v ? v : 0.0f) : v * slope;
    return v > 0.0f ? v : neg;
}

struct EncConvArgs {
    const float *x;      // [B][Cin][Lin]
    float *y;            // [B][Cout][Lout]
    const float *wpk;    // [co_tiles][nchunks][16][MT]
    const float *shift;  // [co_tiles*MT] folded bias/BN shift (zero padded)
    const int *ktab;     // [nchunks32*32][2]: (ci, j*dil - pad_l), ci = -1 for the zero padding of K
    const void *wpk16;   // bf16 A fragments [co_tiles][nchunks32][2][MW][64][8]
    int nchunks32;       // ceil(K / 32)
    int B, Cin, Lin, Cout, Lout, stride;
    int nchunks;
    int residual;        // conv1 of a Res block: add x[b][co][to] after the ReLU
    long Ntot;           // B * Lout
    // generic-TCN use of the same kernel (fp32 only): zero instead of reflection padding and other epilogues
    int pad_zero;        // 1: taps outside [0, Lin) read 0 (TCNBlock conv1 padding), 0: reflection (encoder)
    int epi;             // 0: ReLU (+ same-channel skip); 1: TCN block LeakyReLU -> FiLM -> + grouped 1x1 residual; 2: clamp(-1, 1)
    const float *film;   // epi 1: [film_rows][2*Cout]  (r | b)
    const float *res;    // epi 1: [Cout] grouped 1x1 residual scale; out-channel co reads in-channel co / res_div
    int film_rows, res_div;
    // split-K (gridDim.z = S > 1, fp32 kernel): slice z contracts k-chunks [z * nchunks / S, (z + 1) * nchunks / S) and stores its
    // raw partial sums to part[z][co][n]; enc_splitk_finalize_ncl_kernel adds the slices in order and applies the epilogue.
    // Used for the short wide late layers, whose 128 tiles would otherwise leave half of the 256 CUs idle.
    float *part = nullptr;
    float slope = 0.0f;  // epi 0: activation slope for negative values (enc_act)
    int buf32 = 0;       // enc_conv_kernel: the tile's activations are reachable with 32-bit byte offsets (host-checked): buffer-load gathers
};

template <int MW>
__global__ __launch_bounds__(256) void enc_conv_kernel(EncConvArgs a) {
    constexpr int NW = 4 / MW, MT = 32 * MW, NT = 128 * NW;
    constexpr int NB = NT / 16;                       // B elements gathered per thread per chunk
    constexpr int NA = (16 * MT / 4 + 255) / 256;     // A float4 per thread per chunk
    __shared__ __attribute__((aligned(16))) float As[16 * MT];
    __shared__ float Bs[16 * NT];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int ln = lane & 31, h = lane >> 5;
    const int mi = w % MW, ni = w / MW;
    const long n0 = (long)blockIdx.x * NT;
    const int cot = blockIdx.y;

    // the <= 2 columns this thread gathers for (fixed for the whole K loop).  The gathers are raw buffer loads (round 3): a 32-bit byte
    // offset per lane on a descriptor that starts at the tile's first batch item; rows of K beyond the problem, columns beyond Ntot and
    // (zero-padding mode) taps outside the signal use an offset beyond the descriptor, which reads as 0 - no predicated load (hipcc
    // branches around one and drains vmcnt(0) behind it: the loads of chunk k + 1 then never overlapped the MFMAs of chunk k), and the
    // k-table entries are fetched a chunk ahead of the gathers that need them.
    constexpr int NCOL = (NT + 255) / 256;
    const int item0 = (int)(n0 / a.Lout);
    const size_t item_elems = (size_t)a.Cin * a.Lin, left = ((size_t)a.B - item0) * item_elems * 4;
    const MstStream16 xs = mst_stream16(a.x + (size_t)item0 * item_elems, left < 0x7fffffffu ? (unsigned)left : 0x7fffffffu);
    int colbase[NCOL];                                // element offset of the column's batch item in the descriptor, -1: no column
    int colt[NCOL];
#pragma unroll
    for (int c = 0; c < NCOL; ++c) {
        const long n = n0 + (tid + c * 256) % NT;
        if (n < a.Ntot) {
            const int b = (int)(n / a.Lout), to = (int)(n % a.Lout);
            colbase[c] = (int)((b - item0) * (long)item_elems);
            colt[c] = to * a.stride;
        } else {
            colbase[c] = -1;
            colt[c] = 0;
        }
    }

    f32x16 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[q][i] = 0.0f;

    f32x4 areg[NA];
    float breg[NB];
    const f32x4 *wtile = (const f32x4 *)(a.wpk + (size_t)cot * a.nchunks * 16 * MT);
    const int kc_lo = (int)((long)blockIdx.z * a.nchunks / gridDim.z), kc_hi = (int)((long)(blockIdx.z + 1) * a.nchunks / gridDim.z);

    u32x2 kt[NB];                                     // k-table entries (ci, tap offset) of the chunk the next fetch() gathers
    auto ktab_entries = [&](int kc) {
        const int k2 = kc < kc_hi ? kc : kc_hi - 1;
#pragma unroll
        for (int e = 0; e < NB; ++e) kt[e] = *(const u32x2 *)(a.ktab + (k2 * 16 + (tid + e * 256) / NT) * 2);
    };
    auto fetch = [&](int kc) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int idx = tid + i * 256;
            if (idx < 16 * MT / 4) areg[i] = wtile[(size_t)kc * (16 * MT / 4) + idx];
        }
#pragma unroll
        for (int e = 0; e < NB; ++e) {
            const int c = (NT > 256) ? (e & 1) : 0;
            const int ci = (int)kt[e][0], joff = (int)kt[e][1];
            int ti = colt[c] + joff;
            bool ok = ci >= 0 && colbase[c] >= 0;
            if (a.pad_zero) {
                ok = ok && ti >= 0 && ti < a.Lin;
            } else {
                if (ti < 0) ti = -ti;
                if (ti >= a.Lin) ti = 2 * (a.Lin - 1) - ti;
            }
            if (a.buf32) {
                const unsigned off = ok ? (unsigned)(colbase[c] + mst_mul24(ci, a.Lin) + ti) * 4u : 0xfffffff0u;
                breg[e] = __builtin_bit_cast(float, mst_stream_load4(xs, off, 0u));
            } else {          // activations beyond the 32-bit / 24-bit ranges (uniform): 64-bit addresses, predicated loads
                float v = 0.0f;
                if (ok) v = a.x[(size_t)item0 * item_elems + ((long)(n0 + (tid + (NT > 256 ? (e & 1) : 0) * 256) % NT) / a.Lout - item0) * (long)item_elems +
                                (long)ci * a.Lin + ti];
                breg[e] = v;
            }
        }
        ktab_entries(kc + 1);
    };

    if (kc_lo < kc_hi) {
        ktab_entries(kc_lo);
        fetch(kc_lo);
    }
    for (int kc = kc_lo; kc < kc_hi; ++kc) {
        if (kc > kc_lo) __syncthreads();
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int idx = tid + i * 256;
            if (idx < 16 * MT / 4) ((f32x4 *)As)[idx] = areg[i];
        }
#pragma unroll
        for (int e = 0; e < NB; ++e) Bs[tid + e * 256] = breg[e];
        __syncthreads();
        if (kc + 1 < kc_hi) fetch(kc + 1);
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) {
            const float av = As[(2 * ks + h) * MT + 32 * mi + ln];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float bv = Bs[(2 * ks + h) * NT + 128 * ni + 32 * q + ln];
                acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[q], 0, 0, 0);
            }
        }
    }

    if (a.part) {            // split-K slice: raw partial sums, consecutive lanes = consecutive columns
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const long n = n0 + 128 * ni + 32 * q + ln;
            if (n < a.Ntot) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = cot * MT + 32 * mi + mfma32_row(r, lane);
                    if (co < a.Cout) a.part[((size_t)blockIdx.z * a.Cout + co) * a.Ntot + n] = acc[q][r];
                }
            }
        }
        return;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const long n = n0 + 128 * ni + 32 * q + ln;
        if (n < a.Ntot) {
            const int b = (int)(n / a.Lout), to = (int)(n % a.Lout);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = cot * MT + 32 * mi + mfma32_row(r, lane);
                if (co < a.Cout) {
                    float v = acc[q][r] + a.shift[co];
                    if (a.epi == 0) {
                        v = enc_act(v, a.slope);
                        if (a.residual) v += a.x[((long)b * a.Cin + co) * a.Lin + to];
                    } else if (a.epi == 1) {
                        const float *fr = a.film + (a.film_rows > 1 ? (size_t)b * 2 * a.Cout : 0);
                        v = fr[co] * leaky_relu(v) + fr[a.Cout + co];
                        v += a.res[co] * a.x[((long)b * a.Cin + co / a.res_div) * a.Lin + to];
                    } else {
                        v = fminf(1.0f, fmaxf(-1.0f, v));
                    }
                    a.y[((long)b * a.Cout + co) * a.Lout + to] = v;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Same convolution with bf16 MFMA operands (v_mfma_f32_32x32x16_bf16, fp32 accumulate): the throughput mode.
// Activations stay fp32 NCL in HBM; operands are rounded to bf16 while staging.  K-chunk = 32.
//   A: BN-folded weights pre-packed in fragment order, streamed from L2 straight into registers.
//   B: im2col tile in LDS as Bs[n][32 k] (k contiguous, 64 B per column) so a lane's 8 consecutive k are one
//      ds_read_b128; each staging thread gathers the 8 k of one (n, 16-byte slot) - consecutive lanes take
//      consecutive n, so every one of the 8 gathers is coalesced along time - and writes one ds_write_b128.
//      16-B slot index is XORed with (n >> 2) & 3 so reads and writes are bank-conflict free.
// ------------------------------------------------------------------------------------------------
template <int MW>
__global__ __launch_bounds__(256) void enc_conv_bf16_kernel(EncConvArgs a) {
    constexpr int NW = 4 / MW, MT = 32 * MW, NT = 128 * NW;
    constexpr int NE = NT / 64;                       // 16-byte slots gathered per thread per chunk
    constexpr int NCOL = (NT + 255) / 256;
    __shared__ __attribute__((aligned(16))) unsigned char Bs[NT * 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int ln = lane & 31, h = lane >> 5;
    const int mi = w % MW, ni = w / MW;
    const long n0 = (long)blockIdx.x * NT;
    const int cot = blockIdx.y;

    long colbase[NCOL];
    int colt[NCOL];
#pragma unroll
    for (int c = 0; c < NCOL; ++c) {
        const long n = n0 + (tid + c * 256) % NT;
        if (n < a.Ntot) {
            const int b = (int)(n / a.Lout), to = (int)(n % a.Lout);
            colbase[c] = (long)b * a.Cin * a.Lin;
            colt[c] = to * a.stride;
        } else {
            colbase[c] = -1;
            colt[c] = 0;
        }
    }

    f32x16 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[q][i] = 0.0f;

    const bf16x8 *wtile = (const bf16x8 *)a.wpk16 + (size_t)cot * a.nchunks32 * 2 * MW * 64;
    bf16x8 anxt[2], acur[2];
    float breg[NE][8];

    auto fetch = [&](int kc) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) anxt[ks] = wtile[((size_t)(kc * 2 + ks) * MW + mi) * 64 + lane];
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int idx = tid + e * 256;
            const int slot = idx / NT;
            const int c = (NT > 256) ? (e & 1) : 0;
            const int *kt = a.ktab + (size_t)(kc * 32 + slot * 8) * 2;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int ci = kt[2 * i], joff = kt[2 * i + 1];
                float v = 0.0f;
                if (ci >= 0 && colbase[c] >= 0) {
                    int ti = colt[c] + joff;
                    if (ti < 0) ti = -ti;
                    if (ti >= a.Lin) ti = 2 * (a.Lin - 1) - ti;
                    v = a.x[colbase[c] + (long)ci * a.Lin + ti];
                }
                breg[e][i] = v;
            }
        }
    };

    fetch(0);
    for (int kc = 0; kc < a.nchunks32; ++kc) {
        if (kc) __syncthreads();
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            const int idx = tid + e * 256;
            const int n = idx % NT, slot = idx / NT;
            bf16x8 v;
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = (__bf16)breg[e][i];
            *(bf16x8 *)(Bs + n * 64 + ((slot ^ ((n >> 2) & 3)) << 4)) = v;
        }
        acur[0] = anxt[0];
        acur[1] = anxt[1];
        __syncthreads();
        if (kc + 1 < a.nchunks32) fetch(kc + 1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int nl = 128 * ni + 32 * q + ln;
                const bf16x8 bv = *(const bf16x8 *)(Bs + nl * 64 + (((2 * ks + h) ^ ((nl >> 2) & 3)) << 4));
                acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(acur[ks], bv, acc[q], 0, 0, 0);
            }
        }
    }

#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const long n = n0 + 128 * ni + 32 * q + ln;
        if (n < a.Ntot) {
            const int b = (int)(n / a.Lout), to = (int)(n % a.Lout);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = cot * MT + 32 * mi + mfma32_row(r, lane);
                if (co < a.Cout) {
                    float v = enc_act(acc[q][r] + a.shift[co], a.slope);
                    if (a.residual) v += a.x[((long)b * a.Cin + co) * a.Lin + to];
                    a.y[((long)b * a.Cout + co) * a.Lout + to] = v;
                }
            }
        }
    }
}

// ================================================================================================
// bf16 throughput pipeline, channel-minor ("NLC") activations:  act[b][t][C] bf16.
// With the contraction index ordered k = j*Cin + ci, the 8 consecutive k an MFMA lane needs are 8 consecutive
// channels of ONE input row, i.e. one aligned 16-byte load - the im2col gather costs one load per 8 operands
// (reflection and stride only move whole rows).  Layers whose Cin < 8 (the stereo input block) run on the
// small direct kernel below, which also converts NCL fp32 -> NLC bf16.
// ================================================================================================
struct EncDirectArgs {
    const float *x;      // [B][Cin][Lin] fp32
    void *ylo;           // OUT_NLC and non-null: split mode - the low parts' plane (y then holds the high parts)
    void *y;             // OUT_NLC ? bf16 [B][Lout][Cout] : fp32 [B][Cout][Lout]
    const float *w;      // [Cout][Cin][ksz] BN-folded
    const float *shift;  // [Cout]
    int B, Cin, Lin, Cout, Lout, ksz, stride, dil, pad_l, residual;
    float slope;         // activation slope for negative values (enc_act)
};

// direct VALU convolution for tiny channel counts (Cin <= 4, Cout <= 32): one thread per output time step
template <bool OUT_NLC, int CM>
__global__ __launch_bounds__(256) void enc_direct_kernel(EncDirectArgs a) {
    constexpr int XS_MAX = 4 * (256 * 8 + 64);
    __shared__ float xs[XS_MAX];
    __shared__ __attribute__((aligned(16))) float ws[CM * 4 * 64];
    const int tid = threadIdx.x;
    const int tiles = (a.Lout + 255) / 256;
    const int b = blockIdx.x / tiles, t0 = (blockIdx.x % tiles) * 256;
    const int span = 255 * a.stride + (a.ksz - 1) * a.dil + 1;
    for (int i = tid; i < a.Cin * span; i += 256) {
        const int ci = i / span, k = i % span;
        int ti = t0 * a.stride - a.pad_l + k;
        if (ti < 0) ti = -ti;
        if (ti >= a.Lin) ti = 2 * (a.Lin - 1) - ti;
        xs[i] = (ti >= 0 && ti < a.Lin) ? a.x[((size_t)b * a.Cin + ci) * a.Lin + ti] : 0.0f;
    }
    // weights tap-major [ci * ksz + j][CM] (zero padded): one vector LDS read per 4 (2) channels instead of one read per
    // channel and tap (850 LDS reads per output at 2 -> 16 channels, k = 25)
    static_assert(CM >= 2, "channel tile");
    for (int i = tid; i < a.Cin * a.ksz * CM; i += 256) {
        const int co = i % CM, tap = i / CM;
        ws[i] = co < a.Cout ? a.w[(size_t)co * a.Cin * a.ksz + tap] : 0.0f;
    }
    __syncthreads();
    const int to = t0 + tid;
    float acc[CM];
#pragma unroll
    for (int co = 0; co < CM; ++co) acc[co] = 0.0f;
    for (int ci = 0; ci < a.Cin; ++ci)
        for (int j = 0; j < a.ksz; ++j) {
            const float xv = xs[ci * span + tid * a.stride + j * a.dil];
            const float *wt = ws + (ci * a.ksz + j) * CM;
            if constexpr (CM >= 4) {
#pragma unroll
                for (int c4 = 0; c4 < CM / 4; ++c4) {
                    const f32x4 wv = *(const f32x4 *)(wt + 4 * c4);
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[4 * c4 + i] = fmaf(wv[i], xv, acc[4 * c4 + i]);
                }
            } else {
                acc[0] = fmaf(wt[0], xv, acc[0]);
                acc[1] = fmaf(wt[1], xv, acc[1]);
            }
        }
    if (to >= a.Lout) return;
#pragma unroll
    for (int co = 0; co < CM; ++co) {
        if (co < a.Cout) {
            float v = enc_act(acc[co] + a.shift[co], a.slope);
            if (a.residual) v += xs[co * span + tid + a.pad_l];
            acc[co] = v;
        }
    }
    if (OUT_NLC) {
        __bf16 *yp = (__bf16 *)a.y + ((size_t)b * a.Lout + to) * a.Cout;
        __bf16 *ypl = a.ylo ? (__bf16 *)a.ylo + ((size_t)b * a.Lout + to) * a.Cout : nullptr;
#pragma unroll
        for (int c8 = 0; c8 < CM / 8; ++c8) {
            if (c8 * 8 < a.Cout) {
                bf16x8 o, ol;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    o[i] = (__bf16)acc[c8 * 8 + i];
                    ol[i] = (__bf16)(acc[c8 * 8 + i] - (float)o[i]);
                }
                *(bf16x8 *)(yp + c8 * 8) = o;
                if (ypl) *(bf16x8 *)(ypl + c8 * 8) = ol;
            }
        }
    } else {
        float *yp = (float *)a.y + (size_t)b * a.Cout * a.Lout + to;
#pragma unroll
        for (int co = 0; co < CM; ++co)
            if (co < a.Cout) yp[(size_t)co * a.Lout] = acc[co];
    }
}

// ------------------------------------------------------------------------------------------------
// The stereo block of the default encoder in ONE launch (round 5): Res_ConvBlock 0 = Conv1d_layer(2 -> 2, k = 25, stride 1) + skip, then
// Conv1d_layer(2 -> 16, k = 25, stride 4) (network_utils.py:96-119 on configs.yaml's first entries).  Two enc_direct_kernel launches took
// 71 + 60 us per 32 segments for 2.5 GFLOP and 4 x 33.5 MB: one thread per output step, one LDS read per multiply-add, the 33.5 MB
// intermediate through HBM.  A first fused form on packed VALU multiply-adds with the weights through the scalar cache ran 94 us: every
// tap waited for its scalar loads (SMEM returns out of order: s_waitcnt lgkmcnt(0) each time).  This form puts both convolutions on
// v_mfma_f32_16x16x4_f32 - exact fp32, bit for bit a k-ordered fmaf chain, at the fp32 vector rate with the WEIGHTS RESIDENT IN REGISTERS as A
// fragments (16 + 14 per lane, packed by the host) and one ds_read_b32 per MFMA for the B operand:
//   * second conv: D[channel][time] = sum_k W[channel][k] T[k][time], k = ci * 28 + j (taps 25 .. 27: zero weights): 14 MFMAs per 16 output
//     steps; lane (n, kq) reads intermediate sample 4 (t + n) + 4 a + kq.
//   * first conv (2 output channels would fill an eighth of the rows): TOEPLITZ form - rows (co, r), r = 0 .. 7 the position inside a block of
//     eight, columns = blocks: D[(co, r)][q] = sum_(ci, k') w[co][ci][k' - r] x[ci][8 q + k'], k' = 0 .. 31 (zero where k' - r is no tap):
//     16 MFMAs per 128 positions x 2 channels, 1.6 x the useful multiply-adds instead of 8 x.
// Zero weights are exact no-ops of an fmaf chain (finite data), the taps come in the direct kernels' order (ci outer, tap inner, from
// zero, then shift / activation / skip): the same bits as the two direct kernels.  A workgroup owns TO = 240 outputs: 1056 staged input
// samples per channel (reflection applied), 1024 intermediate slots per channel in LDS; both LDS images are skewed (10 floats per 8 input
// samples, 6 per 4 intermediate samples) so that the 16 columns of a B fragment fall into different banks.  Intermediate positions outside
// the segment (the second conv's reflection padding) are copies of their mirror positions inside the tile.
// ------------------------------------------------------------------------------------------------
struct EncStereoArgs {
    const float *x;               // [B][2][L] fp32
    void *y, *ylo;                // bf16 [B][Lout][16]; ylo non-null: split mode, the low parts' plane
    const float *a0, *shift0;     // first conv: Toeplitz A fragments [16 k-steps][64 lanes] (enc_stereo_pack_a0), shift [2]
    const float *a1, *shift1;     // second conv: A fragments [14 k-steps][64 lanes] (enc_stereo_pack_a1), shift [16]
    int B, L, Lout, tiles;        // tiles = ceil(Lout / TO) per item
    float slope0, slope1;
};
constexpr int ENC_STEREO_TO = 240, ENC_STEREO_K = 25, ENC_STEREO_KS0 = 16, ENC_STEREO_KS1 = 14;
// host side: the fragment images of BN-folded weights w[Cout][2][25]
inline void enc_stereo_pack_a0(const float *w, float *frag) {          // lane (row = (co, r), kq), k-step kk: ci = kk / 8, k' = 4 (kk % 8) + kq, tap k' - r
    for (int kk = 0; kk < ENC_STEREO_KS0; ++kk)
        for (int l = 0; l < 64; ++l) {
            const int row = l & 15, kq = l >> 4, co = row >> 3, r = row & 7, ci = kk >> 3, j = 4 * (kk & 7) + kq - r;
            frag[kk * 64 + l] = (j >= 0 && j < ENC_STEREO_K) ? w[(co * 2 + ci) * ENC_STEREO_K + j] : 0.0f;
        }
}
inline void enc_stereo_pack_a1(const float *w, float *frag) {          // lane (row = channel, kq), k-step kk: ci = kk / 7, tap 4 (kk % 7) + kq
    for (int kk = 0; kk < ENC_STEREO_KS1; ++kk)
        for (int l = 0; l < 64; ++l) {
            const int co = l & 15, kq = l >> 4, ci = kk / 7, j = 4 * (kk % 7) + kq;
            frag[kk * 64 + l] = j < ENC_STEREO_K ? w[(co * 2 + ci) * ENC_STEREO_K + j] : 0.0f;
        }
}
__device__ __forceinline__ int enc_reflect(int t, int L) {
    if (t < 0) t = -t;
    if (t >= L) t = 2 * (L - 1) - t;
    return t;
}
__global__ __launch_bounds__(256) void enc_stereo_block_kernel(EncStereoArgs a) {
    constexpr int KSZ = ENC_STEREO_K, S1 = 4, C1 = 16, TO = ENC_STEREO_TO, PAD = (KSZ - 1) / 2;
    constexpr int NT = 1024, NX = NT + 32;               // intermediate slots (8 tiles of 16 blocks of 8); staged input samples (k' < 32)
    constexpr int XP = NX / 8 * 10, TP = NT / 4 * 6;     // skewed images
    constexpr int NT1 = TO / 16;                         // column tiles of the second conv
    static_assert(TO % 16 == 0 && S1 * (TO - 1) + 4 * 7 <= NT && NT1 <= 16, "tile geometry");
    __shared__ __attribute__((aligned(16))) float xs[2][XP];
    __shared__ __attribute__((aligned(16))) float ts[2][TP];
    auto xi = [](int p) { return p + 2 * (p >> 3); };                  // input sample p of the tile
    auto ti = [](int s) { return 6 * (s >> 2) + (s & 3); };            // intermediate slot s
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = lane & 15, g = lane >> 4;
    const int b = blockIdx.x / a.tiles, t0 = (blockIdx.x % a.tiles) * TO;
    const int p_first = S1 * t0 - PAD;                     // position (in the intermediate signal) of slot 0
    const float *xb = a.x + (size_t)b * 2 * a.L;
    // A fragments: constant per launch, 30 registers
    float A0[ENC_STEREO_KS0], A1[ENC_STEREO_KS1];
#pragma unroll
    for (int kk = 0; kk < ENC_STEREO_KS0; ++kk) A0[kk] = a.a0[kk * 64 + lane];
#pragma unroll
    for (int kk = 0; kk < ENC_STEREO_KS1; ++kk) A1[kk] = a.a1[kk * 64 + lane];
    // ---- stage the input samples p_first - PAD + [0, NX).  An interior tile (p_first - PAD is a multiple of 4): all of a thread's
    // 16-byte loads are in flight before the first LDS write; border tiles go element by element through the reflection
    static_assert(NX % 8 == 0 && (2 * NX / 4 + 255) / 256 == 3, "three 16-byte pieces per thread");
    if (p_first - PAD >= 0 && p_first - PAD + NX <= a.L && (a.L & 3) == 0) {          // uniform
        f32x4 v[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int i = tid + 256 * r, ci = i >= NX / 4 ? 1 : 0, k = i - ci * (NX / 4);
            if (i < 2 * NX / 4) v[r] = *(const f32x4 *)(xb + (size_t)ci * a.L + (p_first - PAD) + 4 * k);
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int i = tid + 256 * r, ci = i >= NX / 4 ? 1 : 0, k = i - ci * (NX / 4);
            if (i < 2 * NX / 4) {                           // four samples of one block of eight: contiguous in the skewed image, 8-byte aligned
                float *q = &xs[ci][xi(4 * k)];
                *(f32x2 *)q = f32x2{v[r][0], v[r][1]};
                *(f32x2 *)(q + 2) = f32x2{v[r][2], v[r][3]};
            }
        }
    } else {
        for (int i = tid; i < 2 * NX; i += 256) {
            const int ci = i >= NX ? 1 : 0, k = i - ci * NX;
            const int t = enc_reflect(p_first - PAD + k, a.L);
            xs[ci][xi(k)] = (t >= 0 && t < a.L) ? xb[(size_t)ci * a.L + t] : 0.0f;
        }
    }
    __syncthreads();
    // ---- first conv (Toeplitz) + shift + activation + skip: wave w owns column tiles 2 w, 2 w + 1 (128 slots each), interleaved (the
    // dependent-accumulator latency of the instruction is 40 cycles against its 32-cycle issue)
    {
        f32x4 acc[2] = {f32x4{0.0f, 0.0f, 0.0f, 0.0f}, f32x4{0.0f, 0.0f, 0.0f, 0.0f}};
        const float *bx = &xs[0][10 * (32 * w + n) + g];          // xi(8 q + 4 a + kq) = 10 q + 4 a + kq + 2 (a >> 1), q = 16 T + n
#pragma unroll
        for (int kk = 0; kk < ENC_STEREO_KS0; ++kk) {
            const int ci = kk >> 3, av = kk & 7, off = ci * XP + 4 * av + 2 * (av >> 1);
#pragma unroll
            for (int T = 0; T < 2; ++T) acc[T] = __builtin_amdgcn_mfma_f32_16x16x4f32(A0[kk], bx[off + 160 * T], acc[T], 0, 0, 0);
        }
        // lane (n, g): channel co = g >> 1, slots s = 8 q + 4 (g & 1) + 0 .. 3
        const int co = g >> 1;
        const float sh = a.shift0[co];
#pragma unroll
        for (int T = 0; T < 2; ++T) {
            const int s = 8 * (16 * (2 * w + T) + n) + 4 * (g & 1);
            const float *xr = &xs[co][xi(s + PAD)];                 // the skip: input sample of the same position (one block of eight: contiguous)
            const f32x2 x01 = *(const f32x2 *)xr, x23 = *(const f32x2 *)(xr + 2);
            float *q = &ts[co][ti(s)];
            *(f32x2 *)q = f32x2{enc_act(acc[T][0] + sh, a.slope0) + x01.x, enc_act(acc[T][1] + sh, a.slope0) + x01.y};
            *(f32x2 *)(q + 2) = f32x2{enc_act(acc[T][2] + sh, a.slope0) + x23.x, enc_act(acc[T][3] + sh, a.slope0) + x23.y};
        }
    }
    __syncthreads();
    // ---- the second conv's reflection padding: a slot outside the segment takes the value of its mirror position
    if (p_first < 0 || p_first + NT > a.L) {               // uniform: the first / last tiles of an item
        float fix[2][4];
        bool any = false;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int s = 4 * tid + p, pos = p_first + s;
            fix[0][p] = ts[0][ti(s)];
            fix[1][p] = ts[1][ti(s)];
            if (pos < 0 || pos >= a.L) {
                const int pr = enc_reflect(pos, a.L), sr = pr - p_first;
                if (pr >= 0 && pr < a.L && sr >= 0 && sr < NT) {
                    fix[0][p] = ts[0][ti(sr)];
                    fix[1][p] = ts[1][ti(sr)];
                } else {                                       // (a mirror position outside the tile: no default-geometry tile has one) computed from the input
#pragma unroll 1
                    for (int co = 0; co < 2; ++co) {
                        float acc = 0.0f;
                        if (pr >= 0 && pr < a.L) {
#pragma unroll 1
                            for (int ci = 0; ci < 2; ++ci)
#pragma unroll 1
                                for (int j = 0; j < KSZ; ++j) {
                                    const int t = enc_reflect(pr - PAD + j, a.L);
                                    // tap j of (co, ci) sits in row (co, r = 0) of the Toeplitz image at k' = j
                                    const float wv = a.a0[(8 * ci + (j >> 2)) * 64 + 16 * (j & 3) + 8 * co];
                                    acc = fmaf(wv, (t >= 0 && t < a.L) ? xb[(size_t)ci * a.L + t] : 0.0f, acc);
                                }
                            acc = enc_act(acc + a.shift0[co], a.slope0) + xb[(size_t)co * a.L + pr];
                        }
                        fix[co][p] = acc;
                    }
                }
                any = true;
            }
        }
        __syncthreads();                                       // every mirror source has been read
        if (any) {
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                ts[0][ti(4 * tid + p)] = fix[0][p];
                ts[1][ti(4 * tid + p)] = fix[1][p];
            }
        }
        __syncthreads();
    }
    // ---- second conv: wave w owns column tiles w, w + 4, w + 8, w + 12 (16 output steps each), two at a time
    const f32x4 sh1 = *(const f32x4 *)(a.shift1 + 4 * g);
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
        f32x4 acc[2] = {f32x4{0.0f, 0.0f, 0.0f, 0.0f}, f32x4{0.0f, 0.0f, 0.0f, 0.0f}};
        const int T0 = w + 8 * pr;                               // and T0 + 4
        const float *bt[2];                                      // ti(4 (16 T + n) + 4 a + kq) = 6 (16 T + n + a) + kq
#pragma unroll
        for (int T = 0; T < 2; ++T) bt[T] = &ts[0][6 * (16 * (T0 + 4 * T < NT1 ? T0 + 4 * T : NT1 - 1) + n) + g];
#pragma unroll
        for (int kk = 0; kk < ENC_STEREO_KS1; ++kk) {
            const int ci = kk / 7, av = kk % 7, off = ci * TP + 6 * av;
#pragma unroll
            for (int T = 0; T < 2; ++T) acc[T] = __builtin_amdgcn_mfma_f32_16x16x4f32(A1[kk], bt[T][off], acc[T], 0, 0, 0);
        }
#pragma unroll
        for (int T = 0; T < 2; ++T) {
            const int o = 16 * (T0 + 4 * T) + n, to = t0 + o;        // lane (n, g): output step o of the tile, channels 4 g .. 4 g + 3
            if (T0 + 4 * T < NT1 && to < a.Lout) {
                bf16x4 hi, lo;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = enc_act(acc[T][e] + sh1[e], a.slope1);
                    hi[e] = (__bf16)v;
                    lo[e] = (__bf16)(v - (float)hi[e]);
                }
                const size_t at = ((size_t)b * a.Lout + to) * C1 + 4 * g;
                *(bf16x4 *)((__bf16 *)a.y + at) = hi;
                if (a.ylo) *(bf16x4 *)((__bf16 *)a.ylo + at) = lo;
            }
        }
    }
}

struct EncNlcArgs {
    const __bf16 *x;     // [B][Lin][Cin]
    __bf16 *y;           // [B][Lout][Cout]
    const __bf16 *xlo;   // split mode (X3): the low parts of the input, same layout (x = x_hi + x_lo, both bf16)
    __bf16 *ylo;         // split mode: the low parts of the output
    const void *wpk_lo;  // split mode: the low parts of the folded weights, same fragment order
    float *part;         // split-K partial sums [S][Ntot][Cout] fp32 (null when S == 1)
    const void *wpk;     // bf16 A fragments [co_tiles][nchunks][4][MW][64][8], k = j*Cin + ci
    const float *shift;  // [co_tiles*MT]
    const int *stab;     // [nchunks*8][2]: 16-byte slot -> (j*dil - pad_l, ci0); ci0 = -1 beyond K
    int B, Cin, Lin, Cout, Lout, stride, nchunks, residual, S;
    long Ntot;
    int ksz, pad_l;      // enc_conv_rows_kernel only
    float slope;         // activation slope for negative values (enc_act)
    int wmajor;          // enc_conv_nlc_kernel: > 0 = 1-d grid in WEIGHT-major order, value = number of channel tiles (see the kernel)
    const void *zeros;   // enc_conv_nlc_kernel: 16 bytes of zeros (rows / k-slots outside the problem are fetched from here)
};

// implicit-GEMM convolution on NLC bf16 activations, v_mfma_f32_32x32x16_bf16, K-chunk = 64 (8 slots per row).
// Tile (32*MW) channels x (128*4/MW) columns; optional split-K over blockIdx.z for the short, wide late layers.
// split mode ("bf16x3", the encoder's <= 1e-4 mode on the bf16 matrix cores): every fp32 value travels as two bf16 values
// x = x_hi + x_lo (x_hi = bf16(x), x_lo = bf16(x - x_hi): 16 significant bits; products of bf16 values are exact in fp32), activations as
// two NLC planes, weights as two fragment images, and a product is three MFMAs W_lo x_hi + W_hi x_lo + W_hi x_hi into one fp32 accumulator.
__device__ __forceinline__ void enc_split4(const float (&v)[4], bf16x4 &hi, bf16x4 &lo) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        hi[i] = (__bf16)v[i];
        lo[i] = (__bf16)(v[i] - (float)hi[i]);
    }
}

template <int MW, bool X3 = false>
__global__ __launch_bounds__(256) void enc_conv_nlc_kernel(EncNlcArgs a) {
    constexpr int NW = 4 / MW, MT = 32 * MW, NT = 128 * NW;
    constexpr int NL = NT / 32;                        // 16-byte loads per thread per chunk
    __shared__ __attribute__((aligned(16))) unsigned char Bs[(X3 ? 2 : 1) * NT * 128];
    unsigned char *const Bl = Bs + NT * 128;           // split mode: the low parts' tile
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int ln = lane & 31, h = lane >> 5;
    const int mi = w % MW, ni = w / MW;
    // workgroup -> (column tile, channel tile, k-slice).  Workgroups go round-robin over the 8 XCDs (their own L2 each).  Default order:
    // column tile fastest - the channel tiles / k-slices of a column tile meet in one L2 and share its ACTIVATION rows.  The short wide late
    // layers (1024 columns, 10-42 MB of weights) are the other way round: there every XCD fetched the whole weight image (8 x 42 MB
    // through the fabric per launch); in weight-major order (channel tile, k-slice) runs fastest, so that all column tiles of one weight
    // slice sit on ONE XCD and the slice crosses the fabric once.
    long n0;
    int cot, z;
    if (a.wmajor > 0) {
        const int cz = a.wmajor * a.S, q = (int)(blockIdx.x % cz);
        n0 = (long)(blockIdx.x / cz) * NT;
        cot = q % a.wmajor;
        z = q / a.wmajor;
    } else {
        n0 = (long)blockIdx.x * NT;
        cot = blockIdx.y;
        z = blockIdx.z;
    }
    const int kc_lo = (int)((long)z * a.nchunks / a.S), kc_hi = (int)((long)(z + 1) * a.nchunks / a.S);
    const int slot = tid & 7;

    // Operand loads as raw buffer loads (round 3): the address of a load is a 32-bit per-lane byte offset + a scalar offset on top of a
    // workgroup-uniform descriptor - no 64-bit address arithmetic in vector registers (the im2col gather spent ~80 VALU instructions per
    // wave and chunk on it, in front of every 16 MFMAs), and an offset beyond the descriptor's size returns ZEROS, which is what rows /
    // k-slots outside the problem need.  Activation descriptor: from the first batch item of this tile on (a tile spans at most NT items).
    const int item0 = (int)(n0 / a.Lout);
    const size_t item_elems = (size_t)a.Lin * a.Cin, left = ((size_t)a.B - item0) * item_elems * 2;
    const unsigned xbytes = left < 0x7fffffffu ? (unsigned)left : 0x7fffffffu;
    const MstStream16 xs = mst_stream16(a.x + (size_t)item0 * item_elems, xbytes);
    const MstStream16 xls = mst_stream16((X3 ? a.xlo : a.x) + (size_t)item0 * item_elems, xbytes);
    int rowb[NL], rowt[NL];                           // element offset of the row's batch item in the descriptor (-1: no row) / first input time
#pragma unroll
    for (int e = 0; e < NL; ++e) {
        const long n = n0 + (tid >> 3) + 32 * e;
        if (n < a.Ntot) {
            rowb[e] = (int)((n / a.Lout - item0) * (long)item_elems);
            rowt[e] = (int)(n % a.Lout) * a.stride;
        } else {
            rowb[e] = -1;
            rowt[e] = 0;
        }
    }

    f32x16 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[q][i] = 0.0f;

    const unsigned wbytes = (unsigned)a.nchunks * 4u * MW * 64u * 16u;                      // one channel tile's fragments (host: < 2^31)
    const MstStream16 ws = mst_stream16((const unsigned char *)a.wpk + (size_t)cot * wbytes, wbytes);
    const MstStream16 wls = mst_stream16((const unsigned char *)a.wpk_lo + (size_t)cot * wbytes, wbytes);
    const unsigned wlane = (unsigned)(mi * 64 + lane) * 16u;
    bf16x8 anxt[4], acur[4], breg[NL];
    bf16x8 anxt_lo[X3 ? 4 : 1], acur_lo[X3 ? 4 : 1], breg_lo[X3 ? NL : 1];

    // The loads of chunk kc + 1 are issued at the top of chunk kc's MFMA block and must stay in flight across it.  Two things kept them
    // from doing so (ISA of round 3: `s_waitcnt vmcnt(0)` BEFORE the MFMAs, i.e. two serial memory latencies per chunk and no overlap
    // inside a wave): (1) the row addresses depend on the slot table entry, itself a load - the entry is now fetched one chunk earlier
    // (sj / sc); (2) rows / k-slots outside the problem were zeroed by a select on the loaded value, which hipcc schedules right behind the
    // load - they are now fetched from a zero page instead (select on the ADDRESS, nothing to do on the value).
    int sj = 0, sc = -1;                              // slot table entry of the chunk the next fetch() stages
    auto stab_entry = [&](int kc) {
        const int k2 = kc < kc_hi ? kc : kc_hi - 1;
        const u32x2 e = *(const u32x2 *)(a.stab + (k2 * 8 + slot) * 2);
        sj = (int)e[0];
        sc = (int)e[1];
    };
    auto fetch = [&](int kc) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const unsigned so = (unsigned)(kc * 4 + ks) * (MW * 64u * 16u);
            anxt[ks] = __builtin_bit_cast(bf16x8, mst_stream_load16(ws, wlane, so));
            if constexpr (X3) anxt_lo[ks] = __builtin_bit_cast(bf16x8, mst_stream_load16(wls, wlane, so));
        }
        const int joff = sj, ci0 = sc;
#pragma unroll
        for (int e = 0; e < NL; ++e) {
            const bool ok = ci0 >= 0 && rowb[e] >= 0;
            int ti = rowt[e] + joff;
            if (ti < 0) ti = -ti;
            if (ti >= a.Lin) ti = 2 * (a.Lin - 1) - ti;
            const unsigned off = ok ? (unsigned)(rowb[e] + mst_mul24(ti, a.Cin) + ci0) * 2u : 0xfffffff0u;      // beyond the descriptor: zeros
            breg[e] = __builtin_bit_cast(bf16x8, mst_stream_load16(xs, off, 0u));
            if constexpr (X3) breg_lo[e] = __builtin_bit_cast(bf16x8, mst_stream_load16(xls, off, 0u));
        }
        stab_entry(kc + 1);
    };

    if (kc_lo < kc_hi) {
        stab_entry(kc_lo);
        fetch(kc_lo);
    }
    for (int kc = kc_lo; kc < kc_hi; ++kc) {
        if (kc > kc_lo) __syncthreads();
#pragma unroll
        for (int e = 0; e < NL; ++e) {
            const int n = (tid >> 3) + 32 * e;
            *(bf16x8 *)(Bs + n * 128 + ((slot ^ ((n >> 1) & 7)) << 4)) = breg[e];
            if constexpr (X3) *(bf16x8 *)(Bl + n * 128 + ((slot ^ ((n >> 1) & 7)) << 4)) = breg_lo[e];
        }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            acur[ks] = anxt[ks];
            if constexpr (X3) acur_lo[ks] = anxt_lo[ks];
        }
        __syncthreads();
        // (round 5, phase clocks of this loop on the 2048 -> 2048 layers - profiles/r05_enc_conv_phase_clocks.txt: issuing the next chunk's
        //  eight loads and their address arithmetic took 1650 of a chunk's 5400 clocks - the co-resident workgroups' MFMA streams starve a
        //  wave's VALU / VMEM issue; the issue runs at raised priority)
        __builtin_amdgcn_s_setprio(3);
        if (kc + 1 < kc_hi) fetch(kc + 1);
        __builtin_amdgcn_s_setprio(0);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int nl = 128 * ni + 32 * q + ln;
                const int off = nl * 128 + (((2 * ks + h) ^ ((nl >> 1) & 7)) << 4);
                const bf16x8 bv = *(const bf16x8 *)(Bs + off);
                if constexpr (X3) {          // the small terms first
                    const bf16x8 bl = *(const bf16x8 *)(Bl + off);
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(acur_lo[ks], bv, acc[q], 0, 0, 0);
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(acur[ks], bl, acc[q], 0, 0, 0);
                }
                acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(acur[ks], bv, acc[q], 0, 0, 0);
            }
        }
    }

#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const long n = n0 + 128 * ni + 32 * q + ln;
        if (n < a.Ntot) {
            const int b = (int)(n / a.Lout), to = (int)(n % a.Lout);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int co0 = cot * MT + 32 * mi + 8 * g + 4 * h;
                if (co0 < a.Cout) {
                    if (a.part) {
                        f32x4 o;
#pragma unroll
                        for (int i = 0; i < 4; ++i) o[i] = acc[q][4 * g + i];
                        *(f32x4 *)(a.part + ((size_t)z * a.Ntot + n) * a.Cout + co0) = o;
                    } else {
                        const f32x4 sh = *(const f32x4 *)(a.shift + co0);
                        bf16x4 o, r = {0, 0, 0, 0};
                        if (a.residual) r = *(const bf16x4 *)(a.x + (size_t)n * a.Cin + co0);
                        if constexpr (X3) {
                            bf16x4 rl = {0, 0, 0, 0}, ol;
                            if (a.residual) rl = *(const bf16x4 *)(a.xlo + ((size_t)b * a.Lin + to) * a.Cin + co0);
                            float v[4];
#pragma unroll
                            for (int i = 0; i < 4; ++i) v[i] = enc_act(acc[q][4 * g + i] + sh[i], a.slope) + ((float)r[i] + (float)rl[i]);
                            enc_split4(v, o, ol);
                            *(bf16x4 *)(a.ylo + ((size_t)b * a.Lout + to) * a.Cout + co0) = ol;
                        } else {
#pragma unroll
                            for (int i = 0; i < 4; ++i) o[i] = (__bf16)(enc_act(acc[q][4 * g + i] + sh[i], a.slope) + (float)r[i]);
                        }
                        *(bf16x4 *)(a.y + (size_t)n * a.Cout + co0) = o;
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The 128-channel conv kernel on RAW INPUT ROWS with loader waves (round 5, bf16 mode): blocks 4 ... 11 of the default encoder.
// enc_conv_nlc_kernel<4> stages an im2col B tile (128 columns x 64 k = 16 KB) per k-chunk and uses it for 16 MFMAs per wave: on the late
// layers the B tiles (332 MB per launch) and the weight fragments (each crosses L2 -> CU once per 128-column tile: 336 MB) together run the
// L2 at ~13 TB/s - that, not the matrix pipe (0.28 busy), bounds the launch (EXPERIMENTS.md D.12: loader waves on the same tiles and wider
// tiles alone change nothing).  This kernel is built like the TCN's: a workgroup = 8 waves = 128 channels x 256 columns; per 64-CHANNEL BLOCK
// the loader waves (4-7) fetch the input rows of the tile's columns ONCE by LDS-DMA (a 32-column sub-tile is 32 consecutive output steps of
// one item: 31 s + k input rows of 128 bytes, mirrored at the item's ends) into one of two buffers, and the matrix waves (0-3: 32 channels x
// 256 columns = 8 accumulator tiles of 32 x 32 each) walk ALL k taps over them - tap j of column n is row n s + j - so a staged byte feeds k
// times the MFMAs (5-10 x less staging), a weight fragment twice the MFMAs, and there is ONE barrier per channel block (k chunks = 160-320
// MFMAs per wave).  The k-chunks are the four-wave kernel's (chunk = tap j x 64-channel block cb: its A fragments are fetched as they lie),
// visited block-major instead of tap-major; split-K runs over channel blocks.  Same products, another fp32 summation order.
// ------------------------------------------------------------------------------------------------
struct EncTapsArgs {
    const __bf16 *x;     // [B][Lin][Cin]
    __bf16 *y;           // [B][Lout][Cout]
    float *part;         // split-K partial sums [S][Ntot][Cout] fp32 (null when S == 1)
    const void *wpk;     // bf16 A fragments of v_mfma_f32_16x16x32_bf16 [co_tiles][nchunks][2][8][64][8] (enc_taps_pack)
    const float *shift;  // [co_tiles * 128]
    int B, Cin, Lin, Cout, Lout, stride, ksz, pad_l, nchunks, residual, S;
    long Ntot;
    float slope;
    const void *zeros;   // 16 bytes of zeros
};
template <int KSZ, int STRIDE>
__global__ __launch_bounds__(512, 1) void enc_conv_taps_kernel(EncTapsArgs a) {
    constexpr int MT = 128, NQ = 8, NT = 32 * NQ, RQ = 31 * STRIDE + KSZ;      // rows of a 32-column sub-tile
    constexpr int NR = (NQ * RQ + 7) / 8 * 8, BUF = NR * 128, NP = NR / 8, NPW = (NP + 3) / 4;      // image rows (whole DMA pieces of 8), pieces, pieces per loader wave
    static_assert(2 * BUF <= 160 * 1024 - 512, "two images fit the CU's LDS");
    __shared__ __attribute__((aligned(1024))) unsigned char Bs[2 * BUF];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const bool loader = wv >= 4;
    const int w = wv & 3;
    const long n0 = (long)blockIdx.x * NT;
    const int cot = blockIdx.y, z = blockIdx.z;
    const int nblk = a.Cin / 64;                                        // channel blocks; chunk (tap j, block cb) = j * nblk + cb
    const int cb_lo = (int)((long)z * nblk / a.S), cb_hi = (int)((long)(z + 1) * nblk / a.S), nb = cb_hi - cb_lo;

    if (loader) {
        // ================================================================= loader waves: piece pi = w + 4 i = image rows 8 pi .. 8 pi + 7; lane = (row lane >> 3, position lane & 7)
        const unsigned char *rowp[NPW];                                 // the lane's row in HBM at channel block 0, at its 16-byte piece; zeros: no such row
        bool live[NPW];
#pragma unroll
        for (int i = 0; i < NPW; ++i) {
            const int R = 8 * (w + 4 * i) + (lane >> 3), q = R / RQ, r = R - q * RQ;
            const long n = n0 + 32 * q;                                  // first column of the sub-tile: (item, first output step)
            live[i] = w + 4 * i < NP && q < NQ && n < a.Ntot;
            const unsigned nn = live[i] ? (unsigned)n : 0u;                // (host: Ntot < 2^31 - one 32-bit division per piece on the way to the first DMA)
            const int b = (int)(nn / (unsigned)a.Lout), to = (int)(nn - (unsigned)b * (unsigned)a.Lout);
            int ti = to * STRIDE - a.pad_l + r;
            if (ti < 0) ti = -ti;
            if (ti >= a.Lin) ti = 2 * (a.Lin - 1) - ti;
            live[i] = live[i] && ti >= 0 && ti < a.Lin;
            // position p of row R holds the 16-byte slot p ^ (R & 7)
            rowp[i] = (const unsigned char *)(a.x + ((size_t)b * a.Lin + (live[i] ? ti : 0)) * a.Cin) + 16 * ((lane & 7) ^ (R & 7));
            // the first block's piece leaves as soon as its pointer exists (the HBM latency of piece i under the address arithmetic of piece i + 1)
            if (nb > 0 && w + 4 * i < NP) mst_dma16(live[i] ? rowp[i] + (size_t)cb_lo * 128 : (const unsigned char *)a.zeros, Bs + (w + 4 * i) * 1024);
        }
        auto stage = [&](int cb, int buf) {
#pragma unroll
            for (int i = 0; i < NPW; ++i) {
                if (w + 4 * i < NP) {                                     // uniform per wave
                    const unsigned char *src = live[i] ? rowp[i] + (size_t)cb * 128 : (const unsigned char *)a.zeros;
                    mst_dma16(src, Bs + buf * BUF + (w + 4 * i) * 1024);
                }
            }
        };
        mst_dma_wait_barrier<0>();                                       // (P) block cb_lo has landed
        for (int i = 0; i < nb; ++i) {
            if (i + 1 < nb) stage(cb_lo + i + 1, (i + 1) & 1);           // the other buffer: everybody left it at barrier i - 1
            mst_dma_wait_barrier<0>();                                   // (i) block i + 1 has landed; the matrix waves are done with block i
        }
        return;
    }

    // ===================================================================== matrix waves, 2 x 2: wave w = channels 64 (w & 1) .. + 63, columns 128 (w >> 1) .. + 127 of the tile,
    // on v_mfma_f32_16x16x32_bf16 (four row tiles x eight column tiles of 16 x 16 = 128 accumulator registers): a B fragment (one ds_read_b128) feeds
    // FOUR MFMAs, an A fragment eight.  (A first form on v_mfma_f32_32x32x16_bf16 - the four-wave kernel's instruction and weight image - ran 45 us
    // on the 2048 -> 2048 layers whatever its operand traffic: knock-out builds without the weight stream and without the LDS reads took the same
    // time, i.e. that instruction stream itself issued at ~76 nominal clocks per MFMA; the TCN's 16 x 16 x 32 stream sustains twice that.)
    __builtin_amdgcn_s_setprio(2);
    const int n16 = lane & 15, kg = lane >> 4, mi2 = w & 1, ni2 = w >> 1;
    f32x4 acc[4][8];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[m][c] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    // A fragments: w16[channel tile][chunk = tap * nblk + block][k-step 0..1][row tile 0..7][lane] x 16 bytes (enc_taps_pack)
    const unsigned wbytes = (unsigned)a.nchunks * 2u * 8u * 64u * 16u;                      // one channel tile's fragments (host: < 2^31)
    const MstStream16 ws = mst_stream16((const unsigned char *)a.wpk + (size_t)cot * wbytes, wbytes);
    const unsigned wlane = (unsigned)((4 * mi2) * 64 + lane) * 16u;
    bf16x8 A0[2][4], A1[2][4];
    auto fetch_a = [&](bf16x8 (&A)[2][4], int t) {       // tap t of the sequence of all blocks' taps (clamped)
        const int tt = t < nb * KSZ ? t : nb * KSZ - 1, ib = tt / KSZ, jt = tt - ib * KSZ, kc = jt * nblk + cb_lo + ib;
#pragma unroll
        for (int kh = 0; kh < 2; ++kh)
#pragma unroll
            for (int m = 0; m < 4; ++m)
                A[kh][m] = __builtin_bit_cast(bf16x8, mst_stream_load16(ws, wlane + m * 1024u, (unsigned)(kc * 2 + kh) * (8u * 64u * 16u)));
    };
    if (nb > 0) fetch_a(A0, 0);
    mst_dma_wait_barrier<63>();                                          // (P)
    int t = 0, j = 0, blk = 0;                                           // tap of the sequence = (block blk, tap j)
    // B fragments half a k-step ahead (a ring of two sets of four column tiles)
    bf16x8 Bf[2][4];
    auto read_b = [&](bf16x8 (&B)[4], int blkr, int jr, int grp) {     // group grp = 2 kh + hq: k-step kh, column tiles 4 hq .. 4 hq + 3 of the wave
        const int kh = grp >> 1, hq = grp & 1;
        const unsigned char *bt = Bs + (blkr & 1) * BUF + ((4 * ni2 + 2 * hq) * RQ + jr) * 128;
        int lr = n16 * STRIDE, kk = kg;                  // (opaque per read set: hipcc otherwise keeps the swizzled addresses of all (tap, column tile) pairs live and spills)
        asm volatile("" : "+v"(lr), "+v"(kk));
        const int jj = jr + (4 * ni2 + 2 * hq) * RQ;
#pragma unroll
        for (int c = 0; c < 4; ++c) {                                    // column tile 4 hq + c: 32-column sub-tile 2 hq + (c >> 1) of the wave's four, its half c & 1
            const int R = (c >> 1) * RQ + (c & 1) * 16 * STRIDE + lr, sw = (R + jj) & 7;
            B[c] = *(const bf16x8 *)(bt + R * 128 + (((4 * kh + kk) ^ sw) << 4));
        }
    };
    auto tap = [&](bf16x8 (&A)[2][4], bf16x8 (&Anext)[2][4]) {
        if (blk >= nb) return;                                           // uniform
        fetch_a(Anext, t + 1);
        if (j == 0) read_b(Bf[0], blk, 0, 0);                            // a block's first fragments: its image has just landed (barrier)
#pragma unroll
        for (int grp = 0; grp < 4; ++grp) {
            if (grp < 3) read_b(Bf[(grp + 1) & 1], blk, j, grp + 1);
            else if (j + 1 < KSZ) read_b(Bf[0], blk, j + 1, 0);          // uniform
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    acc[m][4 * (grp & 1) + c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[grp >> 1][m], Bf[grp & 1][c], acc[m][4 * (grp & 1) + c], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);                          // (keeps the reads of one group ahead, not of a whole tap)
        }
        ++t;
        if (++j == KSZ) {
            j = 0;
            ++blk;
            mst_dma_wait_barrier<63>();                                  // (blk - 1): done with this block's image; the next one has landed
        }
    };
    while (blk < nb) {
        tap(A0, A1);
        tap(A1, A0);
    }
    // D: lane (n16, kg) holds rows 4 kg .. 4 kg + 3 of a row tile = four consecutive channels of one column
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const long n = n0 + 128 * ni2 + 16 * c + n16;
        if (n < a.Ntot) {                                                // (column n = (item, step) of y, and - a residual layer keeps the shape - of x)
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int co0 = cot * MT + 64 * mi2 + 16 * m + 4 * kg;
                if (co0 < a.Cout) {
                    if (a.part) {
                        *(f32x4 *)(a.part + ((size_t)z * a.Ntot + n) * a.Cout + co0) = acc[m][c];
                    } else {
                        const f32x4 sh = *(const f32x4 *)(a.shift + co0);
                        bf16x4 o, r = {0, 0, 0, 0};
                        if (a.residual) r = *(const bf16x4 *)(a.x + (size_t)n * a.Cin + co0);
#pragma unroll
                        for (int i = 0; i < 4; ++i) o[i] = (__bf16)(enc_act(acc[m][c][i] + sh[i], a.slope) + (float)r[i]);
                        *(bf16x4 *)(a.y + (size_t)n * a.Cout + co0) = o;
                    }
                }
            }
        }
    }
}
// host side: the A fragments of enc_conv_taps_kernel for weights w[Cout][Cin][ksz] times the BN scale of their channel (Cin a multiple of 64), channel tile ct
// of the image [channel tile of 128][chunk = tap * (Cin / 64) + block][k-step 0..1][row tile 0..7][lane (row = l & 15, kg = l >> 4)][8]: k = 32 kh + 8 kg + e inside the block
inline void enc_taps_pack(const float *w, const float *scale, int cout, int cin, int ksz, int ct, __bf16 *img) {
    const int nblk = cin / 64;
    for (int j = 0; j < ksz; ++j)
        for (int cb = 0; cb < nblk; ++cb)
            for (int kh = 0; kh < 2; ++kh)
                for (int rt = 0; rt < 8; ++rt)
                    for (int l = 0; l < 64; ++l) {
                        const int co = ct * 128 + 16 * rt + (l & 15), ci0 = 64 * cb + 32 * kh + 8 * (l >> 4);
                        __bf16 *q = img + (((((size_t)ct * ksz * nblk + (j * nblk + cb)) * 2 + kh) * 8 + rt) * 64 + l) * 8;
                        for (int e = 0; e < 8; ++e) q[e] = (__bf16)(co < cout ? w[((size_t)co * cin + ci0 + e) * ksz + j] * scale[co] : 0.0f);
                    }
}

// ------------------------------------------------------------------------------------------------
// Res_ConvBlocks 1 and 2 of the default encoder in ONE launch each, bf16 mode (round 5): Conv1d_layer(C -> C, k, stride 1) + skip, then
// Conv1d_layer(C -> 2 C, k, stride S) (network_utils.py:96-119) for (C, k, S) = (16, 25, 4) and (32, 15, 2).  The two launches a block took
// (enc_conv_rows_kernel + enc_conv_nlc_kernel / enc_conv_rows_kernel: 50 + 34 us and 23 + 24 us per 32 segments) move the intermediate
// twice through HBM and are bound by memory and by launch-sized latencies; at 16 channels their 32-row MFMA tiles are half empty.  Here a
// workgroup owns TO = 256 outputs: its input rows arrive by LDS-DMA (the image is contiguous in HBM), the intermediate rows live in LDS
// only, both convs run on v_mfma_f32_16x16x32_bf16 with the contraction k = tap * C + ci (a k-step = 32 / C taps; taps beyond k have zero
// weights) and the weights RESIDENT in registers as A fragments (KS per 16-row tile; the second conv in passes of two row tiles).  B
// fragments are 16-byte reads of channel-minor rows: consecutive rows for the first conv, every S-th row for the second - the intermediate
// image is skewed by 16 bytes per S rows so that those reads spread over the banks.  Same operands as the two-launch form (bf16 weights,
// bf16 input, the intermediate rounded to bf16), fp32 accumulation in another order (k-steps of 32 instead of 16): results agree to
// accumulation rounding, not bit for bit.  The first conv of block 1 (16 output channels: every 1 KB B fragment feeds ONE MFMA) runs at the
// LDS read rate, twice its MFMA time (phase clocks: tools/micro/enc_block1_probe.hip).
// ------------------------------------------------------------------------------------------------
struct EncBlock1Args {
    const __bf16 *x;              // [B][L][C]
    __bf16 *y;                    // [B][Lout][2 C]
    const void *a0, *a1;          // A fragments: [C / 16 row tiles][KS][64 lanes] x 16 bytes / [2 C / 16][KS][64] x 16 bytes (enc_block1_pack)
    const float *shift0, *shift1; // [C] / [2 C]
    int B, L, Lout, tiles;
    float slope0, slope1;
    const void *zeros;            // 16 bytes of zeros (rows outside a reflected segment: shorter than the padding)
};
constexpr int ENC_B1_TO = 256;      // outputs per workgroup: 32 x 8192 / 256 = 1024 (block 1) and 32 x 4096 / 256 = 512 (block 2) workgroups = whole rounds at two per CU
constexpr int enc_block1_ks(int cin, int ksz) { return (cin * ksz + 31) / 32; }
// host side: A fragments of one 16-row tile of BN-folded weights w[Cout][cin][ksz]: lane (row, kg), k-step kk, element e: k = 32 kk + 8 kg + e = tap * cin + ci
inline void enc_block1_pack(const float *w, int row0, int cin, int ksz, __bf16 *frag) {
    for (int kk = 0; kk < enc_block1_ks(cin, ksz); ++kk)
        for (int l = 0; l < 64; ++l)
            for (int e = 0; e < 8; ++e) {
                const int co = row0 + (l & 15), k = 32 * kk + 8 * (l >> 4) + e, j = k / cin, ci = k % cin;
                frag[(kk * 64 + l) * 8 + e] = (__bf16)(j < ksz ? w[(co * cin + ci) * ksz + j] : 0.0f);
            }
}
template <int CIN, int KSZ, int S1, int NCT>          // NCT: 16-slot column tiles of the first conv a workgroup computes
__global__ __launch_bounds__(256, 2) void enc_block1_fused_kernel(EncBlock1Args a) {
    constexpr int COUT = 2 * CIN, RB = 2 * CIN, TO = ENC_B1_TO, PAD = (KSZ - 1) / 2, KS = enc_block1_ks(CIN, KSZ);
    constexpr int MA = CIN / 16, MB = COUT / 16, NT = 16 * NCT, NX = NT + 32, NT1 = TO / 16, JMAX = (32 * KS - 1) / CIN;      // JMAX: last tap a k-step touches
    constexpr int XB = NX * RB, TB = NT * RB + (NT / S1) * 16;
    static_assert(KSZ % 2 == 1 && (CIN == 16 || CIN == 32), "odd kernels; a k-step is a whole number of taps");
    static_assert(S1 * (TO - 1) + JMAX < NT && NT + JMAX <= NX && XB % 1024 == 0 && NT1 == 16 && NCT % 16 <= 4 && NT % S1 == 0 && S1 * RB == 128,
                  "tile geometry (the last group of first-conv tiles holds at most one tile per wave; lanes of a second-conv read are 144 bytes apart)");
    static_assert(2 * (XB + TB) <= 160 * 1024, "two workgroups per CU");
    __shared__ __attribute__((aligned(1024))) unsigned char xs[XB];      // input rows p_first - PAD + [0, NX): RB bytes each
    __shared__ __attribute__((aligned(16))) unsigned char ts[TB];        // intermediate slot s at RB s + 16 (s / S1)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, n = lane & 15, g = lane >> 4;
    const int b = blockIdx.x / a.tiles, t0 = (blockIdx.x % a.tiles) * TO;
    const int p_first = S1 * t0 - PAD;
    const unsigned char *xb = (const unsigned char *)a.x + (size_t)b * a.L * RB;
    // ---- stage the input rows: interior tiles by LDS-DMA (pieces of 1 KB: the image is contiguous in HBM), border tiles piece by piece
    if (p_first - PAD >= 0 && p_first - PAD + NX <= a.L) {          // uniform
        const unsigned char *src = xb + (size_t)(p_first - PAD) * RB + lane * 16;
        for (int k = w; k < XB / 1024; k += 4) mst_dma16(src + k * 1024, xs + k * 1024);
    } else {
        constexpr int PR = RB / 16;                                  // 16-byte pieces per row
        for (int i = tid; i < PR * NX; i += 256) {
            const int r = i / PR, t = enc_reflect(p_first - PAD + r, a.L);
            *(u32x4 *)(xs + 16 * i) = *(const u32x4 *)((t >= 0 && t < a.L) ? xb + (size_t)t * RB + 16 * (i % PR) : (const unsigned char *)a.zeros);
        }
    }
    // lane (n, kg = g) of k-step kk reads 16 bytes of row (column + tap), tap = (32 kk + 8 g) / CIN, at channel (32 kk + 8 g) % CIN
    auto tap_of = [](int kk, int kg) { return (32 * kk + 8 * kg) / CIN; };
    auto chb_of = [](int kk, int kg) { return 2 * ((32 * kk + 8 * kg) % CIN); };
    {
        bf16x8 A0[MA][KS];
#pragma unroll
        for (int m = 0; m < MA; ++m)
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) A0[m][kk] = ((const bf16x8 *)a.a0)[(m * KS + kk) * 64 + lane];
        mst_dma_wait_barrier<0>();
        // ---- first conv + shift + activation + skip: wave w owns column tiles w, w + 4, ... (16 slots each), four at a time, all row tiles
        f32x4 sh[MA];
#pragma unroll
        for (int m = 0; m < MA; ++m) sh[m] = *(const f32x4 *)(a.shift0 + 16 * m + 4 * g);
        // byte offset of the lane's piece in k-step 0 of column tile 0; a k-step adds 32 / CIN rows (CIN = 16: the odd k groups sit one row further)
        const unsigned char *bx = xs + (n + tap_of(0, g)) * RB + chb_of(0, g);
        constexpr int KSTEP = (32 / CIN) * RB;                       // bytes per k-step (CIN <= 32: a whole number of rows)
#pragma unroll 1
        for (int grp = 0; grp < (NCT + 15) / 16; ++grp) {           // column tile T = w + 4 (4 grp + c); the last group: one tile on the first waves
            const int nc = NCT - (w + 16 * grp) > 12 ? 4 : (NCT - (w + 16 * grp) + 3) / 4;      // uniform per wave
            if (nc <= 0) break;
            f32x4 acc[4][MA];
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int m = 0; m < MA; ++m) acc[c][m] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            const unsigned char *bg = bx + (w + 16 * grp) * 16 * RB;
            if (nc == 4) {
#pragma unroll
                for (int kk = 0; kk < KS; ++kk)
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const bf16x8 bv = *(const bf16x8 *)(bg + c * 64 * RB + kk * KSTEP);
#pragma unroll
                        for (int m = 0; m < MA; ++m) acc[c][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A0[m][kk], bv, acc[c][m], 0, 0, 0);
                        if (c == 3 && kk % 2 == 1) __builtin_amdgcn_sched_barrier(0);      // (keeps the scheduler from hoisting all 4 KS fragment reads: it spilled 326 registers at C = 32)
                    }
            } else {
#pragma unroll
                for (int kk = 0; kk < KS; ++kk) {
                    const bf16x8 bv = *(const bf16x8 *)(bg + kk * KSTEP);
#pragma unroll
                    for (int m = 0; m < MA; ++m) acc[0][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A0[m][kk], bv, acc[0][m], 0, 0, 0);
                }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {          // lane (n, g): slot sl, channels 16 m + 4 g .. + 3
                if (c < nc) {
                    const int sl = 16 * (w + 4 * (4 * grp + c)) + n;
#pragma unroll
                    for (int m = 0; m < MA; ++m) {
                        const bf16x4 r = *(const bf16x4 *)(xs + (sl + PAD) * RB + 32 * m + 8 * g);
                        bf16x4 o;
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] = (__bf16)(enc_act(acc[c][m][e] + sh[m][e], a.slope0) + (float)r[e]);
                        *(bf16x4 *)(ts + RB * sl + 16 * (sl / S1) + 32 * m + 8 * g) = o;
                    }
                }
            }
        }
    }
    bf16x8 A1[2][KS];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) A1[m][kk] = ((const bf16x8 *)a.a1)[(m * KS + kk) * 64 + lane];
    __syncthreads();
    // ---- the second conv's reflection padding: a slot outside the segment takes the row of its mirror position (inside the tile for every
    // slot an output reads; slots beyond those keep what the first conv made of the zero / mirrored input - finite, multiplied by zero weights)
    if (p_first < 0 || p_first + NT > a.L) {               // uniform: the first / last tiles of an item
        constexpr int PR = RB / 16, NF = (PR * NT + 255) / 256;
        u32x4 fix[NF];
        bool any[NF];
#pragma unroll
        for (int p = 0; p < NF; ++p) {
            const int i = tid + 256 * p, sl = i / PR, pos = p_first + sl, pr = enc_reflect(pos, a.L), sr = pr - p_first;
            any[p] = i < PR * NT && (pos < 0 || pos >= a.L) && pr >= 0 && pr < a.L && sr >= 0 && sr < NT;
            if (any[p]) fix[p] = *(const u32x4 *)(ts + RB * sr + 16 * (sr / S1) + 16 * (i % PR));
        }
        __syncthreads();                                       // every mirror source has been read
#pragma unroll
        for (int p = 0; p < NF; ++p) {
            const int i = tid + 256 * p, sl = i / PR;
            if (any[p]) *(u32x4 *)(ts + RB * sl + 16 * (sl / S1) + 16 * (i % PR)) = fix[p];
        }
        __syncthreads();
    }
    // ---- second conv: wave w owns column tiles w, w + 4, w + 8, w + 12 (16 output steps each), two at a time, two row tiles per pass
#pragma unroll 1
    for (int mp = 0; mp < MB / 2; ++mp) {
        if (mp > 0) {
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int kk = 0; kk < KS; ++kk) A1[m][kk] = ((const bf16x8 *)a.a1)[((2 * mp + m) * KS + kk) * 64 + lane];
        }
        const f32x4 sh1[2] = {*(const f32x4 *)(a.shift1 + 32 * mp + 4 * g), *(const f32x4 *)(a.shift1 + 32 * mp + 16 + 4 * g)};
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
            f32x4 acc[2][2];
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int m = 0; m < 2; ++m) acc[c][m] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            const int T0 = w + 8 * pr;                               // and T0 + 4
            const unsigned char *bt[2];                              // row S c + j at RB (S c + j) + 16 (c + j / S) = 144 c + ..., c = 16 T + n
#pragma unroll
            for (int c = 0; c < 2; ++c) bt[c] = ts + (S1 * RB + 16) * (16 * (T0 + 4 * c) + n);
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) {
                const int j = tap_of(kk, g);                         // lane-dependent when a k-step spans two taps
                const int off = RB * j + 16 * (j / S1) + chb_of(kk, g);
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const bf16x8 bv = *(const bf16x8 *)(bt[c] + off);
#pragma unroll
                    for (int m = 0; m < 2; ++m) acc[c][m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A1[m][kk], bv, acc[c][m], 0, 0, 0);
                }
                if (kk % 2 == 1) __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int o = 16 * (T0 + 4 * c) + n, to = t0 + o;        // lane (n, g): output step o of the tile, channels 32 mp + 16 m + 4 g ..
                if (to < a.Lout) {
#pragma unroll
                    for (int m = 0; m < 2; ++m) {
                        bf16x4 ov;
#pragma unroll
                        for (int e = 0; e < 4; ++e) ov[e] = (__bf16)enc_act(acc[c][m][e] + sh1[m][e], a.slope1);
                        *(bf16x4 *)(a.y + ((size_t)b * a.Lout + to) * COUT + 32 * mp + 16 * m + 4 * g) = ov;
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The same convolution for the long early layers, with the input rows of a tile RESIDENT in LDS.  The im2col form above
// stages a fresh 64-k slice of the B operand per chunk, i.e. it reads every input row ksz times (and once more per
// channel tile) from L2: 3.6 GB per encoder pass, the bound of those launches.  Here a workgroup owns NT consecutive
// output times of ONE batch item, stages the (NT-1)*stride + ksz input rows it needs once (reflection applied while
// staging), and every k-step of 16 = one tap x 16 input channels reads its B fragment straight from those rows: no
// barrier in the main loop, A fragments stream from L2 as before.  Rows are stored phase-major (row r at phase r % stride,
// index r / stride) with a pitch of Cin*2 + 16 bytes, so that the 32 rows of a fragment - stride apart in time - are
// consecutive LDS rows an odd number of 16-byte units apart: conflict-free ds_read_b128.
// Host-side eligibility: Cin % 16 == 0, no split-K (>= 512 tiles), Lout >= NT, rows fit 64 KB.
// ------------------------------------------------------------------------------------------------
template <int MW, bool X3 = false>
__global__ __launch_bounds__(256, 2) void enc_conv_rows_kernel(EncNlcArgs a) {
    constexpr int NW = 4 / MW, MT = 32 * MW, NT = 128 * NW;
    constexpr int ROWS_BYTES = X3 ? 80 * 1024 : 64 * 1024;       // split mode: the high parts' rows, then the low parts' (host: both fit)
    __shared__ __attribute__((aligned(16))) unsigned char rows[ROWS_BYTES];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int ln = lane & 31, h = lane >> 5;
    const int mi = w % MW, ni = w / MW;
    const int tiles_item = (a.Lout + NT - 1) / NT;
    const int b = blockIdx.x / tiles_item, to0 = (blockIdx.x % tiles_item) * NT;
    const int cot = blockIdx.y;
    const int s = a.stride, pitch = a.Cin * 2 + 16, c8n = a.Cin / 8;
    const int R = (NT - 1) * s + a.ksz, rpp = (R + s - 1) / s;
    const __bf16 *xb = a.x + (size_t)b * a.Lin * a.Cin;
    const __bf16 *xbl = X3 ? a.xlo + (size_t)b * a.Lin * a.Cin : nullptr;
    const int lo_off = s * rpp * pitch;                               // split mode: byte offset of the low parts' rows
    for (int p = tid; p < R * c8n; p += 256) {
        const int r = p / c8n, c8 = p - r * c8n;
        int ti = to0 * s - a.pad_l + r;
        if (ti < 0) ti = -ti;
        if (ti >= a.Lin) ti = 2 * (a.Lin - 1) - ti;
        const bool ok = ti >= 0 && ti < a.Lin;                       // rows of a ragged last tile can fall outside even after reflection
        const bf16x8 ld = *(const bf16x8 *)(xb + (size_t)(ok ? ti : 0) * a.Cin + c8 * 8);
        *(bf16x8 *)(rows + ((r % s) * rpp + r / s) * pitch + c8 * 16) = ok ? ld : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if constexpr (X3) {
            const bf16x8 ll = *(const bf16x8 *)(xbl + (size_t)(ok ? ti : 0) * a.Cin + c8 * 8);
            *(bf16x8 *)(rows + lo_off + ((r % s) * rpp + r / s) * pitch + c8 * 16) = ok ? ll : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
    }
    f32x16 acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[q][i] = 0.0f;
    // A fragments: raw buffer loads (lane offset + scalar k-step offset), a ring of four k-steps: the fragment of k-step ks + 4 is requested
    // right behind the MFMAs of k-step ks (one k-step ahead, as before round 3, left the L2 latency of every fragment exposed: there
    // is nothing else to wait for in this loop)
    const unsigned wbytes = (unsigned)a.nchunks * 4u * MW * 64u * 16u;
    const MstStream16 ws = mst_stream16((const unsigned char *)a.wpk + (size_t)cot * wbytes, wbytes);
    const MstStream16 wls = mst_stream16((const unsigned char *)a.wpk_lo + (size_t)cot * wbytes, wbytes);
    const unsigned wlane = (unsigned)(mi * 64 + lane) * 16u;
    const int nks = (a.Cin * a.ksz) / 16;                             // k-steps that carry weights (K = Cin * ksz is a multiple of 16)
    bf16x8 ar[4], arl[X3 ? 4 : 1];
    auto fetch_a = [&](int ks, int u) {
        const unsigned so = (unsigned)(ks < nks ? ks : nks - 1) * (MW * 64u * 16u);
        ar[u] = __builtin_bit_cast(bf16x8, mst_stream_load16(ws, wlane, so));
        if constexpr (X3) arl[u] = __builtin_bit_cast(bf16x8, mst_stream_load16(wls, wlane, so));
    };
#pragma unroll
    for (int u = 0; u < 4; ++u) fetch_a(u, u);
    __syncthreads();
    const unsigned char *lanebase = rows + (128 * ni + ln) * pitch + 16 * h;
    for (int ks0 = 0; ks0 < nks; ks0 += 4) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int ks = ks0 + u;
            if (ks < nks) {          // uniform
                const int k0 = ks * 16, j = k0 / a.Cin, ci0 = k0 - j * a.Cin;
                const unsigned char *bp = lanebase + ((j % s) * rpp + j / s) * pitch + ci0 * 2;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const bf16x8 bv = *(const bf16x8 *)(bp + 32 * q * pitch);
                    if constexpr (X3) {
                        const bf16x8 bl = *(const bf16x8 *)(bp + lo_off + 32 * q * pitch);
                        acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(arl[u], bv, acc[q], 0, 0, 0);
                        acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ar[u], bl, acc[q], 0, 0, 0);
                    }
                    acc[q] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ar[u], bv, acc[q], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);          // the reload stays behind the MFMAs that read the same registers
                fetch_a(ks + 4, u);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int to = to0 + 128 * ni + 32 * q + ln;
        if (to < a.Lout) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int co0 = cot * MT + 32 * mi + 8 * g + 4 * h;
                if (co0 < a.Cout) {
                    const f32x4 sh = *(const f32x4 *)(a.shift + co0);
                    bf16x4 o, r = {0, 0, 0, 0};
                    if (a.residual) r = *(const bf16x4 *)(xb + (size_t)to * a.Cin + co0);
                    if constexpr (X3) {
                        bf16x4 rl = {0, 0, 0, 0}, ol;
                        if (a.residual) rl = *(const bf16x4 *)(xbl + (size_t)to * a.Cin + co0);
                        float v[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) v[i] = enc_act(acc[q][4 * g + i] + sh[i], a.slope) + ((float)r[i] + (float)rl[i]);
                        enc_split4(v, o, ol);
                        *(bf16x4 *)(a.ylo + ((size_t)b * a.Lout + to) * a.Cout + co0) = ol;
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i) o[i] = (__bf16)(enc_act(acc[q][4 * g + i] + sh[i], a.slope) + (float)r[i]);
                    }
                    *(bf16x4 *)(a.y + ((size_t)b * a.Lout + to) * a.Cout + co0) = o;
                }
            }
        }
    }
}

// split-K epilogue: sum the S partial tiles, + shift, ReLU, + residual, -> bf16 NLC
// (xres_lo / y_lo non-null: split mode - the residual is x_hi + x_lo, the result leaves as two planes)
__global__ __launch_bounds__(256) void enc_splitk_finalize_kernel(const float *part, int S, long Ntot, int Cout,
                                                                  const float *shift, const __bf16 *xres, __bf16 *y,
                                                                  const __bf16 *xres_lo, __bf16 *y_lo, float slope) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;       // one thread per 4 channels
    const long total = Ntot * (Cout / 4);
    if (i >= total) return;
    const long n = i / (Cout / 4);
    const int co0 = (int)(i % (Cout / 4)) * 4;
    f32x4 s = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int zz = 0; zz < S; ++zz) s += *(const f32x4 *)(part + ((size_t)zz * Ntot + n) * Cout + co0);
    const f32x4 sh = *(const f32x4 *)(shift + co0);
    bf16x4 r = {0, 0, 0, 0}, o;
    if (xres) r = *(const bf16x4 *)(xres + (size_t)n * Cout + co0);
    if (y_lo) {
        bf16x4 rl = {0, 0, 0, 0}, ol;
        if (xres_lo) rl = *(const bf16x4 *)(xres_lo + (size_t)n * Cout + co0);
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = enc_act(s[k] + sh[k], slope) + ((float)r[k] + (float)rl[k]);
        enc_split4(v, o, ol);
        *(bf16x4 *)(y_lo + (size_t)n * Cout + co0) = ol;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = (__bf16)(enc_act(s[k] + sh[k], slope) + (float)r[k]);
    }
    *(bf16x4 *)(y + (size_t)n * Cout + co0) = o;
}

// split-K finalize of the fp32 NCL kernel (encoder epilogue): y[b][co][to] = relu(sum_z part[z][co][n] + shift[co]) (+ x[b][co][to])
__global__ __launch_bounds__(256) void enc_splitk_finalize_ncl_kernel(const float *part, int S, long Ntot, int Cout, int Lout,
                                                                      const float *shift, const float *xres, float *y, float slope) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= Ntot * Cout) return;
    const int co = (int)(i / Ntot);
    const long n = i % Ntot;
    float s = 0.0f;
    for (int z = 0; z < S; ++z) s += part[((size_t)z * Cout + co) * Ntot + n];
    const long b = n / Lout, to = n % Lout;
    const size_t o = ((size_t)b * Cout + co) * Lout + to;
    float v = enc_act(s + shift[co], slope);
    if (xres) v += xres[o];
    y[o] = v;
}

// global average pool over time of an NLC bf16 activation -> fp32 [B][C]
__global__ __launch_bounds__(256) void enc_avgpool_nlc_kernel(const __bf16 *x, const __bf16 *xlo, float *y, int B, int Lf, int C) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * C) return;
    const int b = (int)(i / C), c = (int)(i % C);
    float s = 0.0f;
    for (int t = 0; t < Lf; ++t) {
        const size_t o = ((size_t)b * Lf + t) * C + c;
        s += xlo ? (float)x[o] + (float)xlo[o] : (float)x[o];
    }
    y[i] = s / (float)Lf;
}

// NLC bf16 -> NCL fp32 (parity probe only)
__global__ void enc_unpack_nlc_kernel(const __bf16 *x, const __bf16 *xlo, float *y, int B, int L, int C) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)B * L * C) return;
    const int c = i % C;
    const size_t bt = i / C;
    const int t = bt % L;
    const int b = bt / L;
    y[((size_t)b * C + c) * L + t] = xlo ? (float)x[i] + (float)xlo[i] : (float)x[i];
}

// AdaptiveAvgPool1d(1) + squeeze (architectures.py:62,67): one wave per (b, c) row.
__global__ __launch_bounds__(256) void enc_avgpool_kernel(const float *x, float *y, long rows, int Lf) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    float s = 0.0f;
    for (int t = lane; t < Lf; t += 64) s += x[row * Lf + t];
    s = wave_sum(s);
    if (lane == 0) y[row] = s / (float)Lf;
}

// mean over segment embeddings in canonical row order (style_transfer.py:152-153)
__global__ void embedding_mean_kernel(const float *emb, int n_rows, int dim, float *out) {
    const int d = blockIdx.x * 256 + threadIdx.x;
    if (d >= dim) return;
    float s = 0.0f;
    for (int r = 0; r < n_rows; ++r) s += emb[(size_t)r * dim + d];
    out[d] = s / (float)n_rows;
}

// ------------------------------------------------------------------------------------------------
// Conv1d_layer(mode="deconv") (reference network_utils.py:24-26,38-42: nn.ConvTranspose1d with padding = dilation * (k - 1) / 2 and
// output_padding = stride > 1): a transposed convolution IS the stride-1 convolution of the zero-stuffed input (x[i] at position
// pad_left + i * stride of a zero row of length Lu) with the tap-reversed, channel-transposed kernel - the conv kernels above then do the
// arithmetic (VALID padding).  This kernel writes the zero-stuffed rows: y[row][u] = x[row][(u - pad_left) / stride] where that is a
// sample, 0 elsewhere.  rows = B * C.  HBM-bound copy; training-only mode of the reference, provided for API completeness.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void enc_zero_stuff_kernel(const float *x, float *y, long rows, long L, int stride, long pad_left, long Lu) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * Lu) return;
    const long row = i / Lu, u = i - row * Lu, v = u - pad_left;
    float out = 0.0f;
    if (v >= 0 && v % stride == 0 && v / stride < L) out = x[row * L + v / stride];
    y[i] = out;
}
