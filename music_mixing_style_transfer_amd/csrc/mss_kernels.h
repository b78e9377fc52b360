// Fused multi-scale spectral distance (reference modules/loss.py MultiScale_Spectral_Loss_MidSide_DDSP over modules/front_back_end.py
// FrontEnd "mag"): one workgroup reads the samples of G = 4096 / n_fft consecutive frames of `est` and `tgt` of one (item, channel, scale),
// windows them, transforms them in LDS and leaves TWO doubles - sum |m_e - m_t| and sum (log10(m_e + eps) - log10(m_t + eps))^2 over
// bins 1 .. n_fft / 2 of its frames; no frame, spectrum or magnitude goes to HBM.  A second epilogue of the same kernel stores the
// magnitudes instead ([B, C, F, T], FrontEnd's own output).
//
// Transform.  A real frame of n samples is read as m = n / 2 complex numbers z[c] = x[2c] + i x[2c + 1] (csrc/fft_kernels.h's R2C form),
// so the 4096-complex LDS buffer holds 2 G sub-transforms: frame g of est at slot 2 g, of tgt at slot 2 g + 1.  est and tgt are NOT
// packed into one complex transform: every sub-transform runs the same instructions on the same twiddles, so identical inputs give
// identical bits (the distance of a signal to itself is exactly 0), an all-zero side channel stays exactly zero, and a signal's error
// depends on its own level only.  The complex FFT is decimation in frequency, in place, output in digit-reversed order (the epilogue
// reads bin k at mss_pos(k); nothing is re-ordered): an optional radix-2 pass when log2(m) is odd, then radix-4 passes.  Two
// consecutive radix-4 passes touch 16 elements base + j + e s, e < 16, which one thread holds in registers ("double pass"), so a
// 2048-point sub-transform is four LDS round trips: R2, S(256), D(16), D(1).  Element i lives at float2 index i + i / 16: with that
// skew the three access patterns - consecutive i (strides >= 64), 16 lanes x 16 strided (D(16)), 16 contiguous per lane (D(1): 17 l + e)
// - fall on distinct banks per half-wave.  Twiddles W_m^j, j < m / 2, sit in LDS (a global twiddle load per butterfly is an exposed L2
// round trip, see fft_lds16), float64 sine / cosine rounded once, like the window table.
//
// Sums.  Every thread adds its bins in float64 in a fixed order; the wave reduces by xor-shuffles, the four waves through LDS in wave
// order; mss_finalize_kernel adds the workgroup partials of one (item, channel) in group order.  No atomics: the value of an item does
// not depend on the run or on what else is in the batch.
#pragma once
#include "fft_kernels.h"

#define MSS_PTS 4096                                    // complex points per workgroup
#define MSS_LDS (MSS_PTS + MSS_PTS / 16)                // with the skew
#define MSS_EPI_TERMS 0
#define MSS_EPI_MAG 1

// The compiler may not choose which product of a * b + c * d it fuses: est and tgt are handled by different unrolled copies of the same
// statements, and two copies that fuse differently differ in the last bit (seen on the MI355X: the distance of a signal to itself came
// out as 1e-6 instead of 0).  Contraction is off from here to the end of this header (restored there); every fused multiply-add below
// is written out as fmaf.
#pragma clang fp contract(off)
__device__ __forceinline__ float2 mss_cmul(float2 a, float2 b) {
    return make_float2(fmaf(a.x, b.x, -(a.y * b.y)), fmaf(a.x, b.y, a.y * b.x));
}
__device__ __forceinline__ int mss_pad(int i) { return i + (i >> 4); }
// W_m^idx, idx < m, from the half table
__device__ __forceinline__ float2 mss_tw(const float2 *wl, int idx, int half) {
    float2 w = wl[idx & (half - 1)];
    if (idx & half) { w.x = -w.x; w.y = -w.y; }
    return w;
}
__device__ __forceinline__ void mss_r4(float2 &a0, float2 &a1, float2 &a2, float2 &a3) {
    const float2 s02 = make_float2(a0.x + a2.x, a0.y + a2.y), d02 = make_float2(a0.x - a2.x, a0.y - a2.y);
    const float2 s13 = make_float2(a1.x + a3.x, a1.y + a3.y), d13 = make_float2(a1.x - a3.x, a1.y - a3.y);
    a0 = make_float2(s02.x + s13.x, s02.y + s13.y);
    a1 = make_float2(d02.x + d13.y, d02.y - d13.x);      // d02 - i d13
    a2 = make_float2(s02.x - s13.x, s02.y - s13.y);
    a3 = make_float2(d02.x - d13.y, d02.y + d13.x);      // d02 + i d13
}
// radix-2 pass, stride s = m / 2 = 2^LOGS: 2048 butterflies, 8 per thread
template <int LOGM, int LOGS> __device__ __forceinline__ void mss_pass2(float2 *buf, const float2 *wl, int tid) {
#pragma unroll
    for (int e = 0; e < MSS_PTS / 2 / 256; ++e) {
        const int j = tid + 256 * e, jj = j & ((1 << LOGS) - 1), base = ((j >> LOGS) << (LOGS + 1)) + jj;
        const int p0 = mss_pad(base), p1 = mss_pad(base + (1 << LOGS));
        const float2 a = buf[p0], b = buf[p1];
        buf[p0] = make_float2(a.x + b.x, a.y + b.y);
        buf[p1] = mss_cmul(wl[jj << (LOGM - 1 - LOGS)], make_float2(a.x - b.x, a.y - b.y));
    }
    __syncthreads();
}
// radix-4 pass, stride s = 2^LOGS, blocks of 4 s: 1024 butterflies, 4 per thread
template <int LOGM, int LOGS> __device__ __forceinline__ void mss_pass4(float2 *buf, const float2 *wl, int tid) {
    constexpr int s = 1 << LOGS, half = 1 << (LOGM - 1);
#pragma unroll
    for (int e = 0; e < MSS_PTS / 4 / 256; ++e) {
        const int j = tid + 256 * e, jj = j & (s - 1), base = ((j >> LOGS) << (LOGS + 2)) + jj;
        float2 a0 = buf[mss_pad(base)], a1 = buf[mss_pad(base + s)], a2 = buf[mss_pad(base + 2 * s)], a3 = buf[mss_pad(base + 3 * s)];
        mss_r4(a0, a1, a2, a3);
        const int t = jj << (LOGM - 2 - LOGS);
        buf[mss_pad(base)] = a0;
        buf[mss_pad(base + s)] = mss_cmul(mss_tw(wl, t, half), a1);
        buf[mss_pad(base + 2 * s)] = mss_cmul(mss_tw(wl, 2 * t, half), a2);
        buf[mss_pad(base + 3 * s)] = mss_cmul(mss_tw(wl, 3 * t, half), a3);
    }
    __syncthreads();
}
// two radix-4 passes (strides 4 s and s, s = 2^LOGS, blocks of 16 s) on the 16 elements base + j + e s of one thread: the same
// butterflies and twiddles as mss_pass4<LOGS + 2> followed by mss_pass4<LOGS>, with the intermediate in registers
template <int LOGM, int LOGS> __device__ __forceinline__ void mss_pass16(float2 *buf, const float2 *wl, int tid) {
    constexpr int s = 1 << LOGS, half = 1 << (LOGM - 1);
    const int jj = tid & (s - 1), base = ((tid >> LOGS) << (LOGS + 4)) + jj;
    float2 x[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) x[a][b] = buf[mss_pad(base + (4 * a + b) * s)];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        mss_r4(x[0][b], x[1][b], x[2][b], x[3][b]);
        const int t = (jj + b * s) << (LOGM - 4 - LOGS);
        x[1][b] = mss_cmul(mss_tw(wl, t, half), x[1][b]);
        x[2][b] = mss_cmul(mss_tw(wl, 2 * t, half), x[2][b]);
        x[3][b] = mss_cmul(mss_tw(wl, 3 * t, half), x[3][b]);
    }
    const int t2 = jj << (LOGM - 2 - LOGS);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        mss_r4(x[u][0], x[u][1], x[u][2], x[u][3]);
        if (LOGS > 0) {
            x[u][1] = mss_cmul(mss_tw(wl, t2, half), x[u][1]);
            x[u][2] = mss_cmul(mss_tw(wl, 2 * t2, half), x[u][2]);
            x[u][3] = mss_cmul(mss_tw(wl, 3 * t2, half), x[u][3]);
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) buf[mss_pad(base + (4 * u + v) * s)] = x[u][v];
    }
    __syncthreads();
}
// the 2 G sub-transforms of m = 2^LOGM points in place
template <int LOGM> __device__ __forceinline__ void mss_fft(float2 *buf, const float2 *wl, int tid) {
    if (LOGM == 11) { mss_pass2<11, 10>(buf, wl, tid); mss_pass4<11, 8>(buf, wl, tid); mss_pass16<11, 4>(buf, wl, tid); mss_pass16<11, 0>(buf, wl, tid); }
    if (LOGM == 10) { mss_pass4<10, 8>(buf, wl, tid); mss_pass16<10, 4>(buf, wl, tid); mss_pass16<10, 0>(buf, wl, tid); }
    if (LOGM == 9) { mss_pass2<9, 8>(buf, wl, tid); mss_pass16<9, 4>(buf, wl, tid); mss_pass16<9, 0>(buf, wl, tid); }
    if (LOGM == 8) { mss_pass16<8, 4>(buf, wl, tid); mss_pass16<8, 0>(buf, wl, tid); }
    if (LOGM == 7) { mss_pass2<7, 6>(buf, wl, tid); mss_pass4<7, 4>(buf, wl, tid); mss_pass16<7, 0>(buf, wl, tid); }
}
// where bin k < m of a sub-transform ends up: the radix-2 digit (if any) on top, the base-4 digits of the rest reversed
template <int LOGM> __device__ __forceinline__ int mss_pos(int k) {
    constexpr int bits = LOGM & ~1;
    const unsigned v = (unsigned)(LOGM & 1 ? k >> 1 : k);
    unsigned r = __brev(v) >> (32 - bits);
    r = ((r & 0x55555555u) << 1) | ((r >> 1) & 0x55555555u);
    return (int)r + (LOGM & 1 ? (k & 1) << (LOGM - 1) : 0);
}
// one sample of the analysed signal: x[i] (mix == 0), x[i] + x[i + L] (mix == 1: mid) or x[i] - x[i + L] (mix == 2: side); the sum is
// float32 like the reference's to_mid_side
__device__ __forceinline__ float mss_sample(const float *p, long L, int i, int mix) {
    if (!p) return 0.0f;
    const float a = p[i];
    if (mix == 0) return a;
    const float b = p[L + i];
    return mix == 1 ? a + b : a - b;
}
// |X[k]| of the real transform from Z: m2 = re^2 + im^2 + 1e-7 (FrontEnd.mag's own eps), separate products (no contraction across them)
__device__ __forceinline__ float mss_mag(float re, float im) {
    float a = re * re, b = im * im;
    MST_NO_CONTRACT(a);
    MST_NO_CONTRACT(b);
    return sqrtf(a + b + 1e-7f);
}
// the G frames t0 .. of both signals, reflected at the ends and windowed, into their slots (frame g of est at slot 2 g, of tgt at 2 g + 1;
// a frame beyond T is all zeros); ends with the workgroup's barrier.  The distance and its gradient load through this one function.
template <int LOGM>
__device__ __forceinline__ void mss_load_frames(float2 *buf, const float *pe, const float *pt, int L, int mix, const float *win, int hop, int T,
                                                int t0, int tid) {
    constexpr int m = 1 << LOGM, n = 2 * m, G = MSS_PTS / n;
    float *fb = (float *)buf;
#pragma unroll 4
    for (int e = 0; e < G * n / 256; ++e) {
        const int q = tid + 256 * e, g = q >> (LOGM + 1), r = q & (n - 1), t = t0 + g;
        float ve = 0.0f, vt = 0.0f;
        if (t < T) {
            int i = t * hop - m + r;
            if (i < 0) i = -i;
            if (i >= L) i = 2 * (L - 1) - i;
            const float w = win[r];
            ve = w * mss_sample(pe, L, i, mix);
            vt = w * mss_sample(pt, L, i, mix);
        }
        const int ce = (2 * g) * m + (r >> 1);
        fb[2 * mss_pad(ce) + (r & 1)] = ve;
        fb[2 * mss_pad(ce + m) + (r & 1)] = vt;
    }
    __syncthreads();
}

// grid (groups of G frames, channels, items); 256 threads.
//   est / tgt   base of item 0; item b at + b * item_stride, channel c = blockIdx.y at + c * L when mix_mode == 0 (ori); mix_mode == 1
//               (mid / side) reads channels 0 and 1 and forms L + R (c == 0) or L - R (c == 1).  tgt may be null (EPI_MAG, one channel).
//   win [n], tw [m / 2] = W_m^j, twn [m / 2 + 1] = W_n^k
//   T           frames per (item, channel); frame t covers samples t hop - n / 2 .. + n, reflected at both ends (torch.stft center = True)
//   EPI_TERMS   out_terms[((b * gridDim.y + c) * gridDim.x + group) * 2 + {0, 1}]
//   EPI_MAG     out_mag[((b * n_out + slot) * (n / 2) + k - 1) * T + t], slot 0 = est, 1 = tgt, slots < n_out are stored
template <int LOGM, int EPI>
__global__ __launch_bounds__(256) void mss_frames_kernel(const float *est, const float *tgt, long item_stride, int L, int mix_mode,
                                                         const float *win, const float2 *tw, const float2 *twn, int hop, int T, float eps,
                                                         double *out_terms, float *out_mag, int n_out) {
    constexpr int m = 1 << LOGM, n = 2 * m, G = MSS_PTS / n;
    __shared__ float2 buf[MSS_LDS];
    __shared__ float2 wl[m / 2];
    __shared__ double red[4][2];
    const int tid = threadIdx.x, c = blockIdx.y, t0 = blockIdx.x * G;
    const long ibase = (long)blockIdx.z * item_stride + (mix_mode ? 0 : (long)c * L);
    const float *pe = est + ibase, *pt = tgt ? tgt + ibase : nullptr;
    const int mix = mix_mode ? 1 + c : 0;
    for (int j = tid; j < m / 2; j += 256) wl[j] = tw[j];
    mss_load_frames<LOGM>(buf, pe, pt, L, mix, win, hop, T, t0, tid);
    mss_fft<LOGM>(buf, wl, tid);

    // bins: item idx < 1024 = (frame g, kk < m / 2); kk >= 1: the pair (kk, m - kk); kk == 0: bin m (from Z[0]) and bin m / 2
    double acc_m = 0.0, acc_l = 0.0;
#pragma unroll
    for (int e = 0; e < MSS_PTS / 4 / 256; ++e) {
        const int idx = tid + 256 * e, g = idx >> (LOGM - 1), kk = idx & (m / 2 - 1), t = t0 + g;
        if (t >= T) continue;
        const int k = kk ? kk : m / 2, kc = m - k;
        const int pk = mss_pos<LOGM>(k), pc = mss_pos<LOGM>(kc);
        const float2 w = twn[k];
        float mg[2][2], mlast[2];          // [signal][bin k, bin m - k], bin m
#pragma unroll
        for (int sg = 0; sg < 2; ++sg) {
            const float2 *z = buf;
            const int o = (2 * g + sg) * m;
            const float2 a = z[mss_pad(o + pk)], b = z[mss_pad(o + pc)];
            const float ex = 0.5f * (a.x + b.x), ey = 0.5f * (a.y - b.y), dx = 0.5f * (a.x - b.x), dy = 0.5f * (a.y + b.y);
            const float px = fmaf(w.y, dx, w.x * dy), py = fmaf(w.y, dy, -(w.x * dx));          // -i w D
            mg[sg][0] = mss_mag(ex + px, ey + py);
            mg[sg][1] = mss_mag(ex - px, py - ey);
            mlast[sg] = 0.0f;
            if (kk == 0) {          // bin m = n_fft / 2 comes from Z[0]
                const float2 z0 = z[mss_pad(o)];
                mlast[sg] = mss_mag(z0.x - z0.y, 0.0f);
            }
        }
        if (EPI == MSS_EPI_TERMS) {
#pragma unroll
            for (int h = 0; h < 3; ++h) {
                if (h == 1 && kk == 0) continue;          // k == m - k == m / 2: one bin
                if (h == 2 && kk != 0) continue;          // bin m rides with the kk == 0 item
                const float me = h == 2 ? mlast[0] : mg[0][h], mt = h == 2 ? mlast[1] : mg[1][h];
                const float lg = log10f((me + eps) / (mt + eps));
                acc_m += (double)fabsf(me - mt);
                acc_l += (double)lg * (double)lg;
            }
        } else {
            const int F = m;
#pragma unroll
            for (int sg = 0; sg < 2; ++sg) {
                if (sg >= n_out) continue;
                float *o = out_mag + ((long)blockIdx.z * n_out + sg) * F * T + t;
                o[(long)(k - 1) * T] = mg[sg][0];
                if (kk) o[(long)(kc - 1) * T] = mg[sg][1];
                else o[(long)(m - 1) * T] = mlast[sg];
            }
        }
    }
    if (EPI == MSS_EPI_TERMS) {
        for (int s = 32; s >= 1; s >>= 1) {
            acc_m += __shfl_xor(acc_m, s);
            acc_l += __shfl_xor(acc_l, s);
        }
        if ((tid & 63) == 0) { red[tid >> 6][0] = acc_m; red[tid >> 6][1] = acc_l; }
        __syncthreads();
        if (tid < 2) {
            const double v = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
            out_terms[(((long)blockIdx.z * gridDim.y + c) * gridDim.x + blockIdx.x) * 2 + tid] = v;
        }
    }
}

// terms[((b * n_scales + scale) * 2 + c) * 2 + j] = the sum over the groups of partial[((b * 2 + c) * groups + g) * 2 + j], in group order
__global__ __launch_bounds__(64) void mss_finalize_kernel(const double *partial, double *terms, int B, int groups, int n_scales, int scale) {
    const int i = blockIdx.x * 64 + threadIdx.x;          // (b, c, j)
    if (i >= B * 4) return;
    const int j = i & 1, c = (i >> 1) & 1, b = i >> 2;
    const double *p = partial + ((long)(b * 2 + c) * groups) * 2 + j;
    double s = 0.0;
    for (int g = 0; g < groups; ++g) s += p[2 * g];
    terms[(((long)b * n_scales + scale) * 2 + c) * 2 + j] = s;
}

// ---- the gradient of the two sums with respect to est (mst_mss_backward) -----------------------------------------------------------
// Stage 1 repeats the forward's load, window and transform, turns every bin of est into its cotangent
//     Gamma_k = dm X_k / m_k,   dm = a sgn(m_e - m_t) + b 2 (log10(m_e + eps) - log10(m_t + eps)) / ((m_e + eps) ln 10),
// (a, b the cotangents of the two sums), carries it back through the real-sequence un-mix in place and runs the ADJOINT of the
// transform: the forward is decimation in frequency, natural order in, digit-reversed out; its conjugate transpose is decimation in
// time, digit-reversed in, natural out - the same passes in reverse order, each one "conjugate twiddle, then the conjugate butterfly".
// The windowed time gradient of every frame goes to a workspace [B, 2, T, n]; stage 2 gathers it per sample (no atomics).
__device__ __forceinline__ float2 mss_cmulc(float2 w, float2 a) {          // conj(w) a
    return make_float2(fmaf(w.x, a.x, w.y * a.y), fmaf(w.x, a.y, -(w.y * a.x)));
}
__device__ __forceinline__ void mss_r4_adj(float2 &a0, float2 &a1, float2 &a2, float2 &a3) {
    const float2 s02 = make_float2(a0.x + a2.x, a0.y + a2.y), d02 = make_float2(a0.x - a2.x, a0.y - a2.y);
    const float2 s13 = make_float2(a1.x + a3.x, a1.y + a3.y), d13 = make_float2(a1.x - a3.x, a1.y - a3.y);
    a0 = make_float2(s02.x + s13.x, s02.y + s13.y);
    a1 = make_float2(d02.x - d13.y, d02.y + d13.x);      // d02 + i d13
    a2 = make_float2(s02.x - s13.x, s02.y - s13.y);
    a3 = make_float2(d02.x + d13.y, d02.y - d13.x);      // d02 - i d13
}
template <int LOGM, int LOGS> __device__ __forceinline__ void mss_pass2_adj(float2 *buf, const float2 *wl, int tid) {
#pragma unroll
    for (int e = 0; e < MSS_PTS / 2 / 256; ++e) {
        const int j = tid + 256 * e, jj = j & ((1 << LOGS) - 1), base = ((j >> LOGS) << (LOGS + 1)) + jj;
        const int p0 = mss_pad(base), p1 = mss_pad(base + (1 << LOGS));
        const float2 a = buf[p0], b = mss_cmulc(wl[jj << (LOGM - 1 - LOGS)], buf[p1]);
        buf[p0] = make_float2(a.x + b.x, a.y + b.y);
        buf[p1] = make_float2(a.x - b.x, a.y - b.y);
    }
    __syncthreads();
}
template <int LOGM, int LOGS> __device__ __forceinline__ void mss_pass4_adj(float2 *buf, const float2 *wl, int tid) {
    constexpr int s = 1 << LOGS, half = 1 << (LOGM - 1);
#pragma unroll
    for (int e = 0; e < MSS_PTS / 4 / 256; ++e) {
        const int j = tid + 256 * e, jj = j & (s - 1), base = ((j >> LOGS) << (LOGS + 2)) + jj;
        const int t = jj << (LOGM - 2 - LOGS);
        float2 a0 = buf[mss_pad(base)], a1 = mss_cmulc(mss_tw(wl, t, half), buf[mss_pad(base + s)]);
        float2 a2 = mss_cmulc(mss_tw(wl, 2 * t, half), buf[mss_pad(base + 2 * s)]), a3 = mss_cmulc(mss_tw(wl, 3 * t, half), buf[mss_pad(base + 3 * s)]);
        mss_r4_adj(a0, a1, a2, a3);
        buf[mss_pad(base)] = a0;
        buf[mss_pad(base + s)] = a1;
        buf[mss_pad(base + 2 * s)] = a2;
        buf[mss_pad(base + 3 * s)] = a3;
    }
    __syncthreads();
}
// the adjoint of mss_pass16: the stride-s pass undone first, then the stride-4 s pass, the intermediate in registers
template <int LOGM, int LOGS> __device__ __forceinline__ void mss_pass16_adj(float2 *buf, const float2 *wl, int tid) {
    constexpr int s = 1 << LOGS, half = 1 << (LOGM - 1);
    const int jj = tid & (s - 1), base = ((tid >> LOGS) << (LOGS + 4)) + jj;
    float2 x[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) x[a][b] = buf[mss_pad(base + (4 * a + b) * s)];
    const int t2 = jj << (LOGM - 2 - LOGS);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        if (LOGS > 0) {
            x[u][1] = mss_cmulc(mss_tw(wl, t2, half), x[u][1]);
            x[u][2] = mss_cmulc(mss_tw(wl, 2 * t2, half), x[u][2]);
            x[u][3] = mss_cmulc(mss_tw(wl, 3 * t2, half), x[u][3]);
        }
        mss_r4_adj(x[u][0], x[u][1], x[u][2], x[u][3]);
    }
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const int t = (jj + b * s) << (LOGM - 4 - LOGS);
        x[1][b] = mss_cmulc(mss_tw(wl, t, half), x[1][b]);
        x[2][b] = mss_cmulc(mss_tw(wl, 2 * t, half), x[2][b]);
        x[3][b] = mss_cmulc(mss_tw(wl, 3 * t, half), x[3][b]);
        mss_r4_adj(x[0][b], x[1][b], x[2][b], x[3][b]);
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) buf[mss_pad(base + (4 * a + b) * s)] = x[a][b];
    __syncthreads();
}
// mss_fft's conjugate transpose: the 2 G sub-transforms from digit-reversed to natural order, un-normalised
template <int LOGM> __device__ __forceinline__ void mss_fft_adj(float2 *buf, const float2 *wl, int tid) {
    if (LOGM == 11) { mss_pass16_adj<11, 0>(buf, wl, tid); mss_pass16_adj<11, 4>(buf, wl, tid); mss_pass4_adj<11, 8>(buf, wl, tid); mss_pass2_adj<11, 10>(buf, wl, tid); }
    if (LOGM == 10) { mss_pass16_adj<10, 0>(buf, wl, tid); mss_pass16_adj<10, 4>(buf, wl, tid); mss_pass4_adj<10, 8>(buf, wl, tid); }
    if (LOGM == 9) { mss_pass16_adj<9, 0>(buf, wl, tid); mss_pass16_adj<9, 4>(buf, wl, tid); mss_pass2_adj<9, 8>(buf, wl, tid); }
    if (LOGM == 8) { mss_pass16_adj<8, 0>(buf, wl, tid); mss_pass16_adj<8, 4>(buf, wl, tid); }
    if (LOGM == 7) { mss_pass16_adj<7, 0>(buf, wl, tid); mss_pass4_adj<7, 4>(buf, wl, tid); mss_pass2_adj<7, 6>(buf, wl, tid); }
}
// d (a S0 + b S1) / d m_e of one bin, over m_e: ca = a, cb = b 2 / ln 10, both float32.  sgn(0) = 0 and log10f(1) = 0, so equal
// magnitudes give exactly 0, and so do zero cotangents (every factor is finite: m >= sqrt(1e-7))
__device__ __forceinline__ float mss_grad_scale(float me, float mt, float ca, float cb, float eps) {
    const float d = me - mt, sg = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
    const float lg = log10f((me + eps) / (mt + eps));
    return fmaf(ca, sg, cb * (lg / (me + eps))) / me;
}

// grid (groups of G frames, 2 channels, items) and the arguments of mss_frames_kernel;  dterms [B][n_scales][2][2] float64, the cotangents
// of mst_mss_forward's terms;  frames [B, 2, T, n]: the windowed time gradient of every frame of est's analysis channel c
template <int LOGM>
__global__ __launch_bounds__(256) void mss_grad_frames_kernel(const float *est, const float *tgt, long item_stride, int L, int mix_mode,
                                                              const float *win, const float2 *tw, const float2 *twn, int hop, int T, float eps,
                                                              const double *dterms, int n_scales, int scale, float *frames) {
    constexpr int m = 1 << LOGM, n = 2 * m, G = MSS_PTS / n;
    __shared__ float2 buf[MSS_LDS];
    __shared__ float2 wl[m / 2];
    const int tid = threadIdx.x, c = blockIdx.y, t0 = blockIdx.x * G;
    const long ibase = (long)blockIdx.z * item_stride + (mix_mode ? 0 : (long)c * L);
    const float *pe = est + ibase, *pt = tgt + ibase;
    const int mix = mix_mode ? 1 + c : 0;
    const double *ct = dterms + (((long)blockIdx.z * n_scales + scale) * 2 + c) * 2;
    const float ca = (float)ct[0], cb = (float)ct[1] * 0.868588963806503655f;          // 2 / ln 10
    for (int j = tid; j < m / 2; j += 256) wl[j] = tw[j];
    mss_load_frames<LOGM>(buf, pe, pt, L, mix, win, hop, T, t0, tid);
    mss_fft<LOGM>(buf, wl, tid);

    // the forward's items: (frame g, kk < m / 2) owns bins kk and m - kk (kk == 0: bins m / 2 and m), i.e. positions pk, pc (and 0) of
    // both slots; it reads them and writes est's: no other item touches them
#pragma unroll
    for (int e = 0; e < MSS_PTS / 4 / 256; ++e) {
        const int idx = tid + 256 * e, g = idx >> (LOGM - 1), kk = idx & (m / 2 - 1), t = t0 + g;
        if (t >= T) continue;
        const int k = kk ? kk : m / 2, kc = m - k;
        const int pk = mss_pos<LOGM>(k), pc = mss_pos<LOGM>(kc);
        const float2 w = twn[k];
        float2 X[2][2];                    // [signal][bin k, bin m - k]
        float xl[2] = {0.0f, 0.0f};        // bin m (real)
#pragma unroll
        for (int sg = 0; sg < 2; ++sg) {
            const int o = (2 * g + sg) * m;
            const float2 a = buf[mss_pad(o + pk)], b = buf[mss_pad(o + pc)];
            const float ex = 0.5f * (a.x + b.x), ey = 0.5f * (a.y - b.y), dx = 0.5f * (a.x - b.x), dy = 0.5f * (a.y + b.y);
            const float px = fmaf(w.y, dx, w.x * dy), py = fmaf(w.y, dy, -(w.x * dx));          // -i w D
            X[sg][0] = make_float2(ex + px, ey + py);
            X[sg][1] = make_float2(ex - px, py - ey);
            if (kk == 0) {
                const float2 z0 = buf[mss_pad(o)];
                xl[sg] = z0.x - z0.y;
            }
        }
        const int oe = (2 * g) * m;
        const float s1 = mss_grad_scale(mss_mag(X[0][0].x, X[0][0].y), mss_mag(X[1][0].x, X[1][0].y), ca, cb, eps);
        const float2 g1 = make_float2(s1 * X[0][0].x, s1 * X[0][0].y);
        if (kk) {
            const float s2 = mss_grad_scale(mss_mag(X[0][1].x, X[0][1].y), mss_mag(X[1][1].x, X[1][1].y), ca, cb, eps);
            const float2 g2 = make_float2(s2 * X[0][1].x, s2 * X[0][1].y);
            // X_k = E + P, X_{m-k} = conj(E - P), E = (a + conj b) / 2, P = -i w (a - conj b) / 2: cotangents of E, P, D, then of a and b
            const float2 ge = make_float2(g1.x + g2.x, g1.y - g2.y), gp = make_float2(g1.x - g2.x, g1.y + g2.y);
            const float2 gd = make_float2(fmaf(w.y, gp.x, -(w.x * gp.y)), fmaf(w.y, gp.y, w.x * gp.x));          // conj(-i w) gp
            buf[mss_pad(oe + pk)] = make_float2(0.5f * (ge.x + gd.x), 0.5f * (ge.y + gd.y));
            buf[mss_pad(oe + pc)] = make_float2(0.5f * (ge.x - gd.x), -0.5f * (ge.y - gd.y));
        } else {
            // X_{m/2} = conj(Z_{m/2});  X_m = Re Z_0 - Im Z_0, bin 0 carries no cotangent
            buf[mss_pad(oe + pk)] = make_float2(g1.x, -g1.y);
            const float sl = mss_grad_scale(mss_mag(xl[0], 0.0f), mss_mag(xl[1], 0.0f), ca, cb, eps);
            const float gl = sl * xl[0];
            buf[mss_pad(oe)] = make_float2(gl, -gl);
        }
    }
    __syncthreads();
    mss_fft_adj<LOGM>(buf, wl, tid);

    const float *fb = (const float *)buf;
    float *out = frames + (((long)blockIdx.z * gridDim.y + c) * T) * n;
#pragma unroll 4
    for (int e = 0; e < G * n / 256; ++e) {
        const int q = tid + 256 * e, g = q >> (LOGM + 1), r = q & (n - 1), t = t0 + g;
        if (t < T) out[(long)t * n + r] = win[r] * fb[2 * mss_pad((2 * g) * m + (r >> 1)) + (r & 1)];
    }
}

// grid (ceil(L / 256), items); one thread per sample pair.  Padded index q = t hop + j - n / 2 folds onto sample i by the forward's
// reflection: i collects q = i, q = -i (1 <= i <= n / 2) and q = 2 (L - 1) - i (L - 1 - n / 2 <= i <= L - 2), each from the frames that
// cover it, in ascending frame order; then the analysis channels are un-mixed.  accumulate == 0 stores, else adds to what is there.
__global__ __launch_bounds__(256) void mss_grad_gather_kernel(const float *frames, float *grad, int L, int n, int hop, int T, int mix_mode,
                                                              int accumulate) {
    const int i = blockIdx.x * 256 + threadIdx.x, m = n / 2;
    if (i >= L) return;
    float acc[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float *f = frames + (((long)blockIdx.y * 2 + c) * T) * n;
        float s = 0.0f;
        for (int p = 0; p < 3; ++p) {
            if (p == 1 && (i < 1 || i > m)) continue;
            if (p == 2 && (i > L - 2 || i < L - 1 - m)) continue;
            const int u = (p == 0 ? i : p == 1 ? -i : 2 * (L - 1) - i) + m;          // position of q in the padded signal, >= 0
            const int t_lo = u >= n ? (u - n) / hop + 1 : 0, t_hi = u / hop < T ? u / hop : T - 1;
            for (int t = t_lo; t <= t_hi; ++t) s += f[(long)t * n + (u - t * hop)];
        }
        acc[c] = s;
    }
    float *gl = grad + (long)blockIdx.y * 2 * L + i, *gr = gl + L;
    float vl = mix_mode ? acc[0] + acc[1] : acc[0], vr = mix_mode ? acc[0] - acc[1] : acc[1];
    if (accumulate) { vl = *gl + vl; vr = *gr + vr; }
    *gl = vl;
    *gr = vr;
}
#pragma clang fp contract(on)          // the compiler's default for the rest of the translation unit
