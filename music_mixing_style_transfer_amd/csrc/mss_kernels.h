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
#pragma clang fp contract(on)          // the compiler's default for the rest of the translation unit
