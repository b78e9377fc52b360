// Mixing-feature metrics (reference mixing_manipulator/utils_data_normalization.py: get_SPS :109-139, get_panning_rms :682-703,
// get_rms_dynamic_crest :777-811, get_low_freq_weighting :823-846): the per-frame work of the panning, dynamics and low-frequency
// figures, fused so that no spectrum and no per-bin value goes to HBM.
//
// mixfeat_frames_kernel.  The transform is csrc/mss_kernels.h's (mss_fft, mss_pos, the skewed LDS layout, the LDS twiddle table): a
// workgroup owns G = 4096 / n_fft consecutive frames of one item, slot 2 g holds frame g of signal A, slot 2 g + 1 of signal B - the left
// and the right channel (panning) or one channel of the low-passed signal and of the signal itself (low ratio).  Both slots run the same
// instructions on the same twiddles, so A == B gives the same bits in both: a mono frame, or a frame of digital silence, has l == r in
// every bin and leaves exactly 0.  What differs from the spectral distance: librosa.stft(center = False) framing (frame t covers samples
// t hop .. t hop + n_fft - 1, nothing is reflected), the FX layout [n_items][L][C] (time-major, interleaved), a per-item factor folded into
// the load (pyloudnorm.normalize.peak), the window sqrt(hanning(n_fft + 1)[:-1]), all n_fft / 2 + 1 bins (bin 0 from Z[0] too), plain
// magnitudes sqrt(re^2 + im^2), and the epilogues.
//
// Sums.  A thread's bins go through float64 arithmetic and into float64 accumulators in a fixed order; the 64 items of a wave are one
// chunk, reduced by xor-shuffles into LDS; a frame's value is the sum of its chunks in chunk order.  No atomics: a frame's numbers do not
// depend on the run or on what else is in the batch.
//
// mixfeat_dynamics_kernel.  Frames of get_rms_dynamic_crest overlap frame / hop times, and a sample is reduced once: when hop divides
// the frame length a workgroup reduces MIXFEAT_DYN_BLOCKS hop blocks - sum x^2, sum 20 log10(|x| + 1e-30), max |x| per block and channel -
// and a frame is its frame / hop blocks combined in block order (only the frame / hop - 1 blocks two workgroups share are read twice);
// otherwise a block is a whole frame.
#pragma once
#include "mss_kernels.h"

#define MIXFEAT_EPI_PANNING 0
#define MIXFEAT_EPI_PANNING_STORE 1
#define MIXFEAT_EPI_LOW_RATIO 2
#define MIXFEAT_MAX_BANDS 8
#define MIXFEAT_DYN_BLOCKS 64

struct MixfeatBands {          // [lo, hi) in bins, from the host (get_panning_rms_frame's floor(f n_fft / sr))
    int n;
    int lo[MIXFEAT_MAX_BANDS], hi[MIXFEAT_MAX_BANDS];
};

// as in mss_kernels.h: the slots are handled by different unrolled copies of the same statements; no contraction the compiler may choose
#pragma clang fp contract(off)
// |re + i im|, separate products
__device__ __forceinline__ float mixfeat_mag(float re, float im) {
    float a = re * re, b = im * im;
    MST_NO_CONTRACT(a);
    MST_NO_CONTRACT(b);
    return sqrtf(a + b);
}
// get_SPS :122-128 from the two magnitudes: phi = 2 l r / (l^2 + r^2), SPS = (1 - phi) sign(r - l); l == r == 0 is l == r: phi = 1
__device__ __forceinline__ void mixfeat_sps(float l, float r, double &phi, double &sps) {
    const double ld = (double)l, rd = (double)r, den = ld * ld + rd * rd;
    phi = den > 0.0 ? 2.0 * ld * rd / den : 1.0;
    sps = r > l ? 1.0 - phi : (r < l ? phi - 1.0 : 0.0);
}

// grid (groups of G frames, channels, items); 256 threads.
//   xa / xb     base of signal A / B of item 0 and the first channel of the grid: item b at + b * item_stride, the grid's channel y at + y,
//               sample i at + i * C (EPI_PANNING*: gridDim.y == 1, xb = xa + 1; EPI_LOW_RATIO: xa the low-passed signal, xb the signal)
//   scale_a / b per-item factor of the load, x * s rounded to float32 before the window (NumPy's float32 array times a scalar); null: 1
//   win [n], tw [m / 2] = W_m^j, twn [m / 2 + 1] = W_n^k;  T = 1 + (L - n) / hop frames, all inside the signal
//   EPI_PANNING        out_sum[((b * T) + t) * bands.n + j] = sum over bins [lo_j, hi_j) of SPS^2
//   EPI_PANNING_STORE  out_phi / out_sps[((b * T) + t) * (m + 1) + k]
//   EPI_LOW_RATIO      out_sum[(b * gridDim.y + y) * T + t] = sum over all m + 1 bins of A_k / (B_k + 1e-5)
template <int LOGM, int EPI>
__global__ __launch_bounds__(256) void mixfeat_frames_kernel(const float *xa, const float *xb, long item_stride, int C, const float *scale_a,
                                                             const float *scale_b, const float *win, const float2 *tw, const float2 *twn,
                                                             int hop, int T, MixfeatBands bands, double *out_sum, float *out_phi,
                                                             float *out_sps) {
    constexpr int m = 1 << LOGM, n = 2 * m, G = MSS_PTS / n, NB = EPI == MIXFEAT_EPI_PANNING ? MIXFEAT_MAX_BANDS : 1;
    constexpr int CHUNKS = MSS_PTS / 4 / 64, CPF = CHUNKS / G;          // chunks of 64 items; per frame
    __shared__ float2 buf[MSS_LDS];
    __shared__ float2 wl[m / 2];
    __shared__ double part[CHUNKS][NB];
    const int tid = threadIdx.x, t0 = blockIdx.x * G;
    const long ibase = (long)blockIdx.z * item_stride + blockIdx.y;
    const float *pa = xa + ibase, *pb = xb + ibase;
    const float sa = scale_a ? scale_a[blockIdx.z] : 1.0f, sb = scale_b ? scale_b[blockIdx.z] : 1.0f;
    for (int j = tid; j < m / 2; j += 256) wl[j] = tw[j];
    float *fb = (float *)buf;
#pragma unroll 4
    for (int e = 0; e < G * n / 256; ++e) {
        const int q = tid + 256 * e, g = q >> (LOGM + 1), r = q & (n - 1), t = t0 + g;
        float va = 0.0f, vb = 0.0f;
        if (t < T) {
            const long i = ((long)t * hop + r) * C;
            const float w = win[r];
            va = w * (pa[i] * sa);
            vb = w * (pb[i] * sb);
        }
        const int ce = (2 * g) * m + (r >> 1);
        fb[2 * mss_pad(ce) + (r & 1)] = va;
        fb[2 * mss_pad(ce + m) + (r & 1)] = vb;
    }
    __syncthreads();
    mss_fft<LOGM>(buf, wl, tid);

    // items idx < 1024 = (frame g, kk < m / 2); kk >= 1: the bins kk and m - kk; kk == 0: bin m / 2, bin m and bin 0 (both from Z[0])
#pragma unroll
    for (int e = 0; e < MSS_PTS / 4 / 256; ++e) {
        const int idx = tid + 256 * e, g = idx >> (LOGM - 1), kk = idx & (m / 2 - 1), t = t0 + g;
        double acc[NB];
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[j] = 0.0;
        if (t < T) {
            const int k = kk ? kk : m / 2, kc = m - k;
            const int pk = mss_pos<LOGM>(k), pc = mss_pos<LOGM>(kc);
            const float2 w = twn[k];
            float mg[2][4];          // [signal][bin k, bin m - k, bin m, bin 0]
#pragma unroll
            for (int sg = 0; sg < 2; ++sg) {
                const int o = (2 * g + sg) * m;
                const float2 a = buf[mss_pad(o + pk)], b = buf[mss_pad(o + pc)];
                const float ex = 0.5f * (a.x + b.x), ey = 0.5f * (a.y - b.y), dx = 0.5f * (a.x - b.x), dy = 0.5f * (a.y + b.y);
                const float px = fmaf(w.y, dx, w.x * dy), py = fmaf(w.y, dy, -(w.x * dx));          // -i w D
                // EPI_PANNING*: |X + 1e-20| like get_SPS :119-120 (complex64 plus a real number)
                const float tiny = EPI == MIXFEAT_EPI_LOW_RATIO ? 0.0f : 1e-20f;
                mg[sg][0] = mixfeat_mag(ex + px + tiny, ey + py);
                mg[sg][1] = mixfeat_mag(ex - px + tiny, py - ey);
                mg[sg][2] = mg[sg][3] = 0.0f;
                if (kk == 0) {
                    const float2 z0 = buf[mss_pad(o)];
                    mg[sg][2] = mixfeat_mag(z0.x - z0.y + tiny, 0.0f);
                    mg[sg][3] = mixfeat_mag(z0.x + z0.y + tiny, 0.0f);
                }
            }
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                if (h == 1 && kk == 0) continue;          // k == m - k == m / 2: one bin
                if (h >= 2 && kk != 0) continue;          // bins m and 0 ride with the kk == 0 item
                const int bin = h == 0 ? k : (h == 1 ? kc : (h == 2 ? m : 0));
                if (EPI == MIXFEAT_EPI_LOW_RATIO) {
                    acc[0] += (double)mg[0][h] / ((double)mg[1][h] + 1e-5);
                } else {
                    double phi, sps;
                    mixfeat_sps(mg[0][h], mg[1][h], phi, sps);
                    if (EPI == MIXFEAT_EPI_PANNING) {
                        const double s2 = sps * sps;
#pragma unroll
                        for (int j = 0; j < NB; ++j)
                            if (j < bands.n && bin >= bands.lo[j] && bin < bands.hi[j]) acc[j] += s2;
                    } else {
                        const long o = ((long)blockIdx.z * T + t) * (m + 1) + bin;
                        out_phi[o] = (float)phi;
                        out_sps[o] = (float)sps;
                    }
                }
            }
        }
        if (EPI != MIXFEAT_EPI_PANNING_STORE) {
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                if (j >= bands.n) continue;          // uniform
                double v = acc[j];
                for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
                if ((tid & 63) == 0) part[idx >> 6][j] = v;
            }
        }
    }
    if (EPI != MIXFEAT_EPI_PANNING_STORE) {
        __syncthreads();
        const int nb = bands.n;
        if (tid < G * nb) {
            const int g = tid / nb, j = tid - g * nb, t = t0 + g;
            if (t < T) {
                double s = 0.0;
                for (int c = 0; c < CPF; ++c) s += part[g * CPF + c][j];
                out_sum[(((long)blockIdx.z * gridDim.y + blockIdx.y) * T + t) * nb + j] = s;
            }
        }
    }
}

// grid (groups of frames, 1, items); 256 threads; C = 1 or 2.  A workgroup reduces nblk <= MIXFEAT_DYN_BLOCKS blocks of `blk` samples
// (all channels), block j starting at sample (t0 + j) hop, and leaves fpw = nblk - R + 1 frames, frame f = blocks f .. f + R - 1
// (R = frame / hop and blk = hop when hop divides the frame, R = 1 and blk = frame otherwise).  A block is read as blk * C consecutive
// floats by one wave, lane l taking the elements l, l + 64, ..: with C = 2 a lane stays on one channel (l & 1), and the xor-shuffles stop
// above 1.  x * scale is rounded to float32 (see above), everything after it is float64.
//   out[((b * C + c) * T + t) * 3 + {0, 1, 2}] = sum x^2, sum 20 log10(|x| + 1e-30), max |x|
__global__ __launch_bounds__(256) void mixfeat_dynamics_kernel(const float *x, long item_stride, int C, const float *scale, int blk, int hop,
                                                               int R, int fpw, int T, double *out) {
    __shared__ double part[MIXFEAT_DYN_BLOCKS][2][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, t0 = blockIdx.x * fpw;
    const int nfr = T - t0 < fpw ? T - t0 : fpw, nblk = nfr + R - 1;
    const float *p = x + (long)blockIdx.z * item_stride;
    const float s = scale ? scale[blockIdx.z] : 1.0f;
    for (int j = wave; j < nblk; j += 4) {
        const float *q = p + (long)(t0 + j) * hop * C;
        double s2 = 0.0, lg = 0.0, mx = 0.0;
        for (int e = lane; e < blk * C; e += 64) {
            const double a = (double)fabsf(q[e] * s);
            s2 += a * a;
            lg += 20.0 * log10(a + 1e-30);
            mx = fmax(mx, a);
        }
        for (int d = 32; d >= C; d >>= 1) {
            s2 += __shfl_xor(s2, d);
            lg += __shfl_xor(lg, d);
            mx = fmax(mx, __shfl_xor(mx, d));
        }
        if (lane < C) { part[j][lane][0] = s2; part[j][lane][1] = lg; part[j][lane][2] = mx; }
    }
    __syncthreads();
    if (tid < nfr * C) {
        const int f = tid / C, c = tid - f * C;
        double s2 = 0.0, lg = 0.0, mx = 0.0;
        for (int r = 0; r < R; ++r) {
            s2 += part[f + r][c][0];
            lg += part[f + r][c][1];
            mx = fmax(mx, part[f + r][c][2]);
        }
        double *o = out + (((long)blockIdx.z * C + c) * T + t0 + f) * 3;
        o[0] = s2;
        o[1] = lg;
        o[2] = mx;
    }
}
// The spectral epilogue (the issue's MIXFEAT_EPI_SPECTRAL, a kernel of its own): the per-frame work of librosa.feature.spectral_centroid / _bandwidth / _rolloff / _flatness / _contrast
// (reference compute_spectral_features :509-679).  A sibling of mixfeat_frames_kernel - same load phase, same transform, the magnitudes
// without the 1e-20 term - because its epilogue is of another kind: a centroid needs the frame's total before the second moment, the
// roll-off a prefix sum over the bins in natural order, the contrast order statistics inside bands.  After the un-mix every thread
// holds its magnitudes in registers, `buf` is free, and the 2 G spectra (G frames x the two channels of an item) go back into it in
// natural bin order, m + 1 floats each (an odd stride: slots of one wave sit on different banks).  From there on, per slot:
//   sums       TPS = 256 / (2 G) threads; thread j adds the bins j, j + TPS, .. in float64 (consecutive lanes read consecutive words),
//              xor-shuffles inside the wave, chunks in chunk order through LDS: sum S, sum k S, sum log P, sum P (P = max(1e-10, S^2));
//              then, with c = sum k S / sum S known to every thread, sum S (k - c)^2 the same way - NOT sum k^2 S - c^2 sum S, which
//              cancels on a narrow-band frame
//   roll-off   thread j owns the 17 consecutive bins from 17 j on (stride 17: conflict-free): segment sum, inclusive scan over the slot's
//              threads (__shfl_up steps, the first wave's total through LDS when a slot spans two waves), then a walk over its own bins;
//              the answer is the smallest k whose cumulative sum reaches 0.85 sum S (a silent frame: 0 >= 0 at k = 0)
//   contrast   the sum of the k smallest and of the k largest magnitudes of each band [lo, hi).  Non-negative floats order like their
//              bit patterns, so the k-th smallest value is the largest pattern v with #{x < v} < k and the k-th largest the largest v
//              with #{x >= v} >= k: both are built bit by bit from the top, 31 counting passes over the band, shared by the two.  A
//              (slot, band) task belongs to a group of SW = n_fft / 64 lanes of ONE wave and the band sits in the lanes' registers, so
//              a pass is compares and an integer xor-shuffle sum: no LDS word, no barrier, no atomic.  The sum is then the values strictly beyond the threshold, in thread
//              order, plus (k - their count) times the threshold: every tie is counted once.  Tasks are dealt from the top band down,
//              so the long bands of the slots start on different groups.
// A frame of digital silence gives 0 in slots 0 .. 3 and 6 .. 15.  The kernel works in bins; the host turns bins into Hz.
//   grid (groups of G frames, 1, items); x [n_items][L][C]: slot 2 g is channel 0, slot 2 g + 1 channel 1 of frame t0 + g (C == 1: the
//   same channel again, not stored);  out[((b * C + c) * T + t) * 16 + q], q as in include/mst_hip.h
#define MIXFEAT_SPEC_OUT 16
#define MIXFEAT_SPEC_BANDS ((MIXFEAT_SPEC_OUT - 6) / 2)          // bands whose two sums fit behind the six frame sums
struct MixfeatSelBands {          // bins [lo, hi) and the count k of each band, 1 <= k <= hi - lo, from the host; n <= MIXFEAT_SPEC_BANDS
    int n;
    int lo[MIXFEAT_SPEC_BANDS], hi[MIXFEAT_SPEC_BANDS], k[MIXFEAT_SPEC_BANDS];
};

// The sum of the kq smallest and of the kq largest of mq[lo .. hi) by a group of SW lanes of one wave (lane gl of it); NE * SW >= hi - lo.
// A lane's values sit in NE registers as bit patterns (past the band: all ones, above every candidate); 31 passes build both thresholds
// from the top bit, each a count of the registers below two candidates and one integer xor-shuffle sum.  Every lane of the wave calls it.
template <int NE, int SW>
__device__ __forceinline__ void mixfeat_select(const float *mq, int lo, int hi, int kq, int gl, double &lsum, double &hsum) {
    unsigned v[NE];
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        const int k = lo + gl + i * SW;
        v[i] = k < hi ? __builtin_bit_cast(unsigned, mq[k]) : 0xffffffffu;
    }
    unsigned vs = 0u, vl = 0u;          // the kq-th smallest / the kq-th largest pattern
    for (int bit = 30; bit >= 0; --bit) {
        const unsigned cs = vs | (1u << bit), cg = vl | (1u << bit);
        int cnt = 0;          // #{x < cs} + 2^16 #{x < cg}: a band has at most 2049 bins
#pragma unroll
        for (int i = 0; i < NE; ++i) cnt += (v[i] < cs ? 1 : 0) + (v[i] < cg ? 0x10000 : 0);
        for (int s = SW / 2; s >= 1; s >>= 1) cnt += __shfl_xor(cnt, s);
        if ((cnt & 0xffff) < kq) vs = cs;
        if (hi - lo - (cnt >> 16) >= kq) vl = cg;
    }
    double ls = 0.0, hs = 0.0;
    int ln = 0, hn = 0;
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        const double x = (double)__builtin_bit_cast(float, v[i]);
        if (v[i] < vs) { ls += x; ++ln; }
        if (v[i] > vl && v[i] != 0xffffffffu) { hs += x; ++hn; }
    }
    for (int s = SW / 2; s >= 1; s >>= 1) {
        ls += __shfl_xor(ls, s);
        hs += __shfl_xor(hs, s);
        ln += __shfl_xor(ln, s);
        hn += __shfl_xor(hn, s);
    }
    lsum = ls + (double)(kq - ln) * (double)__builtin_bit_cast(float, vs);          // ties at the threshold: as many as are missing
    hsum = hs + (double)(kq - hn) * (double)__builtin_bit_cast(float, vl);
}

template <int LOGM>
__global__ __launch_bounds__(256) void mixfeat_spectral_kernel(const float *x, long item_stride, int C, const float *scale, const float *win,
                                                               const float2 *tw, const float2 *twn, int hop, int T, MixfeatSelBands bands,
                                                               double *out) {
    constexpr int m = 1 << LOGM, n = 2 * m, G = MSS_PTS / n, NS = 2 * G, TPS = 256 / NS;
    constexpr int CW = TPS < 64 ? TPS : 64, CPS = TPS / CW, NCH = 256 / CW;          // lanes of a chunk, chunks per slot, chunks
    constexpr int SEG = 17, NSV = (m + TPS) / TPS, SW = 64 >> (11 - LOGM), NG = 256 / SW;          // roll-off segment, strided bins; lanes and number of select groups
    static_assert(TPS * SEG >= m + 1 && NS * (m + 1) <= 2 * MSS_LDS, "the spectra must fit buf, the segments a spectrum");
    __shared__ float2 buf[MSS_LDS];
    __shared__ float2 wl[m / 2];
    __shared__ double part[NCH][5];
    __shared__ double wtot[4];
    __shared__ int rpart[NCH];
    __shared__ int sb[3][MIXFEAT_SPEC_BANDS];
    const int tid = threadIdx.x, t0 = blockIdx.x * G;
    const float *pa = x + (long)blockIdx.z * item_stride, *pb = pa + (C == 2 ? 1 : 0);
    const float sa = scale ? scale[blockIdx.z] : 1.0f;
    for (int j = tid; j < m / 2; j += 256) wl[j] = tw[j];
#pragma unroll
    for (int j = 0; j < MIXFEAT_SPEC_BANDS; ++j)
        if (tid == j) { sb[0][j] = bands.lo[j]; sb[1][j] = bands.hi[j]; sb[2][j] = bands.k[j]; }
    float *fb = (float *)buf;
#pragma unroll 4
    for (int e = 0; e < G * n / 256; ++e) {
        const int q = tid + 256 * e, g = q >> (LOGM + 1), r = q & (n - 1), t = t0 + g;
        float va = 0.0f, vb = 0.0f;
        if (t < T) {
            const long i = ((long)t * hop + r) * C;
            const float w = win[r];
            va = w * (pa[i] * sa);
            vb = w * (pb[i] * sa);
        }
        const int ce = (2 * g) * m + (r >> 1);
        fb[2 * mss_pad(ce) + (r & 1)] = va;
        fb[2 * mss_pad(ce + m) + (r & 1)] = vb;
    }
    __syncthreads();
    mss_fft<LOGM>(buf, wl, tid);

    // the un-mix of mixfeat_frames_kernel, all of a thread's magnitudes kept: [item of the thread][signal][bin k, bin m - k, bin m, bin 0]
    float mg[MSS_PTS / 4 / 256][2][4];
#pragma unroll
    for (int e = 0; e < MSS_PTS / 4 / 256; ++e) {
        const int idx = tid + 256 * e, g = idx >> (LOGM - 1), kk = idx & (m / 2 - 1);
        const int k = kk ? kk : m / 2, kc = m - k;
        const int pk = mss_pos<LOGM>(k), pc = mss_pos<LOGM>(kc);
        const float2 w = twn[k];
#pragma unroll
        for (int sg = 0; sg < 2; ++sg) {
            const int o = (2 * g + sg) * m;
            const float2 a = buf[mss_pad(o + pk)], b = buf[mss_pad(o + pc)];
            const float ex = 0.5f * (a.x + b.x), ey = 0.5f * (a.y - b.y), dx = 0.5f * (a.x - b.x), dy = 0.5f * (a.y + b.y);
            const float px = fmaf(w.y, dx, w.x * dy), py = fmaf(w.y, dy, -(w.x * dx));          // -i w D
            mg[e][sg][0] = mixfeat_mag(ex + px, ey + py);
            mg[e][sg][1] = mixfeat_mag(ex - px, py - ey);
            mg[e][sg][2] = mg[e][sg][3] = 0.0f;
            if (kk == 0) {
                const float2 z0 = buf[mss_pad(o)];
                mg[e][sg][2] = mixfeat_mag(z0.x - z0.y, 0.0f);
                mg[e][sg][3] = mixfeat_mag(z0.x + z0.y, 0.0f);
            }
        }
    }
    __syncthreads();          // every thread holds its magnitudes: buf is free
#pragma unroll
    for (int e = 0; e < MSS_PTS / 4 / 256; ++e) {
        const int idx = tid + 256 * e, g = idx >> (LOGM - 1), kk = idx & (m / 2 - 1);
        const int k = kk ? kk : m / 2;
#pragma unroll
        for (int sg = 0; sg < 2; ++sg) {
            float *ms = fb + (2 * g + sg) * (m + 1);
            ms[k] = mg[e][sg][0];
            if (kk) {
                ms[m - k] = mg[e][sg][1];
            } else {
                ms[m] = mg[e][sg][2];
                ms[0] = mg[e][sg][3];
            }
        }
    }
    __syncthreads();

    const int slot = tid / TPS, j = tid & (TPS - 1), cl = tid & (CW - 1), chunk = tid / CW;
    const float *ms = fb + slot * (m + 1);
    // a thread's bins come out of LDS once, into registers: NSV strided ones for the sums, SEG consecutive ones for the roll-off (a loop that
    // waits for every LDS word it compares costs the LDS latency per bin; bins past m are 0 and add nothing)
    float sv[NSV], cv[SEG];
#pragma unroll
    for (int i = 0; i < NSV; ++i) sv[i] = j + i * TPS <= m ? ms[j + i * TPS] : 0.0f;
    const int k0 = j * SEG;
#pragma unroll
    for (int i = 0; i < SEG; ++i) cv[i] = k0 + i <= m ? ms[k0 + i] : 0.0f;
    {          // sum S, sum k S, sum log P, sum P
        double a0 = 0.0, a1 = 0.0, a4 = 0.0, a5 = 0.0;
#pragma unroll
        for (int i = 0; i < NSV; ++i) {
            const int k = j + i * TPS;
            if (k <= m) {
                const double s = (double)sv[i], p = fmax(1e-10, s * s);
                a0 += s;
                a1 += (double)k * s;
                a4 += log(p);
                a5 += p;
            }
        }
        for (int s = CW / 2; s >= 1; s >>= 1) {
            a0 += __shfl_xor(a0, s);
            a1 += __shfl_xor(a1, s);
            a4 += __shfl_xor(a4, s);
            a5 += __shfl_xor(a5, s);
        }
        if (cl == 0) { part[chunk][0] = a0; part[chunk][1] = a1; part[chunk][3] = a4; part[chunk][4] = a5; }
    }
    // the roll-off's scan does not need the total: segment sums and their inclusive scan over the slot's threads
    double inc = 0.0;
#pragma unroll
    for (int i = 0; i < SEG; ++i) inc += (double)cv[i];
    for (int d = 1; d < CW; d <<= 1) {
        const double v = __shfl_up(inc, d);
        if (cl >= d) inc += v;
    }
    double cum = __shfl_up(inc, 1);          // exclusive: what lies below the thread's first bin
    if (cl == 0) cum = 0.0;
    if ((tid & 63) == 63) wtot[tid >> 6] = inc;
    __syncthreads();
    double s0 = 0.0, s1 = 0.0;
    for (int c = 0; c < CPS; ++c) {
        s0 += part[slot * CPS + c][0];
        s1 += part[slot * CPS + c][1];
    }
    if (CPS == 2 && (chunk & 1)) cum += wtot[chunk - 1];
    {          // sum S (k - c)^2 and the first bin whose cumulative sum reaches 0.85 sum S
        const double cb = s0 > 0.0 ? s1 / s0 : 0.0, thr = 0.85 * s0;
        double a2 = 0.0;
#pragma unroll
        for (int i = 0; i < NSV; ++i) {
            const double d = (double)(j + i * TPS) - cb;
            a2 += (double)sv[i] * (d * d);
        }
        int first = m;
#pragma unroll
        for (int i = 0; i < SEG; ++i) {
            cum += (double)cv[i];
            if (k0 + i <= m && cum >= thr && k0 + i < first) first = k0 + i;
        }
        for (int s = CW / 2; s >= 1; s >>= 1) {
            a2 += __shfl_xor(a2, s);
            const int o = __shfl_xor(first, s);
            first = o < first ? o : first;
        }
        if (cl == 0) { part[chunk][2] = a2; rpart[chunk] = first; }
    }

    // contrast: (slot, band) tasks, one per group of SW lanes and round, the top band first.  NG = 2 NS, so a round is two bands over all
    // slots: the longer of the two decides - for the whole workgroup - how many registers per lane the round's values take
    const int nb = bands.n, ntask = NS * nb, gl = tid & (SW - 1);
    for (int q0 = 0; q0 < ntask; q0 += NG) {          // uniform: every lane of a wave takes every shuffle
        const int q = q0 + tid / SW;
        const bool live = q < ntask;
        const int bj = live ? nb - 1 - q / NS : 0, sl = q & (NS - 1);
        const int lo = live ? sb[0][bj] : 0, hi = live ? sb[1][bj] : 0, kq = live ? sb[2][bj] : 1;
        const int b1 = nb - 1 - q0 / NS, b2 = b1 > 0 ? b1 - 1 : b1;
        const int len1 = sb[1][b1] - sb[0][b1], len2 = sb[1][b2] - sb[0][b2], longest = len1 > len2 ? len1 : len2;
        double lsum, hsum;
        if (longest <= 4 * SW) mixfeat_select<4, SW>(fb + sl * (m + 1), lo, hi, kq, gl, lsum, hsum);
        else mixfeat_select<(m + SW) / SW, SW>(fb + sl * (m + 1), lo, hi, kq, gl, lsum, hsum);
        const int t = t0 + (sl >> 1), c = sl & 1;
        if (live && gl == 0 && t < T && c < C) {
            double *o = out + (((long)blockIdx.z * C + c) * T + t) * MIXFEAT_SPEC_OUT + 6 + 2 * bj;
            o[0] = lsum;
            o[1] = hsum;
        }
    }
    __syncthreads();
    if (j == 0) {
        const int t = t0 + (slot >> 1), c = slot & 1;
        if (t < T && c < C) {
            double s2 = 0.0, s4 = 0.0, s5 = 0.0;
            int first = m;
            for (int cc = 0; cc < CPS; ++cc) {
                const int ch = slot * CPS + cc;
                s2 += part[ch][2];
                s4 += part[ch][3];
                s5 += part[ch][4];
                first = rpart[ch] < first ? rpart[ch] : first;
            }
            double *o = out + (((long)blockIdx.z * C + c) * T + t) * MIXFEAT_SPEC_OUT;
            o[0] = s0;
            o[1] = s1;
            o[2] = s2;
            o[3] = (double)first;
            o[4] = s4;
            o[5] = s5;
        }
    }
}
#pragma clang fp contract(on)          // the compiler's default for the rest of the translation unit
