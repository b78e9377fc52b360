// Training batches on the device (data_loader/data_loader.py: the MUSDB datasets): the two streaming kernels around the per-item FX launches.
//
// batch_gather_pcm_kernel.  Row r of out [n][frames][2] (float32, time-major: the FX layout) = frames table[r] .. table[r] + frames - 1 of a
// bank of interleaved stereo PCM (16- or 32-bit, many files back to back).  Arithmetic of loader_utils.load_wav_device: int / 2^(8 width - 1)
// in float64 (exact), rounded once to float32.  Rows may repeat and overlap; an offset has no alignment beyond one frame (4 or 8 bytes).
//
// batch_finish_kernel.  out[r][c][t] = clamp(x[rows[r]][start[r] + t][c], -1, 1): the crop of the over-read, the collate's per-item crop, the
// transpose to channel-major and torch.clamp in one pass (compare-and-select: NaN stays NaN, -0.0 stays -0.0).
//
// Both are pure streaming kernels, aligned on their OUTPUT: a row's address decides a scalar head (up to the next 16-byte boundary), the
// body is one 16-byte store per lane and group of four floats (lane i at base + 16 i: 1 KiB per wave instruction), a scalar tail ends the row.
// The loads of the body are 16 bytes per lane too, at the alignment the source happens to have (4 or 8 bytes: one global_load_dwordx4,
// which needs dword alignment only).  Heads and tails are block 0's.  The host checks every range before the launch (mst_fx.hip); nothing
// here reads or writes outside [table[r], table[r] + frames) / [start[r], start[r] + len) of its row.
#pragma once
#include "mst_dev.h"

#define BATCH_THREADS 256
#define BATCH_GROUPS_PER_BLOCK 1024          // groups of four floats (finish) / four frames (gather) per workgroup: four per lane

typedef unsigned batch_u32x4 __attribute__((ext_vector_type(4), aligned(4)));      // 16 bytes at dword alignment
typedef float batch_f32x4_any __attribute__((ext_vector_type(4), aligned(4)));
typedef float batch_f32x4 __attribute__((ext_vector_type(4)));                     // 16-byte aligned

template <int W> __device__ __forceinline__ float batch_pcm_value(int v) {
    return (float)((double)v / (W == 2 ? 32768.0 : 2147483648.0));
}
// one frame, scalar: two samples -> two floats
template <int W> __device__ __forceinline__ void batch_gather_frame(const unsigned char *src, float *o, long f) {
    if (W == 2) {
        const short *s = (const short *)src + 2 * f;
        o[2 * f] = batch_pcm_value<2>(s[0]);
        o[2 * f + 1] = batch_pcm_value<2>(s[1]);
    } else {
        const int *s = (const int *)src + 2 * f;
        o[2 * f] = batch_pcm_value<4>(s[0]);
        o[2 * f + 1] = batch_pcm_value<4>(s[1]);
    }
}

// grid (ceil(groups / BATCH_GROUPS_PER_BLOCK) or 1, n); BATCH_THREADS threads.  W: bytes per sample (2 or 4); out 8-byte aligned (host check)
template <int W>
__global__ __launch_bounds__(BATCH_THREADS) void batch_gather_pcm_kernel(const unsigned char *bank, const long *table, float *out, long frames) {
    const int tid = threadIdx.x;
    const long r = blockIdx.y;
    const unsigned char *src = bank + table[r] * (2 * W);
    float *o = out + r * frames * 2;
    const long head = ((uintptr_t)o & 15) ? (frames < 1 ? frames : 1) : 0;       // a row is 8-byte aligned: one frame reaches the 16-byte boundary
    const long nbody = (frames - head) / 4;                                        // groups of four frames = two 16-byte stores
    const long g1 = nbody < ((long)blockIdx.x + 1) * BATCH_GROUPS_PER_BLOCK ? nbody : ((long)blockIdx.x + 1) * BATCH_GROUPS_PER_BLOCK;
    for (long g = (long)blockIdx.x * BATCH_GROUPS_PER_BLOCK + tid; g < g1; g += BATCH_THREADS) {
        const long f = head + 4 * g;
        batch_f32x4 lo, hi;
        if (W == 2) {
            const batch_u32x4 v = *(const batch_u32x4 *)(src + 4 * f);             // four frames of two int16
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                lo[2 * k] = batch_pcm_value<2>((short)(v[k] & 0xffffu));
                lo[2 * k + 1] = batch_pcm_value<2>((short)(v[k] >> 16));
                hi[2 * k] = batch_pcm_value<2>((short)(v[2 + k] & 0xffffu));
                hi[2 * k + 1] = batch_pcm_value<2>((short)(v[2 + k] >> 16));
            }
        } else {
            const batch_u32x4 a = *(const batch_u32x4 *)(src + 8 * f), b = *(const batch_u32x4 *)(src + 8 * f + 16);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                lo[k] = batch_pcm_value<4>((int)a[k]);
                hi[k] = batch_pcm_value<4>((int)b[k]);
            }
        }
        *(batch_f32x4 *)(o + 2 * f) = lo;
        *(batch_f32x4 *)(o + 2 * f + 4) = hi;
    }
    if (blockIdx.x == 0) {                                                         // the head frame and the up to three tail frames
        const long tail0 = head + 4 * nbody;
        if (tid < head) batch_gather_frame<W>(src, o, tid);
        if (tid >= 64 && tail0 + (tid - 64) < frames) batch_gather_frame<W>(src, o, tail0 + (tid - 64));
    }
}

__device__ __forceinline__ float batch_clamp(float v) { return v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v); }

// grid (ceil(groups / BATCH_GROUPS_PER_BLOCK) or 1, m, C); BATCH_THREADS threads.  x [n][Lp][C], out [m][C][len]; a workgroup writes one
// channel of one output row (the two channels of a row start at different phases of a 16-byte line when len is odd; the frames a stereo
// group loads are shared with the other channel's workgroup through the caches)
template <int C>
__global__ __launch_bounds__(BATCH_THREADS) void batch_finish_kernel(const float *x, const long *rows, const long *start, float *out, long Lp, long len) {
    const int tid = threadIdx.x, c = blockIdx.z;
    const long r = blockIdx.y;
    const float *src = x + (rows[r] * Lp + start[r]) * C + c;                      // sample t of the row: src[t * C]
    float *o = out + (r * C + c) * len;
    long head = (long)(((16 - ((uintptr_t)o & 15)) & 15) >> 2);                    // floats up to the next 16-byte boundary
    if (head > len) head = len;
    const long nbody = (len - head) / 4;
    const long g1 = nbody < ((long)blockIdx.x + 1) * BATCH_GROUPS_PER_BLOCK ? nbody : ((long)blockIdx.x + 1) * BATCH_GROUPS_PER_BLOCK;
    for (long g = (long)blockIdx.x * BATCH_GROUPS_PER_BLOCK + tid; g < g1; g += BATCH_THREADS) {
        const long t = head + 4 * g;
        batch_f32x4 y;
        if (C == 1) {
            const batch_f32x4_any v = *(const batch_f32x4_any *)(src + t);
#pragma unroll
            for (int k = 0; k < 4; ++k) y[k] = batch_clamp(v[k]);
        } else {
            const float *p = src - c + 2 * t;                                      // four interleaved frames
            const batch_f32x4_any a = *(const batch_f32x4_any *)p, b = *(const batch_f32x4_any *)(p + 4);
            y[0] = batch_clamp(a[c]);
            y[1] = batch_clamp(a[2 + c]);
            y[2] = batch_clamp(b[c]);
            y[3] = batch_clamp(b[2 + c]);
        }
        *(batch_f32x4 *)(o + t) = y;
    }
    if (blockIdx.x == 0) {
        const long tail0 = head + 4 * nbody;
        if (tid < head) o[tid] = batch_clamp(src[(long)tid * C]);
        if (tid >= 64 && tail0 + (tid - 64) < len) o[tail0 + (tid - 64)] = batch_clamp(src[(tail0 + (tid - 64)) * C]);
    }
}
