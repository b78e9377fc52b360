// Rational polyphase FIR resampler over the FX layout (fp32 [n_items][L][C], C = 1 or 2): stems at another sample rate are brought to the
// networks' 44.1 kHz where their decoded PCM already is.  The reference has no counterpart: its loaders raise for every other rate.
//
// Arithmetic.  y[m] = sum_j h[m down - j up + half] x[j], h the 2 half + 1 float32 prototype taps (host design in mst_fx.hip), x zero outside
// the buffer the caller passes: scipy.signal.resample_poly(padtype = 'constant') - output 0 sits on input 0, no delay.  With
// n = m down + half, q = n / up and r = n % up the sum runs over t = 0 .. T - 1 (T = 2 half / up + 1 taps per phase) as
// h[r + t up] x[q - t]: tap-major, the table is the prototype itself, zero-padded to T up entries.  A product of two float32 values is exact in
// float64; the products are added in float64 in the order of t - a function of m alone, never of the batch, the tile, the chunk or the run -
// and the sum is rounded once to float32.  A term outside the filter or the buffer is a product with an exact zero and leaves the sum as
// it is, so a chunked call gives the bits of the whole-signal call.  No atomics.
//
// resample_kernel.  One workgroup per (tile of RESAMPLE_TILE consecutive output frames, item), one lane per output frame.  The tile's input
// span - (tile - 1) down / up + T frames at most - is staged once into LDS with coalesced loads of the interleaved frames (zeros outside the
// buffer); a lane then walks its T taps: one cached global load of the tap (lanes of a wave differ in r: at one t they read inside one
// stretch of `up` floats), one LDS read of the frame (ds_read_b64 for stereo: both channels use the tap), one float64 fma per channel.
// Positions are 64-bit once per workgroup (m down passes 2^31 inside a one-hour 192 kHz file) and 32-bit relative to the tile after that.
#pragma once
#include "mst_dev.h"

#define RESAMPLE_TILE 256
#define RESAMPLE_LDS_FLOATS 4608          // 18 KiB: 2304 stereo frames; the host refuses a ratio whose tile span does not fit

// grid (tiles, 1, items); RESAMPLE_TILE threads.
//   x  [n_items][n_in][C]: inputs in_start .. in_start + n_in - 1 of each item's signal;  y [n_items][n_out][C]: outputs out_start ..
//   taps [T * up]: h zero-padded;  span_max * C <= RESAMPLE_LDS_FLOATS (checked by the host)
template <int C>
__global__ __launch_bounds__(RESAMPLE_TILE) void resample_kernel(const float *x, long n_in, long in_start, float *y, long n_out, long out_start,
                                                                const float *taps, int up, int down, int half, int T) {
    __shared__ float2 xs2[RESAMPLE_LDS_FLOATS / 2];
    float *xs = (float *)xs2;
    const int tid = threadIdx.x;
    const long o0 = (long)blockIdx.x * RESAMPLE_TILE;                                  // first output of the tile, relative to out_start
    const int nv = n_out - o0 < RESAMPLE_TILE ? (int)(n_out - o0) : RESAMPLE_TILE;     // outputs of this tile
    const long n0 = (out_start + o0) * (long)down + half;
    const long q0 = n0 / up;
    const int r0 = (int)(n0 - q0 * up);
    const long j_lo = q0 - (T - 1);                                                    // first input frame any lane of the tile reads
    const int span = (r0 + (nv - 1) * down) / up + T;
    const float *xi = x + (long)blockIdx.z * n_in * C;
    const long g0 = (j_lo - in_start) * C, g1 = n_in * C;                              // LDS float e is buffer float g0 + e
    for (int e = tid; e < span * C; e += RESAMPLE_TILE) {
        const long g = g0 + e;
        xs[e] = g >= 0 && g < g1 ? xi[g] : 0.0f;
    }
    __syncthreads();
    if (tid >= nv) return;
    const int a = r0 + tid * down, dq = a / up, r = a - dq * up;
    const int jr = dq + T - 1;                                                         // LDS frame of input q; tap t reads frame jr - t
    const float *hp = taps + r;
    double acc0 = 0.0, acc1 = 0.0;
#pragma unroll 4
    for (int t = 0; t < T; ++t) {
        const double h = (double)hp[t * up];
        if (C == 2) {
            const float2 v = xs2[jr - t];
            acc0 = fma(h, (double)v.x, acc0);
            acc1 = fma(h, (double)v.y, acc1);
        } else {
            acc0 = fma(h, (double)xs[jr - t], acc0);
        }
    }
    float *yo = y + ((long)blockIdx.z * n_out + o0 + tid) * C;
    if (C == 2) *(float2 *)yo = make_float2((float)acc0, (float)acc1);
    else yo[0] = (float)acc0;
}
