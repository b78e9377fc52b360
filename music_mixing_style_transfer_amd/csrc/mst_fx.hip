// libmst_hip.so, FX-processor part of the C ABI (mst_fx_*): equaliser, compressor, imager, gain, Haas / panner, FFT convolution, STFT,
// algorithmic reverb, multi-scale spectral distance, mixing-feature metrics - launches of csrc/fx_kernels.h, csrc/fft_kernels.h, csrc/mss_kernels.h and
// csrc/mixfeat_kernels.h - and the training-batch launches mst_batch_* of csrc/batch_kernels.h.  See include/mst_hip.h for the contract.
#include "mst_host.h"
#include "fft_kernels.h"
#include "fx_kernels.h"
#include "mss_kernels.h"
#include "contrast_kernels.h"
#include "mixfeat_kernels.h"
#include "resample_kernels.h"
#include "batch_kernels.h"

// =================================================================================================
// FX processors
// =================================================================================================
namespace {
// an MstFxFuse built against another layout of the struct would be read as garbage: its first member is its own size
int fuse_check(const MstFxFuse *fuse, const char *who) {
    if (fuse && fuse->struct_size != sizeof(MstFxFuse)) return fail(MST_ERR_ARG, std::string(who) + ": MstFxFuse.struct_size does not match this library's layout");
    if (fuse && (fuse->forms & ~(MST_FX_FORM_EQ_LANE_APPLY | MST_FX_FORM_EQ_VALU_ENDS | MST_FX_FORM_COMP_SLICE_SMALL))) return fail(MST_ERR_ARG, std::string(who) + ": unknown MstFxFuse.forms bits");
    return MST_OK;
}
// Steps per chunk of the time-parallel biquad cascade: the number of 511-chunk scan blocks that minimises
//     16 us per scan block + two chunk passes at 0.19 us per step of a chunk
// (measured on an MI355X; a pass is one lane per chunk and its time falls with the chunk length until every SIMD holds a wave = 65536
// lanes, after which it is the total work that counts: 144-step chunks at 116 k lanes take the same 105 us as 272-step chunks at 62 k).
// A 131072-sample segment x 128 sequences: 1 block, 272 steps, 482 chunks; a 3-minute stem x 2: ~16 blocks, ~976 steps.
int biquad_chunk(long L, long n_seq) {
    auto up16 = [](long v) { return (int)((v + 15) / 16 * 16); };
    int best_m = 64;
    double best = 1e300;
    for (int B = 1; B <= 64; ++B) {
        int m = up16((L + 511L * B - 1) / (511L * B));
        if (m < 64) m = 64;
        const long nchunks = (L + m - 1) / m;
        const double lanes = (double)n_seq * (double)nchunks;
        const double cost = 16.0 * (double)((nchunks + 510) / 511) + 0.39 * m * (lanes > 65536.0 ? lanes / 65536.0 : 1.0);
        if (cost < best) {
            best = cost;
            best_m = m;
        }
        if (m == 64) break;
    }
    return best_m;
}
// what mst_fx_biquad_cascade does with a scratch buffer, and the workgroup size of its scan: shared with mst_fx_biquad_plan
bool biquad_time_parallel(long nchunks, int n_bands) { return nchunks > 1 && n_bands > 0; }
int biquad_scan_threads(long nchunks) { return nchunks > 255 ? 512 : 256; }
void biquad_coefs(const double *coef, int n_bands, double (*out)[5]) {
    for (int k = 0; k < MST_MAX_BANDS; ++k)
        for (int i = 0; i < 5; ++i) out[k][i] = 0.0;
    for (int k = 0; k < n_bands; ++k) {
        const double a0 = coef[6 * k + 3];
        out[k][0] = coef[6 * k + 0] / a0;
        out[k][1] = coef[6 * k + 1] / a0;
        out[k][2] = coef[6 * k + 2] / a0;
        out[k][3] = coef[6 * k + 4] / a0;
        out[k][4] = coef[6 * k + 5] / a0;
    }
}
}  // namespace

namespace {
// The host-side tables of a coefficient set at chunk length M, [M][S] impulse states | [levels][S][S] powers (A^M)^(2^l) | A fragments: what
// biquad_impulse_table uploads and mst_fx_biquad_tables shows
void biquad_host_tables(const double (*coef)[5], int n_bands, int M, double *host) {
    const int S = 2 * n_bands;
    const size_t n_tab = (size_t)M * S, n_pow = (size_t)MST_BIQUAD_LEVELS * S * S, n_frag = (size_t)((M + 15) / 16) * 4 * 64;
    std::vector<double> z(S, 0.0);
    for (int m = 0; m < M; ++m) {
        double v = m == 0 ? 1.0 : 0.0;
        for (int b = 0; b < n_bands; ++b) v = fx_biquad_band(v, z[2 * b], z[2 * b + 1], coef[b]);
        for (int j = 0; j < S; ++j) host[(size_t)m * S + j] = z[j];
    }
    {   // A^M column by column (the cascade run M steps on zero input from each unit state), then squared up level by level
        double *pm = host + n_tab;
        for (int col = 0; col < S; ++col) {
            std::vector<double> u(S, 0.0);
            u[col] = 1.0;
            for (int n = 0; n < M; ++n) {
                double v = 0.0;
                for (int b = 0; b < n_bands; ++b) v = fx_biquad_band(v, u[2 * b], u[2 * b + 1], coef[b]);
            }
            for (int row = 0; row < S; ++row) pm[(size_t)row * S + col] = u[row];
        }
        for (int l = 1; l < MST_BIQUAD_LEVELS; ++l) {
            const double *cur = pm + (size_t)(l - 1) * S * S;
            double *nxt = pm + (size_t)l * S * S;
            for (int r = 0; r < S; ++r)
                for (int c = 0; c < S; ++c) {
                    double acc = 0.0;
                    for (int j = 0; j < S; ++j) acc += cur[r * S + j] * cur[j * S + c];
                    nxt[r * S + c] = acc;
                }
        }
    }
    {   // fragment (slab sb, k-step kk), lane (state j = l & 15, kq = l >> 4): the weight of sample 16 sb + 4 kk + kq in the end state, h_(M - 1 - sample)[j]
        double *fr = host + n_tab + n_pow;
        for (size_t i = 0; i < n_frag; ++i) {
            const int l = (int)(i % 64), kk = (int)(i / 64 % 4), sb = (int)(i / 256), j = l & 15, smp = 16 * sb + 4 * kk + (l >> 4);
            fr[i] = (j < S && smp < M) ? host[(size_t)(M - 1 - smp) * S + j] : 0.0;
        }
    }
}
// Impulse-state table of a biquad cascade for fx_biquad_ends_kernel: h_m = the cascade's state m steps after a unit impulse, m = 0 .. M - 1,
// [M][2 * n_bands] float64.  Built on the host (the kernels' own recursion) and kept on the device per (device, coefficients, M): a chain calls
// its equaliser with the same settings again and again.  An entry owns its host copy (the asynchronous upload reads it) and its device
// buffer; the 16 most recent entries per device are kept.  A miss (rare: a new equaliser setting) uploads and WAITS for the upload; evicting
// an entry also waits for the device (randomised parameter sweeps) - neither can happen inside a stream capture.
struct BiquadTab {
    int dev = -1, n_bands = 0, M = 0;
    double coef[MST_MAX_BANDS][5];
    std::vector<double> host;
    double *devp = nullptr;
    unsigned long stamp = 0;
};
// (the same entry carries the scan's matrix powers (A^M)^(2^l), l = 0 .. MST_BIQUAD_LEVELS - 1, behind the table: [M][S] | [levels][S][S];
//  round 4 squared them up on the device with a one-workgroup launch per call - 5-8 us on the chain's critical path)
const double *biquad_impulse_table(const double (*coef)[5], int n_bands, int M, void *stream) {
    static std::mutex mu;
    static std::vector<BiquadTab *> tabs;
    static unsigned long clock_ = 0;
    const int dev = mst_current_device();
    std::lock_guard<std::mutex> lock(mu);
    BiquadTab *oldest = nullptr;
    int n_dev = 0;
    for (BiquadTab *t : tabs) {
        if (t->dev != dev) continue;
        ++n_dev;
        if (t->n_bands == n_bands && t->M == M && std::memcmp(t->coef, coef, sizeof(double) * 5 * n_bands) == 0) {
            t->stamp = ++clock_;
            return t->devp;
        }
        if (!oldest || t->stamp < oldest->stamp) oldest = t;
    }
    const int S = 2 * n_bands;
    BiquadTab *t = nullptr;
    if (n_dev >= 16) {
        t = oldest;
        if (hipDeviceSynchronize() != hipSuccess) return nullptr;      // nobody reads the evicted table any more
    } else {
        t = new BiquadTab;
        tabs.push_back(t);
    }
    t->dev = dev;
    t->n_bands = n_bands;
    t->M = M;
    std::memset(t->coef, 0, sizeof(t->coef));
    std::memcpy(t->coef, coef, sizeof(double) * 5 * n_bands);
    t->stamp = ++clock_;
    // [M][S] table | [levels][S][S] powers | [M / 16][4][64] the table as A fragments of v_mfma_f64_16x16x4_f64 (state rows, 16 samples per slab)
    const size_t n_tab = (size_t)M * S, n_pow = (size_t)MST_BIQUAD_LEVELS * S * S, n_frag = (size_t)((M + 15) / 16) * 4 * 64, n_all = n_tab + n_pow + n_frag;
    if (t->host.size() < n_all) {
        if (t->devp) (void)hipFree(t->devp);
        t->devp = nullptr;
        t->host.assign(n_all, 0.0);
    }
    biquad_host_tables(coef, n_bands, M, t->host.data());
    if (!t->devp && hipMalloc((void **)&t->devp, t->host.size() * sizeof(double)) != hipSuccess) {
        t->dev = -1;
        t->devp = nullptr;
        return nullptr;
    }
    // a cache HIT hands devp to whatever stream (or thread) asks next, with no ordering against this upload: the table is complete before
    // this function - and with it the mutex - lets anybody see the entry (a miss is rare: once per equaliser setting)
    if (hipMemcpyAsync(t->devp, t->host.data(), n_all * sizeof(double), hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess) {
        t->dev = -1;
        return nullptr;
    }
    return t->devp;
}
}  // namespace

extern "C" size_t mst_fx_biquad_scratch_bytes(int n_items, long L, int C, int n_bands) {
    if (n_items < 1 || L < 1 || C < 1 || n_bands < 1) return 0;
    const int M = biquad_chunk(L, (long)n_items * C);
    const long nchunks = (L + M - 1) / M;
    const size_t states = (size_t)n_items * C * nchunks * 2 * MST_MAX_BANDS;
    return (2 * states + (size_t)MST_BIQUAD_LEVELS * 4 * MST_MAX_BANDS * MST_MAX_BANDS) * sizeof(double);      // ends | starts | (A^M)^(2^l)
}

extern "C" int mst_fx_biquad_plan(int n_items, long L, int C, int n_bands, MstFxBiquadPlan *plan) {
    if (!plan || plan->struct_size != sizeof(MstFxBiquadPlan)) return fail(MST_ERR_ARG, "mst_fx_biquad_plan: MstFxBiquadPlan.struct_size does not match this library's layout");
    if (n_items < 1 || L < 1 || C < 1 || n_bands < 0 || n_bands > MST_MAX_BANDS) return fail(MST_ERR_ARG, "mst_fx_biquad_plan: bad argument");
    const int M = biquad_chunk(L, (long)n_items * C);
    const long nchunks = (L + M - 1) / M;
    plan->M = M;
    plan->nchunks = nchunks;
    plan->time_parallel = biquad_time_parallel(nchunks, n_bands);            // what mst_fx_biquad_cascade does when it is given the scratch buffer
    plan->scan_threads = plan->time_parallel ? biquad_scan_threads(nchunks) : 0;
    plan->record_doubles = 2 * MST_MAX_BANDS;
    plan->ends_offset = 0;
    plan->starts_offset = (size_t)n_items * C * nchunks * 2 * MST_MAX_BANDS * sizeof(double);
    return MST_OK;
}

extern "C" int mst_fx_biquad_tables(const double *coef, int n_bands, int M, double *table_host, double *powers_host) {
    if (!coef || !table_host || !powers_host || n_bands < 1 || n_bands > MST_MAX_BANDS || M < 16 || M % 16) return fail(MST_ERR_ARG, "mst_fx_biquad_tables: bad argument");
    double cf[MST_MAX_BANDS][5];
    biquad_coefs(coef, n_bands, cf);
    const int S = 2 * n_bands;
    const size_t n_tab = (size_t)M * S, n_pow = (size_t)MST_BIQUAD_LEVELS * S * S, n_frag = (size_t)((M + 15) / 16) * 4 * 64;
    std::vector<double> host(n_tab + n_pow + n_frag, 0.0);
    biquad_host_tables(cf, n_bands, M, host.data());
    std::memcpy(table_host, host.data(), n_tab * sizeof(double));
    std::memcpy(powers_host, host.data() + n_tab, n_pow * sizeof(double));
    return MST_OK;
}

extern "C" int mst_fx_biquad_cascade(const float *x, float *y, int n_items, long L, int C, const double *coef, int n_bands,
                                     double *scratch, size_t scratch_bytes, const MstFxFuse *fuse, void *stream) {
    if (!x || !y || !coef || n_items < 1 || L < 1 || C < 1) return fail(MST_ERR_ARG, "mst_fx_biquad_cascade: bad argument");
    if (int rc = fuse_check(fuse, "mst_fx_biquad_cascade")) return rc;
    // kernel forms of THIS call (MstFxFuse.forms; results do not depend on them): the reference forms of the stereo passes
    const bool eq_lane_apply = fuse && (fuse->forms & MST_FX_FORM_EQ_LANE_APPLY), eq_valu_ends = fuse && (fuse->forms & MST_FX_FORM_EQ_VALU_ENDS);
    if (fuse && fuse->post_rms) return fail(MST_ERR_UNSUPPORTED, "mst_fx_biquad_cascade: tail folding (post_rms) is the imager's");
    if (fuse && (fuse->out_ms_dev || fuse->in_ms_dev)) return fail(MST_ERR_UNSUPPORTED, "mst_fx_biquad_cascade: the mid / side energies travel from the compressor to the imager");
    if (n_bands < 0 || n_bands > MST_MAX_BANDS) return fail(MST_ERR_UNSUPPORTED, "mst_fx_biquad_cascade: at most 8 bands");
    const int M = biquad_chunk(L, (long)n_items * C);
    const long nchunks = (L + M - 1) / M;
    if (scratch && biquad_time_parallel(nchunks, n_bands)) {
        if (scratch_bytes < mst_fx_biquad_scratch_bytes(n_items, L, C, n_bands))
            return fail(MST_ERR_WORKSPACE, "mst_fx_biquad_cascade: scratch too small");
        BiquadChunkArgs a;
        a.x = x;
        a.y = y;
        a.n_seq = n_items * C;
        a.C = C;
        a.nchunks = (int)nchunks;
        a.M = M;
        a.L = L;
        a.n_bands = n_bands;
        a.in_scale = fuse ? fuse->in_scale_dev : nullptr;
        a.out_sumsq = fuse ? fuse->out_sumsq_dev : nullptr;
        a.out_in_sumsq = fuse ? fuse->out_in_sumsq_dev : nullptr;
        biquad_coefs(coef, n_bands, a.coef);
        const size_t states = (size_t)a.n_seq * nchunks * 2 * MST_MAX_BANDS;
        double *ends = scratch, *starts = scratch + states;
        a.ends = ends;
        a.starts = starts;
        const int S = 2 * n_bands;
        const long lanes = (long)a.n_seq * nchunks;
        const dim3 cg((unsigned)((lanes + 63) / 64));
        auto launch_chunks = [&](auto APPLY) {         // the band count is a template parameter: no per-band branches in the recursion
            constexpr bool ap = decltype(APPLY)::value;
            switch (n_bands) {
                case 1: MST_LAUNCH((fx_biquad_chunk_kernel<ap, 1>), cg, dim3(64), stream, a); break;
                case 2: MST_LAUNCH((fx_biquad_chunk_kernel<ap, 2>), cg, dim3(64), stream, a); break;
                case 3: MST_LAUNCH((fx_biquad_chunk_kernel<ap, 3>), cg, dim3(64), stream, a); break;
                case 4: MST_LAUNCH((fx_biquad_chunk_kernel<ap, 4>), cg, dim3(64), stream, a); break;
                case 5: MST_LAUNCH((fx_biquad_chunk_kernel<ap, 5>), cg, dim3(64), stream, a); break;
                case 6: MST_LAUNCH((fx_biquad_chunk_kernel<ap, 6>), cg, dim3(64), stream, a); break;
                case 7: MST_LAUNCH((fx_biquad_chunk_kernel<ap, 7>), cg, dim3(64), stream, a); break;
                default: MST_LAUNCH((fx_biquad_chunk_kernel<ap, 8>), cg, dim3(64), stream, a); break;
            }
        };
        // pass 1: zero-state end states as dot products with the cascade's impulse-state table (fx_biquad_ends_kernel)
        const double *htab = biquad_impulse_table(a.coef, n_bands, M, stream);
        if (!htab) return fail(MST_ERR_HIP, "mst_fx_biquad_cascade: impulse-state table");
        const long npairs = (long)n_items * nchunks;                       // stereo: (item, chunk) pairs - 32 per wave, slabs through LDS
        if (C == 2 && !eq_valu_ends && M % 16 == 0) {          // stereo: the end states as a matrix product on the float64 matrix cores
            const dim3 eg((unsigned)((npairs + 127) / 128));
            MST_LAUNCH(fx_biquad_stereo_ends_mfma_kernel, eg, dim3(256), stream, a, htab + (size_t)M * S + (size_t)MST_BIQUAD_LEVELS * S * S);
        } else if (C == 2) {
            const dim3 eg((unsigned)((npairs + 127) / 128));
            switch (n_bands) {
                case 1: MST_LAUNCH(fx_biquad_stereo_ends_kernel<1>, eg, dim3(256), stream, a, htab); break;
                case 2: MST_LAUNCH(fx_biquad_stereo_ends_kernel<2>, eg, dim3(256), stream, a, htab); break;
                case 3: MST_LAUNCH(fx_biquad_stereo_ends_kernel<3>, eg, dim3(256), stream, a, htab); break;
                case 4: MST_LAUNCH(fx_biquad_stereo_ends_kernel<4>, eg, dim3(256), stream, a, htab); break;
                case 5: MST_LAUNCH(fx_biquad_stereo_ends_kernel<5>, eg, dim3(256), stream, a, htab); break;
                case 6: MST_LAUNCH(fx_biquad_stereo_ends_kernel<6>, eg, dim3(256), stream, a, htab); break;
                case 7: MST_LAUNCH(fx_biquad_stereo_ends_kernel<7>, eg, dim3(256), stream, a, htab); break;
                default: MST_LAUNCH(fx_biquad_stereo_ends_kernel<8>, eg, dim3(256), stream, a, htab); break;
            }
        } else {
            const dim3 eg((unsigned)((4 * lanes + 255) / 256));          // four lanes per chunk
            switch (n_bands) {
                case 1: MST_LAUNCH(fx_biquad_ends_kernel<1>, eg, dim3(256), stream, a, htab); break;
                case 2: MST_LAUNCH(fx_biquad_ends_kernel<2>, eg, dim3(256), stream, a, htab); break;
                case 3: MST_LAUNCH(fx_biquad_ends_kernel<3>, eg, dim3(256), stream, a, htab); break;
                case 4: MST_LAUNCH(fx_biquad_ends_kernel<4>, eg, dim3(256), stream, a, htab); break;
                case 5: MST_LAUNCH(fx_biquad_ends_kernel<5>, eg, dim3(256), stream, a, htab); break;
                case 6: MST_LAUNCH(fx_biquad_ends_kernel<6>, eg, dim3(256), stream, a, htab); break;
                case 7: MST_LAUNCH(fx_biquad_ends_kernel<7>, eg, dim3(256), stream, a, htab); break;
                default: MST_LAUNCH(fx_biquad_ends_kernel<8>, eg, dim3(256), stream, a, htab); break;
            }
        }
        MST_CHECK_LAUNCH("fx_biquad_ends_kernel");
        const dim3 sg((unsigned)a.n_seq);
        const double *pmat = htab + (size_t)M * S;          // (A^M)^(2^l), l = 0 .. 8: behind the impulse-state table (cached per coefficient set)
        auto launch_scan = [&](auto NBv) {
            constexpr int nb = decltype(NBv)::value;
            const double *e = ends, *pmc = pmat;
            switch (n_bands) {
                case 1: MST_LAUNCH((fx_biquad_scan_kernel<1, nb>), sg, dim3(nb), stream, e, starts, pmc, a.n_seq, (int)nchunks); break;
                case 2: MST_LAUNCH((fx_biquad_scan_kernel<2, nb>), sg, dim3(nb), stream, e, starts, pmc, a.n_seq, (int)nchunks); break;
                case 3: MST_LAUNCH((fx_biquad_scan_kernel<3, nb>), sg, dim3(nb), stream, e, starts, pmc, a.n_seq, (int)nchunks); break;
                case 4: MST_LAUNCH((fx_biquad_scan_kernel<4, nb>), sg, dim3(nb), stream, e, starts, pmc, a.n_seq, (int)nchunks); break;
                case 5: MST_LAUNCH((fx_biquad_scan_kernel<5, nb>), sg, dim3(nb), stream, e, starts, pmc, a.n_seq, (int)nchunks); break;
                case 6: MST_LAUNCH((fx_biquad_scan_kernel<6, nb>), sg, dim3(nb), stream, e, starts, pmc, a.n_seq, (int)nchunks); break;
                case 7: MST_LAUNCH((fx_biquad_scan_kernel<7, nb>), sg, dim3(nb), stream, e, starts, pmc, a.n_seq, (int)nchunks); break;
                default: MST_LAUNCH((fx_biquad_scan_kernel<8, nb>), sg, dim3(nb), stream, e, starts, pmc, a.n_seq, (int)nchunks); break;
            }
        };
        if (biquad_scan_threads(nchunks) == 512) launch_scan(std::integral_constant<int, 512>{});
        else launch_scan(std::integral_constant<int, 256>{});
        MST_CHECK_LAUNCH("fx_biquad_scan_kernel");
        if (C == 2 && !eq_lane_apply) {          // stereo: the chunks travel in 16-frame slabs through LDS, in and out
            const dim3 ag((unsigned)((npairs + 127) / 128));
            switch (n_bands) {
                case 1: MST_LAUNCH(fx_biquad_stereo_apply_kernel<1>, ag, dim3(256), stream, a); break;
                case 2: MST_LAUNCH(fx_biquad_stereo_apply_kernel<2>, ag, dim3(256), stream, a); break;
                case 3: MST_LAUNCH(fx_biquad_stereo_apply_kernel<3>, ag, dim3(256), stream, a); break;
                case 4: MST_LAUNCH(fx_biquad_stereo_apply_kernel<4>, ag, dim3(256), stream, a); break;
                case 5: MST_LAUNCH(fx_biquad_stereo_apply_kernel<5>, ag, dim3(256), stream, a); break;
                case 6: MST_LAUNCH(fx_biquad_stereo_apply_kernel<6>, ag, dim3(256), stream, a); break;
                case 7: MST_LAUNCH(fx_biquad_stereo_apply_kernel<7>, ag, dim3(256), stream, a); break;
                default: MST_LAUNCH(fx_biquad_stereo_apply_kernel<8>, ag, dim3(256), stream, a); break;
            }
        } else {
            launch_chunks(std::true_type{});
        }
        MST_CHECK_LAUNCH("fx_biquad_chunk_kernel<apply>");
        return MST_OK;
    }
    if (fuse && (fuse->in_scale_dev || fuse->out_sumsq_dev || fuse->out_in_sumsq_dev))
        return fail(MST_ERR_UNSUPPORTED, "mst_fx_biquad_cascade: chain fusion needs the time-parallel path (scratch, more than one chunk, >= 1 band)");
    BiquadArgs a;
    a.x = x;
    a.y = y;
    a.n_seq = n_items * C;
    a.C = C;
    a.L = L;
    a.n_bands = n_bands;
    biquad_coefs(coef, n_bands, a.coef);
    MST_LAUNCH(fx_biquad_kernel, dim3((a.n_seq + 63) / 64), dim3(64), stream, a);
    MST_CHECK_LAUNCH("fx_biquad_kernel");
    return MST_OK;
}

// ---- per-item parameters: the equaliser ---------------------------------------------------------------------------
namespace {
// the scratch of mst_fx_biquad_cascade_items: the shared call's layout (ends | starts | the shared call's powers, unused here), then one
// block per item: [M][S] impulse states | [levels][S][S] powers | [MST_MAX_BANDS][5] normalised coefficients
struct EqItems { int M; long nchunks; size_t shared_bytes; long n_tab, n_pow, stride; };
EqItems eq_items(int n_items, long L, int C, int n_bands) {
    EqItems e;
    e.M = biquad_chunk(L, (long)n_items * C);
    e.nchunks = (L + e.M - 1) / e.M;
    e.shared_bytes = mst_fx_biquad_scratch_bytes(n_items, L, C, n_bands);
    const long S = 2 * n_bands;
    e.n_tab = (long)e.M * S;
    e.n_pow = (long)MST_BIQUAD_LEVELS * S * S;
    e.stride = e.n_tab + e.n_pow + MST_MAX_BANDS * 5;
    return e;
}
}  // namespace

extern "C" size_t mst_fx_biquad_items_scratch_bytes(int n_items, long L, int C, int n_bands) {
    if (n_items < 1 || L < 1 || C < 1 || n_bands < 1 || n_bands > MST_MAX_BANDS) return 0;
    const EqItems e = eq_items(n_items, L, C, n_bands);
    return e.shared_bytes + (size_t)n_items * e.stride * sizeof(double);
}

extern "C" int mst_fx_biquad_items_plan(int n_items, long L, int C, int n_bands, MstFxBiquadItemsPlan *plan) {
    if (!plan || plan->struct_size != sizeof(MstFxBiquadItemsPlan)) return fail(MST_ERR_ARG, "mst_fx_biquad_items_plan: MstFxBiquadItemsPlan.struct_size does not match this library's layout");
    if (n_items < 1 || L < 1 || C < 1 || n_bands < 1 || n_bands > MST_MAX_BANDS) return fail(MST_ERR_ARG, "mst_fx_biquad_items_plan: bad argument");
    const EqItems e = eq_items(n_items, L, C, n_bands);
    plan->M = e.M;
    plan->tables_offset = e.shared_bytes;
    plan->item_stride = (size_t)e.stride * sizeof(double);
    plan->powers_offset = (size_t)e.n_tab * sizeof(double);
    plan->coef_offset = (size_t)(e.n_tab + e.n_pow) * sizeof(double);
    plan->total_bytes = e.shared_bytes + (size_t)n_items * e.stride * sizeof(double);
    return MST_OK;
}

#define MST_BANDS_SWITCH(NB_EXPR, LAUNCH)                                                                                               \
    switch (NB_EXPR) {                                                                                                                  \
        case 1: { constexpr int NBv = 1; LAUNCH; } break;                                                                               \
        case 2: { constexpr int NBv = 2; LAUNCH; } break;                                                                               \
        case 3: { constexpr int NBv = 3; LAUNCH; } break;                                                                               \
        case 4: { constexpr int NBv = 4; LAUNCH; } break;                                                                               \
        case 5: { constexpr int NBv = 5; LAUNCH; } break;                                                                               \
        case 6: { constexpr int NBv = 6; LAUNCH; } break;                                                                               \
        case 7: { constexpr int NBv = 7; LAUNCH; } break;                                                                               \
        default: { constexpr int NBv = 8; LAUNCH; } break;                                                                              \
    }

extern "C" int mst_fx_biquad_cascade_items(const float *x, float *y, int n_items, long L, int C, const double *coef_dev, int n_bands,
                                           double *scratch, size_t scratch_bytes, const MstFxFuse *fuse, void *stream) {
    if (!x || !y || n_items < 1 || n_items > 65535 || L < 1 || C < 1 || (!coef_dev && n_bands > 0)) return fail(MST_ERR_ARG, "mst_fx_biquad_cascade_items: bad argument");
    if (int rc = fuse_check(fuse, "mst_fx_biquad_cascade_items")) return rc;
    const bool eq_lane_apply = fuse && (fuse->forms & MST_FX_FORM_EQ_LANE_APPLY);
    if (fuse && fuse->post_rms) return fail(MST_ERR_UNSUPPORTED, "mst_fx_biquad_cascade_items: tail folding (post_rms) is the imager's");
    if (fuse && (fuse->out_ms_dev || fuse->in_ms_dev)) return fail(MST_ERR_UNSUPPORTED, "mst_fx_biquad_cascade_items: the mid / side energies travel from the compressor to the imager");
    if (n_bands < 0 || n_bands > MST_MAX_BANDS) return fail(MST_ERR_UNSUPPORTED, "mst_fx_biquad_cascade_items: at most 8 bands");
    if (scratch && n_bands > 0) {
        const EqItems e = eq_items(n_items, L, C, n_bands);
        if (biquad_time_parallel(e.nchunks, n_bands)) {
            if (scratch_bytes < e.shared_bytes + (size_t)n_items * e.stride * sizeof(double))
                return fail(MST_ERR_WORKSPACE, "mst_fx_biquad_cascade_items: scratch too small");
            const long nchunks = e.nchunks;
            BiquadChunkArgs a;
            a.x = x;
            a.y = y;
            a.n_seq = n_items * C;
            a.C = C;
            a.nchunks = (int)nchunks;
            a.M = e.M;
            a.L = L;
            a.n_bands = n_bands;
            a.in_scale = fuse ? fuse->in_scale_dev : nullptr;
            a.out_sumsq = fuse ? fuse->out_sumsq_dev : nullptr;
            a.out_in_sumsq = fuse ? fuse->out_in_sumsq_dev : nullptr;
            std::memset(a.coef, 0, sizeof(a.coef));                      // every kernel reads its item's coefficients from the item's block
            const size_t states = (size_t)a.n_seq * nchunks * 2 * MST_MAX_BANDS;
            a.ends = scratch;
            a.starts = scratch + states;
            FxiEqTabs t;
            t.base = (double *)((unsigned char *)scratch + e.shared_bytes);
            t.stride = e.stride;
            t.off_pow = e.n_tab;
            t.off_coef = e.n_tab + e.n_pow;
            t.M = e.M;
            t.n_bands = n_bands;
            const unsigned ni = (unsigned)n_items;
            // every item's tables, built where they are used: no host build, no upload, no cache entry
            MST_LAUNCH(fxi_eq_tables_kernel, dim3(ni), dim3(64), stream, coef_dev, t);
            MST_CHECK_LAUNCH("fxi_eq_tables_kernel");
            const long lanes = (long)C * nchunks;                          // per item
            if (C == 2) {          // stereo: the VALU state pass on slabs whatever MST_FX_FORM_EQ_VALU_ENDS says (the same bits as the matrix-core one)
                MST_BANDS_SWITCH(n_bands, MST_LAUNCH(fxi_eq_stereo_ends_kernel<NBv>, dim3((unsigned)((nchunks + 127) / 128), ni), dim3(256), stream, a, t))
            } else {
                MST_BANDS_SWITCH(n_bands, MST_LAUNCH(fxi_eq_ends_kernel<NBv>, dim3((unsigned)((4 * lanes + 255) / 256), ni), dim3(256), stream, a, t))
            }
            MST_CHECK_LAUNCH("fxi_eq_ends_kernel");
            const dim3 sg((unsigned)a.n_seq);
            const double *ends = a.ends;
            double *starts = scratch + states;
            if (biquad_scan_threads(nchunks) == 512) {
                MST_BANDS_SWITCH(n_bands, MST_LAUNCH((fxi_eq_scan_kernel<NBv, 512>), sg, dim3(512), stream, ends, starts, t, C, (int)nchunks))
            } else {
                MST_BANDS_SWITCH(n_bands, MST_LAUNCH((fxi_eq_scan_kernel<NBv, 256>), sg, dim3(256), stream, ends, starts, t, C, (int)nchunks))
            }
            MST_CHECK_LAUNCH("fxi_eq_scan_kernel");
            if (C == 2 && !eq_lane_apply) {
                MST_BANDS_SWITCH(n_bands, MST_LAUNCH(fxi_eq_stereo_apply_kernel<NBv>, dim3((unsigned)((nchunks + 127) / 128), ni), dim3(256), stream, a, t))
            } else {
                MST_BANDS_SWITCH(n_bands, MST_LAUNCH(fxi_eq_chunk_apply_kernel<NBv>, dim3((unsigned)((lanes + 63) / 64), ni), dim3(64), stream, a, t))
            }
            MST_CHECK_LAUNCH("fxi_eq_apply_kernel");
            return MST_OK;
        }
    }
    if (fuse && (fuse->in_scale_dev || fuse->out_sumsq_dev || fuse->out_in_sumsq_dev))
        return fail(MST_ERR_UNSUPPORTED, "mst_fx_biquad_cascade_items: chain fusion needs the time-parallel path (scratch, more than one chunk, >= 1 band)");
    BiquadArgs a;
    a.x = x;
    a.y = y;
    a.n_seq = n_items * C;
    a.C = C;
    a.L = L;
    a.n_bands = n_bands;
    std::memset(a.coef, 0, sizeof(a.coef));
    MST_LAUNCH(fxi_eq_serial_kernel, dim3((unsigned)((a.n_seq + 63) / 64)), dim3(64), stream, a, coef_dev);
    MST_CHECK_LAUNCH("fxi_eq_serial_kernel");
    return MST_OK;
}

namespace {
// scratch = level differences [L][n_seq] (serial fallback only) | chunk maps [n_seq][nchunks][NP + 1] | chunk start values
// [nchunks][n_seq] | log10 table [256] | carry [n_seq] | energy partials of the apply pass [ceil(L / 64)][max(n_seq, 3 n_items)]
struct CompScratch { size_t xl, maps, ystart, tab, carry, tsums, total; long nchunks, ntiles; };
CompScratch comp_scratch(int n_items, long L, int C) {
    CompScratch c;
    const size_t n_seq = (size_t)n_items * C;
    c.nchunks = (L + MST_COMP_T - 1) / MST_COMP_T;
    c.xl = c.nchunks < 4 ? n_seq * (size_t)L * sizeof(double) : 0;      // only the serial form of very short signals stores them
    c.maps = n_seq * (size_t)c.nchunks * MST_COMP_REC * sizeof(double);
    c.ystart = n_seq * (size_t)c.nchunks * sizeof(double);
    c.tab = 256 * sizeof(double);
    c.carry = n_seq * sizeof(double);                                      // the smoother's value between two time slices of the chain
    c.ntiles = (L + 63) / 64;
    c.tsums = (size_t)c.ntiles * std::max(n_seq, (size_t)3 * n_items) * sizeof(double);      // the apply pass's energy partials per 64-sample tile
    c.total = c.xl + c.maps + c.ystart + c.tab + c.carry + c.tsums;
    return c;
}
}  // namespace

extern "C" size_t mst_fx_compressor_scratch_bytes(int n_items, long L, int C) {
    if (n_items < 1 || L < 1 || C < 1) return 0;
    return comp_scratch(n_items, L, C).total;
}

namespace {
// Conditioning of the time-parallel smoother ("FX passes").  The pieces of a chunk's map have slopes aA^(T-p) aR^p; the
// chain walk rebuilds intercepts and crossing inputs from the stored values by dividing by those slopes, so its start values carry the
// rounding of the stored values times kappa_T = (largest / smallest slope) = (max(aA, aR) / min(aA, aR))^T.  The start-value bound
//     C_START 2^-53 max|x_l| (min(L, 1 / (1 - max(aA, aR))) + kappa_T)
// times ln 10 / 20 (level -> relative gain) has to stay at or below 2^-27, a quarter of a float32 output ulp, with max|x_l| = 120 dB (the
// level difference of any sample between 1e-6 and 1e6 at any threshold in that range).  Beyond that the serial forms run.  The reach grows with L
// and the slower time constant: past about 6e5 samples of both (a release above ~14 s at 44.1 kHz on a signal that long - far outside any
// processor's range) the limit is negative and every such call is serial or refused whatever kappa: the recursion's own rounding has then used
// the quarter ulp up.
constexpr double FX_COMP_C_START = 8.0;
constexpr double FX_COMP_XL_MAX = 120.0;
double comp_kappa(double aA, double aR) {
    const double lo = std::min(aA, aR), hi = std::max(aA, aR);
    return lo > 0.0 ? std::pow(hi / lo, MST_COMP_T) : HUGE_VAL;
}
double comp_kappa_limit(double aA, double aR, long L) {
    const double amax = std::max(aA, aR);
    const double reach = amax < 1.0 ? std::min((double)L, 1.0 / (1.0 - amax)) : (double)L;
    return 0x1p-27 / (FX_COMP_C_START * 0x1p-53 * FX_COMP_XL_MAX * 0.11512925464970228420) - reach;
}
bool comp_well_conditioned(double aA, double aR, long L) { return comp_kappa(aA, aR) <= comp_kappa_limit(aA, aR, L); }
double comp_alpha(double sample_rate, double ms) { return std::exp(-1.0 / (0.001 * sample_rate * ms)); }
constexpr int FX_SLICES = 3;    // time slices of a large compressor call (compressor_run; measured: 0.523-0.539 ms per chain with 3, 0.540-0.550 with 4, 0.556-0.580 with 2, 0.67 with 8; profiles/r05_fx_slices_ab.txt)
int comp_slices(int nbatch, long n_seq, long L, bool slice_small) {
    return ((nbatch >= 32 && (double)n_seq * (double)L >= 4.0e6) || (slice_small && nbatch >= 8)) ? FX_SLICES : 1;
}
std::string comp_refusal(const char *who, double aA, double aR, long L) {
    char buf[320];
    std::snprintf(buf, sizeof(buf), "%s: attack / release coefficients %.6g / %.6g spread the chunk maps' slopes by kappa = %.3g, beyond the limit %.3g of "
                  "the time-parallel smoother; this call (chain fusion or parameter grid) has no serial form - use plain mst_fx_compressor calls",
                  who, aA, aR, comp_kappa(aA, aR), comp_kappa_limit(aA, aR, L));
    return buf;
}
}  // namespace

extern "C" int mst_fx_compressor_plan(int n_items, long L, int C, double attack_ms, double release_ms, double sample_rate, int forms,
                                      MstFxCompressorPlan *plan) {
    if (!plan || plan->struct_size != sizeof(MstFxCompressorPlan)) return fail(MST_ERR_ARG, "mst_fx_compressor_plan: MstFxCompressorPlan.struct_size does not match this library's layout");
    if (n_items < 1 || L < 1 || C < 1 || attack_ms <= 0 || release_ms <= 0 || sample_rate <= 0) return fail(MST_ERR_ARG, "mst_fx_compressor_plan: bad argument");
    const CompScratch cs = comp_scratch(n_items, L, C);
    const double aA = comp_alpha(sample_rate, attack_ms), aR = comp_alpha(sample_rate, release_ms);
    plan->nchunks = cs.nchunks;
    plan->nbatch = (cs.nchunks + MST_CHAIN_CB - 1) / MST_CHAIN_CB;
    plan->ntiles = cs.ntiles;
    plan->kappa = comp_kappa(aA, aR);
    plan->kappa_limit = comp_kappa_limit(aA, aR, L);
    plan->form = cs.nchunks < 4 ? MST_FX_COMP_SPLIT_SERIAL : (plan->kappa <= plan->kappa_limit ? MST_FX_COMP_TIME_PARALLEL : MST_FX_COMP_WAVE_SERIAL);
    plan->nslices = plan->form == MST_FX_COMP_TIME_PARALLEL ? comp_slices((int)plan->nbatch, (long)n_items * C, L, (forms & MST_FX_FORM_COMP_SLICE_SMALL) != 0) : 1;
    plan->record_doubles = MST_COMP_REC;
    plan->xl_offset = 0;
    plan->maps_offset = cs.xl;
    plan->ystart_offset = cs.xl + cs.maps;
    plan->tab_offset = cs.xl + cs.maps + cs.ystart;
    plan->carry_offset = plan->tab_offset + cs.tab;
    plan->tsums_offset = plan->carry_offset + cs.carry;
    plan->total_bytes = cs.total;
    return MST_OK;
}

namespace {
// fx_log10_table_kernel's 256 doubles, one copy per device, made by the first compressor call there (kept for the life of the process)
const double *log10_table(void *stream) {
    static std::mutex mu;
    static double *tabs[64] = {};
    const int dev = mst_current_device();
    if (dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    if (!tabs[dev]) {
        double *t = nullptr;
        if (hipMalloc((void **)&t, 256 * sizeof(double)) != hipSuccess) return nullptr;
        MST_LAUNCH(fx_log10_table_kernel, dim3(1), dim3(128), stream, t);
        if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) {
            (void)hipFree(t);
            return nullptr;
        }
        tabs[dev] = t;
    }
    return tabs[dev];
}

// the side stream of the time-parallel FX kernels (compressor_run): one per device, non-blocking, lowest priority, with the events of one
// fork / join; kept for the life of the process
struct FxSide {
    hipStream_t stream = nullptr;
    hipEvent_t fork = nullptr, join = nullptr, map_done[8] = {}, chain_done[8] = {};
    std::mutex mu;
};
FxSide *fx_side() {
    static std::mutex mu;
    static FxSide *sides[64] = {};
    const int dev = mst_current_device();
    if (dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    if (!sides[dev]) {
        FxSide *f = new FxSide;
        int lo = 0, hi = 0;
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);          // lo = the numerically greatest = lowest priority
        bool ok = hipStreamCreateWithPriority(&f->stream, hipStreamNonBlocking, lo) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&f->fork, hipEventDisableTiming) == hipSuccess;
        ok = ok && hipEventCreateWithFlags(&f->join, hipEventDisableTiming) == hipSuccess;
        for (int i = 0; i < 8 && ok; ++i)
            ok = hipEventCreateWithFlags(&f->map_done[i], hipEventDisableTiming) == hipSuccess &&
                 hipEventCreateWithFlags(&f->chain_done[i], hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            delete f;
            return nullptr;
        }
        sides[dev] = f;
    }
    return sides[dev];
}

// the slope of the piece at sorted position p of a chunk map and its reciprocal; [0]: a chunk of T steps, [1]: a last chunk of n_last steps
void comp_slopes(double aA, double aR, int n_last, double (*slope)[MST_COMP_NP], double (*inv_slope)[MST_COMP_NP]) {
    for (int which = 0; which < 2; ++which) {
        const int n = which ? n_last : MST_COMP_T;
        for (int p = 0; p < MST_COMP_NP; ++p) {
            slope[which][p] = p <= n ? std::pow(aA, n - p) * std::pow(aR, p) : 0.0;
            inv_slope[which][p] = p <= n ? 1.0 / slope[which][p] : 0.0;
        }
    }
}

// items: mst_fx_compressor_items - attack / release coefficients and slope rows per item from the prepared table (every item vetted by
// mst_fx_compressor_items_prepare: no serial-only dispatch here), the same launches with the per-item kernels
int compressor_run(CompArgs a, int n_items, long L, int C, double *scratch, size_t scratch_bytes, void *stream, bool slice_small = false,
                   const FxiCmpTab *items = nullptr) {
    // a pass that meets a time constant has two kernels over one body (fx_kernels.h, fxb_comp_*): the per-item one takes the table last
    auto launch = [&](auto *shared, auto *per_item, dim3 grid, dim3 block, void *st, auto... args) {
        if (items) MST_LAUNCH(per_item, grid, block, st, args..., *items);
        else MST_LAUNCH(shared, grid, block, st, args...);
    };
    // the time-parallel smoother only where its chunk maps are well conditioned (one host comparison, comp_well_conditioned); beyond, the plain
    // call runs one wave per sequence; a call that form cannot serve (chain fusion, parameter grid) is refused, never answered with garbage
    const bool serial_only = !items && (L + MST_COMP_T - 1) / MST_COMP_T >= 4 && !comp_well_conditioned(a.alpha_att, a.alpha_rel, L);
    if (serial_only && (a.thr_items || a.in_scale || a.out_sumsq))
        return fail(MST_ERR_UNSUPPORTED, comp_refusal(a.thr_items ? "mst_fx_compressor_grid" : "mst_fx_compressor", a.alpha_att, a.alpha_rel, L));
    if (!scratch || serial_only) {
        launch(fx_compressor_kernel, fxi_cmp_serial_kernel, dim3((a.n_seq + 3) / 4), dim3(256), stream, a);
        MST_CHECK_LAUNCH("fx_compressor_kernel");
        return MST_OK;
    }
    if (scratch_bytes < mst_fx_compressor_scratch_bytes(n_items, L, C))
        return fail(MST_ERR_WORKSPACE, "mst_fx_compressor: scratch too small");
    if (a.out_ms && C != 2) return fail(MST_ERR_ARG, "mst_fx_compressor: mid / side energies need stereo items");
    const CompScratch cs = comp_scratch(n_items, L, C);
    const dim3 tiles((unsigned)cs.ntiles, (unsigned)((a.n_seq + 63) / 64));      // 64 x 64 (time x sequence) tiles
    double *tsums = (double *)((unsigned char *)scratch + cs.xl + cs.maps + cs.ystart + cs.tab + cs.carry);
    // the energy sums of the output (chain fusion): per-tile partials from the apply pass, reduced in a fixed order
    auto finish = [&]() -> int {
        if (!a.out_sumsq) return MST_OK;
        MST_LAUNCH(fx_tile_sums_kernel, dim3((unsigned)n_items), dim3(MST_TILE_SUBS * MST_SUMSQ_SLOTS), stream, (const double *)tsums, cs.ntiles, n_items, C,
                   a.out_ms ? 1 : 0, a.out_sumsq, a.out_ms);
        MST_CHECK_LAUNCH("fx_tile_sums_kernel");
        return MST_OK;
    };
    if (cs.nchunks < 4) {                               // very short signals: level differences, serial smoother, gain application
        MST_LAUNCH(fx_comp_gain_kernel, tiles, dim3(256), stream, a, scratch);
        MST_CHECK_LAUNCH("fx_comp_gain_kernel");
        launch(fx_comp_smooth_kernel, fxi_cmp_smooth_kernel, dim3((a.n_seq + 63) / 64), dim3(64), stream, a, scratch);
        MST_CHECK_LAUNCH("fx_comp_smooth_kernel");
        MST_LAUNCH((fx_comp_apply_kernel<false>), tiles, dim3(256), stream, a, (const double *)scratch, (const double *)nullptr, 0, 0, tsums);
        MST_CHECK_LAUNCH("fx_comp_apply_kernel");
        return finish();
    }
    // the smoother parallel in time: chunk maps (convex piecewise-linear), a chain over chunks, the rest in one pass
    CompMapArgs m;
    const double *tab = log10_table(stream);          // a constant of the device: built on first use
    if (!tab) return fail(MST_ERR_HIP, "mst_fx_compressor: log10 table");
    m.log_tab = tab;
    m.maps = (double *)((unsigned char *)scratch + cs.xl);
    m.ystart = (double *)((unsigned char *)scratch + cs.xl + cs.maps);
    m.n_seq = a.n_seq;
    m.nchunks = (int)cs.nchunks;
    m.L = L;
    m.aA = a.alpha_att;
    m.aR = a.alpha_rel;
    m.use_min = a.alpha_att > a.alpha_rel ? 1 : 0;
    // the piece at sorted position p of a chunk of n steps has been through n - p attack and p release steps
    const int n_last = (int)(L - (cs.nchunks - 1) * MST_COMP_T);
    comp_slopes(m.aA, m.aR, n_last, m.slope, m.inv_slope);
    m.ycarry = (double *)((unsigned char *)scratch + cs.xl + cs.maps + cs.ystart + cs.tab);
    // Time slices.  The chain is ONE dependent walk per sequence (n_seq workgroups, latency-bound: most of the chip idles beside it) while
    // the map and apply kernels are throughput work.  The signal is cut into FX_SLICES (three) slices of whole chain batches; the caller's
    // stream runs the chain of slice 0, 1, ... back to back, a side stream (lower priority) the maps of slice 1, 2, ... and the applies of slice
    // 0 .. NS - 2 beside it (events order map_i -> chain_i -> apply_i); the last apply follows the last chain on the caller's stream, which
    // then waits for the side stream.  Same arithmetic, same results (the smoother's value crosses a slice boundary as a float64 in
    // ycarry); without concurrency (a profiler serialising the queues) the launches simply run one after the other.
    // (Round 6 measured two other ways of overlapping the three kernels - the tail inside the chain kernel, and ONE chain launch that polls
    //  the map kernel's progress counters with the apply kernel polling the chain's: 0.74 and 0.51 ms per chain against 0.49 with the slices;
    //  EXPERIMENTS.md section E.3, tools/proto/r06_fx_*.)
    const int nbatch = (int)((cs.nchunks + MST_CHAIN_CB - 1) / MST_CHAIN_CB);
    const int gy = (a.n_seq + 63) / 64;
    int ns = comp_slices(nbatch, a.n_seq, L, slice_small);
    FxSide *side = ns > 1 ? fx_side() : nullptr;
    if (!side) ns = 1;
    auto launch_map = [&](int b0, int b1, void *st) -> int {
        CompMapArgs mm = m;
        mm.chunk0 = b0 * MST_CHAIN_CB;
        const long c1 = std::min<long>((long)b1 * MST_CHAIN_CB, cs.nchunks);
        const dim3 cg((unsigned)(c1 - mm.chunk0), (unsigned)gy);
        launch(m.use_min ? fx_comp_map_kernel<true> : fx_comp_map_kernel<false>, fxi_cmp_map_kernel, cg, dim3(64), st, mm, a);
        MST_CHECK_LAUNCH("fx_comp_map_kernel");
        return MST_OK;
    };
    auto launch_chain = [&](int b0, int b1, void *st) -> int {
        CompMapArgs mm = m;
        mm.batch0 = b0;
        mm.batch1 = b1;
        launch(fx_comp_chain_kernel, fxi_cmp_chain_kernel, dim3(a.n_seq), dim3(MST_CHAIN_THREADS), st, mm);
        MST_CHECK_LAUNCH("fx_comp_chain_kernel");
        return MST_OK;
    };
    auto launch_apply = [&](int b0, int b1, void *st) -> int {      // a batch is 32 chunks = 16 time tiles of 64 samples
        const long t0 = (long)b0 * (MST_CHAIN_CB / 2), t1 = std::min<long>((long)b1 * (MST_CHAIN_CB / 2), (long)tiles.x);
        launch(fx_comp_apply_kernel<true>, fxi_cmp_apply_kernel<true>, dim3((unsigned)(t1 - t0), tiles.y), dim3(256), st, a, tab, (const double *)m.ystart, m.nchunks, (int)t0, tsums);
        MST_CHECK_LAUNCH("fx_comp_apply_kernel");
        return MST_OK;
    };
    static_assert(MST_COMP_T == 32 && MST_CHAIN_CB % 2 == 0, "two chunks per 64-sample apply tile");
    int rc;
    if (ns == 1) {
        if ((rc = launch_map(0, nbatch, stream)) || (rc = launch_chain(0, nbatch, stream)) || (rc = launch_apply(0, nbatch, stream))) return rc;
        return finish();
    }
    std::lock_guard<std::mutex> lock(side->mu);          // one fork / join at a time per device: the events are reused
    hipStream_t main_s = (hipStream_t)stream, side_s = side->stream;
    auto bound = [&](int i) { return (int)((long)nbatch * i / ns); };
    if ((rc = launch_map(0, bound(1), stream))) return rc;          // slice 0's map: nothing to overlap it with
    MST_HIP_TRY(hipEventRecord(side->fork, main_s));               // the side stream sees the input
    MST_HIP_TRY(hipStreamWaitEvent(side_s, side->fork, 0));
    // From here on the side stream may hold work on the caller's buffers.  Whatever goes wrong below, the caller's stream is made to wait
    // for it before this call returns (torch's allocator hands the buffers to the next user of the CALLER's stream).
    auto forked = [&]() -> int {
        int r;
        hipError_t e;
        for (int i = 1; i < ns; ++i) {
            if ((r = launch_map(bound(i), bound(i + 1), side_s))) return r;
            if ((e = hipEventRecord(side->map_done[i], side_s)) != hipSuccess) return fail(MST_ERR_HIP, std::string("hipEventRecord: ") + hipGetErrorString(e));
        }
        for (int i = 0; i < ns; ++i) {
            if (i > 0 && (e = hipStreamWaitEvent(main_s, side->map_done[i], 0)) != hipSuccess) return fail(MST_ERR_HIP, std::string("hipStreamWaitEvent: ") + hipGetErrorString(e));
            if ((r = launch_chain(bound(i), bound(i + 1), stream))) return r;
            if (i + 1 < ns) {
                if ((e = hipEventRecord(side->chain_done[i], main_s)) != hipSuccess || (e = hipStreamWaitEvent(side_s, side->chain_done[i], 0)) != hipSuccess)
                    return fail(MST_ERR_HIP, std::string("chain -> apply event: ") + hipGetErrorString(e));
                if ((r = launch_apply(bound(i), bound(i + 1), side_s))) return r;
            }
        }
        return launch_apply(bound(ns - 1), nbatch, stream);
    };
    rc = forked();
    hipError_t e = hipEventRecord(side->join, side_s);
    if (e == hipSuccess) e = hipStreamWaitEvent(main_s, side->join, 0);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(side_s);            // the join could not be expressed as an event: wait for the side stream here
        if (rc == MST_OK) rc = fail(MST_ERR_HIP, std::string("mst_fx_compressor: side stream join: ") + hipGetErrorString(e));
    }
    return rc ? rc : finish();
}
}  // namespace

extern "C" int mst_fx_compressor(const float *x, float *y, int n_items, long L, int C, double threshold_db,
                                 double attack_ms, double release_ms, double ratio, double sample_rate, double *scratch,
                                 size_t scratch_bytes, const MstFxFuse *fuse, void *stream) {
    if (!x || !y || n_items < 1 || L < 1 || C < 1 || attack_ms <= 0 || release_ms <= 0 || ratio <= 0 || sample_rate <= 0)
        return fail(MST_ERR_ARG, "mst_fx_compressor: bad argument");
    if (int rc = fuse_check(fuse, "mst_fx_compressor")) return rc;
    const bool fused = fuse && (fuse->in_scale_dev || fuse->out_sumsq_dev);
    if (fuse && (fuse->post_rms || fuse->out_in_sumsq_dev))
        return fail(MST_ERR_UNSUPPORTED, "mst_fx_compressor: tail folding (post_rms) is the imager's, out_in_sumsq_dev the equaliser's");
    if (fused && (!scratch || (threshold_db == 0.0 && ratio == 1.0)))
        return fail(MST_ERR_UNSUPPORTED, "mst_fx_compressor: chain fusion needs the scratch buffer and an active compressor");
    if (threshold_db == 0.0 && ratio == 1.0) {   // bypass (common_audioeffects.py:637)
        if (x != y) MST_HIP_TRY(hipMemcpyAsync(y, x, (size_t)n_items * L * C * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
        return MST_OK;
    }
    CompArgs a;
    a.x = x;
    a.y = y;
    a.n_seq = n_items * C;
    a.C = C;
    a.L = L;
    a.threshold = threshold_db;
    a.ratio = ratio;
    a.alpha_att = comp_alpha(sample_rate, attack_ms);
    a.alpha_rel = comp_alpha(sample_rate, release_ms);
    a.makeup = 0.0;
    a.in_scale = fuse ? fuse->in_scale_dev : nullptr;
    a.out_sumsq = fuse ? fuse->out_sumsq_dev : nullptr;
    if (fuse && fuse->in_ms_dev) return fail(MST_ERR_UNSUPPORTED, "mst_fx_compressor: in_ms_dev is the imager's");
    if (fuse && fuse->out_ms_dev) {
        if (C != 2 || !fuse->out_sumsq_dev) return fail(MST_ERR_UNSUPPORTED, "mst_fx_compressor: out_ms_dev needs stereo audio and out_sumsq_dev");
        a.out_ms = fuse->out_ms_dev;
    }
    return compressor_run(a, n_items, L, C, scratch, scratch_bytes, stream, fuse && (fuse->forms & MST_FX_FORM_COMP_SLICE_SMALL));
}

extern "C" int mst_fx_compressor_grid(const float *x, float *y, int n_items, long L, int C, const double *threshold_db_dev,
                                      const double *ratio_dev, double attack_ms, double release_ms, double sample_rate,
                                      double *scratch, size_t scratch_bytes, double *peak_dev, void *stream) {
    if (!x || !y || !threshold_db_dev || !ratio_dev || !scratch || n_items < 1 || L < 1 || C < 1 || attack_ms <= 0 ||
        release_ms <= 0 || sample_rate <= 0)
        return fail(MST_ERR_ARG, "mst_fx_compressor_grid: bad argument");
    CompArgs a;
    a.x = x;
    a.y = y;
    a.n_seq = n_items * C;
    a.C = C;
    a.L = L;
    a.threshold = 0.0;
    a.ratio = 1.0;
    a.thr_items = threshold_db_dev;
    a.ratio_items = ratio_dev;
    a.shared_x = 1;
    a.alpha_att = comp_alpha(sample_rate, attack_ms);
    a.alpha_rel = comp_alpha(sample_rate, release_ms);
    a.makeup = 0.0;
    int rc;
    if ((rc = compressor_run(a, n_items, L, C, scratch, scratch_bytes, stream))) return rc;
    if (peak_dev) {          // `compress` clips a candidate whose peak reaches 1 (utils_data_normalization.py:352-353)
        MST_LAUNCH(fx_item_peak_kernel, dim3(64, n_items), dim3(256), stream, (const float *)y, L * C, peak_dev);
        MST_CHECK_LAUNCH("fx_item_peak_kernel");
        MST_LAUNCH(fx_clip_if_kernel, dim3((unsigned)((L * C + 255) / 256), n_items), dim3(256), stream, y, L * C, (const double *)peak_dev);
        MST_CHECK_LAUNCH("fx_clip_if_kernel");
    }
    return MST_OK;
}

// ---- per-item parameters: the compressor ---------------------------------------------------------------------------------------------------
// table (float64): thr [n] | ratio [n] | aA [n] | aR [n] | slope [n][2][NP] | inv_slope [n][2][NP]
extern "C" size_t mst_fx_compressor_items_table_bytes(int n_items) {
    return n_items < 1 ? 0 : (size_t)n_items * (4 + 4 * MST_COMP_NP) * sizeof(double);
}

extern "C" int mst_fx_compressor_items_prepare(const double *params_host, int n_items, long L, int C, double sample_rate, int forms,
                                               double *table_host, size_t table_bytes, int *first_refused_item) {
    if (first_refused_item) *first_refused_item = -1;
    if (!params_host || !table_host || n_items < 1 || L < 1 || C < 1 || sample_rate <= 0) return fail(MST_ERR_ARG, "mst_fx_compressor_items_prepare: bad argument");
    if (forms & ~(MST_FX_FORM_EQ_LANE_APPLY | MST_FX_FORM_EQ_VALU_ENDS | MST_FX_FORM_COMP_SLICE_SMALL)) return fail(MST_ERR_ARG, "mst_fx_compressor_items_prepare: unknown forms bits");
    if (table_bytes < mst_fx_compressor_items_table_bytes(n_items)) return fail(MST_ERR_WORKSPACE, "mst_fx_compressor_items_prepare: table too small");
    const long nchunks = (L + MST_COMP_T - 1) / MST_COMP_T;
    const int n_last = (int)(L - (nchunks - 1) * MST_COMP_T);
    const size_t n = (size_t)n_items;
    double *thr = table_host, *ratio = thr + n, *aA = ratio + n, *aR = aA + n, *slope = aR + n, *inv = slope + n * 2 * MST_COMP_NP;
    for (int i = 0; i < n_items; ++i) {
        const double *p = params_host + 4 * (size_t)i;
        char buf[160];
        if (!(p[1] > 0) || !(p[2] > 0) || !(p[3] > 0)) {
            std::snprintf(buf, sizeof(buf), "mst_fx_compressor_items_prepare: item %d: attack, release and ratio must be positive", i);
            if (first_refused_item) *first_refused_item = i;
            return fail(MST_ERR_ARG, buf);
        }
        if (p[0] == 0.0 && p[3] == 1.0) {          // Compressor.process returns its input for this pair (:637): not a compressor call
            std::snprintf(buf, sizeof(buf), "mst_fx_compressor_items_prepare: item %d is the bypass (threshold 0 dB, ratio 1): leave it out of the batch", i);
            if (first_refused_item) *first_refused_item = i;
            return fail(MST_ERR_UNSUPPORTED, buf);
        }
        thr[i] = p[0];
        ratio[i] = p[3];
        aA[i] = comp_alpha(sample_rate, p[1]);
        aR[i] = comp_alpha(sample_rate, p[2]);
        if (nchunks >= 4 && !comp_well_conditioned(aA[i], aR[i], L)) {          // mst_fx_compressor_plan's rule, per item
            if (first_refused_item) *first_refused_item = i;
            std::snprintf(buf, sizeof(buf), "mst_fx_compressor_items_prepare: item %d", i);
            return fail(MST_ERR_UNSUPPORTED, comp_refusal(buf, aA[i], aR[i], L));
        }
        comp_slopes(aA[i], aR[i], n_last, (double (*)[MST_COMP_NP])(slope + (size_t)i * 2 * MST_COMP_NP), (double (*)[MST_COMP_NP])(inv + (size_t)i * 2 * MST_COMP_NP));
    }
    return MST_OK;
}

extern "C" int mst_fx_compressor_items(const float *x, float *y, int n_items, long L, int C, const double *table_dev, double *scratch,
                                       size_t scratch_bytes, const MstFxFuse *fuse, void *stream) {
    if (!x || !y || !table_dev || n_items < 1 || L < 1 || C < 1) return fail(MST_ERR_ARG, "mst_fx_compressor_items: bad argument");
    if (int rc = fuse_check(fuse, "mst_fx_compressor_items")) return rc;
    const bool fused = fuse && (fuse->in_scale_dev || fuse->out_sumsq_dev);
    if (fuse && (fuse->post_rms || fuse->out_in_sumsq_dev))
        return fail(MST_ERR_UNSUPPORTED, "mst_fx_compressor_items: tail folding (post_rms) is the imager's, out_in_sumsq_dev the equaliser's");
    if (fused && !scratch) return fail(MST_ERR_UNSUPPORTED, "mst_fx_compressor_items: chain fusion needs the scratch buffer");
    if (fuse && fuse->in_ms_dev) return fail(MST_ERR_UNSUPPORTED, "mst_fx_compressor_items: in_ms_dev is the imager's");
    const size_t n = (size_t)n_items;
    CompArgs a;
    a.x = x;
    a.y = y;
    a.n_seq = n_items * C;
    a.C = C;
    a.L = L;
    a.threshold = 0.0;
    a.ratio = 1.0;
    a.thr_items = table_dev;
    a.ratio_items = table_dev + n;
    a.alpha_att = 0.0;          // per item: FxiCmpTab
    a.alpha_rel = 0.0;
    a.makeup = 0.0;
    a.in_scale = fuse ? fuse->in_scale_dev : nullptr;
    a.out_sumsq = fuse ? fuse->out_sumsq_dev : nullptr;
    if (fuse && fuse->out_ms_dev) {
        if (C != 2 || !fuse->out_sumsq_dev) return fail(MST_ERR_UNSUPPORTED, "mst_fx_compressor_items: out_ms_dev needs stereo audio and out_sumsq_dev");
        a.out_ms = fuse->out_ms_dev;
    }
    FxiCmpTab t;
    t.aA = table_dev + 2 * n;
    t.aR = table_dev + 3 * n;
    t.slope = table_dev + 4 * n;
    t.inv = t.slope + n * 2 * MST_COMP_NP;
    t.C = C;
    return compressor_run(a, n_items, L, C, scratch, scratch_bytes, stream, fuse && (fuse->forms & MST_FX_FORM_COMP_SLICE_SMALL), &t);
}

extern "C" int mst_fx_range_reduce(const float *x, long L, int C, int channel, const int *item_dev, const long *lo_dev,
                                   const long *hi_dev, int n_ranges, int mode, double *out_dev, void *stream) {
    if (!x || !item_dev || !lo_dev || !hi_dev || !out_dev || L < 1 || C < 1 || channel < 0 || channel >= C || n_ranges < 1 ||
        (mode != 0 && mode != 1))
        return fail(MST_ERR_ARG, "mst_fx_range_reduce: bad argument");
    MST_LAUNCH(fx_range_reduce_kernel, dim3(n_ranges), dim3(256), stream, x, L, C, channel, item_dev, lo_dev, hi_dev, mode, out_dev);
    MST_CHECK_LAUNCH("fx_range_reduce_kernel");
    return MST_OK;
}

extern "C" int mst_fx_onset_hfc(const float *x, int n_items, long L, int C, int channel, int win, float *out_dev, void *stream) {
    if (!x || !out_dev || n_items < 1 || L < 1 || C < 1 || channel < 0 || channel >= C)
        return fail(MST_ERR_ARG, "mst_fx_onset_hfc: bad argument");
    if (win != 256 && win != 512 && win != 1024 && win != 2048)
        return fail(MST_ERR_UNSUPPORTED, "mst_fx_onset_hfc: window must be 256, 512, 1024 or 2048 samples");
    const long n_frames = L / win;          // whole frames only (librosa.util.frame)
    if (n_frames < 1) return MST_OK;
    const dim3 grid((unsigned)(n_frames * n_items));
    switch (win) {
        case 256: MST_LAUNCH((fx_onset_hfc_kernel<256>), grid, dim3(256), stream, x, L, C, channel, n_frames, (float2 *)out_dev); break;
        case 512: MST_LAUNCH((fx_onset_hfc_kernel<512>), grid, dim3(256), stream, x, L, C, channel, n_frames, (float2 *)out_dev); break;
        case 1024: MST_LAUNCH((fx_onset_hfc_kernel<1024>), grid, dim3(256), stream, x, L, C, channel, n_frames, (float2 *)out_dev); break;
        default: MST_LAUNCH((fx_onset_hfc_kernel<2048>), grid, dim3(256), stream, x, L, C, channel, n_frames, (float2 *)out_dev); break;
    }
    MST_CHECK_LAUNCH("fx_onset_hfc_kernel");
    return MST_OK;
}

namespace {
int energy(const float *x, double *acc, int n_items, long per_item, int mode, void *stream) {
    MST_HIP_TRY(hipMemsetAsync(acc, 0, (size_t)n_items * 2 * sizeof(double), (hipStream_t)stream));
    const long frames = mode == 1 ? per_item / 2 : per_item;
    int chunks = (int)std::min<long>(64, (frames + 8191) / 8192);
    if (chunks < 1) chunks = 1;
    MST_LAUNCH(fx_energy_kernel, dim3(n_items * chunks), dim3(256), stream, x, acc, per_item, mode, chunks);
    MST_CHECK_LAUNCH("fx_energy_kernel");
    return MST_OK;
}

// what mst_fx_midside_imager and mst_fx_midside_imager_items (who) do ahead of their apply launch: the refusals of a fuse they cannot serve,
// then the mid / side energy parts the apply pass reads
int imager_parts(const char *who, const float *x, int n_items, long L, double *scratch, const MstFxFuse *fuse, void *stream, const double **parts,
                 int *chunks) {
    if (int rc = fuse_check(fuse, who)) return rc;
    if (fuse && fuse->out_in_sumsq_dev) return fail(MST_ERR_UNSUPPORTED, std::string(who) + ": out_in_sumsq_dev is the equaliser's");
    if (fuse && fuse->post_rms && !fuse->in_sumsq_dev) return fail(MST_ERR_ARG, std::string(who) + ": post_rms needs in_sumsq_dev");
    if (fuse && fuse->out_ms_dev) return fail(MST_ERR_UNSUPPORTED, std::string(who) + ": out_ms_dev is the compressor's");
    *chunks = (int)std::min<long>(MST_SUMSQ_SLOTS, (L + 8191) / 8192);
    if (*chunks < 1) *chunks = 1;
    *parts = scratch;
    if (fuse && fuse->in_ms_dev) {          // the producer of x (the compressor's apply pass) left the mid / side energies behind: no energy pass
        *parts = fuse->in_ms_dev;
        *chunks = MST_SUMSQ_SLOTS;
    } else {
        MST_LAUNCH(fx_energy_parts_kernel, dim3(n_items * *chunks), dim3(256), stream, x, scratch, L, *chunks);
        MST_CHECK_LAUNCH("fx_energy_parts_kernel");
    }
    return MST_OK;
}
// mst_fx_gain and mst_fx_gain_items (who) take in_scale_dev from a fuse and nothing else
int gain_fuse_check(const MstFxFuse *fuse, const char *who) {
    if (int rc = fuse_check(fuse, who)) return rc;
    if (fuse && (fuse->post_rms || fuse->out_in_sumsq_dev || fuse->out_ms_dev || fuse->in_ms_dev))
        return fail(MST_ERR_UNSUPPORTED, std::string(who) + ": tail folding (post_rms) is the imager's, out_in_sumsq_dev the equaliser's, the mid / side energies the compressor's / imager's");
    return MST_OK;
}
}  // namespace

extern "C" int mst_fx_midside_imager(const float *x, float *y, int n_items, long L, double bal, double *scratch, const MstFxFuse *fuse,
                                     void *stream) {
    if (!x || !y || !scratch || n_items < 1 || L < 1) return fail(MST_ERR_ARG, "mst_fx_midside_imager: bad argument");
    const double *parts;
    int chunks;
    if (int rc = imager_parts("mst_fx_midside_imager", x, n_items, L, scratch, fuse, stream, &parts, &chunks)) return rc;
    const bool fold = fuse && fuse->post_rms;
    const double bal_r = std::round(bal * 1000.0) / 1000.0;   // round(bal, 3) (:980)
    MST_LAUNCH(fx_imager_apply_kernel, dim3((unsigned)((L + MST_IMAGER_FRAMES - 1) / MST_IMAGER_FRAMES), n_items), dim3(256), stream, x, y,
               parts, chunks, L, bal_r, fuse ? fuse->in_scale_dev : (const double *)nullptr,
               fuse ? fuse->out_sumsq_dev : (double *)nullptr, fold ? fuse->in_sumsq_dev : (const double *)nullptr,
               fold ? fuse->post_gain : 1.0f);
    MST_CHECK_LAUNCH("fx_imager_apply_kernel");
    return MST_OK;
}

extern "C" int mst_fx_gain(const float *x, float *y, int n_items, long L, int C, double gain_db, int invert, const MstFxFuse *fuse,
                           void *stream) {
    if (!x || !y || n_items < 1 || L < 1 || C < 1) return fail(MST_ERR_ARG, "mst_fx_gain: bad argument");
    if (int rc = gain_fuse_check(fuse, "mst_fx_gain")) return rc;
    const long per = L * C;
    MST_LAUNCH(fx_scale_kernel, dim3((unsigned)((per + 255) / 256), n_items), dim3(256), stream, x, y, per, fx_gain_factor(gain_db, invert),
               (const double *)nullptr, (const double *)nullptr, 0, per, fuse ? fuse->in_scale_dev : (const double *)nullptr);
    MST_CHECK_LAUNCH("fx_scale_kernel");
    return MST_OK;
}

extern "C" int mst_fx_midside_imager_items(const float *x, float *y, int n_items, long L, const double *bal_dev, double *scratch,
                                           const float *post_gain_dev, const MstFxFuse *fuse, void *stream) {
    if (!x || !y || !scratch || !bal_dev || n_items < 1 || n_items > 65535 || L < 1) return fail(MST_ERR_ARG, "mst_fx_midside_imager_items: bad argument");
    const double *parts;
    int chunks;
    if (int rc = imager_parts("mst_fx_midside_imager_items", x, n_items, L, scratch, fuse, stream, &parts, &chunks)) return rc;
    const bool fold = fuse && fuse->post_rms;
    MST_LAUNCH(fxi_imager_apply_kernel, dim3((unsigned)((L + MST_IMAGER_FRAMES - 1) / MST_IMAGER_FRAMES), n_items), dim3(256), stream, x, y,
               parts, chunks, L, bal_dev, fuse ? fuse->in_scale_dev : (const double *)nullptr,
               fuse ? fuse->out_sumsq_dev : (double *)nullptr, fold ? fuse->in_sumsq_dev : (const double *)nullptr,
               fold ? post_gain_dev : (const float *)nullptr, fold ? fuse->post_gain : 1.0f);
    MST_CHECK_LAUNCH("fxi_imager_apply_kernel");
    return MST_OK;
}

extern "C" int mst_fx_gain_items(const float *x, float *y, int n_items, long L, int C, const double *gain_db_dev, const int *invert_dev,
                                 const MstFxFuse *fuse, void *stream) {
    if (!x || !y || !gain_db_dev || n_items < 1 || n_items > 65535 || L < 1 || C < 1) return fail(MST_ERR_ARG, "mst_fx_gain_items: bad argument");
    if (int rc = gain_fuse_check(fuse, "mst_fx_gain_items")) return rc;
    const long per = L * C;
    MST_LAUNCH(fxi_gain_kernel, dim3((unsigned)((per + 255) / 256), n_items), dim3(256), stream, x, y, per, gain_db_dev, invert_dev,
               fuse ? fuse->in_scale_dev : (const double *)nullptr);
    MST_CHECK_LAUNCH("fxi_gain_kernel");
    return MST_OK;
}

extern "C" int mst_fx_haas(const float *x, float *y, int n_items, long L, int c_in, long delay, double feedback,
                           int wet_channel, void *stream) {
    if (!x || !y || n_items < 1 || L < 1) return fail(MST_ERR_ARG, "mst_fx_haas: bad argument");
    if (c_in != 1 && c_in != 2) return fail(MST_ERR_ARG, "mst_fx_haas: Haas effect only works with monaural or stereo audio");
    if (wet_channel != 0 && wet_channel != 1) return fail(MST_ERR_ARG, "mst_fx_haas: wet_channel must be 0 (left) or 1 (right)");
    if (x == y) return fail(MST_ERR_ARG, "mst_fx_haas: in-place operation is not supported (circular read)");
    long shift = delay % L;
    if (shift < 0) shift += L;
    MST_LAUNCH(fx_haas_kernel, dim3((unsigned)((L + 255) / 256), n_items), dim3(256), stream, x, y, L, c_in, shift,
               (float)feedback, wet_channel);
    MST_CHECK_LAUNCH("fx_haas_kernel");
    return MST_OK;
}

extern "C" int mst_fx_panner(const float *x, float *y, int n_items, long L, int c_in, float g0, float g1, void *stream) {
    if (!x || !y || n_items < 1 || L < 1) return fail(MST_ERR_ARG, "mst_fx_panner: bad argument");
    if (c_in != 1 && c_in != 2) return fail(MST_ERR_ARG, "mst_fx_panner: Panner only works with monaural or stereo audio");
    if (x == y && c_in != 2) return fail(MST_ERR_ARG, "mst_fx_panner: in-place needs a stereo input");
    MST_LAUNCH(fx_panner_kernel, dim3((unsigned)((L + 255) / 256), n_items), dim3(256), stream, x, y, L, c_in, g0, g1);
    MST_CHECK_LAUNCH("fx_panner_kernel");
    return MST_OK;
}

extern "C" int mst_fx_panner_items(const float *x, float *y, int n_items, long L, int c_in, const float *gains_dev, void *stream) {
    if (!x || !y || !gains_dev || n_items < 1 || n_items > 65535 || L < 1) return fail(MST_ERR_ARG, "mst_fx_panner_items: bad argument");
    if (c_in != 1 && c_in != 2) return fail(MST_ERR_ARG, "mst_fx_panner_items: Panner only works with monaural or stereo audio");
    if (x == y && c_in != 2) return fail(MST_ERR_ARG, "mst_fx_panner_items: in-place needs a stereo input");
    MST_LAUNCH(fxsi_panner_kernel, dim3((unsigned)((L + 255) / 256), n_items), dim3(256), stream, x, y, L, c_in, gains_dev);
    MST_CHECK_LAUNCH("fxsi_panner_kernel");
    return MST_OK;
}

extern "C" int mst_fx_haas_items(const float *x, float *y, int n_items, long L, int c_in, const long *delay_dev, const double *feedback_dev,
                                 const int *wet_channel_dev, void *stream) {
    if (!x || !y || !delay_dev || !feedback_dev || !wet_channel_dev || n_items < 1 || n_items > 65535 || L < 1)
        return fail(MST_ERR_ARG, "mst_fx_haas_items: bad argument");
    if (c_in != 1 && c_in != 2) return fail(MST_ERR_ARG, "mst_fx_haas_items: Haas effect only works with monaural or stereo audio");
    if (x == y) return fail(MST_ERR_ARG, "mst_fx_haas_items: in-place operation is not supported (circular read)");
    MST_LAUNCH(fxsi_haas_kernel, dim3((unsigned)((L + 255) / 256), n_items), dim3(256), stream, x, y, L, c_in, delay_dev, feedback_dev,
               wet_channel_dev);
    MST_CHECK_LAUNCH("fxsi_haas_kernel");
    return MST_OK;
}

// ---- power-of-two real FFTs (csrc/fft_kernels.h): plans for the FFT convolution and the STFT ---------------------------------------
struct MstFftPlan {
    long n = 0, m = 0;              // transform length, m = n / 2 complex points
    int log2m = 0;
    int passes = 0;                 // Stockham passes: log2(m) / 2 of radix 4, one of radix 2 in front when log2(m) is odd
    float2 *tw_m = nullptr;         // exp(-2 pi i j / m), j < m / 2
    float2 *tw_n = nullptr;         // exp(-2 pi i k / n), k <= m / 2
};

namespace {
void fft_plan_destroy(MstFftPlan *p) {
    if (!p) return;
    (void)hipFree(p->tw_m);
    (void)hipFree(p->tw_n);
    delete p;
}
// n: a power of two >= 4.  The twiddle tables are written on the null stream and waited for: plans are made once.
constexpr long MST_FFT_MAX_N = 1L << 21;          // the four-step kernels' largest transform (fft_kernels.h: LOGMAX 10 columns x 10 rows of complex points)
int fft_plan_create(MstFftPlan **out, long n) {
    if (n < 4 || (n & (n - 1)) || n > MST_FFT_MAX_N) return fail(MST_ERR_UNSUPPORTED, "FFT length must be a power of two in 4 ... 2^21");
    auto *p = new MstFftPlan;
    p->n = n;
    p->m = n / 2;
    for (long v = p->m; v > 1; v >>= 1) p->log2m++;
    p->passes = p->log2m >= 8 ? 2 : p->log2m / 2 + p->log2m % 2;          // four-step form (two kernels) from 256 complex points on
    const long cm = std::max<long>(1, p->m / 2), cn = p->m / 2 + 1;
    if (hipMalloc((void **)&p->tw_m, (size_t)cm * sizeof(float2)) != hipSuccess || hipMalloc((void **)&p->tw_n, (size_t)cn * sizeof(float2)) != hipSuccess) {
        fft_plan_destroy(p);
        return fail(MST_ERR_HIP, "FFT plan: hipMalloc failed");
    }
    MST_LAUNCH(fft_twiddle_kernel, dim3((unsigned)((cm + 255) / 256)), dim3(256), nullptr, p->tw_m, p->m, cm);
    MST_LAUNCH(fft_twiddle_kernel, dim3((unsigned)((cn + 255) / 256)), dim3(256), nullptr, p->tw_n, p->n, cn);
    if (hipStreamSynchronize(nullptr) != hipSuccess) {
        fft_plan_destroy(p);
        return fail(MST_ERR_HIP, "FFT plan: twiddle kernels failed");
    }
    *out = p;
    return MST_OK;
}
// the size-m complex FFT of nb sequences, ping-pong between a (stride sa) and b (stride sb), starting in `a`; returns where the result is
int fft_passes(const MstFftPlan *p, float2 *a, long sa, float2 *b, long sb, int nb, int inverse, void *stream, float2 **res, long *sres) {
    float2 *src = a, *dst = b;
    long ss = sa, sd = sb;
    if (p->log2m >= 8) {          // four-step: columns (a -> b), rows (b -> a)
        const int l1 = (p->log2m + 1) / 2, l2 = p->log2m - l1;
        const dim3 ga((unsigned)((1L << l2) / 16), (unsigned)nb), gb((unsigned)((1L << l1) / 16), (unsigned)nb);
#define MST_FFT_STEP(KERN, GRID, LG)                                                                                                         \
    if ((LG) <= 6) MST_LAUNCH((KERN<6>), GRID, dim3(256), stream, (const float2 *)src, dst, (const float2 *)p->tw_m, p->m, l1, l2, ss, sd, inverse); \
    else if ((LG) <= 8) MST_LAUNCH((KERN<8>), GRID, dim3(256), stream, (const float2 *)src, dst, (const float2 *)p->tw_m, p->m, l1, l2, ss, sd, inverse); \
    else if ((LG) <= 9) MST_LAUNCH((KERN<9>), GRID, dim3(256), stream, (const float2 *)src, dst, (const float2 *)p->tw_m, p->m, l1, l2, ss, sd, inverse); \
    else MST_LAUNCH((KERN<10>), GRID, dim3(256), stream, (const float2 *)src, dst, (const float2 *)p->tw_m, p->m, l1, l2, ss, sd, inverse);
        MST_FFT_STEP(fft_cols_kernel, ga, l1)
        MST_CHECK_LAUNCH("fft_cols_kernel");
        std::swap(src, dst);
        std::swap(ss, sd);
        MST_FFT_STEP(fft_rows_kernel, gb, l2)
        MST_CHECK_LAUNCH("fft_rows_kernel");
#undef MST_FFT_STEP
        std::swap(src, dst);
        std::swap(ss, sd);
        *res = src;
        *sres = ss;
        return MST_OK;
    }
    long Ns = 1;
    if (p->log2m % 2) {
        MST_LAUNCH(fft_stockham2_kernel, dim3((unsigned)((p->m / 2 + 255) / 256), (unsigned)nb), dim3(256), stream, (const float2 *)src, dst,
                   (const float2 *)p->tw_m, p->m, Ns, ss, sd, inverse);
        MST_CHECK_LAUNCH("fft_stockham2_kernel");
        std::swap(src, dst);
        std::swap(ss, sd);
        Ns = 2;
    }
    for (; Ns < p->m; Ns <<= 2) {
        MST_LAUNCH(fft_stockham4_kernel, dim3((unsigned)((p->m / 4 + 255) / 256), (unsigned)nb), dim3(256), stream, (const float2 *)src, dst,
                   (const float2 *)p->tw_m, p->m, Ns, ss, sd, inverse);
        MST_CHECK_LAUNCH("fft_stockham4_kernel");
        std::swap(src, dst);
        std::swap(ss, sd);
    }
    *res = src;
    *sres = ss;
    return MST_OK;
}
// hipfftExecR2C's contract: in [nb][n] reals (DESTROYED: it is one of the two work buffers), out [nb][n / 2 + 1] bins, unnormalised
int fft_exec_r2c(const MstFftPlan *p, float *in, float2 *out, int nb, void *stream) {
    if (nb < 1) return MST_OK;
    if (nb > 65535) return fail(MST_ERR_UNSUPPORTED, "FFT: more than 65535 sequences per call");
    float2 *z;
    long sz;
    int rc = fft_passes(p, (float2 *)in, p->m, out, p->m + 1, nb, 0, stream, &z, &sz);
    if (rc) return rc;
    MST_LAUNCH(fft_r2c_post_kernel, dim3((unsigned)((p->m / 2 + 1 + 255) / 256), (unsigned)nb), dim3(256), stream, (const float2 *)z, out,
               (const float2 *)p->tw_n, p->m, sz, p->m + 1);
    MST_CHECK_LAUNCH("fft_r2c_post_kernel");
    return MST_OK;
}
// hipfftExecC2R's contract: in [nb][n / 2 + 1] bins (DESTROYED), out [nb][n] reals = n * irfft(in)
int fft_exec_c2r(const MstFftPlan *p, float2 *in, float *out, int nb, void *stream) {
    if (nb < 1) return MST_OK;
    if (nb > 65535) return fail(MST_ERR_UNSUPPORTED, "FFT: more than 65535 sequences per call");
    float2 *o = (float2 *)out;
    // the passes alternate between the two buffers and must end in `out`: an even number starts there, an odd number starts in `in`
    float2 *start = (p->passes % 2 == 0) ? o : in;
    const long sstart = (p->passes % 2 == 0) ? p->m : p->m + 1;
    MST_LAUNCH(fft_c2r_pre_kernel, dim3((unsigned)((p->m / 2 + 1 + 255) / 256), (unsigned)nb), dim3(256), stream, (const float2 *)in, start,
               (const float2 *)p->tw_n, p->m, p->m + 1, sstart);
    MST_CHECK_LAUNCH("fft_c2r_pre_kernel");
    float2 *other = (start == o) ? in : o;
    const long sother = (start == o) ? p->m + 1 : p->m;
    float2 *z;
    long sz;
    int rc = fft_passes(p, start, sstart, other, sother, nb, 1, stream, &z, &sz);
    if (rc) return rc;
    if (z != o) return fail(MST_ERR_STATE, "FFT: inverse passes ended in the wrong buffer");
    return MST_OK;
}
}  // namespace

// ---- FFT convolution (ConvolutionalReverb) ---------------------------------------------------------------------------
struct MstConvolver {
    long L = 0, Lh_max = 0, n_fft = 0;
    long step = 0, shift = 0;       // overlap-save: block b holds the samples b * step - shift + i; one block: step = n_fft, shift = 0
    int nb = 1;                     // blocks per (item, channel)
    int n_items = 0, C = 0;
    MstFftPlan *plan = nullptr;     // one plan serves the signal blocks, the impulse response and the inverse
};

extern "C" int mst_fx_convolver_create(long L, long Lh_max, int n_items, int C, MstConvolver **out) {
    if (!out || L < 1 || Lh_max < 1 || n_items < 1 || C < 1) return fail(MST_ERR_ARG, "mst_fx_convolver_create: bad argument");
    long n = 4;
    while (n < L + Lh_max - 1) n <<= 1;
    long step = n, shift = 0;
    int nb = 1;
    if (n > (1L << 18)) {
        // a long signal: overlap-save blocks of max(2^16, 4 x the response rounded up to a power of two) samples - one plan for every
        // signal length, float32 rounding of a 2^16..2^19-point transform
        long nh = 1;
        while (nh < Lh_max) nh <<= 1;
        long nblk = 4 * nh > (1L << 16) ? 4 * nh : (1L << 16);
        if (nblk > MST_FFT_MAX_N) nblk = 2 * nh;          // a response longer than 2^19 samples (11.9 s at 44.1 kHz): blocks of twice its length
        if (nblk < n) {
            n = nblk;
            shift = Lh_max - 1;
            step = n - shift;
            nb = (int)((L + Lh_max - 1 + step - 1) / step);
        }
    }
    if (n > MST_FFT_MAX_N)
        return fail(MST_ERR_UNSUPPORTED, "mst_fx_convolver_create: impulse responses longer than 2^20 samples (23.8 s at 44.1 kHz) need a transform beyond 2^21 points");
    if ((long)n_items * C * nb > 65535) return fail(MST_ERR_UNSUPPORTED, "mst_fx_convolver_create: more than 65535 transform blocks (split the batch)");
    auto *cv = new MstConvolver;
    cv->L = L; cv->Lh_max = Lh_max; cv->n_fft = n; cv->n_items = n_items; cv->C = C;
    cv->step = step; cv->shift = shift; cv->nb = nb;
    const int rc = fft_plan_create(&cv->plan, n);
    if (rc) {
        mst_fx_convolver_destroy(cv);
        return rc;
    }
    *out = cv;
    return MST_OK;
}

extern "C" void mst_fx_convolver_destroy(MstConvolver *cv) {
    if (!cv) return;
    fft_plan_destroy(cv->plan);
    delete cv;
}

extern "C" size_t mst_fx_convolver_workspace_bytes(const MstConvolver *cv) {
    if (!cv) return 0;
    const size_t nbin = (size_t)cv->n_fft / 2 + 1, seqs = (size_t)cv->n_items * cv->C * cv->nb + cv->C;
    return seqs * (size_t)cv->n_fft * sizeof(float) + seqs * nbin * sizeof(float2) + 256;
}

extern "C" int mst_fx_convolve(MstConvolver *cv, const float *x, const float *h, long Lh, float *y, long offset, double dry,
                               double wet, void *ws, size_t ws_bytes, void *stream) {
    if (!cv || !x || !h || !y || !ws) return fail(MST_ERR_ARG, "mst_fx_convolve: bad argument");
    if (Lh < 1 || Lh > cv->Lh_max) return fail(MST_ERR_ARG, "mst_fx_convolve: impulse response longer than the convolver was created for");
    if (offset < 0 || offset > Lh - 1) return fail(MST_ERR_ARG, "mst_fx_convolve: offset outside [0, Lh-1]");
    if (ws_bytes < mst_fx_convolver_workspace_bytes(cv)) return fail(MST_ERR_WORKSPACE, "mst_fx_convolve: workspace too small");
    const long n = cv->n_fft, nbin = n / 2 + 1;
    const int nseq = cv->n_items * cv->C, C = cv->C, nb = cv->nb, nblk = nseq * nb;
    int rc;
    float *rx = (float *)ws, *rh = rx + (size_t)nblk * n;
    float2 *cx = (float2 *)(((uintptr_t)(rh + (size_t)C * n) + 255) & ~(uintptr_t)255), *ch = cx + (size_t)nblk * nbin;
    const unsigned gb = (unsigned)((n + 255) / 256);
    MST_LAUNCH(fx_conv_pack_kernel, dim3(gb, nblk), dim3(256), stream, x, rx, cv->L, C, n, nb, cv->step, cv->shift);
    MST_CHECK_LAUNCH("fx_conv_pack_kernel");
    MST_LAUNCH(fx_conv_pack_kernel, dim3(gb, C), dim3(256), stream, h, rh, Lh, C, n, 1, n, 0L);       // the IR is one [Lh][C] "item"
    MST_CHECK_LAUNCH("fx_conv_pack_kernel");
    if ((rc = fft_exec_r2c(cv->plan, rx, cx, nblk, stream)) || (rc = fft_exec_r2c(cv->plan, rh, ch, C, stream))) return rc;
    MST_LAUNCH(fx_conv_mul_kernel, dim3((unsigned)((nbin + 255) / 256), nblk), dim3(256), stream, cx, (const float2 *)ch, nbin, C, nb,
               1.0f / (float)n);
    MST_CHECK_LAUNCH("fx_conv_mul_kernel");
    if ((rc = fft_exec_c2r(cv->plan, cx, rx, nblk, stream))) return rc;
    const long per = cv->L * C;
    MST_LAUNCH(fx_conv_mix_kernel, dim3((unsigned)((per + 255) / 256), cv->n_items), dim3(256), stream, x, (const float *)rx, y, cv->L,
               C, n, nb, cv->step, cv->shift, offset, (float)dry, (float)wet);
    MST_CHECK_LAUNCH("fx_conv_mix_kernel");
    return MST_OK;
}

// ---- a response per item: the responses of a batch back to back in one bank, each packed and transformed once ------------------------
extern "C" size_t mst_fx_convolver_items_workspace_bytes(const MstConvolver *cv, int n_resp) {
    if (!cv || n_resp < 1) return 0;
    const size_t nbin = (size_t)cv->n_fft / 2 + 1, seqs = (size_t)cv->n_items * cv->C * cv->nb + (size_t)n_resp * cv->C;
    return seqs * (size_t)cv->n_fft * sizeof(float) + seqs * nbin * sizeof(float2) + 256;
}

extern "C" size_t mst_fx_convolve_items_table_bytes(int n_items, int n_resp) {
    if (n_items < 1 || n_resp < 1) return 0;
    return ((size_t)n_resp * 2 + (size_t)n_items * MST_CONV_ITEM_FIELDS) * sizeof(double);
}

extern "C" int mst_fx_convolve_items_prepare(const MstConvolver *cv, const long *resp_start_host, const long *resp_len_host, int n_resp,
                                             long bank_frames, const double *params_host, int n_items, double *table_host,
                                             size_t table_bytes, int *first_bad_item) {
    if (first_bad_item) *first_bad_item = -1;
    if (!cv || !resp_start_host || !resp_len_host || !params_host || !table_host || n_resp < 1 || n_items < 1 || bank_frames < 1)
        return fail(MST_ERR_ARG, "mst_fx_convolve_items_prepare: bad argument");
    if (table_bytes < mst_fx_convolve_items_table_bytes(n_items, n_resp)) return fail(MST_ERR_WORKSPACE, "mst_fx_convolve_items_prepare: table too small");
    char buf[200];
    if (n_items > cv->n_items) {
        if (first_bad_item) *first_bad_item = cv->n_items;
        std::snprintf(buf, sizeof(buf), "mst_fx_convolve_items_prepare: item %d: the convolver was created for %d items", cv->n_items, cv->n_items);
        return fail(MST_ERR_ARG, buf);
    }
    if (((long)n_items * cv->nb + n_resp) * cv->C > 65535)
        return fail(MST_ERR_UNSUPPORTED, "mst_fx_convolve_items_prepare: more than 65535 transform blocks (split the batch)");
    for (int r = 0; r < n_resp; ++r) {
        const long start = resp_start_host[r], len = resp_len_host[r];
        if (len < 1 || len > cv->Lh_max) {
            std::snprintf(buf, sizeof(buf), "mst_fx_convolve_items_prepare: response %d: %ld frames, the convolver takes 1 ... %ld", r, len, cv->Lh_max);
            return fail(MST_ERR_ARG, buf);
        }
        if (start < 0 || start > bank_frames - len) {
            std::snprintf(buf, sizeof(buf), "mst_fx_convolve_items_prepare: response %d: frames %ld ... %ld lie outside the bank of %ld", r, start, start + len, bank_frames);
            return fail(MST_ERR_ARG, buf);
        }
        table_host[2 * r] = (double)start;
        table_host[2 * r + 1] = (double)len;
    }
    double *items = table_host + 2 * (size_t)n_resp;
    for (int i = 0; i < n_items; ++i) {
        const double *p = params_host + 4 * (size_t)i;
        double *t = items + (size_t)i * MST_CONV_ITEM_FIELDS;
        if (!(p[0] >= 0 && p[0] < n_resp) || p[0] != std::floor(p[0])) {
            if (first_bad_item) *first_bad_item = i;
            std::snprintf(buf, sizeof(buf), "mst_fx_convolve_items_prepare: item %d: response index %g outside [0, %d)", i, p[0], n_resp);
            return fail(MST_ERR_ARG, buf);
        }
        const long len = resp_len_host[(int)p[0]];
        if (!(p[1] >= 0 && p[1] <= (double)(len - 1)) || p[1] != std::floor(p[1])) {
            if (first_bad_item) *first_bad_item = i;
            std::snprintf(buf, sizeof(buf), "mst_fx_convolve_items_prepare: item %d: offset %g outside [0, Lh-1] of its response of %ld frames", i, p[1], len);
            return fail(MST_ERR_ARG, buf);
        }
        t[0] = p[0];
        t[1] = p[1];
        t[2] = p[2];
        t[3] = p[3];
        t[4] = p[3] == 0.0 ? 1.0 : 0.0;          // ConvolutionalReverb.process returns x when wet == 0
    }
    return MST_OK;
}

extern "C" int mst_fx_convolve_items(MstConvolver *cv, const float *x, const float *bank, const double *table_dev, int n_items, int n_resp,
                                     float *y, void *ws, size_t ws_bytes, void *stream) {
    if (!cv || !x || !bank || !table_dev || !y || !ws || n_items < 1 || n_resp < 1) return fail(MST_ERR_ARG, "mst_fx_convolve_items: bad argument");
    if (n_items > cv->n_items) return fail(MST_ERR_ARG, "mst_fx_convolve_items: more items than the convolver was created for");
    if (((long)n_items * cv->nb + n_resp) * cv->C > 65535) return fail(MST_ERR_UNSUPPORTED, "mst_fx_convolve_items: more than 65535 transform blocks (split the batch)");
    if (ws_bytes < mst_fx_convolver_items_workspace_bytes(cv, n_resp)) return fail(MST_ERR_WORKSPACE, "mst_fx_convolve_items: workspace too small");
    const long n = cv->n_fft, nbin = n / 2 + 1;
    const int C = cv->C, nb = cv->nb, nblk = n_items * C * nb, nh = n_resp * C;
    int rc;
    // the layout of mst_fx_convolve with the convolver's full item capacity in front of the responses
    float *rx = (float *)ws, *rh = rx + (size_t)cv->n_items * C * nb * n;
    float2 *cx = (float2 *)(((uintptr_t)(rh + (size_t)nh * n) + 255) & ~(uintptr_t)255), *ch = cx + (size_t)cv->n_items * C * nb * nbin;
    const double *items = table_dev + 2 * (size_t)n_resp;
    const unsigned gb = (unsigned)((n + 255) / 256);
    MST_LAUNCH(fx_conv_pack_kernel, dim3(gb, nblk), dim3(256), stream, x, rx, cv->L, C, n, nb, cv->step, cv->shift);
    MST_CHECK_LAUNCH("fx_conv_pack_kernel");
    MST_LAUNCH(fxsi_conv_pack_bank_kernel, dim3(gb, nh), dim3(256), stream, bank, rh, table_dev, C, n);
    MST_CHECK_LAUNCH("fxsi_conv_pack_bank_kernel");
    if ((rc = fft_exec_r2c(cv->plan, rx, cx, nblk, stream)) || (rc = fft_exec_r2c(cv->plan, rh, ch, nh, stream))) return rc;
    MST_LAUNCH(fxsi_conv_mul_kernel, dim3((unsigned)((nbin + 255) / 256), nblk), dim3(256), stream, cx, (const float2 *)ch, items, nbin, C, nb,
               1.0f / (float)n);
    MST_CHECK_LAUNCH("fxsi_conv_mul_kernel");
    if ((rc = fft_exec_c2r(cv->plan, cx, rx, nblk, stream))) return rc;
    const long per = cv->L * C;
    MST_LAUNCH(fxsi_conv_mix_kernel, dim3((unsigned)((per + 255) / 256), n_items), dim3(256), stream, x, (const float *)rx, y, items, cv->L, C, n,
               nb, cv->step, cv->shift);
    MST_CHECK_LAUNCH("fxsi_conv_mix_kernel");
    return MST_OK;
}

extern "C" int mst_fx_rms_normalize(const float *x, float *y, int n_items, long per_x, long per_y, double *scratch, void *stream) {
    if (!x || !y || !scratch || n_items < 1 || per_x < 1 || per_y < 1) return fail(MST_ERR_ARG, "mst_fx_rms_normalize: bad argument");
    int rc;
    if ((rc = energy(x, scratch, n_items, per_x, 0, stream))) return rc;
    if ((rc = energy(y, scratch + 2 * n_items, n_items, per_y, 0, stream))) return rc;
    MST_LAUNCH(fx_scale_kernel, dim3((unsigned)((per_y + 255) / 256), n_items), dim3(256), stream, x, y, per_y, 1.0f,
               (const double *)scratch, (const double *)(scratch + 2 * n_items), 1, per_x, (const double *)nullptr);
    MST_CHECK_LAUNCH("fx_scale_kernel");
    return MST_OK;
}

// ---- chain fusion helpers -------------------------------------------------------------------------------------------------
extern "C" int mst_fx_sumsq(const float *x, int n_items, long per_item, double *out, void *stream) {
    if (!x || !out || n_items < 1 || per_item < 1) return fail(MST_ERR_ARG, "mst_fx_sumsq: bad argument");
    int chunks = (int)std::min<long>(MST_SUMSQ_SLOTS, (per_item + 8191) / 8192);
    if (chunks < 1) chunks = 1;
    MST_LAUNCH(fx_sumsq_kernel, dim3(n_items * chunks), dim3(256), stream, x, out, per_item, chunks);
    MST_CHECK_LAUNCH("fx_sumsq_kernel");
    return MST_OK;
}

extern "C" int mst_fx_rms_pending(const double *scale_x, const double *sumsq_x, long per_x, const double *sumsq_y, long per_y,
                                  double *scale_out, int n_items, void *stream) {
    if (!sumsq_x || !sumsq_y || !scale_out || n_items < 1 || per_x < 1 || per_y < 1) return fail(MST_ERR_ARG, "mst_fx_rms_pending: bad argument");
    MST_LAUNCH(fx_rms_pending_kernel, dim3(n_items), dim3(64), stream, scale_x, sumsq_x, per_x, sumsq_y, per_y, scale_out, n_items);
    MST_CHECK_LAUNCH("fx_rms_pending_kernel");
    return MST_OK;
}

extern "C" int mst_fx_scale_items(const float *x, float *y, int n_items, long per_item, const double *scale, void *stream) {
    if (!x || !y || !scale || n_items < 1 || per_item < 1) return fail(MST_ERR_ARG, "mst_fx_scale_items: bad argument");
    MST_LAUNCH(fx_scale_kernel, dim3((unsigned)((per_item + 255) / 256), n_items), dim3(256), stream, x, y, per_item, 1.0f,
               (const double *)nullptr, (const double *)nullptr, 0, per_item, scale);
    MST_CHECK_LAUNCH("fx_scale_kernel");
    return MST_OK;
}

// ---- STFT mean magnitude (EQ matching front end) ---------------------------------------------------------------------
struct MstStft {
    long n_fft = 0, hop = 0;
    int batch = 0;
    MstFftPlan *plan = nullptr;     // R2C of up to `batch` frames of n_fft
    float *win = nullptr;           // [n_fft] analysis window (device)
};

extern "C" int mst_fx_stft_create(long n_fft, long hop, const float *window_host, int max_batch, MstStft **out) {
    if (!out || !window_host || n_fft < 2 || hop < 1 || max_batch < 1) return fail(MST_ERR_ARG, "mst_fx_stft_create: bad argument");
    auto *st = new MstStft;
    st->n_fft = n_fft; st->hop = hop; st->batch = max_batch;
    const int rcp = fft_plan_create(&st->plan, n_fft);          // frame lengths are powers of two (the reference's FFT_SIZE is 65536)
    if (rcp) {
        delete st;
        return rcp;
    }
    if (hipMalloc((void **)&st->win, (size_t)n_fft * sizeof(float)) != hipSuccess ||
        hipMemcpy(st->win, window_host, (size_t)n_fft * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        fft_plan_destroy(st->plan);
        delete st;
        return fail(MST_ERR_HIP, "mst_fx_stft_create: hipMalloc failed");
    }
    *out = st;
    return MST_OK;
}

extern "C" void mst_fx_stft_destroy(MstStft *st) {
    if (!st) return;
    fft_plan_destroy(st->plan);
    (void)hipFree(st->win);
    delete st;
}

extern "C" size_t mst_fx_stft_workspace_bytes(const MstStft *st) {
    if (!st) return 0;
    return (size_t)st->batch * st->n_fft * sizeof(float) + (size_t)st->batch * (st->n_fft / 2 + 1) * sizeof(float2) + 512;
}

extern "C" int mst_fx_stft_mean_magnitude(MstStft *st, const float *x, long L, int C, int channel, float *mean_dev, void *ws,
                                          size_t ws_bytes, void *stream) {
    if (!st || !x || !mean_dev || !ws || C < 1 || channel < 0 || channel >= C) return fail(MST_ERR_ARG, "mst_fx_stft_mean_magnitude: bad argument");
    if (L < st->n_fft) return fail(MST_ERR_ARG, "mst_fx_stft_mean_magnitude: signal shorter than one frame");
    if (ws_bytes < mst_fx_stft_workspace_bytes(st)) return fail(MST_ERR_WORKSPACE, "mst_fx_stft_mean_magnitude: workspace too small");
    const long n = st->n_fft, nbin = n / 2 + 1;
    const long n_frames = 1 + (L - n) / st->hop;          // common_miscellaneous.py:64
    float *frames = (float *)ws;
    float2 *spec = (float2 *)(((uintptr_t)(frames + (size_t)st->batch * n) + 255) & ~(uintptr_t)255);
    MST_HIP_TRY(hipMemsetAsync(mean_dev, 0, (size_t)nbin * sizeof(float), (hipStream_t)stream));
    for (long f0 = 0; f0 < n_frames; f0 += st->batch) {
        const int nb = (int)std::min<long>(st->batch, n_frames - f0);
        MST_LAUNCH(fx_stft_frame_kernel, dim3((unsigned)((n + 255) / 256), nb), dim3(256), stream, x, frames, (const float *)st->win, L,
                   C, channel, n, st->hop, f0, n_frames);
        MST_CHECK_LAUNCH("fx_stft_frame_kernel");
        const int rcf = fft_exec_r2c(st->plan, frames, spec, nb, stream);          // only the frames that exist
        if (rcf) return rcf;
        MST_LAUNCH(fx_stft_mag_accum_kernel, dim3((unsigned)((nbin + 255) / 256)), dim3(256), stream, (const float2 *)spec, mean_dev, nbin, nb);
        MST_CHECK_LAUNCH("fx_stft_mag_accum_kernel");
    }
    MST_LAUNCH(fx_scale_inplace_kernel, dim3((unsigned)((nbin + 255) / 256)), dim3(256), stream, mean_dev, nbin, 1.0f / (float)n_frames);
    MST_CHECK_LAUNCH("fx_scale_inplace_kernel");
    return MST_OK;
}


extern "C" int mst_fx_stereo_moments(const float *x, int n_items, long L, double *out, void *stream) {
    if (!x || !out || n_items < 1 || L < 1) return fail(MST_ERR_ARG, "mst_fx_stereo_moments: bad argument");
    MST_HIP_TRY(hipMemsetAsync(out, 0, (size_t)n_items * 3 * sizeof(double), (hipStream_t)stream));
    const unsigned chunks = (unsigned)std::min<long>(256, (L + 4095) / 4096);
    MST_LAUNCH(fx_stereo_moments_kernel, dim3(chunks, n_items), dim3(256), stream, x, L, out);
    MST_CHECK_LAUNCH("fx_stereo_moments_kernel");
    return MST_OK;
}

extern "C" int mst_fx_stereo_mix(const float *x, float *y, int n_items, long L, float m00, float m01, float m10, float m11, void *stream) {
    if (!x || !y || n_items < 1 || L < 1) return fail(MST_ERR_ARG, "mst_fx_stereo_mix: bad argument");
    const long n = (long)n_items * L;
    MST_LAUNCH(fx_stereo_mix_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), stream, x, y, n, m00, m01, m10, m11);
    MST_CHECK_LAUNCH("fx_stereo_mix_kernel");
    return MST_OK;
}

// ---- AlgorithmicReverb -------------------------------------------------------------------------------------------------
extern "C" size_t mst_fx_algorithmic_reverb_scratch_bytes(int n_items, long L, int n_combs) {
    if (n_items < 1 || L < 1 || n_combs < 1) return 0;
    return ((size_t)n_combs + 1) * n_items * 2 * (size_t)L * sizeof(double);
}

namespace {
// params_dev == NULL: the shared call with its five scalars; else DEVICE [n_items][5] = damping, room_size, wet1, wet2, dry read per item
int reverb_run(const char *who, const float *x, float *y, int n_items, long L, int C, const int *comb_delays, int n_combs,
               const int *allpass_delays, int n_allpass, int stereo_spread, double damping, double room_size, double in_gain, double wet1,
               double wet2, double dry, const double *params_dev, double *scratch, size_t scratch_bytes, void *stream) {
    const std::string name(who);
    if (!x || !y || !comb_delays || !allpass_delays || !scratch || n_items < 1 || L < 1 || (C != 1 && C != 2) || n_combs < 1 ||
        n_combs > 8 || n_allpass < 1 || stereo_spread < 0)
        return fail(MST_ERR_ARG, (name + ": bad argument").c_str());
    if (scratch_bytes < mst_fx_algorithmic_reverb_scratch_bytes(n_items, L, n_combs))
        return fail(MST_ERR_WORKSPACE, (name + ": scratch too small").c_str());
    CombArgs a;
    a.x = x;
    a.y = scratch + (size_t)n_items * 2 * L;            // [n_combs][n_items * 2][L] behind the wet buffer
    a.L = L;
    a.C = C;
    a.n_items = n_items;
    a.n_combs = n_combs;
    for (int k = 0; k < n_combs; ++k) {
        if (comb_delays[k] < 1 || comb_delays[k] + stereo_spread > 2048)
            return fail(MST_ERR_UNSUPPORTED, (name + ": comb delays up to 2048 samples").c_str());
        a.delay[k][0] = comb_delays[k];
        a.delay[k][1] = comb_delays[k] + stereo_spread;
    }
    a.damp = damping;
    a.feedback = room_size;
    a.in_gain = in_gain;
    if (params_dev) MST_LAUNCH(fxsi_comb_kernel, dim3(n_combs, n_items * 2), dim3(64), stream, a, params_dev);
    else MST_LAUNCH(fx_comb_kernel, dim3(n_combs, n_items * 2), dim3(64), stream, a);
    MST_CHECK_LAUNCH("fx_comb_kernel");
    double *wet = scratch;                                // [n_items * 2][L]
    for (int k = 0; k < n_allpass; ++k) {
        const int dl = allpass_delays[2 * k], dr = allpass_delays[2 * k + 1];
        if (dl < 1 || dr < 1) return fail(MST_ERR_ARG, (name + ": all-pass delay < 1").c_str());
        const int threads = std::min(1024, std::max(64, ((std::max(dl, dr) + 63) / 64) * 64));
        if (params_dev)
            MST_LAUNCH(fxsi_allpass_kernel, dim3(n_items * 2), dim3(threads), stream, wet, (const double *)a.y, k == 0 ? n_combs : 0, 0, L,
                       n_items * 2, dl, dr, params_dev);
        else
            MST_LAUNCH(fx_allpass_kernel, dim3(n_items * 2), dim3(threads), stream, wet, (const double *)a.y, k == 0 ? n_combs : 0, 0, L,
                       n_items * 2, dl, dr, room_size);
        MST_CHECK_LAUNCH("fx_allpass_kernel");
    }
    if (params_dev)
        MST_LAUNCH(fxsi_reverb_mix_kernel, dim3((unsigned)((L + 255) / 256), n_items), dim3(256), stream, x, (const double *)wet, y, L, C, params_dev);
    else
        MST_LAUNCH(fx_reverb_mix_kernel, dim3((unsigned)((L + 255) / 256), n_items), dim3(256), stream, x, (const double *)wet, y, L, C, wet1,
                   wet2, dry);
    MST_CHECK_LAUNCH("fx_reverb_mix_kernel");
    return MST_OK;
}
}  // namespace

extern "C" int mst_fx_algorithmic_reverb(const float *x, float *y, int n_items, long L, int C, const int *comb_delays, int n_combs,
                                         const int *allpass_delays, int n_allpass, int stereo_spread, double damping, double room_size,
                                         double in_gain, double wet1, double wet2, double dry, double *scratch, size_t scratch_bytes,
                                         void *stream) {
    return reverb_run("mst_fx_algorithmic_reverb", x, y, n_items, L, C, comb_delays, n_combs, allpass_delays, n_allpass, stereo_spread, damping,
                      room_size, in_gain, wet1, wet2, dry, nullptr, scratch, scratch_bytes, stream);
}

extern "C" int mst_fx_algorithmic_reverb_items(const float *x, float *y, int n_items, long L, int C, const int *comb_delays, int n_combs,
                                               const int *allpass_delays, int n_allpass, int stereo_spread, double in_gain,
                                               const double *params_dev, double *scratch, size_t scratch_bytes, void *stream) {
    if (!params_dev || n_items > 32767) return fail(MST_ERR_ARG, "mst_fx_algorithmic_reverb_items: bad argument");
    return reverb_run("mst_fx_algorithmic_reverb_items", x, y, n_items, L, C, comb_delays, n_combs, allpass_delays, n_allpass, stereo_spread, 0.0,
                      0.0, in_gain, 0.0, 0.0, 0.0, params_dev, scratch, scratch_bytes, stream);
}

// ---- multi-scale spectral distance (csrc/mss_kernels.h) ------------------------------------------------------------------
struct MstMss {
    MstMssDesc d;
    int logm[MST_MSS_MAX_SCALES];                 // log2(n_fft / 2)
    float *win[MST_MSS_MAX_SCALES];               // [n_fft]
    float2 *tw[MST_MSS_MAX_SCALES];               // [n_fft / 4]      exp(-2 pi i j / (n_fft / 2))
    float2 *twn[MST_MSS_MAX_SCALES];              // [n_fft / 4 + 1]  exp(-2 pi i k / n_fft)
};

namespace {
int mss_frames(const MstMss *h, int s, long L) {          // FrontEnd: T = 1 + L // hop, minus one when L % round(n_fft / 4) == 0
    long T = 1 + L / h->d.hop[s];
    if (L % (h->d.n_fft[s] / 4) == 0) T -= 1;
    return (int)T;
}
int mss_groups(const MstMss *h, int s, long L) {
    const int G = MSS_PTS / h->d.n_fft[s];
    return (mss_frames(h, s, L) + G - 1) / G;
}
// the scales first .. last of the handle must fit L and B the grid's z extent
int mss_check_length(const MstMss *h, int first, int last, int B, long L, const char *who) {
    if (B > 65535) return fail(MST_ERR_UNSUPPORTED, std::string(who) + ": B = " + std::to_string(B) + " (at most 65535 items per call)");
    for (int s = first; s <= last; ++s) {
        if (L <= h->d.n_fft[s] / 2 || L >= (1L << 30))
            return fail(MST_ERR_UNSUPPORTED, std::string(who) + ": L = " + std::to_string(L) + " must exceed n_fft / 2 = " +
                                                 std::to_string(h->d.n_fft[s] / 2) + " (reflection padding) and stay below 2^30");
        if (mss_frames(h, s, L) < 1)
            return fail(MST_ERR_UNSUPPORTED, std::string(who) + ": L = " + std::to_string(L) + " leaves no frame at n_fft = " +
                                                 std::to_string(h->d.n_fft[s]) + ", hop = " + std::to_string(h->d.hop[s]));
    }
    return MST_OK;
}
template <int EPI>
int mss_launch(const MstMss *h, int s, const float *est, const float *tgt, long item_stride, int B, int nchan, long L, int mix_mode,
               double *terms, float *mag, int n_out, void *stream) {
    const dim3 grid((unsigned)mss_groups(h, s, L), (unsigned)nchan, (unsigned)B);
    const int T = mss_frames(h, s, L);
    const float eps = (float)h->d.eps;
#define MSS_CASE(LM)                                                                                                                  \
    case LM:                                                                                                                          \
        MST_LAUNCH((mss_frames_kernel<LM, EPI>), grid, dim3(256), stream, est, tgt, item_stride, (int)L, mix_mode,                   \
                   (const float *)h->win[s], (const float2 *)h->tw[s], (const float2 *)h->twn[s], h->d.hop[s], T, eps, terms, mag, n_out); \
        break;
    switch (h->logm[s]) {
        MSS_CASE(7) MSS_CASE(8) MSS_CASE(9) MSS_CASE(10) MSS_CASE(11)
    }
#undef MSS_CASE
    MST_CHECK_LAUNCH("mss_frames_kernel");
    return MST_OK;
}
}  // namespace

extern "C" int mst_mss_destroy(MstMss *h) {
    if (!h) return MST_OK;
    for (int s = 0; s < MST_MSS_MAX_SCALES; ++s) {
        (void)hipFree(h->win[s]);
        (void)hipFree(h->tw[s]);
        (void)hipFree(h->twn[s]);
    }
    delete h;
    return MST_OK;
}

extern "C" int mst_mss_create(const MstMssDesc *desc, MstMss **out) {
    if (!desc || !out) return fail(MST_ERR_ARG, "mst_mss_create: null argument");
    if (desc->struct_size != sizeof(MstMssDesc)) return fail(MST_ERR_ARG, "mst_mss_create: MstMssDesc.struct_size does not match this library's layout");
    if (desc->mode != MST_MSS_MIDSIDE && desc->mode != MST_MSS_ORI)
        return fail(MST_ERR_UNSUPPORTED, "mst_mss_create: mode = " + std::to_string(desc->mode) + " (0 = midside, 1 = ori)");
    if (desc->n_scales < 1 || desc->n_scales > MST_MSS_MAX_SCALES)
        return fail(MST_ERR_UNSUPPORTED, "mst_mss_create: n_scales = " + std::to_string(desc->n_scales) + " (1 .. 8)");
    if (desc->window != MST_MSS_HANN && desc->window != MST_MSS_HAMMING)
        return fail(MST_ERR_UNSUPPORTED, "mst_mss_create: window = " + std::to_string(desc->window) + " (0 = hann, 1 = hamming)");
    if (!(desc->eps >= 0.0) || !(desc->eps < 1.0)) return fail(MST_ERR_UNSUPPORTED, "mst_mss_create: eps = " + std::to_string(desc->eps) + " (0 <= eps < 1)");
    for (int s = 0; s < desc->n_scales; ++s) {
        const int n = desc->n_fft[s];
        if (n < 256 || n > 4096 || (n & (n - 1)))
            return fail(MST_ERR_UNSUPPORTED, "mst_mss_create: n_fft = " + std::to_string(n) + " (a power of two, 256 .. 4096)");
        if (desc->hop[s] < 1 || desc->hop[s] > n)
            return fail(MST_ERR_UNSUPPORTED, "mst_mss_create: hop = " + std::to_string(desc->hop[s]) + " (1 .. n_fft = " + std::to_string(n) + ")");
        if (desc->win_length[s] < 1 || desc->win_length[s] > n)
            return fail(MST_ERR_UNSUPPORTED, "mst_mss_create: win_length = " + std::to_string(desc->win_length[s]) + " (1 .. n_fft = " + std::to_string(n) + ")");
    }
    auto *h = new MstMss();
    h->d = *desc;
    const double pi = 3.14159265358979323846;
    for (int s = 0; s < desc->n_scales; ++s) {
        const int n = desc->n_fft[s], m = n / 2, wl = desc->win_length[s], left = (n - wl) / 2;
        int lg = 0;
        while ((1 << lg) < m) ++lg;
        h->logm[s] = lg;
        std::vector<float> win((size_t)n, 0.0f);          // periodic window, centred in the frame like torch.stft pads it
        for (int i = 0; i < wl; ++i) {
            const double cs = cos(2.0 * pi * (double)i / (double)wl);
            win[(size_t)left + i] = (float)(desc->window == MST_MSS_HANN ? 0.5 - 0.5 * cs : 0.54 - 0.46 * cs);
        }
        std::vector<float2> tw((size_t)m / 2), twn((size_t)m / 2 + 1);
        for (int j = 0; j < m / 2; ++j) tw[j] = make_float2((float)cos(-2.0 * pi * j / m), (float)sin(-2.0 * pi * j / m));
        for (int k = 0; k <= m / 2; ++k) twn[k] = make_float2((float)cos(-2.0 * pi * k / n), (float)sin(-2.0 * pi * k / n));
        int rc;
        if ((rc = upload(&h->win[s], win)) || (rc = upload(&h->tw[s], tw)) || (rc = upload(&h->twn[s], twn))) {
            mst_mss_destroy(h);
            return rc;
        }
    }
    *out = h;
    return MST_OK;
}

extern "C" int mst_mss_frames(const MstMss *h, int scale, long L) {
    if (!h || scale < 0 || scale >= h->d.n_scales || L < 1) return fail(MST_ERR_ARG, "mst_mss_frames: bad argument");
    return mss_frames(h, scale, L);
}

extern "C" size_t mst_mss_workspace_bytes(const MstMss *h, int B, long L) {
    if (!h || B < 1 || L < 1) return 0;
    size_t total = 256;
    for (int s = 0; s < h->d.n_scales; ++s) total += align_up((size_t)B * 2 * std::max(1, mss_groups(h, s, L)) * 2 * sizeof(double), 256);
    return total;
}

extern "C" int mst_mss_forward(MstMss *h, const float *est, const float *tgt, int B, long L, double *terms, void *ws, size_t ws_bytes,
                               void *stream) {
    if (!h || !est || !tgt || !terms || B < 1 || L < 1) return fail(MST_ERR_ARG, "mst_mss_forward: bad argument");
    int rc;
    if ((rc = mss_check_length(h, 0, h->d.n_scales - 1, B, L, "mst_mss_forward"))) return rc;
    if (!ws || ws_bytes < mst_mss_workspace_bytes(h, B, L)) return fail(MST_ERR_WORKSPACE, "mst_mss_forward: workspace null or too small");
    unsigned char *p = (unsigned char *)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    for (int s = 0; s < h->d.n_scales; ++s) {
        double *partial = (double *)p;
        const int groups = mss_groups(h, s, L);
        if ((rc = mss_launch<MSS_EPI_TERMS>(h, s, est, tgt, 2 * L, B, 2, L, h->d.mode == MST_MSS_MIDSIDE ? 1 : 0, partial, nullptr, 0, stream)))
            return rc;
        MST_LAUNCH(mss_finalize_kernel, dim3((unsigned)((B * 4 + 63) / 64)), dim3(64), stream, (const double *)partial, terms, B, groups,
                   h->d.n_scales, s);
        MST_CHECK_LAUNCH("mss_finalize_kernel");
        p += align_up((size_t)B * 2 * groups * 2 * sizeof(double), 256);
    }
    return MST_OK;
}

// one frames workspace [B, 2, T, n_fft] fp32, reused scale after scale: the largest of them
extern "C" size_t mst_mss_backward_workspace_bytes(const MstMss *h, int B, long L) {
    if (!h || B < 1 || L < 1) return 0;
    size_t most = 0;
    for (int s = 0; s < h->d.n_scales; ++s)
        most = std::max(most, (size_t)B * 2 * (size_t)std::max(1, mss_frames(h, s, L)) * (size_t)h->d.n_fft[s] * sizeof(float));
    return 256 + align_up(most, 256);
}

extern "C" int mst_mss_backward(MstMss *h, const float *est, const float *tgt, int B, long L, const double *dterms, float *grad, void *ws,
                                size_t ws_bytes, void *stream) {
    if (!h || !est || !tgt || !dterms || !grad || B < 1 || L < 1) return fail(MST_ERR_ARG, "mst_mss_backward: bad argument");
    int rc;
    for (int s = 0; s < h->d.n_scales; ++s)
        if (h->d.hop[s] * 16 < h->d.n_fft[s])
            return fail(MST_ERR_UNSUPPORTED, "mst_mss_backward: hop = " + std::to_string(h->d.hop[s]) + " is below n_fft / 16 at n_fft = " +
                                                 std::to_string(h->d.n_fft[s]) + " (the frames workspace would exceed 16 waveforms per channel)");
    if ((rc = mss_check_length(h, 0, h->d.n_scales - 1, B, L, "mst_mss_backward"))) return rc;
    if (!ws || ws_bytes < mst_mss_backward_workspace_bytes(h, B, L)) return fail(MST_ERR_WORKSPACE, "mst_mss_backward: workspace null or too small");
    float *frames = (float *)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    const int mix_mode = h->d.mode == MST_MSS_MIDSIDE ? 1 : 0;
    for (int s = 0; s < h->d.n_scales; ++s) {
        const int T = mss_frames(h, s, L);
        const dim3 grid((unsigned)mss_groups(h, s, L), 2u, (unsigned)B);
#define MSS_CASE(LM)                                                                                                                  \
    case LM:                                                                                                                          \
        MST_LAUNCH((mss_grad_frames_kernel<LM>), grid, dim3(256), stream, est, tgt, 2 * L, (int)L, mix_mode, (const float *)h->win[s],    \
                   (const float2 *)h->tw[s], (const float2 *)h->twn[s], h->d.hop[s], T, (float)h->d.eps, dterms, h->d.n_scales, s, frames); \
        break;
        switch (h->logm[s]) {
            MSS_CASE(7) MSS_CASE(8) MSS_CASE(9) MSS_CASE(10) MSS_CASE(11)
        }
#undef MSS_CASE
        MST_CHECK_LAUNCH("mss_grad_frames_kernel");
        MST_LAUNCH(mss_grad_gather_kernel, dim3((unsigned)((L + 255) / 256), (unsigned)B), dim3(256), stream, (const float *)frames, grad, (int)L,
                   h->d.n_fft[s], h->d.hop[s], T, mix_mode, s > 0 ? 1 : 0);
        MST_CHECK_LAUNCH("mss_grad_gather_kernel");
    }
    return MST_OK;
}

extern "C" int mst_mss_spectrogram(MstMss *h, int scale, const float *x, int B, int C, long L, float *mag, void *stream) {
    if (!h || !x || !mag || B < 1 || L < 1 || scale < 0 || scale >= h->d.n_scales) return fail(MST_ERR_ARG, "mst_mss_spectrogram: bad argument");
    if (C != 1 && C != 2) return fail(MST_ERR_UNSUPPORTED, "mst_mss_spectrogram: C = " + std::to_string(C) + " (1 or 2 channels)");
    int rc;
    if ((rc = mss_check_length(h, scale, scale, B, L, "mst_mss_spectrogram"))) return rc;
    return mss_launch<MSS_EPI_MAG>(h, scale, x, C == 2 ? x + L : nullptr, (long)C * L, B, 1, L, 0, nullptr, mag, C, stream);
}

// ---- contrastive and gain training losses (csrc/contrast_kernels.h) ---------------------------------------------------------------------
namespace {
struct NtxPlan {
    int N, M, Nc;                   // rows of cat(a, b); rows and columns of S (mode 0: N x N, mode 1: n_a x n_b)
    double *rowterm;                // [N] float64
    float *S, *zh, *invn;           // [M, Nc], [N, D], [2, N]
};
size_t ntx_bytes(int n_a, int n_b, int D) {
    const size_t N = (size_t)n_a + (size_t)n_b;
    return 256 + align_up(N * sizeof(double), 256) + align_up(N * N * sizeof(float), 256) + align_up(N * (size_t)D * sizeof(float), 256) +
           align_up(2 * N * sizeof(float), 256);
}
int ntx_check(const char *who, const float *a, const float *b, int n_a, int n_b, int D, double inv_tau, double eps, int mode, const void *ws,
              size_t ws_bytes, NtxPlan &p) {
    if (!a || !b || n_a < 1 || n_b < 1 || D < 1 || !(inv_tau > 0.0) || !(eps >= 0.0) || (mode != 0 && mode != 1))
        return fail(MST_ERR_ARG, std::string(who) + ": bad argument");
    if (n_a != n_b)
        return fail(MST_ERR_UNSUPPORTED, std::string(who) + ": n_a = " + std::to_string(n_a) + ", n_b = " + std::to_string(n_b) + " (the two views must have as many rows)");
    const long N = (long)n_a + n_b;
    if (N > 4096) return fail(MST_ERR_UNSUPPORTED, std::string(who) + ": N = " + std::to_string(N) + " rows (at most 4096)");
    if (mode == 0 && (N & 1)) return fail(MST_ERR_UNSUPPORTED, std::string(who) + ": N = " + std::to_string(N) + " rows (NT-Xent pairs row i with row i + N / 2: N must be even)");
    if (D > 8192) return fail(MST_ERR_UNSUPPORTED, std::string(who) + ": D = " + std::to_string(D) + " (at most 8192)");
    if (!ws || ws_bytes < ntx_bytes(n_a, n_b, D)) return fail(MST_ERR_WORKSPACE, std::string(who) + ": workspace null or too small");
    p.N = (int)N;
    p.M = mode == 0 ? (int)N : n_a;
    p.Nc = mode == 0 ? (int)N : n_b;
    unsigned char *q = (unsigned char *)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    p.rowterm = (double *)q;
    q += align_up((size_t)N * sizeof(double), 256);
    p.S = (float *)q;
    q += align_up((size_t)N * N * sizeof(float), 256);
    p.zh = (float *)q;
    q += align_up((size_t)N * D * sizeof(float), 256);
    p.invn = (float *)q;
    return MST_OK;
}
// normalise and S (skipped when the workspace still holds a forward's), then per row: `dloss` null the loss terms, otherwise G in place of S
int ntx_front(const NtxPlan &p, const float *a, const float *b, int n_a, int D, double inv_tau, double eps, int mode, const double *dloss,
              bool have_s, void *stream) {
    if (!have_s) {
        MST_LAUNCH(ntx_normalize_kernel, dim3((unsigned)p.N), dim3(NTX_THREADS), stream, a, b, n_a, p.N, D, eps, p.zh, p.invn);
        MST_CHECK_LAUNCH("ntx_normalize_kernel");
        const float *Y = mode == 0 ? p.zh : p.zh + (size_t)n_a * D;
        MST_LAUNCH(ntx_gram_kernel, dim3((unsigned)((p.M + NTX_TILE - 1) / NTX_TILE), (unsigned)((p.Nc + NTX_COLS - 1) / NTX_COLS)), dim3(NTX_THREADS), stream,
                   (const float *)p.zh, Y, p.M, p.Nc, D, (float)inv_tau, p.S);
        MST_CHECK_LAUNCH("ntx_gram_kernel");
    }
    MST_LAUNCH(ntx_rows_kernel, dim3((unsigned)p.M), dim3(NTX_THREADS), stream, p.S, p.M, p.Nc, mode == 0 ? 1 : 0, mode == 0 ? p.N / 2 : 0, dloss,
               p.rowterm);
    MST_CHECK_LAUNCH("ntx_rows_kernel");
    return MST_OK;
}
}  // namespace

extern "C" size_t mst_ntxent_workspace_bytes(int n_a, int n_b, int D, int with_grad) {
    (void)with_grad;      // the backward writes G over S: it needs no more than the forward
    if (n_a < 1 || n_b < 1 || D < 1 || (long)n_a + n_b > 4096 || D > 8192) return 0;
    return ntx_bytes(n_a, n_b, D);
}

extern "C" int mst_ntxent_forward(const float *a, const float *b, int n_a, int n_b, int D, double inv_tau, double eps, int mode, double *loss,
                                  void *ws, size_t ws_bytes, void *stream) {
    NtxPlan p;
    int rc;
    if (!loss) return fail(MST_ERR_ARG, "mst_ntxent_forward: bad argument");
    if ((rc = ntx_check("mst_ntxent_forward", a, b, n_a, n_b, D, inv_tau, eps, mode, ws, ws_bytes, p))) return rc;
    if ((rc = ntx_front(p, a, b, n_a, D, inv_tau, eps, mode, nullptr, false, stream))) return rc;
    MST_LAUNCH(ntx_mean_kernel, dim3(1), dim3(NTX_THREADS), stream, (const double *)p.rowterm, p.M, loss);
    MST_CHECK_LAUNCH("ntx_mean_kernel");
    return MST_OK;
}

extern "C" int mst_ntxent_backward(const float *a, const float *b, int n_a, int n_b, int D, double inv_tau, double eps, int mode,
                                   const double *dloss, float *grad_a, float *grad_b, int ws_from_forward, void *ws, size_t ws_bytes,
                                   void *stream) {
    NtxPlan p;
    int rc;
    if (!dloss || !grad_a || !grad_b || grad_a == grad_b) return fail(MST_ERR_ARG, "mst_ntxent_backward: bad argument");
    if ((rc = ntx_check("mst_ntxent_backward", a, b, n_a, n_b, D, inv_tau, eps, mode, ws, ws_bytes, p))) return rc;
    if ((rc = ntx_front(p, a, b, n_a, D, inv_tau, eps, mode, dloss, ws_from_forward != 0, stream))) return rc;
    const unsigned gy = (unsigned)((D + NTX_COLS - 1) / NTX_COLS);
    if (mode == 0) {
        MST_LAUNCH(ntx_grad_kernel, dim3((unsigned)((p.N + NTX_TILE - 1) / NTX_TILE), gy), dim3(NTX_THREADS), stream, (const float *)p.S, p.N, p.N, p.N, 1, 1,
                   (const float *)p.zh, D, (float)inv_tau, grad_a, grad_b, n_a);
        MST_CHECK_LAUNCH("ntx_grad_kernel");
    } else {
        const dim3 grid((unsigned)((n_a + NTX_TILE - 1) / NTX_TILE), gy);
        MST_LAUNCH(ntx_grad_kernel, grid, dim3(NTX_THREADS), stream, (const float *)p.S, n_a, n_b, n_b, 1, 0, (const float *)(p.zh + (size_t)n_a * D), D,
                   (float)inv_tau, grad_a, grad_a, n_a);
        MST_CHECK_LAUNCH("ntx_grad_kernel");
        MST_LAUNCH(ntx_grad_kernel, grid, dim3(NTX_THREADS), stream, (const float *)p.S, n_b, n_a, n_b, 0, 1, (const float *)p.zh, D, (float)inv_tau, grad_b,
                   grad_b, n_b);
        MST_CHECK_LAUNCH("ntx_grad_kernel");
    }
    MST_LAUNCH(ntx_project_kernel, dim3((unsigned)p.N), dim3(NTX_THREADS), stream, grad_a, grad_b, n_a, (const float *)p.zh, (const float *)(p.invn + p.N), D);
    MST_CHECK_LAUNCH("ntx_project_kernel");
    return MST_OK;
}

namespace {
struct RmsPlan {
    int nchunks;
    double *partial, *coef, *rms;      // [2, rows, nchunks], [rows], [2, rows]
};
size_t rms_bytes(int rows, long T) {
    const size_t nchunks = (size_t)((T + RMS_CHUNK - 1) / RMS_CHUNK);
    return 256 + align_up(2 * (size_t)rows * nchunks * sizeof(double), 256) + align_up((size_t)rows * sizeof(double), 256) +
           align_up(2 * (size_t)rows * sizeof(double), 256);
}
int rms_check(const char *who, const float *est, const float *tgt, int rows, long T, double wf, const void *ws, size_t ws_bytes, RmsPlan &p) {
    if (!est || !tgt || rows < 1 || T < 1 || !(wf > 0.0)) return fail(MST_ERR_ARG, std::string(who) + ": bad argument");
    if (rows > 65535) return fail(MST_ERR_UNSUPPORTED, std::string(who) + ": rows = " + std::to_string(rows) + " (at most 65535 rows per call)");
    if (T >= (1L << 30)) return fail(MST_ERR_UNSUPPORTED, std::string(who) + ": T = " + std::to_string(T) + " (below 2^30)");
    if (!ws || ws_bytes < rms_bytes(rows, T)) return fail(MST_ERR_WORKSPACE, std::string(who) + ": workspace null or too small");
    p.nchunks = (int)((T + RMS_CHUNK - 1) / RMS_CHUNK);
    unsigned char *q = (unsigned char *)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    p.partial = (double *)q;
    q += align_up(2 * (size_t)rows * p.nchunks * sizeof(double), 256);
    p.coef = (double *)q;
    q += align_up((size_t)rows * sizeof(double), 256);
    p.rms = (double *)q;
    return MST_OK;
}
int rms_front(const RmsPlan &p, const float *est, const float *tgt, int rows, long T, double wf, const double *dloss, double *loss, void *stream) {
    MST_LAUNCH(rms_rows_kernel, dim3((unsigned)p.nchunks, (unsigned)rows, 2u), dim3(NTX_THREADS), stream, est, tgt, T, p.nchunks, p.partial);
    MST_CHECK_LAUNCH("rms_rows_kernel");
    MST_LAUNCH(rms_finish_kernel, dim3(1), dim3(NTX_THREADS), stream, (const double *)p.partial, rows, p.nchunks, T, wf, dloss, loss, p.coef, p.rms);
    MST_CHECK_LAUNCH("rms_finish_kernel");
    return MST_OK;
}
}  // namespace

extern "C" size_t mst_rms_loss_workspace_bytes(int rows, long T) {
    if (rows < 1 || rows > 65535 || T < 1 || T >= (1L << 30)) return 0;
    return rms_bytes(rows, T);
}

extern "C" int mst_rms_loss_forward(const float *est, const float *tgt, int rows, long T, double weight_factor, double *loss, void *ws,
                                    size_t ws_bytes, void *stream) {
    RmsPlan p;
    int rc;
    if (!loss) return fail(MST_ERR_ARG, "mst_rms_loss_forward: bad argument");
    if ((rc = rms_check("mst_rms_loss_forward", est, tgt, rows, T, weight_factor, ws, ws_bytes, p))) return rc;
    return rms_front(p, est, tgt, rows, T, weight_factor, nullptr, loss, stream);
}

extern "C" int mst_rms_loss_backward(const float *est, const float *tgt, int rows, long T, double weight_factor, const double *dloss,
                                     float *grad_est, void *ws, size_t ws_bytes, void *stream) {
    RmsPlan p;
    int rc;
    if (!dloss || !grad_est) return fail(MST_ERR_ARG, "mst_rms_loss_backward: bad argument");
    if ((rc = rms_check("mst_rms_loss_backward", est, tgt, rows, T, weight_factor, ws, ws_bytes, p))) return rc;
    if ((rc = rms_front(p, est, tgt, rows, T, weight_factor, dloss, nullptr, stream))) return rc;
    MST_LAUNCH(rms_grad_kernel, dim3((unsigned)p.nchunks, (unsigned)rows), dim3(NTX_THREADS), stream, est, (const double *)p.coef, T, grad_est);
    MST_CHECK_LAUNCH("rms_grad_kernel");
    return MST_OK;
}

// ---- mixing-feature metrics (csrc/mixfeat_kernels.h) -----------------------------------------------------------------------
struct MstMixfeat {
    int n_fft = 0, hop = 0, logm = 0;          // logm = log2(n_fft / 2)
    float *win = nullptr;                      // [n_fft]          sqrt(hanning(n_fft + 1)[:-1])
    float2 *tw = nullptr;                      // [n_fft / 4]      exp(-2 pi i j / (n_fft / 2))
    float2 *twn = nullptr;                     // [n_fft / 4 + 1]  exp(-2 pi i k / n_fft)
};

namespace {
long mixfeat_frames(const MstMixfeat *h, long L) { return L < h->n_fft ? 0 : 1 + (L - h->n_fft) / h->hop; }
int mixfeat_check(const MstMixfeat *h, const void *x, const void *out, int n_items, long L, const char *who) {
    if (!h || !x || !out || n_items < 1 || L < 1) return fail(MST_ERR_ARG, std::string(who) + ": bad argument");
    if (n_items > 65535) return fail(MST_ERR_UNSUPPORTED, std::string(who) + ": n_items = " + std::to_string(n_items) + " (at most 65535 items per call)");
    if (L < h->n_fft || L >= (1L << 30))
        return fail(MST_ERR_UNSUPPORTED, std::string(who) + ": L = " + std::to_string(L) + " leaves no frame at n_fft = " + std::to_string(h->n_fft) +
                                             " (or reaches 2^30)");
    return MST_OK;
}
template <int EPI>
int mixfeat_launch(const MstMixfeat *h, const float *xa, const float *xb, int n_items, int nchan, long L, int C, const float *sa, const float *sb,
                   const MixfeatBands &bands, double *out_sum, float *phi, float *sps, void *stream) {
    const int T = (int)mixfeat_frames(h, L), G = MSS_PTS / h->n_fft;
    const dim3 grid((unsigned)((T + G - 1) / G), (unsigned)nchan, (unsigned)n_items);
#define MIXFEAT_CASE(LM)                                                                                                              \
    case LM:                                                                                                                          \
        MST_LAUNCH((mixfeat_frames_kernel<LM, EPI>), grid, dim3(256), stream, xa, xb, L * C, C, sa, sb, (const float *)h->win,        \
                   (const float2 *)h->tw, (const float2 *)h->twn, h->hop, T, bands, out_sum, phi, sps);                               \
        break;
    switch (h->logm) {
        MIXFEAT_CASE(8) MIXFEAT_CASE(9) MIXFEAT_CASE(10) MIXFEAT_CASE(11)
    }
#undef MIXFEAT_CASE
    MST_CHECK_LAUNCH("mixfeat_frames_kernel");
    return MST_OK;
}
}  // namespace

extern "C" int mst_mixfeat_destroy(MstMixfeat *h) {
    if (!h) return MST_OK;
    (void)hipFree(h->win);
    (void)hipFree(h->tw);
    (void)hipFree(h->twn);
    delete h;
    return MST_OK;
}

extern "C" int mst_mixfeat_create(int n_fft, int hop, MstMixfeat **out) {
    if (!out) return fail(MST_ERR_ARG, "mst_mixfeat_create: null argument");
    if (n_fft < 512 || n_fft > 4096 || (n_fft & (n_fft - 1)))
        return fail(MST_ERR_UNSUPPORTED, "mst_mixfeat_create: n_fft = " + std::to_string(n_fft) + " (a power of two, 512 .. 4096)");
    if (hop < 1 || hop > n_fft) return fail(MST_ERR_UNSUPPORTED, "mst_mixfeat_create: hop = " + std::to_string(hop) + " (1 .. n_fft = " + std::to_string(n_fft) + ")");
    auto *h = new MstMixfeat();
    h->n_fft = n_fft;
    h->hop = hop;
    const int n = n_fft, m = n / 2;
    while ((1 << h->logm) < m) ++h->logm;
    const double pi = 3.14159265358979323846;
    std::vector<float> win((size_t)n);          // numpy: hanning(n + 1)[i] = 0.5 - 0.5 cos(2 pi i / n), float64; the root rounded once
    for (int i = 0; i < n; ++i) win[i] = (float)sqrt(0.5 - 0.5 * cos(2.0 * pi * (double)i / (double)n));
    std::vector<float2> tw((size_t)m / 2), twn((size_t)m / 2 + 1);
    for (int j = 0; j < m / 2; ++j) tw[j] = make_float2((float)cos(-2.0 * pi * j / m), (float)sin(-2.0 * pi * j / m));
    for (int k = 0; k <= m / 2; ++k) twn[k] = make_float2((float)cos(-2.0 * pi * k / n), (float)sin(-2.0 * pi * k / n));
    int rc;
    if ((rc = upload(&h->win, win)) || (rc = upload(&h->tw, tw)) || (rc = upload(&h->twn, twn))) {
        mst_mixfeat_destroy(h);
        return rc;
    }
    *out = h;
    return MST_OK;
}

extern "C" int mst_mixfeat_frames(const MstMixfeat *h, long L) {
    if (!h || L < 1) return fail(MST_ERR_ARG, "mst_mixfeat_frames: bad argument");
    return (int)mixfeat_frames(h, L);
}

extern "C" int mst_mixfeat_panning(MstMixfeat *h, const float *x, int n_items, long L, const float *scale, const int *band_lo, const int *band_hi,
                                   int n_bands, double *out, void *stream) {
    int rc;
    if ((rc = mixfeat_check(h, x, out, n_items, L, "mst_mixfeat_panning"))) return rc;
    if (!band_lo || !band_hi) return fail(MST_ERR_ARG, "mst_mixfeat_panning: null band edges");
    if (n_bands < 1 || n_bands > MIXFEAT_MAX_BANDS)
        return fail(MST_ERR_UNSUPPORTED, "mst_mixfeat_panning: n_bands = " + std::to_string(n_bands) + " (1 .. 8)");
    MixfeatBands bands;
    bands.n = n_bands;
    for (int j = 0; j < MIXFEAT_MAX_BANDS; ++j) bands.lo[j] = bands.hi[j] = 0;
    for (int j = 0; j < n_bands; ++j) {
        if (band_lo[j] < 0 || band_hi[j] < band_lo[j] || band_hi[j] > h->n_fft / 2 + 1)
            return fail(MST_ERR_ARG, "mst_mixfeat_panning: band " + std::to_string(j) + " = [" + std::to_string(band_lo[j]) + ", " +
                                         std::to_string(band_hi[j]) + ") is not inside 0 .. n_fft / 2 + 1");
        bands.lo[j] = band_lo[j];
        bands.hi[j] = band_hi[j];
    }
    return mixfeat_launch<MIXFEAT_EPI_PANNING>(h, x, x + 1, n_items, 1, L, 2, scale, scale, bands, out, nullptr, nullptr, stream);
}

extern "C" int mst_mixfeat_sps(MstMixfeat *h, const float *x, int n_items, long L, const float *scale, float *phi, float *sps, void *stream) {
    int rc;
    if ((rc = mixfeat_check(h, x, phi, n_items, L, "mst_mixfeat_sps"))) return rc;
    if (!sps) return fail(MST_ERR_ARG, "mst_mixfeat_sps: bad argument");
    MixfeatBands bands;
    bands.n = 0;
    return mixfeat_launch<MIXFEAT_EPI_PANNING_STORE>(h, x, x + 1, n_items, 1, L, 2, scale, scale, bands, nullptr, phi, sps, stream);
}

extern "C" int mst_mixfeat_low_ratio(MstMixfeat *h, const float *x_low, const float *x, int n_items, long L, int C, const float *scale_low,
                                     const float *scale, double *out, void *stream) {
    int rc;
    if ((rc = mixfeat_check(h, x, out, n_items, L, "mst_mixfeat_low_ratio"))) return rc;
    if (!x_low) return fail(MST_ERR_ARG, "mst_mixfeat_low_ratio: bad argument");
    if (C != 1 && C != 2) return fail(MST_ERR_UNSUPPORTED, "mst_mixfeat_low_ratio: C = " + std::to_string(C) + " (1 or 2 channels)");
    MixfeatBands bands;
    bands.n = 1;
    return mixfeat_launch<MIXFEAT_EPI_LOW_RATIO>(h, x_low, x, n_items, C, L, C, scale_low, scale, bands, out, nullptr, nullptr, stream);
}

extern "C" int mst_mixfeat_spectral(MstMixfeat *h, const float *x, int n_items, long L, int C, const float *scale, const int *band_lo,
                                    const int *band_hi, const int *band_k, int n_bands, double *out, void *stream) {
    int rc;
    if ((rc = mixfeat_check(h, x, out, n_items, L, "mst_mixfeat_spectral"))) return rc;
    if (C != 1 && C != 2) return fail(MST_ERR_UNSUPPORTED, "mst_mixfeat_spectral: C = " + std::to_string(C) + " (1 or 2 channels)");
    if (!band_lo || !band_hi || !band_k) return fail(MST_ERR_ARG, "mst_mixfeat_spectral: null band arrays");
    if (n_bands < 1 || n_bands > MIXFEAT_SPEC_BANDS)          // the 16 numbers of a frame hold five bands' pairs behind the six sums
        return fail(MST_ERR_UNSUPPORTED, "mst_mixfeat_spectral: n_bands = " + std::to_string(n_bands) + " (1 .. 5: a frame's 16 numbers hold no more)");
    MixfeatSelBands bands;
    bands.n = n_bands;
    for (int j = 0; j < MIXFEAT_SPEC_BANDS; ++j) {
        bands.lo[j] = bands.hi[j] = 0;
        bands.k[j] = 1;
    }
    for (int j = 0; j < n_bands; ++j) {
        if (band_lo[j] < 0 || band_hi[j] <= band_lo[j] || band_hi[j] > h->n_fft / 2 + 1)
            return fail(MST_ERR_ARG, "mst_mixfeat_spectral: band " + std::to_string(j) + " = [" + std::to_string(band_lo[j]) + ", " +
                                         std::to_string(band_hi[j]) + ") is empty or not inside 0 .. n_fft / 2 + 1");
        if (band_k[j] < 1 || band_k[j] > band_hi[j] - band_lo[j])
            return fail(MST_ERR_ARG, "mst_mixfeat_spectral: band " + std::to_string(j) + ": k = " + std::to_string(band_k[j]) + " (1 .. " +
                                         std::to_string(band_hi[j] - band_lo[j]) + ", the band's bins)");
        bands.lo[j] = band_lo[j];
        bands.hi[j] = band_hi[j];
        bands.k[j] = band_k[j];
    }
    const int T = (int)mixfeat_frames(h, L), G = MSS_PTS / h->n_fft;
    const dim3 grid((unsigned)((T + G - 1) / G), 1, (unsigned)n_items);
#define MIXFEAT_CASE(LM)                                                                                                              \
    case LM:                                                                                                                          \
        MST_LAUNCH((mixfeat_spectral_kernel<LM>), grid, dim3(256), stream, x, L * C, C, scale, (const float *)h->win,                 \
                   (const float2 *)h->tw, (const float2 *)h->twn, h->hop, T, bands, out);                                             \
        break;
    switch (h->logm) {
        MIXFEAT_CASE(8) MIXFEAT_CASE(9) MIXFEAT_CASE(10) MIXFEAT_CASE(11)
    }
#undef MIXFEAT_CASE
    MST_CHECK_LAUNCH("mixfeat_spectral_kernel");
    return MST_OK;
}

extern "C" int mst_mixfeat_dynamics(const float *x, int n_items, long L, int C, const float *scale, int frame_length, int hop, double *out,
                                    void *stream) {
    if (!x || !out || n_items < 1 || L < 1) return fail(MST_ERR_ARG, "mst_mixfeat_dynamics: bad argument");
    if (C != 1 && C != 2) return fail(MST_ERR_UNSUPPORTED, "mst_mixfeat_dynamics: C = " + std::to_string(C) + " (1 or 2 channels)");
    if (n_items > 65535) return fail(MST_ERR_UNSUPPORTED, "mst_mixfeat_dynamics: n_items = " + std::to_string(n_items) + " (at most 65535 items per call)");
    if (frame_length < 1 || frame_length > (1 << 20))
        return fail(MST_ERR_UNSUPPORTED, "mst_mixfeat_dynamics: frame_length = " + std::to_string(frame_length) + " (1 .. 2^20)");
    if (hop < 1) return fail(MST_ERR_UNSUPPORTED, "mst_mixfeat_dynamics: hop = " + std::to_string(hop) + " (at least 1)");
    if (L < frame_length || L >= (1L << 30))
        return fail(MST_ERR_UNSUPPORTED, "mst_mixfeat_dynamics: L = " + std::to_string(L) + " leaves no frame of " + std::to_string(frame_length) +
                                             " samples (or reaches 2^30)");
    const long T = 1 + (L - frame_length) / hop;
    // hop blocks combined in a fixed order when hop divides the frame length (and a frame's blocks fit half a workgroup's table), else whole frames
    const bool blocked = frame_length % hop == 0 && frame_length / hop <= MIXFEAT_DYN_BLOCKS / 2;
    const int R = blocked ? frame_length / hop : 1, blk = blocked ? hop : frame_length, fpw = MIXFEAT_DYN_BLOCKS - R + 1;
    MST_LAUNCH(mixfeat_dynamics_kernel, dim3((unsigned)((T + fpw - 1) / fpw), 1, (unsigned)n_items), dim3(256), stream, x, L * C, C, scale, blk,
               hop, R, fpw, (int)T, out);
    MST_CHECK_LAUNCH("mixfeat_dynamics_kernel");
    return MST_OK;
}

// ---- polyphase resampler (csrc/resample_kernels.h) ---------------------------------------------------------------------------
struct MstResampler {
    int rate_in = 0, rate_out = 0, up = 0, down = 0, half = 0, T = 0;
    std::vector<float> h;                      // the 2 half + 1 prototype taps, float32
    float *taps = nullptr;                     // [T * up]: h, zero-padded
};

namespace {
const long RESAMPLE_MAX_POS = 1L << 48;        // positions below it: m down + half stays far inside 63 bits
// I0(x), the power series sum ((x / 2)^k / k!)^2: every term positive, relative error of a few float64 steps at x <= 12
double resample_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 200 && term > 1e-18 * sum; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
    }
    return sum;
}
int resample_gcd(int a, int b) {
    while (b) { const int t = a % b; a = b; b = t; }
    return a;
}
}  // namespace

extern "C" int mst_resample_destroy(MstResampler *r) {
    if (!r) return MST_OK;
    (void)hipFree(r->taps);
    delete r;
    return MST_OK;
}

extern "C" int mst_resample_create(int rate_in, int rate_out, MstResampler **out) {
    if (!out) return fail(MST_ERR_ARG, "mst_resample_create: null argument");
    if (rate_in < 1 || rate_out < 1)
        return fail(MST_ERR_ARG, "mst_resample_create: rates " + std::to_string(rate_in) + " -> " + std::to_string(rate_out) + " (positive rates)");
    if (rate_in == rate_out) return fail(MST_ERR_ARG, "mst_resample_create: equal rates (" + std::to_string(rate_in) + "): nothing to resample");
    const int g = resample_gcd(rate_in, rate_out), up = rate_out / g, down = rate_in / g;
    const std::string ratio = std::to_string(rate_in) + " -> " + std::to_string(rate_out) + " Hz = " + std::to_string(up) + " / " + std::to_string(down);
    if (up > 441 || down > 640) return fail(MST_ERR_UNSUPPORTED, "mst_resample_create: " + ratio + " (up <= 441 and down <= 640)");
    const int mx = std::max(up, down), half = 64 * mx, n = 2 * half + 1, T = 2 * half / up + 1;
    const long span = ((long)up - 1 + (long)(RESAMPLE_TILE - 1) * down) / up + T;          // input frames under one tile of outputs, at most
    if (span * 2 > RESAMPLE_LDS_FLOATS)
        return fail(MST_ERR_UNSUPPORTED, "mst_resample_create: " + ratio + ": a tile of " + std::to_string(RESAMPLE_TILE) + " outputs spans " +
                                             std::to_string(span) + " input frames (at most " + std::to_string(RESAMPLE_LDS_FLOATS / 2) + ")");
    auto *r = new MstResampler();
    r->rate_in = rate_in; r->rate_out = rate_out; r->up = up; r->down = down; r->half = half; r->T = T;
    // up * scipy.signal.firwin(n, fc, window = ('kaiser', 12)), float64: sinc low-pass at fc (in units of Nyquist), Kaiser window, unit DC gain
    const double pi = 3.14159265358979323846, fc = 0.945 / (double)mx, beta = 12.0, i0b = resample_i0(beta);
    std::vector<double> gv((size_t)n);
    double sum = 0.0;
    for (int i = 0; i < n; ++i) {
        const double m = (double)(i - half), a = pi * (fc * m), u = m / (double)half;          // numpy.sinc's pi * x of x = fc m
        const double sinc = i == half ? 1.0 : sin(a) / a;
        gv[i] = fc * sinc * resample_i0(beta * sqrt(std::max(0.0, 1.0 - u * u))) / i0b;
        sum += gv[i];
    }
    r->h.resize((size_t)n);
    for (int i = 0; i < n; ++i) r->h[i] = (float)((double)up * gv[i] / sum);
    std::vector<float> tab((size_t)T * up, 0.0f);
    std::copy(r->h.begin(), r->h.end(), tab.begin());
    const int rc = upload(&r->taps, tab);
    if (rc) {
        mst_resample_destroy(r);
        return rc;
    }
    *out = r;
    return MST_OK;
}

extern "C" int mst_resample_info(const MstResampler *r, int *up, int *down, int *half_len, int *taps_per_phase) {
    if (!r) return fail(MST_ERR_ARG, "mst_resample_info: null handle");
    if (up) *up = r->up;
    if (down) *down = r->down;
    if (half_len) *half_len = r->half;
    if (taps_per_phase) *taps_per_phase = r->T;
    return MST_OK;
}

extern "C" long mst_resample_length(const MstResampler *r, long n_in) {
    if (!r || n_in < 0 || n_in >= RESAMPLE_MAX_POS) return fail(MST_ERR_ARG, "mst_resample_length: bad argument");
    return (n_in * r->up + r->down - 1) / r->down;
}

extern "C" int mst_resample_taps(const MstResampler *r, float *taps_host, int n) {
    if (!r || !taps_host) return fail(MST_ERR_ARG, "mst_resample_taps: null argument");
    if (n != 2 * r->half + 1)
        return fail(MST_ERR_ARG, "mst_resample_taps: n = " + std::to_string(n) + " (the filter has " + std::to_string(2 * r->half + 1) + " taps)");
    std::copy(r->h.begin(), r->h.end(), taps_host);
    return MST_OK;
}

extern "C" int mst_resample_forward(MstResampler *r, const float *x, long n_in, long in_start, float *y, long n_out, long out_start, int n_items,
                                    int C, void *stream) {
    if (!r || !x || !y) return fail(MST_ERR_ARG, "mst_resample_forward: null argument");
    if (C != 1 && C != 2) return fail(MST_ERR_ARG, "mst_resample_forward: C = " + std::to_string(C) + " (1 or 2 channels)");
    if (n_items < 1 || n_in < 1 || n_out < 1 || in_start < 0 || out_start < 0) return fail(MST_ERR_ARG, "mst_resample_forward: bad argument");
    if (C == 2 && ((uintptr_t)y & 7)) return fail(MST_ERR_ARG, "mst_resample_forward: y_dev of a stereo call must be 8-byte aligned");
    if (n_items > 65535) return fail(MST_ERR_UNSUPPORTED, "mst_resample_forward: n_items = " + std::to_string(n_items) + " (at most 65535 items per call)");
    if (n_in >= (1L << 30) || n_out >= (1L << 30))
        return fail(MST_ERR_UNSUPPORTED, "mst_resample_forward: " + std::to_string(n_in) + " -> " + std::to_string(n_out) +
                                             " frames in one call (below 2^30 each: cut a longer signal into chunks)");
    if (in_start >= RESAMPLE_MAX_POS || out_start >= RESAMPLE_MAX_POS)
        return fail(MST_ERR_UNSUPPORTED, "mst_resample_forward: in_start / out_start reach 2^48");
    const dim3 grid((unsigned)((n_out + RESAMPLE_TILE - 1) / RESAMPLE_TILE), 1, (unsigned)n_items);
    if (C == 2)
        MST_LAUNCH(resample_kernel<2>, grid, dim3(RESAMPLE_TILE), stream, x, n_in, in_start, y, n_out, out_start, (const float *)r->taps, r->up,
                   r->down, r->half, r->T);
    else
        MST_LAUNCH(resample_kernel<1>, grid, dim3(RESAMPLE_TILE), stream, x, n_in, in_start, y, n_out, out_start, (const float *)r->taps, r->up,
                   r->down, r->half, r->T);
    MST_CHECK_LAUNCH("resample_kernel");
    return MST_OK;
}

// ---- training batches (csrc/batch_kernels.h) -------------------------------------------------------------------------------------
namespace {
unsigned batch_grid_x(long groups) { return (unsigned)std::max(1L, (groups + BATCH_GROUPS_PER_BLOCK - 1) / BATCH_GROUPS_PER_BLOCK); }
}  // namespace

extern "C" int mst_batch_gather_pcm(const void *bank, long n_bank_frames, int width, const long *table_dev, const long *table_host, int n,
                                    long frames, float *out, void *stream) {
    if (!bank || !table_dev || !table_host || !out || n < 1 || frames < 1 || n_bank_frames < 1) return fail(MST_ERR_ARG, "mst_batch_gather_pcm: bad argument");
    if (width != 2 && width != 4) return fail(MST_ERR_ARG, "mst_batch_gather_pcm: width = " + std::to_string(width) + " (2 or 4 bytes per sample)");
    if (n > 65535) return fail(MST_ERR_UNSUPPORTED, "mst_batch_gather_pcm: n = " + std::to_string(n) + " (at most 65535 rows per call)");
    if ((uintptr_t)out & 7) return fail(MST_ERR_ARG, "mst_batch_gather_pcm: out_dev must be 8-byte aligned");
    if (frames > n_bank_frames) return fail(MST_ERR_ARG, "mst_batch_gather_pcm: " + std::to_string(frames) + " frames per row from a bank of " + std::to_string(n_bank_frames));
    for (int r = 0; r < n; ++r)
        if (table_host[r] < 0 || table_host[r] > n_bank_frames - frames)
            return fail(MST_ERR_ARG, "mst_batch_gather_pcm: row " + std::to_string(r) + ": frames " + std::to_string(table_host[r]) + " ... " +
                                         std::to_string(table_host[r]) + " + " + std::to_string(frames) + " lie outside the bank of " + std::to_string(n_bank_frames));
    const dim3 grid(batch_grid_x(frames / 4), (unsigned)n);
    if (width == 2) MST_LAUNCH(batch_gather_pcm_kernel<2>, grid, dim3(BATCH_THREADS), stream, (const unsigned char *)bank, table_dev, out, frames);
    else MST_LAUNCH(batch_gather_pcm_kernel<4>, grid, dim3(BATCH_THREADS), stream, (const unsigned char *)bank, table_dev, out, frames);
    MST_CHECK_LAUNCH("batch_gather_pcm_kernel");
    return MST_OK;
}

extern "C" int mst_batch_finish(const float *x, int n, long Lp, int C, const long *rows_dev, const long *rows_host, const long *start_dev,
                                const long *start_host, int m, long len, float *out, void *stream) {
    if (!x || !rows_dev || !rows_host || !start_dev || !start_host || !out || n < 1 || m < 1 || Lp < 1 || len < 1)
        return fail(MST_ERR_ARG, "mst_batch_finish: bad argument");
    if (C != 1 && C != 2) return fail(MST_ERR_ARG, "mst_batch_finish: C = " + std::to_string(C) + " (1 or 2 channels)");
    if (m > 65535) return fail(MST_ERR_UNSUPPORTED, "mst_batch_finish: m = " + std::to_string(m) + " (at most 65535 rows per call)");
    if (x == out) return fail(MST_ERR_ARG, "mst_batch_finish: in-place operation is not supported (the layout changes)");
    if (len > Lp) return fail(MST_ERR_ARG, "mst_batch_finish: len = " + std::to_string(len) + " of rows of " + std::to_string(Lp) + " samples");
    for (int r = 0; r < m; ++r) {
        if (rows_host[r] < 0 || rows_host[r] >= n)
            return fail(MST_ERR_ARG, "mst_batch_finish: row " + std::to_string(r) + ": source row " + std::to_string(rows_host[r]) + " outside [0, " + std::to_string(n) + ")");
        if (start_host[r] < 0 || start_host[r] > Lp - len)
            return fail(MST_ERR_ARG, "mst_batch_finish: row " + std::to_string(r) + ": samples " + std::to_string(start_host[r]) + " ... " +
                                         std::to_string(start_host[r]) + " + " + std::to_string(len) + " lie outside the " + std::to_string(Lp) + " of a row");
    }
    const dim3 grid(batch_grid_x(len / 4), (unsigned)m, (unsigned)C);
    if (C == 2) MST_LAUNCH(batch_finish_kernel<2>, grid, dim3(BATCH_THREADS), stream, x, rows_dev, start_dev, out, Lp, len);
    else MST_LAUNCH(batch_finish_kernel<1>, grid, dim3(BATCH_THREADS), stream, x, rows_dev, start_dev, out, Lp, len);
    MST_CHECK_LAUNCH("batch_finish_kernel");
    return MST_OK;
}
