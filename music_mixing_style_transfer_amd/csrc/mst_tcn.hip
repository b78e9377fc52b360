// libmst_hip.so, MixFXcloner part of the C ABI (mst_tcn_*, mst_calib_mainloop, mst_film_forward): weight packing into MFMA fragment order,
// tile geometry and launches of csrc/tcn_kernels.h.  See include/mst_hip.h for the contract.
#include "mst_host.h"
#include "tcn_kernels.h"

// =================================================================================================
// TCN
// =================================================================================================
struct MstTcnBlock {
    void *w_bf16 = nullptr;   // blocks >= 1: [60][2][4][64][8] bf16 (A fragments of v_mfma_f32_16x16x32_bf16)
    void *w_x3 = nullptr;     // blocks >= 1: [hi | lo][120][4][64][8] bf16 (bf16x3 mode: W' = W'_hi + W'_lo)
    float *w_f32 = nullptr;   // blocks >= 1: [15][4][4][4][64][4] fp32 ; block 0: [2][15][128]
    float *shift = nullptr;   // [128]
    float *res = nullptr;     // [128]
    bool loaded = false;
};

// kernel forms: the mst_tcn_set_tuning flags (include/mst_hip.h; measured at 32 x 131072: bit 0 5.13 against 5.45 ms per bf16x3 launch,
// bit 5 -0.2 ms per bf16 forward, bit 6 572 against 566 bf16x3 segments/s - profiles/r05_x3_ab_bit6_53_117.jsonl)
struct TcnTuning {
    int flags;
    bool x3_small_tiles() const { return flags & 1; }               // bf16x3: 128-time tiles of <= 2 phases, two workgroups per CU
    bool bf16_cm() const { return ((flags >> 1) & 3) == 2; }        // bf16 form 2: two- / four-phase blocks on class-major 256-time tiles
    bool bf16_fuse0() const { return bf16_cm() && (flags & 32); }   // bf16: block 0 inside the d = 2 block's launch
    bool x3_half_cm() const { return flags & 64; }                  // bf16x3: class-major loop in the eight-phase half-tile kernel
    bool bf16_whole() const { return bf16_cm() && (flags & 128); }  // bf16: whole-sequence 256-time tiles, class-major head of a four-phase last block
};

constexpr int TCN_FILM_ROWS0 = 64;      // FiLM rows reserved at create time (14 blocks x 64 rows x 256 floats = 0.9 MB)
struct MstTcn {
    MstTcnDesc d;
    bool generic = false;              // configuration outside the specialised 128-channel / k=15 kernels
    std::vector<MstEncConv> gconv;     // generic path: one packed conv per block + the output head (fp32 implicit GEMM)
    std::vector<MstTcnBlock> blk;
    float *film_w = nullptr;  // [nblocks][2C][D]
    float *film_b = nullptr;  // [nblocks][2C]
    float *film = nullptr;    // [nblocks][rows][2C]
    int film_rows = 0, film_cap = 0;
    std::vector<float *> film_retired;   // FiLM tables outgrown by a larger set_cond: kept until destroy (a forward still in flight may read them; no hipFree - a device-wide wait - on the data path)
    float *out_w = nullptr, *out_b = nullptr;
    bool out_loaded = false;
    void *zero_row = nullptr;     // 1 KB of zeros: what the block kernels stage for time steps outside the segment
    int tuning = 245;             // TcnTuning flags (mst_tcn_set_tuning)
    int last_fused0 = 0;          // whether the last forward of this handle really ran block 0 inside block 1's launch (mst_tcn_get_tuning)
    int fusion = 0;               // mst_tcn_set_fusion flags: launch-level, beside the tuning flags (a fresh handle's launch table is what the tuning flags say)
    int last_fused_tail = 0;      // whether the last forward of this handle ran its last three blocks as one launch (mst_tcn_get_fusion)
    int chunk = MST_TCN_CHUNK_WHOLE;   // mst_tcn_set_chunk: batch items per chunk of a full bf16 forward, 0 = automatic (tcn_chunk_items); like the fusion flags, a fresh handle's launch table is what the tuning flags say
    int last_chunks = 1;          // how many chunks the last forward of this handle ran (mst_tcn_get_chunk)
    hipStream_t side = nullptr;   // the second chunk chain's stream and the events of one fork / join: taken on the first chunked forward
    hipEvent_t side_fork = nullptr, side_join = nullptr;
    int side_dev = -1;
    std::vector<hipEvent_t> ev;   // timing hook: (nblocks + 2) events per chunk of a recorded forward (a pool: ev_next of them are taken)
    struct TimedForward {
        size_t first;             // its first event in ev
        int chunks, chains;       // chunks x (nblocks + 2) events; the chunks ran on `chains` streams at a time
        bool tail;                // its last three blocks were one launch (their events coincide)
    };
    std::vector<TimedForward> ev_fwd;
    size_t ev_next = 0;
    int ev_max = 0;
};

// side streams outlive the handles that use them: a destroyed handle's stream (its last work joined into the caller's stream long ago) goes
// to the next handle that chunks on the same device
static std::mutex tcn_side_mu;
static std::vector<std::pair<int, hipStream_t>> tcn_side_free;


extern "C" int mst_tcn_create(const MstTcnDesc *desc, MstTcn **out) {
    if (!desc || !out) return fail(MST_ERR_ARG, "mst_tcn_create: null argument");
    const MstTcnDesc &d = *desc;
    if (d.nblocks < 1 || d.nblocks > MST_MAX_BLOCKS) return fail(MST_ERR_ARG, "mst_tcn_create: nblocks out of range");
    if (d.channels < 1 || d.kernel_size < 1 || d.ninputs < 1 || d.noutputs < 1 || d.cond_dim < 1)
        return fail(MST_ERR_ARG, "mst_tcn_create: bad layer description");
    if (d.channels % d.ninputs != 0)
        return fail(MST_ERR_UNSUPPORTED, "mst_tcn_create: channel_width must be a multiple of ninputs (grouped 1x1 residual)");
    const bool fast = d.channels == 128 && d.kernel_size == 15 && d.ninputs == 2 && d.noutputs <= 2 && d.dilations[0] == 1 && !d.causal;
    for (int n = 0; n < d.nblocks; ++n)
        if (d.dilations[n] < 1) return fail(MST_ERR_ARG, "mst_tcn_create: dilation < 1");
    MstTcn *t = new MstTcn();
    t->d = d;
    t->generic = !fast;
    t->blk.resize(d.nblocks);
    if (t->generic) {
        t->gconv.resize(d.nblocks + 1);
        for (int n = 0; n < d.nblocks; ++n) {
            const int span = (d.kernel_size - 1) * d.dilations[n];          // architectures.py:199: span/2 each side, or all of it on the
            const int pad_l = d.causal ? span : span / 2;                   // left for a causal block (pad both sides, drop the tail)
            conv_geometry(t->gconv[n], n == 0 ? d.ninputs : d.channels, d.channels, d.kernel_size, 1, d.dilations[n], pad_l, span - pad_l);
        }
        conv_geometry(t->gconv[d.nblocks], d.channels, d.noutputs, 1, 1, 1, 0, 0);
    }
    const size_t fw = (size_t)d.nblocks * 2 * d.channels * d.cond_dim;
    if (hipMalloc((void **)&t->film_w, fw * sizeof(float)) != hipSuccess ||
        hipMalloc((void **)&t->film_b, (size_t)d.nblocks * 2 * d.channels * sizeof(float)) != hipSuccess ||
        hipMalloc(&t->zero_row, 1024) != hipSuccess || hipMemset(t->zero_row, 0, 1024) != hipSuccess ||
        hipMalloc((void **)&t->film, (size_t)d.nblocks * TCN_FILM_ROWS0 * 2 * d.channels * sizeof(float)) != hipSuccess) {
        (void)hipFree(t->film_w);
        (void)hipFree(t->film_b);
        (void)hipFree(t->zero_row);
        (void)hipFree(t->film);
        delete t;
        return fail(MST_ERR_HIP, "mst_tcn_create: hipMalloc failed");
    }
    t->film_cap = TCN_FILM_ROWS0;
    *out = t;
    return MST_OK;
}

extern "C" int mst_tcn_destroy(MstTcn *t) {
    if (!t) return MST_OK;
    for (auto &b : t->blk) {
        (void)hipFree(b.w_bf16);
        (void)hipFree(b.w_x3);
        (void)hipFree(b.w_f32);
        (void)hipFree(b.shift);
        (void)hipFree(b.res);
    }
    (void)hipFree(t->film_w);
    (void)hipFree(t->film_b);
    (void)hipFree(t->film);
    for (float *f : t->film_retired) (void)hipFree(f);
    (void)hipFree(t->out_w);
    (void)hipFree(t->out_b);
    (void)hipFree(t->zero_row);
    for (auto &c : t->gconv) {
        (void)hipFree(c.wpk);
        (void)hipFree(c.ktab);
        (void)hipFree(c.shift);
    }
    for (auto e : t->ev) (void)hipEventDestroy(e);
    if (t->side_fork) (void)hipEventDestroy(t->side_fork);
    if (t->side_join) (void)hipEventDestroy(t->side_join);
    if (t->side_dev >= 0) {
        std::lock_guard<std::mutex> lock(tcn_side_mu);
        tcn_side_free.emplace_back(t->side_dev, t->side);
    }
    delete t;
    return MST_OK;
}

extern "C" int mst_tcn_load_block(MstTcn *t, int n, const float *conv_w, const float *bn_weight, const float *bn_bias,
                                  const float *bn_mean, const float *bn_var, float bn_eps, const float *film_w,
                                  const float *film_b, const float *res_w, void *) {
    if (!t || !conv_w || !bn_weight || !bn_bias || !bn_mean || !bn_var || !film_w || !film_b || !res_w)
        return fail(MST_ERR_ARG, "mst_tcn_load_block: null argument");
    if (n < 0 || n >= t->d.nblocks) return fail(MST_ERR_ARG, "mst_tcn_load_block: block index out of range");
    const int C = t->d.channels, K = t->d.kernel_size;
    const int cin = n == 0 ? t->d.ninputs : C;
    std::vector<float> scale, shift;
    bn_fold(bn_weight, bn_bias, bn_mean, bn_var, bn_eps, C, scale, shift);
    MstTcnBlock &b = t->blk[n];
    auto W = [&](int co, int ci, int j) { return conv_w[((size_t)co * cin + ci) * K + j] * scale[co]; };
    int rc;
    if (t->generic) {
        MstEncConv &c = t->gconv[n];
        if ((rc = pack_conv_f32(c, conv_w, scale))) return rc;
        std::vector<float> sh((size_t)((C + 32 * c.mw - 1) / (32 * c.mw)) * 32 * c.mw, 0.0f);
        for (int co = 0; co < C; ++co) sh[co] = shift[co];
        if ((rc = upload(&c.shift, sh))) return rc;
        c.loaded = true;
    } else if (n == 0) {
        std::vector<float> w0((size_t)cin * K * C);
        for (int ci = 0; ci < cin; ++ci)
            for (int j = 0; j < K; ++j)
                for (int co = 0; co < C; ++co) w0[((size_t)ci * K + j) * C + co] = W(co, ci, j);
        if ((rc = upload(&b.w_f32, w0))) return rc;
        // bf16 A fragments of the matrix-core block-0 kernel: [s][wave][lane][e], k = ci * 15 + j
        std::vector<__bf16> wb((size_t)2 * 4 * 64 * 8);
        for (int sI = 0; sI < 2; ++sI)
            for (int w = 0; w < 4; ++w)
                for (int l = 0; l < 64; ++l)
                    for (int e = 0; e < 8; ++e) {
                        const int k = 16 * sI + 8 * (l >> 5) + e;
                        wb[(((size_t)sI * 4 + w) * 64 + l) * 8 + e] = k < 30 ? (__bf16)W(32 * w + (l & 31), k / 15, k % 15) : (__bf16)0.0f;
                    }
        if ((rc = upload((__bf16 **)&b.w_bf16, wb))) return rc;
    } else {
        // bf16 A fragments of v_mfma_f32_16x16x32_bf16: [ks = j*4 + kk][row tile m][wave][lane][e]; bf16x3 mode: the same fragment image twice,
        // W'_hi = bf16(W') and W'_lo = bf16(W' - W'_hi)
        const size_t image = (size_t)120 * 4 * 64 * 8;
        std::vector<__bf16> wb(image), wx(2 * image);
        for (int j = 0; j < K; ++j)
            for (int kk = 0; kk < 4; ++kk)
                for (int m = 0; m < 2; ++m)
                    for (int w = 0; w < 4; ++w)
                        for (int l = 0; l < 64; ++l)
                            for (int e = 0; e < 8; ++e) {
                                const float v = W(32 * w + 16 * m + (l & 15), 32 * kk + 8 * (l >> 4) + e, j);
                                const __bf16 hi = (__bf16)v;
                                const size_t idx = (((((size_t)(j * 4 + kk) * 2 + m) * 4 + w) * 64 + l) * 8) + e;
                                wb[idx] = wx[idx] = hi;
                                wx[image + idx] = (__bf16)(v - (float)hi);
                            }
        if ((rc = upload((__bf16 **)&b.w_bf16, wb))) return rc;
        if ((rc = upload((__bf16 **)&b.w_x3, wx))) return rc;
        // fp32 A fragments of v_mfma_f32_32x32x2_f32: [j][chunk c][ksg][wave][lane][i]
        std::vector<float> wf((size_t)K * 4 * 4 * 4 * 64 * 4);
        for (int j = 0; j < K; ++j)
            for (int c = 0; c < 4; ++c)
                for (int ksg = 0; ksg < 4; ++ksg)
                    for (int w = 0; w < 4; ++w)
                        for (int l = 0; l < 64; ++l)
                            for (int i = 0; i < 4; ++i)
                                wf[(((((size_t)(j * 4 + c) * 4 + ksg) * 4 + w) * 64 + l) * 4) + i] =
                                    W(32 * w + (l & 31), 32 * c + 2 * (4 * ksg + i) + (l >> 5), j);
        if ((rc = upload(&b.w_f32, wf))) return rc;
    }
    if (!t->generic && (rc = upload(&b.shift, shift))) return rc;      // (the generic conv keeps its shift, padded, with its packed weights)
    std::vector<float> res(res_w, res_w + C);
    if ((rc = upload(&b.res, res))) return rc;
    const size_t fwn = (size_t)2 * C * t->d.cond_dim;
    MST_HIP_TRY(hipMemcpy(t->film_w + (size_t)n * fwn, film_w, fwn * sizeof(float), hipMemcpyHostToDevice));
    MST_HIP_TRY(hipMemcpy(t->film_b + (size_t)n * 2 * C, film_b, 2 * C * sizeof(float), hipMemcpyHostToDevice));
    b.loaded = true;
    return MST_OK;
}

extern "C" int mst_tcn_load_output(MstTcn *t, const float *w, const float *b, void *) {
    if (!t || !w || !b) return fail(MST_ERR_ARG, "mst_tcn_load_output: null argument");
    int rc;
    if (t->generic) {
        MstEncConv &c = t->gconv[t->d.nblocks];
        std::vector<float> ones(t->d.noutputs, 1.0f);
        if ((rc = pack_conv_f32(c, w, ones))) return rc;
        std::vector<float> sh((size_t)32 * c.mw * ((t->d.noutputs + 32 * c.mw - 1) / (32 * c.mw)), 0.0f);
        for (int o = 0; o < t->d.noutputs; ++o) sh[o] = b[o];
        if ((rc = upload(&c.shift, sh))) return rc;
        c.loaded = t->out_loaded = true;
        return MST_OK;
    }
    std::vector<float> wv(w, w + (size_t)t->d.noutputs * 128), bv(b, b + t->d.noutputs);
    if ((rc = upload(&t->out_w, wv))) return rc;
    if ((rc = upload(&t->out_b, bv))) return rc;
    t->out_loaded = true;
    return MST_OK;
}

extern "C" int mst_tcn_set_cond(MstTcn *t, const float *cond_dev, int n_rows, long block_stride, void *stream) {
    if (!t || !cond_dev || n_rows < 1 || block_stride < 0) return fail(MST_ERR_ARG, "mst_tcn_set_cond: bad argument");
    for (auto &b : t->blk)
        if (!b.loaded) return fail(MST_ERR_STATE, "mst_tcn_set_cond: block weights not loaded");
    if (n_rows > t->film_cap) {
        // the table is a high-water buffer: mst_tcn_create reserves TCN_FILM_ROWS0 rows (one pass of the whole-stem engine at 131072-sample
        // segments), so the per-pass set_cond of the interpolation loop never allocates.  More rows than ever before: a NEW table of at least
        // twice the size; the old one is retired, not freed (hipFree waits for the whole device and a forward in flight may still read it)
        const int cap = std::max(n_rows, 2 * t->film_cap);
        float *grown = nullptr;
        MST_HIP_TRY(hipMalloc((void **)&grown, (size_t)t->d.nblocks * cap * 2 * t->d.channels * sizeof(float)));
        t->film_retired.push_back(t->film);
        t->film = grown;
        t->film_cap = cap;
    }
    FilmArgs a;
    a.fw = t->film_w;
    a.fb = t->film_b;
    a.cond = cond_dev;
    a.film = t->film;
    a.nblocks = t->d.nblocks;
    a.two_c = 2 * t->d.channels;
    a.D = t->d.cond_dim;
    a.rows = n_rows;
    a.block_stride = block_stride;
    const int outs = t->d.nblocks * 2 * t->d.channels;
    MST_LAUNCH(tcn_film_kernel, dim3((outs + 3) / 4), dim3(256), stream, a);
    MST_CHECK_LAUNCH("tcn_film_kernel");
    t->film_rows = n_rows;
    return MST_OK;
}

namespace {

size_t tcn_elem(int precision) { return precision == MST_PREC_BF16 ? 2 : 4; }      // bf16x3 keeps fp32 activations in HBM

// ---- the launch plan of one dense block (blocks >= 1): everything that is decided per block, decided once, by tcn_plan_block ----
enum TcnFamily { TCN_BF16, TCN_BF16X3, TCN_BF16X3_HALF, TCN_F32 };      // tcn_block_bf16_kernel, _bf16x3_kernel, _bf16x3_half_kernel, _f32_kernel
struct TcnBlockPlan {
    TcnFamily family;
    int P;            // phases per tile, P | d
    int tile;         // output times per tile, 256 or 128 (the kernels' NQ = tile / 32): a tile is P phases x tile / P steps
    int form;         // bf16, the kernel's WHOLE: 0 tap-major loop, 1 unrolled loop of a tile that spans its whole phase sequence, 2 class-major
                      // loop; bf16x3 half-tile kernel: 1 = class-major loop (CM)
    bool head;        // the output head runs in this block's epilogue (no tcn_output_kernel)
    bool block0;      // bf16: block 0 is computed in this block's staging (FUSE0; no block-0 kernel)
    int tiles_phase;  // d / P
    int tiles_step;   // ceil(steps per phase / steps per tile)
    long grid;        // B * tiles_phase * tiles_step workgroups
    int xcd_tiles;    // XCD-aware tile order (TcnBlockArgs::xcd_tiles): measured read traffic 1.38 -> 1.20 GB per bf16 launch at P = 4 (1.07 algorithmic)
};

// `head`: the block is the last one of a forward (not of a probe); `behind_block0`: it is block 1 of a net that goes on behind it and whose
// block 0 has dilation 1 - the only place block 0 can move into.
TcnBlockPlan tcn_plan_block(int tuning, int precision, int d, int L, int B, bool head, bool behind_block0) {
    const TcnTuning f{tuning};
    const long nsteps = ((long)L + d - 1) / d;      // steps per phase
    TcnBlockPlan p = {};
    // phases per tile: P | d.  P = 4 with 256-time tiles (bf16: 78 KB of LDS, 2 workgroups per CU) whenever a tile's 64 steps fit the segment
    int P = (d % 4 == 0) ? 4 : (d % 2 == 0 ? 2 : 1);
    p.tile = 256;
    if (precision == MST_PREC_F32) {
        // fp32 kernel: 256-time tiles only (its LDS tile is a 32-channel chunk), up to 16 phases; the separate head
        p.family = TCN_F32;
        while (P < 16 && d % (2 * P) == 0 && 256 / P > nsteps) P *= 2;
    } else if (precision == MST_PREC_BF16X3) {
        // two LDS tiles (hi, lo).  The head is fused: the kernels exist for up to 8 phases, which is every dilation here
        p.head = head;
        const int Q = std::min(P, 2);
        if (f.x3_small_tiles() && 128 / Q <= nsteps) P = Q;       // bit 0: 2 phases wherever a 128-time tile's 64 steps fit the segment
        else if (P == 4 && d % 8 == 0 && nsteps < 64) P = 8;       // large dilations: 8 phases
        if (P == 8) {
            // the input staged in two halves of 64 channels, 128-time tiles (60 KB of LDS, two workgroups per CU)
            p.family = TCN_BF16X3_HALF;
            p.tile = 128;
            p.form = f.x3_half_cm() ? 1 : 0;
        } else {
            // 256-time tiles up to P = 4; bit 0: every block of <= 2 phases on 128-time tiles (2 x 39 KB of LDS, two workgroups = 8 waves per CU)
            p.family = TCN_BF16X3;
            if (f.x3_small_tiles() && P <= 2) p.tile = 128;
        }
    } else {
        p.family = TCN_BF16;
        p.head = head;
        // for larger dilations P = 8; P = 16 (256-time tiles, 16 steps per tile) only for segments with fewer than 16 steps per phase
        while (P < 8 && d % (2 * P) == 0 && 256 / P > nsteps) P *= 2;
        if (P == 8 && d % 16 == 0 && nsteps < 16) P = 16;
        if (P == 8) {
            // P = 8 tiles of 256 times need 94 KB of LDS (one workgroup per CU); 128-time tiles (16 steps per tile, 61 KB) keep two resident:
            // measured 1.98 -> 1.70 ms for the d = 4096 block at L = 131072
            p.tile = 128;
            // 17 ... 32 steps per phase (d = 4096 at L = 131072): 128-time tiles of FOUR phases x 32 steps (184 rows staged per 128 outputs, three
            // workgroups per CU) instead of eight phases x 16 steps (240 rows, two workgroups per CU).  (The same 128-time form for EVERY block
            // measured 1.53-1.58 ms per launch against 1.48-1.53 for round 3's persistent 256-time kernel: it only wins where the eight-phase
            // tiles' halo is the alternative)
            if (nsteps > 16 && nsteps <= 32) P = 4;
        }
        // bit 7, a block whose phase sequences are EXACTLY one 256-time tile - sixteen phases x 16 steps (d = 8192 at L = 131072, the last block),
        // eight x 32 (d = 4096), four x 64 (d = 2048): the unrolled class-major loop without the all-padding (column tile, tap) pairs, an LDS image
        // without the halo steps no live row window reaches (256 / 272 / 280 rows), two workgroups per CU.  With the fused head only the
        // sixteen-phase form fits 256 registers (248; the other two would spill)
        const int Pw = nsteps == 16 ? 16 : (nsteps == 32 ? 8 : (nsteps == 64 ? 4 : 0));
        if (f.bf16_whole() && Pw && d % Pw == 0 && (long)L == nsteps * d && (!head || Pw == 16)) {
            P = Pw;
            p.tile = 256;
            p.form = 1;
        } else if (p.tile == 128) {
            p.form = nsteps == 128 / P ? 1 : 0;      // the one tile of a phase spans its whole sequence: unrolled class-major loop
        } else if (f.bf16_cm() && ((P == 4 && (!head || f.bf16_whole())) || (P == 2 && !head))) {
            // form 2: the two- and four-phase blocks on 256-time class-major tiles, two workgroups per CU (round 6: 1.31 ms per launch against 1.40
            // for round 3's persistent kernel with the same loop); P = 1, sixteen phases and a two-phase last block run the tap-major loop, and
            // so does a four-phase last block (the head of a long segment) without bit 7
            p.form = 2;
            p.block0 = P == 2 && d == 2 && behind_block0 && f.bf16_fuse0();      // bit 5: the d = 2 block computes block 0 in its staging
        }
    }
    p.P = P;
    p.tiles_phase = d / P;
    const int tile_steps = p.tile / P;
    p.tiles_step = (int)((nsteps + tile_steps - 1) / tile_steps);
    p.grid = (long)B * p.tiles_phase * p.tiles_step;
    p.xcd_tiles = p.grid % 8 == 0 ? (int)(p.grid / 8) : 0;
    return p;
}

// every instantiation of the four block kernels, once, keyed by the plan fields that are template arguments
struct TcnBlockKernel {
    TcnFamily family;
    int P, tile, form;
    bool head, block0;      // (bf16 only: the other kernels test TcnBlockArgs::y_out)
    void (*kernel)(TcnBlockArgs);
    const char *name;
};
#define TCN_BF16_KERNEL(P, HEAD, NQ, WHOLE, FUSE0) \
    {TCN_BF16, P, 32 * NQ, WHOLE, HEAD, FUSE0, tcn_block_bf16_kernel<P, HEAD, NQ, WHOLE, FUSE0>, "tcn_block_bf16_kernel"}
#define TCN_X3_KERNEL(P, NQ) {TCN_BF16X3, P, 32 * NQ, 0, false, false, tcn_block_bf16x3_kernel<P, NQ>, "tcn_block_bf16x3_kernel"}
#define TCN_X3_HALF_KERNEL(P, NQ, CM) \
    {TCN_BF16X3_HALF, P, 32 * NQ, CM, false, false, tcn_block_bf16x3_half_kernel<P, NQ, CM>, "tcn_block_bf16x3_half_kernel"}
#define TCN_F32_KERNEL(P) {TCN_F32, P, 256, 0, false, false, tcn_block_f32_kernel<P>, "tcn_block_f32_kernel"}
const TcnBlockKernel TCN_BLOCK_KERNELS[] = {
    //              P   head   NQ WHOLE block 0
    TCN_BF16_KERNEL(1,  false, 8, 0, false),      // tap-major 256-time tiles: odd dilations ...
    TCN_BF16_KERNEL(1,  true,  8, 0, false),
    TCN_BF16_KERNEL(2,  false, 8, 0, false),      // ... and, in form 0 (bits 1-2 = 0), every two- / four-phase block
    TCN_BF16_KERNEL(2,  true,  8, 0, false),      // a two-phase last block is tap-major in either form
    TCN_BF16_KERNEL(4,  false, 8, 0, false),
    TCN_BF16_KERNEL(4,  true,  8, 0, false),      // form 2 without bit 7: the head of a long segment
    TCN_BF16_KERNEL(16, false, 8, 0, false),      // fewer than 16 steps per phase
    TCN_BF16_KERNEL(16, true,  8, 0, false),
    TCN_BF16_KERNEL(2,  false, 8, 2, false),      // form 2: class-major 256-time tiles
    TCN_BF16_KERNEL(2,  false, 8, 2, true),       // bit 5: with block 0 in the staging
    TCN_BF16_KERNEL(4,  false, 8, 2, false),
    TCN_BF16_KERNEL(4,  true,  8, 2, false),      // bit 7: the class-major head of a long segment
    TCN_BF16_KERNEL(4,  false, 8, 1, false),      // bit 7: one 256-time tile is the whole phase sequence (64 / 32 / 16 steps) ...
    TCN_BF16_KERNEL(8,  false, 8, 1, false),
    TCN_BF16_KERNEL(16, false, 8, 1, false),
    TCN_BF16_KERNEL(16, true,  8, 1, false),      // ... with the head at sixteen phases only (registers)
    TCN_BF16_KERNEL(4,  false, 4, 0, false),      // 128-time tiles: four phases at 17 ... 32 steps per phase (WHOLE at exactly 32) ...
    TCN_BF16_KERNEL(4,  true,  4, 0, false),
    TCN_BF16_KERNEL(4,  false, 4, 1, false),
    TCN_BF16_KERNEL(4,  true,  4, 1, false),
    TCN_BF16_KERNEL(8,  false, 4, 0, false),      // ... eight phases below and above that (WHOLE at exactly 16 steps)
    TCN_BF16_KERNEL(8,  true,  4, 0, false),
    TCN_BF16_KERNEL(8,  false, 4, 1, false),
    TCN_BF16_KERNEL(8,  true,  4, 1, false),
    //            P  NQ
    TCN_X3_KERNEL(1, 8),
    TCN_X3_KERNEL(2, 8),
    TCN_X3_KERNEL(4, 8),
    TCN_X3_KERNEL(1, 4),                          // bit 0: 128-time tiles
    TCN_X3_KERNEL(2, 4),
    //                 P  NQ CM
    TCN_X3_HALF_KERNEL(8, 4, false),
    TCN_X3_HALF_KERNEL(8, 4, true),               // bit 6
    TCN_F32_KERNEL(1),
    TCN_F32_KERNEL(2),
    TCN_F32_KERNEL(4),
    TCN_F32_KERNEL(8),
    TCN_F32_KERNEL(16),
};
#undef TCN_BF16_KERNEL
#undef TCN_X3_KERNEL
#undef TCN_X3_HALF_KERNEL
#undef TCN_F32_KERNEL

int tcn_launch_block(const TcnBlockPlan &p, const TcnBlockArgs &a, void *stream) {
    for (const TcnBlockKernel &k : TCN_BLOCK_KERNELS)
        if (k.family == p.family && k.P == p.P && k.tile == p.tile && k.form == p.form && k.block0 == p.block0 &&
            (k.head == p.head || p.family != TCN_BF16)) {
            MST_LAUNCH(k.kernel, dim3((unsigned)p.grid), dim3(256), stream, a);
            MST_CHECK_LAUNCH(k.name);
            return MST_OK;
        }
    return fail(MST_ERR_STATE, "mst_tcn_forward: no block kernel of this tile form (with the fused head the whole-sequence 256-time tile exists at "
                               "sixteen phases only)");
}

int tcn_run_generic(MstTcn *t, const float *x, float *y, float *act_out, int B, int L, int n_run, void *ws, void *stream) {
    const int C = t->d.channels;
    const size_t buf_bytes = align_up((size_t)B * L * C * sizeof(float), 256);
    float *buf[2] = {(float *)ws, (float *)((unsigned char *)ws + buf_bytes)};
    const float *cur = x;
    int rc, pp = 0;
    for (int n = 0; n < n_run; ++n) {
        float *dst = (act_out && n == n_run - 1) ? act_out : buf[pp];
        const int cin = n == 0 ? t->d.ninputs : C;
        if ((rc = tcn_launch_generic(t->gconv[n], cur, dst, B, L, 1, t->film + (size_t)n * t->film_rows * 2 * C, t->film_rows,
                                     t->blk[n].res, C / cin, stream)))
            return rc;
        cur = dst;
        pp ^= 1;
    }
    if (act_out) return MST_OK;
    return tcn_launch_generic(t->gconv[t->d.nblocks], cur, y, B, L, 2, nullptr, 1, nullptr, 1, stream);
}

// The launch table of B items: the whole batch, or one chunk of it (tcn_run) - then x and y are the chunk's, film_row0 its first item's FiLM
// row where the table has a row per item (0 otherwise), buf0 / buf1 the chunk chain's two activations and ev the chunk's nblocks + 2 events.
int tcn_run_items(MstTcn *t, const float *x, float *y, float *act_out, int B, int L, int precision, int n_run, unsigned char *buf0,
                  unsigned char *buf1, size_t film_row0, hipEvent_t *ev, void *stream) {
    const int nblocks = t->d.nblocks;
    TcnBlockPlan plan[MST_MAX_BLOCKS] = {};
    for (int n = 1; n < n_run; ++n) {
        // (block 0 moves into block 1's launch only for a net that goes on behind block 1; its own probe, n_run == 1, always runs the separate kernel)
        plan[n] = tcn_plan_block(t->tuning, precision, t->d.dilations[n], L, B, !act_out && n == nblocks - 1,
                                 n == 1 && nblocks > 2 && t->d.dilations[0] == 1);
        if (plan[n].grid > 0x7fffffffL) return fail(MST_ERR_ARG, "mst_tcn_forward: grid too large");
    }
    // the last three blocks as one launch (mst_tcn_set_fusion bit 0, tcn_tail_bf16_kernel): a full bf16 forward whose last three plans are exactly
    // the whole-sequence 256-time forms of four, eight and sixteen phases at dilations d, 2d, 4d (L = 64 d) - their tiles are then the same
    // samples.  Anything else (a step over or under in L, tuning without bit 7, a probe, another precision) runs the launches planned above.
    bool tail = false;
    if (precision == MST_PREC_BF16 && !act_out && n_run == nblocks && nblocks >= 4 && (t->fusion & 1)) {
        const int n0 = nblocks - 3;
        const int d0 = t->d.dilations[n0];
        tail = t->d.dilations[n0 + 1] == 2 * d0 && t->d.dilations[n0 + 2] == 4 * d0;
        for (int k = 0; k < 3; ++k) {
            const TcnBlockPlan &p = plan[n0 + k];
            tail = tail && p.family == TCN_BF16 && p.form == 1 && p.tile == 256 && p.P == (4 << k) && p.tiles_step == 1 && !p.block0 &&
                   p.head == (k == 2) && p.grid == plan[n0].grid;
        }
    }
    t->last_fused_tail = tail ? 1 : 0;
    unsigned char *buf[2] = {buf0, buf1};
    const int Lp = L;
    const float *film = t->film + film_row0 * 256;      // block n's rows: film + n * film_rows * 256
    if (ev) MST_HIP_TRY(hipEventRecord(ev[0], (hipStream_t)stream));

    const bool fuse0 = plan[1].block0;
    t->last_fused0 = fuse0 ? 1 : 0;
    if (!fuse0) {
        TcnBlock0Args a;
        a.x = x;
        a.y = buf[0];
        a.w = t->blk[0].w_f32;
        a.shift = t->blk[0].shift;
        a.film = film;
        a.res = t->blk[0].res;
        a.film_rows = t->film_rows;
        a.B = B;
        a.L = L;
        a.Lp = Lp;
        a.wpk16 = t->blk[0].w_bf16;
        if (precision == MST_PREC_BF16)
            MST_LAUNCH(tcn_block0_mfma_kernel, dim3(B * ((L + 255) / 256)), dim3(256), stream, a);
        else
            MST_LAUNCH((tcn_block0_kernel<float>), dim3(B * ((L + 511) / 512)), dim3(256), stream, a);      // 8 tiles of 64 steps per workgroup
        MST_CHECK_LAUNCH("tcn_block0_kernel");
    }
    if (ev) MST_HIP_TRY(hipEventRecord(ev[1], (hipStream_t)stream));
    int cur = 0;
    for (int n = 1; n < n_run; ++n) {
        const TcnBlockPlan &p = plan[n];
        TcnBlockArgs a;
        a.x = buf[cur];
        a.y = buf[cur ^ 1];
        a.wpk = precision == MST_PREC_BF16 ? t->blk[n].w_bf16 : (precision == MST_PREC_BF16X3 ? t->blk[n].w_x3 : (void *)t->blk[n].w_f32);
        a.shift = t->blk[n].shift;
        a.film = film + (size_t)n * t->film_rows * 256;
        a.res = t->blk[n].res;
        a.film_rows = t->film_rows;
        a.B = B;
        a.L = L;
        a.Lp = Lp;
        a.d = t->d.dilations[n];
        a.tiles_phase = p.tiles_phase;
        a.tiles_step = p.tiles_step;
        a.out_w = t->out_w;
        a.out_b = t->out_b;
        a.y_out = p.head ? y : nullptr;
        a.nout = t->d.noutputs;
        a.xcd_tiles = p.xcd_tiles;
        a.zeros = t->zero_row;
        if (p.block0) {
            a.x0 = x;
            a.w0pk = t->blk[0].w_bf16;
            a.shift0 = t->blk[0].shift;
            a.film0 = film;
            a.res0 = t->blk[0].res;
        }
        if (tail && n == nblocks - 3) {
            // one launch of the four-phase block's grid and tile order; the head's arguments are already in `a`
            TcnTailArgs ta;
            ta.a = a;
            ta.a.y = nullptr;
            ta.a.y_out = y;
            for (int k = 0; k < 3; ++k) {
                ta.wpk[k] = t->blk[n + k].w_bf16;
                ta.shift[k] = t->blk[n + k].shift;
                ta.film[k] = film + (size_t)(n + k) * t->film_rows * 256;
                ta.res[k] = t->blk[n + k].res;
            }
            MST_LAUNCH(tcn_tail_bf16_kernel, dim3((unsigned)p.grid), dim3(256), stream, ta);
            MST_CHECK_LAUNCH("tcn_tail_bf16_kernel");
            if (ev)          // the three blocks' events coincide: mst_tcn_timing_end shares the launch's time among them
                for (int k = 0; k < 3; ++k) MST_HIP_TRY(hipEventRecord(ev[n + k + 1], (hipStream_t)stream));
            break;
        }
        int rc;
        if ((rc = tcn_launch_block(p, a, stream))) return rc;
        if (ev) MST_HIP_TRY(hipEventRecord(ev[n + 1], (hipStream_t)stream));
        cur ^= 1;
    }
    if (act_out) {
        const size_t total = (size_t)B * L * 128;
        const unsigned grid = (unsigned)((total + 255) / 256);
        if (precision == MST_PREC_BF16)
            MST_LAUNCH((tcn_unpack_kernel<__bf16>), dim3(grid), dim3(256), stream, (const void *)buf[cur], act_out, B, L, Lp);
        else
            MST_LAUNCH((tcn_unpack_kernel<float>), dim3(grid), dim3(256), stream, (const void *)buf[cur], act_out, B, L, Lp);
        MST_CHECK_LAUNCH("tcn_unpack_kernel");
        return MST_OK;
    }
    if (!plan[nblocks - 1].head) {      // (a fused head: the output conv ran inside the last block kernel)
        TcnOutArgs o;
        o.x = buf[cur];
        o.y = y;
        o.w = t->out_w;
        o.bias = t->out_b;
        o.nout = t->d.noutputs;
        o.B = B;
        o.L = L;
        o.Lp = Lp;
        const int grid = B * ((L + 63) / 64);
        if (precision == MST_PREC_BF16)
            MST_LAUNCH((tcn_output_kernel<__bf16>), dim3(grid), dim3(256), stream, o);
        else
            MST_LAUNCH((tcn_output_kernel<float>), dim3(grid), dim3(256), stream, o);
        MST_CHECK_LAUNCH("tcn_output_kernel");
    }
    if (ev) MST_HIP_TRY(hipEventRecord(ev[nblocks + 1], (hipStream_t)stream));
    return MST_OK;
}

// ---- the batch in chunks that stay in the Infinity Cache (mst_tcn_set_chunk; EXPERIMENTS.md E.9) ----
// Items are independent through the whole net.  As one launch per block over a large batch, a line block k writes is followed by gigabytes of
// other traffic before block k + 1 reads it: every activation goes to HBM and comes back.  As chunks of c items through ALL blocks, every
// chunk on the same two ping-pong buffers, block k + 1 finds block k's output on die.  One chain of chunks loses more at its launch seams
// (c rounds of the chip's workgroup slots per launch instead of B) than the traffic saves; TWO chains on two streams fill each other's
// seams.  Measured at 32 x 131072 against the full batch, six pairs each: one chain c = 1 / 2 / 4 / 8 / 16 +15.6 / +5.5 / +0.3 / +0.9 /
// +0.5 % slower; two chains c = 1 / 2 / 3 / 4: -1.3 / -2.5 / -0.3 / 0.0 %.
constexpr size_t TCN_CACHE_BYTES = (size_t)256 << 20;      // MI355X Infinity Cache
constexpr int TCN_CHUNK_CHAINS = 2;

// The automatic rule, in bytes, not shapes: a batch whose ONE activation no longer fits the cache (no line can survive from block k to
// block k + 1) runs in chunks of the largest c whose resident set - two chains x (input + output) x c items - fits it: c = 2 at L = 131072,
// exactly 256 MiB, the winner of the gate.  c < 1 (an item pair per chain alone overflows the cache: measured break-even) or a batch that
// fits: the whole batch, as before.
int tcn_chunk_items(int B, int L) {
    const size_t item = (size_t)L * 128 * 2;
    if ((size_t)B * item <= TCN_CACHE_BYTES) return B;
    const size_t c = TCN_CACHE_BYTES / (2 * TCN_CHUNK_CHAINS * item);
    return c >= 1 ? (int)c : B;
}

// the handle's side stream (from the pool of retired ones, or new) and its two events
int tcn_side_stream(MstTcn *t) {
    const int dev = mst_current_device();
    if (t->side_dev >= 0 && t->side_dev != dev) return fail(MST_ERR_STATE, "mst_tcn_forward: the handle's side stream lives on another device");
    if (t->side_dev >= 0) return MST_OK;
    if (!t->side_fork) MST_HIP_TRY(hipEventCreateWithFlags(&t->side_fork, hipEventDisableTiming));
    if (!t->side_join) MST_HIP_TRY(hipEventCreateWithFlags(&t->side_join, hipEventDisableTiming));
    {
        std::lock_guard<std::mutex> lock(tcn_side_mu);
        for (size_t i = 0; i < tcn_side_free.size(); ++i)
            if (tcn_side_free[i].first == dev) {
                t->side = tcn_side_free[i].second;
                t->side_dev = dev;
                tcn_side_free.erase(tcn_side_free.begin() + i);
                return MST_OK;
            }
    }
    MST_HIP_TRY(hipStreamCreateWithPriority(&t->side, hipStreamNonBlocking, 0));
    t->side_dev = dev;
    return MST_OK;
}

int tcn_run(MstTcn *t, const float *x, float *y, float *act_out, int B, int L, int precision, int n_run, void *ws,
            size_t ws_bytes, void *stream) {
    if (!t || !x || B < 1 || L < 1) return fail(MST_ERR_ARG, "mst_tcn_forward: bad argument");
    if (precision != MST_PREC_F32 && precision != MST_PREC_BF16 && precision != MST_PREC_BF16X3)
        return fail(MST_ERR_ARG, "mst_tcn_forward: bad precision");
    for (auto &b : t->blk)
        if (!b.loaded) return fail(MST_ERR_STATE, "mst_tcn_forward: block weights not loaded");
    if (!t->out_loaded) return fail(MST_ERR_STATE, "mst_tcn_forward: output conv not loaded");
    if (t->film_rows == 0) return fail(MST_ERR_STATE, "mst_tcn_forward: mst_tcn_set_cond has not been called");
    if (t->film_rows != 1 && t->film_rows != B)
        return fail(MST_ERR_ARG, "mst_tcn_forward: condition rows must be 1 or equal the batch size");
    const size_t need = mst_tcn_workspace_bytes(t, B, L, precision);
    if (!ws || ws_bytes < need) return fail(MST_ERR_WORKSPACE, "mst_tcn_forward: workspace too small");
    t->last_chunks = 1;
    if (t->generic) return tcn_run_generic(t, x, y, act_out, B, L, n_run, ws, stream);
    const int nblocks = t->d.nblocks;
    const int per = nblocks + 2;
    // only a full bf16 forward is chunked; the other precisions and the probes keep the whole batch
    int c = B;
    if (precision == MST_PREC_BF16 && !act_out && n_run == nblocks && nblocks >= 2) c = std::min(B, t->chunk > 0 ? t->chunk : tcn_chunk_items(B, L));
    const int chunks = (B + c - 1) / c;
    const size_t buf_bytes = align_up((size_t)c * L * 128 * tcn_elem(precision), 256);
    // the second chain needs two buffers of its own inside the same workspace: where they do not fit, one chain on the caller's stream
    const int chains = chunks >= 2 && 2 * TCN_CHUNK_CHAINS * buf_bytes <= need ? TCN_CHUNK_CHAINS : 1;
    int rc;
    if (chains > 1 && (rc = tcn_side_stream(t))) return rc;
    hipEvent_t *ev = nullptr;
    if (!act_out && (int)t->ev_fwd.size() < t->ev_max) {
        while (t->ev.size() < t->ev_next + (size_t)chunks * per) {
            hipEvent_t e = nullptr;
            MST_HIP_TRY(hipEventCreate(&e));
            t->ev.push_back(e);
        }
        ev = t->ev.data() + t->ev_next;
        t->ev_fwd.push_back({t->ev_next, chunks, chains, false});
        t->ev_next += (size_t)chunks * per;
    }
    if (chains > 1) {
        MST_HIP_TRY(hipEventRecord(t->side_fork, (hipStream_t)stream));
        MST_HIP_TRY(hipStreamWaitEvent(t->side, t->side_fork, 0));
    }
    rc = MST_OK;
    for (int k = 0; k < chunks && rc == MST_OK; ++k) {
        const int b0 = k * c, nb = std::min(c, B - b0);
        const int chain = k % chains;
        unsigned char *base = (unsigned char *)ws + (size_t)chain * 2 * buf_bytes;
        rc = tcn_run_items(t, x + (size_t)b0 * t->d.ninputs * L, y ? y + (size_t)b0 * t->d.noutputs * L : nullptr, act_out, nb, L, precision, n_run,
                           base, base + buf_bytes, t->film_rows > 1 ? (size_t)b0 : 0, ev ? ev + (size_t)k * per : nullptr,
                           chain ? (void *)t->side : stream);
    }
    if (chains > 1) {
        // joined even after a failed launch: nothing stays pending on the side stream behind the caller's back
        hipError_t e = hipEventRecord(t->side_join, t->side);
        if (e == hipSuccess) e = hipStreamWaitEvent((hipStream_t)stream, t->side_join, 0);
        if (e != hipSuccess && rc == MST_OK) rc = fail(MST_ERR_HIP, std::string("mst_tcn_forward: joining the side stream: ") + hipGetErrorString(e));
    }
    if (ev) t->ev_fwd.back().tail = t->last_fused_tail != 0;
    t->last_chunks = chunks;
    return rc;
}

}  // namespace

extern "C" int mst_tcn_set_tuning(MstTcn *t, int flags) {
    if (!t) return fail(MST_ERR_ARG, "mst_tcn_set_tuning: null handle");
    const int form = (flags >> 1) & 3;
    if (flags < 0 || flags > 255 || (form != 0 && form != 2) || ((flags >> 3) & 1) || (form == 2 && !((flags >> 4) & 1)))
        return fail(MST_ERR_ARG, "mst_tcn_set_tuning: unknown flag bits (bits 1-2 = 0 or 2, form 2 with bit 4, no bit 3: the kernels the others "
                                 "selected left the library)");
    t->tuning = flags;
    return MST_OK;
}

extern "C" int mst_tcn_get_tuning(const MstTcn *t, int *flags, int *last_forward_fused_block0) {
    if (!t) return fail(MST_ERR_ARG, "mst_tcn_get_tuning: null handle");
    if (flags) *flags = t->tuning;
    if (last_forward_fused_block0) *last_forward_fused_block0 = t->last_fused0;
    return MST_OK;
}

extern "C" int mst_tcn_set_fusion(MstTcn *t, int flags) {
    if (!t) return fail(MST_ERR_ARG, "mst_tcn_set_fusion: null handle");
    if (flags < 0 || flags > 1) return fail(MST_ERR_ARG, "mst_tcn_set_fusion: unknown flag bits (bit 0: the last three blocks as one launch)");
    t->fusion = flags;
    return MST_OK;
}

extern "C" int mst_tcn_get_fusion(const MstTcn *t, int *flags, int *last_forward_fused_tail) {
    if (!t) return fail(MST_ERR_ARG, "mst_tcn_get_fusion: null handle");
    if (flags) *flags = t->fusion;
    if (last_forward_fused_tail) *last_forward_fused_tail = t->last_fused_tail;
    return MST_OK;
}

extern "C" int mst_tcn_set_chunk(MstTcn *t, int items) {
    if (!t) return fail(MST_ERR_ARG, "mst_tcn_set_chunk: null handle");
    if (items < 0) return fail(MST_ERR_ARG, "mst_tcn_set_chunk: items < 0 (0: automatic, n: n items per chunk, MST_TCN_CHUNK_WHOLE: never)");
    t->chunk = items;
    return MST_OK;
}

extern "C" int mst_tcn_get_chunk(const MstTcn *t, int *items, int *ran_chunks) {
    if (!t) return fail(MST_ERR_ARG, "mst_tcn_get_chunk: null handle");
    if (items) *items = t->chunk;
    if (ran_chunks) *ran_chunks = t->last_chunks;
    return MST_OK;
}

extern "C" int mst_tcn_context(const MstTcn *t, long *left, long *right) {
    if (!t) return fail(MST_ERR_ARG, "mst_tcn_context: null handle");
    long l = 0, r = 0;
    for (int n = 0; n < t->d.nblocks; ++n) {      // the blocks' zero paddings (mst_tcn_create), summed
        const long span = (long)(t->d.kernel_size - 1) * t->d.dilations[n];
        const long pad_l = t->d.causal ? span : span / 2;
        l += pad_l;
        r += span - pad_l;
    }
    if (left) *left = l;
    if (right) *right = r;
    return MST_OK;
}

extern "C" int mst_tcn_timing_begin(MstTcn *t, int max_forwards) {
    if (!t || max_forwards < 1) return fail(MST_ERR_ARG, "mst_tcn_timing_begin: bad argument");
    for (auto e : t->ev) (void)hipEventDestroy(e);
    t->ev.assign((size_t)max_forwards * (t->d.nblocks + 2), nullptr);      // (a chunked forward takes more: tcn_run creates them as it goes)
    for (auto &e : t->ev) MST_HIP_TRY(hipEventCreate(&e));
    t->ev_fwd.clear();
    t->ev_fwd.reserve((size_t)max_forwards);
    t->ev_max = max_forwards;
    t->ev_next = 0;
    return MST_OK;
}

extern "C" int mst_tcn_timing_end(MstTcn *t, float *ms_out, int *n_forwards) {
    if (!t || !ms_out || !n_forwards) return fail(MST_ERR_ARG, "mst_tcn_timing_end: bad argument");
    const int per = t->d.nblocks + 2;
    for (int k = 0; k <= t->d.nblocks; ++k) ms_out[k] = 0.0f;
    const int used = (int)t->ev_fwd.size();
    for (const MstTcn::TimedForward &f : t->ev_fwd)
        for (int c = 0; c < f.chunks; ++c) {
            // a chunked forward: a block's launches summed over the chunks; launches of two chains overlap, each counted in full on its own
            // stream, so the sum is divided by the number of chains - the figures still add up to about the forward's time
            const hipEvent_t *ev = t->ev.data() + f.first + (size_t)c * per;
            MST_HIP_TRY(hipEventSynchronize(ev[per - 1]));
            float ms[MST_MAX_BLOCKS + 1] = {};
            for (int k = 0; k <= t->d.nblocks; ++k) MST_HIP_TRY(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]));
            if (f.tail) {      // the last three blocks were one launch: its time in equal shares
                const int n0 = t->d.nblocks - 3;
                ms[n0] = ms[n0 + 1] = ms[n0 + 2] = (ms[n0] + ms[n0 + 1] + ms[n0 + 2]) / 3.0f;
            }
            for (int k = 0; k <= t->d.nblocks; ++k) ms_out[k] += ms[k] / (float)f.chains;
        }
    if (used > 0)
        for (int k = 0; k <= t->d.nblocks; ++k) ms_out[k] /= (float)used;
    *n_forwards = used;
    for (auto e : t->ev) (void)hipEventDestroy(e);
    t->ev.clear();
    t->ev_fwd.clear();
    t->ev_max = 0;
    t->ev_next = 0;
    return MST_OK;
}

extern "C" int mst_calib_mainloop(int launches, float *ms_per_launch, float *sclk_mhz, void *stream) {
    if (launches < 2 || !ms_per_launch || !sclk_mhz) return fail(MST_ERR_ARG, "mst_calib_mainloop: bad argument");
    constexpr int WG = 512, REP = 32;                      // 512 x 32 tiles of 256 times = 32 x 131072 output steps
    const size_t wbytes = (size_t)120 * 256 * 16;          // 60 k-steps x 2 row tiles x 4 waves x 64 lanes x 16 B
    void *w = nullptr;
    float *out = nullptr;
    long long *clk = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = MST_OK;
    auto cleanup = [&]() {
        if (w) (void)hipFree(w);
        if (out) (void)hipFree(out);
        if (clk) (void)hipFree(clk);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    };
#define MST_CALIB_TRY(x)                                                        \
    if ((x) != hipSuccess) {                                                    \
        rc = fail(MST_ERR_HIP, "mst_calib_mainloop: HIP call failed");          \
        cleanup();                                                              \
        return rc;                                                              \
    }
    MST_CALIB_TRY(hipMalloc(&w, wbytes));
    MST_CALIB_TRY(hipMalloc((void **)&out, (size_t)WG * 256 * sizeof(float)));
    MST_CALIB_TRY(hipMalloc((void **)&clk, 2 * sizeof(long long)));
    MST_CALIB_TRY(hipEventCreate(&e0));
    MST_CALIB_TRY(hipEventCreate(&e1));
    MST_LAUNCH(tcn_calib_fill_kernel, dim3((unsigned)(wbytes / 4 + 255) / 256), dim3(256), stream, (unsigned *)w, (int)(wbytes / 4));
    const int warm = launches / 2, timed = launches - warm;
    for (int i = 0; i < warm; ++i) MST_LAUNCH(tcn_calib_mainloop_kernel, dim3(WG), dim3(256), stream, (const void *)w, out, clk, REP);
    MST_CALIB_TRY(hipEventRecord(e0, (hipStream_t)stream));
    for (int i = 0; i < timed; ++i) MST_LAUNCH(tcn_calib_mainloop_kernel, dim3(WG), dim3(256), stream, (const void *)w, out, clk, REP);
    MST_CALIB_TRY(hipEventRecord(e1, (hipStream_t)stream));
    MST_CALIB_TRY(hipEventSynchronize(e1));
    float ms = 0.0f;
    MST_CALIB_TRY(hipEventElapsedTime(&ms, e0, e1));
    long long c[2] = {0, 0};
    MST_CALIB_TRY(hipMemcpy(c, clk, sizeof(c), hipMemcpyDeviceToHost));
#undef MST_CALIB_TRY
    *ms_per_launch = ms / (float)timed;
    *sclk_mhz = c[1] > 0 ? (float)((double)c[0] / ((double)c[1] / 100.0)) : 0.0f;      // shader clocks per microsecond
    cleanup();
    return MST_OK;
}

extern "C" size_t mst_tcn_workspace_bytes(const MstTcn *t, int B, int L, int precision) {
    if (B < 1 || L < 1) return 0;
    if (t && t->generic) return 2 * align_up((size_t)B * L * t->d.channels * sizeof(float), 256);
    return 2 * align_up((size_t)B * L * 128 * tcn_elem(precision), 256);
}

extern "C" int mst_tcn_forward(MstTcn *t, const float *x, float *y, int B, int L, int precision, void *ws,
                               size_t ws_bytes, void *stream) {
    if (!y) return fail(MST_ERR_ARG, "mst_tcn_forward: null output");
    return tcn_run(t, x, y, nullptr, B, L, precision, t ? t->d.nblocks : 0, ws, ws_bytes, stream);
}

extern "C" int mst_tcn_forward_blocks(MstTcn *t, const float *x, float *act, int B, int L, int precision, int n_run,
                                      void *ws, size_t ws_bytes, void *stream) {
    if (!t || !act || n_run < 1 || n_run > t->d.nblocks) return fail(MST_ERR_ARG, "mst_tcn_forward_blocks: bad argument");
    return tcn_run(t, x, nullptr, act, B, L, precision, n_run, ws, ws_bytes, stream);
}

extern "C" int mst_film_forward(const float *w, const float *b, const float *cond, int rows, int cond_dim, int C, const float *x,
                                float *y, int B, long L, float *table, void *stream) {
    if (!w || !b || !cond || !x || !y || !table || rows < 1 || cond_dim < 1 || C < 1 || B < 1 || L < 1)
        return fail(MST_ERR_ARG, "mst_film_forward: bad argument");
    if (rows != 1 && rows != B) return fail(MST_ERR_ARG, "mst_film_forward: condition rows must be 1 or equal the batch size");
    FilmArgs a;
    a.fw = w;
    a.fb = b;
    a.cond = cond;
    a.film = table;
    a.nblocks = 1;
    a.two_c = 2 * C;
    a.D = cond_dim;
    a.rows = rows;
    a.block_stride = 0;
    MST_LAUNCH(tcn_film_kernel, dim3((2 * C + 3) / 4), dim3(256), stream, a);
    MST_CHECK_LAUNCH("tcn_film_kernel");
    const long total = (long)B * C * L;
    MST_LAUNCH(film_apply_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), stream, x, y, (const float *)table, rows, C, L, total);
    MST_CHECK_LAUNCH("film_apply_kernel");
    return MST_OK;
}

