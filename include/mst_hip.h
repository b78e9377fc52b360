/* mst_hip.h - C ABI of libmst_hip.so: the MI355X (gfx950) hot path of the music-mixing-style-transfer
 * inference pipeline (FXencoder -> mean FX embedding -> FiLM-conditioned TCN "MixFXcloner", plus the
 * FX-manipulator processors).
 *
 * The reference (jhtonyKoo/music_mixing_style_transfer) is pure Python and has no native boundary; its
 * boundary for this path is the torch module API `from networks import FXencoder, TCNModel`
 * (inference/style_transfer.py:22,47-57,149,161).  The entry points below are what sits directly under
 * those modules' forward() in this build - each one names the reference code it replaces.  A binding
 * only needs raw pointers, sizes and a hipStream_t: there are no torch types in any signature.
 *
 * Conventions
 *   - every function returns MST_OK (0) or a negative MstStatus; nothing throws or exits;
 *     mst_last_error() returns a thread-local human readable message for the last failure.
 *   - "host" pointers are CPU memory in the REFERENCE's own tensor layouts (state_dict layouts);
 *     "dev" pointers are device memory owned by the caller.  The library owns only the opaque handle,
 *     its packed/folded weights and the FiLM factor table; forward() allocates nothing - the caller
 *     passes a workspace of mst_*_workspace_bytes().
 *   - all kernels are enqueued on the caller's stream and return immediately.
 *   - a handle belongs to one device and is not thread-safe (one stream at a time).
 */
#ifndef MST_HIP_H
#define MST_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    MST_OK = 0,
    MST_ERR_ARG = -1,          /* bad argument (null pointer, non-positive size, ...) */
    MST_ERR_UNSUPPORTED = -2,  /* configuration outside what the gfx950 kernels implement */
    MST_ERR_HIP = -3,          /* HIP runtime error (see mst_last_error) */
    MST_ERR_STATE = -4,        /* weights / condition not loaded before forward */
    MST_ERR_WORKSPACE = -5     /* workspace pointer null or too small */
} MstStatus;

/* arithmetic mode of the dense convolutions (TCN blocks 1..n-1, all FXencoder convs) */
typedef enum {
    MST_PREC_F32 = 0,   /* v_mfma_f32_32x32x2_f32, fp32 activations in HBM: the parity mode */
    MST_PREC_BF16 = 1,  /* bf16 operands / fp32 accumulate (TCN blocks: v_mfma_f32_16x16x32_bf16, FXencoder: v_mfma_f32_32x32x16_bf16), bf16 activations in HBM */
    MST_PREC_BF16X3 = 2 /* every fp32 operand split x = hi + lo into two bf16 values, three bf16 MFMAs per product
                         * (hi*hi + hi*lo + lo*hi): fp32-class accuracy at a third of the bf16 rate.  TCN: fp32 activations in HBM,
                         * <= 1e-4 on the waveform (measured 4e-6).  FXencoder: the channel-minor bf16 pipeline in the same split
                         * arithmetic (two bf16 planes per activation), <= 1e-4 * max|embedding| (measured 6e-6) - NOT the exact
                         * MST_PREC_F32 kernels: use MST_PREC_F32 where bit-level parity with the fp32 reference order matters. */
} MstPrecision;

#define MST_MAX_BLOCKS 32

int mst_version(void);          /* 111: mst_ntxent_forward / mst_ntxent_backward / mst_rms_loss_forward / mst_rms_loss_backward and their workspace queries; 110: mst_tcn_set_chunk / mst_tcn_get_chunk; 109: mst_mss_backward / mst_mss_backward_workspace_bytes; 108: mst_batch_gather_pcm / mst_batch_finish; 107: mst_tcn_context; 106: mst_mixfeat_spectral; 105: panner, Haas and both reverbs per item, mst_fx_panner_items / mst_fx_haas_items / mst_fx_convolve_items (+ its prepare, table and workspace queries) / mst_fx_algorithmic_reverb_items; 104: mst_tcn_set_fusion / mst_tcn_get_fusion; 103: per-item FX parameters, mst_fx_biquad_cascade_items / mst_fx_compressor_items / mst_fx_midside_imager_items / mst_fx_gain_items; 102: the diagnostic plan queries mst_fx_biquad_plan / mst_fx_compressor_plan; 101: the mst_resample_* entry points */
const char *mst_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * MixFXcloner: TCNModel (networks/architectures.py:76-174) / TCNBlock (:177-234) / FiLM
 * (networks/network_utils.py:156-182).
 * ---------------------------------------------------------------------------------------------- */
typedef struct MstTcn MstTcn;

typedef struct {
    int nblocks;                   /* TCNModel(nblocks)                      default cfg: 14  */
    int ninputs;                   /* input channels of block 0              default cfg: 2   */
    int noutputs;                  /* channels of the 1x1 output conv        default cfg: 2   */
    int channels;                  /* channel_width                          default cfg: 128 */
    int kernel_size;               /*                                        default cfg: 15  */
    int cond_dim;                  /* FiLM condition length                  default cfg: 2048 */
    int dilations[MST_MAX_BLOCKS]; /* dilation_growth ** (n % stack_size), architectures.py:122 */
    int causal;                    /* TCNBlock(causal=True): zero padding (k-1)*d on the left only - the reference pads both
                                    * sides by (k-1)*d and drops the last (k-1)*d outputs (architectures.py:199,230-231) */
} MstTcnDesc;

/* replaces TCNModel.__init__ (architectures.py:93-133): conditional blocks of dense convolutions (a grouped conv1 is handed
 * over as its block-diagonal dense weight).  The configs.yaml shape (channel_width 128, kernel_size 15, ninputs 2,
 * noutputs <= 2, non-causal - what inference/style_transfer.py:48-57 constructs) runs on the specialised kernels in every
 * precision; any other channel width / kernel size / input width / dilation / a causal net runs on a generic exact-fp32
 * implicit-GEMM path (the precision argument is then ignored).  A single TCNBlock is a net of one block run through
 * mst_tcn_forward_blocks. */
int mst_tcn_create(const MstTcnDesc *desc, MstTcn **out);
int mst_tcn_destroy(MstTcn *tcn);

/* replaces load_state_dict for blocks.{n}.* (style_transfer.py:94-108).  Host fp32, reference layouts:
 *   conv_w  [channels, cin, k]      blocks.n.conv1.weight (bias=False, architectures.py:201-207)
 *   bn_*    [channels]              blocks.n.bn.{weight,bias,running_mean,running_var}; eval-mode BN is
 *                                   folded into the conv weight + a per-channel shift
 *   film_w  [2*channels, cond_dim]  blocks.n.film.film_fc.weight ; film_b [2*channels]
 *   res_w   [channels]              blocks.n.res.weight ([channels,1,1]: grouped 1x1, groups=cin,
 *                                   architectures.py:216-220; block 0: out-channel o reads in-channel
 *                                   o / (channels/ninputs)) */
int mst_tcn_load_block(MstTcn *tcn, int n, const float *conv_w, const float *bn_weight, const float *bn_bias,
                       const float *bn_mean, const float *bn_var, float bn_eps, const float *film_w,
                       const float *film_b, const float *res_w, void *stream);
/* output.weight [noutputs, channels(,1)] , output.bias [noutputs]  (architectures.py:133) */
int mst_tcn_load_output(MstTcn *tcn, const float *w, const float *b, void *stream);

/* replaces FiLM.forward's film_fc(condition) for all blocks at once (network_utils.py:180-181): computes
 * the (r, b) factor table.  cond_dev: device fp32; n_rows = 1 (one embedding broadcast over the batch,
 * what style_transfer.py:161 passes) or B (one row per batch item).  block_stride (in floats) = 0 when
 * every block sees the same condition, else block n reads cond_dev + n*block_stride (the reference's
 * list-of-conditions branch, architectures.py:139-140). */
int mst_tcn_set_cond(MstTcn *tcn, const float *cond_dev, int n_rows, long block_stride, void *stream);

size_t mst_tcn_workspace_bytes(const MstTcn *tcn, int B, int L, int precision);

/* replaces TCNModel.forward (architectures.py:135-147): x_dev fp32 [B, ninputs, L] (NCL, contiguous) ->
 * y_dev fp32 [B, noutputs, L], clamped to [-1, 1].  Zero padding ((k-1)*d)//2 both sides per block. */
int mst_tcn_forward(MstTcn *tcn, const float *x_dev, float *y_dev, int B, int L, int precision,
                    void *workspace, size_t workspace_bytes, void *stream);
/* parity probe: run only the first n_run blocks and return that block's output activations as fp32
 * [B, channels, L] (NCL, the reference's layout) - the per-block hook the parity tests compare. */
int mst_tcn_forward_blocks(MstTcn *tcn, const float *x_dev, float *act_dev, int B, int L, int precision, int n_run,
                           void *workspace, size_t workspace_bytes, void *stream);

/* ---- Kernel-form switches at a glance ------------------------------------------------------------------------------------------------------
 * None of them changes WHAT is computed; "=" bit-identical to the default, "~" equal up to fp32 summation order.  The library keeps no
 * process-wide switch: every one lives in a handle or in the arguments of one call.  Defaults are the measured-fastest forms.
 *
 *   where                          bit / field            default  selects                                                  result  why it is still here
 *   mst_tcn_set_tuning (handle)    bit 0                  1        bf16x3: 128-time tiles of <= 2 phases, 2 workgroups / CU   ~       256-time form needed where < 64 steps per phase
 *                                  bits 1-2               2        bf16: 2 = the class-major family - two- / four-phase       ~       0 = tcn_block_bf16_kernel's tap-major loop for every
 *                                                                  blocks on 256-time class-major tiles, 2 workgroups / CU;           bf16 block: the reference form of the tests
 *                                                                  1 and 3 rejected (MST_ERR_ARG)
 *                                  bit 3                  0        rejected (MST_ERR_ARG)
 *                                  bit 4                  1        required with form 2 (form 2 without it: MST_ERR_ARG); ignored with form 0
 *                                  bit 5                  1        bf16, form 2: block 0 inside the d = 2 block's launch      =       separate block-0 kernel = block 0's own probe, other precisions, nets it cannot apply to
 *                                  bit 6                  1        bf16x3: class-major loop in the eight-phase half kernel    ~       other side of a GPU test
 *                                  bit 7                  1        bf16, form 2: whole-sequence 256-time tiles and the        =/~     off = those blocks on the general tilings and the
 *                                                                  class-major fused head of a four-phase last block                  tap-major head: the other side of the tests
 *   mst_enc_set_tuning (handle)    rows_min_tiles         512      bf16: rows-resident conv kernel from this many tiles on    =       small layers run the im2col kernel
 *   mst_enc_set_schedule (handle)  bit 0                  1        weight-major workgroup order of weight-heavy layers        =
 *                                  bit 1                  0        rejected (MST_ERR_ARG)
 *                                  bit 2                  0        fp32: 64-bit gather addresses                              =       the path > 4 GiB activations take anyway (test hook)
 *                                  bit 3                  0        stereo block as two direct launches                        =       reference form of the fused kernel's bit-identity test
 *                                  bit 4                  0        blocks 1 / 2 as two launches each                          ~       reference form of the fused kernel's test
 *                                  bit 5                  0        128-channel layers on the four-wave im2col kernel          ~       reference form of the raw-rows kernel's test; layers the raw-rows kernel cannot take
 *   MstFxFuse.forms (per call)     EQ_LANE_APPLY          0        stereo equaliser apply pass, one lane per chunk            =       reference form of a GPU / emulator test; non-stereo path
 *                                  EQ_VALU_ENDS           0        stereo equaliser state pass on VALU dot products           =       reference form; chunk lengths that are no multiple of 16
 *                                  COMP_SLICE_SMALL       0        compressor: three time slices whatever the size            =       lets small emulated problems take the pipelined path
 * ------------------------------------------------------------------------------------------------------------------------------------------ */
/* tuning flags of the handle (the table above; default 245 = bits 0, 2, 4, 5, 6, 7), in detail:
 *   bf16 form 2: the two- and four-phase blocks that are not the last one run tcn_block_bf16_kernel<P, false, 8, 2> (one 256-time tile per
 *     workgroup, two workgroups per CU, B fragments reused across the taps of a class); every other block - P = 1 (odd dilations), the 128-time
 *     and sixteen-phase tilings - runs what form 0 runs, bit 7's forms aside.  The two forms agree to fp32 accumulation rounding.
 *   bit 5: applies only when block 1 is the d = 2 block (two-phase tiles at every segment length) of a net of more than two blocks and at
 *     least two blocks run; otherwise the separate block-0 kernel runs - mst_tcn_get_tuning reports which happened.  Same bits either way.
 *   bit 7: a block whose phase sequences are EXACTLY one 256-time tile (L = 64 d, 32 d or 16 d: d = 2048 / 4096 / 8192 at L = 131072) runs the
 *     unrolled forms <4 | 8 | 16, ., 8, 1> (no all-padding (column tile, tap) pair; the sixteen-phase form carries the fused head): the
 *     four-phase form is bit-identical to bit 7 off, the other two one bf16 ulp away on the activation.  A four-phase LAST block (segments of
 *     >= 2^19 samples) runs the class-major head <4, true, 8, 2> instead of the tap-major <4, true, 8>: the waveform moves by <= 2e-3 (a
 *     two-phase last block is tap-major either way).
 * Measurements behind the defaults: EXPERIMENTS.md and profiles/.  mst_tcn_get_tuning returns the flags as set. */
int mst_tcn_set_tuning(MstTcn *tcn, int flags);
/* the flags in force and whether the handle's LAST forward ran block 0 inside block 1's launch (bit 5 is a request: see its conditions above);
 * either pointer may be null. */
int mst_tcn_get_tuning(const MstTcn *tcn, int *flags, int *last_forward_fused_block0);

/* Launch-level fusion of the handle (since mst_version() 104), beside the tuning flags: which KERNEL FORM a block runs stays what
 * mst_tcn_set_tuning says; this decides whether blocks that qualify share a launch.  Same bits either way.
 *   bit 0: the last three blocks of a full bf16 forward run as ONE launch (tcn_tail_bf16_kernel: the two activations between them stay in
 *     LDS) when the net has at least four blocks and the three are planned as the whole-sequence 256-time forms of four, eight and sixteen
 *     phases at dilations d, 2d, 4d with L = 64 d (tuning bit 7; d = 2048 / 4096 / 8192 at L = 131072).  Anything else - another length,
 *     tuning without bit 7, mst_tcn_forward_blocks, another precision - runs one launch per block as before.
 *   other bits: MST_ERR_ARG.
 * A handle from mst_tcn_create starts with 0: its launch table is the one the tuning flags describe.  The Python modules set bit 0
 * (_lib.TCN_FUSION_DEFAULT).  mst_tcn_get_fusion returns the flags and whether the handle's LAST forward ran the fused tail; either pointer
 * may be null. */
int mst_tcn_set_fusion(MstTcn *tcn, int flags);
int mst_tcn_get_fusion(const MstTcn *tcn, int *flags, int *last_forward_fused_tail);

/* The order of the work over the batch (since mst_version() 110).  Same kernels, same bits: items are independent through the whole net.
 * A full bf16 forward of a large batch runs in CHUNKS of `items` batch items, every chunk through all blocks (the launch table of an
 * `items`-sized batch, fused tail included) before the next one starts, two chains of chunks side by side - the caller's stream and a side
 * stream the handle owns, forked from the caller's stream and joined back into it before the call returns; no device-wide wait, nothing
 * left pending behind the caller's stream.  Every chunk of a chain reuses the same two activations of the workspace, so the next block finds
 * the last one's output in the 256 MiB Infinity Cache instead of HBM (measured at 32 x 131072: -2.5 % on the forward).
 *   items = 0: automatic - chunk only a batch whose ONE activation, B * L * 256 bytes, exceeds the cache, in chunks of the largest count for
 *     which both chains' two activations fit it (2 at L = 131072; none above L = 262144: the whole batch then).
 *   items = n >= 1: n items per chunk whatever the size (n >= B, MST_TCN_CHUNK_WHOLE: the whole batch, one launch per block as before).
 *   items < 0: MST_ERR_ARG.
 * Where the second chain's two activations do not fit the workspace beside the first's (n > B / 2) the chunks run one after the other on the
 * caller's stream.  mst_tcn_workspace_bytes is what it was.  fp32, bf16x3, mst_tcn_forward_blocks and the generic path are never chunked.
 * A handle from mst_tcn_create starts with MST_TCN_CHUNK_WHOLE: its launch table is the one the tuning flags describe.  The Python modules
 * set 0 (_lib.TCN_CHUNK_DEFAULT).  mst_tcn_get_chunk returns the setting and how many chunks the handle's LAST forward ran (1: the whole
 * batch); either pointer may be null.  The timing hook below sums a block's launches over the chunks (divided by the number of chains that
 * ran side by side). */
#define MST_TCN_CHUNK_WHOLE 0x7fffffff
int mst_tcn_set_chunk(MstTcn *tcn, int items);
int mst_tcn_get_chunk(const MstTcn *tcn, int *items, int *ran_chunks);

/* Context of the net (since mst_version() 107), host only, any handle (the generic path's included): *left / *right = how many input samples
 * before / after an output sample the forward reads - the blocks' zero paddings summed, ((k-1)*d)/2 per side and block, or (k-1)*d on the left
 * alone for a causal net; (rf - 1) / 2 = 114681 each side for the default configuration.  A caller that converts a long sequence by windows
 * reproduces the whole-sequence forward when window [a, b) runs on samples [max(0, a - left), min(L, b + right)) - clipped at the sequence's
 * ends, NOT extended with zeros: the blocks pad their ACTIVATIONS with zeros, and a zero waveform does not give zero activations - and keeps the
 * outputs of [a, b) (inference/segmentation.py plan_windows, StyleTransferEngine.convert_stem_seamless).  Either pointer may be null. */
int mst_tcn_context(const MstTcn *tcn, long *left, long *right);

/* measurement hook (bench.py's roofline leg): between _begin and _end every mst_tcn_forward records HIP events
 * on its stream around each kernel; _end synchronises, writes the AVERAGE milliseconds per forward of
 * block kernels 0..nblocks-1 followed by the output kernel into ms_out[nblocks+1], and the number of
 * forwards seen into *n_forwards.  A forward whose last three blocks ran as one launch (mst_tcn_set_fusion) reports that
 * launch's time in three equal shares, one per block. */
int mst_tcn_timing_begin(MstTcn *tcn, int max_forwards);
int mst_tcn_timing_end(MstTcn *tcn, float *ms_out, int *n_forwards);

/* Calibration of the box (measurement infrastructure, bench.py "roofline.calib_ms"): runs the BARE main loop of the bf16 TCN block
 * kernel (csrc/tcn_kernels.h::tcn_calib_mainloop_kernel: the MFMAs, weight stream and LDS reads of one dense 32 x 131072 block launch =
 * 2.06 TFLOP; no staging, no epilogue, no store) `launches` times back to back on `stream` on synthetic operands with realistic
 * statistics; the first half settles the power controller, the second half is timed with HIP events.  *ms_per_launch = average duration
 * of a timed launch, *sclk_mhz = the shader clock the last launch ran at (s_memtime / s_memrealtime inside the kernel).  Allocates and
 * frees 1.1 MB of device memory; blocks until done.  No reference counterpart. */
int mst_calib_mainloop(int launches, float *ms_per_launch, float *sclk_mhz, void *stream);

/* ------------------------------------------------------------------------------------------------
 * FXencoder (networks/architectures.py:26-70) = Res_ConvBlock x N (network_utils.py:96-119), each two
 * Conv1d_layer (network_utils.py:15-89: ReflectionPad1d -> Conv1d -> BatchNorm1d(eval) -> ReLU), then
 * AdaptiveAvgPool1d(1).
 * ---------------------------------------------------------------------------------------------- */
typedef struct MstEnc MstEnc;

typedef struct {
    int nblocks;                       /* len(config["kernels"])                                   */
    int channels[MST_MAX_BLOCKS + 1];  /* [2] + config["channels"]  (architectures.py:30)           */
    int kernels[MST_MAX_BLOCKS];
    int strides[MST_MAX_BLOCKS];
    int dilations[MST_MAX_BLOCKS];
    int valid_padding;                 /* Conv1d_layer(padding="VALID"): no reflection padding, L_out = (L - (k-1)d - 1)/s + 1   */
    float act_slope;                   /* activation of every layer (network_utils.py:76-80) as the slope for negative values:
                                        * 0 = ReLU (config "relu", the zero-initialised default), 0.01 = LeakyReLU ("lrelu"), 1 = none */
} MstEncDesc;

int mst_enc_create(const MstEncDesc *desc, MstEnc **out);
int mst_enc_destroy(MstEnc *enc);
/* which = 0: encoder.{block}.conv1 (cin->cin, stride 1), 1: encoder.{block}.conv2 (cin->cout, stride s).
 * w [cout, cin, k]; bias [cout] or NULL; BN arrays [cout].  Host side: BN folding and the MFMA-fragment images of the layer (fp32, bf16, bf16 hi / lo, raw-rows),
 * packed on up to 16 short-lived host threads (one per 128-channel tile) before the synchronous upload; the default encoder's 81 M weights load in a few hundred ms. */
int mst_enc_load_conv(MstEnc *enc, int block, int which, const float *w, const float *bias,
                      const float *bn_weight, const float *bn_bias, const float *bn_mean, const float *bn_var,
                      float bn_eps, void *stream);
/* tuning (bf16 / bf16x3 modes): a conv layer (bf16 mode: with at most 64 input channels) whose launch has at least rows_min_tiles tiles keeps its
 * input rows resident in LDS (enc_conv_rows_kernel) instead of gathering an im2col slice per k-chunk; default 512, 0 = whenever a
 * layer qualifies (any channel count), negative = never.  Both forms produce identical bits. */
int mst_enc_set_tuning(MstEnc *enc, long rows_min_tiles);
/* workgroup order of the channel-minor conv kernel (bf16 / bf16x3 modes).  bit 0 (default on): layers with more weight bytes than
 * activation bytes run their workgroups in weight-major order - all column tiles of one (channel tile, k-slice) on one XCD, so a
 * weight slice crosses the fabric once instead of once per XCD.  bit 1: rejected (MST_ERR_ARG; it selected a 2 x 2 wave
 * tiling of the 128-channel kernel, measured 7-12 % slower).  bit 2 (exact-fp32 mode, a test hook): gather through 64-bit addresses - the path that activations beyond the 32-bit offset range take
 * by themselves - instead of buffer loads.  Same bits either way.  (Round 5 built and measured an in-kernel split-K finalize - tickets, last
 * workgroup of a tile sums the partial tiles - as bit 3: correct, and 5 x SLOWER per layer (the device-scope release fence writes the
 * whole L2 back on this part; EXPERIMENTS.md D.3): not in the library.)
 * bit 3 (default off, the reference form of a GPU / emulator test): the default encoder's stereo block (2 -> 2, k = 25 with skip; 2 -> 16, k = 25,
 * stride 4) as two direct-kernel launches with the intermediate in HBM instead of the fused enc_stereo_block_kernel.  Same bits either way.
 * bit 4 (default off, bf16 mode): blocks 1 and 2 of the default encoder (16 -> 16, k = 25 with skip; 16 -> 32, k = 25, stride 4 / 32 -> 32, k = 15;
 * 32 -> 64, k = 15, stride 2) as their two conv launches each instead of the fused enc_block1_fused_kernel (intermediate in LDS, weights resident in registers); same operands, another fp32 summation
 * order: the two forms agree to accumulation rounding (one bf16 ulp on isolated elements).
 * bit 5 (default off, bf16 mode): the 128-channel layers (kernel 5 / 10, stride 1 / 2, input channels a multiple of 64, output length a multiple
 * of 32) on the four-wave im2col kernel (enc_conv_nlc_kernel<4>) instead of enc_conv_taps_kernel (raw input rows staged once per 64-channel
 * block by LDS-DMA, loader + matrix waves, 256-column tiles, split-K over channel blocks); same operands, another fp32 summation order. */
int mst_enc_set_schedule(MstEnc *enc, int flags);
/* nn.AdaptiveAvgPool1d(1) on its own (architectures.py:63,67; FXencoder(conv_block='conv') runs its ConvBlocks one by one through
 * mst_enc_forward_conv and pools here): x_dev fp32 [rows, L] -> y_dev[rows] = mean over L. */
int mst_global_avgpool(const float *x_dev, float *y_dev, long rows, int L, void *stream);
/* Conv1d_layer(mode="deconv") (network_utils.py:24-26,38-42, nn.ConvTranspose1d): the zero-stuffed input of the equivalent stride-1
 * convolution - y_dev[row][pad_left + i * stride] = x_dev[row][i], zeros elsewhere; x_dev fp32 [rows, L] -> y_dev fp32 [rows, Lu],
 * Lu >= pad_left + (L - 1) * stride + 1.  The convolution itself is mst_enc_forward_conv of a handle loaded with the tap-reversed,
 * channel-transposed weights and VALID padding (networks/network_utils.py does both). */
int mst_enc_zero_stuff(const float *x_dev, float *y_dev, long rows, long L, int stride, long pad_left, long Lu, void *stream);
size_t mst_enc_workspace_bytes(const MstEnc *enc, int B, int L);
/* replaces FXencoder.forward (architectures.py:65-70): x_dev fp32 [B, 2, L] -> emb_dev fp32 [B, C_last].
 * precision: MST_PREC_F32 (exact fp32 MFMA, parity mode) or MST_PREC_BF16 (bf16 operands, fp32 accumulate;
 * activations stay fp32 in HBM). */
int mst_enc_forward(MstEnc *enc, const float *x_dev, float *emb_dev, int B, int L, int precision, void *workspace,
                    size_t workspace_bytes, void *stream);
/* parity probe: run only the first n_run Res_ConvBlocks; out_dev fp32 [B, channels[n_run], L_out(n_run)] */
int mst_enc_forward_blocks(MstEnc *enc, const float *x_dev, float *out_dev, int B, int L, int precision, int n_run,
                           void *workspace, size_t workspace_bytes, void *stream);
/* Conv1d_layer.forward on its own (network_utils.py:86-89): ONE conv of the handle - which = 0: encoder.{block}.conv1
 * (cin->cin, stride 1), 1: conv2 (cin->cout, stride s) - ReflectionPad1d -> Conv1d -> BatchNorm1d(eval) -> ReLU, exact fp32;
 * x_dev [B, cin, L] -> y_dev [B, cout, mst_enc_conv_length(...)].  Only that conv needs to be loaded. */
int mst_enc_conv_length(const MstEnc *enc, int block, int which, int L);
int mst_enc_forward_conv(MstEnc *enc, int block, int which, const float *x_dev, float *y_dev, int B, int L, void *stream);
/* output length of Res_ConvBlock `block` for input length L ("SAME" padding ignores the stride:
 * L_out = floor((L-1)/s)+1, network_utils.py:30-34,48-51) */
int mst_enc_block_length(const MstEnc *enc, int block, int L);

/* FiLM.forward on its own (network_utils.py:163-182): f = film_fc(cond) [rows, 2C]; y = f[:, :C] * x + f[:, C:] over x_dev
 * [B, C, L] (NCL); rows = 1 (broadcast) or B.  w_dev [2C, cond_dim], b_dev [2C], cond_dev [rows, cond_dim] are device fp32
 * (the module's parameters); table_dev: >= rows * 2C floats of caller scratch. */
int mst_film_forward(const float *w_dev, const float *b_dev, const float *cond_dev, int rows, int cond_dim, int C,
                     const float *x_dev, float *y_dev, int B, long L, float *table_dev, void *stream);

/* replaces torch.stack/reshape/mean(axis=0) over segment embeddings (style_transfer.py:152-153):
 * out[d] = mean over rows of emb[n_rows, dim], summed in row order (so the result does not depend on
 * how rows were sharded across GPUs before the all-gather). */
int mst_embedding_mean(const float *emb_dev, int n_rows, int dim, float *out_dev, void *stream);

/* ------------------------------------------------------------------------------------------------
 * FX-manipulator processors (mixing_manipulator/common_audioeffects.py).  Audio layout as in the
 * reference processors: [n_items][L][C] time-major, interleaved channels, fp32.  One (item, channel)
 * sequence per lane for the serial recursions; float64 internal arithmetic like the reference.
 * ---------------------------------------------------------------------------------------------- */
/* Chain fusion (AugmentationChain.apply_processor :115-148 without its extra passes).  A processor entry point that takes an
 * MstFxFuse reads its input as x * (float)in_scale_dev[item] - the PENDING factor of the previous processor's rms-normalise,
 * applied in float32 exactly like the separate scale pass would - and leaves sum(y^2) of every item of its raw output in
 * out_sumsq_dev[item] (float64; the first launch of the call clears the slots, the caller need not; the imager writes its closed
 * form), so that an rms-normalise step costs
 * one tiny mst_fx_rms_pending launch instead of two energy passes and a scale pass over the audio.  fuse = NULL or both
 * members NULL: the plain processor.  mst_fx_scale_items applies a pending factor when a chain ends with one. */
#define MST_SUMSQ_SLOTS 64     /* an energy sum is kept as 64 partial sums per item (producers spread their atomics over them) */
#define MST_FX_FORM_EQ_LANE_APPLY 1   /* MstFxFuse.forms */
#define MST_FX_FORM_EQ_VALU_ENDS 2
#define MST_FX_FORM_COMP_SLICE_SMALL 4
typedef struct {
    /* = sizeof(MstFxFuse) of the header the CALLER was built against: an entry point given another value returns MST_ERR_ARG instead of
     * reading a struct of another layout (the struct has grown twice) */
    unsigned struct_size;
    /* kernel forms of this call - per call, not per process (round 6: the library keeps no mutable global state); results do not depend on
     * them.  mst_fx_biquad_cascade, stereo: MST_FX_FORM_EQ_LANE_APPLY = the apply pass one lane per chunk straight from global memory
     * (fx_biquad_chunk_kernel<true>) instead of 16-frame slabs through LDS (fx_biquad_stereo_apply_kernel), identical bits;
     * MST_FX_FORM_EQ_VALU_ENDS = the state pass as float64 VALU dot products with the impulse-state table in LDS
     * (fx_biquad_stereo_ends_kernel) instead of v_mfma_f64_16x16x4_f64 with the table as A fragments (fx_biquad_stereo_ends_mfma_kernel),
     * the same products added in the same (sample) order.  Both are the reference forms of a GPU test.  mst_fx_compressor:
     * MST_FX_FORM_COMP_SLICE_SMALL = cut the time-parallel compressor into its three time slices (map / apply kernels of neighbouring slices
     * on an internal low-priority side stream beside the chain kernel, events order map_i -> chain_i -> apply_i, the caller's stream joins
     * the side stream before the call returns) whatever the size of the batch (>= 8 chain batches) - large batches (>= 32 chain batches of
     * 1024 samples and >= 4e6 samples in all) always are; the hook lets small emulated problems take that path.  0: the defaults. */
    int forms;
    const double *in_scale_dev;   /* [n_items] or NULL */
    double *out_sumsq_dev;        /* [n_items][MST_SUMSQ_SLOTS] or NULL; overwritten */
    /* tail folding (mst_fx_midside_imager only; the other entry points refuse post_rms != 0): the rms-normalise that FOLLOWS the
     * processor and a Gain behind it happen in the processor's own last pass, y_out = (y * s) * post_gain in float32 - the values the
     * separate mst_fx_rms_pending + mst_fx_gain launches produce - with s from in_sumsq_dev = sum(x_raw^2) of the processor's raw input
     * ([n_items][MST_SUMSQ_SLOTS]) and the closed-form energy of y */
    const double *in_sumsq_dev;
    int post_rms;
    float post_gain;
    /* mst_fx_biquad_cascade only (the others refuse it): also leave sum(x_raw^2) of the call's raw input here
     * ([n_items][MST_SUMSQ_SLOTS], the arithmetic of mst_fx_sumsq) - the first rms-normalise of a chain then needs no energy pass over x */
    double *out_in_sumsq_dev;
    /* mid / side energies handed from mst_fx_compressor (stereo; the others refuse it) to mst_fx_midside_imager: the compressor leaves
     * sum((l + r)^2), sum((l - r)^2) of its raw output - float32 sums and squares per frame, float64 accumulation, the arithmetic of the
     * imager's own energy pass - as MST_SUMSQ_SLOTS pairs per item in out_ms_dev ([n_items][MST_SUMSQ_SLOTS][2]: slot s covers a 64th of the
     * frames, summed in a fixed order - deterministic since round 6), and an imager given the same array as in_ms_dev skips its energy pass
     * over the audio.  NULL: off. */
    double *out_ms_dev;
    const double *in_ms_dev;
} MstFxFuse;
int mst_fx_sumsq(const float *x_dev, int n_items, long per_item, double *out_dev, void *stream);   /* out[item][slot]: partial sums of x^2 */
/* scale_out[item] = float32(sqrt(mean(x_true^2) / max(1e-7, mean(y^2)))), mean(x_true^2) = scale_x^2 sum_slots(sumsq_x) / per_x
 * (scale_x NULL = 1); sumsq_x / sumsq_y in the [n_items][MST_SUMSQ_SLOTS] form */
int mst_fx_rms_pending(const double *scale_x_dev, const double *sumsq_x_dev, long per_x, const double *sumsq_y_dev, long per_y,
                       double *scale_out_dev, int n_items, void *stream);
int mst_fx_scale_items(const float *x_dev, float *y_dev, int n_items, long per_item, const double *scale_dev, void *stream);

/* Equaliser.process (:500-525): cascade of n_bands biquads, zero initial state per band; coef host
 * float64 [n_bands][6] = (b0,b1,b2,a0,a1,a2) shared by all items.  With a scratch buffer of
 * mst_fx_biquad_scratch_bytes() the cascade runs parallel in time (chunked state-space scan, same float64
 * per-sample recursion); with scratch_dev = NULL it runs one lane per (item, channel) sequence. */
size_t mst_fx_biquad_scratch_bytes(int n_items, long L, int C, int n_bands);
int mst_fx_biquad_cascade(const float *x_dev, float *y_dev, int n_items, long L, int C, const double *coef_host,
                          int n_bands, double *scratch_dev, size_t scratch_bytes, const MstFxFuse *fuse, void *stream);

/* DIAGNOSTIC (since mst_version() 102): what mst_fx_biquad_cascade does with a scratch buffer for this shape, and where its float64
 * intermediates lie in that buffer after the call.  Host only, launches nothing.  The layout is an implementation detail: it may change
 * with mst_version().  ends / starts: [n_items * C][nchunks][record_doubles] float64, state order (z1, z2) per band, the states beyond
 * 2 * n_bands unused; ends = the zero-state end state of every FULL chunk of M samples (a short last chunk's record is zeros), starts =
 * the true state at the start of every chunk.  time_parallel 0: the serial kernel runs (one chunk, or no band) and the buffer is unused. */
typedef struct {
    unsigned struct_size;        /* = sizeof(MstFxBiquadPlan) of the caller's header; another value: MST_ERR_ARG */
    int time_parallel;
    int M;                       /* samples per chunk */
    int scan_threads;            /* 256 or 512: workgroup size of the scan over the chunk states (0: no scan) */
    int record_doubles;          /* float64 values per chunk record */
    long nchunks;
    size_t ends_offset, starts_offset;      /* bytes from scratch_dev */
} MstFxBiquadPlan;
int mst_fx_biquad_plan(int n_items, long L, int C, int n_bands, MstFxBiquadPlan *plan);
/* DIAGNOSTIC (since mst_version() 102), host only: the tables the time-parallel cascade of coef_host ([n_bands][6] as for
 * mst_fx_biquad_cascade) uploads for chunk length M (a multiple of 16; MstFxBiquadPlan.M) - made by the very code the call runs -
 * table_host [M][2 n_bands]: the state m steps after a unit impulse; powers_host [9][2 n_bands][2 n_bands] row-major: (A^M)^(2^l),
 * l = 0 .. 8, A^M by the float64 recursion, squared up level by level. */
int mst_fx_biquad_tables(const double *coef_host, int n_bands, int M, double *table_host, double *powers_host);

/* PER-ITEM PARAMETERS (since mst_version() 103).  mst_fx_biquad_cascade with a coefficient set per item, in the launches of the shared call
 * plus one: coef_dev is DEVICE float64 [n_items][n_bands][6], rows in coef_host's order (b0 b1 b2 a0 a1 a2); n_bands is common to the
 * batch.  A launch on the caller's stream builds every item's tables on the device - the impulse states [M][2 n_bands] and the powers
 * (A^M)^(2^l), l = 0 .. 8 - with M the chunk length of the shared call on this shape (the state pass of stereo audio is the VALU one for
 * every item: no A-fragment image; MST_FX_FORM_EQ_VALU_ENDS changes nothing here): no host build, no upload, no cache entry, no mutex, no synchronisation, nothing the stream does not order.  The tables are
 * the bits mst_fx_biquad_tables returns for the item's coefficients, and item i's output and by-products are the bits of
 * mst_fx_biquad_cascade on the same batch with item i's coefficients.  scratch_dev: mst_fx_biquad_items_scratch_bytes(); it starts
 * with the shared call's layout (ends / starts where mst_fx_biquad_plan says), the per-item tables lie behind
 * (mst_fx_biquad_items_plan).  fuse: as mst_fx_biquad_cascade (in_scale_dev, out_sumsq_dev, out_in_sumsq_dev, the EQ forms).
 * scratch_dev = NULL or a single chunk: the serial kernel with per-item coefficients (no fusion).  n_items <= 65535. */
size_t mst_fx_biquad_items_scratch_bytes(int n_items, long L, int C, int n_bands);
int mst_fx_biquad_cascade_items(const float *x_dev, float *y_dev, int n_items, long L, int C, const double *coef_dev, int n_bands,
                                double *scratch_dev, size_t scratch_bytes, const MstFxFuse *fuse, void *stream);
/* DIAGNOSTIC, host only: where mst_fx_biquad_cascade_items leaves item i's tables - at tables_offset + i * item_stride bytes from
 * scratch_dev: [M][2 n_bands] impulse states, at + powers_offset [9][2 n_bands][2 n_bands] powers, at + coef_offset [8][5] b0 b1 b2 a1 a2 over a0 (zeros beyond n_bands).  The layout may change with mst_version(). */
typedef struct {
    unsigned struct_size;        /* = sizeof(MstFxBiquadItemsPlan) of the caller's header; another value: MST_ERR_ARG */
    int M;                       /* samples per chunk: MstFxBiquadPlan.M of the same shape */
    size_t tables_offset, item_stride, powers_offset, coef_offset, total_bytes;      /* bytes */
} MstFxBiquadItemsPlan;
int mst_fx_biquad_items_plan(int n_items, long L, int C, int n_bands, MstFxBiquadItemsPlan *plan);

/* Compressor.process / compressor_process (:529-587, :637-649), makeup gain 0.  With a scratch buffer of
 * mst_fx_compressor_scratch_bytes() (about 9 bytes per sample) the gain computer and the gain application run over all samples
 * in parallel and the attack/release smoother runs parallel in time (per-chunk convex piecewise-linear maps + one walk over the
 * chunk summaries of each sequence); scratch_dev = NULL runs the serial form, one wave per sequence.
 * The time-parallel smoother runs only where its chunk maps are well conditioned: the pieces of a 32-step chunk map have slopes
 * aA^(32-p) aR^p (aA, aR = exp(-1 / (0.001 sample_rate time_ms))), and the walk over the chunks loses kappa = (max / min)^32 of them in
 * float64.  Beyond kappa_limit (MstFxCompressorPlan; about 6e5: at 44.1 kHz an attack below ~0.055 ms against a slow release) a plain call
 * runs the serial form whatever the scratch buffer, and a call that form cannot serve - chain fusion (in_scale_dev / out_sumsq_dev), or
 * mst_fx_compressor_grid - returns MST_ERR_UNSUPPORTED, the message naming the attack and release coefficients and the limit.
 * kappa_limit = 6.07e5 - min(L, 1 / (1 - max(aA, aR))): it falls with the signal length and the slower time constant and is negative once
 * both pass about 6e5 samples (a release above ~14 s at 44.1 kHz on a signal that long); every such call is serial or refused. */
size_t mst_fx_compressor_scratch_bytes(int n_items, long L, int C);
/* DIAGNOSTIC (since mst_version() 102): which form mst_fx_compressor / mst_fx_compressor_grid take for this shape and these times when given
 * the scratch buffer, and where the intermediates lie in it after the call.  Host only, launches nothing; the layout may change with
 * mst_version().  forms: MstFxFuse.forms of the call.
 *   xl      [L][n_seq] float64 (SPLIT_SERIAL only; n_seq = n_items * C): the smoothed level y_l of every sample
 *   maps    [n_seq][nchunks][record_doubles]: per 32-sample chunk b_0 (intercept of the all-attack piece), lb_1 .. lb_n (the sorted values at
 *           which the pieces of the chunk's map meet, n = samples of the chunk), 1e300 beyond the chunk's pieces
 *   ystart  [nchunks][n_seq]: the smoother's value at the start of every chunk
 *   tab     [256]: unused by the call (the log10 table lives in a buffer of the library's)
 *   carry   [n_seq]: the smoother's value behind the last sample (between two time slices: behind the slice)
 *   tsums   per 64-sample tile: [tile][n_items][3] = sum y^2, sum (l + r)^2, sum (l - r)^2 with out_ms_dev, else [tile][n_seq] = sum y^2
 * Time slice i of nslices covers the chain batches (32 chunks each) nbatch * i / nslices .. nbatch * (i + 1) / nslices - 1. */
#define MST_FX_COMP_SPLIT_SERIAL 0     /* fewer than four chunks: gain / smoother / apply kernels, one lane per sequence in the smoother */
#define MST_FX_COMP_TIME_PARALLEL 1    /* chunk maps, chain walk, apply */
#define MST_FX_COMP_WAVE_SERIAL 2      /* kappa > kappa_limit: one wave per sequence, no scratch use; fusion and grid calls are refused */
typedef struct {
    unsigned struct_size;        /* = sizeof(MstFxCompressorPlan) of the caller's header; another value: MST_ERR_ARG */
    int form;                    /* MST_FX_COMP_* */
    int nslices;
    int record_doubles;          /* float64 values per chunk record of maps */
    long nchunks, nbatch, ntiles;
    double kappa, kappa_limit;
    size_t xl_offset, maps_offset, ystart_offset, tab_offset, carry_offset, tsums_offset, total_bytes;      /* bytes from scratch_dev */
} MstFxCompressorPlan;
int mst_fx_compressor_plan(int n_items, long L, int C, double attack_ms, double release_ms, double sample_rate, int forms,
                           MstFxCompressorPlan *plan);
int mst_fx_compressor(const float *x_dev, float *y_dev, int n_items, long L, int C, double threshold_db,
                      double attack_ms, double release_ms, double ratio, double sample_rate, double *scratch_dev,
                      size_t scratch_bytes, const MstFxFuse *fuse, void *stream);
/* The compressor with threshold, attack, release and ratio PER ITEM (since mst_version() 103), in the launches of mst_fx_compressor: the same
 * forms (split-serial below four chunks, time-parallel, time slices), the scratch buffer and its layout are mst_fx_compressor's
 * (mst_fx_compressor_scratch_bytes, mst_fx_compressor_plan), fusion as there including out_ms_dev; per-item x.  One batch may mix items with
 * attack slower and faster than release and ratios above, below and equal to 1.  Item i gets the bits of mst_fx_compressor on the same batch
 * with item i's settings.
 * mst_fx_compressor_items_prepare (host only, launches nothing) fills the table the call reads - table_host, of
 * mst_fx_compressor_items_table_bytes(n_items), meant to be pinned and uploaded without waiting - from params_host [n_items][4] = threshold
 * dB, attack ms, release ms, ratio, with the functions the shared call uses: per item threshold and ratio (the curve), the attack / release
 * coefficients and the two slope / inverse-slope rows of the chunk maps.  It applies mst_fx_compressor_plan's kappa_limit rule per item: an
 * item beyond it makes the call return MST_ERR_UNSUPPORTED - the message names the item, its coefficients and the limit - and writes its index
 * to first_refused_item (else -1); run such an item alone through mst_fx_compressor.  The bypass pair (threshold 0, ratio 1) is refused the same
 * way.  table_dev must come from a successful prepare for the same n_items, L, C.  scratch_dev = NULL: the serial kernel. */
size_t mst_fx_compressor_items_table_bytes(int n_items);
int mst_fx_compressor_items_prepare(const double *params_host, int n_items, long L, int C, double sample_rate, int forms,
                                    double *table_host, size_t table_bytes, int *first_refused_item);
int mst_fx_compressor_items(const float *x_dev, float *y_dev, int n_items, long L, int C, const double *table_dev, double *scratch_dev,
                            size_t scratch_bytes, const MstFxFuse *fuse, void *stream);
/* MidSideImager.process (:964-1007), stereo only; scratch_dev: >= n_items * 2 * MST_SUMSQ_SLOTS doubles (partial energy sums) */
int mst_fx_midside_imager(const float *x_dev, float *y_dev, int n_items, long L, double bal, double *scratch_dev,
                          const MstFxFuse *fuse, void *stream);
/* The imager with a balance per item (since mst_version() 103): bal_dev is DEVICE float64 [n_items], rounded to three places on the device
 * like the shared call does on the host.  post_gain_dev: DEVICE float32 [n_items], the per-item gain of the tail folding (fuse->post_rms);
 * NULL: fuse->post_gain for every item.  Everything else as mst_fx_midside_imager, whose bits item i gets for bal_dev[i]. */
int mst_fx_midside_imager_items(const float *x_dev, float *y_dev, int n_items, long L, const double *bal_dev, double *scratch_dev,
                                const float *post_gain_dev, const MstFxFuse *fuse, void *stream);
/* Haas.process / haas_process (:768-786, :826-843): y = x, y[:, wet] += feedback * np.roll(x[:, wet], delay) - the roll is
 * circular, delay may be negative; wet_channel 0 = 'left', 1 = 'right'.  c_in = 1 (mono, repeated to stereo) or 2;
 * y is always [n_items, L, 2]. */
int mst_fx_haas(const float *x_dev, float *y_dev, int n_items, long L, int c_in, long delay, double feedback,
                int wet_channel, void *stream);
/* Panner.process (:927-943): x * gains with the two gains of Panner._calculate_pan_coefficents (:882-912) computed by
 * the caller (float32, like the reference's self.gains); c_in = 1 or 2, y is [n_items, L, 2]. */
int mst_fx_panner(const float *x_dev, float *y_dev, int n_items, long L, int c_in, float gain_left, float gain_right,
                  void *stream);
/* ConvolutionalReverb.process (:727-764): y = dry * x + wet * (x (*) h)[offset : offset + L] per channel, x (*) h the FULL
 * linear convolution (scipy.signal.oaconvolve(x, h, mode='full', axes=0) in the reference).  Computed as one FFT convolution of
 * n_fft = next power of two >= L + Lh_max - 1 per (item, channel): the library's own FFT kernels (csrc/fft_kernels.h) + three HIP kernels.
 * The caller resolves what the reference does on the host: IR choice / decay fade (:704-725), mono <-> stereo IR (:739-742),
 * offset = argmax_t max_c |h| + pre-delay samples, clipped to [0, Lh-1] (:757-761).  x/y: [n_items, L, C]; h: [Lh, C] device
 * float32, one impulse response for all items (apply_same_processor, :150-154).  All L + Lh - 1 samples are exact linear
 * convolution (no circular wrap).  A convolver owns its FFT plans; workspace is caller memory. */
typedef struct MstConvolver MstConvolver;
int mst_fx_convolver_create(long L, long Lh_max, int n_items, int C, MstConvolver **out);
void mst_fx_convolver_destroy(MstConvolver *cv);
size_t mst_fx_convolver_workspace_bytes(const MstConvolver *cv);
int mst_fx_convolve(MstConvolver *cv, const float *x_dev, const float *h_dev, long Lh, float *y_dev, long offset, double dry,
                    double wet, void *workspace_dev, size_t workspace_bytes, void *stream);
/* PER-ITEM PARAMETERS, continued (since mst_version() 105): the panner, the Haas effect and both reverbs.  The conventions of the 103 entry
 * points: parameters in device arrays, the item on the grid's y axis (n_items <= 65535), no global state, no synchronisation, nothing the
 * caller's stream does not order.  Item i gets the bits of the shared-parameter call on the same batch with item i's settings: a per-item
 * kernel runs the `__device__` body of its shared kernel with values read per item (the spectrum product repeats fx_conv_mul_kernel's).
 * mst_fx_panner_items: gains_dev DEVICE float32 [n_items][2], the two gains of the pan law (computed by the caller, as for mst_fx_panner). */
int mst_fx_panner_items(const float *x_dev, float *y_dev, int n_items, long L, int c_in, const float *gains_dev, void *stream);
/* mst_fx_haas_items: delay_dev DEVICE int64 [n_items], of any sign and size - reduced on the device as mst_fx_haas does on the host, delay % L,
 * + L if negative; feedback_dev DEVICE float64 [n_items], rounded to float32 as there; wet_channel_dev DEVICE int [n_items], 0 or 1 - any other
 * value makes that item a plain copy of the stereo-expanded input (the reference's if / elif falls through).  In-place calls are refused. */
int mst_fx_haas_items(const float *x_dev, float *y_dev, int n_items, long L, int c_in, const long *delay_dev, const double *feedback_dev,
                      const int *wet_channel_dev, void *stream);
/* mst_fx_convolve with an impulse response, an offset, dry and wet PER ITEM, on an existing convolver: its L, Lh_max, C and item capacity fix
 * the transform size and the overlap-save geometry, so item i has the bits of mst_fx_convolve on that convolver with item i's response and
 * settings.  bank_dev: DEVICE float32 [bank_frames][C], the n_resp DISTINCT responses of the batch back to back in the audio layout; several
 * items may name the same response, which is packed and transformed once per call.  An item whose wet is 0 is its input exactly, whatever dry
 * is (ConvolutionalReverb.process returns x).
 * mst_fx_convolve_items_prepare (host only, launches nothing) checks and fills the table the call reads - table_host, of
 * mst_fx_convolve_items_table_bytes(n_items, n_resp), meant to be pinned and uploaded without waiting - from resp_start_host / resp_len_host
 * [n_resp] (first frame and frames of each response in the bank) and params_host [n_items][4] = response index, offset, dry, wet.  Refused:
 * a response with len outside 1 ... Lh_max or start + len > bank_frames (MST_ERR_ARG, the message names the response, first_bad_item -1); an
 * item whose response index is outside [0, n_resp) or whose offset is outside [0, len - 1] (MST_ERR_ARG, the message names the item, its index
 * in first_bad_item); n_items beyond the convolver's capacity (MST_ERR_ARG, first_bad_item = the capacity, the first item without a place);
 * (n_items * blocks per sequence + n_resp) * C > 65535 (MST_ERR_UNSUPPORTED: split the batch).  workspace: caller memory of
 * mst_fx_convolver_items_workspace_bytes(cv, n_resp), else MST_ERR_WORKSPACE. */
size_t mst_fx_convolver_items_workspace_bytes(const MstConvolver *cv, int n_resp);
size_t mst_fx_convolve_items_table_bytes(int n_items, int n_resp);
int mst_fx_convolve_items_prepare(const MstConvolver *cv, const long *resp_start_host, const long *resp_len_host, int n_resp, long bank_frames,
                                  const double *params_host, int n_items, double *table_host, size_t table_bytes, int *first_bad_item);
int mst_fx_convolve_items(MstConvolver *cv, const float *x_dev, const float *bank_dev, const double *table_dev, int n_items, int n_resp,
                          float *y_dev, void *workspace_dev, size_t workspace_bytes, void *stream);
/* Gain.process (:1041-1051) */
int mst_fx_gain(const float *x_dev, float *y_dev, int n_items, long L, int C, double gain_db, int invert, const MstFxFuse *fuse,
                void *stream);
/* Gain with a value per item (since mst_version() 103): gain_db_dev DEVICE float64 [n_items], invert_dev DEVICE int [n_items] (NULL: none
 * inverted).  The float32 factor comes from the function mst_fx_gain uses on the host, compiled for the device. */
int mst_fx_gain_items(const float *x_dev, float *y_dev, int n_items, long L, int C, const double *gain_db_dev, const int *invert_dev,
                      const MstFxFuse *fuse, void *stream);
/* AugmentationChain.apply_processor rms_normalize branch (:143-146): y *= sqrt(mean(x^2)/max(1e-7, mean(y^2)))
 * per item; per_x / per_y = samples per item of x and of y (L * channels each: the means are scalars over each array, and a
 * processor such as Panner / Haas may turn mono into stereo); scratch_dev: >= n_items*4 doubles */
int mst_fx_rms_normalize(const float *x_dev, float *y_dev, int n_items, long per_x, long per_y, double *scratch_dev, void *stream);


/* ------------------------------------------------------------------------------------------------
 * Kernels under the input normaliser Audio_Effects_Normalizer (mixing_manipulator/data_normalization.py:76-155), which
 * inference/style_transfer.py applies to the input stems by default (data_loader.py:586-587).  The normaliser's control
 * flow (feature tables, gating, FIR design, the search loop) is host code in the package; these entry points carry its
 * sample-rate work.
 * ---------------------------------------------------------------------------------------------- */
/* The threshold x ratio search of get_comp_matching (utils_data_normalization.py:384-398): n_items candidate settings of
 * compressor_process applied to ONE input signal x_dev [L, C]; item i uses (threshold_db_dev[i], ratio_dev[i]) (device
 * float64 arrays) and writes y_dev[i] [L, C].  scratch as for mst_fx_compressor with n_items items.  peak_dev (n_items * 64
 * doubles, may be NULL): when given, a candidate whose peak reaches 1.0 is clipped to [-1, 1] like `compress` does (:352-353). */
int mst_fx_compressor_grid(const float *x_dev, float *y_dev, int n_items, long L, int C, const double *threshold_db_dev,
                           const double *ratio_dev, double attack_ms, double release_ms, double sample_rate,
                           double *scratch_dev, size_t scratch_bytes, double *peak_dev, void *stream);
/* out_dev[r] = sum of squares (mode 0) or max |x| (mode 1), float64, over x_dev[item_dev[r]][lo_dev[r] : hi_dev[r]][channel]
 * of a [n_items, L, C] batch.  Mode 0 gives the BS.1770 gating-block energies of lufs_normalize (fx_utils.py:220-238;
 * pyloudnorm Meter.integrated_loudness), mode 1 the peak of every inter-onset interval of get_mean_peak
 * (utils_data_normalization.py:316-321). */
int mst_fx_range_reduce(const float *x_dev, long L, int C, int channel, const int *item_dev, const long *lo_dev,
                        const long *hi_dev, int n_ranges, int mode, double *out_dev, void *stream);
/* Onset-detection function of aubio.onset('hfc', buf_size = hop_size = win) as driven by get_mean_peak
 * (utils_data_normalization.py:304-314), for every whole frame of `win` samples of channel `channel` of each item:
 * out_dev[item][frame] = (hfc, mean square of the frame) as float pairs; hfc = sum_k (k+1) log(|X_k| + 1) over the
 * hanningz-windowed frame's spectrum.  win in {256, 512, 1024, 2048}.  The peak picking over this short sequence is host code. */
int mst_fx_onset_hfc(const float *x_dev, int n_items, long L, int C, int channel, int win, float *out_dev, void *stream);
/* Mean STFT magnitude of get_eq_matching (utils_data_normalization.py:74-79: librosa.stft(center=False) with the given window,
 * |.|, mean over frames): mean_dev[k], k = 0 .. n_fft/2, of channel `channel` of x_dev [L, C].  Transforms in batches
 * of at most max_batch frames (csrc/fft_kernels.h: n_fft must be a power of two >= 4 - the reference's FFT_SIZE is 65536 - otherwise
 * MST_ERR_UNSUPPORTED); the analysis window is host float32 [n_fft]. */
typedef struct MstStft MstStft;
int mst_fx_stft_create(long n_fft, long hop, const float *window_host, int max_batch, MstStft **out);
void mst_fx_stft_destroy(MstStft *st);
size_t mst_fx_stft_workspace_bytes(const MstStft *st);
int mst_fx_stft_mean_magnitude(MstStft *st, const float *x_dev, long L, int C, int channel, float *mean_dev, void *workspace_dev,
                               size_t workspace_bytes, void *stream);
/* normalize_imager / process_balance (normalization_imager.py:22-99): out_dev[item] = (sum L^2, sum R^2, sum L*R) in float64 of a
 * stereo batch [n_items, L, 2] - the mid / side / left / right energies of every step of the balancing follow from these -
 * and y = M x per stereo sample, the composed re-mix (l', r') = (m00 l + m01 r, m10 l + m11 r). */
int mst_fx_stereo_moments(const float *x_dev, int n_items, long L, double *out_dev, void *stream);
int mst_fx_stereo_mix(const float *x_dev, float *y_dev, int n_items, long L, float m00, float m01, float m10, float m11, void *stream);
/* AlgorithmicReverb.process (common_audioeffects.py:1447-1495): per side (left / right, the right delays longer by
 * stereo_spread samples) the SUM of n_combs damped feedback comb filters on in_gain * x, then n_allpass all-pass sections in
 * series, then out_L = wet1 xL + wet2 xR + dry x_L, out_R = wet1 xR + wet2 xL + dry x_R.  comb_delays [n_combs] and
 * allpass_delays [n_allpass][2] (left, right) are host arrays; feedback of both filter kinds = room_size.  x_dev [n_items, L, C]
 * (C = 1 or 2) -> y_dev [n_items, L, 2].  The caller resolves the reference's quirks (only combs 5..8 reach the output, the
 * 255-sample right delay of the last all-pass).  Comb / all-pass arithmetic restated from the published Schroeder / Freeverb
 * structure (pymixconsole.components, not vendored): parity unpinned. */
size_t mst_fx_algorithmic_reverb_scratch_bytes(int n_items, long L, int n_combs);
int mst_fx_algorithmic_reverb(const float *x_dev, float *y_dev, int n_items, long L, int C, const int *comb_delays, int n_combs,
                              const int *allpass_delays, int n_allpass, int stereo_spread, double damping, double room_size,
                              double in_gain, double wet1, double wet2, double dry, double *scratch_dev, size_t scratch_bytes,
                              void *stream);

/* mst_fx_algorithmic_reverb with damping, room_size, wet1, wet2 and dry PER ITEM (since mst_version() 105): params_dev DEVICE float64
 * [n_items][5] in that order; in_gain, the delays and stereo_spread stay shared (class constants of the processor).  Scratch as for the shared
 * call, whose bits item i gets for its row; n_items <= 32767 (two sides per item on a grid axis). */
int mst_fx_algorithmic_reverb_items(const float *x_dev, float *y_dev, int n_items, long L, int C, const int *comb_delays, int n_combs,
                                    const int *allpass_delays, int n_allpass, int stereo_spread, double in_gain, const double *params_dev,
                                    double *scratch_dev, size_t scratch_bytes, void *stream);

/* ------------------------------------------------------------------------------------------------
 * Multi-scale spectral distance: MultiScale_Spectral_Loss_MidSide_DDSP (modules/loss.py:99-213) over FrontEnd(mode=["mag"])
 * (modules/front_back_end.py:9-82), forward only.  Per scale: torch.stft(center=True, reflect) magnitudes m = sqrt(re^2 + im^2 + 1e-7) of
 * bins 1 .. n_fft / 2 (FrontEnd drops the DC bin) over T = 1 + L / hop frames, minus the last one when L % (n_fft / 4) == 0, of the mid /
 * side (L + R, L - R: mode midside) or left / right (mode ori) signals of est and tgt.  One fused kernel per scale
 * (csrc/mss_kernels.h): frames, spectra and magnitudes never reach HBM.
 * ---------------------------------------------------------------------------------------------- */
#define MST_MSS_MAX_SCALES 8
#define MST_MSS_MIDSIDE 0
#define MST_MSS_ORI 1
#define MST_MSS_HANN 0
#define MST_MSS_HAMMING 1
typedef struct MstMss MstMss;
typedef struct {
    unsigned struct_size;                 /* = sizeof(MstMssDesc) of the caller's header; another value: MST_ERR_ARG */
    int mode;                             /* MST_MSS_MIDSIDE / MST_MSS_ORI */
    int n_scales;                         /* 1 .. MST_MSS_MAX_SCALES */
    int n_fft[MST_MSS_MAX_SCALES];        /* n_filters: a power of two, 256 .. 4096 */
    int hop[MST_MSS_MAX_SCALES];          /* hops_size: 1 .. n_fft */
    int win_length[MST_MSS_MAX_SCALES];   /* windows_size: 1 .. n_fft; a shorter window is centred in the frame (torch.stft) */
    int window;                           /* MST_MSS_HANN / MST_MSS_HAMMING, periodic, float64 cosine rounded once */
    double eps;                           /* added to both magnitudes before log10 (the loss's eps, default 1e-7) */
} MstMssDesc;
/* anything outside the ranges above: MST_ERR_UNSUPPORTED, the message names the offending value */
int mst_mss_create(const MstMssDesc *desc, MstMss **out);
int mst_mss_destroy(MstMss *h);
/* frames per (item, channel) of scale `scale` for signals of L samples (negative: MstStatus) */
int mst_mss_frames(const MstMss *h, int scale, long L);
size_t mst_mss_workspace_bytes(const MstMss *h, int B, long L);
/* est_dev, tgt_dev fp32 [B, 2, L] -> terms_dev float64 [B][n_scales][2][2]: for item b, scale s, channel c (mid, side / left, right)
 *   [0] sum over bins and frames of |m_est - m_tgt|,  [1] sum of (log10(m_est + eps) - log10(m_tgt + eps))^2
 * (the loss's means are these sums over B * (n_fft / 2) * T).  float32 transforms, float64 sums added in a fixed order without atomics:
 * an item's terms are the same bits in every run and in every batch; est == tgt gives exactly 0.  L must exceed n_fft / 2 of every scale
 * (reflection padding), else MST_ERR_UNSUPPORTED. */
int mst_mss_forward(MstMss *h, const float *est_dev, const float *tgt_dev, int B, long L, double *terms_dev, void *workspace,
                    size_t workspace_bytes, void *stream);
/* FrontEnd.forward(mode=["mag"]) of one scale: x_dev fp32 [B, C, L], C = 1 (channel="mono") or 2 ("stereo") -> mag_dev fp32
 * [B, C, n_fft / 2, mst_mss_frames()].  The handle's mode and its other scales play no part: L must exceed n_fft / 2 of THIS scale.
 * (Both entry points take at most 65535 items per call: MST_ERR_UNSUPPORTED beyond.) */
int mst_mss_spectrogram(MstMss *h, int scale, const float *x_dev, int B, int C, long L, float *mag_dev, void *stream);
/* The gradient of mst_mss_forward's terms with respect to est (since mst_version() 109): the vector-Jacobian product
 *   grad_est_dev[b] = sum over scales s, channels c of  dterms_dev[b][s][c][0] d S0 / d est + dterms_dev[b][s][c][1] d S1 / d est,
 * S0, S1 the two sums of (b, s, c) that mst_mss_forward leaves; sgn(0) = 0 as in torch.  Per scale one fused kernel repeats the forward's
 * transform, forms the per-bin cotangent and runs the adjoint transform in LDS, leaving windowed gradient frames in the workspace; a second
 * gathers them per sample through the reflection padding and un-mixes mid / side.  The cotangents are read on the device (no host
 * synchronisation) and rounded to float32.  No atomics: an item's gradient is the same bits in every run and in every batch; est == tgt,
 * est == 0 and zero cotangents give exact zeros.  grad_est_dev fp32 [B, 2, L] is written, not accumulated.  Limits of mst_mss_forward, and
 * hop >= n_fft / 16 for every scale (MST_ERR_UNSUPPORTED otherwise; the forward accepts smaller hops).  The workspace is one
 * [B, 2, T, n_fft] fp32 frames buffer, the largest over the scales. */
size_t mst_mss_backward_workspace_bytes(const MstMss *h, int B, long L);
int mst_mss_backward(MstMss *h, const float *est_dev, const float *tgt_dev, int B, long L, const double *dterms_dev, float *grad_est_dev,
                     void *workspace, size_t workspace_bytes, void *stream);

/* ----------------------------------------------------------------------------------------------
 * Mixing-feature metrics (csrc/mixfeat_kernels.h): the per-frame work of the reference's panning, dynamics and low-frequency features
 * (mixing_manipulator/utils_data_normalization.py: get_SPS :109-139, get_panning_rms :682-703, get_rms_dynamic_crest :777-811,
 * get_low_freq_weighting :823-846).  Audio in the FX layout, fp32 [n_items][L][C].  Framing is librosa.stft(center = False): frame t
 * covers samples t hop .. t hop + n_fft - 1, T = 1 + (L - n_fft) / hop frames; the window is sqrt(hanning(n_fft + 1)[:-1]).  scale_dev
 * (fp32 [n_items], may be NULL = 1): every sample is x * scale[item], rounded to float32, before anything else
 * (pyloudnorm.normalize.peak folded into the load).  float32 transforms and magnitudes, float64 per-bin arithmetic and sums in a fixed
 * order without atomics: an item's numbers are the same bits alone, in a batch and from run to run.  At most 65535 items per call.
 * ---------------------------------------------------------------------------------------------- */
typedef struct MstMixfeat MstMixfeat;
/* n_fft a power of two, 512 .. 4096, hop 1 .. n_fft; anything else MST_ERR_UNSUPPORTED */
int mst_mixfeat_create(int n_fft, int hop, MstMixfeat **out);
int mst_mixfeat_destroy(MstMixfeat *h);
/* frames of a signal of L samples (0 when L < n_fft; negative: MstStatus) */
int mst_mixfeat_frames(const MstMixfeat *h, long L);
/* x_dev [n_items][L][2] -> out_dev float64 [n_items][T][n_bands]: the sum over the bins band_lo[j] <= k < band_hi[j] (host arrays,
 * n_bands 1 .. 8, inside 0 .. n_fft / 2 + 1) of SPS_k^2, where from l = |X_left + 1e-20| and r = |X_right + 1e-20| (float32)
 * phi = 2 l r / (l^2 + r^2) and SPS = (1 - phi) sign(r - l) in float64.  A frame with l == r in every bin (mono, digital silence) gives
 * exactly 0. */
int mst_mixfeat_panning(MstMixfeat *h, const float *x_dev, int n_items, long L, const float *scale_dev, const int *band_lo,
                        const int *band_hi, int n_bands, double *out_dev, void *stream);
/* get_SPS(frames=True): phi_dev, sps_dev fp32 [n_items][T][n_fft / 2 + 1] of x_dev [n_items][L][2] */
int mst_mixfeat_sps(MstMixfeat *h, const float *x_dev, int n_items, long L, const float *scale_dev, float *phi_dev, float *sps_dev,
                    void *stream);
/* x_low_dev, x_dev [n_items][L][C], C = 1 or 2 -> out_dev float64 [n_items][C][T]: the sum over all n_fft / 2 + 1 bins of
 * |X_low_k| / (|X_k| + 1e-5) */
int mst_mixfeat_low_ratio(MstMixfeat *h, const float *x_low_dev, const float *x_dev, int n_items, long L, int C,
                          const float *scale_low_dev, const float *scale_dev, double *out_dev, void *stream);
/* The per-frame work of the reference's compute_spectral_features (:509-679: librosa.feature.spectral_centroid / _bandwidth / _rolloff /
 * _flatness / _contrast).  Since mst_version() 106.  x_dev [n_items][L][C], C = 1 or 2 -> out_dev float64 [n_items][C][T][16]; with S_k,
 * k = 0 .. n_fft / 2, the float32 magnitudes of a frame and P_k = max(1e-10, S_k^2), everything after them in float64:
 *   0  sum S_k        1  sum k S_k        2  sum S_k (k - c)^2, c = [1] / [0] (formed from the magnitudes, not from sum k^2 S_k)
 *   3  the first k whose cumulative sum S_0 + .. + S_k reaches 0.85 [0]        4  sum log P_k        5  sum P_k
 *   6 + 2 j, 7 + 2 j   the sum of the band_k[j] smallest and of the band_k[j] largest S_k with band_lo[j] <= k < band_hi[j]: exact
 *                      multiset sums, ties counted once (host arrays; n_bands 1 .. 5 - what 16 numbers hold -, bands non-empty and inside
 *                      0 .. n_fft / 2 + 1, 1 <= band_k[j] <= band_hi[j] - band_lo[j]; slots of bands beyond n_bands are not written)
 * All in bins: the caller turns them into Hz.  A frame of digital silence gives exactly 0 in every slot but 4 and 5. */
int mst_mixfeat_spectral(MstMixfeat *h, const float *x_dev, int n_items, long L, int C, const float *scale_dev, const int *band_lo,
                         const int *band_hi, const int *band_k, int n_bands, double *out_dev, void *stream);
/* x_dev [n_items][L][C], C = 1 or 2 -> out_dev float64 [n_items][C][T][3], T = 1 + (L - frame_length) / hop: per frame of frame_length
 * samples sum x^2, sum 20 log10(|x| + 1e-30) and max |x| (a zero sample adds -600 dB, as in get_rms_dynamic_crest) */
int mst_mixfeat_dynamics(const float *x_dev, int n_items, long L, int C, const float *scale_dev, int frame_length, int hop,
                         double *out_dev, void *stream);

/* ----------------------------------------------------------------------------------------------
 * Sample-rate conversion (csrc/resample_kernels.h): a rational polyphase FIR resampler over the FX layout, fp32 [n_items][L][C], C = 1 or
 * 2.  No reference counterpart: the reference's loaders raise for every rate but 44.1 kHz.  Since mst_version() 101.
 *   ratio   up / down = rate_out / rate_in reduced by their gcd; up <= 441 and down <= 640 (8, 11.025, 16, 22.05, 24, 32, 48, 88.2, 96,
 *           192 kHz -> 44.1 kHz, 44.1 -> 176.4 kHz), and a tile of 256 outputs may span at most 2304 input frames (down / up up to about
 *           6): anything else MST_ERR_UNSUPPORTED, the message names the ratio.  Equal rates: MST_ERR_ARG (skip the call).
 *   filter  half = 64 max(up, down), fc = 0.945 / max(up, down); h = up * scipy.signal.firwin(2 half + 1, fc, window = ('kaiser', 12.0)),
 *           designed in float64 on the host and rounded once to float32.
 *   sum     y[m] = sum_j h[m down - j up + half] x[j], x zero outside the signal: scipy.signal.resample_poly(padtype = 'constant'), output
 *           0 on input 0, no delay.  Every product is formed in float64 (exact), added in float64 in an order that depends on m alone, and
 *           the sum is rounded once to float32; no atomics: an item's bits are the same alone, in a batch, in chunks and in every run.
 * ---------------------------------------------------------------------------------------------- */
typedef struct MstResampler MstResampler;
int mst_resample_create(int rate_in, int rate_out, MstResampler **out);
int mst_resample_destroy(MstResampler *r);
/* any of the four pointers may be null; taps_per_phase = 2 half_len / up + 1 products per output */
int mst_resample_info(const MstResampler *r, int *up, int *down, int *half_len, int *taps_per_phase);
/* ceil(n_in * up / down): the outputs of a signal of n_in frames (negative: MstStatus) */
long mst_resample_length(const MstResampler *r, long n_in);
/* the 2 half_len + 1 float32 prototype taps h into taps_host; n must be that count */
int mst_resample_taps(const MstResampler *r, float *taps_host, int n);
/* x_dev [n_items][n_in][C] holds inputs in_start .. in_start + n_in - 1 of each item's signal, the call writes outputs out_start ..
 * out_start + n_out - 1 into y_dev [n_items][n_out][C]; inputs outside the buffer are zero.  in_start = out_start = 0 and
 * n_out = mst_resample_length(n_in): the whole signal.  Output m reads inputs (m down - half) / up .. (m down + half) / up: a chunk whose
 * buffer covers that range of its outputs gives the bits of the whole-signal call.  All positions are 64-bit (below 2^48); n_in and n_out
 * below 2^30 per call, at most 65535 items; y_dev of a stereo call 8-byte aligned. */
int mst_resample_forward(MstResampler *r, const float *x_dev, long n_in, long in_start, float *y_dev, long n_out, long out_start,
                         int n_items, int C, void *stream);

/* ----------------------------------------------------------------------------------------------
 * Training batches (csrc/batch_kernels.h; data_loader/data_loader.py: the MUSDB datasets).  Since mst_version() 108.  Two streaming launches
 * around the per-item FX calls: random segments cut out of a resident bank of PCM, and the finishing pass behind the chains.  The tables
 * are passed twice: *_dev is what the kernel reads, *_host the same values in host memory (pinned, on their way to the device), which
 * the call checks before it launches anything - a row out of range is MST_ERR_ARG, mst_last_error() names the first one; no device-side
 * trap.  At most 65535 rows per call.
 * ---------------------------------------------------------------------------------------------- */
/* bank_dev: n_bank_frames interleaved stereo frames of `width` (2 or 4) bytes per sample, many files back to back.  table [n] int64: the
 * first frame of row r (any frame: no alignment beyond one frame; rows may repeat or overlap), 0 <= table[r] and
 * table[r] + frames <= n_bank_frames.  out_dev float32 [n][frames][2] (8-byte aligned) = int / 2^(8 width - 1) in float64, rounded once to
 * float32: loader_utils.load_wav_device's arithmetic. */
int mst_batch_gather_pcm(const void *bank_dev, long n_bank_frames, int width, const long *table_dev, const long *table_host, int n,
                         long frames, float *out_dev, void *stream);
/* x_dev float32 [n][Lp][C], C = 1 or 2; rows / start int64 [m]: out_dev [m][C][len], out[r][c][t] = clamp(x[rows[r]][start[r] + t][c], -1, 1)
 * with torch.clamp's semantics (NaN stays NaN, -0.0 stays -0.0); 0 <= rows[r] < n, 0 <= start[r], start[r] + len <= Lp.  Not in place. */
int mst_batch_finish(const float *x_dev, int n, long Lp, int C, const long *rows_dev, const long *rows_host, const long *start_dev,
                     const long *start_host, int m, long len, float *out_dev, void *stream);

/* ----------------------------------------------------------------------------------------------
 * Contrastive and gain training losses (csrc/contrast_kernels.h; modules/loss.py: NT_Xent :24-71, RMSLoss :77-93, infoNCE :228-238), value
 * and gradient.  Since mst_version() 111.  a_dev [n_a, D] and b_dev [n_b, D] fp32 are the two views; every row is divided by
 * max(|row|, eps) (the norm summed in float64), S = rows . rows * inv_tau on the exact-fp32 MFMA in k order, and
 *   mode 0  NT-Xent over cat(a, b), N = n_a + n_b rows: loss = (1 / N) sum_i [-S_i,p(i) + log sum_{j != i} exp S_ij], p(i) = i +- N / 2;
 *   mode 1  infoNCE: S = A B^T * inv_tau, loss = mean cross-entropy of row i against label i, no masked diagonal.
 * Max subtraction, exp, log and every sum over a row or over the rows in float64 in a fixed order; no atomics: the same inputs give the
 * same bits in every run.  loss_dev is one float64.  fp32 operands only - there is no bf16 mode.
 * The forward-only call writes no G and runs no gradient kernel; it leaves S, the normalised rows and the norms in its workspace.  The
 * backward either takes that workspace back (ws_from_forward = 1: the SAME operands, sizes and mode, the buffer untouched since the forward
 * and handed over ONCE - the backward writes G over S) or recomputes S from a_dev and b_dev (ws_from_forward = 0: any workspace of the
 * size).  Both give the same bits.  G = (softmax - one-hot) * dloss / rows over S in place, dZh = (G + G^T) Zh * inv_tau (mode 1: dA = G B,
 * dB = G^T A) on the same MFMA, then each row through its normalisation.  dloss_dev is one float64 read on the device (no host synchronisation);
 * grad_a_dev [n_a, D] and grad_b_dev [n_b, D] are written, not accumulated.  A row whose norm is below eps has similarity 0 to everything
 * and gets a gradient of exact zeros.
 * Limits (MST_ERR_UNSUPPORTED, the message names the number): n_a == n_b, n_a + n_b <= 4096 (even in mode 0 by construction), D <= 8192.
 * The workspace holds S (N^2 fp32), the normalised rows (N D fp32) and 3 N scalars; with_grad asks no more (G overwrites S).
 * ---------------------------------------------------------------------------------------------- */
size_t mst_ntxent_workspace_bytes(int n_a, int n_b, int D, int with_grad);
int mst_ntxent_forward(const float *a_dev, const float *b_dev, int n_a, int n_b, int D, double inv_tau, double eps, int mode,
                       double *loss_dev, void *workspace, size_t workspace_bytes, void *stream);
int mst_ntxent_backward(const float *a_dev, const float *b_dev, int n_a, int n_b, int D, double inv_tau, double eps, int mode,
                        const double *dloss_dev, float *grad_a_dev, float *grad_b_dev, int ws_from_forward, void *workspace,
                        size_t workspace_bytes, void *stream);
/* RMSLoss: est_dev, tgt_dev fp32 [rows, T] (the reference's [B, C, T] with rows = B C).  Per row rms = sqrt(mean x^2) from a float64 sum of
 * squares in a fixed order; w = weight_factor * max(|rms_t - rms_e|, 1 / weight_factor); loss = mean_r(w^1.5) * mean_r((rms_e - rms_t)^2) -
 * nn.MSELoss(reduce=None) is the MEAN reduction.  loss_dev is one float64.  The backward recomputes the sums and writes
 * grad_est_dev[r, t] = c_r est[r, t], c_r formed on the device from the row sums and dloss_dev (one float64); a row of est without energy
 * gets exact zeros, and |rms_t - rms_e| < 1 / weight_factor passes no gradient through w (torch.clamp).  rows <= 65535, T < 2^30. */
size_t mst_rms_loss_workspace_bytes(int rows, long T);
int mst_rms_loss_forward(const float *est_dev, const float *tgt_dev, int rows, long T, double weight_factor, double *loss_dev,
                         void *workspace, size_t workspace_bytes, void *stream);
int mst_rms_loss_backward(const float *est_dev, const float *tgt_dev, int rows, long T, double weight_factor, const double *dloss_dev,
                          float *grad_est_dev, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MST_HIP_H */
