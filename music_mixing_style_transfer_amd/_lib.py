"""ctypes binding of libmst_hip.so (the C ABI declared in include/mst_hip.h).

The product path has NO fallback: if the HIP library is missing, import of anything that needs it raises.
(tests/ may bind the CPU emulator build of the same sources through `bind(path)`; the product never does.)
"""
import ctypes as C
import os

import torch  # noqa: F401  - MUST precede loading libmst_hip.so: the library has to share torch's HIP runtime
#                            (same libamdhip64 instance => same streams / device pointers); loading it first binds
#                            /opt/rocm's copy and every hipMalloc then fails with "no ROCm-capable device".

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libmst_hip.so")

MST_OK = 0
MST_PREC_F32 = 0
MST_PREC_BF16 = 1
MST_PREC_BF16X3 = 2
MST_MAX_BLOCKS = 32
TCN_TUNING_DEFAULT = 245    # mst_tcn_set_tuning flags a fresh handle starts with (include/mst_hip.h: bit 0 bf16x3 small tiles, bits 1-2 = 2 the bf16 class-major family with bit 4 required, bit 5 block 0 fused into block 1, bit 6 bf16x3 half-tile class-major loop, bit 7 bf16 whole-sequence tiles / class-major four-phase head; bit 3 is refused)
TCN_FUSION_DEFAULT = 1      # mst_tcn_set_fusion flags TCNModel sets on its handle (a raw mst_tcn_create handle starts with 0): bit 0 the last three blocks of a qualifying bf16 forward as one launch
TCN_CHUNK_DEFAULT = 0       # mst_tcn_set_chunk items TCNModel sets on its handle (a raw mst_tcn_create handle starts with TCN_CHUNK_WHOLE): 0 = a full bf16 forward whose one activation exceeds the Infinity Cache runs in chunks that fit it, on two streams
TCN_CHUNK_WHOLE = 0x7fffffff
PRECISIONS = {"fp32": MST_PREC_F32, "f32": MST_PREC_F32, "bf16": MST_PREC_BF16, "bf16x3": MST_PREC_BF16X3}

STATUS_NAMES = {0: "MST_OK", -1: "MST_ERR_ARG", -2: "MST_ERR_UNSUPPORTED", -3: "MST_ERR_HIP", -4: "MST_ERR_STATE",
                -5: "MST_ERR_WORKSPACE"}


class MstTcnDesc(C.Structure):
    _fields_ = [("nblocks", C.c_int), ("ninputs", C.c_int), ("noutputs", C.c_int), ("channels", C.c_int),
                ("kernel_size", C.c_int), ("cond_dim", C.c_int), ("dilations", C.c_int * MST_MAX_BLOCKS), ("causal", C.c_int)]


FX_FORM_EQ_LANE_APPLY, FX_FORM_EQ_VALU_ENDS, FX_FORM_COMP_SLICE_SMALL = 1, 2, 4          # MstFxFuse.forms (include/mst_hip.h)


class MstFxFuse(C.Structure):
    """include/mst_hip.h MstFxFuse; struct_size is filled in here (the library refuses a struct of another layout)."""
    _fields_ = [("struct_size", C.c_uint), ("forms", C.c_int), ("in_scale_dev", C.c_void_p), ("out_sumsq_dev", C.c_void_p),
                ("in_sumsq_dev", C.c_void_p), ("post_rms", C.c_int), ("post_gain", C.c_float), ("out_in_sumsq_dev", C.c_void_p),
                ("out_ms_dev", C.c_void_p), ("in_ms_dev", C.c_void_p)]

    def __init__(self, in_scale_dev=None, out_sumsq_dev=None, in_sumsq_dev=None, post_rms=0, post_gain=0.0, out_in_sumsq_dev=None,
                 out_ms_dev=None, in_ms_dev=None, forms=0):
        super().__init__(C.sizeof(MstFxFuse), forms, in_scale_dev, out_sumsq_dev, in_sumsq_dev, post_rms, post_gain, out_in_sumsq_dev,
                         out_ms_dev, in_ms_dev)


FX_COMP_SPLIT_SERIAL, FX_COMP_TIME_PARALLEL, FX_COMP_WAVE_SERIAL = 0, 1, 2      # MstFxCompressorPlan.form


class MstFxBiquadItemsPlan(C.Structure):
    """include/mst_hip.h MstFxBiquadItemsPlan (diagnostic; the layout may change with mst_version())."""
    _fields_ = [("struct_size", C.c_uint), ("M", C.c_int), ("tables_offset", C.c_size_t), ("item_stride", C.c_size_t), ("powers_offset", C.c_size_t),
                ("coef_offset", C.c_size_t), ("total_bytes", C.c_size_t)]

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.struct_size = C.sizeof(MstFxBiquadItemsPlan)


class MstFxBiquadPlan(C.Structure):
    """include/mst_hip.h MstFxBiquadPlan (diagnostic; the layout may change with mst_version())."""
    _fields_ = [("struct_size", C.c_uint), ("time_parallel", C.c_int), ("M", C.c_int), ("scan_threads", C.c_int), ("record_doubles", C.c_int),
                ("nchunks", C.c_long), ("ends_offset", C.c_size_t), ("starts_offset", C.c_size_t)]

    def __init__(self):
        super().__init__(C.sizeof(MstFxBiquadPlan))


class MstFxCompressorPlan(C.Structure):
    """include/mst_hip.h MstFxCompressorPlan (diagnostic; the layout may change with mst_version())."""
    _fields_ = [("struct_size", C.c_uint), ("form", C.c_int), ("nslices", C.c_int), ("record_doubles", C.c_int), ("nchunks", C.c_long),
                ("nbatch", C.c_long), ("ntiles", C.c_long), ("kappa", C.c_double), ("kappa_limit", C.c_double), ("xl_offset", C.c_size_t),
                ("maps_offset", C.c_size_t), ("ystart_offset", C.c_size_t), ("tab_offset", C.c_size_t), ("carry_offset", C.c_size_t),
                ("tsums_offset", C.c_size_t), ("total_bytes", C.c_size_t)]

    def __init__(self):
        super().__init__(C.sizeof(MstFxCompressorPlan))


class MstEncDesc(C.Structure):
    _fields_ = [("nblocks", C.c_int), ("channels", C.c_int * (MST_MAX_BLOCKS + 1)), ("kernels", C.c_int * MST_MAX_BLOCKS),
                ("strides", C.c_int * MST_MAX_BLOCKS), ("dilations", C.c_int * MST_MAX_BLOCKS), ("valid_padding", C.c_int), ("act_slope", C.c_float)]


MST_MSS_MAX_SCALES = 8
MSS_MODES = {"midside": 0, "ori": 1}          # MST_MSS_MIDSIDE / MST_MSS_ORI
MSS_WINDOWS = {"hann": 0, "hamming": 1}       # MST_MSS_HANN / MST_MSS_HAMMING


class MstMssDesc(C.Structure):
    """include/mst_hip.h MstMssDesc; struct_size is filled in here (the library refuses a struct of another layout)."""
    _fields_ = [("struct_size", C.c_uint), ("mode", C.c_int), ("n_scales", C.c_int), ("n_fft", C.c_int * MST_MSS_MAX_SCALES),
                ("hop", C.c_int * MST_MSS_MAX_SCALES), ("win_length", C.c_int * MST_MSS_MAX_SCALES), ("window", C.c_int),
                ("eps", C.c_double)]

    def __init__(self, mode=0, n_fft=(), hop=(), win_length=(), window=0, eps=1e-7):
        super().__init__()
        self.struct_size, self.mode, self.n_scales, self.window, self.eps = C.sizeof(MstMssDesc), mode, len(n_fft), window, eps
        for i in range(min(len(n_fft), MST_MSS_MAX_SCALES)):
            self.n_fft[i], self.hop[i], self.win_length[i] = n_fft[i], hop[i], win_length[i]


_P = C.c_void_p
_F = C.c_void_p   # float* passed as integer addresses (tensor.data_ptr())

# name -> (restype, argtypes); kept in sync with include/mst_hip.h (tests/test_abi.py checks the export list)
SIGNATURES = {
    "mst_version": (C.c_int, []),
    "mst_last_error": (C.c_char_p, []),
    "mst_tcn_create": (C.c_int, [C.POINTER(MstTcnDesc), C.POINTER(_P)]),
    "mst_tcn_destroy": (C.c_int, [_P]),
    "mst_tcn_load_block": (C.c_int, [_P, C.c_int, _F, _F, _F, _F, _F, C.c_float, _F, _F, _F, _P]),
    "mst_tcn_load_output": (C.c_int, [_P, _F, _F, _P]),
    "mst_tcn_set_cond": (C.c_int, [_P, _F, C.c_int, C.c_long, _P]),
    "mst_tcn_workspace_bytes": (C.c_size_t, [_P, C.c_int, C.c_int, C.c_int]),
    "mst_tcn_forward": (C.c_int, [_P, _F, _F, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "mst_tcn_forward_blocks": (C.c_int, [_P, _F, _F, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "mst_tcn_set_tuning": (C.c_int, [_P, C.c_int]),
    "mst_tcn_get_tuning": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mst_tcn_set_fusion": (C.c_int, [_P, C.c_int]),
    "mst_tcn_get_fusion": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mst_tcn_set_chunk": (C.c_int, [_P, C.c_int]),
    "mst_tcn_get_chunk": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mst_tcn_context": (C.c_int, [_P, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "mst_tcn_timing_begin": (C.c_int, [_P, C.c_int]),
    "mst_tcn_timing_end": (C.c_int, [_P, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
    "mst_calib_mainloop": (C.c_int, [C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float), _P]),
    "mst_enc_create": (C.c_int, [C.POINTER(MstEncDesc), C.POINTER(_P)]),
    "mst_enc_destroy": (C.c_int, [_P]),
    "mst_enc_load_conv": (C.c_int, [_P, C.c_int, C.c_int, _F, _F, _F, _F, _F, _F, C.c_float, _P]),
    "mst_enc_set_tuning": (C.c_int, [_P, C.c_long]),
    "mst_enc_set_schedule": (C.c_int, [_P, C.c_int]),
    "mst_global_avgpool": (C.c_int, [_F, _F, C.c_long, C.c_int, _P]),
    "mst_enc_zero_stuff": (C.c_int, [_F, _F, C.c_long, C.c_long, C.c_int, C.c_long, C.c_long, _P]),
    "mst_enc_workspace_bytes": (C.c_size_t, [_P, C.c_int, C.c_int]),
    "mst_enc_forward": (C.c_int, [_P, _F, _F, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "mst_enc_forward_blocks": (C.c_int, [_P, _F, _F, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    "mst_enc_block_length": (C.c_int, [_P, C.c_int, C.c_int]),
    "mst_enc_conv_length": (C.c_int, [_P, C.c_int, C.c_int, C.c_int]),
    "mst_enc_forward_conv": (C.c_int, [_P, C.c_int, C.c_int, _F, _F, C.c_int, C.c_int, _P]),
    "mst_film_forward": (C.c_int, [_F, _F, _F, C.c_int, C.c_int, C.c_int, _F, _F, C.c_int, C.c_long, _F, _P]),
    "mst_embedding_mean": (C.c_int, [_F, C.c_int, C.c_int, _F, _P]),
    "mst_fx_biquad_scratch_bytes": (C.c_size_t, [C.c_int, C.c_long, C.c_int, C.c_int]),
    "mst_fx_biquad_plan": (C.c_int, [C.c_int, C.c_long, C.c_int, C.c_int, C.POINTER(MstFxBiquadPlan)]),
    "mst_fx_biquad_tables": (C.c_int, [C.POINTER(C.c_double), C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "mst_fx_compressor_plan": (C.c_int, [C.c_int, C.c_long, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.POINTER(MstFxCompressorPlan)]),
    "mst_fx_biquad_cascade": (C.c_int, [_F, _F, C.c_int, C.c_long, C.c_int, C.POINTER(C.c_double), C.c_int, _P, C.c_size_t, _P, _P]),
    "mst_fx_biquad_items_scratch_bytes": (C.c_size_t, [C.c_int, C.c_long, C.c_int, C.c_int]),
    "mst_fx_biquad_items_plan": (C.c_int, [C.c_int, C.c_long, C.c_int, C.c_int, C.POINTER(MstFxBiquadItemsPlan)]),
    "mst_fx_biquad_cascade_items": (C.c_int, [_F, _F, C.c_int, C.c_long, C.c_int, _P, C.c_int, _P, C.c_size_t, _P, _P]),
    "mst_fx_compressor_items_table_bytes": (C.c_size_t, [C.c_int]),
    "mst_fx_compressor_items_prepare": (C.c_int, [_P, C.c_int, C.c_long, C.c_int, C.c_double, C.c_int, _P, C.c_size_t, C.POINTER(C.c_int)]),
    "mst_fx_compressor_items": (C.c_int, [_F, _F, C.c_int, C.c_long, C.c_int, _P, _P, C.c_size_t, _P, _P]),
    "mst_fx_midside_imager_items": (C.c_int, [_F, _F, C.c_int, C.c_long, _P, _P, _P, _P, _P]),
    "mst_fx_gain_items": (C.c_int, [_F, _F, C.c_int, C.c_long, C.c_int, _P, _P, _P, _P]),
    "mst_fx_sumsq": (C.c_int, [_F, C.c_int, C.c_long, _P, _P]),
    "mst_fx_rms_pending": (C.c_int, [_P, _P, C.c_long, _P, C.c_long, _P, C.c_int, _P]),
    "mst_fx_scale_items": (C.c_int, [_F, _F, C.c_int, C.c_long, _P, _P]),
    "mst_fx_compressor_scratch_bytes": (C.c_size_t, [C.c_int, C.c_long, C.c_int]),
    "mst_fx_compressor": (C.c_int, [_F, _F, C.c_int, C.c_long, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double,
                                    C.c_double, _P, C.c_size_t, _P, _P]),
    "mst_fx_midside_imager": (C.c_int, [_F, _F, C.c_int, C.c_long, C.c_double, _P, _P, _P]),
    "mst_fx_gain": (C.c_int, [_F, _F, C.c_int, C.c_long, C.c_int, C.c_double, C.c_int, _P, _P]),
    "mst_fx_haas": (C.c_int, [_F, _F, C.c_int, C.c_long, C.c_int, C.c_long, C.c_double, C.c_int, _P]),
    "mst_fx_panner": (C.c_int, [_F, _F, C.c_int, C.c_long, C.c_int, C.c_float, C.c_float, _P]),
    "mst_fx_rms_normalize": (C.c_int, [_F, _F, C.c_int, C.c_long, C.c_long, _P, _P]),
    "mst_fx_convolver_create": (C.c_int, [C.c_long, C.c_long, C.c_int, C.c_int, C.POINTER(_P)]),
    "mst_fx_convolver_destroy": (None, [_P]),
    "mst_fx_convolver_workspace_bytes": (C.c_size_t, [_P]),
    "mst_fx_compressor_grid": (C.c_int, [_F, _F, C.c_int, C.c_long, C.c_int, _F, _F, C.c_double, C.c_double, C.c_double, _P, C.c_size_t,
                                         _P, _P]),
    "mst_fx_range_reduce": (C.c_int, [_F, C.c_long, C.c_int, C.c_int, _P, _P, _P, C.c_int, C.c_int, _P, _P]),
    "mst_fx_onset_hfc": (C.c_int, [_F, C.c_int, C.c_long, C.c_int, C.c_int, C.c_int, _F, _P]),
    "mst_fx_stft_create": (C.c_int, [C.c_long, C.c_long, C.POINTER(C.c_float), C.c_int, C.POINTER(_P)]),
    "mst_fx_stft_destroy": (None, [_P]),
    "mst_fx_stft_workspace_bytes": (C.c_size_t, [_P]),
    "mst_fx_stft_mean_magnitude": (C.c_int, [_P, _F, C.c_long, C.c_int, C.c_int, _F, _P, C.c_size_t, _P]),
    "mst_fx_algorithmic_reverb_scratch_bytes": (C.c_size_t, [C.c_int, C.c_long, C.c_int]),
    "mst_fx_algorithmic_reverb": (C.c_int, [_F, _F, C.c_int, C.c_long, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.c_int,
                                            C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _P, C.c_size_t, _P]),
    "mst_fx_stereo_moments": (C.c_int, [_F, C.c_int, C.c_long, _P, _P]),
    "mst_fx_stereo_mix": (C.c_int, [_F, _F, C.c_int, C.c_long, C.c_float, C.c_float, C.c_float, C.c_float, _P]),
    "mst_mss_create": (C.c_int, [C.POINTER(MstMssDesc), C.POINTER(_P)]),
    "mst_mss_destroy": (C.c_int, [_P]),
    "mst_mss_frames": (C.c_int, [_P, C.c_int, C.c_long]),
    "mst_mss_workspace_bytes": (C.c_size_t, [_P, C.c_int, C.c_long]),
    "mst_mss_forward": (C.c_int, [_P, _F, _F, C.c_int, C.c_long, _P, _P, C.c_size_t, _P]),
    "mst_mss_spectrogram": (C.c_int, [_P, C.c_int, _F, C.c_int, C.c_int, C.c_long, _F, _P]),
    "mst_mss_backward_workspace_bytes": (C.c_size_t, [_P, C.c_int, C.c_long]),
    "mst_mss_backward": (C.c_int, [_P, _F, _F, C.c_int, C.c_long, _P, _F, _P, C.c_size_t, _P]),
    "mst_mixfeat_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(_P)]),
    "mst_mixfeat_destroy": (C.c_int, [_P]),
    "mst_mixfeat_frames": (C.c_int, [_P, C.c_long]),
    "mst_mixfeat_panning": (C.c_int, [_P, _F, C.c_int, C.c_long, _F, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, _P, _P]),
    "mst_mixfeat_sps": (C.c_int, [_P, _F, C.c_int, C.c_long, _F, _F, _F, _P]),
    "mst_mixfeat_low_ratio": (C.c_int, [_P, _F, _F, C.c_int, C.c_long, C.c_int, _F, _F, _P, _P]),
    "mst_mixfeat_spectral": (C.c_int, [_P, _F, C.c_int, C.c_long, C.c_int, _F, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int,
                             _P, _P]),
    "mst_mixfeat_dynamics": (C.c_int, [_F, C.c_int, C.c_long, C.c_int, _F, C.c_int, C.c_int, _P, _P]),
    "mst_resample_create": (C.c_int, [C.c_int, C.c_int, C.POINTER(_P)]),
    "mst_resample_destroy": (C.c_int, [_P]),
    "mst_resample_info": (C.c_int, [_P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mst_resample_length": (C.c_long, [_P, C.c_long]),
    "mst_resample_taps": (C.c_int, [_P, C.POINTER(C.c_float), C.c_int]),
    "mst_resample_forward": (C.c_int, [_P, _F, C.c_long, C.c_long, _F, C.c_long, C.c_long, C.c_int, C.c_int, _P]),
    "mst_fx_panner_items": (C.c_int, [_F, _F, C.c_int, C.c_long, C.c_int, _P, _P]),
    "mst_fx_haas_items": (C.c_int, [_F, _F, C.c_int, C.c_long, C.c_int, _P, _P, _P, _P]),
    "mst_fx_convolver_items_workspace_bytes": (C.c_size_t, [_P, C.c_int]),
    "mst_fx_convolve_items_table_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "mst_fx_convolve_items_prepare": (C.c_int, [_P, _P, _P, C.c_int, C.c_long, _P, C.c_int, _P, C.c_size_t, C.POINTER(C.c_int)]),
    "mst_fx_convolve_items": (C.c_int, [_P, _F, _F, _P, C.c_int, C.c_int, _F, _P, C.c_size_t, _P]),
    "mst_fx_algorithmic_reverb_items": (C.c_int, [_F, _F, C.c_int, C.c_long, C.c_int, C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_int), C.c_int,
                                                  C.c_int, C.c_double, _P, _P, C.c_size_t, _P]),
    "mst_fx_convolve": (C.c_int, [_P, _F, _F, C.c_long, _F, C.c_long, C.c_double, C.c_double, _P, C.c_size_t, _P]),
    "mst_batch_gather_pcm": (C.c_int, [_P, C.c_long, C.c_int, _P, _P, C.c_int, C.c_long, _F, _P]),
    "mst_batch_finish": (C.c_int, [_F, C.c_int, C.c_long, C.c_int, _P, _P, _P, _P, C.c_int, C.c_long, _F, _P]),
    "mst_ntxent_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mst_ntxent_forward": (C.c_int, [_F, _F, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, _P, _P, C.c_size_t, _P]),
    "mst_ntxent_backward": (C.c_int, [_F, _F, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, _P, _F, _F, C.c_int, _P, C.c_size_t, _P]),
    "mst_rms_loss_workspace_bytes": (C.c_size_t, [C.c_int, C.c_long]),
    "mst_rms_loss_forward": (C.c_int, [_F, _F, C.c_int, C.c_long, C.c_double, _P, _P, C.c_size_t, _P]),
    "mst_rms_loss_backward": (C.c_int, [_F, _F, C.c_int, C.c_long, C.c_double, _P, _F, _P, C.c_size_t, _P]),
}


class MstError(RuntimeError):
    pass


class Binding:
    """A loaded library with typed entry points and status checking."""

    def __init__(self, path):
        if not os.path.exists(path):
            raise ImportError(
                f"{path} not found: the HIP extension has not been built (python -c 'import __graft_entry__ as g; "
                f"g.build()' or make -C music_mixing_style_transfer_amd/csrc).  There is no CPU fallback.")
        self.path = path
        self.cdll = C.CDLL(path)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(self.cdll, name)   # AttributeError if the symbol is missing: fail loudly
            fn.restype = res
            fn.argtypes = args
            setattr(self, name, fn)

    def require_device(self, t, what):
        """The kernels run on the MI355X only: a tensor that is not in HBM is an error (there is no CPU path)."""
        if not t.is_cuda:
            raise RuntimeError(f"{what}: input must live on the MI355X (a CUDA/HIP tensor); there is no CPU path")

    def to_device(self, t):
        """Host arrays handed to a processor travel to the MI355X (numpy in -> numpy out at that boundary)."""
        if t.is_cuda:
            return t
        if not torch.cuda.is_available():
            raise RuntimeError("the kernels run on the MI355X only; no GPU is visible and there is no CPU path")
        return t.cuda()

    def stream_ptr(self, t):
        """The caller's current HIP stream for tensor t's device (what every entry point takes as `stream`)."""
        return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)

    def device_ctx(self, t):
        """Context that makes t's device the current HIP device: handles, weights and the FiLM table are allocated on,
        and kernels launched on, the device the data lives on (not whatever device happens to be current)."""
        return torch.cuda.device(t.device)

    def check(self, status, what=""):
        if status != MST_OK:
            msg = self.mst_last_error()
            msg = msg.decode() if msg else ""
            code = STATUS_NAMES.get(status, str(status))
            if status == -2:
                raise NotImplementedError(f"{what}: {code}: {msg}")
            if status == -1:
                raise ValueError(f"{what}: {code}: {msg}")
            raise MstError(f"{what}: {code}: {msg}")


def bind(path):
    return Binding(path)


_default = None


def lib():
    """The product binding (libmst_hip.so), loaded on first use."""
    global _default
    if _default is None:
        _default = Binding(LIB_PATH)
    return _default


def set_default_binding(binding):
    """TEST HOOK: route the module API through another build of the same C ABI (the CPU SIMT emulator)."""
    global _default
    _default = binding
