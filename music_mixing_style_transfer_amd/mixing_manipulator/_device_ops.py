"""Device calls under the input normaliser: thin typed wrappers over the C ABI (include/mst_hip.h) working on torch device
tensors.  Host-side control flow lives in fx_utils.py / utils_data_normalization.py / normalization_imager.py."""
import contextlib
import ctypes as C

import numpy as np
import torch

from .. import _lib


def to_device(x):
    """numpy / torch [L] or [L, C] float -> contiguous float32 device tensor [L, C]."""
    b = _lib.lib()
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)) if isinstance(x, np.ndarray) else x.to(torch.float32)
    if t.dim() == 1:
        t = t[:, None]
    return b.to_device(t).contiguous()


def _i64(values, device):
    return torch.from_numpy(np.asarray(values, dtype=np.int64)).to(device)


class RangeIndex:
    """(item, lo, hi) arrays of a set of ranges, uploaded once per device: pass it as `items` of range_reduce (with the same lo / hi lists)
    when the same ranges are reduced again and again - the BS.1770 gating blocks of a stem are measured four times per normalisation."""

    def __init__(self, items, lo, hi):
        self.items, self.lo, self.hi = np.asarray(items, dtype=np.int32), np.asarray(lo, dtype=np.int64), np.asarray(hi, dtype=np.int64)
        self._dev = {}

    def on(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = tuple(torch.from_numpy(a).to(device) for a in (self.items, self.lo, self.hi))
        return self._dev[key]


def biquad(x, b, a):
    """One second-order section over the whole signal from zero state (scipy.signal.lfilter recursion, float64 inside,
    float32 result): x device [L, C]."""
    lib = _lib.lib()
    coef = np.ascontiguousarray([[b[0], b[1], b[2], a[0], a[1], a[2]]], dtype=np.float64)
    L, Cn = x.shape
    y = torch.empty_like(x)
    with lib.device_ctx(x):
        nbytes = lib.mst_fx_biquad_scratch_bytes(1, L, Cn, 1)
        sc = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=x.device)
        lib.check(lib.mst_fx_biquad_cascade(x.data_ptr(), y.data_ptr(), 1, L, Cn, coef.ctypes.data_as(C.POINTER(C.c_double)), 1,
                                            sc.data_ptr(), nbytes, None, lib.stream_ptr(x)), "mst_fx_biquad_cascade")
    return y


_MAX_SPLIT = 1 << 15      # samples per workgroup of a max-reduction (fx_range_reduce_kernel runs ONE workgroup per range)


def range_reduce(x, items, lo, hi, channel=0, mode="sumsq"):
    """x device [n, L, C] (or [L, C]); float64 numpy [n_ranges]: sum of squares / max |x| over x[items[r], lo[r]:hi[r], channel].
    A max over a long range (the peak of a whole stem: 16 M samples on one workgroup took 17 ms) is cut into pieces of 2^15 samples
    that run as separate ranges and are combined on the host - a maximum does not depend on the order, the result is the same bits."""
    lib = _lib.lib()
    if x.dim() == 2:
        x = x[None]
    n, L, Cn = x.shape
    r = len(lo)
    if r == 0:
        return np.zeros(0)
    owner = None
    if mode != "sumsq" and not isinstance(items, RangeIndex) and any(min(int(b), L) - max(int(a), 0) > _MAX_SPLIT for a, b in zip(lo, hi)):
        items2, lo2, hi2, owner = [], [], [], []
        for k, (it, a, b) in enumerate(zip(items, lo, hi)):
            a, b = max(int(a), 0), min(int(b), L)
            starts = range(a, b, _MAX_SPLIT) if b > a else [a]
            for s0 in starts:
                items2.append(it)
                lo2.append(s0)
                hi2.append(min(b, s0 + _MAX_SPLIT))
                owner.append(k)
        items, lo, hi = items2, lo2, hi2
    dev = x.device
    if isinstance(items, RangeIndex):          # index arrays that already live on the device (the loudness meter's gating blocks)
        it, lo_t, hi_t = items.on(dev)
    else:
        it = torch.from_numpy(np.asarray(items, dtype=np.int32)).to(dev)
        lo_t, hi_t = _i64(lo, dev), _i64(hi, dev)
    out = torch.empty(len(lo), dtype=torch.float64, device=dev)
    with lib.device_ctx(x):
        lib.check(lib.mst_fx_range_reduce(x.data_ptr(), L, Cn, channel, it.data_ptr(), lo_t.data_ptr(), hi_t.data_ptr(), len(lo),
                                          0 if mode == "sumsq" else 1, out.data_ptr(), lib.stream_ptr(x)), "mst_fx_range_reduce")
    res = out.cpu().numpy()
    if owner is None:
        return res
    full = np.zeros(r)
    np.maximum.at(full, np.asarray(owner), res)
    return full


class StftMeanMagnitude:
    """Mean |STFT| over frames (librosa.stft(center=False) framing), one channel at a time."""

    def __init__(self, n_fft, hop, window, max_batch=64):
        self.lib = _lib.lib()
        self.n_fft, self.hop = int(n_fft), int(hop)
        win = np.ascontiguousarray(window, dtype=np.float32)
        h = C.c_void_p()
        self.lib.check(self.lib.mst_fx_stft_create(self.n_fft, self.hop, win.ctypes.data_as(C.POINTER(C.c_float)), max_batch, C.byref(h)),
                       "mst_fx_stft_create")
        self.handle = h
        self.ws = None

    def __call__(self, x, channel=0):
        lib = self.lib
        L, Cn = x.shape
        with lib.device_ctx(x):
            nbytes = lib.mst_fx_stft_workspace_bytes(self.handle)
            if self.ws is None or self.ws.numel() < nbytes or self.ws.device != x.device:
                self.ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
            out = torch.empty(self.n_fft // 2 + 1, dtype=torch.float32, device=x.device)
            lib.check(lib.mst_fx_stft_mean_magnitude(self.handle, x.data_ptr(), L, Cn, channel, out.data_ptr(), self.ws.data_ptr(), nbytes,
                                                     lib.stream_ptr(x)), "mst_fx_stft_mean_magnitude")
        return out.cpu().numpy()

    def __del__(self):
        try:
            self.lib.mst_fx_stft_destroy(self.handle)
        except Exception:
            pass


_convolvers = {}


def fir_causal(x, taps):
    """y[n] = sum_k taps[k] * x[n - k] with x[m < 0] := x[0] (an FIR started from the steady state of its first sample, what
    scipy.signal.lfilter(b, 1, x, zi=lfilter_zi(b, 1) * x[0]) computes): x device [L, 1] -> [L, 1].  FFT convolution."""
    lib = _lib.lib()
    nt = len(taps)
    L = x.shape[0]
    xe = torch.cat((x[:1].expand(nt - 1, 1), x), 0).contiguous()
    Le = xe.shape[0]
    h = torch.from_numpy(np.ascontiguousarray(taps, dtype=np.float32)[:, None])
    h = lib.to_device(h).to(x.device)
    key = (lib.path, Le, nt, str(x.device))
    with lib.device_ctx(x):
        cv = _convolvers.get(key)
        if cv is None:
            if len(_convolvers) > 4:
                for old in list(_convolvers.values()):
                    lib.mst_fx_convolver_destroy(old)
                _convolvers.clear()
            hdl = C.c_void_p()
            lib.check(lib.mst_fx_convolver_create(Le, nt, 1, 1, C.byref(hdl)), "mst_fx_convolver_create")
            cv = _convolvers[key] = hdl
        nbytes = lib.mst_fx_convolver_workspace_bytes(cv)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        y = torch.empty_like(xe)
        lib.check(lib.mst_fx_convolve(cv, xe.data_ptr(), h.data_ptr(), nt, y.data_ptr(), nt - 1, 0.0, 1.0, ws.data_ptr(), nbytes,
                                      lib.stream_ptr(x)), "mst_fx_convolve")
    return y[:L]


def compressor_grid(x, thresholds, ratios, attack_ms, release_ms, sample_rate, clip=True):
    """All (threshold, ratio) candidates on ONE signal: x device [L, C] -> device [n, L, C]."""
    lib = _lib.lib()
    n = len(thresholds)
    L, Cn = x.shape
    dev = x.device
    th = torch.tensor(thresholds, dtype=torch.float64, device=dev)
    ra = torch.tensor(ratios, dtype=torch.float64, device=dev)
    y = torch.empty(n, L, Cn, dtype=torch.float32, device=dev)
    with lib.device_ctx(x):
        plan = _lib.MstFxCompressorPlan()
        lib.check(lib.mst_fx_compressor_plan(n, L, Cn, float(attack_ms), float(release_ms), float(sample_rate), 0, C.byref(plan)),
                  "mst_fx_compressor_plan")
        if plan.form == _lib.FX_COMP_WAVE_SERIAL:
            # attack / release beyond the time-parallel smoother's conditioning limit: the grid launch is refused there; every candidate
            # runs as a plain serial call on the shared signal (rare: far outside the normaliser's own settings)
            xc = x.contiguous()
            for i, (t_db, r) in enumerate(zip(thresholds, ratios)):
                t_db = 1.0 if float(r) == 1.0 else float(t_db)      # ratio 1 never reads the threshold; (0 dB, 1) would mean "bypass" to mst_fx_compressor
                lib.check(lib.mst_fx_compressor(xc.data_ptr(), y[i].data_ptr(), 1, L, Cn, t_db, float(attack_ms), float(release_ms), float(r),
                                                float(sample_rate), None, 0, None, lib.stream_ptr(x)), "mst_fx_compressor")
                if clip and float(peaks(y[i:i + 1])[0]) >= 1.0:
                    y[i].clamp_(-1.0, 1.0)
            return y
        nbytes = lib.mst_fx_compressor_scratch_bytes(n, L, Cn)
        sc = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        pk = torch.empty(n * 64, dtype=torch.float64, device=dev) if clip else None
        lib.check(lib.mst_fx_compressor_grid(x.data_ptr(), y.data_ptr(), n, L, Cn, th.data_ptr(), ra.data_ptr(), float(attack_ms),
                                             float(release_ms), float(sample_rate), sc.data_ptr(), nbytes,
                                             pk.data_ptr() if clip else None, lib.stream_ptr(x)), "mst_fx_compressor_grid")
    return y


def onset_hfc(x, win, channel=0):
    """x device [n, L, C] -> numpy float32 [n, L // win, 2]: (hfc, mean square) of every whole frame of `win` samples."""
    lib = _lib.lib()
    if x.dim() == 2:
        x = x[None]
    n, L, Cn = x.shape
    nf = L // win
    out = torch.zeros(n, nf, 2, dtype=torch.float32, device=x.device)
    if nf:
        with lib.device_ctx(x):
            lib.check(lib.mst_fx_onset_hfc(x.data_ptr(), n, L, Cn, channel, win, out.data_ptr(), lib.stream_ptr(x)), "mst_fx_onset_hfc")
    return out.cpu().numpy()


# ---------------------------------------------------------------------------------------- mixing-feature metrics (csrc/mixfeat_kernels.h)
def _batch(x):
    """device [L, C] or [n, L, C] float32 -> contiguous [n, L, C]"""
    return (x[None] if x.dim() == 2 else x).contiguous()


def peaks(x):
    """x device [n, L, C] -> float64 numpy [n]: max |x| of every item over all its channels (mst_fx_range_reduce)."""
    n, L, Cn = x.shape
    out = np.zeros(n)
    for c in range(Cn):
        out = np.maximum(out, range_reduce(x, list(range(n)), [0] * n, [L] * n, channel=c, mode="max"))
    return out


def _scale_ptr(scale, n, device):
    """per-item load factor: None, or n float32 values -> (tensor kept alive, pointer)"""
    if scale is None:
        return None, None
    t = torch.from_numpy(np.ascontiguousarray(scale, dtype=np.float32).reshape(n)).to(device)
    return t, t.data_ptr()


class MixFeat:
    """The framed mixing-feature kernels at one (n_fft, hop): band sums of SPS^2, phi / SPS per bin, the low-frequency ratio."""
    _cache = {}

    @classmethod
    def get(cls, n_fft, hop):
        lib = _lib.lib()
        key = (lib.path, int(n_fft), int(hop))
        if key not in cls._cache:
            if len(cls._cache) > 8:
                cls._cache.clear()
            cls._cache[key] = cls(lib, n_fft, hop)
        return cls._cache[key]

    def __init__(self, lib, n_fft, hop):
        self.lib, self.n_fft, self.hop = lib, int(n_fft), int(hop)
        self._handles = {}

    def _handle(self, x):
        key = str(x.device)
        if key not in self._handles:
            h = C.c_void_p()
            with self.lib.device_ctx(x):
                self.lib.check(self.lib.mst_mixfeat_create(self.n_fft, self.hop, C.byref(h)), "mst_mixfeat_create")
            self._handles[key] = h
        return self._handles[key]

    def frames(self, L):
        return max(0, 1 + (L - self.n_fft) // self.hop) if L >= self.n_fft else 0

    def _stereo(self, x, what):
        self.lib.require_device(x, what)
        x = _batch(x)
        if x.dtype != torch.float32 or x.shape[2] != 2:
            raise ValueError(f"{what}: float32 [L, 2] or [n, L, 2] expected, got {x.dtype} {tuple(x.shape)}")
        return x

    def panning(self, x, bands, scale=None):
        """x device [n, L, 2]; bands [(lo, hi)] in bins -> float64 numpy [n, T, n_bands]: sum of SPS^2 over each band, per frame"""
        lib = self.lib
        x = self._stereo(x, "mst_mixfeat_panning")
        n, L, _ = x.shape
        lo = (C.c_int * len(bands))(*[int(b[0]) for b in bands])
        hi = (C.c_int * len(bands))(*[int(b[1]) for b in bands])
        keep, sp = _scale_ptr(scale, n, x.device)
        with lib.device_ctx(x):
            out = torch.empty(n, self.frames(L), len(bands), dtype=torch.float64, device=x.device)
            lib.check(lib.mst_mixfeat_panning(self._handle(x), x.data_ptr(), n, L, sp, lo, hi, len(bands), out.data_ptr(), lib.stream_ptr(x)),
                      "mst_mixfeat_panning")
        return out.cpu().numpy()

    def sps(self, x, scale=None):
        """x device [n, L, 2] -> (phi, SPS) device float32 [n, T, n_fft / 2 + 1]"""
        lib = self.lib
        x = self._stereo(x, "mst_mixfeat_sps")
        n, L, _ = x.shape
        keep, sp = _scale_ptr(scale, n, x.device)
        with lib.device_ctx(x):
            phi = torch.empty(n, self.frames(L), self.n_fft // 2 + 1, dtype=torch.float32, device=x.device)
            sps = torch.empty_like(phi)
            lib.check(lib.mst_mixfeat_sps(self._handle(x), x.data_ptr(), n, L, sp, phi.data_ptr(), sps.data_ptr(), lib.stream_ptr(x)),
                      "mst_mixfeat_sps")
        return phi, sps

    def low_ratio(self, x_low, x, scale_low=None, scale=None):
        """x_low, x device [n, L, C] -> float64 numpy [n, C, T]: sum over the bins of |X_low| / (|X| + 1e-5), per channel and frame"""
        lib = self.lib
        lib.require_device(x, "mst_mixfeat_low_ratio")
        x_low, x = _batch(x_low), _batch(x)
        if x.dtype != torch.float32 or x_low.dtype != torch.float32 or x.shape != x_low.shape:
            raise ValueError(f"mst_mixfeat_low_ratio: two float32 tensors of one shape expected, got {tuple(x_low.shape)} and {tuple(x.shape)}")
        n, L, Cn = x.shape
        keep_a, sa = _scale_ptr(scale_low, n, x.device)
        keep_b, sb = _scale_ptr(scale, n, x.device)
        with lib.device_ctx(x):
            out = torch.empty(n, Cn, self.frames(L), dtype=torch.float64, device=x.device)
            lib.check(lib.mst_mixfeat_low_ratio(self._handle(x), x_low.data_ptr(), x.data_ptr(), n, L, Cn, sa, sb, out.data_ptr(),
                                                lib.stream_ptr(x)), "mst_mixfeat_low_ratio")
        return out.cpu().numpy()

    def spectral(self, x, bands, scale=None):
        """x device [n, L, C], C = 1 or 2; bands [(lo, hi, k)] in bins -> float64 numpy [n, C, T, 16] per frame: sum S, sum k S,
        sum S (k - c)^2, the roll-off bin, sum log P, sum P, then per band the sum of its k smallest and of its k largest magnitudes
        (include/mst_hip.h, mst_mixfeat_spectral; slots of bands that were not asked for are 0)"""
        lib = self.lib
        lib.require_device(x, "mst_mixfeat_spectral")
        x = _batch(x)
        if x.dtype != torch.float32:
            raise ValueError(f"mst_mixfeat_spectral: float32 expected, got {x.dtype}")
        n, L, Cn = x.shape
        lo, hi, kk = ((C.c_int * len(bands))(*[int(b[i]) for b in bands]) for i in range(3))
        keep, sp = _scale_ptr(scale, n, x.device)
        with lib.device_ctx(x):
            out = torch.zeros(n, Cn, self.frames(L), 16, dtype=torch.float64, device=x.device)
            lib.check(lib.mst_mixfeat_spectral(self._handle(x), x.data_ptr(), n, L, Cn, sp, lo, hi, kk, len(bands), out.data_ptr(),
                                               lib.stream_ptr(x)), "mst_mixfeat_spectral")
        return out.cpu().numpy()

    def __del__(self):
        try:
            for h in self._handles.values():
                self.lib.mst_mixfeat_destroy(h)
        except Exception:
            pass


def frame_dynamics(x, frame_length, hop, scale=None):
    """x device [n, L, C] -> float64 numpy [n, C, T, 3]: per frame sum x^2, sum 20 log10(|x| + 1e-30), max |x|"""
    lib = _lib.lib()
    lib.require_device(x, "mst_mixfeat_dynamics")
    x = _batch(x)
    if x.dtype != torch.float32:
        raise ValueError(f"mst_mixfeat_dynamics: float32 expected, got {x.dtype}")
    n, L, Cn = x.shape
    T = 1 + (L - frame_length) // hop if L >= frame_length else 0
    keep, sp = _scale_ptr(scale, n, x.device)
    with lib.device_ctx(x):
        out = torch.empty(n, Cn, T, 3, dtype=torch.float64, device=x.device)
        lib.check(lib.mst_mixfeat_dynamics(x.data_ptr(), n, L, Cn, sp, int(frame_length), int(hop), out.data_ptr(), lib.stream_ptr(x)),
                  "mst_mixfeat_dynamics")
    return out.cpu().numpy()


def biquad_cascade(x, sos):
    """A cascade of second-order sections from rest over x device [n, L, C] (float64 recursion, float32 result); sos rows (b0, b1, b2, a0, a1, a2)"""
    lib = _lib.lib()
    x = _batch(x)
    coef = np.ascontiguousarray(sos, dtype=np.float64)
    n, L, Cn = x.shape
    y = torch.empty_like(x)
    with lib.device_ctx(x):
        nbytes = lib.mst_fx_biquad_scratch_bytes(n, L, Cn, len(coef))
        sc = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=x.device)
        lib.check(lib.mst_fx_biquad_cascade(x.data_ptr(), y.data_ptr(), n, L, Cn, coef.ctypes.data_as(C.POINTER(C.c_double)), len(coef),
                                            sc.data_ptr(), nbytes, None, lib.stream_ptr(x)), "mst_fx_biquad_cascade")
    return y


# ---------------------------------------------------------------------------------------- sample-rate conversion (csrc/resample_kernels.h)
class Resampler:
    """The polyphase resampler of one pair of rates: y[m] = sum_j h[m down - j up + half] x[j] (scipy.signal.resample_poly with
    padtype='constant'), float64 sums of exact products rounded once to float32."""
    _cache = {}

    @classmethod
    def get(cls, rate_in, rate_out):
        lib = _lib.lib()
        key = (lib.path, int(rate_in), int(rate_out))
        if key not in cls._cache:
            if len(cls._cache) > 8:
                cls._cache.clear()
            cls._cache[key] = cls(lib, rate_in, rate_out)
        return cls._cache[key]

    def __init__(self, lib, rate_in, rate_out):
        self.lib, self.rate_in, self.rate_out = lib, int(rate_in), int(rate_out)
        self._handles = {}
        g = np.gcd(self.rate_in, self.rate_out) if self.rate_in > 0 and self.rate_out > 0 else 1
        self.up, self.down = self.rate_out // int(g), self.rate_in // int(g)

    def _handle(self, device=None):
        """the handle on `device` (its tap table lives there); None: any handle there is - what info() and taps() ask is host data"""
        if device is None and self._handles:
            return next(iter(self._handles.values()))
        key = str(device)
        if key not in self._handles:
            h = C.c_void_p()
            on = torch.cuda.device(device) if device is not None and torch.device(device).type == "cuda" else contextlib.nullcontext()
            with on:
                self.lib.check(self.lib.mst_resample_create(self.rate_in, self.rate_out, C.byref(h)), "mst_resample_create")
            self._handles[key] = h
        return self._handles[key]

    def info(self):
        """(up, down, half_len, taps_per_phase)"""
        v = [C.c_int() for _ in range(4)]
        self.lib.check(self.lib.mst_resample_info(self._handle(), *[C.byref(a) for a in v]), "mst_resample_info")
        return tuple(a.value for a in v)

    def length(self, n_in):
        """ceil(n_in * up / down): the frames a signal of n_in frames comes out with"""
        return -((-int(n_in) * self.up) // self.down)

    def taps(self):
        """the 2 half_len + 1 float32 prototype taps as the library designed them"""
        n = 2 * self.info()[2] + 1
        out = np.empty(n, dtype=np.float32)
        self.lib.check(self.lib.mst_resample_taps(self._handle(), out.ctypes.data_as(C.POINTER(C.c_float)), n), "mst_resample_taps")
        return out

    def forward(self, x, n_out=None, in_start=0, out_start=0):
        """x device float32 [n, n_in, C] = inputs in_start .. of every item -> [n, n_out, C] = outputs out_start ..; the defaults resample
        the whole signal"""
        lib = self.lib
        lib.require_device(x, "mst_resample_forward")
        if x.dtype != torch.float32 or x.dim() != 3:
            raise ValueError(f"mst_resample_forward: float32 [n, L, C] expected, got {x.dtype} {tuple(x.shape)}")
        x = x.contiguous()
        n, n_in, Cn = x.shape
        n_out = self.length(n_in) if n_out is None else int(n_out)
        y = torch.empty(n, n_out, Cn, dtype=torch.float32, device=x.device)
        if n_in and n_out and n:
            with lib.device_ctx(x):
                lib.check(lib.mst_resample_forward(self._handle(x.device), x.data_ptr(), n_in, int(in_start), y.data_ptr(), n_out,
                                                   int(out_start), n, Cn, lib.stream_ptr(x)), "mst_resample_forward")
        else:
            y.zero_()
        return y

    def __del__(self):
        try:
            for h in self._handles.values():
                self.lib.mst_resample_destroy(h)
        except Exception:
            pass


def resample(x, rate_in, rate_out):
    """x float tensor [n, L, C] or [L, C], on the device or on the host (it then travels there and the result comes back) -> float32 of the same
    rank at ceil(L * rate_out / rate_in) frames.  Equal rates: x as float32, nothing runs."""
    t = x.to(torch.float32)
    if int(rate_in) == int(rate_out):
        return t
    lib = _lib.lib()
    y = Resampler.get(rate_in, rate_out).forward(_batch(lib.to_device(t)))
    y = y[0] if x.dim() == 2 else y
    return y if x.is_cuda else y.cpu()
