"""FrontEnd of the reference (modules/front_back_end.py:9-82), mode ["mag"]: STFT magnitudes on the MI355X (mst_mss_spectrogram).

Forward only: there is no autograd through the kernel, so an input that requires grad is refused instead of silently detached.
"cplx" features and BackEnd (the way back to a waveform) belong to training and are not built."""
import ctypes as C

import torch
import torch.nn as nn

from .. import _lib


def _refuse_grad(t, what):
    if t.requires_grad:
        raise NotImplementedError(f"{what}: forward only - the input requires grad and there is no backward through the HIP kernel")


class _MssHandle:
    """One mst_mss handle (the tables of its scales live on the device that was current at creation), freed with the object."""

    def __init__(self, binding, mode, scales, window, eps):
        if window not in _lib.MSS_WINDOWS:
            raise NotImplementedError(f"window={window!r}: 'hann' or 'hamming'")
        if mode not in _lib.MSS_MODES:
            raise NotImplementedError(f"mode={mode!r}: 'midside' or 'ori'")
        if len(scales) > _lib.MST_MSS_MAX_SCALES:
            raise NotImplementedError(f"{len(scales)} scales: at most {_lib.MST_MSS_MAX_SCALES}")
        self.binding, self.scales = binding, tuple(scales)
        desc = _lib.MstMssDesc(_lib.MSS_MODES[mode], [int(s[0]) for s in scales], [int(s[1]) for s in scales], [int(s[2]) for s in scales],
                               _lib.MSS_WINDOWS[window], float(eps))
        self.ptr = C.c_void_p()
        binding.check(binding.mst_mss_create(C.byref(desc), C.byref(self.ptr)), "mst_mss_create")

    def frames(self, scale, L):
        return self.binding.mst_mss_frames(self.ptr, scale, L)

    def __del__(self):
        if getattr(self, "ptr", None):
            self.binding.mst_mss_destroy(self.ptr)
            self.ptr = None


class _MssModule(nn.Module):
    """Keeps one handle per (binding, device, descriptor): attributes changed after the first call get a handle of their own."""

    def _handle_for(self, b, t, mode, scales, window, eps):
        key = (id(b), str(t.device), mode, tuple(tuple(int(v) for v in s) for s in scales), window, float(eps))
        cache = self.__dict__.setdefault("_handles", {})
        if key not in cache:
            with b.device_ctx(t):
                cache[key] = _MssHandle(b, mode, scales, window, eps)
        return cache[key]


class FrontEnd(_MssModule):
    def __init__(self, channel='stereo', n_fft=2048, hop_length=None, win_length=None, window="hann", device=torch.device("cpu")):
        super().__init__()
        self.channel = channel
        self.n_fft = n_fft
        self.hop_length = n_fft // 4 if hop_length is None else hop_length
        self.win_length = n_fft if win_length is None else win_length
        self.window_kind = window

    def forward(self, input, mode):
        """input [B, L] (channel="mono") or [B, 2, L] ("stereo"), float32 on the device -> [B, 1 | 2, n_fft / 2, T]."""
        mode = list(mode)
        if not mode:
            raise NameError("NameError at FrontEnd: check using features for front-end")
        if mode != ["mag"]:
            raise NotImplementedError(f"FrontEnd.forward(mode={mode}): only ['mag'] is built ('cplx' belongs to training)")
        b = _lib.lib()
        b.require_device(input, "FrontEnd.forward")
        _refuse_grad(input, "FrontEnd.forward")
        if input.dtype != torch.float32:
            raise TypeError(f"FrontEnd.forward: float32 input expected, got {input.dtype}")
        if self.channel == "mono":
            if input.dim() != 2:
                raise ValueError(f"FrontEnd(channel='mono').forward: expected [B, L], got {tuple(input.shape)}")
            x, Cn = input.contiguous(), 1
        elif self.channel == "stereo":
            if input.dim() != 3 or input.shape[1] < 2:
                raise ValueError(f"FrontEnd(channel='stereo').forward: expected [B, 2, L], got {tuple(input.shape)}")
            x, Cn = input[:, :2].contiguous(), 2
        else:
            raise NotImplementedError(f"FrontEnd(channel={self.channel!r})")
        B, L = x.shape[0], x.shape[-1]
        h = self._handle_for(b, x, "ori", [(self.n_fft, self.hop_length, self.win_length)], self.window_kind, 1e-7)
        with b.device_ctx(x):
            T = h.frames(0, L)
            out = torch.empty(B, Cn, self.n_fft // 2, max(T, 0), dtype=torch.float32, device=x.device)
            b.check(b.mst_mss_spectrogram(h.ptr, 0, x.data_ptr(), B, Cn, L, out.data_ptr(), b.stream_ptr(x)), "mst_mss_spectrogram")
        return out


class BackEnd(nn.Module):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("BackEnd (spectrogram -> waveform) belongs to training and is not built")
