"""MultiScale_Spectral_Loss_MidSide_DDSP of the reference (modules/loss.py:99-213) on the MI355X: one fused kernel per scale reads the two
waveforms and leaves the sums (mst_mss_forward); nothing per frame goes to HBM.  By default it is a score (an input that requires grad is
refused); with differentiable=True the sums carry their closed-form gradient with respect to the estimate (mst_mss_backward), so
loss(est, tgt).backward() works - the gradient with respect to the targets is not built."""
import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from .front_back_end import _MssModule, _refuse_grad


def _mss_forward(b, h, est, tgt):
    B, _, L = est.shape
    with b.device_ctx(est):
        out = torch.empty(B, len(h.scales), 2, 2, dtype=torch.float64, device=est.device)
        nbytes = b.mst_mss_workspace_bytes(h.ptr, B, L)
        ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=est.device)
        b.check(b.mst_mss_forward(h.ptr, est.data_ptr(), tgt.data_ptr(), B, L, out.data_ptr(), ws.data_ptr(), nbytes, b.stream_ptr(est)),
                "mst_mss_forward")
    return out


class _MssSums(torch.autograd.Function):
    """mst_mss_forward's sums with mst_mss_backward as their vector-Jacobian product with respect to est"""

    @staticmethod
    def forward(ctx, est, tgt, b, h):
        ctx.save_for_backward(est, tgt)
        ctx.binding, ctx.handle = b, h
        return _mss_forward(b, h, est, tgt)

    @staticmethod
    @once_differentiable
    def backward(ctx, dterms):
        est, tgt = ctx.saved_tensors
        b, h = ctx.binding, ctx.handle
        B, _, L = est.shape
        dterms = dterms.to(torch.float64).contiguous()
        with b.device_ctx(est):
            grad = torch.empty_like(est)
            nbytes = b.mst_mss_backward_workspace_bytes(h.ptr, B, L)
            ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=est.device)
            b.check(b.mst_mss_backward(h.ptr, est.data_ptr(), tgt.data_ptr(), B, L, dterms.data_ptr(), grad.data_ptr(), ws.data_ptr(), nbytes,
                                       b.stream_ptr(est)), "mst_mss_backward")
        return grad, None, None, None


class MultiScale_Spectral_Loss_MidSide_DDSP(_MssModule):
    def __init__(self, mode='midside', reduce=True, n_filters=None, windows_size=None, hops_size=None, window="hann", eps=1e-7,
                 device=torch.device("cpu"), differentiable=False):
        super().__init__()
        if not reduce:
            raise NotImplementedError("MultiScale_Spectral_Loss_MidSide_DDSP(reduce=False): the kernel returns sums, not elementwise maps")
        self.mode = mode
        self.eps = eps
        self.mid_weight = 0.5
        self.logmag_weight = 0.1
        n_filters = [4096, 2048, 1024, 512] if n_filters is None else list(n_filters)
        windows_size = [4096, 2048, 1024, 512] if windows_size is None else list(windows_size)
        hops_size = [1024, 512, 256, 128] if hops_size is None else list(hops_size)
        self.scales = [(n_filters[i], hops_size[i], windows_size[i]) for i in range(len(windows_size))]
        self.window_kind = window
        self.differentiable = differentiable

    def _check(self, est, tgt, what):
        b = _lib.lib()
        for t in (est, tgt):
            b.require_device(t, what)
            if not self.differentiable:
                _refuse_grad(t, what)
            elif t is tgt and t.requires_grad:
                raise NotImplementedError(f"{what}(differentiable=True): `targets` requires grad - only the gradient with respect to the "
                                          f"estimate is built")
            if t.dtype != torch.float32:
                raise TypeError(f"{what}: float32 input expected, got {t.dtype}")
        if est.dim() != 3 or est.shape[1] != 2 or est.shape != tgt.shape or est.device != tgt.device:
            raise ValueError(f"{what}: two [B, 2, L] tensors of one shape on one device expected, got {tuple(est.shape)} and {tuple(tgt.shape)}")
        return b

    def sums(self, est_targets, targets):
        """float64 [B, n_scales, 2, 2]: per item, scale and channel (mid, side / left, right) the two sums mst_mss_forward leaves."""
        b = self._check(est_targets, targets, "MultiScale_Spectral_Loss_MidSide_DDSP")
        est, tgt = est_targets.contiguous(), targets.contiguous()
        B, _, L = est.shape
        h = self._handle_for(b, est, self.mode, self.scales, self.window_kind, self.eps)
        out = _MssSums.apply(est, tgt, b, h) if self.differentiable else _mss_forward(b, h, est, tgt)
        return out, self._counts(h, L, est.device)

    def _counts(self, h, L, device):
        """bins x frames of every scale as a device tensor, made once per (handle, L)"""
        cache = self.__dict__.setdefault("_count_cache", {})
        key = (id(h), L)
        if key not in cache:
            cache[key] = torch.tensor([(s[0] // 2) * h.frames(i, L) for i, s in enumerate(h.scales)], dtype=torch.float64, device=device)
        return cache[key]

    def terms(self, est, tgt):
        """float64 [B, n_scales, 2, 2]: item b's magnitude term [..., 0] and log term [..., 1] of every scale and channel, as means over
        that item's bins and frames.  Their mean over the items is the batch's term; forward() combines those."""
        sums, counts = self.sums(est, tgt)
        return sums / counts.view(1, -1, 1, 1)

    def forward(self, est_targets, targets):
        v = self.terms(est_targets, targets).mean(dim=0)                      # [scale, channel, term]
        ch = self.mid_weight * v[:, 0, :] + (1.0 - self.mid_weight) * v[:, 1, :]
        return ((1.0 - self.logmag_weight) * ch[:, 0].sum() + self.logmag_weight * ch[:, 1].sum()).to(torch.float32)
