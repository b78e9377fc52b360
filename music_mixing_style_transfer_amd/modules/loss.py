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


# ---- NT_Xent (:24-71), infoNCE (:228-238): csrc/contrast_kernels.h through mst_ntxent_forward / mst_ntxent_backward -----------------------
_NTX_MODE, _NCE_MODE = 0, 1
_NTX_EPS, _NCE_EPS = 1e-8, 1e-12          # nn.CosineSimilarity's and F.normalize's clamp of the norm


def _check_views(b, x, y, what, names, differentiable):
    for t, name in zip((x, y), names):
        b.require_device(t, what)
        if not differentiable:
            _refuse_grad(t, what)
        if t.dtype != torch.float32:
            raise TypeError(f"{what}: float32 input expected, `{name}` is {t.dtype}")
    if x.dim() != 2 or x.shape != y.shape or x.device != y.device:
        raise ValueError(f"{what}: two [n, D] tensors of one shape on one device expected, got {tuple(x.shape)} and {tuple(y.shape)}")


def _ntx_workspace(b, x, with_grad):
    n, D = x.shape
    nbytes = b.mst_ntxent_workspace_bytes(n, n, D, with_grad)
    return torch.empty(max(nbytes, 256), dtype=torch.uint8, device=x.device), nbytes


def _ntx_forward(b, x, y, inv_tau, eps, mode, what, keep=None):
    n, D = x.shape
    with b.device_ctx(x):
        out = torch.empty((), dtype=torch.float64, device=x.device)
        ws, nbytes = _ntx_workspace(b, x, 0 if keep is None else 1)
        b.check(b.mst_ntxent_forward(x.data_ptr(), y.data_ptr(), n, n, D, inv_tau, eps, mode, out.data_ptr(), ws.data_ptr(), nbytes,
                                     b.stream_ptr(x)), what)
    if keep is not None:
        keep.ws = ws
    return out


class _NtXentValue(torch.autograd.Function):
    """mst_ntxent_forward's float64 loss with mst_ntxent_backward as its gradient to both views.  The forward's workspace (the similarities,
    the normalised rows) stays alive for the first backward, which consumes it; a second backward over a retained graph recomputes it."""

    @staticmethod
    def forward(ctx, x, y, b, inv_tau, eps, mode, what):
        ctx.save_for_backward(x, y)
        ctx.cfg = (b, inv_tau, eps, mode, what)
        return _ntx_forward(b, x, y, inv_tau, eps, mode, what, keep=ctx)

    @staticmethod
    @once_differentiable
    def backward(ctx, dloss):
        x, y = ctx.saved_tensors
        b, inv_tau, eps, mode, what = ctx.cfg
        n, D = x.shape
        dloss = dloss.to(torch.float64).contiguous()
        kept, ctx.ws = getattr(ctx, "ws", None), None
        with b.device_ctx(x):
            gx, gy = torch.empty_like(x), torch.empty_like(y)
            ws, nbytes = (kept, b.mst_ntxent_workspace_bytes(n, n, D, 1)) if kept is not None else _ntx_workspace(b, x, 1)
            b.check(b.mst_ntxent_backward(x.data_ptr(), y.data_ptr(), n, n, D, inv_tau, eps, mode, dloss.data_ptr(), gx.data_ptr(), gy.data_ptr(),
                                          0 if kept is None else 1, ws.data_ptr(), nbytes, b.stream_ptr(x)), what + " (backward)")
        return (gx if ctx.needs_input_grad[0] else None), (gy if ctx.needs_input_grad[1] else None), None, None, None, None, None


class NT_Xent(torch.nn.Module):
    """The reference's NT_Xent without its [N, N, D] broadcast: the Gram matrix of the normalised rows and a row-wise log-sum-exp.  A score
    by default; with differentiable=True the value carries its gradient to both views.  `mask` is kept for callers who read it."""

    def __init__(self, batch_size, temperature, world_size, differentiable=False):
        super().__init__()
        if world_size > 1:
            raise NotImplementedError(f"NT_Xent(world_size={world_size}): the multi-rank gather is not built (the reference's own Loss passes 1)")
        self.batch_size = batch_size
        self.temperature = temperature
        self.world_size = world_size
        self.mask = self.mask_correlated_samples(batch_size, world_size)
        self.differentiable = differentiable

    def mask_correlated_samples(self, batch_size, world_size):
        N = 2 * batch_size * world_size
        mask = torch.ones((N, N), dtype=bool)
        mask = mask.fill_diagonal_(0)
        for i in range(batch_size * world_size):
            mask[i, batch_size + i] = 0
            mask[batch_size + i, i] = 0
        return mask

    def forward(self, z_i, z_j):
        b = _lib.lib()
        _check_views(b, z_i, z_j, "NT_Xent", ("z_i", "z_j"), self.differentiable)
        if z_i.shape[0] != self.batch_size * self.world_size:
            raise ValueError(f"NT_Xent(batch_size={self.batch_size}): views of {z_i.shape[0]} rows")
        x, y = z_i.contiguous(), z_j.contiguous()
        args = (x, y, b, 1.0 / float(self.temperature), _NTX_EPS, _NTX_MODE, "mst_ntxent_forward")
        out = _NtXentValue.apply(*args) if self.differentiable else _ntx_forward(b, x, y, *args[3:])
        return out.to(torch.float32)


def infoNCE(nn, p, temperature=0.1):
    """DirectCLR's infoNCE as in the reference, one rank (gather_from_all is the identity there).  Differentiable when an input requires
    grad: the gradient goes to both arguments."""
    b = _lib.lib()
    _check_views(b, nn, p, "infoNCE", ("nn", "p"), True)
    x, y = nn.contiguous(), p.contiguous()
    args = (x, y, b, 1.0 / float(temperature), _NCE_EPS, _NCE_MODE, "mst_ntxent_forward")
    out = _NtXentValue.apply(*args) if (x.requires_grad or y.requires_grad) else _ntx_forward(b, x, y, *args[3:])
    return out.to(torch.float32)


# ---- RMSLoss (:77-93): rms_rows_kernel / rms_finish_kernel / rms_grad_kernel ------------------------------------------------------------
def _rms_forward(b, est, tgt, wf):
    rows, T = est.shape[0] * est.shape[1], est.shape[2]
    with b.device_ctx(est):
        out = torch.empty((), dtype=torch.float64, device=est.device)
        nbytes = b.mst_rms_loss_workspace_bytes(rows, T)
        ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=est.device)
        b.check(b.mst_rms_loss_forward(est.data_ptr(), tgt.data_ptr(), rows, T, wf, out.data_ptr(), ws.data_ptr(), nbytes, b.stream_ptr(est)),
                "mst_rms_loss_forward")
    return out


class _RmsValue(torch.autograd.Function):
    """mst_rms_loss_forward's float64 loss with mst_rms_loss_backward as its gradient with respect to est"""

    @staticmethod
    def forward(ctx, est, tgt, b, wf):
        ctx.save_for_backward(est, tgt)
        ctx.cfg = (b, wf)
        return _rms_forward(b, est, tgt, wf)

    @staticmethod
    @once_differentiable
    def backward(ctx, dloss):
        est, tgt = ctx.saved_tensors
        b, wf = ctx.cfg
        rows, T = est.shape[0] * est.shape[1], est.shape[2]
        dloss = dloss.to(torch.float64).contiguous()
        with b.device_ctx(est):
            grad = torch.empty_like(est)
            nbytes = b.mst_rms_loss_workspace_bytes(rows, T)
            ws = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=est.device)
            b.check(b.mst_rms_loss_backward(est.data_ptr(), tgt.data_ptr(), rows, T, wf, dloss.data_ptr(), grad.data_ptr(), ws.data_ptr(), nbytes,
                                            b.stream_ptr(est)), "mst_rms_loss_backward")
        return grad, None, None, None


class RMSLoss(torch.nn.Module):
    """The reference's gain loss, its quirk kept: nn.MSELoss(reduce=None) is the mean reduction, so the value is
    mean(weight ** 1.5) * mse(rms_est, rms_tgt).  The gradient (differentiable=True) is with respect to the estimate only."""

    def __init__(self, reduce, loss_type="l2", differentiable=False):
        super().__init__()
        if loss_type != "l2":
            raise NotImplementedError(f"RMSLoss(loss_type={loss_type!r}): the reference defines 'l2' only")
        self.weight_factor = 100.
        self.differentiable = differentiable

    def forward(self, est_targets, targets):
        b = _lib.lib()
        what = "RMSLoss"
        for t in (est_targets, targets):
            b.require_device(t, what)
            if not self.differentiable:
                _refuse_grad(t, what)
            elif t is targets and t.requires_grad:
                raise NotImplementedError(f"{what}(differentiable=True): `targets` requires grad - only the gradient with respect to the "
                                          f"estimate is built")
            if t.dtype != torch.float32:
                raise TypeError(f"{what}: float32 input expected, got {t.dtype}")
        if est_targets.dim() != 3 or est_targets.shape != targets.shape or est_targets.device != targets.device:
            raise ValueError(f"{what}: two [B, C, T] tensors of one shape on one device expected, got {tuple(est_targets.shape)} and "
                             f"{tuple(targets.shape)}")
        est, tgt = est_targets.contiguous(), targets.contiguous()
        wf = float(self.weight_factor)
        out = _RmsValue.apply(est, tgt, b, wf) if self.differentiable else _rms_forward(b, est, tgt, wf)
        return out.to(torch.float32)


class Loss:
    """The reference's container of objective functions (:244-258), built from the trainer's args; its device-backed members carry
    gradients."""

    def __init__(self, args, reduce=True):
        device = torch.device("cpu")
        if torch.cuda.is_available():
            device = torch.device(f"cuda:{args.gpu}")
        self.l1 = torch.nn.L1Loss(reduce=reduce)
        self.mse = torch.nn.MSELoss(reduce=reduce)
        self.ce = torch.nn.CrossEntropyLoss()
        self.triplet = torch.nn.TripletMarginLoss(margin=1., p=2)

        self.ntxent = NT_Xent(args.batch_size_total * (args.num_strong_negatives + 1), args.temperature, world_size=1, differentiable=True)
        self.multi_scale_spectral_midside = MultiScale_Spectral_Loss_MidSide_DDSP(mode='midside', eps=args.eps, device=device, differentiable=True)
        self.multi_scale_spectral_ori = MultiScale_Spectral_Loss_MidSide_DDSP(mode='ori', eps=args.eps, device=device, differentiable=True)
        self.gain = RMSLoss(reduce=reduce, differentiable=True)
        self.infonce = infoNCE
