"""TEST INFRASTRUCTURE: the checks the emulator tests and the GPU tests of the spectral loss's gradient share - mst_mss_backward through the
raw C ABI and through loss(est, tgt).backward(), sample by sample against the float64 restatement and its bound (tests/mss_grad_ref.py)."""
import ctypes as C

import numpy as np
import torch

import mss_grad_ref as GR
import mss_ref as R
from music_mixing_style_transfer_amd import _lib
from music_mixing_style_transfer_amd.modules import MultiScale_Spectral_Loss_MidSide_DDSP

TIE_CAP = 1e-3          # tie bins (charged 2 |a| by the bound) may be at most 0.1 % of a bounded item's bins

# (scales, window): the smallest shapes at which each piece can go wrong - one per transform size the forward instantiates, both mirrors on
# the same samples, the dropped last frame, a hop that does not divide n_fft, a short Hamming window, several scales accumulating
SHAPES = {
    "n4096_mirrors_overlap": (((4096, 1024, 4096),), "hann", 2049),
    "n4096_last_frame_dropped": (((4096, 1024, 4096),), "hann", 8192),
    "n2048": (((2048, 512, 2048),), "hann", 3001),
    "n1024_hop100": (((1024, 100, 1024),), "hann", 7001),
    "n512_groups_of_8": (((512, 128, 512),), "hann", 3000),
    "n512_win300_hamming": (((512, 128, 300),), "hamming", 7001),
    "n256": (((256, 64, 256),), "hann", 1000),
    "default_scales": (R.DEFAULT_SCALES, "hann", 5000),
}
GENERIC, IDENTICAL, ZERO, MONO = 0, 1, 2, 3


def batch_of_four(L, seed=0):
    """est, tgt [4, 2, L]: independent noise at different levels (no tie bins); est identical to tgt; est all zero; a mono pair"""
    rng = np.random.default_rng(seed)
    tgt = rng.uniform(-1.0, 1.0, size=(4, 2, L)).astype(np.float32)
    est = (np.float32(0.3) * rng.uniform(-1.0, 1.0, size=(4, 2, L))).astype(np.float32)
    est[IDENTICAL] = tgt[IDENTICAL]
    est[ZERO] = 0.0
    est[MONO, 1], tgt[MONO, 1] = est[MONO, 0], tgt[MONO, 0]
    return est, tgt


def module(mode, scales, kind, differentiable=True):
    return MultiScale_Spectral_Loss_MidSide_DDSP(mode=mode, n_filters=[s[0] for s in scales], hops_size=[s[1] for s in scales],
                                                 windows_size=[s[2] for s in scales], window=kind, differentiable=differentiable)


def backward_abi(b, est, tgt, cot, mode, scales, kind, device=None, eps=1e-7):
    """mst_mss_backward through the raw C ABI of binding b: numpy in, numpy float32 [B, 2, L] out"""
    e, t, ct = torch.from_numpy(est), torch.from_numpy(tgt), torch.from_numpy(np.ascontiguousarray(cot, dtype=np.float64))
    if device is not None:
        e, t, ct = e.to(device), t.to(device), ct.to(device)
    B, _, L = e.shape
    desc = _lib.MstMssDesc(_lib.MSS_MODES[mode], [s[0] for s in scales], [s[1] for s in scales], [s[2] for s in scales], _lib.MSS_WINDOWS[kind], eps)
    h = C.c_void_p()
    with b.device_ctx(e):
        b.check(b.mst_mss_create(C.byref(desc), C.byref(h)), "mst_mss_create")
        try:
            nbytes = b.mst_mss_backward_workspace_bytes(h, B, L)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=e.device)
            grad = torch.full_like(e, float("nan"))          # written, not accumulated
            b.check(b.mst_mss_backward(h, e.data_ptr(), t.data_ptr(), B, L, ct.data_ptr(), grad.data_ptr(), ws.data_ptr(), nbytes, b.stream_ptr(e)),
                    "mst_mss_backward")
            out = grad.cpu().numpy()
        finally:
            b.mst_mss_destroy(h)
    return out


def backward_module(est, tgt, mode, scales, kind, device=None):
    """(loss value, d value / d est) through loss(est, tgt).backward()"""
    loss = module(mode, scales, kind)
    e, t = torch.from_numpy(est), torch.from_numpy(tgt)
    if device is not None:
        e, t = e.to(device), t.to(device)
    e.requires_grad_(True)
    out = loss(e, t)
    out.backward()
    return out.detach(), e.grad.cpu().numpy()


def all_bits_zero(a):
    return not np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).any()


def check_batch_of_four(got, est, tgt, cot, mode, scales, kind, what):
    """got [4, 2, L] against the restatement: the generic and the mono item within the bound sample by sample (few tie bins), the identical
    and the all-zero item all bits zero, the mono item's side contribution exactly nothing.  Returns the largest error / bound."""
    assert got.dtype == np.float32 and got.shape == est.shape
    assert all_bits_zero(got[IDENTICAL]), f"{what}: est identical to tgt must give an all-zero gradient"
    assert all_bits_zero(got[ZERO]), f"{what}: est == 0 must give an all-zero gradient"
    worst = 0.0
    for i in (GENERIC, MONO):
        ct = np.array(cot[i:i + 1], dtype=np.float64)
        if i == MONO and mode == "midside":
            assert np.array_equal(got[i, 0].view(np.uint32), got[i, 1].view(np.uint32)), f"{what}: the side channel of a mono item contributes"
            ct[:, :, 1, :] = 0.0          # ... exactly nothing, in float64 too: bounded without charging the side's (all tie) bins
        ref, bnd, ties, bins = GR.vjp(est[i:i + 1], tgt[i:i + 1], ct, mode, scales, kind)
        assert ties <= TIE_CAP * bins, f"{what}: {ties} tie bins of {bins}"
        r = GR.ratio(np.abs(got[i:i + 1].astype(np.float64) - ref), bnd)
        print(f"{what} item {i}: max |g| = {np.abs(ref).max():.4g}, max error / bound = {r:.4f}, max error / max |g| = "
              f"{np.abs(got[i:i + 1] - ref).max() / np.abs(ref).max():.2e}, tie bins {ties} of {bins}")
        assert r <= 1.0, (what, i, r)
        worst = max(worst, r)
    return worst


def random_cotangents(B, n_scales, seed=1):
    """non-uniform cotangents of both signs over three decades, one (item, scale, channel) row zero"""
    rng = np.random.default_rng(seed)
    cot = rng.uniform(-1.0, 1.0, size=(B, n_scales, 2, 2)) * 10.0 ** rng.uniform(-5.0, -2.0, size=(B, n_scales, 2, 1))
    cot[GENERIC, 0, 1, :] = 0.0
    return cot
