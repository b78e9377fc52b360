"""TEST INFRASTRUCTURE: the checks the emulator tests and the GPU tests of the multi-scale spectral kernel share - a golden case's terms
and a spectrogram against the float64 restatement and its bounds (tests/mss_ref.py)."""
import numpy as np
import torch

import mss_ref as R
from music_mixing_style_transfer_amd.modules import MultiScale_Spectral_Loss_MidSide_DDSP


def _module(kw):
    sc = kw["scales"]
    return MultiScale_Spectral_Loss_MidSide_DDSP(mode=kw["mode"], n_filters=[s[0] for s in sc], hops_size=[s[1] for s in sc],
                                                 windows_size=[s[2] for s in sc], window=kw["kind"], eps=kw["eps"])


def _ratio(err, bnd):
    """max err / bound; an error where the bound is zero counts as infinite"""
    err, bnd = np.asarray(err, dtype=np.float64), np.asarray(bnd, dtype=np.float64)
    r = np.divide(err, bnd, out=np.zeros_like(err), where=bnd > 0)
    r[(bnd == 0) & (err > 0)] = np.inf
    return float(r.max())


def check_case(name, length, device=None):
    est, tgt, kw = R.case_inputs(name, length)
    loss = _module(kw)
    e, t = torch.from_numpy(est), torch.from_numpy(tgt)
    if device is not None:
        e, t = e.to(device), t.to(device)
    got = loss.terms(e, t).cpu().numpy()
    val, bnd = R.terms(est, tgt, **kw)
    ratio = _ratio(np.abs(got - val), bnd)
    tot, tot_bnd = R.loss(est, tgt, **kw)
    got_tot = float(loss(e, t))
    print(f"{name:16s} L = {est.shape[-1]:7d}  max term err / bound = {ratio:.4f}   total {got_tot:.9g} (float64 {tot:.12g})")
    assert ratio <= 1.0, name
    assert abs(got_tot - tot) <= tot_bnd + 2.0 ** -23 * abs(tot), name          # + the rounding of the float32 result itself
    return ratio, got, val


def check_front_end(got, x, n_fft, hop, wl, kind, what):
    """every element within delta_elem and every frame's rms error within delta (tests/mss_ref.py)"""
    assert got.dtype == np.float32
    r_elem, r_frame, r_plain = R.front_end_ratios(got, x, n_fft, hop, wl, kind)
    print(f"FrontEnd {what}: {got.shape}, max element err / bound = {r_elem:.4f}, max frame rms err / delta = {r_frame:.4f} (max element err / plain delta: {r_plain:.3f})")
    assert r_elem <= 1.0 and r_frame <= 1.0, what
    return r_elem, r_frame
