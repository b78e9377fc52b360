#!/usr/bin/env python
"""The spectral-feature kernel on one MI355X: HIP-event time of the fused path (csrc/mixfeat_kernels.h, mixfeat_spectral_kernel: 16
numbers per frame, no spectrum in HBM) against the same arithmetic composed on torch-ROCm from torch.stft(center=False), torch.sort,
cumsum and elementwise ops (restated below - the baseline: the capability is new, so there is no earlier figure of this library's own).
Two workloads at n_fft 4096 / hop 1024: 32 items of [131072, 2] and one pair of 3-minute stems.  The two paths are timed in the same
process, alternating, after both have been warmed; each round is `--steps` calls between two events.  Both start from the batch on the
device; the fused path's copy of its 16 numbers per frame to the host is part of its time.  Prints ONE JSON line.

    python tools/bench_specfeat.py [--rounds 7] [--steps 5] [--kernel-only N]

--kernel-only N: N fused calls per workload after the warm-up and nothing else (for a profiler run of its own)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SR, N_FFT, HOP = 44100, 4096, 1024


def torch_baseline(x, window, bands):
    """x [n, L, 2] -> [n, 2, T, 16] float64, slot for slot what the kernel leaves: float32 spectra and magnitudes, float64 after them"""
    n, L, C = x.shape
    m = N_FFT // 2
    X = torch.stft(x.permute(0, 2, 1).reshape(n * C, L), n_fft=N_FFT, hop_length=HOP, window=window, center=False, return_complex=True)
    S32 = X.abs().reshape(n, C, m + 1, -1).permute(0, 1, 3, 2)          # [n, C, T, bins]
    S = S32.double()
    k = torch.arange(m + 1, dtype=torch.float64, device=x.device)
    s0, s1 = S.sum(-1), (S * k).sum(-1)
    c = torch.where(s0 > 0, s1 / s0, torch.zeros_like(s0))
    s2 = (S * (k - c[..., None]) ** 2).sum(-1)
    ro = (S.cumsum(-1) >= (0.85 * s0)[..., None]).double().argmax(-1).double()
    P = (S * S).clamp_min(1e-10)
    out = [s0, s1, s2, ro, P.log().sum(-1), P.sum(-1)]
    for lo, hi, kk in bands:
        srt = torch.sort(S32[..., lo:hi], dim=-1).values.double()
        out += [srt[..., :kk].sum(-1), srt[..., -kk:].sum(-1)]
    return torch.stack(out, dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--kernel-only", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_specfeat.py measures on the MI355X; no GPU is visible and there is no CPU path")
    from music_mixing_style_transfer_amd.mixing_manipulator import _device_ops as D
    from music_mixing_style_transfer_amd.mixing_manipulator import utils_data_normalization as U
    dev = torch.device("cuda:0")
    window = torch.from_numpy(np.sqrt(np.hanning(N_FFT + 1)[:-1]).astype(np.float32)).to(dev)
    mf = D.MixFeat.get(N_FFT, HOP)
    bands = U.contrast_bands(SR, N_FFT)
    results = {}
    for tag, (n, L) in {"segments_32x131072": (32, 131072), "stem_pair_3min": (2, 7_938_000)}.items():
        g = torch.Generator().manual_seed(0)
        mid = 0.3 * torch.randn(n, L, 1, generator=g)
        x = torch.cat((mid + 0.1 * torch.randn(n, L, 1, generator=g), 0.8 * mid + 0.1 * torch.randn(n, L, 1, generator=g)), 2).clamp_(-1, 1).to(dev)
        x = (x * torch.from_numpy(U._peak_gain(x)).to(dev)[:, None, None]).contiguous()
        fused = lambda: mf.spectral(x, bands)
        base = lambda: torch_baseline(x, window, bands)
        for _ in range(2):
            fused()
            if not a.kernel_only:
                base()
        torch.cuda.synchronize()
        if a.kernel_only:
            for _ in range(a.kernel_only):
                fused()
            torch.cuda.synchronize()
            continue

        def timed(fn):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.steps):
                fn()
            e.record()
            torch.cuda.synchronize()
            return s.elapsed_time(e) / a.steps

        t_fused, t_base = [], []
        for _ in range(a.rounds):          # alternating: a drift of the clock or a neighbour on the host hits both
            t_fused.append(timed(fused))
            t_base.append(timed(base))
        got, ref = fused(), base().cpu().numpy()
        q = 6 + 2 * len(bands)
        scale = np.maximum(np.abs(ref[..., :q]).max(axis=(0, 1, 2)), 1e-300)
        rel = (np.abs(got[..., :q] - ref[..., :q]).max(axis=(0, 1, 2)) / scale)
        rel[3] = float(np.abs(got[..., 3] - ref[..., 3]).max())          # the roll-off index: the largest difference in bins
        mf_, mb = statistics.median(t_fused), statistics.median(t_base)
        ratio = mb / mf_
        results[tag] = {"items": n, "length": L, "frames": int(got.shape[2]), "fused_ms": mf_, "fused_ms_min_max": [min(t_fused), max(t_fused)],
                        "torch_ms": mb, "torch_ms_min_max": [min(t_base), max(t_base)], "torch_over_fused": ratio,
                        "verdict": "draw (ratio under 1.1)" if 1 / 1.1 < ratio < 1.1 else ("fused faster" if ratio > 1 else "torch faster"),
                        "max_rel_diff_per_slot": [float(v) for v in rel], "waveform_bytes": x.numel() * 4}
    if not a.kernel_only:
        print(json.dumps({"metric": "spectral-feature per-frame numbers, ms per call", "n_fft": N_FFT, "hop": HOP, "rounds": a.rounds,
                          "steps": a.steps, **results}))


if __name__ == "__main__":
    main()
