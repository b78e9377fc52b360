#!/usr/bin/env python
"""The mixing-feature metrics on one MI355X: HIP-event time of the fused path (csrc/mixfeat_kernels.h: the band sums of SPS^2, the frame
sums of the dynamics, the low-passed spectrum over the spectrum - with the device low-pass in front of it) against the same arithmetic
composed on torch-ROCm from torch.stft(center=False) and elementwise ops (restated below - the baseline: the capability is new, so there
is no earlier figure of this library's own).  Two workloads: 32 items of [131072, 2] and one pair of 3-minute stems.  The two paths are
timed in the same process, alternating, after both have been warmed; each round is `--steps` calls between two events.  Both paths
start from the peak-normalised batch and the low-passed batch on the device and end with the per-frame sequences on the device (the
fused path's copies of a few KB to the host are part of its time; the low-pass itself, common to both, is timed separately).
Prints ONE JSON line.

    python tools/bench_mixfeat.py [--rounds 7] [--steps 5] [--kernel-only N]

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

SR, N_FFT, HOP = 44100, 2048, 1024
BANDS = [(0, 1024), (0, 11), (11, 116), (116, 1024)]


def torch_baseline(x, x_low, window):
    """x, x_low [n, L, 2] peak-normalised -> (band sums of SPS^2 [n, T, 4], frame sums [n, 2, T, 3], low ratio [n, 2, T]) in float32 / float64
    like the fused path: float32 spectra and magnitudes, float64 per-bin arithmetic and sums"""
    n, L, C = x.shape

    def mags(v):
        S = torch.stft(v.permute(0, 2, 1).reshape(n * C, L), n_fft=N_FFT, hop_length=HOP, window=window, center=False, return_complex=True)
        return S.reshape(n, C, N_FFT // 2 + 1, -1)
    X = mags(x)
    l, r = (X[:, 0] + 1e-20).abs().double(), (X[:, 1] + 1e-20).abs().double()
    q = 1.0 - 2.0 * l * r / (l * l + r * r)
    s2 = q * q
    pan = torch.stack([s2[:, a:b].sum(dim=1) for a, b in BANDS], dim=-1)
    ratio = (mags(x_low).abs().double() / (X.abs().double() + 1e-5)).sum(dim=2)
    fr = x.permute(0, 2, 1).unfold(2, N_FFT, HOP).abs().double()
    dyn = torch.stack([(fr * fr).sum(-1), (20.0 * torch.log10(fr + 1e-30)).sum(-1), fr.amax(-1)], dim=-1)
    return pan, dyn, ratio


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--kernel-only", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mixfeat.py measures on the MI355X; no GPU is visible and there is no CPU path")
    from music_mixing_style_transfer_amd.mixing_manipulator import _device_ops as D
    from music_mixing_style_transfer_amd.mixing_manipulator import utils_data_normalization as U
    dev = torch.device("cuda:0")
    window = torch.from_numpy(np.sqrt(np.hanning(N_FFT + 1)[:-1]).astype(np.float32)).to(dev)
    mf = D.MixFeat.get(N_FFT, HOP)
    results = {}
    for tag, (n, L) in {"segments_32x131072": (32, 131072), "stem_pair_3min": (2, 7_938_000)}.items():
        g = torch.Generator().manual_seed(0)
        mid = 0.3 * torch.randn(n, L, 1, generator=g)
        x = torch.cat((mid + 0.1 * torch.randn(n, L, 1, generator=g), 0.8 * mid + 0.1 * torch.randn(n, L, 1, generator=g)), 2).clamp_(-1, 1).to(dev)
        x = (x * torch.from_numpy(U._peak_gain(x)).to(dev)[:, None, None]).contiguous()
        lowpass = lambda: U._lowpass_batch(x, 1000, SR)
        x_low = lowpass()

        def fused():
            return mf.panning(x, BANDS), D.frame_dynamics(x, N_FFT, HOP), mf.low_ratio(x_low, x)

        base = lambda: torch_baseline(x, x_low, window)
        for _ in range(2):
            fused()
            if not a.kernel_only:
                base()
        torch.cuda.synchronize()
        if a.kernel_only:
            for _ in range(a.kernel_only):
                fused()
                lowpass()
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

        t_fused, t_base, t_low = [], [], []
        for _ in range(a.rounds):          # alternating: a drift of the clock or a neighbour on the host hits both
            t_fused.append(timed(fused))
            t_base.append(timed(base))
            t_low.append(timed(lowpass))
        pf, df, rf = fused()
        pb, db, rb = (v.cpu().numpy() for v in base())
        rel = lambda u, v: float(np.abs(u - v).max() / max(np.abs(v).max(), 1e-300))
        mf_, mb = statistics.median(t_fused), statistics.median(t_base)
        ratio = mb / mf_
        results[tag] = {"items": n, "length": L, "fused_ms": mf_, "fused_ms_min_max": [min(t_fused), max(t_fused)], "torch_ms": mb,
                        "torch_ms_min_max": [min(t_base), max(t_base)], "torch_over_fused": ratio,
                        "verdict": "draw (ratio under 1.1)" if 1 / 1.1 < ratio < 1.1 else ("fused faster" if ratio > 1 else "torch faster"),
                        "lowpass_ms": statistics.median(t_low), "max_rel_diff": {"panning": rel(pf, pb), "dynamics": rel(df, db), "low_ratio": rel(rf, rb)},
                        "waveform_bytes": 2 * x.numel() * 4}
    if not a.kernel_only:
        print(json.dumps({"metric": "mixing-feature per-frame sequences, ms per call", "n_fft": N_FFT, "hop": HOP, "rounds": a.rounds, "steps": a.steps,
                          **results}))


if __name__ == "__main__":
    main()
