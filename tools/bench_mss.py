#!/usr/bin/env python
"""The multi-scale spectral distance at 32 x 2 x 131072 on one MI355X: HIP-event time of mst_mss_forward (one fused kernel per scale,
csrc/mss_kernels.h) against the same arithmetic on torch-ROCm (torch.stft on the GPU, restated below - the baseline: the capability
is new, so there is no earlier figure of this library's own).  The two are timed in the same process, alternating, after both have
been warmed; each round is `--steps` calls between two events.  Prints ONE JSON line: the median round of each, the spread, the ratio,
the two values (they agree to float32 rounding) and the waveform bytes / transform points behind the rates.

    python tools/bench_mss.py [--batch 32] [--length 131072] [--mode midside] [--rounds 7] [--steps 10] [--kernel-only N]

--kernel-only N: N fused forwards after the warm-up and nothing else (for a profiler run of its own)."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SCALES = ((4096, 1024), (2048, 512), (1024, 256), (512, 128))


def torch_baseline(est, tgt, windows, mode, eps=1e-7):
    """the reference's arithmetic on torch-ROCm: float32 torch.stft (center, reflect), m = sqrt(re^2 + im^2 + 1e-7), bins 1 .., the last
    frame dropped when L % (n_fft / 4) == 0, 0.9 L1 + 0.1 L2 of log10 over mid / side (or left / right)"""
    if mode == "midside":
        sig = lambda x: (x[:, 0] + x[:, 1], x[:, 0] - x[:, 1])
    else:
        sig = lambda x: (x[:, 0], x[:, 1])
    L = est.shape[-1]
    mag_total = log_total = 0.0
    for (n_fft, hop), w in zip(SCALES, windows):
        def mags(x):
            S = torch.stft(x, n_fft=n_fft, hop_length=hop, win_length=n_fft, window=w, return_complex=True)
            m = torch.sqrt(S.real ** 2 + S.imag ** 2 + 1e-7)
            if L % (n_fft // 4) == 0:
                m = m[:, :, :-1]
            return m[:, 1:]
        for e, t in zip(sig(est), sig(tgt)):
            me, mt = mags(e), mags(t)
            mag_total = mag_total + 0.5 * (me - mt).abs().mean()
            log_total = log_total + 0.5 * ((torch.log10(me + eps) - torch.log10(mt + eps)) ** 2).mean()
    return 0.9 * mag_total + 0.1 * log_total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--length", type=int, default=131072)
    ap.add_argument("--mode", default="midside")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--kernel-only", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mss.py measures on the MI355X; no GPU is visible and there is no CPU path")
    from music_mixing_style_transfer_amd.modules import MultiScale_Spectral_Loss_MidSide_DDSP
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    tgt = (0.3 * torch.randn(a.batch, 2, a.length, generator=g)).clamp_(-1, 1).to(dev)
    est = (tgt + 0.02 * torch.randn(a.batch, 2, a.length, generator=g).to(dev)).clamp_(-1, 1)
    loss = MultiScale_Spectral_Loss_MidSide_DDSP(mode=a.mode)
    windows = [torch.hann_window(n, periodic=True, device=dev) for n, _ in SCALES]
    fused = lambda: loss.sums(est, tgt)[0]          # mst_mss_forward and the allocation of its 1 KB result / workspace; no host sync
    base = lambda: torch_baseline(est, tgt, windows, a.mode)
    for _ in range(3):
        fused()
        if not a.kernel_only:
            base()
    torch.cuda.synchronize()
    if a.kernel_only:
        for _ in range(a.kernel_only):
            fused()
        torch.cuda.synchronize()
        return

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
    v_fused, v_base = float(loss(est, tgt)), float(base())
    mf, mb = statistics.median(t_fused), statistics.median(t_base)
    frames = sum((a.length // hop + 1 - (1 if a.length % (n // 4) == 0 else 0)) * n for n, hop in SCALES)          # samples transformed per signal
    points = 4 * a.batch * frames
    flops = sum(4 * a.batch * (a.length // hop + 1) * 2.5 * n * math.log2(n) for n, hop in SCALES)                # real FFT: 2.5 n log2 n
    print(json.dumps({"metric": "multi-scale spectral distance, ms per call", "batch": a.batch, "length": a.length, "mode": a.mode,
                      "fused_ms": mf, "fused_ms_min_max": [min(t_fused), max(t_fused)], "torch_stft_ms": mb,
                      "torch_stft_ms_min_max": [min(t_base), max(t_base)], "speedup_vs_torch_stft": mb / mf, "rounds": a.rounds, "steps": a.steps,
                      "value_fused": v_fused, "value_torch_stft": v_base, "segments_per_s": a.batch / (mf * 1e-3),
                      "waveform_bytes": 2 * a.batch * 2 * a.length * 4, "transformed_points": points,
                      "fft_gflops_fused": flops / (mf * 1e-3) / 1e9}))


if __name__ == "__main__":
    main()
