#!/usr/bin/env python
"""Value + gradient of the multi-scale spectral loss at 32 x 2 x 131072 on one MI355X: loss(est, tgt).backward() through the fused kernels
(mst_mss_forward + mst_mss_backward, csrc/mss_kernels.h) against the same arithmetic through torch.stft + autograd on the same device
(tools/bench_mss.py's restatement - the baseline: the capability is new, so there is no earlier figure of this library's own).  The two
are timed in the same process, alternating, after both have been warmed; each round is `--steps` value + gradient calls between two events.
Peak memory is torch's allocator peak over one call of each, above what was allocated before it.  Prints ONE JSON line per mode and writes
them to --out.

    python tools/bench_mss_grad.py [--batch 32] [--length 131072] [--modes midside ori] [--rounds 7] [--steps 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from bench_mss import SCALES, torch_baseline  # noqa: E402


def measure(a, mode):
    from music_mixing_style_transfer_amd.modules import MultiScale_Spectral_Loss_MidSide_DDSP
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    tgt = (0.3 * torch.randn(a.batch, 2, a.length, generator=g)).clamp_(-1, 1).to(dev)
    est = (tgt + 0.02 * torch.randn(a.batch, 2, a.length, generator=g).to(dev)).clamp_(-1, 1).requires_grad_(True)
    loss = MultiScale_Spectral_Loss_MidSide_DDSP(mode=mode, differentiable=True)
    windows = [torch.hann_window(n, periodic=True, device=dev) for n, _ in SCALES]

    def fused():
        est.grad = None
        v = loss(est, tgt)
        v.backward()
        return v

    def base():
        est.grad = None
        v = torch_baseline(est, tgt, windows, mode)
        v.backward()
        return v

    for _ in range(3):
        fused()
        base()
    torch.cuda.synchronize()

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.steps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.steps

    def peak(fn):
        est.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before

    t_fused, t_base = [], []
    for _ in range(a.rounds):          # alternating: a drift of the clock or a neighbour on the host hits both
        t_fused.append(timed(fused))
        t_base.append(timed(base))
    v_fused = float(fused())
    g_fused = est.grad.clone()
    v_base = float(base())
    g_base = est.grad.clone()
    p_fused, p_base = peak(fused), peak(base)
    mf, mb = statistics.median(t_fused), statistics.median(t_base)
    return {"metric": "multi-scale spectral loss, value + gradient, ms per call", "batch": a.batch, "length": a.length, "mode": mode,
            "fused_ms": mf, "fused_ms_min_max": [min(t_fused), max(t_fused)], "torch_stft_autograd_ms": mb,
            "torch_stft_autograd_ms_min_max": [min(t_base), max(t_base)], "speedup_vs_torch_stft_autograd": mb / mf, "rounds": a.rounds,
            "steps": a.steps, "value_fused": v_fused, "value_torch_stft": v_base,
            "grad_max_abs_diff_over_max_abs": float((g_fused - g_base).abs().max() / g_base.abs().max()),
            "peak_bytes_fused": p_fused, "peak_bytes_torch_stft_autograd": p_base, "peak_ratio": p_base / max(p_fused, 1),
            "waveform_bytes": 2 * a.batch * 2 * a.length * 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--length", type=int, default=131072)
    ap.add_argument("--modes", nargs="+", default=["midside", "ori"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mss_grad_bench_mi355x.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mss_grad.py measures on the MI355X; no GPU is visible and there is no CPU path")
    results = []
    for mode in a.modes:
        results.append(measure(a, mode))
        print(json.dumps(results[-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
