#!/usr/bin/env python
"""The polyphase resampler on one MI355X (csrc/resample_kernels.h): a three-minute stereo stem, 8 640 000 frames at 48 kHz -> 7 938 000 at
44.1 kHz, HIP-event time per call after warm-up (each round is `--steps` calls between two events), against
scipy.signal.resample_poly(x, 147, 160, window=taps / 147) of the same samples in float64 on the host (timed once with the host clock: the
baseline a user without the kernel has; the capability is new, so there is no earlier figure of this library's own and no gate).  Bytes
moved = (n_in + n_out) * C * 4: every input frame read once, every output frame written once; the achieved bandwidth is that over the
kernel's time - the kernel does 140 float64 multiply-adds per output sample, so it is not expected to sit at the HBM roof.
Prints ONE JSON line.

    python tools/bench_resample.py [--rounds 7] [--steps 10] [--kernel-only N]

--kernel-only N: N calls after the warm-up and nothing else (for a profiler run of its own)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

RATE_IN, RATE_OUT, N_IN, C = 48000, 44100, 8_640_000, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--kernel-only", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample.py measures on the MI355X; no GPU is visible and there is no CPU path")
    from music_mixing_style_transfer_amd.mixing_manipulator import _device_ops as D
    dev = torch.device("cuda:0")
    rs = D.Resampler.get(RATE_IN, RATE_OUT)
    up, down, half, T = rs.info()
    x = (0.3 * torch.randn(1, N_IN, C, generator=torch.Generator().manual_seed(0))).clamp_(-1, 1)
    xd = x.to(dev)
    n_out = rs.length(N_IN)
    for _ in range(3):
        y = rs.forward(xd)
    torch.cuda.synchronize()
    if a.kernel_only:
        for _ in range(a.kernel_only):
            rs.forward(xd)
        torch.cuda.synchronize()
        return
    times = []
    for _ in range(a.rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.steps):
            rs.forward(xd)
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e) / a.steps)
    from scipy.signal import resample_poly
    x64 = x[0].numpy().astype(np.float64)
    t0 = time.perf_counter()
    ref = resample_poly(x64, up, down, axis=0, window=rs.taps().astype(np.float64) / up)
    host_ms = (time.perf_counter() - t0) * 1e3
    ms = statistics.median(times)
    nbytes = (N_IN + n_out) * C * 4
    print(json.dumps({"metric": "polyphase resampler, ms per call", "rate_in": RATE_IN, "rate_out": RATE_OUT, "up": up, "down": down,
                      "taps_per_phase": T, "frames_in": N_IN, "frames_out": n_out, "channels": C, "rounds": a.rounds, "steps": a.steps,
                      "device_ms": ms, "device_ms_min_max": [min(times), max(times)], "bytes_moved": nbytes,
                      "achieved_GBps": nbytes / (ms * 1e-3) / 1e9, "multiply_adds": n_out * C * T,
                      "achieved_f64_GFMAps": n_out * C * T / (ms * 1e-3) / 1e9, "host_resample_poly_ms": host_ms, "host_over_device": host_ms / ms,
                      "max_abs_diff_to_host_float64": float(np.abs(y[0].cpu().numpy() - ref).max())}))


if __name__ == "__main__":
    main()
