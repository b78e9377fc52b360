#!/usr/bin/env python
"""Randomised augmentation as one batch: AugmentationChain.call_items against today's route to the same result and against the
shared-parameter chain, on one MI355X.  64 segments of [131072, 2] through EQ -> rms -> compressor -> rms -> imager -> rms -> gain
(BASELINE configs[3]'s processors, probability 1, parameters randomised), a fresh seeded draw per call:
  (a) chain.call_items(x)                      item i with its own draw, batched per processor
  (b) [chain([x[i]])[0] for i in range(64)]    the same result today: 64 calls with one item
  (c) chain([x])                               one draw for the whole batch: the work of bench.py's fx_chain leg
HIP events around each call, the three alternating in one process, ROUNDS rounds of CALLS calls after a warm-up; prints one JSON object
(median, minimum and maximum of the per-round means, in ms per call) and writes it to --out.  With --builder-only the process runs the
equaliser's per-item call alone, for a kernel trace of its own (the table builder's time)."""
import argparse
import json
import os
import random
import statistics
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def make_chain():
    from music_mixing_style_transfer_amd.mixing_manipulator import AugmentationChain, Compressor, Equaliser, Gain, MidSideImager
    return AugmentationChain(fxs=[(Equaliser(2, 44100), 1.0, True), (Compressor(44100), 1.0, True), (MidSideImager(), 1.0, True), (Gain(), 1.0, False)],
                             randomize_param_value=True)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--length", type=int, default=131072)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--builder-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    x = (0.1 * torch.randn(a.items, a.length, 2, generator=torch.Generator().manual_seed(0))).clamp_(-1, 1).to(dev)
    chain = make_chain()
    random.seed(0)
    np.random.seed(0)
    if a.builder_only:
        eq = chain.fxs[0][0]
        from music_mixing_style_transfer_amd.mixing_manipulator.common_audioeffects import parameter_values
        for _ in range(a.calls):
            values = []
            for _ in range(a.items):
                eq.randomize()
                values.append(parameter_values(eq))
            eq.process_items(x, values)
        torch.cuda.synchronize()
        return
    legs = {"call_items": lambda: chain.call_items(x),
            "loop_of_single_items": lambda: [chain([x[i]])[0] for i in range(a.items)],
            "shared_parameters": lambda: chain([x])}
    for fn in legs.values():          # warm-up: per-device tables, streams, allocator
        fn()
        fn()
    torch.cuda.synchronize()
    means = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            means[k].append(statistics.mean(timed(fn) for _ in range(a.calls)))
    res = {"workload": f"{a.items} x [{a.length}, 2]: EQ -> rms -> compressor -> rms -> imager -> rms -> gain, probability 1, randomised parameters",
           "rounds": a.rounds, "calls_per_round": a.calls, "unit": "ms per call (HIP events), median / min / max of the per-round means",
           "device": torch.cuda.get_device_name(0)}
    for k, v in means.items():
        res[k] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    res["call_items_over_loop"] = round(res["call_items"]["median"] / res["loop_of_single_items"]["median"], 4)
    res["call_items_over_shared"] = round(res["call_items"]["median"] / res["shared_parameters"]["median"], 4)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
