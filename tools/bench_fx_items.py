#!/usr/bin/env python
"""Randomised augmentation as one batch: AugmentationChain.call_items against today's route to the same result and against the
shared-parameter chain, on one MI355X.  64 segments of [131072, 2] through EQ -> rms -> compressor -> rms -> imager -> rms -> gain
(BASELINE configs[3]'s processors, probability 1, parameters randomised), a fresh seeded draw per call:
  (a) chain.call_items(x)                      item i with its own draw, batched per processor
  (b) [chain([x[i]])[0] for i in range(64)]    the same result today: 64 calls with one item
  (c) chain([x])                               one draw for the whole batch: the work of bench.py's fx_chain leg
HIP events around each call, the three alternating in one process, ROUNDS rounds of CALLS calls after a warm-up; prints one JSON object
(median, minimum and maximum of the per-round means, in ms per call) and writes it to --out.  With --builder-only the process runs the
equaliser's per-item call alone, for a kernel trace of its own (the table builder's time).
--chain inst: the "vocals" instrument chain instead (create_inst_effects_augmentation_chain, every probability 1): shuffled EQ / compressor,
shuffled panner / imager, the convolution reverb in a parallel branch, gain - over a synthetic impulse-response directory the tool writes
itself (decaying stereo noise, RT60 0.3 ... 3 s, two responses per RT60 group); legs (a) and (b) only.  The record names the transform size the
batch's convolver ended up with."""
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


IR_SECONDS = {"300-600": (0.3, 0.5), "600-1200": (0.8, 1.0), "1200-3000": (1.5, 2.5), "3000-6000": (3.0,)}


def make_inst_chain(ir_root):
    """the "vocals" FX manipulator over synthetic impulse responses written below ir_root: noise whose envelope falls 60 dB in the RT60"""
    from music_mixing_style_transfer_amd.data_loader import save_wav_pcm16
    from music_mixing_style_transfer_amd.mixing_manipulator.audio_effects_chain import create_inst_effects_augmentation_chain
    rng = np.random.default_rng(0)
    for group, seconds in IR_SECONDS.items():
        for k, sec in enumerate(seconds):
            d = os.path.join(ir_root, "IR_set1", "RT60_avg", group, f"room{k}")
            os.makedirs(d, exist_ok=True)
            n = int(sec * 44100)
            h = rng.standard_normal((n, 2)) * np.power(10.0, -3.0 * np.arange(n) / n)[:, None] * 0.5
            save_wav_pcm16(os.path.join(d, "impulse_response.wav"), h.astype(np.float32))
    probs = {"eq": 1, "comp": 1, "pan": 1, "imager": 1, "reverb": 1, "gain": 1}
    return create_inst_effects_augmentation_chain("vocals", probs, ir_dir_path=os.path.join(ir_root, "IR_"))


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
    ap.add_argument("--chain", choices=["config4", "inst"], default="config4")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    x = (0.1 * torch.randn(a.items, a.length, 2, generator=torch.Generator().manual_seed(0))).clamp_(-1, 1).to(dev)
    tmp = None
    if a.chain == "inst":
        import tempfile
        tmp = tempfile.TemporaryDirectory()
        chain = make_inst_chain(tmp.name)
    else:
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
    if a.chain == "inst":
        del legs["shared_parameters"]
    for fn in legs.values():          # warm-up: per-device tables, streams, allocator
        fn()
        fn()
    torch.cuda.synchronize()
    means = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            means[k].append(statistics.mean(timed(fn) for _ in range(a.calls)))
    what = ("EQ -> rms -> compressor -> rms -> imager -> rms -> gain" if a.chain == "config4" else
            "the vocals instrument chain (shuffled EQ / compressor, shuffled panner / imager, parallel convolution reverb over synthetic responses of 0.3 ... 3 s, gain)")
    res = {"workload": f"{a.items} x [{a.length}, 2]: {what}, probability 1, randomised parameters",
           "rounds": a.rounds, "calls_per_round": a.calls, "unit": "ms per call (HIP events), median / min / max of the per-round means",
           "device": torch.cuda.get_device_name(0)}
    for k, v in means.items():
        res[k] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    res["call_items_over_loop"] = round(res["call_items"]["median"] / res["loop_of_single_items"]["median"], 4)
    if "shared_parameters" in res:
        res["call_items_over_shared"] = round(res["call_items"]["median"] / res["shared_parameters"]["median"], 4)
    if a.chain == "inst":
        from music_mixing_style_transfer_amd.mixing_manipulator import ConvolutionalReverb
        rv = next(fx for fx in chain._processors() if isinstance(fx, ConvolutionalReverb))
        res["convolver_transform_size"] = getattr(rv, "last_n_fft", None)          # of the last call_items batch; None: a build that convolves item by item
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
