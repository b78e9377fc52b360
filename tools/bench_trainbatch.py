#!/usr/bin/env python
"""A training batch on the device: MUSDB_Dataset_Mixing_Manipulated_Style_Transfer.get_batch against the item loop on the same build, on one
MI355X.  Synthetic stems written to a temporary directory (FILES files of SECONDS s of 16-bit noise per instrument) and the synthetic impulse
responses of bench_fx_items.py --chain inst; the dataset at segment_length_ref = SEGMENT with pad_b4_manipulation, 'full' mode with the default
probability tables, BATCH indices per batch:
  (a) ds.get_batch(indices)            the draws of the batch, then per instrument one gather and one call_plans, then one finishing launch
  (b) [ds[i] for i in indices]         the same items today: segments cut on the host, one chain call per item and instrument, torch ops
Host wall clock from a device synchronise to a device synchronise (the host plan is part of the cost), the two legs alternating in one
process, a fresh random_seed per round (both legs draw the same parameters), ROUNDS rounds after WARMUP warm-up rounds.  Separately: the host
plan alone (the draws of a batch, no audio), and the gather launch (one instrument's 2 BATCH rows out of the resident bank) and the finishing
launch (all 12 BATCH rows) alone with HIP events, with the bytes they move over that time.  Prints one JSON object and writes it to --out."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import wave

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
ORDER = "eqcompimagegain"


def write_stems(root, files, seconds, rate=44100):
    d = os.path.join(root, "val")
    os.makedirs(d)
    rng = np.random.default_rng(0)
    n = int(seconds * rate)
    env = (0.05 + 0.3 * np.exp(-(np.arange(n) % 22050) / 6000.0))[:, None]
    for inst in ("drums", "bass", "other", "vocals"):
        for k in range(files):
            pcm = np.clip(np.rint(rng.standard_normal((n, 2), dtype=np.float32) * env * 32767), -32768, 32767).astype("<i2")
            with wave.open(os.path.join(d, f"{inst}_normalized_{ORDER}_silence_trimmed_{k}.wav"), "w") as w:
                w.setnchannels(2)
                w.setsampwidth(2)
                w.setframerate(rate)
                w.writeframes(pcm.tobytes())
    return root + "/"


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def event_ms(fn, calls=20):
    fn()
    times = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segment", type=int, default=131072)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--files", type=int, default=8)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_trainbatch.py measures on the MI355X: no GPU is visible"
    import bench_fx_items
    from music_mixing_style_transfer_amd.data_loader import MUSDB_Dataset_Mixing_Manipulated_Style_Transfer, batch_finish
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as tmp:
        bench_fx_items.make_inst_chain(os.path.join(tmp, "ir"))          # writes the synthetic responses
        args = argparse.Namespace(data_dir=write_stems(os.path.join(tmp, "musdb"), a.files, a.seconds), using_dataset="musdb", use_normalized=True,
                                  normalization_order=ORDER, random_seed=1, pad_b4_manipulation=True, ir_dir_path=os.path.join(tmp, "ir", "IR_"),
                                  sample_rate=44100, segment_length=a.segment, segment_length_ref=a.segment, num_strong_negatives=1,
                                  batch_size_total=a.batch, reference_length=a.segment)
        legs = {"get_batch": MUSDB_Dataset_Mixing_Manipulated_Style_Transfer(args, "val", device=dev),
                "item_loop": MUSDB_Dataset_Mixing_Manipulated_Style_Transfer(args, "val", device=dev)}
        indices = list(range(1, a.batch + 1))
        run = {"get_batch": lambda ds: ds.get_batch(indices), "item_loop": lambda ds: [ds[i] for i in indices]}
        times, plan = {k: [] for k in legs}, []
        for r in range(a.warmup + a.rounds):
            for k, ds in legs.items():
                ds.fixed_random_seed = 1000 + r          # val mode seeds item idx with idx * random_seed: fresh draws per round, the same for both legs
                t = wall_ms(lambda: run[k](ds))
                if r >= a.warmup:
                    times[k].append(t)
            if r >= a.warmup:
                t0 = time.perf_counter()
                [legs["get_batch"]._draw_item(i) for i in indices]
                plan.append((time.perf_counter() - t0) * 1e3)
        ds = legs["get_batch"]
        bank, frames = ds._bank("drums"), ds.load_duration
        rng = np.random.default_rng(1)
        files = rng.integers(0, a.files, 2 * a.batch)
        starts = rng.integers(0, int(a.seconds * 44100) - frames, 2 * a.batch)
        gather_ms = event_ms(lambda: bank.gather(files, starts, frames))
        x = torch.randn(16 * a.batch, frames, 2, device=dev)
        rows = rng.permutation(16 * a.batch)[:12 * a.batch]
        finish_ms = event_ms(lambda: batch_finish(x, rows, [2048] * len(rows), a.segment))
    gather_bytes = 2 * a.batch * frames * (2 * 2 + 2 * 4)          # 16-bit stereo frames in, float32 stereo frames out
    finish_bytes = 12 * a.batch * a.segment * 2 * 4 * 2             # float32 stereo in and out
    res = {"workload": f"Style_Transfer dataset, 'full' mode, default probabilities, 4 x {a.files} stems of {a.seconds:g} s, segment_length_ref {a.segment} "
                       f"with pad_b4_manipulation, {a.batch} indices per batch (items of 12 x [2, {a.segment}])",
           "rounds": a.rounds, "warmup_rounds": a.warmup, "device": torch.cuda.get_device_name(0),
           "unit": "ms per batch, host wall clock between device synchronises; median / min / max over the rounds",
           "get_batch": spread(times["get_batch"]), "item_loop": spread(times["item_loop"]), "host_plan": spread(plan),
           "get_batch_ms": round(statistics.median(times["get_batch"]), 3), "item_loop_ms": round(statistics.median(times["item_loop"]), 3),
           "host_plan_ms": round(statistics.median(plan), 3),
           "get_batch_over_item_loop": round(statistics.median(times["get_batch"]) / statistics.median(times["item_loop"]), 4),
           "gather_ms": round(gather_ms, 4), "gather_gb_s": round(gather_bytes / gather_ms / 1e6, 1),
           "finish_ms": round(finish_ms, 4), "finish_gb_s": round(finish_bytes / finish_ms / 1e6, 1),
           "launch_note": "gather_ms / finish_ms: HIP events around one StemBank.gather (2 x batch rows) / one batch_finish (12 x batch rows) call, "
                          "table upload and output allocation included; GB/s = bytes read + written over that time"}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
