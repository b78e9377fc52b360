#!/usr/bin/env python
"""Seam-free conversion against segment mode on one MI355X: one stem pair (input and reference, 7 938 000 samples = three minutes at
44.1 kHz, device-resident) through StyleTransferEngine.transfer_stem with the default networks, synthetic weights, HIP events.
Three modes alternate in one process after all have been warmed: seam-free at --window (default 2**21), segment mode at 131072-sample
segments (the headline configuration) and at 2**19 (the reference's default).  The reference embedding is the same work in all three, so
the MixFXcloner part alone (convert_stem / convert_stem_seamless with the embedding given) is timed the same way beside it.

From the code alone the seam-free cost is the halo share, 1 + 2 H / W = 1.109 at W = 2**21, times the loss of the whole-sequence tile forms
and the fused tail that exist only at L = 131072: about 0.85 of segment-mode throughput.  Prints ONE JSON line with the median round of each
mode, the spread, the ratios and the box's calib_ms (mst_calib_mainloop: the bare bf16 main loop, for comparing boxes).

    python tools/bench_seamless.py [--length 7938000] [--window 2097152] [--precision bf16] [--rounds 5] [--steps 2]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch
import yaml

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=int, default=7938000)
    ap.add_argument("--window", type=int, default=1 << 21)
    ap.add_argument("--precision", default="bf16", choices=["fp32", "bf16", "bf16x3"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_seamless.py measures on the MI355X; no GPU is visible and there is no CPU path")
    from music_mixing_style_transfer_amd import _lib
    from music_mixing_style_transfer_amd.inference import StyleTransferEngine, build_models
    from music_mixing_style_transfer_amd.utils import synth
    dev = torch.device("cuda:0")
    with open(os.path.join(REPO, "music_mixing_style_transfer_amd", "networks", "configs.yaml")) as f:
        cfgs = yaml.full_load(f)
    enc_cfg, tcn_cfg = cfgs["Effects_Encoder"]["default"], cfgs["TCN"]["default"]
    enc, tcn = build_models({k: (list(v) if isinstance(v, list) else v) for k, v in enc_cfg.items()}, tcn_cfg, dev, a.precision)
    enc.load_state_dict(synth.fxencoder_state_dict(enc_cfg, seed=0))
    tcn.load_state_dict(synth.tcn_state_dict(seed=0))
    eng = StyleTransferEngine(enc, tcn)
    x = synth.synth_music(2, a.length, seed=1).to(dev)
    ref = synth.synth_music(2, a.length, seed=2).to(dev)
    emb = eng.stem_embedding(ref, 131072, 131072)
    h_l, h_r = tcn.context()
    modes = {
        "seamless": (lambda: eng.transfer_stem(x, ref, 131072, 131072, seamless=True, window=a.window),
                     lambda: eng.convert_stem_seamless(x, emb, window=a.window)),
        "segments_131072": (lambda: eng.transfer_stem(x, ref, 131072, 131072), lambda: eng.convert_stem(x, emb, 131072)),
        "segments_524288": (lambda: eng.transfer_stem(x, ref, 1 << 19, 1 << 19), lambda: eng.convert_stem(x, emb, 1 << 19)),
    }
    for whole, conv in modes.values():
        for _ in range(2):
            whole()
            conv()
    torch.cuda.synchronize()

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.steps):
            fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) / a.steps

    ms = {k: ([], []) for k in modes}
    for _ in range(a.rounds):          # alternating: a drift of the clock or a neighbour on the box hits all three
        for k, (whole, conv) in modes.items():
            ms[k][0].append(timed(whole))
            ms[k][1].append(timed(conv))
    lib = _lib.lib()
    calib, sclk = C.c_float(0), C.c_float(0)
    lib.check(lib.mst_calib_mainloop(20, C.byref(calib), C.byref(sclk), lib.stream_ptr(x)), "mst_calib_mainloop")
    y_seam = eng.convert_stem_seamless(x, emb, window=a.window)[0]
    out = {"metric": "one stem pair through transfer_stem, ms", "length": a.length, "precision": a.precision, "window": a.window,
           "context": [h_l, h_r], "halo_share": 1.0 + (h_l + h_r) / a.window, "rounds": a.rounds, "steps": a.steps,
           "calib_ms": calib.value, "sclk_mhz": sclk.value}
    for k, (whole, conv) in ms.items():
        out[k] = {"pair_ms": statistics.median(whole), "pair_ms_min_max": [min(whole), max(whole)], "convert_ms": statistics.median(conv),
                  "convert_ms_min_max": [min(conv), max(conv)], "convert_samples_per_s": a.length / (statistics.median(conv) * 1e-3)}
    for k in ("segments_131072", "segments_524288"):
        out[f"throughput_vs_{k}"] = {"pair": out[k]["pair_ms"] / out["seamless"]["pair_ms"],
                                     "convert": out[k]["convert_ms"] / out["seamless"]["convert_ms"]}
        y_seg = eng.convert_stem(x, emb, int(k.split("_")[1]))[0]
        out[f"max_abs_difference_from_{k}"] = float((y_seam - y_seg).abs().max())          # what the segment seams cost in the audio
    out["output_rms"] = float(y_seam.pow(2).mean().sqrt())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
