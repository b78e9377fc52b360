"""Score a transfer against a target on the MI355X:

    python -m music_mixing_style_transfer_amd.inference.evaluate --est A.wav --target B.wav [--segment_length N] [--mode midside|ori] [--json OUT]
                                                                 [--metrics mss,loudness,panning,dynamic,spectral] [--feature_fft 2048] [--feature_hop 1024]

The multi-scale spectral distance of modules/loss.py between the two files, cut into whole segments (a remainder shorter than a
segment is dropped; a file shorter than one segment is one segment).  --est / --target may be two directories: every wav file of --est
is scored against the file of the same name in --target.  Prints ONE JSON line: the mean over all segments and the per-segment values.

--metrics adds the reference's audio-feature errors (mixing_manipulator/utils_data_normalization.py compute_loudness_features /
compute_panning_features / compute_dynamic_features / compute_spectral_features) of every file pair, over the whole file, under the key
"features"; with the default, "mss", the line is what it always was.  "spectral" needs 800 frames of --feature_fft / --feature_hop (the
reference's running mean of the flatness): a shorter file is refused."""
import argparse
import json
import os
import sys

import torch

from ..data_loader.loader_utils import load_wav_segment, read_wav_raw
from ..modules.loss import MultiScale_Spectral_Loss_MidSide_DDSP

METRICS = ("mss", "loudness", "panning", "dynamic", "spectral")


def _load(path):
    rate, width, nch, n, raw = read_wav_raw(path)
    x = load_wav_segment(path, axis=0, sample_rate=rate, preread={path: (rate, width, nch, n, raw)})
    if nch == 1:
        x = x[None, :]
    return rate, nch, torch.from_numpy(x.astype("float32"))


def segments(est, tgt, segment_length):
    """[2, L] x 2 -> [n, 2, S] x 2"""
    L = est.shape[-1]
    S = L if L < segment_length else segment_length
    n = max(1, L // S)
    cut = lambda x: x[:, :n * S].reshape(2, n, S).permute(1, 0, 2).contiguous()
    return cut(est), cut(tgt)


def feature_errors(e, t, rate, metrics, n_fft, hop, device):
    """e, t [2, L] -> {"loudness": {...}, "panning": {...}, "dynamic": {...}, "spectral": {...}} for the metrics asked for: the whole
    file, not segments"""
    from ..mixing_manipulator import utils_data_normalization as U
    args = (e.t().contiguous().to(device), t.t().contiguous().to(device), 0, rate, n_fft, hop, 2)
    fns = {"loudness": U.compute_loudness_features, "panning": U.compute_panning_features, "dynamic": U.compute_dynamic_features,
           "spectral": U.compute_spectral_features}
    return {m: {k: float(v[0]) for k, v in fns[m](args).items()} for m in METRICS[1:] if m in metrics}


def score_pair(est_path, tgt_path, loss, segment_length, device, batch=32, metrics=("mss",), feature_fft=2048, feature_hop=1024):
    (re, ce, e), (rt, ct, t) = _load(est_path), _load(tgt_path)
    if re != rt or ce != ct or e.shape != t.shape:
        raise ValueError(f"{est_path} and {tgt_path} differ in rate, channels or length: ({re} Hz, {ce} ch, {e.shape[-1]} samples) "
                         f"against ({rt} Hz, {ct} ch, {t.shape[-1]} samples)")
    if ce != 2:
        raise ValueError(f"{est_path}: stereo files expected, got {ce} channel(s)")
    features = feature_errors(e, t, re, metrics, feature_fft, feature_hop, device)
    if "mss" not in metrics:
        return {"est": est_path, "target": tgt_path, "sample_rate": re, "features": features}
    es, ts = segments(e, t, segment_length)
    values = []
    for i in range(0, es.shape[0], batch):
        v = loss.terms(es[i:i + batch].to(device), ts[i:i + batch].to(device))          # [b, scale, channel, term]
        ch = loss.mid_weight * v[:, :, 0, :] + (1.0 - loss.mid_weight) * v[:, :, 1, :]
        per = (1.0 - loss.logmag_weight) * ch[:, :, 0].sum(dim=1) + loss.logmag_weight * ch[:, :, 1].sum(dim=1)
        values += [float(x) for x in per.cpu()]
    out = {"est": est_path, "target": tgt_path, "sample_rate": re, "segment_length": int(es.shape[-1]), "segments": values,
           "mean": sum(values) / len(values)}
    if features:
        out["features"] = features
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--est", required=True)
    ap.add_argument("--target", required=True)
    ap.add_argument("--segment_length", type=int, default=2 ** 19)
    ap.add_argument("--mode", choices=["midside", "ori"], default="midside")
    ap.add_argument("--json", default=None, help="also write the result to this file")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--metrics", default="mss", help="comma list out of " + ",".join(METRICS))
    ap.add_argument("--feature_fft", type=int, default=2048, help="frame length of the feature metrics")
    ap.add_argument("--feature_hop", type=int, default=1024)
    a = ap.parse_args(argv)
    if a.segment_length < 1:
        ap.error("--segment_length must be positive")
    metrics = tuple(m for m in a.metrics.split(",") if m)
    if not metrics or any(m not in METRICS for m in metrics):
        ap.error(f"--metrics takes a comma list out of {','.join(METRICS)}, got {a.metrics!r}")
    if os.path.isdir(a.est) != os.path.isdir(a.target):
        ap.error("--est and --target must both be files or both be directories")
    if os.path.isdir(a.est):
        names = sorted(f for f in os.listdir(a.est) if f.lower().endswith(".wav"))
        missing = [f for f in names if not os.path.isfile(os.path.join(a.target, f))]
        if not names or missing:
            ap.error(f"no wav files in {a.est}" if not names else f"{a.target} lacks {missing}")
        pairs = [(os.path.join(a.est, f), os.path.join(a.target, f)) for f in names]
    else:
        pairs = [(a.est, a.target)]
    loss = MultiScale_Spectral_Loss_MidSide_DDSP(mode=a.mode)
    TooFewFrames = ()          # the feature module is imported only where a feature metric asks for it
    if "spectral" in metrics:
        from ..mixing_manipulator.utils_data_normalization import TooFewFrames
    try:
        files = [score_pair(e, t, loss, a.segment_length, torch.device(a.device), metrics=metrics, feature_fft=a.feature_fft,
                            feature_hop=a.feature_hop) for e, t in pairs]
    except TooFewFrames as err:
        ap.error(str(err))
    if "mss" in metrics:
        allv = [v for f in files for v in f["segments"]]
        out = {"metric": "multi_scale_spectral_" + a.mode, "mean": sum(allv) / len(allv), "n_segments": len(allv)}
    else:
        out = {"metric": "audio_features"}
    if len(files) == 1:
        out.update({k: files[0][k] for k in ("segments", "segment_length", "sample_rate", "features") if k in files[0]})
    else:
        out["files"] = files
    line = json.dumps(out)
    print(line)
    if a.json:
        with open(a.json, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
