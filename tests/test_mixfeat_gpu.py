"""The mixing-feature kernels on the MI355X against the float64 restatement (tests/mixfeat_ref.py) within the derived bounds: every
kernel form and the three Python functions at the length of a 3-minute stem and on the committed real stems, a batch of 32 segments,
bit identity from run to run / alone / in a batch, inference/evaluate.py --metrics end to end.  Each check prints its max err / bound
(the table of DESIGN.md 5)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import mixfeat_ref as R  # noqa: E402
import real_audio as RA  # noqa: E402
from mss_ref import _stem  # noqa: E402

pytestmark = pytest.mark.gpu

from mixfeat_checks import check_features, check_frames, ratio  # noqa: E402
from music_mixing_style_transfer_amd.mixing_manipulator import _device_ops as D  # noqa: E402
from music_mixing_style_transfer_amd.mixing_manipulator import utils_data_normalization as U  # noqa: E402

DEV = "cuda:0"
STEM = 7_938_000          # 3 minutes at 44.1 kHz
GOLD = np.load(os.path.join(HERE, "golden", "mixfeat.npz"))


def _real_pair(stem):
    z = np.load(os.path.join(HERE, "golden", "real_audio.npz"))
    a, b = _stem(z, "input", stem).T, _stem(z, "reference", stem).T
    n = min(len(a), len(b))
    return np.ascontiguousarray(a[:n]), np.ascontiguousarray(b[:n])


@pytest.mark.parametrize("name", R.CASES)
def test_golden_cases_on_the_device(name):
    """the golden cases at their own lengths: kernels against the restatement, functions against the REAL reference's dictionaries"""
    out, tar, sr, n_fft, hop = R.case_inputs(name)
    check_frames(name, tar if name != "mono" else out, sr, n_fft, hop, DEV)
    worst = check_features(name, out, tar, sr, n_fft, hop, DEV, golden={k: GOLD[f"{name}/{k}"] for k in ("loudness", "panning", "dynamic")})
    if name == "identical":
        assert all(v == 0.0 for v in worst.values())


@pytest.mark.parametrize("name", ["noise_pan", "silence_gap", "compressed"])
def test_three_minute_stems(name):
    out, tar, sr, n_fft, hop = R.case_inputs(name, STEM)
    if name == "noise_pan":
        check_frames(name, tar, sr, n_fft, hop, DEV)
    check_features(name, out, tar, sr, n_fft, hop, DEV)


@pytest.mark.parametrize("stem", ["drums", "bass"])
def test_whole_real_stems(stem):
    """the committed stems from end to end (15 s): the `input` stem against the `reference` stem"""
    out, tar = _real_pair(stem)
    check_frames(f"real_{stem}", tar, 44100, 2048, 1024, DEV)
    check_features(f"real_{stem}", out, tar, 44100, 2048, 1024, DEV)


def test_batch_of_32_segments_and_bit_identity():
    rng = np.random.default_rng(7)
    base = R.case_inputs("noise_pan", 131072)[1]
    xs = np.stack([np.roll(base, 997 * i, axis=0) * np.float32(10.0 ** rng.uniform(-3.0, 0.0)) for i in range(32)]).astype(np.float32)
    xs[5, :, 1] = xs[5, :, 0]
    xs[6, 40000:60000] = 0.0
    xd = torch.from_numpy(xs).to(DEV)
    gain = np.asarray([R.peak_gain(x) for x in xs], dtype=np.float32)
    sr, n_fft, hop = 44100, 2048, 1024
    mf = D.MixFeat.get(n_fft, hop)
    bands = R.band_bins(sr, n_fft)
    low = U._lowpass_batch(xd, 1000, sr)
    forms = {"panning": lambda x, g, i: mf.panning(x, bands, g), "low_ratio": lambda x, g, i: mf.low_ratio(low[i], x, g, g),
             "dynamics": lambda x, g, i: D.frame_dynamics(x, n_fft, hop, g), "dynamics_direct": lambda x, g, i: D.frame_dynamics(x, n_fft, hop - 1, g)}
    for what, fn in forms.items():
        a = fn(xd, gain, slice(None))
        assert np.array_equal(a, fn(xd, gain, slice(None))), what
        for i in (0, 5, 6, 17, 31):
            assert np.array_equal(fn(xd[i:i + 1], gain[i:i + 1], slice(i, i + 1))[0], a[i]), (what, i)
    phi, sps = mf.sps(xd, gain)
    phi2, sps2 = mf.sps(xd[17:18], gain[17:18])
    assert torch.equal(phi[17], phi2[0]) and torch.equal(sps[17], sps2[0]) and bool((sps[5] == 0).all())
    assert torch.equal(U._lowpass_batch(xd[17:18], 1000, sr)[0], low[17])
    S = mf.panning(xd, bands, gain)
    assert np.all(S[5] == 0.0) and np.all(S[6, 40:57] == 0.0)
    worst = 0.0
    for i in (0, 6, 17, 31):
        f = R.panning_frames(R.peak_normalize(xs[i]), sr, n_fft, hop)
        worst = max(worst, ratio(np.abs(S[i] - f["S"]), f["dS"]))
    print(f"32 x 131072 x 2: max band-sum err / bound = {worst:.4g}")
    assert worst <= 1.0


def test_device_tensors_stay_on_the_device():
    out, tar, sr, n_fft, hop = R.case_inputs("noise_pan")
    xd = torch.from_numpy(R.peak_normalize(tar)).to(DEV)
    sps_mean, phi_mean, sps, phi = U.get_SPS(xd, n_fft=n_fft, hop_length=hop, smooth=True, frames=True)
    assert sps.is_cuda and phi.is_cuda and isinstance(sps_mean, np.ndarray) and sps_mean.shape == (n_fft // 2 + 1,)
    y = U.lowpassFiltering(xd, 1000, sr)
    assert y.is_cuda and y.shape == xd.shape
    with pytest.raises(RuntimeError, match="no CPU path"):
        D.MixFeat.get(n_fft, hop).sps(torch.from_numpy(tar)[None])
    a = U.compute_dynamic_features((torch.from_numpy(out).to(DEV), xd, 0, sr, n_fft, hop))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        b = U.compute_dynamic_features((torch.from_numpy(out).to(DEV), xd, 0, sr, n_fft, hop))
    s.synchronize()
    assert a == b


def test_evaluate_cli_with_feature_metrics(tmp_path):
    z = np.load(os.path.join(HERE, "golden", "real_audio.npz"))
    n = 300000
    a, b = RA.unpack(z["pcm/input/drums"])[:n], RA.unpack(z["pcm/reference/drums"])[:n]
    RA.write_wav(tmp_path / "a.wav", a)
    RA.write_wav(tmp_path / "b.wav", b)
    cmd = [sys.executable, "-m", "music_mixing_style_transfer_amd.inference.evaluate", "--est", str(tmp_path / "a.wav"), "--target",
           str(tmp_path / "b.wav"), "--segment_length", "131072"]
    runs = [subprocess.run(cmd + extra, cwd=REPO, capture_output=True, text=True, timeout=900)
            for extra in ([], ["--metrics", "mss"], ["--metrics", "mss,loudness,panning,dynamic"], ["--metrics", "mss,loudness,panning,dynamic"])]
    for r in runs:
        assert r.returncode == 0, r.stderr
    assert runs[0].stdout == runs[1].stdout and runs[2].stdout == runs[3].stdout          # the default line; run-to-run bit identity
    plain, full = json.loads(runs[0].stdout), json.loads(runs[2].stdout)
    assert list(plain) == ["metric", "mean", "n_segments", "segments", "segment_length", "sample_rate"]
    assert {k: v for k, v in full.items() if k != "features"} == plain
    fa, fb = ((v.astype(np.float64) / 32768.0).astype(np.float32) for v in (a, b))
    for title, ref in (("loudness", R.loudness_features(fa, fb, 44100)), ("panning", R.panning_features(fa, fb, 44100, 2048, 1024)),
                       ("dynamic", R.dynamic_features(fa, fb, 44100, 2048, 1024))):
        exact, bound = ref[0], ref[1]
        for k in exact:
            got = full["features"][title][k]
            print(f"evaluate {title}.{k}: {got:.12g} (float64 {exact[k]:.12g}, bound {bound[k]:.3g})")
            assert abs(got - exact[k]) <= bound[k] + 8 * R.EPS64 * abs(exact[k]), (title, k)
