"""The mixing-feature kernels (csrc/mixfeat_kernels.h) on the CPU SIMT emulator: every kernel form against the float64 restatement
within the derived bounds (tests/mixfeat_ref.py), exact zeros where the arithmetic promises them, bit identity alone and in a batch, the
Python functions against the REAL reference's dictionaries (tests/golden/mixfeat.npz), the command line, every refusal."""
import ctypes as C
import io
import json
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import mixfeat_ref as R  # noqa: E402
import real_audio as RA  # noqa: E402
from mixfeat_checks import check_features, check_frames, ratio  # noqa: E402

from music_mixing_style_transfer_amd import _lib  # noqa: E402
from music_mixing_style_transfer_amd.mixing_manipulator import _device_ops as D  # noqa: E402
from music_mixing_style_transfer_amd.mixing_manipulator import utils_data_normalization as U  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "mixfeat.npz"))


@pytest.mark.parametrize("name", R.CASES)
def test_every_kernel_form_within_the_bound(emu_default, name):
    out, tar, sr, n_fft, hop = R.case_inputs(name)
    cut = 12 * hop + n_fft + 321          # a short stretch (13 frames and a remainder): the emulator runs one fiber per thread
    check_frames(name, tar[:cut] if name != "mono" else out[:cut], sr, n_fft, hop)


@pytest.mark.parametrize("n_fft,hop", [(1024, 512), (1024, 300), (4096, 4096), (512, 100)])
def test_other_frame_sizes_and_hops(emu_default, n_fft, hop):
    x = R.case_inputs("noise_pan")[1][:3 * n_fft + 777]
    check_frames(f"noise {n_fft}/{hop}", x, R.SR, n_fft, hop)


def test_silence_gives_exactly_zero_and_mono_gives_sps_zero(emu_default):
    out, tar, sr, n_fft, hop = R.case_inputs("silence_gap")
    lo = len(tar) // 3 - 4 * hop
    x = tar[lo:lo + 14 * hop + n_fft]
    mf = D.MixFeat.get(n_fft, hop)
    gain = np.asarray([R.peak_gain(x)], dtype=np.float32)
    S = mf.panning(torch.from_numpy(x)[None], R.band_bins(sr, n_fft), gain)[0]
    silent = np.asarray([not np.any(x[t * hop:t * hop + n_fft]) for t in range(S.shape[0])])
    assert silent.sum() >= 3 and np.all(S[silent] == 0.0) and np.all(S[~silent][:, 0] > 0.0)
    sums = D.frame_dynamics(torch.from_numpy(x)[None], n_fft, hop, gain)[0]
    assert np.all(sums[:, silent, 0] == 0.0) and np.all(sums[:, silent, 1] == -600.0 * n_fft) and np.all(sums[:, silent, 2] == 0.0)
    rms, dyn, crest = U._dynamics_from_sums(sums, n_fft)
    assert np.all(rms[0, silent] == -600.0) and np.all(dyn[0, silent] == 0.0) and np.all(crest[0, silent] == 1.0)
    mono = R.case_inputs("mono")[0][:8 * hop + n_fft]
    phi, sps = mf.sps(torch.from_numpy(mono)[None])
    assert bool((sps == 0).all()) and bool((phi == 1).all())
    assert np.all(mf.panning(torch.from_numpy(mono)[None], R.band_bins(sr, n_fft))[0] == 0.0)
    sps_mean, phi_mean, _, _ = U.get_SPS(mono, n_fft=n_fft, hop_length=hop)
    assert np.all(sps_mean == 0.0) and np.all(phi_mean == 1.0)


def test_low_pass_through_a_stretch_of_silence(emu_default):
    """the whole silence_gap target: inside the gap the filter's tail falls from the signal's level through float32's range to nothing;
    the low-passed signal and the low ratio of every frame, the silent ones included, stay within their bounds"""
    out, tar, sr, n_fft, hop = R.case_inputs("silence_gap")
    xn = R.peak_normalize(tar)
    xd = torch.from_numpy(xn)[None]
    low = U._lowpass_batch(xd, 1000, sr)
    assert ratio(np.abs(low[0].numpy().astype(np.float64) - R.lowpass(xn, 1000, sr)), R.lowpass_sample_bound(xn, 1000, sr)) <= 1.0
    lr = R.low_ratio_frames(xn, sr, n_fft, hop)
    got = D.MixFeat.get(n_fft, hop).low_ratio(low, xd)[0]
    assert ratio(np.abs(got - lr["per_channel"]), lr["per_channel_bound"]) <= 1.0
    assert (lr["ratio"] < 1e-20).sum() >= 3          # frames wholly inside the gap


def test_bit_identical_alone_in_a_batch_and_from_run_to_run(emu_default):
    out, tar, sr, n_fft, hop = R.case_inputs("noise_pan")
    n = 9 * hop + n_fft + 5
    xs = torch.from_numpy(np.stack([tar[:n], out[:n], R.case_inputs("compressed")[0][:n], tar[1000:1000 + n]]))
    gain = np.asarray([0.9, 1.1, 2.0, 0.5], dtype=np.float32)
    mf = D.MixFeat.get(n_fft, hop)
    bands = R.band_bins(sr, n_fft)
    low = U._lowpass_batch(xs, 1000, sr)
    forms = {"panning": lambda x, g, i: mf.panning(x, bands, g), "sps": lambda x, g, i: torch.stack(mf.sps(x, g)).numpy(),
             "low_ratio": lambda x, g, i: mf.low_ratio(low[i], x, g, g), "dynamics": lambda x, g, i: D.frame_dynamics(x, n_fft, hop, g),
             "dynamics_direct": lambda x, g, i: D.frame_dynamics(x, n_fft, hop - 1, g)}
    for what, fn in forms.items():
        a, b = fn(xs, gain, slice(None)), fn(xs, gain, slice(None))
        assert np.array_equal(a, b), what
        a = np.moveaxis(a, 1, 0) if what == "sps" else a
        for i in range(xs.shape[0]):
            one = fn(xs[i:i + 1], gain[i:i + 1], slice(i, i + 1))
            one = one[:, 0] if what == "sps" else one[0]
            assert np.array_equal(one, a[i]), (what, i)
    assert torch.equal(U._lowpass_batch(xs[2:3], 1000, sr)[0], low[2])


@pytest.mark.parametrize("name", R.CASES)
def test_python_functions_against_the_reference_dictionaries(emu_default, name):
    out, tar, sr, n_fft, hop = R.case_inputs(name)
    gold = {k: GOLD[f"{name}/{k}"] for k in ("loudness", "panning", "dynamic")}
    worst = check_features(name, out, tar, sr, n_fft, hop, golden=gold)
    if name == "identical":
        assert all(v == 0.0 for v in worst.values())
        for fn in (U.compute_loudness_features, U.compute_panning_features, U.compute_dynamic_features):
            assert all(v[0] == 0.0 for v in fn((out, tar, 0, sr, n_fft, hop)).values())
    if name == "mono":
        assert all(U.compute_panning_features((out, tar, 0, sr, n_fft, hop))[k][0] == 1.0 for k in R.PANNING_KEYS)


def test_per_frame_sequences_against_the_reference(emu_default):
    """get_panning_rms(get_SPS), get_rms_dynamic_crest and get_low_freq_weighting as the reference calls them, on the peak-normalised target"""
    name = "noise_pan"
    out, tar, sr, n_fft, hop = R.case_inputs(name)
    xn = R.peak_normalize(tar)
    f, d, l = R.panning_frames(xn, sr, n_fft, hop), R.dynamics_frames(xn, n_fft, hop), R.low_ratio_frames(xn, sr, n_fft, hop)
    sps_mean, phi_mean, sps, phi = U.get_SPS(xn, n_fft=n_fft, hop_length=hop, smooth=False, frames=True)
    assert sps.dtype == np.float32 and sps.shape == (R.n_frames(len(xn), n_fft, hop), n_fft // 2 + 1)
    freqs = [[0, sr // 2], [0, 250], [250, 2500], [2500, sr // 2]]
    p = U.get_panning_rms(sps, freqs=freqs, sr=sr, n_fft=n_fft)
    own = np.abs(GOLD[f"{name}/p_rms_tar"] - f["p_rms"])
    # through the stored float32 SPS: one more rounding of every bin, 2^-24 relative to p_rms
    assert np.all(np.abs(p - GOLD[f"{name}/p_rms_tar"]) <= f["dp"] + own + 2.0 ** -23 * f["p_rms"])
    assert p[3, 1] == U.get_panning_rms_frame(sps[3], freqs=[0, 250], sr=sr, n_fft=n_fft)
    g_sps, g_phi = GOLD[f"{name}/sps_mean"].astype(np.float64), GOLD[f"{name}/phi_mean"].astype(np.float64)
    _, sps64, dq2 = R.sps_exact(xn, n_fft, hop)
    dmean = np.sqrt(dq2).mean(axis=0) + 2.0 ** -22          # d|SPS| <= sqrt(d(SPS^2)); the reference's float32 mean of float32 values
    assert np.all(np.abs(sps_mean - g_sps) <= dmean) and np.all(np.abs(phi_mean - g_phi) <= dmean)
    rms, dyn, crest = U.get_rms_dynamic_crest(xn, n_fft, hop)
    for got, key, row in ((rms, "rms", 0), (dyn, "dyn", 1), (crest, "crest", 2)):
        gold = GOLD[f"{name}/rdc_tar"][row]
        assert got.shape == (1, len(gold)) and np.all(np.abs(got[0] - gold) <= d["d_" + key] + np.abs(gold - d[key]) + 1e-12)
    low = U.get_low_freq_weighting(xn, sr, n_fft, hop, f0=1000)
    gold = GOLD[f"{name}/low_tar"]
    assert low.shape == (1, len(gold)) and np.all(np.abs(low[0] - gold) <= l["d_ratio"] + np.abs(gold - l["ratio"]))
    y = U.lowpassFiltering(xn, 1000, sr)
    assert isinstance(y, np.ndarray) and y.shape == xn.shape
    m, s = U.get_running_stats(np.arange(12.0).reshape(6, 2), [0, 1], N=3)
    assert np.allclose(m, [[2, 4, 6, 8], [3, 5, 7, 9]]) and np.allclose(s, np.sqrt(8.0 / 3.0))


def _wavs(tmp_path, n=70000):
    z = np.load(os.path.join(HERE, "golden", "real_audio.npz"))
    a, b = RA.unpack(z["pcm/input/drums"])[200000:200000 + n], RA.unpack(z["pcm/reference/drums"])[250000:250000 + n]
    RA.write_wav(tmp_path / "a.wav", a)
    RA.write_wav(tmp_path / "b.wav", b)
    return a, b


def _evaluate(argv):
    from music_mixing_style_transfer_amd.inference import evaluate
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert evaluate.main(argv) == 0
    return buf.getvalue()


def test_evaluate_default_line_is_unchanged_and_metrics_are_added(emu_default, tmp_path):
    from music_mixing_style_transfer_amd.inference import evaluate
    a, b = _wavs(tmp_path)
    base = ["--est", str(tmp_path / "a.wav"), "--target", str(tmp_path / "b.wav"), "--segment_length", "32768", "--device", "cpu"]
    line = _evaluate(base)
    # what the command printed before it knew of --metrics: these keys, in this order, from score_pair's values
    loss = evaluate.MultiScale_Spectral_Loss_MidSide_DDSP(mode="midside")
    f = evaluate.score_pair(str(tmp_path / "a.wav"), str(tmp_path / "b.wav"), loss, 32768, torch.device("cpu"))
    assert list(f) == ["est", "target", "sample_rate", "segment_length", "segments", "mean"]
    want = {"metric": "multi_scale_spectral_midside", "mean": sum(f["segments"]) / 2, "n_segments": 2, "segments": f["segments"],
            "segment_length": 32768, "sample_rate": 44100}
    assert line == json.dumps(want) + "\n"
    assert _evaluate(base + ["--metrics", "mss"]) == line
    full = json.loads(_evaluate(base + ["--metrics", "mss,loudness,panning,dynamic", "--json", str(tmp_path / "o.json")]))
    assert {k: v for k, v in full.items() if k != "features"} == want and list(full)[-1] == "features"
    assert full == json.loads(open(tmp_path / "o.json").read())
    fa, fb = ((v.astype(np.float64) / 32768.0).astype(np.float32) for v in (a, b))
    for title, ref in (("loudness", R.loudness_features(fa, fb, 44100)), ("panning", R.panning_features(fa, fb, 44100, 2048, 1024)),
                       ("dynamic", R.dynamic_features(fa, fb, 44100, 2048, 1024))):
        exact, bound = ref[0], ref[1]
        assert list(full["features"][title]) == list(exact)
        for k in exact:
            assert abs(full["features"][title][k] - exact[k]) <= bound[k] + 8 * R.EPS64 * abs(exact[k]), (title, k)
    only = json.loads(_evaluate(base + ["--metrics", "panning", "--feature_fft", "1024", "--feature_hop", "512"]))
    assert only["metric"] == "audio_features" and list(only["features"]) == ["panning"] and "segments" not in only
    exact, bound = R.panning_features(fa, fb, 44100, 1024, 512)[:2]
    assert all(abs(only["features"]["panning"][k] - exact[k]) <= bound[k] for k in exact)
    with pytest.raises(SystemExit):
        evaluate.main(base + ["--metrics", "mss,spectral"])


def _create(emu, n_fft=2048, hop=1024):
    h = C.c_void_p()
    rc = emu.mst_mixfeat_create(n_fft, hop, C.byref(h))
    return rc, h, (emu.mst_last_error() or b"").decode()


@pytest.mark.parametrize("n_fft,hop,needle", [(1000, 500, "n_fft = 1000"), (256, 128, "n_fft = 256"), (8192, 4096, "n_fft = 8192"),
                                              (2048, 0, "hop = 0"), (2048, 2049, "hop = 2049")])
def test_unsupported_sizes_name_the_offending_value(emu, n_fft, hop, needle):
    rc, _, msg = _create(emu, n_fft, hop)
    assert rc == -2 and needle in msg, (rc, msg)


def test_refusals_and_frame_counts(emu):
    rc, h, _ = _create(emu)
    assert rc == 0
    assert emu.mst_mixfeat_frames(h, 2047) == 0 and emu.mst_mixfeat_frames(h, 2048) == 1 and emu.mst_mixfeat_frames(h, 131072) == 127
    x = torch.zeros(1, 4096, 2)
    out = torch.zeros(1, 3, 8, dtype=torch.float64)
    lo, hi = (C.c_int * 2)(0, 11), (C.c_int * 2)(11, 1024)
    assert emu.mst_mixfeat_panning(h, x.data_ptr(), 1, 4096, None, lo, hi, 2, out.data_ptr(), None) == 0
    assert emu.mst_mixfeat_panning(h, x.data_ptr(), 1, 2000, None, lo, hi, 2, out.data_ptr(), None) == -2 and b"L = 2000" in emu.mst_last_error()
    assert emu.mst_mixfeat_panning(h, x.data_ptr(), 1, 4096, None, lo, hi, 9, out.data_ptr(), None) == -2 and b"n_bands = 9" in emu.mst_last_error()
    assert emu.mst_mixfeat_panning(h, x.data_ptr(), 1, 4096, None, lo, (C.c_int * 2)(11, 1026), 2, out.data_ptr(), None) == -1
    assert emu.mst_mixfeat_panning(h, x.data_ptr(), 70000, 4096, None, lo, hi, 2, out.data_ptr(), None) == -2 and b"n_items = 70000" in emu.mst_last_error()
    assert emu.mst_mixfeat_panning(h, None, 1, 4096, None, lo, hi, 2, out.data_ptr(), None) == -1
    assert emu.mst_mixfeat_sps(h, x.data_ptr(), 1, 4096, None, None, None, None) == -1
    assert emu.mst_mixfeat_low_ratio(h, x.data_ptr(), x.data_ptr(), 1, 4096, 3, None, None, out.data_ptr(), None) == -2 and b"C = 3" in emu.mst_last_error()
    assert emu.mst_mixfeat_dynamics(x.data_ptr(), 1, 4096, 3, None, 2048, 1024, out.data_ptr(), None) == -2 and b"C = 3" in emu.mst_last_error()
    assert emu.mst_mixfeat_dynamics(x.data_ptr(), 1, 1000, 2, None, 2048, 1024, out.data_ptr(), None) == -2 and b"L = 1000" in emu.mst_last_error()
    assert emu.mst_mixfeat_dynamics(x.data_ptr(), 1, 4096, 2, None, 2048, 0, out.data_ptr(), None) == -2 and b"hop = 0" in emu.mst_last_error()
    assert emu.mst_mixfeat_dynamics(x.data_ptr(), 1, 4096, 2, None, 0, 1024, out.data_ptr(), None) == -2 and b"frame_length = 0" in emu.mst_last_error()
    assert emu.mst_mixfeat_destroy(h) == 0 and emu.mst_mixfeat_destroy(None) == 0


def test_refusals_on_the_product_binding():
    """no CPU path: the product library refuses host tensors (no GPU is needed to be refused)"""
    x = torch.zeros(8192, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        D.MixFeat.get(2048, 1024).panning(x[None], [(0, 1024)])
    with pytest.raises(RuntimeError, match="no CPU path"):
        D.frame_dynamics(x[None], 2048, 1024)


def test_module_level_refusals(emu_default):
    with pytest.raises(NotImplementedError, match="n_fft = 3000"):
        U.get_SPS(np.zeros((8192, 2), np.float32), n_fft=3000, hop_length=1000)
    with pytest.raises(ValueError):
        D.MixFeat.get(2048, 1024).panning(torch.zeros(1, 8192, 1), [(0, 1024)])
    with pytest.raises(ValueError, match="one shape"):
        U.compute_panning_features((np.zeros((9000, 2), np.float32), np.zeros((9001, 2), np.float32), 0, 44100, 2048, 1024))
