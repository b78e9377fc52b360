"""The float64 / reference-format restatement of the mixing-feature errors (tests/mixfeat_ref.py) against the REAL reference's output
(tests/golden/mixfeat.npz, written by tests/golden/make_golden_mixfeat.py): every recorded quantity at 1e-9 relative; and the condition
that keeps the derived bounds honest - on the broadband cases the bound of every per-frame figure is itself below 1e-3 of the figure,
checked from the reference's side alone (no kernel runs here)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mixfeat_ref as R  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "mixfeat.npz"))
LOUDNESS_KEYS = ("d_lufs", "d_peak")


def _close(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want)
    assert np.all(err <= 1e-9 * np.abs(want)), (what, float(err.max()), float(np.abs(want).max()))


@pytest.fixture(scope="module", params=R.CASES)
def case(request):
    name = request.param
    out, tar, sr, n_fft, hop = R.case_inputs(name)
    return name, (out, tar, sr, n_fft, hop), R.panning_features(out, tar, sr, n_fft, hop), R.dynamic_features(out, tar, sr, n_fft, hop)


def test_restatement_matches_the_reference(case):
    name, (out, tar, sr, n_fft, hop), (pe, pb, pr, fo, ft), (de, db, dr, (do, lo), (dt, lt)) = case
    _close([pr[k] for k in R.PANNING_KEYS + ("mape_mean",)], GOLD[f"{name}/panning"], f"{name} panning")
    _close([dr[k] for k in R.DYNAMIC_KEYS], GOLD[f"{name}/dynamic"], f"{name} dynamic")
    _close([R.loudness_features(out, tar, sr)[2][k] for k in LOUDNESS_KEYS], GOLD[f"{name}/loudness"], f"{name} loudness")
    for tag, f, d, l in (("out", fo, do, lo), ("tar", ft, dt, lt)):
        _close(f["p_rms_rounded"], GOLD[f"{name}/p_rms_{tag}"], f"{name} p_rms {tag}")
        _close(np.stack([d["rms_rounded"], d["dyn_rounded"], d["crest_rounded"]]), GOLD[f"{name}/rdc_{tag}"], f"{name} rms / dyn / crest {tag}")
        _close(l["ratio_rounded"], GOLD[f"{name}/low_{tag}"], f"{name} low ratio {tag}")


def test_sps_means_match_the_reference():
    tar, n_fft, hop = R.case_inputs("noise_pan")[1], 2048, 1024
    sps_mean, phi_mean, sps, phi = R.sps_rounded(R.peak_normalize(tar), n_fft, hop)
    _close(sps_mean, GOLD["noise_pan/sps_mean"], "SPS mean")
    _close(phi_mean, GOLD["noise_pan/phi_mean"], "phi mean")
    # the exact form says the same to float32 resolution of phi: SPS = (1 - phi) sign(r - l)
    phi64, sps64, _ = R.sps_exact(R.peak_normalize(tar), n_fft, hop)
    assert np.abs(phi64 - phi).max() <= 8 * R.U and np.abs(np.abs(sps64) - np.abs(sps)).max() <= 8 * R.U


def test_exact_and_reference_formats_agree_to_float32_noise(case):
    """the reference's own error (float32 arithmetic, complex64 spectra) is small against the figures: the two restatements are one"""
    name, _, (pe, pb, pr, fo, ft), (de, db, dr, _, _) = case
    for k in pe:
        assert abs(pe[k] - pr[k]) <= 1e-5 * max(1.0, abs(pe[k])), (name, k, pe[k], pr[k])
    for k in de:
        assert abs(de[k] - dr[k]) <= 1e-4 * max(1.0, abs(de[k])), (name, k, de[k], dr[k])


def test_the_bounds_say_something_on_the_broadband_cases(case):
    """a condition, not a measurement: bound / value < 1e-3 for every per-frame p_rms and low ratio of the noise and drum cases; the
    bass stem (little above 1 kHz: its frames' rms level sits far above most of their bins) is exempt and its ratio is printed"""
    name, _, (pe, pb, pr, fo, ft), (de, db, dr, (do, lo), (dt, lt)) = case
    if name not in R.BROADBAND and name != "real_bass":
        return
    with np.errstate(divide="ignore", invalid="ignore"):
        rp = max(float(np.nanmax(f["dp"] / f["p_rms"])) for f in (fo, ft))
        rl = max(float(np.nanmax(f["d_ratio"] / f["ratio"])) for f in (lo, lt))
    print(f"{name}: largest per-frame bound / value: p_rms {rp:.3g}, low ratio {rl:.3g}")
    if name in R.BROADBAND:
        assert rp < 1e-3 and rl < 1e-3, (name, rp, rl)


def test_silence_and_mono_frames_have_zero_value_and_zero_bound():
    out, tar, sr, n_fft, hop = R.case_inputs("silence_gap")
    f = R.panning_frames(R.peak_normalize(tar), sr, n_fft, hop)
    silent = f["p_rms"][:, 0] == 0
    assert silent.sum() >= 5 and np.all(f["dS"][silent] == 0) and np.all(f["p_rms_rounded"][silent] == 0)
    out, tar, sr, n_fft, hop = R.case_inputs("mono")
    f = R.panning_frames(R.peak_normalize(out), sr, n_fft, hop)
    assert np.all(f["S"] == 0) and np.all(f["dS"] == 0) and np.all(f["p_rms_rounded"] == 0)
