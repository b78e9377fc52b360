"""tests/mss_ref.py (the float64 numpy restatement of the multi-scale spectral loss, and its derived bound) against the REAL reference's
own run (tests/golden/mss.npz, written by tests/golden/make_golden_mss.py), and the reference-alone check of the bound's one constant."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mss_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "mss.npz"))


def _close(a, b, rel=1e-9):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.all(np.abs(a - b) <= rel * np.abs(b))


@pytest.mark.parametrize("name", R.CASES)
def test_restatement_matches_the_reference_in_float64(gold, name):
    est, tgt, kw = R.case_inputs(name)
    val, _ = R.terms(est, tgt, **kw)
    assert _close(val.mean(axis=0), gold[f"{name}/terms64"]), name
    assert _close(R.total(val), gold[f"{name}/total64"]), name
    n_fft, hop, wl = kw["scales"][0]
    spec = R.front_end(tgt, n_fft, hop, wl, kw["kind"])[0]
    assert _close(spec.reshape(-1)[gold[f"{name}/probe_pos"]], gold[f"{name}/probe64"]), name
    if name == "identical":
        assert R.total(val) == 0.0 and float(gold[f"{name}/total32"]) == 0.0


def test_frame_count_and_dc_quirks():
    # the last frame goes when L % (n_fft / 4) == 0 - whatever the hop; bin 0 is the one that is dropped
    assert R.n_frames(131072, 4096, 1024) == 128 and R.n_frames(131000, 4096, 1024) == 128 and R.n_frames(131072, 2048, 300) == 436
    x = np.ones((1, 1, 4096))
    m = R.front_end(x, 512)[0]
    # a constant under a Hann window is DC (256) and its two neighbours (128): row 0 is bin 1, and nothing else is left
    assert m.shape == (1, 1, 256, 32) and abs(m[0, 0, 0, 5] - 128.0) < 1e-6 and m[0, 0, 1:, 5].max() < 1e-3


def test_constant_of_the_bound_against_the_reference_alone(gold):
    """C_FFT is twice the largest ratio the reference's own float32 run shows against its float64 run, rounded up: the reference alone
    stays under C_FFT / 2 on every term of every golden case (the bound recomputed here, not read from the file)."""
    worst = 0.0
    for name in R.CASES:
        est, tgt, kw = R.case_inputs(name)
        _, bnd = R.terms(est, tgt, c=1.0, **kw)
        bnd, gap = bnd.mean(axis=0), gold[f"{name}/gap"]
        assert np.all(gap[bnd == 0] == 0), name
        ratio = np.divide(gap, bnd, out=np.zeros_like(gap), where=bnd > 0)
        print(f"{name:16s} reference alone: max |fp32 - float64| / bound(c = 1) = {ratio.max():.4f}")
        assert ratio.max() <= R.C_FFT / 2.0, name
        worst = max(worst, float(ratio.max()))
    assert abs(worst - R.MEASURED_MAX_RATIO) <= 5e-4 and R.C_FFT == float(np.ceil(2.0 * worst))


def test_constant_of_the_element_bound_against_the_reference_alone(gold):
    """C_ELEM by the same rule on the spectrograms: the stored positions are strided probes plus the 64 elements where the reference's
    own float32 run is worst, so the largest ratio over them is the largest over all elements.  The reference alone stays under
    C_ELEM / 2 of the elementwise bound.  (Against the plain per-frame delta it does not - see tests/mss_ref.py.)"""
    worst = 0.0
    for name in R.CASES:
        tgt, kw = R.case_inputs(name)[1:]
        n_fft, hop, wl = kw["scales"][0]
        spec, be, _ = R.front_end(tgt, n_fft, hop, wl, kw["kind"], c=1.0)
        pos = gold[f"{name}/probe_pos"]
        err = np.abs(gold[f"{name}/probe32"].astype(np.float64) - spec.reshape(-1)[pos])
        ratio = float((err / be.reshape(-1)[pos]).max())
        print(f"{name:16s} reference alone: max element |fp32 - float64| / delta_elem(c = 1) = {ratio:.3f}")
        assert abs(ratio - float(gold[f"{name}/probe_ratio"])) <= 1e-6 * ratio and ratio <= R.C_ELEM / 2.0, name
        worst = max(worst, ratio)
    assert abs(worst - R.MEASURED_MAX_RATIO_ELEM) <= 5e-3 and R.C_ELEM == float(np.ceil(2.0 * worst))
