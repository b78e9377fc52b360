"""tests/mss_grad_ref.py (the float64 numpy restatement of the loss's gradient with respect to the estimate, and its derived bound) against
the REAL reference's own autograd run (tests/golden/mss_grad.npz, written by tests/golden/make_golden_mss_grad.py), and the
reference-alone check of the bound's one constant.  No kernel runs here."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mss_grad_ref as GR  # noqa: E402
import mss_ref as R  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "mss_grad.npz"))


@pytest.fixture(scope="module")
def restated():
    """name -> (gradient, bound at c = 1, tie bins, bins), computed once"""
    return {name: GR.loss_gradient(*GR.grad_case_inputs(name)[:2], c=1.0, **GR.grad_case_inputs(name)[2]) for name in GR.GRAD_CASES}


@pytest.mark.parametrize("name", list(GR.GRAD_CASES))
def test_restatement_matches_the_reference_autograd_in_float64(gold, restated, name):
    want = gold[f"{name}/grad64"]
    got = restated[name][0]
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), name
    est, tgt, kw = GR.grad_case_inputs(name)
    assert abs(R.loss(est, tgt, **kw)[0] - float(gold[f"{name}/total64"])) <= 1e-9 * float(gold[f"{name}/total64"])


@pytest.mark.parametrize("name", list(GR.GRAD_CASES))
def test_reference_float32_is_inside_the_bound(gold, restated, name):
    """the stored positions are strided probes plus the 32 samples where the reference's float32 gradient is worst, so the largest ratio
    over them is the largest over all samples"""
    g, bnd, ties, bins = restated[name]
    pos = gold[f"{name}/probe_pos"]
    err = np.abs(gold[f"{name}/probe32"].astype(np.float64) - g.reshape(-1)[pos])
    r = GR.ratio(err, bnd.reshape(-1)[pos])
    print(f"{name:10s} reference alone: max |fp32 - float64| / bound(c = 1) = {r:.4f} (recorded {float(gold[f'{name}/ratio']):.4f}); tie bins {ties} of {bins}")
    assert abs(r - float(gold[f"{name}/ratio"])) <= 1e-6 * r
    assert r <= GR.C_GRAD / 2.0, name
    assert ties <= 1e-3 * bins


def test_constant_of_the_bound_against_the_reference_alone(gold):
    worst = max(float(gold[f"{name}/ratio"]) for name in GR.GRAD_CASES)
    assert abs(worst - float(gold["max_ratio"])) <= 1e-12
    assert abs(worst - GR.MEASURED_MAX_RATIO_GRAD) <= 5e-4
    assert GR.C_GRAD >= 2.0 * worst and GR.C_GRAD == float(np.ceil(2.0 * worst))


def test_fold_is_the_adjoint_of_reflection_padding():
    """<pad(x), P> == <x, fold(P)> for the forward's reflection, at a length where both mirrors reach the same samples"""
    rng = np.random.default_rng(0)
    for L, m in ((2049, 2048), (700, 256), (300, 128)):
        x, P = rng.standard_normal(L), rng.standard_normal(L + 2 * m)
        xp = np.concatenate([x[m:0:-1], x, x[-2:-m - 2:-1]])
        assert abs(np.dot(xp, P) - np.dot(x, GR._fold(P, L, m))) <= 1e-10 * np.abs(P).sum()


def test_zero_properties_of_the_formula():
    """est identical to tgt, and est == 0, give an all-zero gradient in float64 too"""
    est, tgt, kw = GR.grad_case_inputs("batch")
    assert np.all(GR.loss_gradient(tgt, tgt, **kw)[0] == 0.0)
    assert np.all(GR.loss_gradient(np.zeros_like(est), tgt, **kw)[0] == 0.0)
