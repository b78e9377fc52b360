"""tests/contrast_ref.py against the REAL reference (tests/golden/contrast.npz, made by tests/golden/make_golden_contrast.py from the
reference's own NT_Xent, infoNCE and RMSLoss under torch.autograd): the float64 restatement is the reference's float64 run, the reference's
own float32 run lies inside the bounds at the constants in use, the constants are what the rule gives, the mask is the reference's, and the
two departures are exactly the stated ones.  CPU only, no library."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import contrast_ref as CR  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "contrast.npz"))


def _restated(kind, name):
    if kind == "ntx":
        loss, bloss, g, bg = CR.ntxent(*CR.ntx_case_inputs(name))
    elif kind == "nce":
        loss, bloss, (ga, bga), (gb, bgb) = CR.infonce(*CR.nce_case_inputs(name))
        g, bg = np.concatenate([ga, gb]), np.concatenate([bga, bgb])
    else:
        loss, bloss, g, bg = CR.rms_loss(*CR.rms_case_inputs(name))
    return loss, bloss, g.reshape(-1), bg.reshape(-1)


CASES = [("ntx", n) for n in CR.NTX_CASES] + [("nce", n) for n in CR.NCE_CASES] + [("rms", n) for n in CR.RMS_CASES]


@pytest.mark.parametrize("kind,name", CASES)
def test_restatement_is_the_reference_in_float64_and_its_float32_run_is_inside_the_bound(golden, kind, name):
    loss, bloss, g, bg = _restated(kind, name)
    key = f"{kind}/{name}"
    pos, g64, g32 = golden[f"{key}/pos"], golden[f"{key}/grad64"], golden[f"{key}/grad32"]
    assert abs(loss - float(golden[f"{key}/loss64"])) <= 1e-9 * max(abs(loss), 1e-300)
    assert np.abs(g[pos] - g64).max() <= 1e-9 * max(np.abs(g64).max(), 1e-300)
    assert CR.ratio(abs(float(golden[f"{key}/loss32"]) - loss), bloss) <= 1.0
    assert CR.ratio(np.abs(g32.astype(np.float64) - g[pos]), bg[pos]) <= 1.0
    # the stored reference-alone ratios were taken against these bounds at c = 1 (every constant in use is 1)
    assert CR.ratio(np.abs(g32.astype(np.float64) - g[pos]), bg[pos]) == pytest.approx(float(golden[f"{key}/ratio_grad"]), rel=1e-6, abs=1e-12)


def test_the_constants_are_twice_the_reference_alone_ratios_rounded_up(golden):
    for q, c in (("ntx_loss", CR.C_NTX_LOSS), ("ntx_grad", CR.C_NTX_GRAD), ("nce", CR.C_NCE), ("rms", CR.C_RMS)):
        worst = float(golden[f"max_ratio/{q}"])
        assert CR.MEASURED_MAX_RATIO[q] == pytest.approx(worst, abs=5e-5), q
        assert c == max(1.0, float(np.ceil(2.0 * worst))), q


def test_mask_is_the_references():
    """the reference's mask_correlated_samples, written out: everything but the diagonal and the two positive diagonals"""
    for B in (1, 3, 17):
        m = CR.mask_correlated_samples(B)
        i, j = np.indices((2 * B, 2 * B))
        assert np.array_equal(m, (i != j) & (np.abs(i - j) != B))


def test_tiny_case_with_one_row_per_view_is_exactly_zero():
    loss, _, g, _ = CR.ntxent(*CR.ntx_case_inputs("tiny1"))
    assert loss == 0.0 and not g.any()


def test_departure_zero_row_gets_exact_zeros_where_autograd_gives_the_clamp_artefact():
    zi, zj, tau = CR.ntx_case_inputs("zero_row")
    loss, _, g, _ = CR.ntxent(zi, zj, tau)
    assert not g[CR.ZERO_ROW].any() and np.abs(np.delete(g, CR.ZERO_ROW, axis=0)).min(axis=1).max() > 0
    # the reference's formulation under autograd, float64: forward equal, that row's gradient is dzh / eps
    a = torch.from_numpy(zi).double().requires_grad_(True)
    b = torch.from_numpy(zj).double().requires_grad_(True)
    z = torch.cat((a, b))
    sim = torch.nn.CosineSimilarity(dim=2)(z.unsqueeze(1), z.unsqueeze(0)) / tau
    N = z.shape[0]
    logits = sim.masked_fill(torch.eye(N, dtype=bool), -float("inf"))
    ref = torch.nn.functional.cross_entropy(logits, (torch.arange(N) + N // 2) % N)
    ref.backward()
    assert abs(float(ref) - loss) <= 1e-12 * abs(loss)
    assert a.grad[CR.ZERO_ROW].abs().max() > 1e6
    keep = np.arange(zi.shape[0]) != CR.ZERO_ROW
    assert np.abs(a.grad.numpy()[keep] - g[:zi.shape[0]][keep]).max() <= 1e-9 * np.abs(g).max()
    assert np.abs(b.grad.numpy() - g[zi.shape[0]:]).max() <= 1e-9 * np.abs(g).max()


def test_departure_silent_row_gets_zeros_where_autograd_gives_nan():
    est, tgt = CR.rms_case_inputs("silent_row")
    loss, _, g, _ = CR.rms_loss(est, tgt)
    rows = g.reshape(-1, est.shape[-1])
    assert not rows[CR.SILENT_ROW].any() and np.isfinite(g).all()
    e = torch.from_numpy(est).double().requires_grad_(True)
    x, y = e.reshape(-1, est.shape[-1]), torch.from_numpy(tgt).double().reshape(-1, est.shape[-1])
    re, rt = torch.sqrt(torch.mean(x ** 2, dim=-1)), torch.sqrt(torch.mean(y ** 2, dim=-1))
    w = torch.clamp(torch.abs(rt - re), min=1 / 100.) * 100.
    ref = torch.mean(w ** 1.5 * torch.nn.functional.mse_loss(re, rt))
    ref.backward()
    got = e.grad.reshape(-1, est.shape[-1]).numpy()
    assert abs(float(ref) - loss) <= 1e-12 * loss
    assert np.isnan(got[CR.SILENT_ROW]).all()
    keep = np.arange(rows.shape[0]) != CR.SILENT_ROW
    assert np.abs(got[keep] - rows[keep]).max() <= 1e-9 * np.abs(rows).max()


def test_clamped_case_sits_on_the_flat_side():
    est, tgt = CR.rms_case_inputs("clamped")
    e, t = est.astype(np.float64).reshape(-1, est.shape[-1]), tgt.astype(np.float64).reshape(-1, est.shape[-1])
    d = np.abs(np.sqrt((e ** 2).mean(axis=1)) - np.sqrt((t ** 2).mean(axis=1)))
    assert d[2] < 0.5 / CR.WEIGHT_FACTOR and np.delete(d, 2).min() > 2.0 / CR.WEIGHT_FACTOR
