"""The gradient kernels of the multi-scale spectral loss on the MI355X against the float64 restatement (tests/mss_grad_ref.py), within the
derived bound whose constant is fixed against the reference alone: the emulator's cases on cuda:0, one 4 x 2 x 131072 batch per mode
item by item, bit-identity at that size, and a learnable gain whose gradient autograd composes from the kernel's."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mss_grad_checks as K  # noqa: E402
import mss_grad_ref as GR  # noqa: E402
import mss_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

from music_mixing_style_transfer_amd import _lib  # noqa: E402

DEV = "cuda:0"
L_BIG = 131072


@pytest.mark.parametrize("mode", ["midside", "ori"])
@pytest.mark.parametrize("shape", list(K.SHAPES))
def test_every_sample_within_the_bound_through_the_abi(shape, mode):
    scales, kind, L = K.SHAPES[shape]
    est, tgt = K.batch_of_four(L)
    cot = K.random_cotangents(4, len(scales))
    got = K.backward_abi(_lib.lib(), est, tgt, cot, mode, scales, kind, DEV)
    K.check_batch_of_four(got, est, tgt, cot, mode, scales, kind, f"abi {shape} {mode}")


@pytest.mark.parametrize("mode", ["midside", "ori"])
@pytest.mark.parametrize("shape", ["n4096_mirrors_overlap", "n1024_hop100", "n512_win300_hamming", "default_scales"])
def test_every_sample_within_the_bound_through_backward(shape, mode):
    scales, kind, L = K.SHAPES[shape]
    est, tgt = K.batch_of_four(L)
    value, got = K.backward_module(est, tgt, mode, scales, kind, DEV)
    K.check_batch_of_four(got, est, tgt, GR.total_cotangents(4, L, scales), mode, scales, kind, f"backward {shape} {mode}")
    plain = K.module(mode, scales, kind, differentiable=False)(torch.from_numpy(est).to(DEV), torch.from_numpy(tgt).to(DEV))
    assert value.is_cuda and torch.equal(value, plain)


@pytest.fixture(scope="module")
def big():
    """est, tgt [4, 2, 131072] (generic, identical, all-zero, mono) on the host and on the device, made once"""
    est, tgt = K.batch_of_four(L_BIG, seed=9)
    return est, tgt, torch.from_numpy(est).to(DEV), torch.from_numpy(tgt).to(DEV)


@pytest.mark.parametrize("mode", ["midside", "ori"])
def test_batch_of_four_segments(big, mode):
    """4 x 2 x 131072 with the default scales through loss(est, tgt).backward(): checked by the restatement item by item; the same bits
    from run to run and for an item differentiated alone"""
    est, tgt, e, t = big
    loss = K.module(mode, R.DEFAULT_SCALES, "hann")

    def run(ee, tt):
        ee = ee.clone().requires_grad_(True)
        loss.terms(ee, tt).sum().backward()          # cotangent 1 / count of every sum: alone and in the batch the same
        return ee.grad

    g = run(e, t)
    assert torch.equal(g, run(e, t))
    for i in (K.GENERIC, K.MONO):
        assert torch.equal(run(e[i:i + 1], t[i:i + 1])[0], g[i]), (mode, i)
    cot = GR.total_cotangents(1, L_BIG, R.DEFAULT_SCALES) / (R.MID_WEIGHT * np.array([R.MAG_WEIGHT, R.LOG_WEIGHT]))      # 1 / count
    worst = K.check_batch_of_four(g.cpu().numpy(), est, tgt, np.repeat(cot, 4, axis=0), mode, R.DEFAULT_SCALES, "hann", f"4 x 2 x {L_BIG} {mode}")
    print(f"4 x 2 x {L_BIG} {mode}: max error / bound = {worst:.4f}")


def test_a_learnable_gain(big):
    """est = w x with w a torch parameter: autograd carries the kernel's gradient to w.grad = sum g x; against the restatement's sum,
    within the summed bound sum bound |x| (+ the float32 rounding of torch's own products and sum)"""
    est, tgt = big[0][:1, :, :16384], big[1][:1, :, :16384]
    x = torch.from_numpy(est).to(DEV)
    w = torch.nn.Parameter(torch.tensor(0.7, device=DEV))
    loss = K.module("midside", R.DEFAULT_SCALES, "hann")
    loss(w * x, torch.from_numpy(tgt).to(DEV)).backward()
    scaled = (np.float32(0.7) * est).astype(np.float32)
    g, bnd, ties, bins = GR.loss_gradient(scaled, tgt)
    want = float((g * est).sum())
    allowed = float((bnd * np.abs(est)).sum()) + 2.0 ** -24 * (2.0 + np.log2(est.size)) * float(np.abs(g * est).sum())
    print(f"learnable gain: w.grad = {float(w.grad):.9g}, float64 {want:.12g}, bound {allowed:.3g}; tie bins {ties} of {bins}")
    assert ties <= K.TIE_CAP * bins
    assert abs(float(w.grad) - want) <= allowed
