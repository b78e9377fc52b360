"""The contrastive and gain loss kernels (csrc/contrast_kernels.h) on the MI355X, through modules/loss.py: the emulator's cases and checks
(tests/contrast_checks.py) on cuda:0 - every loss and every gradient element against the float64 restatement within the derived bounds of
tests/contrast_ref.py, the exact zeros, bit-identity, the refusals, the descent check - and that the product library is what ran."""
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import contrast_checks as K  # noqa: E402

pytestmark = pytest.mark.gpu

from music_mixing_style_transfer_amd import _lib  # noqa: E402

DEV = "cuda:0"


def test_the_product_library_exports_the_losses():
    lib = _lib.lib()
    assert lib.path.endswith("libmst_hip.so") and lib.mst_version() >= 111


@pytest.mark.parametrize("name", K.NTX_NAMES)
def test_ntxent_loss_and_every_gradient_element_within_the_bound(name):
    K.check_ntx_case(name, DEV)


@pytest.mark.parametrize("name", K.NCE_NAMES)
def test_infonce_loss_and_both_gradients_within_the_bound(name):
    K.check_nce_case(name, DEV)


@pytest.mark.parametrize("name", K.RMS_NAMES)
def test_rms_loss_and_gradient_within_the_bound(name):
    K.check_rms_case(name, DEV)


def test_a_cotangent_scales_the_gradient():
    K.check_cotangent(DEV)


def test_a_second_backward_over_a_retained_graph_gives_the_same_bits():
    K.check_retained_graph(DEV)


def test_refusals():
    K.check_refusals(DEV)
    z = torch.zeros(4, 8)
    with pytest.raises(RuntimeError, match="MI355X"):
        K.NT_Xent(4, 0.1, 1)(z, z)
    with pytest.raises(RuntimeError, match="MI355X"):
        K.infoNCE(z, z)
    with pytest.raises(RuntimeError, match="MI355X"):
        K.RMSLoss(True)(torch.zeros(1, 2, 64), torch.zeros(1, 2, 64))


def test_the_gradients_are_descent_directions_of_the_float64_losses():
    K.check_descent(DEV)


def test_backward_fills_both_views_on_a_side_stream():
    """the kernels run on the caller's current stream"""
    zi, zj, tau = K.CR.ntx_case_inputs("ragged")
    _, ga, gb = K.run_ntx(zi, zj, tau, DEV)
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        _, sa, sb = K.run_ntx(zi, zj, tau, DEV)
    s.synchronize()
    assert torch.equal(K.bits(sa), K.bits(ga)) and torch.equal(K.bits(sb), K.bits(gb))
