"""`Loss(args)`, the trainer's container of the reference (modules/loss.py:244-258), on the MI355X: the reference's attribute names, and one
training step's objectives - NT-Xent on two [8, 2048] views, the gain loss and both multi-scale spectral losses on [2, 2, 8192] - summed and
backpropagated in one backward()."""
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import contrast_ref as CR  # noqa: E402

pytestmark = pytest.mark.gpu

from music_mixing_style_transfer_amd.modules import Loss, MultiScale_Spectral_Loss_MidSide_DDSP, NT_Xent, RMSLoss, infoNCE  # noqa: E402

DEV = "cuda:0"


@pytest.fixture(scope="module")
def loss():
    return Loss(types.SimpleNamespace(gpu=0, batch_size_total=4, num_strong_negatives=1, temperature=0.1, eps=1e-7))


def test_members_have_the_references_names(loss):
    assert isinstance(loss.l1, torch.nn.L1Loss) and isinstance(loss.mse, torch.nn.MSELoss) and isinstance(loss.ce, torch.nn.CrossEntropyLoss)
    assert isinstance(loss.triplet, torch.nn.TripletMarginLoss) and loss.infonce is infoNCE
    assert isinstance(loss.ntxent, NT_Xent) and loss.ntxent.batch_size == 8 and loss.ntxent.temperature == 0.1 and loss.ntxent.world_size == 1
    assert loss.ntxent.mask.shape == (16, 16) and loss.ntxent.mask.dtype == torch.bool and loss.ntxent.differentiable
    assert isinstance(loss.gain, RMSLoss) and loss.gain.differentiable
    for m, mode in ((loss.multi_scale_spectral_midside, "midside"), (loss.multi_scale_spectral_ori, "ori")):
        assert isinstance(m, MultiScale_Spectral_Loss_MidSide_DDSP) and m.mode == mode and m.differentiable


def test_one_training_step_backpropagates_the_sum(loss):
    zi = CR._noise(1, (8, 2048))
    zj = (np.float32(0.7) * zi + np.float32(0.5) * CR._noise(2, (8, 2048))).astype(np.float32)
    tgt = (np.float32(0.3) * CR._noise(3, (2, 2, 8192))).astype(np.float32)
    est = (np.float32(0.5) * tgt + np.float32(0.05) * CR._noise(4, (2, 2, 8192))).astype(np.float32)
    a = torch.from_numpy(zi).to(DEV).requires_grad_(True)
    b = torch.from_numpy(zj).to(DEV).requires_grad_(True)
    e = torch.from_numpy(est).to(DEV).requires_grad_(True)
    t = torch.from_numpy(tgt).to(DEV)
    parts = [loss.ntxent(a, b), loss.gain(e, t), loss.multi_scale_spectral_midside(e, t), loss.multi_scale_spectral_ori(e, t)]
    total = parts[0] + parts[1] + parts[2] + parts[3]
    total.backward()
    assert all(p.dtype == torch.float32 and p.dim() == 0 and torch.isfinite(p) for p in parts)
    # the contrastive part against the float64 restatement; the waveform gradient is the sum of the three members' own gradients
    want, bloss, g, bg = CR.ntxent(zi, zj, 0.1)
    assert abs(float(parts[0]) - want) <= bloss
    got = np.concatenate([a.grad.cpu().numpy(), b.grad.cpu().numpy()]).astype(np.float64)
    assert CR.ratio(np.abs(got - g), bg) <= 1.0
    alone, mass = torch.zeros_like(e), torch.zeros_like(e)
    for member in (loss.gain, loss.multi_scale_spectral_midside, loss.multi_scale_spectral_ori):
        x = torch.from_numpy(est).to(DEV).requires_grad_(True)
        member(x, t).backward()
        alone += x.grad
        mass += x.grad.abs()
    assert torch.isfinite(e.grad).all() and e.grad.abs().sum() > 0
    assert ((e.grad - alone).abs() <= 4 * 2.0 ** -24 * mass).all()          # three float32 additions in either order
    want_gain, bgain, _, _ = CR.rms_loss(est, tgt)
    assert abs(float(parts[1]) - want_gain) <= bgain
    assert float(loss.infonce(a.detach(), b.detach())) > 0.0
