"""TEST INFRASTRUCTURE: the checks tests/test_contrast_emu.py (CPU SIMT emulator) and tests/test_contrast_gpu.py (MI355X) share - the same
cases, the same float64 restatement and bounds (tests/contrast_ref.py), through the module API of modules/loss.py on `device`."""
import functools

import numpy as np
import pytest
import torch

import contrast_ref as CR
from music_mixing_style_transfer_amd.modules import Loss, NT_Xent, RMSLoss, infoNCE  # noqa: F401

NTX_NAMES, NCE_NAMES, RMS_NAMES = list(CR.NTX_CASES), list(CR.NCE_CASES), list(CR.RMS_CASES)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def ntx_reference(name, dloss=1.0):
    zi, zj, tau = CR.ntx_case_inputs(name)
    return (zi, zj, tau) + CR.ntxent(zi, zj, tau, dloss=dloss)


@functools.lru_cache(maxsize=None)
def nce_reference(name):
    a, b, tau = CR.nce_case_inputs(name)
    return (a, b, tau) + CR.infonce(a, b, tau)


@functools.lru_cache(maxsize=None)
def rms_reference(name, dloss=1.0):
    est, tgt = CR.rms_case_inputs(name)
    return (est, tgt) + CR.rms_loss(est, tgt, dloss=dloss)


def run_ntx(zi, zj, tau, device, factor=None):
    a = torch.from_numpy(zi).to(device).requires_grad_(True)
    b = torch.from_numpy(zj).to(device).requires_grad_(True)
    loss = NT_Xent(zi.shape[0], tau, 1, differentiable=True)(a, b)
    (loss if factor is None else factor * loss).backward()
    return loss.detach(), a.grad, b.grad


def check_ntx_case(name, device):
    zi, zj, tau, want, bloss, g, bg = ntx_reference(name)
    loss, ga, gb = run_ntx(zi, zj, tau, device)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and ga.shape == zi.shape and gb.shape == zj.shape
    got = np.concatenate([ga.cpu().numpy(), gb.cpu().numpy()]).astype(np.float64)
    rl, rg = CR.ratio(abs(float(loss) - want), bloss), CR.ratio(np.abs(got - g), bg)
    print(f"ntx {name}: loss {float(loss):.9g} (float64 {want:.12g}), error / bound {rl:.4f}; gradient error / bound {rg:.4f}, max |g| {np.abs(g).max():.3g}")
    assert rl <= 1.0 and rg <= 1.0, (name, rl, rg)
    # the forward-only instance: the same bits, no graph
    plain = NT_Xent(zi.shape[0], tau, 1)(torch.from_numpy(zi).to(device), torch.from_numpy(zj).to(device))
    assert torch.equal(bits(plain), bits(loss)) and not plain.requires_grad
    # a second run: the same bits
    loss2, ga2, gb2 = run_ntx(zi, zj, tau, device)
    assert torch.equal(bits(loss2), bits(loss)) and torch.equal(bits(ga2), bits(ga)) and torch.equal(bits(gb2), bits(gb))
    if name == "tiny1":          # one row per view: the only logit of a row is its positive
        assert float(loss) == 0.0 and not bits(ga).any() and not bits(gb).any()
    if name == "zero_row":
        assert not bits(ga[CR.ZERO_ROW]).any(), "the zero row's gradient is exact zeros"
        assert ga.abs().sum() > 0 and torch.isfinite(ga).all() and torch.isfinite(gb).all()
    return rl, rg


def check_nce_case(name, device):
    a, b, tau, want, bloss, (ga64, bga), (gb64, bgb) = nce_reference(name)
    ta = torch.from_numpy(a).to(device).requires_grad_(True)
    tb = torch.from_numpy(b).to(device).requires_grad_(True)
    loss = infoNCE(ta, tb, temperature=tau)
    loss.backward()
    loss = loss.detach()
    rl = abs(float(loss) - want) / bloss
    ra, rb = CR.ratio(np.abs(ta.grad.cpu().numpy() - ga64), bga), CR.ratio(np.abs(tb.grad.cpu().numpy() - gb64), bgb)
    print(f"nce {name}: loss {float(loss):.9g} (float64 {want:.12g}), error / bound {rl:.4f}; gradient error / bound: nn {ra:.4f}, p {rb:.4f}")
    assert rl <= 1.0 and ra <= 1.0 and rb <= 1.0, (name, rl, ra, rb)
    plain = infoNCE(torch.from_numpy(a).to(device), torch.from_numpy(b).to(device), temperature=tau)
    assert torch.equal(bits(plain), bits(loss)) and not plain.requires_grad
    # one argument alone may require grad
    only = torch.from_numpy(b).to(device).requires_grad_(True)
    infoNCE(torch.from_numpy(a).to(device), only, temperature=tau).backward()
    assert torch.equal(bits(only.grad), bits(tb.grad))
    if name == "zero_row":
        assert not bits(ta.grad[CR.ZERO_ROW]).any() and torch.isfinite(ta.grad).all() and torch.isfinite(tb.grad).all()
    return rl, max(ra, rb)


def run_rms(est, tgt, device, factor=None):
    e = torch.from_numpy(est).to(device).requires_grad_(True)
    loss = RMSLoss(True, differentiable=True)(e, torch.from_numpy(tgt).to(device))
    (loss if factor is None else factor * loss).backward()
    return loss.detach(), e.grad


def check_rms_case(name, device):
    est, tgt, want, bloss, g, bg = rms_reference(name)
    loss, ge = run_rms(est, tgt, device)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and ge.shape == est.shape
    rl, rg = abs(float(loss) - want) / bloss, CR.ratio(np.abs(ge.cpu().numpy() - g), bg)
    print(f"rms {name}: loss {float(loss):.9g} (float64 {want:.12g}), error / bound {rl:.4f}; gradient error / bound {rg:.4f}")
    assert rl <= 1.0 and rg <= 1.0, (name, rl, rg)
    plain = RMSLoss(True)(torch.from_numpy(est).to(device), torch.from_numpy(tgt).to(device))
    assert torch.equal(bits(plain), bits(loss)) and not plain.requires_grad
    loss2, ge2 = run_rms(est, tgt, device)
    assert torch.equal(bits(loss2), bits(loss)) and torch.equal(bits(ge2), bits(ge))
    rows = ge.reshape(-1, est.shape[-1])
    if name == "silent_row":
        assert not bits(rows[CR.SILENT_ROW]).any() and torch.isfinite(ge).all() and rows.abs().sum() > 0
    if name == "clamped":          # row 2 sits on the clamp's flat side: its gradient comes through the squared difference alone
        e64 = est.astype(np.float64).reshape(-1, est.shape[-1])
        t64 = tgt.astype(np.float64).reshape(-1, est.shape[-1])
        assert abs(np.sqrt((e64[2] ** 2).mean()) - np.sqrt((t64[2] ** 2).mean())) < 1.0 / CR.WEIGHT_FACTOR
    return rl, rg


def check_cotangent(device):
    """(3 loss).backward(): the gradient of the tripled value, within the bound of the tripled cotangent"""
    zi, zj, tau, _, _, g, bg = ntx_reference("ragged", 3.0)
    _, ga, gb = run_ntx(zi, zj, tau, device, factor=3.0)
    got = np.concatenate([ga.cpu().numpy(), gb.cpu().numpy()]).astype(np.float64)
    assert CR.ratio(np.abs(got - g), bg) <= 1.0
    _, once_a, _ = run_ntx(zi, zj, tau, device)
    assert not torch.equal(bits(once_a), bits(ga))
    est, tgt, _, _, g, bg = rms_reference("odd", 3.0)
    _, ge = run_rms(est, tgt, device, factor=3.0)
    assert CR.ratio(np.abs(ge.cpu().numpy() - g), bg) <= 1.0


def check_retained_graph(device):
    """the first backward consumes the forward's workspace, a second one over the retained graph recomputes the similarities: the same bits"""
    for run, inputs in ((lambda a, b, tau: NT_Xent(a.shape[0], tau, 1, differentiable=True)(a, b), CR.ntx_case_inputs("ragged")),
                        (lambda a, b, tau: infoNCE(a, b, temperature=tau), CR.nce_case_inputs("sharp"))):
        a = torch.from_numpy(inputs[0]).to(device).requires_grad_(True)
        b = torch.from_numpy(inputs[1]).to(device).requires_grad_(True)
        loss = run(a, b, inputs[2])
        loss.backward(retain_graph=True)
        first = (a.grad.clone(), b.grad.clone())
        a.grad = b.grad = None
        loss.backward()
        assert torch.equal(bits(a.grad), bits(first[0])) and torch.equal(bits(b.grad), bits(first[1])) and first[0].abs().sum() > 0


def check_refusals(device):
    z = torch.zeros(4, 8, device=device)
    with pytest.raises(NotImplementedError, match="world_size"):
        NT_Xent(4, 0.1, 2)
    with pytest.raises(NotImplementedError, match="requires grad"):
        NT_Xent(4, 0.1, 1)(z.clone().requires_grad_(True), z)
    with pytest.raises(TypeError, match="float32"):
        NT_Xent(4, 0.1, 1)(z.double(), z.double())
    with pytest.raises(ValueError, match="rows"):
        NT_Xent(3, 0.1, 1)(z, z)
    with pytest.raises(ValueError, match="one shape"):
        NT_Xent(4, 0.1, 1)(z, z[:, :4])
    with pytest.raises(TypeError, match="float32"):
        infoNCE(z.double(), z.double())
    with pytest.raises(NotImplementedError, match="at most 8192"):
        NT_Xent(1, 0.1, 1)(torch.zeros(1, 8193, device=device), torch.zeros(1, 8193, device=device))
    x = torch.zeros(1, 2, 64, device=device)
    with pytest.raises(NotImplementedError, match="requires grad"):
        RMSLoss(True)(x.clone().requires_grad_(True), x)
    with pytest.raises(NotImplementedError, match="targets"):
        RMSLoss(True, differentiable=True)(x, x.clone().requires_grad_(True))
    with pytest.raises(TypeError, match="float32"):
        RMSLoss(True)(x.double(), x.double())
    with pytest.raises(ValueError, match=r"\[B, C, T\]"):
        RMSLoss(True)(x[0], x[0])
    with pytest.raises(NotImplementedError, match="loss_type"):
        RMSLoss(True, loss_type="l1")


def check_descent(device):
    """no bound involved: a backtracking search along -g finds a smaller value of the float64 restatement"""
    zi, zj, tau = CR.ntx_case_inputs("ragged")
    _, ga, gb = run_ntx(zi, zj, tau, device)
    ga, gb = ga.cpu().numpy().astype(np.float64), gb.cpu().numpy().astype(np.float64)
    base = CR.ntxent(zi, zj, tau)[0]
    step0 = np.sqrt((zi.astype(np.float64) ** 2).sum() + (zj.astype(np.float64) ** 2).sum()) / np.sqrt((ga ** 2).sum() + (gb ** 2).sum())
    for k in range(21):
        s = step0 * 2.0 ** -k
        now = CR.ntxent(zi - s * ga, zj - s * gb, tau)[0]
        if now < base:
            print(f"ntx: loss {base:.9g} -> {now:.9g} at step 2^-{k}")
            break
    else:
        pytest.fail("NT-Xent: no step decreases the float64 loss")
    est, tgt = CR.rms_case_inputs("odd")
    _, ge = run_rms(est, tgt, device)
    ge = ge.cpu().numpy().astype(np.float64)
    base = CR.rms_loss(est, tgt)[0]
    step0 = np.linalg.norm(est) / np.linalg.norm(ge)
    for k in range(21):
        now = CR.rms_loss(est - step0 * 2.0 ** -k * ge, tgt)[0]
        if now < base:
            print(f"rms: loss {base:.9g} -> {now:.9g} at step 2^-{k}")
            return
    pytest.fail("RMSLoss: no step decreases the float64 loss")
