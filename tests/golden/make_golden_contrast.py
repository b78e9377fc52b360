"""Generate tests/golden/contrast.npz: the REAL reference's NT_Xent, infoNCE and RMSLoss (modules/loss.py) with their gradients by
torch.autograd, in float64 and in float32, on the cases of tests/contrast_ref.py.

Run ONLY where the reference checkout is present:   python tests/golden/make_golden_contrast.py
The import shims are make_golden_mss.py's (install_stubs); Tensor.cuda is the identity here (infoNCE moves its labels to the GPU).

Per case (prefix ntx/<case>, nce/<case>, rms/<case>) the file holds
  loss64, loss32        the two runs' values
  pos                   flat positions into the gradient (NT-Xent: cat(z_i, z_j) [2 B, D]; infoNCE: cat(nn, p); RMS: est): every position of a
                        gradient of at most 2500 values, otherwise about 509 evenly strided ones and the 32 where the reference-alone
                        ratio is largest
  grad64, grad32        the float64 and the float32 gradient at those positions
  ratio_loss, ratio_grad   reference alone: |fp32 - float64| / (tests/contrast_ref.py's bound at c = 1), its max over ALL gradient values
and the largest ratios per quantity as max_ratio/<quantity>.  The rows the two stated departures cover (the zero row of `zero_row`, the silent
row of `silent_row`) are checked here against what the reference does - dzh / eps and NaN - stored as this project defines them (zeros) and
left out of the ratios.
Each constant of tests/contrast_ref.py is twice its quantity's largest ratio, rounded up; they are printed at the end.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

import contrast_ref as CR  # noqa: E402
from make_golden_mss import REF, install_stubs  # noqa: E402


def run(fn, arrays, dtype, grads):
    """fn(*tensors) under autograd at `dtype` -> (loss, the gradients of the first `grads` inputs concatenated along axis 0)"""
    torch.set_default_dtype(dtype)
    try:
        ts = [torch.from_numpy(a).to(dtype).requires_grad_(i < grads) for i, a in enumerate(arrays)]
        out = fn(*ts)
        out.backward()
        return float(out.detach()), np.concatenate([t.grad.numpy() for t in ts[:grads]], axis=0)
    finally:
        torch.set_default_dtype(torch.float32)


def store(out, worst, key, quantity_loss, quantity_grad, l64, l32, g64, g32, mine_loss, bloss, mine_grad, bgrad, skip_rows=()):
    keep = np.ones(g64.shape[0], dtype=bool)
    keep[list(skip_rows)] = False
    top = max(np.abs(g64[keep]).max(), 1e-300)
    assert abs(mine_loss - l64) <= 1e-9 * max(abs(l64), 1e-300), (key, mine_loss, l64)
    assert np.abs(mine_grad[keep] - g64[keep]).max() <= 1e-9 * top, (key, np.abs(mine_grad[keep] - g64[keep]).max() / top)
    g64 = np.where(keep.reshape((-1,) + (1,) * (g64.ndim - 1)), g64, mine_grad)          # the departures, as this project defines them
    err = np.abs(g32.astype(np.float64) - g64)
    err[~keep] = 0.0
    assert np.all(bgrad[err > 0] > 0), f"{key}: the reference alone errs where the bound is zero"
    r = np.divide(err, bgrad, out=np.zeros_like(err), where=bgrad > 0).reshape(-1)
    rl = abs(l32 - l64) / bloss if bloss > 0 else 0.0
    assert bloss > 0 or l32 == l64, key
    pos = np.arange(r.size) if r.size <= 2500 else np.unique(np.concatenate([np.arange(0, r.size, r.size // 509), np.argsort(r)[-32:]]))
    g32 = np.where(keep.reshape((-1,) + (1,) * (g32.ndim - 1)), g32, 0.0)
    out.update({f"{key}/loss64": np.float64(l64), f"{key}/loss32": np.float32(l32), f"{key}/pos": pos.astype(np.int64),
                f"{key}/grad64": g64.reshape(-1)[pos].astype(np.float64), f"{key}/grad32": g32.reshape(-1)[pos].astype(np.float32),
                f"{key}/ratio_loss": np.float64(rl), f"{key}/ratio_grad": np.float64(r.max())})
    worst[quantity_loss] = max(worst[quantity_loss], rl)
    worst[quantity_grad] = max(worst[quantity_grad], float(r.max()))
    print(f"{key:16s} loss32 {l32:.9g} loss64 {l64:.12g}  restated within {abs(mine_loss - l64):.1e} / {np.abs(mine_grad[keep] - g64[keep]).max() / top:.1e} "
          f"of max |g| = {top:.4g};  reference alone / bound(c = 1): loss {rl:.4f}, gradient {r.max():.4f}")


def main():
    install_stubs()
    sys.path.insert(0, REF)
    import modules.loss as ref_loss
    torch.Tensor.cuda = lambda self, *a, **k: self
    out, worst = {}, {"ntx_loss": 0.0, "ntx_grad": 0.0, "nce": 0.0, "rms": 0.0}

    for name, (B, D, tau) in CR.NTX_CASES.items():
        zi, zj, tau = CR.ntx_case_inputs(name)
        mine = CR.ntxent(zi, zj, tau, c_loss=1.0, c_grad=1.0)
        assert np.array_equal(ref_loss.NT_Xent(B, tau, 1).mask.numpy(), CR.mask_correlated_samples(B))
        l64, g64 = run(ref_loss.NT_Xent(B, tau, 1), (zi, zj), torch.float64, 2)
        l32, g32 = run(ref_loss.NT_Xent(B, tau, 1), (zi, zj), torch.float32, 2)
        skip = ()
        if name == "zero_row":          # the first departure: the reference's gradient of that row is dzh / eps
            skip = (CR.ZERO_ROW,)
            assert np.abs(g64[CR.ZERO_ROW]).max() > 1e6 and not mine[2][CR.ZERO_ROW].any()
        store(out, worst, f"ntx/{name}", "ntx_loss", "ntx_grad", l64, l32, g64, g32, *mine, skip_rows=skip)

    for name in CR.NCE_CASES:
        a, b, tau = CR.nce_case_inputs(name)
        loss, bloss, (ga, bga), (gb, bgb) = CR.infonce(a, b, tau, c=1.0)
        fn = lambda x, y: ref_loss.infoNCE(x, y, temperature=tau)  # noqa: E731
        l64, g64 = run(fn, (a, b), torch.float64, 2)
        l32, g32 = run(fn, (a, b), torch.float32, 2)
        skip = ()
        if name == "zero_row":
            skip = (CR.ZERO_ROW,)
            assert np.abs(g64[CR.ZERO_ROW]).max() > 1e6 and not ga[CR.ZERO_ROW].any()
        store(out, worst, f"nce/{name}", "nce", "nce", l64, l32, g64, g32, loss, bloss, np.concatenate([ga, gb]), np.concatenate([bga, bgb]),
              skip_rows=skip)

    for name, shape in CR.RMS_CASES.items():
        est, tgt = CR.rms_case_inputs(name)
        loss, bloss, g, bg = CR.rms_loss(est, tgt, c=1.0)
        l64, g64 = run(ref_loss.RMSLoss(reduce=True), (est, tgt), torch.float64, 1)
        l32, g32 = run(ref_loss.RMSLoss(reduce=True), (est, tgt), torch.float32, 1)
        rows = lambda x: x.reshape(-1, shape[2])  # noqa: E731
        skip = ()
        if name == "silent_row":          # the second departure: the reference's gradient of that row is NaN
            skip = (CR.SILENT_ROW,)
            assert np.isnan(rows(g64)[CR.SILENT_ROW]).all() and np.isnan(rows(g32)[CR.SILENT_ROW]).all() and not rows(g)[CR.SILENT_ROW].any()
        store(out, worst, f"rms/{name}", "rms", "rms", l64, l32, rows(g64), rows(g32), loss, bloss, rows(g), rows(bg), skip_rows=skip)

    for k, v in worst.items():
        out[f"max_ratio/{k}"] = np.float64(v)
        print(f"largest reference-alone ratio, {k}: {v:.4f}  ->  constant ceil(2 x) = {int(np.ceil(2.0 * v))}")
    np.savez_compressed(os.path.join(HERE, "contrast.npz"), **out)


if __name__ == "__main__":
    main()
