"""Generate tests/golden/mss_grad.npz: the gradient of the REAL reference's multi-scale spectral loss with respect to the estimate, by
torch.autograd through the reference's own modules/loss.py, on the gradient cases of tests/mss_grad_ref.py.

Run ONLY where the reference checkout is present:   python tests/golden/make_golden_mss_grad.py
The import shims are make_golden_mss.py's (install_stubs: absent third parties, the torch.stft of the reference's day).

Per case the file holds
  <case>/grad64         [B, 2, L] float64: d loss / d est of the reference's forward() under torch.set_default_dtype(float64)
  <case>/total64, /total32   the loss values of the two runs
  <case>/probe_pos, /probe32   the reference's float32 gradient at about 509 evenly strided flat positions and at the 32
                        samples where |fp32 - float64| / bound(c = 1) is largest
  <case>/ratio          max over ALL samples of |fp32 - float64| / (tests/mss_grad_ref.py's bound at c = 1) - attained at a stored position
  <case>/rel            max |fp32 - float64| / max |float64| (for orientation)
Inputs are the integer recipes of mss_grad_ref.grad_case_inputs: nothing but these results is stored.  The largest ratio is printed:
C_GRAD in tests/mss_grad_ref.py is twice it, rounded up.
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

import mss_grad_ref as GR  # noqa: E402
from make_golden_mss import REF, install_stubs  # noqa: E402


def reference_gradient(ref_loss_mod, est, tgt, kw, dtype):
    torch.set_default_dtype(dtype)
    try:
        sc = kw["scales"]
        loss = ref_loss_mod.MultiScale_Spectral_Loss_MidSide_DDSP(mode=kw["mode"], n_filters=[s[0] for s in sc], hops_size=[s[1] for s in sc],
                                                                  windows_size=[s[2] for s in sc], window=kw["kind"], eps=kw["eps"])
        e = torch.from_numpy(est).to(dtype).requires_grad_(True)
        out = loss(e, torch.from_numpy(tgt).to(dtype))
        out.backward()
        return float(out.detach()), e.grad.numpy().copy()
    finally:
        torch.set_default_dtype(torch.float32)


def main():
    install_stubs()
    sys.path.insert(0, REF)
    import modules.loss as ref_loss
    out = {}
    worst = 0.0
    for name in GR.GRAD_CASES:
        est, tgt, kw = GR.grad_case_inputs(name)
        t32, g32 = reference_gradient(ref_loss, est, tgt, kw, torch.float32)
        t64, g64 = reference_gradient(ref_loss, est, tgt, kw, torch.float64)
        mine, bnd, ties, bins = GR.loss_gradient(est, tgt, c=1.0, **kw)
        top = np.abs(g64).max()
        assert np.abs(mine - g64).max() <= 1e-9 * top, (name, np.abs(mine - g64).max() / top)
        err = np.abs(g32.astype(np.float64) - g64)
        assert np.all(bnd[err > 0] > 0), f"{name}: the reference alone errs where the bound is zero"
        r = np.divide(err, bnd, out=np.zeros_like(err), where=bnd > 0).reshape(-1)
        pos = np.unique(np.concatenate([np.arange(0, r.size, max(1, r.size // 509)), np.argsort(r)[-32:]]))
        print(f"{name:10s} total32 {t32:.9g} total64 {t64:.12g}  restated gradient within {np.abs(mine - g64).max() / top:.1e} of max |g| = {top:.4g};  "
              f"reference alone: max |fp32 - float64| / bound(c = 1) = {r.max():.4f}, / max |g| = {err.max() / top:.2e};  tie bins {ties} of {bins}")
        worst = max(worst, float(r.max()))
        out.update({f"{name}/grad64": g64.astype(np.float64), f"{name}/total64": np.float64(t64), f"{name}/total32": np.float32(t32),
                    f"{name}/probe_pos": pos.astype(np.int64), f"{name}/probe32": g32.reshape(-1)[pos].astype(np.float32),
                    f"{name}/ratio": np.float64(r.max()), f"{name}/rel": np.float64(err.max() / top)})
    out["max_ratio"] = np.float64(worst)
    print(f"largest reference-alone |fp32 - float64| / bound(c = 1): {worst:.4f}  ->  C_GRAD = ceil(2 x) = {int(np.ceil(2.0 * worst))}")
    np.savez_compressed(os.path.join(HERE, "mss_grad.npz"), **out)


if __name__ == "__main__":
    main()
