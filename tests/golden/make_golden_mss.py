"""Generate tests/golden/mss.npz: the REAL reference's multi-scale spectral loss on the golden cases of tests/mss_ref.py.

Run ONLY where the reference checkout is present:   python tests/golden/make_golden_mss.py
It imports the reference's own modules/loss.py (absent third parties stubbed as in make_golden.py, plus classy_vision, which
modules/training_utils.py imports; none of them carries arithmetic of this path).  The reference's torch.stft calls predate
`return_complex`: torch.stft is shimmed to view_as_real(stft(..., return_complex=True)), which is what those calls meant.

Per case the file holds
  <case>/total32        the reference's forward() in float32
  <case>/total64        the same code under torch.set_default_dtype(float64) on the same (float32-valued) inputs
  <case>/terms64        [n_scales, 2, 2]: per scale and channel (mid, side / left, right) the reference's magnitude_loss and
                        log_magnitude_loss of its own front end's output, float64
  <case>/gap            |terms32 - terms64|: the reference's own float32 error per term
  <case>/ratio          gap / (tests/mss_ref.py's derived bound at c = 1)   (0 where both are 0)
  <case>/probe_pos, /probe64, /probe32   FrontEnd(channel="stereo", first scale of the case)(tgt, ["mag"]) in float64 and float32 at the
                        flat positions mss_ref.probe_positions(size) and at the 64 elements where the float32 run is worst
  <case>/probe_ratio    max over ALL elements of |fp32 - float64| / (mss_ref's elementwise bound delta_elem at c = 1) - attained at one of the
                        stored positions; printed beside it: the same against the plain per-frame delta(c = 1), which neither the
                        reference's float32 run nor a correctly rounded float64 value meets
Inputs are the integer recipes of mss_ref.case_inputs: nothing but these results is stored.  The largest ratios are printed: C_FFT
(terms) and C_ELEM (spectrogram elements) in tests/mss_ref.py are twice them, rounded up.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/mixing_style_transfer"
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import mss_ref as R  # noqa: E402


def install_stubs():
    ta = types.ModuleType("torchaudio")
    ta.functional = types.ModuleType("torchaudio.functional")
    ta.transforms = types.ModuleType("torchaudio.transforms")
    cv = types.ModuleType("classy_vision")
    cvg = types.ModuleType("classy_vision.generic")
    cvd = types.ModuleType("classy_vision.generic.distributed_util")
    cvd.convert_to_distributed_tensor = cvd.convert_to_normal_tensor = lambda t, *a: t
    cvd.is_distributed_training_run = lambda: False
    cv.generic, cvg.distributed_util = cvg, cvd
    sys.modules.update({"torchaudio": ta, "torchaudio.functional": ta.functional, "torchaudio.transforms": ta.transforms,
                        "classy_vision": cv, "classy_vision.generic": cvg, "classy_vision.generic.distributed_util": cvd})
    orig = torch.stft

    def stft(*a, **k):
        k.setdefault("return_complex", True)
        return torch.view_as_real(orig(*a, **k))

    torch.stft = stft


def reference_run(ref_loss_mod, est, tgt, kw, dtype):
    """(total, terms [S, 2, 2], the flat "mag" spectrogram of tgt) of the reference's own code at `dtype`."""
    torch.set_default_dtype(dtype)
    try:
        sc = kw["scales"]
        loss = ref_loss_mod.MultiScale_Spectral_Loss_MidSide_DDSP(mode=kw["mode"], n_filters=[s[0] for s in sc], hops_size=[s[1] for s in sc],
                                                                  windows_size=[s[2] for s in sc], window=kw["kind"], eps=kw["eps"])
        e, t = torch.from_numpy(est).to(dtype), torch.from_numpy(tgt).to(dtype)
        total = float(loss(e, t))
        terms = np.zeros((len(sc), 2, 2))
        if kw["mode"] == "midside":
            ce, ct = loss.to_mid_side(e), loss.to_mid_side(t)
        for s, scale in enumerate(loss.multiscales):
            fe = scale["front_end"]
            for c in range(2):
                if kw["mode"] == "midside":
                    me, mt = fe(ce[c], mode=["mag"]), fe(ct[c], mode=["mag"])
                else:
                    full_e, full_t = fe(e, mode=["mag"]), fe(t, mode=["mag"])
                    me, mt = full_e[:, c:c + 1], full_t[:, c:c + 1]
                terms[s, c, 0] = float(loss.magnitude_loss(me, mt))
                terms[s, c, 1] = float(loss.log_magnitude_loss(me, mt))
        n_fft, hop, wl = sc[0]
        front = sys.modules["modules.front_back_end"].FrontEnd(channel="stereo", n_fft=n_fft, hop_length=hop, win_length=wl, window=kw["kind"])
        spec = front(t, mode=["mag"]).contiguous()
        return total, terms, spec.reshape(-1).numpy().copy()
    finally:
        torch.set_default_dtype(torch.float32)


def main():
    install_stubs()
    sys.path.insert(0, REF)
    import modules.loss as ref_loss
    out = {}
    worst = worst_elem = 0.0
    for name in R.CASES:
        est, tgt, kw = R.case_inputs(name)
        t32, terms32, p32 = reference_run(ref_loss, est, tgt, kw, torch.float32)
        t64, terms64, p64 = reference_run(ref_loss, est, tgt, kw, torch.float64)
        _, bnd = R.terms(est, tgt, c=1.0, **kw)
        bnd = bnd.mean(axis=0)
        gap = np.abs(terms32 - terms64)
        assert np.all(bnd[gap > 0] > 0), f"{name}: the reference alone errs where the bound is zero"
        ratio = np.divide(gap, bnd, out=np.zeros_like(gap), where=bnd > 0)
        rel = np.divide(gap, terms64, out=np.zeros_like(gap), where=terms64 > 0)
        mine = R.total(R.terms(est, tgt, **kw)[0])
        print(f"{name:16s} total32 {t32:.9g} total64 {t64:.12g} (restated {mine:.12g})  max ratio: mag {ratio[..., 0].max():.4f} log {ratio[..., 1].max():.4f}"
              f"   max rel gap: mag {rel[..., 0].max():.2e} log {rel[..., 1].max():.2e}")
        worst = max(worst, float(ratio.max()))
        n_fft, hop, wl = kw["scales"][0]
        spec, be, bf = R.front_end(tgt, n_fft, hop, wl, kw["kind"], c=1.0, c_frame=1.0)
        ref64, be, bf = spec.reshape(-1), be.reshape(-1), np.ascontiguousarray(np.broadcast_to(bf, spec.shape)).reshape(-1)
        assert np.all(np.abs(p64 - ref64) <= 1e-9 * ref64)
        perr = np.abs(p32.astype(np.float64) - ref64)
        rounded = np.abs(ref64.astype(np.float32).astype(np.float64) - ref64)
        ratio_elem = perr / be
        pos = np.unique(np.concatenate([R.probe_positions(spec.size), np.argsort(ratio_elem)[-64:]]))      # the strided probes and the 64 worst elements
        pr = float(ratio_elem.max())
        print(f"{'':16s} spectrogram, all {spec.size} elements: max |fp32 - float64| / delta_elem(c = 1) {pr:.3f};  against plain delta(c = 1): "
              f"reference {float((perr / bf).max()):.3f}, float64 rounded to float32 {float((rounded / bf).max()):.3f}")
        worst_elem = max(worst_elem, pr)
        out.update({f"{name}/total32": np.float32(t32), f"{name}/total64": np.float64(t64), f"{name}/terms64": terms64, f"{name}/gap": gap,
                    f"{name}/ratio": ratio, f"{name}/probe_pos": pos.astype(np.int64), f"{name}/probe64": p64[pos].astype(np.float64),
                    f"{name}/probe32": p32[pos].astype(np.float32), f"{name}/probe_ratio": np.float64(pr)})
    out["max_ratio"] = np.float64(worst)
    out["max_ratio_elem"] = np.float64(worst_elem)
    print(f"largest reference-alone spectrogram element |fp32 - float64| / delta_elem(c = 1): {worst_elem:.4f}  ->  C_ELEM = ceil(2 x) = {int(np.ceil(2.0 * worst_elem))}")
    print(f"largest reference-alone |fp32 - float64| / bound(c = 1): {worst:.4f}  ->  C_FFT = ceil(2 x) = {int(np.ceil(2.0 * worst))}")
    np.savez_compressed(os.path.join(HERE, "mss.npz"), **out)


if __name__ == "__main__":
    main()
