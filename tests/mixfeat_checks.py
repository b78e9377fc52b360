"""TEST INFRASTRUCTURE: the checks the emulator tests and the GPU tests of the mixing-feature kernels share - every kernel form and
the Python functions against the restatement and its derived bounds (tests/mixfeat_ref.py)."""
import numpy as np
import torch

import mixfeat_ref as R
from music_mixing_style_transfer_amd.mixing_manipulator import _device_ops as D
from music_mixing_style_transfer_amd.mixing_manipulator import utils_data_normalization as U


def ratio(err, bnd):
    """max err / bound; an error where the bound is zero counts as infinite"""
    err, bnd = np.asarray(err, dtype=np.float64), np.asarray(bnd, dtype=np.float64)
    r = np.divide(err, bnd, out=np.zeros_like(err), where=bnd > 0)
    r[(bnd == 0) & (err > 0)] = np.inf
    return float(r.max()) if r.size else 0.0


def _dev(x, device):
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return t if device is None else t.to(device)


def check_frames(name, x, sr, n_fft, hop, device=None):
    """one signal [L, 2] through every kernel form against the exact restatement; returns {figure: max err / bound}"""
    xd = _dev(x, device)[None]
    gain = np.asarray([R.peak_gain(x)], dtype=np.float32)
    xn = R.peak_normalize(x)
    mf = D.MixFeat.get(n_fft, hop)
    out = {}
    # band sums of SPS^2
    f = R.panning_frames(xn, sr, n_fft, hop)
    S = mf.panning(xd, R.band_bins(sr, n_fft), gain)[0]
    out["panning"] = ratio(np.abs(S - f["S"]), f["dS"])
    assert np.all(S[f["S"] == 0] == 0), f"{name}: a frame with l == r in every bin must give exactly 0"
    # phi and SPS per bin: the bound of q = 1 - phi = |SPS| plus the float32 the value is stored in; where |l - r| is inside its own
    # bound the sign of SPS is not determined: there |SPS| itself is added
    phi, sps = (v[0].cpu().numpy().astype(np.float64) for v in mf.sps(xd, gain))
    phi64, sps64, dq2 = R.sps_exact(xn, n_fft, hop)
    q = np.abs(sps64)
    dq = np.where(q > 0, (np.sqrt(q * q + dq2) - q), np.sqrt(dq2))          # dq2 = 2 q dq + dq^2, solved for dq
    out["phi"] = ratio(np.abs(phi - phi64), dq + 2.0 ** -23)
    flip = np.sign(sps) * np.sign(sps64) < 0
    out["sps"] = ratio(np.abs(sps - sps64), dq + 2.0 ** -23 * q + np.where(flip & (q <= dq), 2.0 * q, 0.0))
    # the low-frequency ratio per channel, through the device low-pass
    xnd = xd * torch.from_numpy(gain).to(xd.device)[:, None, None]
    low = U._lowpass_batch(xnd, 1000, sr)
    lr = R.low_ratio_frames(xn, sr, n_fft, hop)
    got = mf.low_ratio(low, xnd)[0]
    out["low_ratio"] = ratio(np.abs(got - lr["per_channel"]), lr["per_channel_bound"])
    # the low-passed signal itself against its per-sample bound
    out["lowpass"] = ratio(np.abs(low[0].cpu().numpy().astype(np.float64) - R.lowpass(xn, 1000, sr)), R.lowpass_sample_bound(xn, 1000, sr))
    # frame sums: hop blocks combined (hop divides the frame) and whole frames (it does not)
    for fr, hp, tag in ((n_fft, hop, "dynamics"), (n_fft, hop - 37, "dynamics_direct")):
        sums, bnd = R.frame_sums(xn, fr, hp)
        got = D.frame_dynamics(xd, fr, hp, gain)[0]
        out[tag] = ratio(np.abs(got - sums), bnd)
        assert np.array_equal(got[..., 2], sums[..., 2]), f"{name}: max |x| is exact"
    print(f"{name:12s} n_fft {n_fft:4d} L {x.shape[0]:8d}  err / bound: " + "  ".join(f"{k} {v:.3g}" for k, v in out.items()))
    for k, v in out.items():
        assert v <= 1.0, (name, k, v)
    return out


def check_features(name, out, tar, sr, n_fft, hop, device=None, golden=None):
    """the three Python functions on a pair against the exact restatement within the derived bound; with `golden` (the reference's own
    values of the three dictionaries) also against those, the bound widened by the reference's own error |golden - exact|"""
    args = (_dev(out, device), _dev(tar, device), 0, sr, n_fft, hop) if device is not None else (out, tar, 0, sr, n_fft, hop)
    worst = {}
    for title, fn, ref in (("loudness", U.compute_loudness_features, lambda: R.loudness_features(out, tar, sr)[:2]),
                           ("panning", U.compute_panning_features, lambda: R.panning_features(out, tar, sr, n_fft, hop)[:2]),
                           ("dynamic", U.compute_dynamic_features, lambda: R.dynamic_features(out, tar, sr, n_fft, hop)[:2])):
        got = fn(args)
        exact, bound = ref()
        assert list(got) == list(exact), (title, list(got), list(exact))
        for i, k in enumerate(exact):
            v = float(got[k][0])
            slack = 8 * R.EPS64 * abs(exact[k])          # the float64 host arithmetic of both sides
            r = ratio([abs(v - exact[k])], [bound[k] + slack])
            worst[f"{title}.{k}"] = r
            assert r <= 1.0, (name, title, k, v, exact[k], bound[k])
            if golden is not None:
                g = float(golden[title][i])
                assert abs(v - g) <= bound[k] + slack + abs(g - exact[k]), (name, title, k, v, g, exact[k], bound[k])
    w = max(worst.values())
    print(f"{name:12s} features: max err / bound = {w:.3g} ({max(worst, key=worst.get)})")
    return worst
