"""TEST INFRASTRUCTURE: the gradient of the multi-scale spectral loss with respect to the estimate in float64 numpy, in this project's own
words on top of tests/mss_ref.py, with a derived per-sample error bound.

What is differentiated.  mst_mss_forward leaves, per item b, scale s = (n, hop, win_length) and analysis channel c (mid = L + R and
side = L - R without a half, or L and R), S0 = sum |m_e - m_t| and S1 = sum (log10(m_e + eps) - log10(m_t + eps))^2 over bins 1 .. n / 2
of every kept frame, m = sqrt(|X|^2 + 1e-7).  vjp() is the vector-Jacobian product of that map: given a = d loss / d S0 and
b = d loss / d S1 for every (b, s, c),
  per bin      dm = a sgn(m_e - m_t) + b 2 (log10(m_e + eps) - log10(m_t + eps)) / ((m_e + eps) ln 10),  sgn(0) = 0;
               Gamma_k = dm X_e,k / m_e,k  (the cotangent of (Re X_k, Im X_k) as one complex number), Gamma_0 = 0;
  per frame    gamma_j = Re sum_{k = 1 .. n/2} Gamma_k exp(+2 pi i j k / n)  (the one-sided bins count once: nothing is doubled), times the
               forward's window table;
  overlap-add  frame t, position j lands on padded index q = t hop + j - n / 2, which the forward's reflection folds onto sample
               -q (q < 0), 2 (L - 1) - q (q >= L) or q;
  un-mix       midside: d / dL = g_mid + g_side, d / dR = g_mid - g_side; ori: the identity;
and the result is summed over the scales.  total_cotangents() gives the (a, b) of the loss value itself (mss_ref.total).

The bound.  With delta = mss_ref.delta(rho_e + rho_t, n, c) the frame's level bound, bin k is charged
  beta_k = |dm_k| delta / m_e,k                                                          (X_e / m_e: the error of the spectrum)
         + |b| (2 / ln 10) [rel / (m_e + eps) + |dlog| delta / (m_e + eps)^2]            (the log difference, `rel` as in mss_ref.terms, and its divisor)
         + 2 |a|  if |m_e - m_t| <= 2 delta                                              (a TIE bin: a float32 sign may legitimately flip)
         + 2^-24 (|a| + |b| 2 |dlog| / ((m_e + eps) ln 10))                              (the cotangents are rounded to float32)
and position j of frame t carries  window_j (sum_k beta_k + c 2^-24 log2(n) sum_k |Gamma_k|)  - the adjoint transform is a float32 FFT of
the Gamma_k, |exp(i x)| = 1.  A sample's bound is the sum of these over every (scale, channel, frame, position) that folds onto it, plus the
float32 rounding of the partial sums: N values added one after the other err by at most 2^-24 N sum |value| (N counts the window
multiplication and the un-mix too).
ONE constant, C_GRAD, fixed by the project's rule against the reference ALONE: tests/golden/make_golden_mss_grad.py runs the reference's
own loss with autograd in float32 and in float64 and records, per case, the largest |fp32 - float64| / bound(c = 1) over the samples;
C_GRAD is twice the largest, rounded up.
"""
import math

import numpy as np

import mss_ref as R

# Reference alone, max over the samples of |fp32 autograd - float64 autograd| / bound(c = 1), per case of tests/golden/mss_grad.npz:
#   noise 0.0154 | noise_big 0.0189 | odd_hop 0.0340 | batch 0.0341 | lowpass 0.0052
# (|fp32 - float64| / max |float64|: 1.0e-4, 6.3e-4, 1.3e-4, 1.8e-5, 2.0e-5; no tie bin in any case).  The bound is made of absolute values over
# n / 2 bins whose errors carry signs: far above what a run shows.  Twice the largest, rounded up:
MEASURED_MAX_RATIO_GRAD = 0.0341
C_GRAD = 1.0

U32 = 2.0 ** -24

# the golden cases: (est recipe, B, L, kwargs); integer recipes, no stored audio
GRAD_CASES = {
    "noise": dict(B=1, L=3500, mode="midside", scales=R.DEFAULT_SCALES[1:], kind="hann"),
    "noise_big": dict(B=1, L=2600, mode="ori", scales=((4096, 1024, 4096),), kind="hann"),
    "odd_hop": dict(B=1, L=2600, mode="ori", scales=((1024, 100, 1024), (512, 128, 300)), kind="hamming"),
    "batch": dict(B=2, L=800, mode="midside", scales=((512, 128, 512), (256, 64, 256)), kind="hann"),
    "lowpass": dict(B=1, L=2100, mode="midside", scales=((2048, 512, 2048), (512, 128, 512)), kind="hann"),
}


def grad_case_inputs(name):
    """(est, tgt, kwargs of vjp / mss_ref.terms) of a golden gradient case: independent noise at different levels (no tie bins), or a
    low-passed pair (a peaked spectrum)"""
    c = GRAD_CASES[name]
    shape = (c["B"], 2, c["L"])
    seed = 100 + sorted(GRAD_CASES).index(name)
    if name == "lowpass":
        tgt = (np.float32(0.1) * R._lowpass(R._noise(seed, shape))).astype(np.float32)
        est = (np.float32(0.5) * tgt + np.float32(0.01) * R._noise(seed + 50, shape)).astype(np.float32)
    else:
        tgt = R._noise(seed, shape)
        est = (np.float32(0.3) * R._noise(seed + 50, shape)).astype(np.float32)
    kw = {"mode": c["mode"], "scales": c["scales"], "kind": c["kind"], "eps": 1e-7}
    return np.ascontiguousarray(est), np.ascontiguousarray(tgt), kw


def total_cotangents(B, L, scales=R.DEFAULT_SCALES):
    """d mss_ref.total / d (S0, S1): [B, n_scales, 2, 2] - the weights over the items and over each scale's bins x frames"""
    cot = np.zeros((B, len(scales), 2, 2))
    for s, (n, hop, _) in enumerate(scales):
        count = B * (n // 2) * R.n_frames(L, n, hop)
        cot[:, s, 0, :] = R.MID_WEIGHT * np.array([R.MAG_WEIGHT, R.LOG_WEIGHT]) / count
        cot[:, s, 1, :] = (1.0 - R.MID_WEIGHT) * np.array([R.MAG_WEIGHT, R.LOG_WEIGHT]) / count
    return cot


def _fold(P, L, m):
    """padded signal [..., L + 2 m] (index q + m) -> [..., L]: the adjoint of the forward's reflection padding"""
    g = P[..., m:m + L].copy()
    i1 = np.arange(1, m + 1)                      # q = -i
    g[..., i1] += P[..., m - i1]
    q2 = np.arange(L, L + m)                      # q >= L -> 2 (L - 1) - q
    g[..., 2 * (L - 1) - q2] += P[..., m + q2]
    return g


def _overlap_add(F, L, n, hop):
    """frames [..., T, n] -> [..., L] through the padded signal"""
    T = F.shape[-2]
    P = np.zeros(F.shape[:-2] + (L + n,))
    for t in range(T):
        P[..., t * hop:t * hop + n] += F[..., t, :]
    return _fold(P, L, n // 2)


def vjp(est, tgt, cot, mode="midside", scales=R.DEFAULT_SCALES, kind="hann", eps=1e-7, c=None):
    """est, tgt [B, 2, L], cot [B, n_scales, 2, 2] -> (grad [B, 2, L] float64, its per-sample bound, charged tie bins, bins)"""
    c = C_GRAD if c is None else c
    e, t = R.channels(est, mode), R.channels(tgt, mode)
    cot = np.asarray(cot, dtype=np.float64)
    B, _, L = e.shape
    grad, bound, mass, count = (np.zeros((B, 2, L)) for _ in range(4))
    ties = bins = 0
    ln10 = math.log(10.0)
    for s, (n, hop, wl) in enumerate(scales):
        w = R.window(kind, n if wl is None else wl, n)
        Xe = R.spectrum(e, n, hop, wl, kind)                       # [B, 2, n / 2 + 1, T]
        Xt = R.spectrum(t, n, hop, wl, kind)
        pe, pt = Xe.real ** 2 + Xe.imag ** 2, Xt.real ** 2 + Xt.imag ** 2
        me, mt = np.sqrt(pe[..., 1:, :] + R.MAG_EPS), np.sqrt(pt[..., 1:, :] + R.MAG_EPS)
        rho = np.sqrt(pe.mean(axis=-2, keepdims=True)) + np.sqrt(pt.mean(axis=-2, keepdims=True))
        d = R.delta(rho, n, c)                                     # [B, 2, 1, T]
        a, b = cot[:, s, :, 0][..., None, None], cot[:, s, :, 1][..., None, None]
        dlog = np.log10(me + eps) - np.log10(mt + eps)
        dm = a * np.sign(me - mt) + b * 2.0 * dlog / ((me + eps) * ln10)
        gam = dm * Xe[..., 1:, :] / me
        full = np.zeros(Xe.shape[:2] + (Xe.shape[-1], n), dtype=np.complex128)
        full[..., 1:n // 2 + 1] = np.swapaxes(gam, -1, -2)
        frames = np.fft.ifft(full, axis=-1).real * n * w           # [B, 2, T, n]
        rel = (d / (me + eps) + d / (mt + eps)) / ln10
        tie = np.abs(me - mt) <= 2.0 * d
        beta = (np.abs(dm) * d / me + np.abs(b) * (2.0 / ln10) * (rel / (me + eps) + np.abs(dlog) * d / (me + eps) ** 2)
                + 2.0 * np.abs(a) * tie + U32 * (np.abs(a) + np.abs(b) * 2.0 * np.abs(dlog) / ((me + eps) * ln10)))
        per_frame = beta.sum(axis=-2) + c * U32 * math.log2(n) * np.abs(gam).sum(axis=-2)          # [B, 2, T]
        ties += int((tie & (a != 0.0)).sum())          # a tie bin is charged only where S0 has a cotangent
        bins += tie.size
        g = _overlap_add(frames, L, n, hop)
        bd = _overlap_add(per_frame[..., None] * w, L, n, hop)
        ab = _overlap_add(np.abs(frames), L, n, hop)
        cn = _overlap_add(np.broadcast_to((w != 0.0).astype(np.float64), frames.shape), L, n, hop)
        if mode == "midside":
            grad += np.stack([g[:, 0] + g[:, 1], g[:, 0] - g[:, 1]], axis=1)
            bound += (bd[:, 0] + bd[:, 1])[:, None]
            mass += (ab[:, 0] + ab[:, 1])[:, None]
            count += (cn[:, 0] + cn[:, 1])[:, None]
        else:
            grad += g
            bound += bd
            mass += ab
            count += cn
    # the window multiplication, the un-mix and the addition to the earlier scales round too: two more per scale
    bound += U32 * (count + 2.0 * len(scales)) * mass
    return grad, bound, ties, bins


def loss_gradient(est, tgt, mode="midside", scales=R.DEFAULT_SCALES, kind="hann", eps=1e-7, c=None):
    """the gradient of mss_ref.loss's value with respect to est, and its bound"""
    est = np.asarray(est)
    return vjp(est, tgt, total_cotangents(est.shape[0], est.shape[-1], scales), mode, scales, kind, eps, c)


def ratio(err, bnd):
    """max err / bound; an error where the bound is zero counts as infinite"""
    err, bnd = np.asarray(err, dtype=np.float64), np.asarray(bnd, dtype=np.float64)
    r = np.divide(err, bnd, out=np.zeros_like(err), where=bnd > 0)
    r[(bnd == 0) & (err > 0)] = np.inf
    return float(r.max())
