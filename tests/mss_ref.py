"""TEST INFRASTRUCTURE: the multi-scale spectral distance in float64 numpy, in this project's own words, with a derived error bound.

What is computed (reference modules/loss.py MultiScale_Spectral_Loss_MidSide_DDSP over modules/front_back_end.py FrontEnd "mag"):
  * per scale (n_fft, hop, win_length): reflect-pad the signal by n_fft / 2 on both sides (torch.stft center=True), cut frames of n_fft
    samples every hop samples, multiply by the periodic Hann / Hamming window (centred and zero-padded when win_length < n_fft), rfft;
  * quirk 1: the LAST frame is dropped when L % round(n_fft / 4) == 0 (whatever the hop is);
  * quirk 2: bin 0 (DC) is dropped - the reference's comment says "discard highest frequency", its slice [:, 1:] drops the lowest;
  * m = sqrt(re^2 + im^2 + 1e-7); magnitude term = mean |m_e - m_t|, log term = mean (log10(m_e + eps) - log10(m_t + eps))^2, the means
    over items, bins and frames; mode "midside" analyses L + R and L - R (no 1/2), mode "ori" L and R;
  * total = 0.9 sum_scales (0.5 mag_a + 0.5 mag_b) + 0.1 sum_scales (0.5 log_a + 0.5 log_b).

The bound.  A float32 FFT of n points leaves an absolute error per bin of about  delta = c 2^-24 log2(n) rho,  rho the frame's rms
spectral level sqrt(mean_k |X_k|^2).  For a pair (est, tgt) both levels are charged to both signals, delta = c 2^-24 log2(n) (rho_e +
rho_t), so that an implementation that packs est and tgt into one complex transform is inside it.  |d m / d X| <= 1, hence per element
  |error of |m_e - m_t||                 <= delta_e + delta_t
  |error of (log10 a - log10 b)^2|       <= 2 |dlog| (delta_e / (m_e + eps) + delta_t / (m_t + eps)) / ln 10 + (the same bracket / ln 10)^2
and a term's bound is the mean of these.  ONE constant, C_FFT, fixed against the reference ALONE: tests/golden/make_golden_mss.py runs
the reference's own code in float32 and in float64 and records, per golden case and term, |fp32 - float64| / bound(c = 1);  C_FFT is
twice the largest ratio, rounded up (the margin covers another FFT factorisation at the same precision).

Spectrogram elements.  delta is a statement about a frame's error in the rms sense (the classic result bounds the NORM of a floating-point
FFT's error by c eps log2(n) times the norm of the spectrum); taken per element it cannot hold on a peaked spectrum: the rounding errors of
the butterflies are relative to the partial sums, and bin k's own partial sums reach |X_k|, which on a 1 kHz sine is 37 rho at n = 4096.
There even the float64 value ROUNDED to float32 misses delta(c = 1) by 2.5 x, and the reference's own float32 run misses it by 10 x (12 x
on the real bass stem; make_golden_mss.py prints these for every case).  So an element is held to
    delta_elem = C_ELEM 2^-24 log2(n) (rho + m_k)
- the frame's level plus the bin's own magnitude, which also covers the float32 representation of the result - with C_ELEM fixed by the
same rule against the reference alone over ALL elements of the golden spectrograms (the worst sit at the mirror images of strong bins,
where a real transform cancels two large numbers), and every FRAME is still held to delta itself in the sense delta is true in:
sqrt(mean_k err_k^2) <= delta at C_FFT.
"""
import math

import numpy as np

# Reference alone, |fp32 - float64| / bound(c = 1), the largest over the terms of each case of tests/golden/mss.npz (magnitude term, log term):
#   noise 0.0010 0.0210 | noise_odd 0.0006 0.0389 | noise_ori 0.0009 0.0193 | noise_hamming 0.0007 0.0412 | noise_shortwin 0.0012 0.0091
#   lowpass 0.0054 0.0017 | silence 0.1147 0 | mono 0.0011 0.0088 | identical 0 0 | sine 0.0038 0.0017 | sine_ori 0.0052 0.0012
#   real_drums 0.0335 0.0021 | real_bass 0.0109 0.0007
# (a sum of many signed per-bin errors: far under a bound made of absolute values; the largest, 0.1147, is silence against noise, where
# |m_e - m_t| = m_t - m_e keeps the sign of every error).  Twice the largest, rounded up:
MEASURED_MAX_RATIO = 0.1147
C_FFT = 1.0
# Reference alone over all elements of the golden spectrograms, max |fp32 - float64| / delta_elem(c = 1):
#   noise 0.564 | noise_odd 0.585 | noise_ori 0.564 | noise_hamming 0.570 | noise_shortwin 0.542 | lowpass 0.905 | silence 0.535 | mono 0.504
#   identical 0.525 | sine 1.912 | sine_ori 1.912 | real_drums 4.094 | real_bass 4.256
# (against the plain delta(c = 1): up to 12.065, and 2.648 for float64 values merely rounded to float32).  Twice the largest, rounded up:
MEASURED_MAX_RATIO_ELEM = 4.256
C_ELEM = 9.0

DEFAULT_SCALES = ((4096, 1024, 4096), (2048, 512, 2048), (1024, 256, 1024), (512, 128, 512))      # (n_fft, hop, win_length)
MAG_WEIGHT, LOG_WEIGHT, MID_WEIGHT = 0.9, 0.1, 0.5
MAG_EPS = 1e-7          # FrontEnd.mag's own eps, under the square root


def window(kind, win_length, n_fft):
    i = np.arange(win_length, dtype=np.float64)
    cs = np.cos(2.0 * np.pi * i / win_length)
    w = {"hann": 0.5 - 0.5 * cs, "hamming": 0.54 - 0.46 * cs}[kind]
    out = np.zeros(n_fft)
    left = (n_fft - win_length) // 2
    out[left:left + win_length] = w
    return out


def n_frames(L, n_fft, hop):
    return 1 + L // hop - (1 if L % round(n_fft / 4) == 0 else 0)


def spectrum(x, n_fft, hop, win_length=None, kind="hann"):
    """x float64 [..., L] -> complex [..., n_fft / 2 + 1, T] (all bins, quirk 1 applied)."""
    x = np.asarray(x, dtype=np.float64)
    L = x.shape[-1]
    assert L > n_fft // 2
    w = window(kind, n_fft if win_length is None else win_length, n_fft)
    pad = n_fft // 2
    xp = np.concatenate([x[..., pad:0:-1], x, x[..., -2:-pad - 2:-1]], axis=-1)
    T = n_frames(L, n_fft, hop)
    idx = (np.arange(T) * hop)[:, None] + np.arange(n_fft)[None, :]
    X = np.fft.rfft(xp[..., idx] * w, axis=-1)                   # [..., T, bins]
    return np.swapaxes(X, -1, -2)


def mag_and_level(x, n_fft, hop, win_length=None, kind="hann"):
    """m [..., n_fft / 2, T] over bins 1 .. n_fft / 2 and the frames' rms spectral level rho [..., 1, T]."""
    X = spectrum(x, n_fft, hop, win_length, kind)
    p = X.real ** 2 + X.imag ** 2
    return np.sqrt(p[..., 1:, :] + MAG_EPS), np.sqrt(p.mean(axis=-2, keepdims=True))


def delta(rho, n_fft, c=None):
    return (C_FFT if c is None else c) * 2.0 ** -24 * math.log2(n_fft) * rho


def front_end(x, n_fft, hop=None, win_length=None, kind="hann", c=None, c_frame=None):
    """FrontEnd(...).forward(x, mode=["mag"]) in float64: x [B, C, L] -> (mag [B, C, F, T], the elementwise bound delta_elem of the same
    shape, the frames' bound delta [B, C, 1, T] on the rms error over a frame's bins)."""
    m, rho = mag_and_level(x, n_fft, n_fft // 4 if hop is None else hop, win_length, kind)
    return m, delta(rho + m, n_fft, C_ELEM if c is None else c), delta(rho, n_fft, c_frame)


def front_end_ratios(got, x, n_fft, hop=None, win_length=None, kind="hann"):
    """(max element error / delta_elem, max frame rms error / delta, max element error / the plain delta - the last a recorded figure, not
    a bound: see the module's text) of a float32 spectrogram `got` against the float64 one; an error where the bound is zero counts as
    infinite"""
    ref, be, bf = front_end(x, n_fft, hop, win_length, kind)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    rms = np.sqrt((err ** 2).mean(axis=-2, keepdims=True))

    def ratio(e, b):
        r = np.divide(e, b, out=np.zeros_like(e), where=b > 0)
        r[(b == 0) & (e > 0)] = np.inf
        return float(r.max())
    return ratio(err, be), ratio(rms, bf), ratio(err, np.broadcast_to(bf, err.shape))


def channels(x, mode):
    x = np.asarray(x, dtype=np.float64)
    if mode == "midside":
        return np.stack([x[:, 0] + x[:, 1], x[:, 0] - x[:, 1]], axis=1)
    assert mode == "ori"
    return x[:, :2]


def terms(est, tgt, mode="midside", scales=DEFAULT_SCALES, kind="hann", eps=1e-7, c=None):
    """est, tgt [B, 2, L] -> (values, bounds), both float64 [B, n_scales, 2, 2]: per item, scale, channel (mid, side / left, right) the
    magnitude term and the log term as means over that item's bins and frames, and the derived bound of each."""
    e, t = channels(est, mode), channels(tgt, mode)
    B = e.shape[0]
    val = np.zeros((B, len(scales), 2, 2))
    bnd = np.zeros_like(val)
    ln10 = math.log(10.0)
    for s, (n_fft, hop, win_length) in enumerate(scales):
        me, re_ = mag_and_level(e, n_fft, hop, win_length, kind)
        mt, rt = mag_and_level(t, n_fft, hop, win_length, kind)
        d = delta(re_ + rt, n_fft, c)                      # both levels charged to both signals
        dlog = np.log10(me + eps) - np.log10(mt + eps)
        rel = (d / (me + eps) + d / (mt + eps)) / ln10
        val[:, s, :, 0] = np.abs(me - mt).mean(axis=(-1, -2))
        val[:, s, :, 1] = (dlog ** 2).mean(axis=(-1, -2))
        bnd[:, s, :, 0] = np.broadcast_to(2.0 * d, me.shape).mean(axis=(-1, -2))
        bnd[:, s, :, 1] = (2.0 * np.abs(dlog) * rel + rel ** 2).mean(axis=(-1, -2))
    return val, bnd


def total(values):
    """The loss value of a batch from terms()'s values (or bounds: the combination is linear with positive weights)."""
    v = np.asarray(values).mean(axis=0)                    # every item has the same number of bins and frames
    ch = MID_WEIGHT * v[:, 0, :] + (1.0 - MID_WEIGHT) * v[:, 1, :]
    return float(MAG_WEIGHT * ch[:, 0].sum() + LOG_WEIGHT * ch[:, 1].sum())


def loss(est, tgt, mode="midside", scales=DEFAULT_SCALES, kind="hann", eps=1e-7, c=None):
    val, bnd = terms(est, tgt, mode, scales, kind, eps, c)
    return total(val), total(bnd)


def probe_positions(size, n=1021):
    """flat positions of the stored spectrogram probes: n positions an odd stride apart (an odd stride walks through bins and frames)"""
    if size <= n:
        return np.arange(size)
    return np.arange(n) * ((size // n) | 1)


# ---- the golden cases: integer recipes, no stored audio -------------------------------------------------------------------
def _noise(seed, shape):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=shape).astype(np.float32)


def _lowpass(x, taps=64):
    k = np.hanning(taps + 2)[1:-1]
    k /= k.sum()
    return np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), -1, x)


def case_inputs(name, length=None):
    """(est, tgt, kwargs of terms()) of a golden case, float32 arrays [B, 2, L]; `length` overrides the case's own L (the emulator tests
    run shorter signals of the same recipe)."""
    scales = DEFAULT_SCALES
    kw = {"mode": "midside", "scales": scales, "kind": "hann", "eps": 1e-7}
    base = name.split("@")[0]
    L = {"noise_odd": 131000}.get(base, 131072) if length is None else length
    if base in ("noise", "noise_odd", "noise_ori", "noise_hamming", "noise_shortwin"):
        tgt = _noise(11, (2, 2, L))
        est = (tgt + np.float32(0.05) * _noise(12, (2, 2, L))).astype(np.float32)
        if base == "noise_ori":
            kw["mode"] = "ori"
        if base == "noise_hamming":
            kw["kind"] = "hamming"
        if base == "noise_shortwin":
            kw["scales"] = ((2048, 512, 1200), (512, 128, 400))
    elif base == "lowpass":
        tgt = (np.float32(0.01) * _lowpass(_noise(21, (2, 2, L)))).astype(np.float32)
        est = (np.float32(0.5) * tgt).astype(np.float32)
    elif base == "silence":
        est = np.zeros((2, 2, L), np.float32)
        tgt = _noise(31, (2, 2, L))
    elif base == "mono":
        a, b = _noise(41, (2, 1, L)), _noise(42, (2, 1, L))
        tgt = np.concatenate([a, a], axis=1)
        e1 = (a + np.float32(0.05) * b).astype(np.float32)
        est = np.concatenate([e1, e1], axis=1)
    elif base == "identical":
        tgt = _noise(51, (2, 2, L))
        est = tgt.copy()
    elif base in ("sine", "sine_ori"):
        t = np.arange(L, dtype=np.float64) / 44100.0
        s = np.sin(2.0 * np.pi * 1000.0 * t)
        tgt = np.stack([np.stack([0.5 * s, 0.4 * s]), np.stack([0.3 * s, 0.3 * np.roll(s, 7)])]).astype(np.float32)
        est = (np.float32(0.25) * tgt).astype(np.float32)
        if base == "sine_ori":
            kw["mode"] = "ori"
    elif base in ("real_drums", "real_bass"):
        import os
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "real_audio.npz"))
        stem = base.split("_")[1]
        n = 1 << 19 if length is None else length
        est = _stem(z, "input", stem)[None, :, :n]
        tgt = _stem(z, "reference", stem)[None, :, :n]
    else:
        raise KeyError(name)
    return np.ascontiguousarray(est, dtype=np.float32), np.ascontiguousarray(tgt, dtype=np.float32), kw


def _stem(z, which, stem):
    """real_audio.npz keeps each stem as packed 16-bit PCM [L, 2] (tests/golden/real_audio.py); -> float32 [2, L] in [-1, 1)."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("_mss_real_audio", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "real_audio.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return (mod.unpack(z[f"pcm/{which}/{stem}"]).astype(np.float32) / np.float32(32768.0)).T


CASES = ("noise", "noise_odd", "noise_ori", "noise_hamming", "noise_shortwin", "lowpass", "silence", "mono", "identical", "sine", "sine_ori",
         "real_drums", "real_bass")
