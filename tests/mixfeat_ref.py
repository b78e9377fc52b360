"""TEST INFRASTRUCTURE: the mixing-feature errors (reference mixing_manipulator/utils_data_normalization.py compute_loudness_features /
compute_panning_features / compute_dynamic_features :483-905 and their helpers) in numpy, in this project's own words, twice:

  * `exact`: float64 from the peak-normalised float32 samples on - what the reference's formulas mean.  The kernels (csrc/mixfeat_kernels.h)
    are held to THIS, within bounds derived below from the operands.
  * `rounded`: the same formulas in the number formats the reference really runs in - its STFT is float64 rounded to complex64, so phi, SPS,
    the band sums, the dB values, the running means and the errors are float32 arithmetic (NumPy >= 2 promotion: a Python scalar does not
    widen a float32).  tests/test_mixfeat_reference.py holds this to the goldens (tests/golden/mixfeat.npz, the REAL reference's output) at
    1e-9.  |rounded - exact| is the reference's own error; a test that compares the product with a golden adds it to the bound.

The bounds.  u = 2^-24.  The transform is csrc/mss_kernels.h's, so a bin magnitude m_k of a frame with rms spectral level rho carries
    delta_k = C_ELEM u log2(n) (rho + m_k)                                  (tests/mss_ref.py: C_ELEM = 9 fixed against the reference alone)
Panning.  With l, r the two magnitudes, SPS^2 = q^2, q = (l - r)^2 / (l^2 + r^2) in [0, 1].  Replacing l, r by values within dl, dr:
    dq <= [2 |l - r| (dl + dr) + (dl + dr)^2] / (l^2 + r^2)  +  q 2 (l dl + r dr) / (l^2 + r^2)
(numerator exactly, denominator in first order), capped by q's range 1;  d(q^2) <= 2 q dq + dq^2, capped by 1; a band sum's bound is the
sum of its bins' bounds, and p_rms = sqrt(S / nbins) is evaluated at S -+ dS.  l == r in every bin (mono, digital silence) has bound 0 and
the kernel gives exactly 0.
Low ratio.  R = sum_k A_k / (B_k + 1e-5), A the low-passed signal's magnitudes:  dR <= sum_k [dA_k + (A_k / (B_k + 1e-5)) dB_k] / (B_k + 1e-5)
with dB_k = delta_k and dA_k = delta_k(A) + sum_n w_n e_n, e_n the bound on sample n of the low-passed signal: the device filters in
float64 but hands the signal from the forward to the backward pass, and out of the backward pass, as float32 -
    e_n = u (sum_j |h_j| |y1_{n + j}| + |x_low_n|)  +  2^-40 max_n |x_n|  +  2^-126 (sum_j |h_j| + 1)
(y1 the forward pass, h the filter's impulse response; the middle term covers the float64 recursions themselves - second-order sections
run as a time-parallel scan there, scipy's transfer-function form here: a float64 recursion's roundings are relative to the largest values
in the filter's memory, not to the output sample, so where the output is a free decay into a stretch of silence, 20 orders of magnitude
below the signal that started it, no pointwise relative bound holds and the floor is 2^-53 of full scale with 13 bits of margin; the last
is float32's underflow: a rounding to float32 is relative only down to the smallest normal number 2^-126, below it the value may go to
zero - in a stretch of digital silence the filter's tail decays through 1e-38 to 1e-200, which float64 holds and float32 does not).
Dynamics.  The kernel's operands are the same float32 products x * gain as numpy's, and everything after is float64: what is left is the
summation order and log10's last bits, (F + 8) 2^-52 sum |term| per frame sum (F the frame length); max |x| is exact.
Loudness.  The BS.1770 meter (fx_utils.Meter) rounds each of its two filter stages to float32.  For a gating block with stage outputs y1,
y2: |dy2| <= u |y2| + u (|h2| * |y1|), so a block's energy moves by at most 2 u (1 + ||(|h2| * |y1|)|| / ||y2||) of itself (norms over the
block), and a loudness - 10 log10 of a mean of block energies - by (10 / ln 10) times the largest such factor.
Every sequence bound is pushed through the running mean (linear, positive weights) and through |t - o| / |t| with
    d(|t - o| / |t|) <= (dt + do) / (|t| - dt) + |t - o| dt / (|t| (|t| - dt)).
"""
import math
import os

import numpy as np
import scipy.signal

from mss_ref import C_ELEM, C_FFT, _noise, _stem

U = 2.0 ** -24
EPS64 = float(np.finfo(np.float64).eps)
N_RUN = 40
SR = 44100


# ---- shared pieces ------------------------------------------------------------------------------------------------------------
def window(n_fft):
    return np.sqrt(np.hanning(n_fft + 1)[:-1])


def n_frames(L, n_fft, hop):
    return 1 + (L - n_fft) // hop


def peak_gain(x, target_db=-1.0):
    """pyloudnorm.normalize.peak's factor as the float32 a float32 signal is multiplied by"""
    return np.float32(np.power(10.0, target_db / 20.0) / np.max(np.abs(x)))


def peak_normalize(x):
    x = np.asarray(x, dtype=np.float32)
    return x * peak_gain(x)


def stft(x, n_fft, hop):
    """x [L] -> complex128 [T, n_fft / 2 + 1], librosa.stft(center=False) framing"""
    x = np.asarray(x)
    T = n_frames(len(x), n_fft, hop)
    idx = (np.arange(T) * hop)[:, None] + np.arange(n_fft)[None, :]
    return np.fft.rfft(x[idx] * window(n_fft), axis=-1)


def frame_weighted_sum(v, n_fft, hop):
    """sum_n w_n v_n of every frame"""
    T = n_frames(len(v), n_fft, hop)
    idx = (np.arange(T) * hop)[:, None] + np.arange(n_fft)[None, :]
    return (v[idx] * window(n_fft)).sum(axis=-1)


def delta_elem(mag, n_fft):
    """the bound of every bin magnitude of [T, bins] magnitudes"""
    rho = np.sqrt((mag ** 2).mean(axis=-1, keepdims=True))
    return C_ELEM * U * math.log2(n_fft) * (rho + mag)


def delta_frame(mag, n_fft):
    """the bound on a frame's rms error over its bins"""
    return C_FFT * U * math.log2(n_fft) * np.sqrt((mag ** 2).mean(axis=-1))


def band_bins(sr, n_fft, freqs=None):
    freqs = [[0, sr // 2], [0, 250], [250, 2500], [2500, sr // 2]] if freqs is None else freqs
    return [(int(np.floor(f[0] * n_fft / sr)), int(np.floor(f[1] * n_fft / sr))) for f in freqs]


def running_mean(x, N=N_RUN):
    c = np.concatenate(([0.0], np.cumsum(np.asarray(x, dtype=np.float64))))
    return (c[N:] - c[:-N]) / float(N)


def mape(t, o):
    t, o = np.asarray(t, dtype=np.float64), np.asarray(o, dtype=np.float64)
    return float(np.mean(np.abs(t - o) / np.maximum(np.abs(t), EPS64)))


def mape_bound(t, o, dt, do):
    t, o, dt, do = (np.asarray(v, dtype=np.float64) for v in (t, o, dt, do))
    at = np.abs(t)
    with np.errstate(divide="ignore", invalid="ignore"):
        b = (dt + do) / (at - dt) + np.abs(t - o) * dt / (at * (at - dt))
    b = np.where((dt + do) == 0, 0.0, np.where(at > dt, b, np.inf))
    return float(np.mean(b))


def mse(t, o):
    t, o = np.asarray(t, dtype=np.float64), np.asarray(o, dtype=np.float64)
    return float(np.mean((t - o) ** 2))


def mse_bound(t, o, dt, do):
    d = np.asarray(dt, dtype=np.float64) + np.asarray(do, dtype=np.float64)
    return float(np.mean(2.0 * np.abs(np.asarray(t, dtype=np.float64) - np.asarray(o, dtype=np.float64)) * d + d * d))


def _mape32(t, o):
    """sklearn.metrics.mean_absolute_percentage_error on float32 arrays: float32 arithmetic"""
    t, o = np.asarray(t), np.asarray(o)
    if t.dtype != np.float32 or o.dtype != np.float32:
        return mape(t, o)
    e = np.abs(o - t) / np.maximum(np.abs(t), np.float32(EPS64))
    return float(np.average(np.average(e, axis=0)))


def _mse32(t, o):
    t, o = np.asarray(t), np.asarray(o)
    if t.dtype != np.float32 or o.dtype != np.float32:
        return mse(t, o)
    return float(np.average(np.average((t - o) ** 2, axis=0)))


def _running_mean_rounded(x, N):
    """the reference's running mean in x's own dtype (a float32 sequence stays float32)"""
    c = np.cumsum(np.insert(x, 0, 0))
    return (c[N:] - c[:-N]) / float(N)


def _stats_rounded(x, n_features, N=N_RUN):
    return np.asarray([_running_mean_rounded(x[:, i], N) for i in range(n_features)])


# ---- panning ------------------------------------------------------------------------------------------------------------------
def sps_exact(xn, n_fft, hop):
    """xn [L, 2] peak-normalised float32 -> phi, SPS, dq2 (the bound of SPS^2), all float64 [T, bins]"""
    X = [stft(xn[:, c].astype(np.float64), n_fft, hop) for c in range(2)]
    l, r = (np.abs(v + 1e-20) for v in X)
    dl, dr = delta_elem(l, n_fft), delta_elem(r, n_fft)
    den = l * l + r * r
    phi = 2.0 * l * r / den
    q = (l - r) ** 2 / den
    sps = q * np.sign(r - l)
    dq = np.minimum(1.0, (2.0 * np.abs(l - r) * (dl + dr) + (dl + dr) ** 2) / den + q * 2.0 * (l * dl + r * dr) / den)
    dq = np.where(l == r, 0.0, dq)          # the same bits through the same instructions
    dq2 = np.minimum(1.0, 2.0 * q * dq + dq * dq)
    return phi, sps, dq2


def sps_rounded(xn, n_fft, hop):
    """get_SPS in the reference's formats: complex64 spectra, float32 arithmetic -> SPS_mean, phi_mean, SPS, phi"""
    D = np.stack([stft(xn[:, c], n_fft, hop).astype(np.complex64) for c in range(2)], axis=1)
    l, r = np.abs(D[:, 0, :] + 1e-20), np.abs(D[:, 1, :] + 1e-20)
    phi = 2 * (l * r) / (l ** 2 + r ** 2)
    delta = (l * r) / (l ** 2) - (r * l) / (r ** 2)
    sps = (1 - phi) * np.sign(delta)
    return np.mean(sps, axis=0), np.mean(phi, axis=0), sps, phi


def panning_frames(xn, sr, n_fft, hop):
    """-> dict: S, dS (band sums of SPS^2 and their bounds, [T, 4]), p_rms, dp (its bound), p_rms_rounded (the reference's formats)"""
    _, sps, dq2 = sps_exact(xn, n_fft, hop)
    bands = band_bins(sr, n_fft)
    S = np.stack([(sps[:, a:b] ** 2).sum(axis=1) for a, b in bands], axis=1)
    dS = np.stack([dq2[:, a:b].sum(axis=1) for a, b in bands], axis=1)
    nb = np.asarray([b - a for a, b in bands], dtype=np.float64)
    p = np.sqrt(S / nb)
    dp = np.maximum(np.sqrt((S + dS) / nb) - p, p - np.sqrt(np.maximum(S - dS, 0.0) / nb))
    sr32 = sps_rounded(xn, n_fft, hop)[2]
    pr = np.asarray([[np.sqrt((1 / (b - a)) * np.sum(fr[a:b] ** 2)) for a, b in bands] for fr in sr32])
    return {"S": S, "dS": dS, "p_rms": p, "dp": dp, "p_rms_rounded": pr}


def _delete_zero_frames(p_tar, p_out, *more):
    if np.min(p_tar) == 0.0:
        keep = p_tar[:, 0] != 0
        return (p_tar[keep], p_out[keep]) + tuple(m[keep] for m in more)
    return (p_tar, p_out) + more


PANNING_KEYS = ("P_t_mean", "P_l_mean", "P_m_mean", "P_h_mean")


def panning_features(out, tar, sr, n_fft, hop):
    """-> (exact, bound, rounded) dictionaries of compute_panning_features, and the two frame dictionaries"""
    fo, ft = panning_frames(peak_normalize(out), sr, n_fft, hop), panning_frames(peak_normalize(tar), sr, n_fft, hop)
    pt, po, dpt, dpo = _delete_zero_frames(ft["p_rms"], fo["p_rms"], ft["dp"], fo["dp"])
    exact, bound = {}, {}
    for i, k in enumerate(PANNING_KEYS):
        mt, mo = running_mean(pt[:, i]), running_mean(po[:, i])
        exact[k] = mape(mt, mo)
        bound[k] = mape_bound(mt, mo, running_mean(dpt[:, i]), running_mean(dpo[:, i]))
    exact["mape_mean"] = float(np.mean([exact[k] for k in PANNING_KEYS]))
    bound["mape_mean"] = float(np.mean([bound[k] for k in PANNING_KEYS]))
    rt, ro = _delete_zero_frames(ft["p_rms_rounded"], fo["p_rms_rounded"])
    mt, mo = _stats_rounded(rt, 4), _stats_rounded(ro, 4)
    rounded = {k: _mape32(mt[i], mo[i]) for i, k in enumerate(PANNING_KEYS)}
    rounded["mape_mean"] = float(np.mean([[rounded[k]] for k in PANNING_KEYS]))
    return exact, bound, rounded, fo, ft


# ---- dynamics -----------------------------------------------------------------------------------------------------------------
def _db(x):
    return 20 * np.log10(x + 1e-30)


def frame_sums(xn, frame, hop):
    """xn [L, C] float32 -> sums float64 [C, T, 3] (sum x^2, sum 20 log10(|x| + 1e-30), max |x|) and their bounds"""
    x = np.abs(np.asarray(xn, dtype=np.float64))
    T = n_frames(x.shape[0], frame, hop)
    idx = (np.arange(T) * hop)[:, None] + np.arange(frame)[None, :]
    fr = x.T[:, idx]                                                  # [C, T, frame]
    db = _db(fr)
    sums = np.stack([(fr ** 2).sum(-1), db.sum(-1), fr.max(-1)], axis=-1)
    g = (frame + 8) * 2.0 ** -52
    bnd = np.stack([g * (fr ** 2).sum(-1), g * np.abs(db).sum(-1), np.zeros(sums.shape[:-1])], axis=-1)
    return sums, bnd


def _rdc(s2, sl, mx, frame):
    rms = _db(np.sqrt(s2 / frame))
    with np.errstate(divide="ignore", invalid="ignore"):
        return rms, (sl - frame * rms) / frame, _db(mx) / rms


def dynamics_frames(xn, frame, hop):
    """rms / dynamic spread / crest [T] as means over the channels, with bounds, and in the reference's formats"""
    sums, bnd = frame_sums(xn, frame, hop)
    s2, sl, mx = sums[..., 0], sums[..., 1], sums[..., 2]
    rms, dyn, crest = _rdc(s2, sl, mx, frame)
    lo, hi = _rdc(np.maximum(s2 - bnd[..., 0], 0.0), sl, mx, frame)[0], _rdc(s2 + bnd[..., 0], sl, mx, frame)[0]
    d_rms = np.maximum(hi - rms, rms - lo)
    d_dyn = bnd[..., 1] / frame + d_rms
    with np.errstate(divide="ignore", invalid="ignore"):
        d_crest = np.maximum(np.abs(_db(mx) / (rms + d_rms) - crest), np.abs(_db(mx) / (rms - d_rms) - crest))
    out = {"sums": sums, "sums_bound": bnd, "rms": rms.mean(0), "dyn": dyn.mean(0), "crest": crest.mean(0), "d_rms": d_rms.mean(0),
           "d_dyn": d_dyn.mean(0), "d_crest": d_crest.mean(0)}
    # the reference's loop, float32 throughout
    xr = np.asarray(xn)
    T = n_frames(xr.shape[0], frame, hop)
    seq = [[], [], []]
    for ch in range(xr.shape[-1]):
        frames = np.stack([xr[i * hop:i * hop + frame, ch] for i in range(T)], 1)
        r_, d_, c_ = [], [], []
        for i in frames.T:
            x_rms = _db(np.sqrt(np.sum(i ** 2) / frame))
            r_.append(x_rms)
            d_.append(np.sum(_db(np.abs(i)) - x_rms) / frame)
            c_.append(_db(np.max(np.abs(i))) / x_rms)
        for s, v in zip(seq, (r_, d_, c_)):
            s.append(v)
    out["rms_rounded"], out["dyn_rounded"], out["crest_rounded"] = (np.mean(np.asarray(s), axis=0) for s in seq)
    return out


# ---- low-frequency ratio ------------------------------------------------------------------------------------------------------
def lowpass(xn, f0=1000, sr=SR):
    """the reference's lowpassFiltering: scipy's filtfilt of a 4th-order Butterworth, per channel -> float64 [L, C]"""
    b, a = scipy.signal.butter(4, f0 / (sr / 2), "lowpass")
    return np.asarray([scipy.signal.filtfilt(b, a, xn[:, ch]).copy(order="F") for ch in range(xn.shape[-1])]).T


def lowpass_sample_bound(xn, f0=1000, sr=SR, taps=4096):
    """e_n of the module's text, [L, C]"""
    b, a = scipy.signal.butter(4, f0 / (sr / 2), "lowpass")
    h = np.abs(scipy.signal.lfilter(b, a, np.concatenate(([1.0], np.zeros(taps - 1)))))
    edge = 15
    out = np.zeros(xn.shape)
    for ch in range(xn.shape[-1]):
        x = np.asarray(xn[:, ch])
        ext = np.concatenate((2 * x[0] - x[edge:0:-1], x, 2 * x[-1] - x[-2:-edge - 2:-1]))
        zi = scipy.signal.lfilter_zi(b, a)
        y1 = scipy.signal.lfilter(b, a, ext, zi=zi * ext[0])[0]
        y2 = scipy.signal.lfilter(b, a, y1[::-1], zi=zi * y1[-1])[0][::-1]
        a1 = np.concatenate((np.abs(y1), np.full(taps, abs(y1[-1]))))
        corr = scipy.signal.fftconvolve(a1, h[::-1], mode="full")[taps - 1:taps - 1 + len(y1)]      # sum_j |h_j| |y1_{n + j}|
        corr = np.maximum(corr, 0.0)          # the FFT convolution's own noise (1e-16 of the largest value) is below the 2^-40 floor
        e = U * (corr + np.abs(y2)) + 2.0 ** -40 * np.max(np.abs(x)) + 2.0 ** -126 * (h.sum() + 1.0)
        out[:, ch] = e[edge:edge + len(x)]
    return out


def low_ratio_frames(xn, sr, n_fft, hop, f0=1000):
    """-> dict: per_channel [C, T] and its bound, ratio [T] (the mean over the channels), d_ratio, ratio_rounded"""
    x_low = lowpass(xn, f0, sr)
    e = lowpass_sample_bound(xn, f0, sr)
    per, bnd = [], []
    for ch in range(xn.shape[-1]):
        A, B = np.abs(stft(x_low[:, ch], n_fft, hop)), np.abs(stft(xn[:, ch].astype(np.float64), n_fft, hop))
        dA = delta_elem(A, n_fft) + frame_weighted_sum(e[:, ch], n_fft, hop)[:, None]
        dB = delta_elem(B, n_fft)
        ratio = A / (B + 1e-5)
        per.append(ratio.sum(-1))
        bnd.append(((dA + ratio * dB) / (B + 1e-5)).sum(-1))
    per, bnd = np.asarray(per), np.asarray(bnd)
    # the reference's formats: complex64 spectra [frames, channels, bins], transposed views, float32 arithmetic
    def spec(sig):
        s = np.empty((n_frames(sig.shape[0], n_fft, hop), sig.shape[1], n_fft // 2 + 1), dtype=np.complex64)
        for c in range(sig.shape[1]):
            s[:, c, :] = stft(sig[:, c], n_fft, hop).astype(np.complex64)
        return np.abs(np.transpose(s, axes=[1, -1, 0]))
    r = spec(x_low) / (spec(np.asarray(xn)) + 1e-5)
    rounded = np.mean(np.sum(r, axis=1), axis=0)
    return {"per_channel": per, "per_channel_bound": bnd, "ratio": per.mean(0), "d_ratio": bnd.mean(0), "ratio_rounded": rounded}


DYNAMIC_KEYS = ("rms_mean", "dyn_mean", "crest_mean", "l_ratio_mean_mape", "l_ratio_mean_l2", "mape_mean")


def dynamic_features(out, tar, sr, n_fft, hop):
    """-> (exact, bound, rounded) dictionaries of compute_dynamic_features, and (dynamics, low ratio) frame dictionaries of out and tar"""
    no, nt = peak_normalize(out), peak_normalize(tar)
    do, dt = dynamics_frames(no, n_fft, hop), dynamics_frames(nt, n_fft, hop)
    lo, lt = low_ratio_frames(no, sr, n_fft, hop), low_ratio_frames(nt, sr, n_fft, hop)
    exact, bound, rounded = {}, {}, {}
    for key, name, f in (("rms_mean", "rms", lambda v: 1.0 - v), ("dyn_mean", "dyn", lambda v: 1.0 - v), ("crest_mean", "crest", lambda v: v)):
        mt, mo = running_mean(f(dt[name])), running_mean(f(do[name]))
        exact[key] = mape(mt, mo)
        bound[key] = mape_bound(mt, mo, running_mean(dt["d_" + name]), running_mean(do["d_" + name]))
        g = (lambda v: (-1 * v) + 1.0) if name != "crest" else (lambda v: v)
        rounded[key] = _mape32(_stats_rounded(g(dt[name + "_rounded"][None]).T, 1), _stats_rounded(g(do[name + "_rounded"][None]).T, 1))
    mt, mo = running_mean(lt["ratio"]), running_mean(lo["ratio"])
    bt, bo = running_mean(lt["d_ratio"]), running_mean(lo["d_ratio"])
    exact["l_ratio_mean_mape"], bound["l_ratio_mean_mape"] = mape(mt, mo), mape_bound(mt, mo, bt, bo)
    exact["l_ratio_mean_l2"], bound["l_ratio_mean_l2"] = mse(mt, mo), mse_bound(mt, mo, bt, bo)
    rt, ro = _stats_rounded(lt["ratio_rounded"][None].T, 1), _stats_rounded(lo["ratio_rounded"][None].T, 1)
    rounded["l_ratio_mean_mape"], rounded["l_ratio_mean_l2"] = _mape32(rt, ro), _mse32(rt, ro)
    for d in (exact, bound):
        d["mape_mean"] = float(np.mean([d["rms_mean"], d["dyn_mean"], d["crest_mean"]]))
    rounded["mape_mean"] = float(np.mean([[rounded["rms_mean"]], [rounded["dyn_mean"]], [rounded["crest_mean"]]]))
    return exact, bound, rounded, (do, lo), (dt, lt)


# ---- loudness -----------------------------------------------------------------------------------------------------------------
def _oracle():
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if repo not in sys.path:
        sys.path.insert(0, repo)
    from oracle import normalizer_ref
    return normalizer_ref


def loudness_bound(x, sr, taps=65536):
    """the bound on fx_utils.Meter's loudness of x [L, C] float32 (see the module's text), in LU"""
    N = _oracle()
    (b1, a1), (b2, a2) = N._kweighting(sr)
    h2 = np.abs(scipy.signal.lfilter(b2, a2, np.concatenate(([1.0], np.zeros(taps - 1)))))
    n = x.shape[0]
    blk, step = 0.4, 0.25
    n_blocks = int(np.round(((n / sr - blk) / (blk * step))) + 1)
    worst = 0.0
    for ch in range(x.shape[1]):
        y1 = scipy.signal.lfilter(b1, a1, x[:, ch].astype(np.float64))
        y2 = scipy.signal.lfilter(b2, a2, y1)
        c = scipy.signal.fftconvolve(np.abs(y1), h2, mode="full")[:n]
        for j in range(n_blocks):
            lo, hi = int(blk * (j * step) * sr), int(blk * (j * step + 1) * sr)
            e2 = np.sqrt(np.sum(y2[lo:hi] ** 2))
            if e2 > 0:
                worst = max(worst, 2.0 * U * (1.0 + np.sqrt(np.sum(c[lo:hi] ** 2)) / e2))
    return 10.0 / math.log(10.0) * worst


def loudness_features(out, tar, sr):
    """-> (exact, bound, rounded) dictionaries of compute_loudness_features"""
    N = _oracle()
    out, tar = np.asarray(out, dtype=np.float32), np.asarray(tar, dtype=np.float32)
    lt, lo = (float(N.integrated_loudness(v.astype(np.float64), sr)) for v in (tar, out))
    pt, po = (20.0 * math.log10(float(np.max(np.abs(v)))) for v in (tar, out))
    exact = {"d_lufs": mape([lt], [lo]), "d_peak": mape([pt], [po])}
    bound = {"d_lufs": mape_bound([lt], [lo], [loudness_bound(tar, sr)], [loudness_bound(out, sr)]),
             "d_peak": mape_bound([pt], [po], [4 * EPS64 * abs(pt)], [4 * EPS64 * abs(po)])}
    rt, ro = (N.integrated_loudness(v, sr) for v in (tar, out))
    qt, qo = (20.0 * np.log10(np.max(np.abs(v))) for v in (tar, out))
    # sklearn takes these as lists of one value: float64 arithmetic on the float32 dB values
    rounded = {"d_lufs": mape([rt], [ro]), "d_peak": mape([qt], [qo])}
    return exact, bound, rounded


# ---- the golden cases ---------------------------------------------------------------------------------------------------------
def _band_pan(s, gains, sr=SR):
    """one noise on both channels with a different (left, right) gain pair per band: FFT-domain masks over the whole signal"""
    S = np.fft.rfft(s.astype(np.float64))
    f = np.fft.rfftfreq(len(s), 1.0 / sr)
    out = np.zeros((len(s), 2))
    for (f0, f1), (gl, gr) in gains:
        band = np.fft.irfft(np.where((f >= f0) & (f < f1), S, 0.0), len(s))
        out[:, 0] += gl * band
        out[:, 1] += gr * band
    return out


PAN = (((0, 250), (0.9, 0.5)), ((250, 2500), (0.4, 0.8)), ((2500, 30000), (0.7, 0.6)))
WIDE = (((0, 250), (0.8, 0.6)), ((250, 2500), (0.6, 0.75)), ((2500, 30000), (0.75, 0.5)))


def _stereo_noise(seed, L, sr=SR):
    """two channels that share most of their content: every band has a stereo image to measure"""
    a, b = _noise(seed, (L,)), _noise(seed + 1, (L,))
    return _band_pan(a, WIDE, sr) + 0.15 * np.stack([b, -b], 1)


def case_inputs(name, length=None):
    """(out, tar, sr, n_fft, hop) of a golden case; out, tar float32 [L, 2]; `length` overrides the case's own (the GPU tests run the same
    recipes at a stem's length)."""
    n_fft, hop = {"noise_512": (512, 256), "noise_4096": (4096, 2048)}.get(name, (2048, 1024))
    # 512 points at a quarter of the rate span what 2048 span at 44.1 kHz: at 44.1 kHz the band below 250 Hz would be two bins, and a
    # per-frame figure made of two Rayleigh-distributed bins has no bound worth the name
    sr = SR // 4 if name == "noise_512" else SR
    L = {"noise_odd": 50001, "noise_4096": 90112, "noise_512": 16384, "real_bass": 65536, "real_drums": 43008}.get(name, 49152)
    L = L if length is None else length
    if name in ("noise_pan", "noise_odd", "noise_512", "noise_4096"):
        # noise_512: seed 101 happens to put a frame's DC bin (a real Gaussian, not a Rayleigh magnitude) at 0.001 of the frame's level, and
        # the bound of that one frame's low band is 7e-3 of its value; the condition on BROADBAND asks for another input, here another seed
        seed = 201 if name == "noise_512" else 101
        tar = _stereo_noise(seed, L, sr)
        out = _band_pan(_noise(seed, (L,)), PAN, sr) + 0.15 * np.stack([_noise(seed + 1, (L,)), -_noise(seed + 1, (L,))], 1)
    elif name == "identical":
        tar = _stereo_noise(111, L)
        out = tar.copy()
    elif name == "mono":
        tar = _stereo_noise(121, L)
        m = 0.5 * _noise(121, (L,)).astype(np.float64)
        out = np.stack([m, m], 1)
    elif name == "silence_gap":
        out = _stereo_noise(131, L)
        tar = 0.8 * _stereo_noise(133, L)
        tar[L // 3:L // 3 + 9000] = 0.0
    elif name == "compressed":
        env = 0.05 + np.abs(np.sin(2.0 * np.pi * 3.0 * np.arange(L) / sr)) ** 4
        tar = _stereo_noise(141, L) * env[:, None]
        out = np.sign(tar) * np.abs(tar) ** 0.6
    elif name == "real_bass":
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "real_audio.npz"))
        start = 2 ** 18
        out = _stem(z, "input", "bass")[:, start:start + L].T
        tar = _stem(z, "reference", "bass")[:, start:start + L].T
    elif name == "real_drums":
        # the densest stretch of the reference's drum stem against a remix of itself (a channel matrix and a mild power-law compression):
        # the only stretch of the committed drum PCM whose frames all keep a bound that says something (BROADBAND below; the "input" drum
        # stem has long kick-only passages and misses that by two orders of magnitude, like the bass)
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "real_audio.npz"))
        start = 243 * 1024
        tar = _stem(z, "reference", "drums")[:, start:start + L].T.astype(np.float64)
        mixed = tar @ np.array([[1.0, 0.15], [-0.1, 0.8]])
        out = np.sign(mixed) * np.abs(mixed) ** 0.85
    else:
        raise KeyError(name)
    return np.ascontiguousarray(out, dtype=np.float32), np.ascontiguousarray(tar, dtype=np.float32), sr, n_fft, hop


CASES = ("noise_pan", "identical", "mono", "silence_gap", "compressed", "real_drums", "real_bass", "noise_odd", "noise_512", "noise_4096")
BROADBAND = ("noise_pan", "noise_odd", "noise_512", "noise_4096", "real_drums")          # the bound itself must stay below 1e-3 of the value
