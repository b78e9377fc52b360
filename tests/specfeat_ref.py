"""TEST INFRASTRUCTURE: the spectral feature errors (reference mixing_manipulator/utils_data_normalization.py compute_spectral_features
:509-679 over librosa.feature.spectral_centroid / _bandwidth / _contrast / _rolloff / _flatness) in numpy, twice, as tests/mixfeat_ref.py
does for its own features:

  * `exact`: float64 from the peak-normalised float32 samples on.  The kernel (csrc/mixfeat_kernels.h, mixfeat_spectral_kernel) and the
    Python function are held to THIS within the bounds below.
  * `rounded`: the librosa 0.9.2 arithmetic, restated from its source because the package is absent, in the number formats it and NumPy
    run in: a complex64 spectrum, float32 magnitudes laid out as the reference's transposed view, util.normalize's float64 length and
    float32 quotient, a float32 cumsum and flatness, float64 valley / peak arrays.  tests/golden/specfeat.npz is the REAL reference
    function run over these restatements (they are its librosa.feature stand-ins), so the golden pins the reference's glue - eps, window
    lengths, which band goes where, the means - and NOT librosa; the definitions themselves are pinned by closed-form anchors
    (tests/test_specfeat_reference.py).

The bounds.  A bin magnitude S_k of a frame carries delta_k = C_ELEM u log2(n) (rho + S_k) (mixfeat_ref.delta_elem, C_ELEM as it
stands); g = (m + 8) 2^-52 covers the float64 summation order (and the last bits of log), relative to the sum of the terms' magnitudes.
    sum S, sum k S, sum P     the sum of the bins' bounds (P = max(amin, S^2) moves by at most max(amin, (S + delta)^2) - P), + g sum
    sum log P                 sum of max(log max(amin, (S + delta)^2) - log P, log P - log max(amin, (S - delta)^2)): amin keeps it finite
    centroid (bins)           dc = sum |k - c| delta_k / (sum S - sum delta)
    F = sum S (k - c)^2       c minimises x -> sum S (k - x)^2, so F(S') <= sum S' (k - c)^2 <= F(S) + sum delta (k - c)^2 and the
                              other way round with c': |dF| <= sum delta (|k - c| + dc)^2
    bandwidth                 B^2 = F / sum S evaluated at (F -+ dF) / (sum S +- d sum S), then the roots
    roll-off                  an index: with cum_k -+ (sum_{j <= k} delta_j + g cum_k) and the threshold 0.85 (sum S -+ d sum S) the first
                              crossing lies in [k_lo, k_hi] - earliest possible, certain at the latest; the kernel's index must lie in it
    k smallest / k largest    a sum of k order statistics is 1-Lipschitz per coordinate and moves only k coordinates' worth: the sum of
                              the band's k largest delta
    contrast                  db = 10 log10 max(1e-10, .) at the ends of the interval; the clip max(db, max db - 80) moves by at most
                              max(own bound, the bound of the array's maximum: the largest bound among the entries that can be it), and
                              by its own bound alone where the clip cannot act
    flatness                  exp(mean log P) / mean P at (sum log P -+ d, sum P +- d)
Sequence bounds go through the running mean and mixfeat_ref.mape_bound like every other feature."""
import os

import numpy as np

import mixfeat_ref as M
from mixfeat_ref import EPS64, SR, mape, mape_bound, n_frames, peak_normalize, running_mean  # noqa: F401

N_RUN, N_FLAT = 40, 800
ROLL, AMIN, TOP_DB = 0.85, 1e-10, 80.0
KEYS = ("centroid_mean", "bandwidth_mean", "contrast_l_mean", "contrast_m_mean", "contrast_h_mean", "rolloff_mean", "flatness_mean")
SEQ = ("centroid", "bandwidth", "rolloff", "flatness", "contrast")
TINY32 = float(np.finfo(np.float32).tiny)


def fft_frequencies(sr, n_fft):
    return np.linspace(0, float(sr) / 2, int(1 + n_fft // 2), endpoint=True)


def contrast_masks(sr, n_fft, fmin=250.0, n_bands=4, quantile=0.02):
    """the issue's band rules, literally, on boolean masks: [(mask of the bins whose values are kept, k)]"""
    f = fft_frequencies(sr, n_fft)
    octa = [0.0] + [fmin * 2.0 ** i for i in range(n_bands + 1)]
    out = []
    for j in range(n_bands + 1):
        mask = (f >= octa[j]) & (f <= octa[j + 1])
        idx = np.flatnonzero(mask)
        if j > 0:
            mask[idx[0] - 1] = True
        if j == n_bands:
            mask[idx[-1] + 1:] = True
        k = max(1, int(np.rint(quantile * mask.sum())))
        if j < n_bands:
            mask[np.flatnonzero(mask)[-1]] = False
        out.append((mask, k))
    return out


def bands(sr, n_fft):
    """[(lo, hi, k)] from the masks (they are contiguous)"""
    out = []
    for mask, k in contrast_masks(sr, n_fft):
        idx = np.flatnonzero(mask)
        assert np.array_equal(idx, np.arange(idx[0], idx[-1] + 1))
        out.append((int(idx[0]), int(idx[-1]) + 1, k))
    return out


# ---- exact --------------------------------------------------------------------------------------------------------------------
def magnitudes(xn_ch, n_fft, hop):
    """one peak-normalised float32 channel [L] -> float64 magnitudes [T, m + 1]"""
    return np.abs(M.stft(np.asarray(xn_ch).astype(np.float64), n_fft, hop))


def exact_slots(S, n_fft, bnds):
    """S [T, m + 1] -> dict: v, b [T, 16] (the kernel's slots and their bounds; slot 3's bound is the interval k_lo, k_hi [T])"""
    T, m = S.shape[0], n_fft // 2
    d = M.delta_elem(S, n_fft)
    g = (m + 8) * 2.0 ** -52
    k = np.arange(m + 1.0)
    v, b = np.zeros((T, 16)), np.zeros((T, 16))
    s0, d0 = S.sum(1), d.sum(1)
    s1 = (S * k).sum(1)
    v[:, 0], b[:, 0] = s0, d0 + g * s0
    v[:, 1], b[:, 1] = s1, (d * k).sum(1) + g * s1
    c = np.where(s0 > 0, s1 / np.where(s0 > 0, s0, 1.0), 0.0)
    dev = np.abs(k[None, :] - c[:, None])
    with np.errstate(divide="ignore", invalid="ignore"):
        dc = np.where(d0 == 0, 0.0, np.where(s0 > d0, (dev * d).sum(1) / (s0 - d0), np.inf))
    F = (S * dev ** 2).sum(1)
    v[:, 2] = F
    with np.errstate(invalid="ignore"):
        b[:, 2] = np.where(d0 == 0, 0.0, (d * (dev + dc[:, None]) ** 2).sum(1)) + g * F
    cum = np.cumsum(S, 1)
    dcum = np.cumsum(d, 1) + g * cum
    thr, dthr = ROLL * s0, ROLL * b[:, 0] + 2 * EPS64 * ROLL * s0
    v[:, 3] = np.argmax(cum >= thr[:, None], 1)
    k_lo = np.argmax(cum + dcum >= (thr - dthr)[:, None], 1)
    sure = cum - dcum >= (thr + dthr)[:, None]
    k_hi = np.where(sure.any(1), np.argmax(sure, 1), m)
    P, Pu, Pl = np.maximum(AMIN, S * S), np.maximum(AMIN, (S + d) ** 2), np.maximum(AMIN, np.maximum(S - d, 0.0) ** 2)
    lp = np.log(P)
    v[:, 4], b[:, 4] = lp.sum(1), np.maximum(np.log(Pu) - lp, lp - np.log(Pl)).sum(1) + 2 * g * np.abs(lp).sum(1)
    v[:, 5], b[:, 5] = P.sum(1), (Pu - P).sum(1) + g * P.sum(1)
    for j, (lo, hi, kk) in enumerate(bnds):
        srt = np.sort(S[:, lo:hi], 1)
        dk = np.sort(d[:, lo:hi], 1)[:, -kk:].sum(1)
        v[:, 6 + 2 * j], v[:, 7 + 2 * j] = srt[:, :kk].sum(1), srt[:, -kk:].sum(1)
        b[:, 6 + 2 * j], b[:, 7 + 2 * j] = dk + g * v[:, 6 + 2 * j], dk + g * v[:, 7 + 2 * j]
    return {"v": v, "b": b, "k_lo": k_lo, "k_hi": k_hi, "dc": dc}


def check_slots(got, ex):
    """the kernel's [T, 16] against exact_slots' dictionary -> {slot: max err / bound}; the roll-off index must lie in [k_lo, k_hi]"""
    out = {}
    for q in range(16):
        if q == 3:
            inside = (got[:, 3] >= ex["k_lo"]) & (got[:, 3] <= ex["k_hi"]) & (got[:, 3] == np.rint(got[:, 3]))
            out[q] = 0.0 if inside.all() else np.inf
            continue
        err, bnd = np.abs(got[:, q] - ex["v"][:, q]), ex["b"][:, q]
        r = np.divide(err, bnd, out=np.zeros_like(err), where=bnd > 0)
        r[(bnd == 0) & (err > 0)] = np.inf
        out[q] = float(r.max()) if r.size else 0.0
    return out


def _db_clipped(x, dx):
    """power_to_db(x) [bands, T] with the top_db clip over the whole array, and its bound"""
    a = 10.0 * np.log10(np.maximum(AMIN, x))
    au, al = 10.0 * np.log10(np.maximum(AMIN, x + dx)), 10.0 * np.log10(np.maximum(AMIN, np.maximum(x - dx, 0.0)))
    da = np.maximum(au - a, a - al)
    dg = da[a + da >= (a - da).max()].max()          # the entries that can be the array's maximum
    gmax = a.max()
    return np.maximum(a, gmax - TOP_DB), np.where(a - da > gmax + dg - TOP_DB, da, np.maximum(da, dg))


def exact_sequences(ex, sr, n_fft, bnds):
    """exact_slots' dictionary -> ({name: sequence}, {name: bound}); contrast [5, T], the others [T]"""
    v, b, m = ex["v"], ex["b"], n_fft // 2
    step = float(sr) / 2 / m
    s0, s1, F, s4, s5 = v[:, 0], v[:, 1], v[:, 2], v[:, 4], v[:, 5]
    b0, b1, bF, b4, b5 = b[:, 0], b[:, 1], b[:, 2], b[:, 4], b[:, 5]
    small = s0 < TINY32
    div = np.where(small, 1.0, s0)
    seq, bnd = {}, {}
    seq["centroid"] = step * s1 / div
    with np.errstate(divide="ignore", invalid="ignore"):
        dcen = np.where(small, b1, ex["dc"] + 4 * EPS64 * s1 / div)
        B2 = F / div
        hi = np.where(small, F + bF, np.where(s0 > b0, (F + bF) / (s0 - b0), np.inf))
        lo = np.where(small, F - bF, (F - bF) / (s0 + b0))
    bnd["centroid"] = step * np.where(b0 == 0, 0.0, dcen)
    seq["bandwidth"] = step * np.sqrt(B2)
    bnd["bandwidth"] = step * np.maximum(np.sqrt(hi) - np.sqrt(B2), np.sqrt(B2) - np.sqrt(np.maximum(lo, 0.0)))
    seq["rolloff"] = step * v[:, 3]
    bnd["rolloff"] = step * np.maximum(ex["k_hi"] - v[:, 3], v[:, 3] - ex["k_lo"])
    n = m + 1.0
    fl = np.exp(s4 / n) / (s5 / n)
    seq["flatness"] = fl
    bnd["flatness"] = np.maximum(np.exp((s4 + b4) / n) / ((s5 - b5) / n) - fl, fl - np.exp((s4 - b4) / n) / ((s5 + b5) / n))
    kq = np.asarray([q[2] for q in bnds], dtype=np.float64)[:, None]
    nb = len(bnds)
    pk, dpk = _db_clipped(v[:, 7:7 + 2 * nb:2].T / kq, b[:, 7:7 + 2 * nb:2].T / kq)
    vl, dvl = _db_clipped(v[:, 6:6 + 2 * nb:2].T / kq, b[:, 6:6 + 2 * nb:2].T / kq)
    seq["contrast"], bnd["contrast"] = pk - vl, dpk + dvl
    seq["valley"], bnd["valley"] = v[:, 6:6 + 2 * nb:2].T / kq, b[:, 6:6 + 2 * nb:2].T / kq
    return seq, bnd


def exact_centroid_bound(S, n_fft, sr):
    """the centroid's own bound sum |f_k - c| delta_k / (sum S - sum delta), [T] in Hz (the conditions on the cases use this one)"""
    m = n_fft // 2
    d = M.delta_elem(S, n_fft)
    k = np.arange(m + 1.0)
    s0, d0 = S.sum(1), d.sum(1)
    c = (S * k).sum(1) / s0
    return float(sr) / 2 / m * (np.abs(k[None, :] - c[:, None]) * d).sum(1) / (s0 - d0)


def channel_exact(xn_ch, sr, n_fft, hop):
    bnds = bands(sr, n_fft)
    ex = exact_slots(magnitudes(xn_ch, n_fft, hop), n_fft, bnds)
    seq, bnd = exact_sequences(ex, sr, n_fft, bnds)
    return ex, seq, bnd


def errors_from_sequences(seq_out, seq_tar, bnd_out=None, bnd_tar=None, mape_fn=mape, stats=None):
    """per channel {name: sequence} of out and tar -> the dictionary (and, with bounds, the bound dictionary)"""
    if stats is None:
        stats = lambda x, N: running_mean(x, N)
    per, perb = {k: [] for k in KEYS}, {k: [] for k in KEYS}
    for c, (so, st) in enumerate(zip(seq_out, seq_tar)):
        if len(st["flatness"]) < N_FLAT:
            raise ValueError(f"{len(st['flatness'])} frames, {N_FLAT} needed")
        bo, bt = (bnd_out[c], bnd_tar[c]) if bnd_out is not None else (None, None)

        def one(key, ft, fo, N=N_RUN, dt=None, do=None):
            mt, mo = stats(ft, N), stats(fo, N)
            per[key].append(mape_fn(mt, mo))
            if dt is not None:
                perb[key].append(mape_bound(mt, mo, running_mean(dt, N), running_mean(do, N)))
        B = lambda d_, name, sl=slice(None): None if d_ is None else d_[name][sl]
        one("centroid_mean", st["centroid"] + 1.0, so["centroid"] + 1.0, dt=B(bt, "centroid"), do=B(bo, "centroid"))
        one("bandwidth_mean", st["bandwidth"] + 1.0, so["bandwidth"] + 1.0, dt=B(bt, "bandwidth"), do=B(bo, "bandwidth"))
        one("rolloff_mean", st["rolloff"] + 1.0, so["rolloff"] + 1.0, dt=B(bt, "rolloff"), do=B(bo, "rolloff"))
        one("flatness_mean", st["flatness"], so["flatness"], N=N_FLAT, dt=B(bt, "flatness"), do=B(bo, "flatness"))
        ct, co = (np.asarray([stats(row, N_RUN) for row in s["contrast"]]) for s in (st, so))
        groups = (("contrast_l_mean", slice(0, 1)), ("contrast_m_mean", slice(1, 4)), ("contrast_h_mean", slice(-1, None)))
        for key, sl in groups:
            mt, mo = np.mean(ct[sl], axis=0), np.mean(co[sl], axis=0)
            per[key].append(mape_fn(mt, mo))
            if bt is not None:
                dt, do = (np.mean([running_mean(row, N_RUN) for row in d_["contrast"][sl]], axis=0) for d_ in (bt, bo))
                perb[key].append(mape_bound(mt, mo, dt, do))
    val = {k: float(np.mean(per[k])) for k in KEYS}
    val["mape_mean"] = float(np.mean([val[k] for k in KEYS]))
    if bnd_out is None:
        return val
    bound = {k: float(np.mean(perb[k])) for k in KEYS}
    bound["mape_mean"] = float(np.mean([bound[k] for k in KEYS]))
    return val, bound


def features_exact(out, tar, sr, n_fft, hop, channels=2):
    """-> (exact, bound) dictionaries of compute_spectral_features and the per-channel (slots, sequences, bounds) of out and tar"""
    no, nt = peak_normalize(out), peak_normalize(tar)
    co, ct = ([channel_exact(x[:, c], sr, n_fft, hop) for c in range(channels)] for x in (no, nt))
    identical = np.array_equal(no, nt)
    val, bound = errors_from_sequences([c[1] for c in co], [c[1] for c in ct], [c[2] for c in co], [c[2] for c in ct])
    if identical:          # the same samples through the same instructions: the same bits, whatever their error
        bound = {k: 0.0 for k in bound}
    return val, bound, co, ct


# ---- rounded: librosa 0.9.2 --------------------------------------------------------------------------------------------------
def spec_rounded(xn, n_fft, hop):
    """compute_stft + transpose + abs of the reference: float32 [C, bins, T], a transposed view's layout"""
    s = np.empty((n_frames(xn.shape[0], n_fft, hop), xn.shape[1], n_fft // 2 + 1), dtype=np.complex64)
    for c in range(xn.shape[1]):
        s[:, c, :] = M.stft(xn[:, c], n_fft, hop).astype(np.complex64)
    return np.abs(np.transpose(s, axes=[1, -1, 0]))


def _normalize(S):
    """librosa.util.normalize(S, norm=1, axis=0)"""
    length = np.sum(np.abs(S).astype(float), axis=0, keepdims=True)
    length[length < np.finfo(S.dtype).tiny] = 1.0
    out = np.empty_like(S)
    out[:] = S / length
    return out


def spectral_centroid(y=None, sr=22050, S=None, n_fft=2048, hop_length=512, **kw):
    freq = fft_frequencies(sr, n_fft).reshape(-1, 1)
    return np.sum(freq * _normalize(S), axis=0, keepdims=True)


def spectral_bandwidth(y=None, sr=22050, S=None, n_fft=2048, hop_length=512, centroid=None, norm=True, p=2, **kw):
    deviation = np.abs(np.subtract.outer(fft_frequencies(sr, n_fft), centroid[0]))
    if norm:
        S = _normalize(S)
    return np.sum(S * deviation ** p, axis=0, keepdims=True) ** (1.0 / p)


def spectral_rolloff(y=None, sr=22050, S=None, n_fft=2048, hop_length=512, roll_percent=0.85, **kw):
    freq = fft_frequencies(sr, n_fft).reshape(-1, 1)
    total_energy = np.cumsum(S, axis=0)
    threshold = roll_percent * total_energy[-1]
    ind = np.where(total_energy < threshold, np.nan, 1)
    return np.nanmin(ind * freq, axis=0, keepdims=True)


def spectral_flatness(y=None, S=None, n_fft=2048, hop_length=512, amin=1e-10, power=2.0, **kw):
    S_thresh = np.maximum(amin, S ** power)
    gmean = np.exp(np.mean(np.log(S_thresh), axis=0, keepdims=True))
    return gmean / np.mean(S_thresh, axis=0, keepdims=True)


def power_to_db(S, amin=1e-10, top_db=80.0):
    log_spec = 10.0 * np.log10(np.maximum(amin, S))
    return np.maximum(log_spec, log_spec.max() - top_db)


def spectral_contrast(y=None, sr=22050, S=None, n_fft=2048, hop_length=512, fmin=200.0, n_bands=6, quantile=0.02, linear=False, **kw):
    freq = fft_frequencies(sr, n_fft)
    octa = np.zeros(n_bands + 2)
    octa[1:] = fmin * (2.0 ** np.arange(0, n_bands + 1))
    valley = np.zeros((n_bands + 1, S.shape[1]))
    peak = np.zeros_like(valley)
    for k, (f_low, f_high) in enumerate(zip(octa[:-1], octa[1:])):
        current_band = np.logical_and(freq >= f_low, freq <= f_high)
        idx = np.flatnonzero(current_band)
        if k > 0:
            current_band[idx[0] - 1] = True
        if k == n_bands:
            current_band[idx[-1] + 1:] = True
        sub_band = S[current_band]
        if k < n_bands:
            sub_band = sub_band[:-1]
        idx = int(np.maximum(np.rint(quantile * np.sum(current_band)), 1))
        sortedr = np.sort(sub_band, axis=0)
        valley[k] = np.mean(sortedr[:idx], axis=0)
        peak[k] = np.mean(sortedr[-idx:], axis=0)
    return peak - valley if linear else power_to_db(peak) - power_to_db(valley)


def rounded_sequences(S, sr, n_fft, hop):
    """S float32 [bins, T] of one channel -> {name: sequence} as the reference calls librosa"""
    sc = spectral_centroid(sr=sr, S=S, n_fft=n_fft, hop_length=hop)
    return {"centroid": sc[0], "bandwidth": spectral_bandwidth(sr=sr, S=S, n_fft=n_fft, hop_length=hop, centroid=sc, norm=True, p=2)[0],
            "rolloff": spectral_rolloff(sr=sr, S=S, n_fft=n_fft, hop_length=hop, roll_percent=0.85)[0],
            "flatness": spectral_flatness(S=S, n_fft=n_fft, hop_length=hop, amin=1e-10, power=2.0)[0],
            "contrast": spectral_contrast(sr=sr, S=S, n_fft=n_fft, hop_length=hop, fmin=250.0, n_bands=4, quantile=0.02, linear=False)}


def features_rounded(out, tar, sr, n_fft, hop, channels=2):
    """-> the dictionary in the reference's formats, and the per-channel sequences of out and tar"""
    so, st = (spec_rounded(peak_normalize(x), n_fft, hop) for x in (out, tar))
    qo, qt = ([rounded_sequences(s[c], sr, n_fft, hop) for c in range(channels)] for s in (so, st))
    val = errors_from_sequences(qo, qt, mape_fn=M._mape32, stats=lambda x, N: M._running_mean_rounded(x, N))
    return val, qo, qt


# ---- the cases ----------------------------------------------------------------------------------------------------------------
CASES = ("noise_pan", "silence_gap", "compressed", "identical", "mono", "real_drums", "real_bass", "noise_4096", "noise_512")
# the cases whose bounds must say something (tests/test_specfeat_reference.py): mixfeat_ref.BROADBAND's recipes.  Its real_drums recipe is
# the densest 43008 samples of the drum stem at 2048 / 1024 - 41 frames, which bound_case_inputs hands out as it stands: the caps are per
# frame and need no 800 frames.  The golden case of the same name is the WHOLE stem (the 800 frames of the flatness mean need it); it has
# the kick-only passages that recipe was cut to avoid, and its figures are printed beside the bass stem's.
BROADBAND = ("noise_pan", "noise_4096", "noise_512", "real_drums")
DRUMS_DENSE = 243 * 1024          # the first sample of that stretch in the stem
_L_REAL = 2048 + 1287 * 512          # 1288 frames of the committed stems
# Bin 0 of a noise frame is a real Gaussian, not a Rayleigh magnitude: over 800 frames it comes within 1e-3 of zero somewhere, and band 0's
# smallest value - one bin, k = 1 - then has a bound of 4 % of itself.  A constant keeps bin 0 (and its window leakage) away from zero.
_DC = 0.05
# noise_4096: the sum of the bin bounds below the roll-off point grows with n_fft: for noise with a flat spectrum the ambiguous window is
# about 2 (0.85 + 0.85) 2049 delta, 9 to 10 % of a bin's magnitude at 4096 points whatever the seed.  mixfeat_ref's recipe, whose top band
# - where the crossing falls - is its quietest, had 10 to 12 % of ambiguous frames; a mix whose top band is the loudest has 9 to 10 %.
# (Darker mixes, with the crossing inside a loud mid band, get 2 %, and lose the flatness cap to their weak top bins instead.)  The seed
# is one whose rarest valley (a k = 1 band's smallest bin over 836 frames) stays inside its cap; so is noise_512's.
_BRIGHT_TAR = (((0, 250), (0.5, 0.4)), ((250, 2500), (0.5, 0.6)), ((2500, 30000), (1.0, 0.9)))
_BRIGHT_OUT = (((0, 250), (0.6, 0.3)), ((250, 2500), (0.4, 0.6)), ((2500, 30000), (0.9, 1.0)))


def case_inputs(name):
    """(out, tar, sr, n_fft, hop), out / tar float32 [L, 2], 800 frames or more each"""
    f32 = lambda v: np.ascontiguousarray(v, dtype=np.float32)
    if name in ("real_drums", "real_bass"):
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "real_audio.npz"))
        kind = name[5:]
        tar = M._stem(z, "reference", kind)[:, :_L_REAL].T.astype(np.float64)
        if kind == "bass":
            out = M._stem(z, "input", kind)[:, :_L_REAL].T
        else:          # mixfeat_ref's drums recipe: a remix of the stem itself
            mixed = tar @ np.array([[1.0, 0.15], [-0.1, 0.8]])
            out = np.sign(mixed) * np.abs(mixed) ** 0.85
        return f32(out), f32(tar), SR, 2048, 512
    if name == "noise_4096":
        L = 860000
        a, b = M._noise(301, (L,)), M._noise(302, (L,))
        side = 0.15 * np.stack([b, -b], 1)
        return f32(M._band_pan(a, _BRIGHT_OUT) + side + _DC), f32(M._band_pan(a, _BRIGHT_TAR) + side + _DC), SR, 4096, 1024
    if name == "noise_512":          # mixfeat_ref's recipe at its own rate, another seed
        L, sr = 512 + 256 * 839, SR // 4
        a, b = M._noise(221, (L,)), M._noise(222, (L,))
        side = 0.15 * np.stack([b, -b], 1)
        return f32(M._band_pan(a, M.PAN, sr) + side + _DC), f32(M._stereo_noise(221, L, sr) + _DC), sr, 512, 256
    o, t, sr, _, _ = M.case_inputs(name, length=860000)
    if name == "noise_pan":
        o, t = f32(o.astype(np.float64) + _DC), f32(t.astype(np.float64) + _DC)
    return o, t, sr, 2048, 1024


def bound_case_inputs(name):
    """the input the caps on the bounds are asserted on: the case itself, but for real_drums mixfeat_ref's own BROADBAND recipe"""
    return M.case_inputs("real_drums") if name == "real_drums" else case_inputs(name)
