"""EQ and compressor matching of the input normaliser (reference mixing_manipulator/utils_data_normalization.py:
get_eq_matching :65-107, get_mean_peak :284-338, compress :340-355, get_comp_matching :357-429), and the audio-feature errors the
reference judges a mix by (compute_loudness_features / compute_spectral_features / compute_panning_features / compute_dynamic_features
:483-905 with their helpers
get_running_stats :41-63, get_SPS :109-139, get_panning_rms :682-703, get_rms_dynamic_crest :777-811, lowpassFiltering :813-820,
get_low_freq_weighting :823-846).

Same function names, arguments and return values as the reference (numpy in, numpy out); the sample-rate work runs on
the MI355X:
  * get_eq_matching: loudness normalisation (BS.1770 meter), the mean STFT magnitude (the library's own FFT kernels), and the
    zero-phase 1001-tap FIR (scipy.signal.filtfilt semantics: odd extension by 3 * ntaps, forward + backward pass from the
    steady state of the first sample) as two FFT convolutions; scipy.signal.firwin2 designs the filter on the host like the
    reference does;
  * get_comp_matching: the reference tries ratio x threshold settings one at a time until the onset-peak statistic drops
    below the target; here a whole row of threshold candidates runs as ONE batch of the time-parallel compressor kernels on
    the same input (mst_fx_compressor_grid), their onset-detection functions and inter-onset peaks are reduced on the device,
    and the first candidate in the reference's scan order that satisfies the condition is returned - the same result as the
    sequential search;
  * the feature errors: the per-frame work - the stereo panning spectrum's band sums, sum x^2 / sum dB / max |x| of every frame, the
    low-passed spectrum over the spectrum - runs in csrc/mixfeat_kernels.h on `out` and `tar` as one batch of two items, with
    pyloudnorm.normalize.peak folded into the kernels' loads; the zero-phase Butterworth low-pass is the float64 biquad cascade run
    forwards and backwards; the short per-frame sequences come back to the host, where the running means over 40 frames, the deletion
    of zero-rms target frames and the errors (sklearn's mean_absolute_percentage_error / mean_squared_error, restated) are float64 numpy;
  * the spectral feature errors: 16 numbers per frame and channel from mixfeat_spectral_kernel (sums, the roll-off bin, the sums of the k
    smallest and largest magnitudes of librosa's contrast bands); librosa.feature's arithmetic (0.9.2, restated: the package is not a
    dependency) turns them into centroid, bandwidth, roll-off, flatness and contrast on the host.
"""
import numpy as np
import scipy.signal

from . import _device_ops as D
from . import fx_utils
from .onset import onset_times


def amp_to_db(x):
    return 20 * np.log10(x + 1e-30)


def db_to_amp(x):
    return 10 ** (x / 20)


# ------------------------------------------------------------------------------------------------ EQ matching
_stft_cache = {}


def _stft(n_fft, hop):
    key = (n_fft, hop)
    if key not in _stft_cache:
        _stft_cache.clear()
        _stft_cache[key] = D.StftMeanMagnitude(n_fft, hop, np.sqrt(np.hanning(n_fft + 1)[:-1]), max_batch=64)
    return _stft_cache[key]


def _filtfilt_fir(taps, x):
    """scipy.signal.filtfilt(taps, 1, x, padtype='odd', padlen=None, method='pad') on the device; x device [L, 1]."""
    import torch
    ntaps = len(taps)
    edge = 3 * ntaps
    L = x.shape[0]
    if L <= edge:
        raise ValueError(f"The length of the input vector x must be greater than padlen, which is {edge}.")
    left = 2 * x[0:1] - torch.flip(x[1:edge + 1], dims=(0,))
    right = 2 * x[L - 1:L] - torch.flip(x[L - edge - 1:L - 1], dims=(0,))
    ext = torch.cat((left, x, right), 0)
    y = D.fir_causal(ext, taps)
    y = D.fir_causal(torch.flip(y, dims=(0,)).contiguous(), taps)
    y = torch.flip(y, dims=(0,))
    return y[edge:edge + L]


def _is_device(x):
    import torch
    return isinstance(x, torch.Tensor)


def get_eq_matching(audio_t, ref_spec, sr=44100, n_fft=65536, hop_length=16384, min_db=-50, ntaps=101, lufs=-30):
    """audio_t: one channel [L]; ref_spec: the target mean magnitude spectrum [n_fft/2+1] -> the EQ-matched channel [L].
    numpy in -> numpy out (the reference's interface); a device tensor in -> a device tensor out (the device-resident normaliser)."""
    on_device = _is_device(audio_t)
    if on_device:
        max_db = amp_to_db(float(audio_t.abs().max()))
        if not max_db > min_db:
            return audio_t
        x = fx_utils.lufs_normalize(D.to_device(audio_t), sr, lufs, log=False)
    else:
        audio_t = np.copy(audio_t)
        max_db = amp_to_db(np.max(np.abs(audio_t)))
        if not max_db > min_db:
            return audio_t
        x = fx_utils.lufs_normalize(D.to_device(audio_t), sr, lufs, log=False)            # device [L, 1], float32
    audio_D_avg = _stft(n_fft, hop_length)(x, 0)
    m = ref_spec.shape[0]
    frq = np.arange(m) / (m / sr) / 2
    diff_eq = np.sqrt(db_to_amp(amp_to_db(ref_spec) - amp_to_db(audio_D_avg)))
    diff_filter = scipy.signal.firwin2(ntaps, frq / np.max(frq), diff_eq, nfreqs=None, window="hamming", antisymmetric=False)
    y = _filtfilt_fir(diff_filter, x)[:, 0]
    return y if on_device else y.cpu().numpy()


# ------------------------------------------------------------------------------------------------ compressor matching
_WIN = 2 ** 10


def _peak_stats(p_value, percentile):
    """mean / std of the onset peaks above the given percentile (all of them when none is above), or None."""
    if not len(p_value):
        return None
    thr = np.percentile(p_value, percentile)
    sel = [p for p in p_value if p > thr]
    use = sel if sel else list(p_value)
    return float(np.mean(use)), float(np.std(use))


def _mean_peak_device(y, sr, percentile):
    """y device [n, L, C] -> list (per item) of [mean peak dB, mean std] over channels, or None like get_mean_peak."""
    n, L, Cn = y.shape
    per_item = [[] for _ in range(n)]
    failed = [False] * n
    for ch in range(Cn):
        od = D.onset_hfc(y, _WIN, ch)                                     # [n, frames, 2]
        onsets = [onset_times(od[i, :, 0], od[i, :, 1], _WIN, sr) for i in range(n)]
        items, lo, hi = [], [], []
        for i, on in enumerate(onsets):
            for k, t in enumerate(on):
                items.append(i)
                lo.append(t)
                hi.append(on[k + 1] if k + 1 < len(on) else L)
        peaks = D.range_reduce(y, items, lo, hi, channel=ch, mode="max") if items else np.zeros(0)
        pos = 0
        for i, on in enumerate(onsets):
            st = _peak_stats(amp_to_db(peaks[pos:pos + len(on)]), percentile)
            pos += len(on)
            if st is None:
                failed[i] = True
            else:
                per_item[i].append(st)
    return [None if failed[i] else [float(np.mean([s[0] for s in per_item[i]])), float(np.mean([s[1] for s in per_item[i]]))]
            for i in range(n)]


def get_mean_peak(audio, sr=44100, true_peak=False, n_mels=128, percentile=75):
    """Mean onset-peak level in dB (peaks above the given percentile) and its spread; audio [samples, channels]."""
    if true_peak:
        raise NotImplementedError("true_peak=True (4x resampled peaks) is not used by the normaliser and not provided")
    return _mean_peak_device(D.to_device(np.asarray(audio))[None], sr, percentile)[0]


def compress(processor, audio, sr, th, ratio, attack, release):
    processor.parameters.threshold.value = th
    processor.parameters.ratio.value = ratio
    processor.parameters.attack_time.value = attack
    processor.parameters.release_time.value = release
    processor.update()
    output = processor.process(audio)
    if np.max(np.abs(output)) >= 1.0:
        output = np.clip(output, -1.0, 1.0)
    return output


def get_comp_matching(audio, ref_peak, ref_std, ratio, attack, release, sr=44100, min_db=-50, comp_peak_norm=-10.0, min_th=-40,
                      max_ratio=20, n_mels=128, true_peak=False, percentile=75, expander=True, batch=16):
    on_device = _is_device(audio)
    out = (lambda t: t) if on_device else (lambda t: t.cpu().numpy())
    if on_device:                                   # device in -> device out: the same steps, the same float32 arithmetic
        x = D.to_device(audio)
        mx = float(x.abs().max())
        if not amp_to_db(mx) > min_db:
            return x
        x = x * np.float32(np.power(10.0, comp_peak_norm / 20.0) / np.float32(mx))
        xd = x
    else:
        x = audio.copy()
        if x.ndim < 2:
            x = np.expand_dims(x, 1)
        max_db = amp_to_db(np.max(np.abs(x)))
        if not max_db > min_db:
            return x
        gain = np.power(10.0, comp_peak_norm / 20.0) / np.max(np.abs(x))              # pyloudnorm.normalize.peak
        x = x * (np.float32(gain) if x.dtype == np.float32 else gain)                 # a float32 signal stays float32 (NumPy 1.x promotion)
        xd = D.to_device(x)
    peak, std = _mean_peak_device(xd[None], sr, percentile)[0]
    if (ref_peak - ref_std) < peak < (ref_peak + ref_std):
        return x
    down = peak > (ref_peak - ref_std)
    if not down and not (expander and peak < (ref_peak + ref_std)):
        return x
    ratios = np.linspace(ratio, max_ratio, max_ratio - ratio + 1)
    if down:
        ths = np.linspace(-1 - 9, min_th, 2 * np.abs(min_th) - 1 - 18)
    else:
        ths = np.linspace(-1, min_th, 2 * np.abs(min_th) - 1)[::-1]
    # the reference's scan order: ratios outer, thresholds inner, stop at the first setting that meets the target.  Here a
    # chunk of `batch` consecutive settings of that order is evaluated at once; the answer is the first that qualifies.
    last = xd
    for rt in ratios:
        for k0 in range(0, len(ths), batch):
            th_chunk = ths[k0:k0 + batch]
            y = D.compressor_grid(xd, list(th_chunk), [rt if down else 1.0 / rt] * len(th_chunk), attack, release, sr, clip=True)
            stats = _mean_peak_device(y, sr, percentile)
            for i, st in enumerate(stats):
                if st is None:                      # the reference would fail on `peak, std = None` here (caught by the caller)
                    raise TypeError("cannot unpack non-iterable NoneType object")
                if (down and st[0] < (ref_peak + ref_std)) or (not down and st[0] > (ref_peak - ref_std)):
                    return out(y[i])
            last = y[len(th_chunk) - 1]
    return out(last)                                # no setting qualified: the reference returns the last one it tried


# ------------------------------------------------------------------------------------------------ audio-feature errors
def running_mean_std(x, N):
    """mean and standard deviation of every window of N consecutive values of x, from cumulative sums (float64)"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        c1 = np.concatenate(([0.0], np.cumsum(x)))
        c2 = np.concatenate(([0.0], np.cumsum(x * x)))
        mean = (c1[N:] - c1[:-N]) / float(N)
        std = np.sqrt((c2[N:] - c2[:-N]) / N - mean * mean)
    return mean, std


def get_running_stats(x, features, N=20):
    """x [frames, n_features] -> (mean, std), each [len(features), frames - N + 1]"""
    stats = [running_mean_std(x[:, i], N) for i in range(len(features))]
    return np.asarray([m for m, _ in stats]), np.asarray([s for _, s in stats])


def _mape(y_true, y_pred):
    """sklearn.metrics.mean_absolute_percentage_error"""
    t, o = np.asarray(y_true, dtype=np.float64), np.asarray(y_pred, dtype=np.float64)
    return float(np.mean(np.abs(t - o) / np.maximum(np.abs(t), np.finfo(np.float64).eps)))


def _mse(y_true, y_pred):
    """sklearn.metrics.mean_squared_error"""
    t, o = np.asarray(y_true, dtype=np.float64), np.asarray(y_pred, dtype=np.float64)
    return float(np.mean((t - o) ** 2))


def _peak_gain(xb, target_db=-1.0):
    """pyloudnorm.normalize.peak's factor of every item of a device batch [n, L, C], as the float32 a float32 signal is multiplied by"""
    with np.errstate(divide="ignore"):
        return (np.power(10.0, target_db / 20.0) / D.peaks(xb)).astype(np.float32)


def _pair(audio_out, audio_tar):
    """the two signals [L, C] as one device batch [2, L, C] (item 0 = out, 1 = tar)"""
    import torch
    o, t = D.to_device(audio_out), D.to_device(audio_tar)
    if o.shape != t.shape:
        raise ValueError(f"the two signals must have one shape, got {tuple(o.shape)} and {tuple(t.shape)}")
    return torch.stack((o, t)).contiguous()


def _band_bins(freqs, sr, n_fft):
    return [(int(np.floor(f[0] * n_fft / sr)), int(np.floor(f[1] * n_fft / sr))) for f in freqs]


def get_SPS(x, n_fft=2048, hop_length=1024, smooth=False, frames=False):
    """Stereo panning spectrum of x [L, 2]: (SPS_mean, phi_mean, SPS, phi), the last two [frames, n_fft / 2 + 1] float32 (they stay on the
    device when x is a device tensor), the means over the frames float64 numpy (Savitzky-Golay smoothed over 501 bins when smooth)."""
    phi, sps = D.MixFeat.get(n_fft, hop_length).sps(D.to_device(x))
    phi, sps = phi[0], sps[0]
    phi_mean, sps_mean = phi.double().mean(dim=0).cpu().numpy(), sps.double().mean(dim=0).cpu().numpy()
    if smooth:
        phi_mean = scipy.signal.savgol_filter(phi_mean, 501, 1, mode="mirror")
        sps_mean = scipy.signal.savgol_filter(sps_mean, 501, 1, mode="mirror")
    if not _is_device(x):
        phi, sps = phi.cpu().numpy(), sps.cpu().numpy()
    return sps_mean, phi_mean, sps, phi


def get_panning_rms_frame(sps_frame, freqs=[0, 22050], sr=44100, n_fft=2048):
    (f1, f2), = _band_bins([freqs], sr, n_fft)
    return np.sqrt((1 / (f2 - f1)) * np.sum(np.asarray(sps_frame[f1:f2], dtype=np.float64) ** 2))


def get_panning_rms(sps, freqs=[[0, 22050]], sr=44100, n_fft=2048):
    """sps [frames, bins] (numpy or device) -> [frames, len(freqs)]: the rms of SPS over each band"""
    sps = np.asarray(sps.cpu() if _is_device(sps) else sps, dtype=np.float64)
    return np.stack([np.sqrt((1 / (f2 - f1)) * np.sum(sps[:, f1:f2] ** 2, axis=1)) for f1, f2 in _band_bins(freqs, sr, n_fft)], axis=1)


def _panning_rms_batch(xb, gain, freqs, sr, n_fft, hop_length):
    """xb device [n, L, 2] -> [n, frames, len(freqs)]: get_panning_rms(get_SPS(x * gain)) in one fused kernel (no spectrum leaves the chip)"""
    bands = _band_bins(freqs, sr, n_fft)
    sums = D.MixFeat.get(n_fft, hop_length).panning(xb, bands, gain)
    return np.sqrt(sums / np.asarray([f2 - f1 for f1, f2 in bands], dtype=np.float64))


def compute_panning_features(args_):
    audio_out_, audio_tar_, idx, sr, fft_size, hop_length = args_[:6]
    xb = _pair(audio_out_, audio_tar_)
    freqs = [[0, sr // 2], [0, 250], [250, 2500], [2500, sr // 2]]
    p_rms_out, p_rms_tar = _panning_rms_batch(xb, _peak_gain(xb), freqs, sr, fft_size, hop_length)
    if np.min(p_rms_tar) == 0.0:                      # frames with zero rms leave the target (and the same frames the output)
        keep = p_rms_tar[:, 0] != 0
        p_rms_tar, p_rms_out = p_rms_tar[keep], p_rms_out[keep]
    mean_tar, _ = get_running_stats(p_rms_tar, freqs, N=40)
    mean_out, _ = get_running_stats(p_rms_out, freqs, N=40)
    panning_ = {key: [_mape(mean_tar[i], mean_out[i])] for i, key in enumerate(["P_t_mean", "P_l_mean", "P_m_mean", "P_h_mean"])}
    panning_["mape_mean"] = [np.mean([panning_[k] for k in ("P_t_mean", "P_l_mean", "P_m_mean", "P_h_mean")])]
    return panning_


def _dynamics_from_sums(sums, frame_length):
    """[C, T, 3] (sum x^2, sum dB, max |x|) -> rms, dynamic spread, crest factor, each [1, T]: the means over the channels"""
    x_rms = amp_to_db(np.sqrt(sums[..., 0] / frame_length))
    x_d = (sums[..., 1] - frame_length * x_rms) / frame_length
    with np.errstate(divide="ignore", invalid="ignore"):
        x_c = amp_to_db(sums[..., 2]) / x_rms                      # the reference's crest factor: a ratio of two dB values
    return tuple(np.expand_dims(np.mean(v, axis=0), 0) for v in (x_rms, x_d, x_c))


def get_rms_dynamic_crest(x, frame_length, hop_length):
    return _dynamics_from_sums(D.frame_dynamics(D.to_device(x), frame_length, hop_length)[0], frame_length)


def _lowpass_batch(xb, f0, sr):
    """scipy.signal.filtfilt(*butter(4, f0 / (sr / 2)), x) along L of a device batch [n, L, C]: odd extension by 15 samples, then the
    float64 biquad cascade forwards and, on the flipped signal, backwards.  scipy starts each pass in the steady state of the pass's first
    sample (lfilter_zi); here the pass is started from rest on a run-in of that sample repeated until the transient is below float64
    resolution - the same state without forming x - x0 in float32."""
    import torch
    sos = scipy.signal.butter(4, f0 / (sr / 2), "lowpass", output="sos")
    edge = 15                                                   # 3 * max(len(a), len(b))
    n, L, Cn = xb.shape
    if L <= edge:
        raise ValueError(f"The length of the input vector x must be greater than padlen, which is {edge}.")
    radius = max(np.abs(np.roots(sec[3:])).max() for sec in sos)
    run = int(np.ceil(np.log(1e-20) / np.log(radius)))

    def one_pass(sig):
        lead = sig[:, :1].expand(-1, run, -1)
        return D.biquad_cascade(torch.cat((lead, sig), 1).contiguous(), sos)[:, run:]

    left = 2 * xb[:, :1] - torch.flip(xb[:, 1:edge + 1], dims=(1,))
    right = 2 * xb[:, L - 1:L] - torch.flip(xb[:, L - edge - 1:L - 1], dims=(1,))
    y = one_pass(torch.cat((left, xb, right), 1))
    y = torch.flip(one_pass(torch.flip(y, dims=(1,))), dims=(1,))
    return y[:, edge:edge + L].contiguous()


def lowpassFiltering(x, f0, sr):
    y = _lowpass_batch(D.to_device(x)[None], f0, sr)[0]
    return y if _is_device(x) else y.cpu().numpy()


def get_low_freq_weighting(x, sr, n_fft, hop_length, f0=1000):
    """[1, frames]: per frame the sum over the bins of |STFT(lowpass(x))| / (|STFT(x)| + 1e-5), averaged over the channels"""
    xb = D.to_device(x)[None]
    ratio = D.MixFeat.get(n_fft, hop_length).low_ratio(_lowpass_batch(xb, f0, sr), xb)[0]
    return np.expand_dims(np.mean(ratio, axis=0), axis=0)


def compute_dynamic_features(args_):
    import torch
    audio_out_, audio_tar_, idx, sr, fft_size, hop_length = args_[:6]
    xb = _pair(audio_out_, audio_tar_)
    gain = _peak_gain(xb)
    sums = D.frame_dynamics(xb, fft_size, hop_length, gain)                      # [2, C, T, 3]
    xn = xb * torch.from_numpy(gain).to(xb.device)[:, None, None]                # the low-pass filters the normalised signal
    ratio = D.MixFeat.get(fft_size, hop_length).low_ratio(_lowpass_batch(xn, 1000, sr), xn).mean(axis=1)          # [2, T]
    N = 40
    (rms_out, dyn_out, crest_out), (rms_tar, dyn_tar, crest_tar) = (_dynamics_from_sums(sums[i], fft_size) for i in range(2))
    stat = lambda v: get_running_stats(v.T, [0], N=N)[0]
    dynamic_ = {"rms_mean": [_mape(stat(1.0 - rms_tar), stat(1.0 - rms_out))],
                "dyn_mean": [_mape(stat(1.0 - dyn_tar), stat(1.0 - dyn_out))],
                "crest_mean": [_mape(stat(crest_tar), stat(crest_out))]}
    low_tar, low_out = stat(ratio[1][None]), stat(ratio[0][None])
    dynamic_["l_ratio_mean_mape"] = [_mape(low_tar, low_out)]
    dynamic_["l_ratio_mean_l2"] = [_mse(low_tar, low_out)]
    dynamic_["mape_mean"] = [np.mean([dynamic_["rms_mean"], dynamic_["dyn_mean"], dynamic_["crest_mean"]])]
    return dynamic_


def compute_loudness_features(args_):
    audio_out_, audio_tar_, idx, sr = args_[:4]
    o, t = D.to_device(audio_out_), D.to_device(audio_tar_)
    with np.errstate(divide="ignore"):
        peak_out_db, peak_tar_db = (20.0 * np.log10(D.peaks(v[None])[0]) for v in (o, t))
    meter = fx_utils.Meter(sr)
    loudness_tar, loudness_out = meter.integrated_loudness(t), meter.integrated_loudness(o)
    return {"d_lufs": [_mape([loudness_tar], [loudness_out])], "d_peak": [_mape([peak_tar_db], [peak_out_db])]}


# ------------------------------------------------------------------------------------------------ spectral feature errors
SPECTRAL_KEYS = ("centroid_mean", "bandwidth_mean", "contrast_l_mean", "contrast_m_mean", "contrast_h_mean", "rolloff_mean", "flatness_mean")
_N_FLATNESS = 800


class TooFewFrames(ValueError):
    """fewer frames than the running mean of the flatness spans: the reference's own call fails there (sklearn on an empty array)"""


def contrast_bands(sr, n_fft, fmin=250.0, n_bands=4, quantile=0.02):
    """The bands of librosa.feature.spectral_contrast (0.9.2) as [(lo, hi, k)] in bins: band j takes the bins with octa[j] <= f_k <=
    octa[j + 1], octa = [0, fmin, 2 fmin, ..]; every band but the first also the bin below; the last every bin above, up to n_fft / 2.
    k = max(1, rint(quantile * that count)); every band but the last then loses its LAST bin from the values, so [lo, hi) are the bins
    the order statistics are taken over."""
    m = n_fft // 2
    freq = np.linspace(0, float(sr) / 2, 1 + m, endpoint=True)
    octa = np.zeros(n_bands + 2)
    octa[1:] = fmin * (2.0 ** np.arange(0, n_bands + 1))
    if np.any(octa[:-1] >= 0.5 * sr):
        raise ValueError(f"contrast_bands: the band edges {octa[:-1]} must stay below the Nyquist frequency {0.5 * sr}")
    bands = []
    for j, (f_low, f_high) in enumerate(zip(octa[:-1], octa[1:])):
        idx = np.flatnonzero(np.logical_and(freq >= f_low, freq <= f_high))
        if not len(idx):
            raise ValueError(f"contrast_bands: no bin between {f_low} and {f_high} Hz at sr = {sr}, n_fft = {n_fft}")
        lo, hi = int(idx[0]), int(idx[-1]) + 1
        if j > 0:
            lo -= 1
        if j == n_bands:
            hi = m + 1
        k = int(max(np.rint(quantile * (hi - lo)), 1))
        if j < n_bands:
            hi -= 1
        if k > hi - lo:
            raise ValueError(f"contrast_bands: band {j} keeps {hi - lo} bin(s) at sr = {sr}, n_fft = {n_fft}, fewer than the {k} it averages")
        bands.append((lo, hi, k))
    return bands


def _power_to_db(x):
    """librosa.power_to_db(x, ref=1.0, amin=1e-10, top_db=80.0) over the whole array"""
    db = 10.0 * np.log10(np.maximum(1e-10, x))
    return np.maximum(db, db.max() - 80.0)


def spectral_sequences(sums, bands, sr, n_fft):
    """The kernel's per-frame numbers of ONE channel, [T, 16] (_device_ops.MixFeat.spectral), -> the five librosa.feature sequences:
    centroid, bandwidth, rolloff, flatness [T] and contrast [len(bands), T]"""
    sums = np.asarray(sums, dtype=np.float64)
    m = n_fft // 2
    step = float(sr) / 2 / m
    s0, s1, s2, ro, slog, sp = (sums[:, i] for i in range(6))
    small = s0 < np.finfo(np.float32).tiny                      # librosa.util.normalize: such a column is divided by 1
    div = np.where(small, 1.0, s0)
    centroid = step * s1 / div
    with np.errstate(divide="ignore", invalid="ignore"):
        cb = np.where(s0 > 0, s1 / s0, 0.0)
    second = np.where(small, s2 + s0 * (cb - s1) ** 2, s2)      # about the centroid in use: the parallel-axis term where it is not [1] / [0]
    bandwidth = step * np.sqrt(second / div)
    flatness = np.exp(slog / (m + 1)) / (sp / (m + 1))
    k = np.asarray([b[2] for b in bands], dtype=np.float64)[:, None]
    valley, peak = sums[:, 6:6 + 2 * len(bands):2].T / k, sums[:, 7:7 + 2 * len(bands):2].T / k
    return centroid, bandwidth, step * ro, flatness, _power_to_db(peak) - _power_to_db(valley)


def _running_mean(x, N=40):
    """the mean of every window of N consecutive values of x (running_mean_std without the std the reference drops here)"""
    c = np.concatenate(([0.0], np.cumsum(np.asarray(x, dtype=np.float64))))
    return (c[N:] - c[:-N]) / float(N)


def spectral_errors(seq_out, seq_tar):
    """The host half of compute_spectral_features: per channel the five sequences of spectral_sequences, of `out` and of `tar`, -> the
    reference's dictionary.  eps = 1 on centroid, bandwidth and roll-off, running means over 40 frames (flatness: 800), MAPE, the mean
    over the channels."""
    per = {k: [] for k in SPECTRAL_KEYS}
    for so, st in zip(seq_out, seq_tar):
        T = len(st[0])
        if T < _N_FLATNESS:
            raise TooFewFrames(f"compute_spectral_features: {T} frames, the running mean of the flatness needs {_N_FLATNESS}")
        run = _running_mean
        for key, i in (("centroid_mean", 0), ("bandwidth_mean", 1), ("rolloff_mean", 2)):
            per[key].append(_mape(run(st[i] + 1.0), run(so[i] + 1.0)))
        ct_t, ct_o = (np.asarray([run(row) for row in s[4]]) for s in (st, so))
        per["contrast_l_mean"].append(_mape(ct_t[0], ct_o[0]))
        per["contrast_m_mean"].append(_mape(np.mean(ct_t[1:4], axis=0), np.mean(ct_o[1:4], axis=0)))
        per["contrast_h_mean"].append(_mape(ct_t[-1], ct_o[-1]))
        per["flatness_mean"].append(_mape(run(st[3], _N_FLATNESS), run(so[3], _N_FLATNESS)))
    spectral_ = {k: [np.mean(per[k])] for k in SPECTRAL_KEYS}
    spectral_["mape_mean"] = [np.mean([np.mean(per[k]) for k in SPECTRAL_KEYS])]
    return spectral_


def compute_spectral_features(args_):
    audio_out_, audio_tar_, idx, sr, fft_size, hop_length, channels = args_[:7]
    both = _pair(audio_out_, audio_tar_)
    if not 1 <= channels <= min(both.shape[2], 2):
        raise ValueError(f"compute_spectral_features: channels = {channels} of signals with {both.shape[2]} (1 or 2, at most the signals' own)")
    xb = both[:, :, :channels].contiguous()
    mf = D.MixFeat.get(fft_size, hop_length)
    T = mf.frames(xb.shape[1])
    if T < _N_FLATNESS:
        raise TooFewFrames(f"compute_spectral_features: {T} frames, the running mean of the flatness needs {_N_FLATNESS}")
    bands = contrast_bands(sr, fft_size)
    gain = _peak_gain(both)                                     # pyloudnorm.normalize.peak: the peak over ALL channels of the signal
    sums = mf.spectral(xb, bands, gain)                         # [2, channels, T, 16]
    seq = [[spectral_sequences(sums[i, c], bands, sr, fft_size) for c in range(channels)] for i in range(2)]
    return spectral_errors(seq[0], seq[1])
