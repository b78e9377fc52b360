"""Generate tests/golden/mixfeat.npz: the REAL reference's audio-feature errors on the golden cases of tests/mixfeat_ref.py.

Run ONLY where the reference checkout is present:   python tests/golden/make_golden_mixfeat.py
It imports the reference's own mixing_manipulator/utils_data_normalization.py and calls its compute_loudness_features,
compute_panning_features, compute_dynamic_features, get_SPS, get_panning_rms, get_rms_dynamic_crest and get_low_freq_weighting.  The
third-party packages that are absent offline get the stand-ins make_golden.py uses (librosa.stft(center=False) as an rfft per frame
rounded to complex64, librosa.util.frame, pyloudnorm.normalize.peak with NumPy 1.x's float32 promotion, pyloudnorm.Meter from
oracle/normalizer_ref.py); sklearn is the real one.

Per case the file holds
  <case>/loudness, /panning, /dynamic     the three dictionaries' values, in the key order of mixfeat_ref (LOUDNESS_KEYS, PANNING_KEYS + mape_mean,
                                          DYNAMIC_KEYS)
  <case>/p_rms_out, /p_rms_tar            get_panning_rms(get_SPS(peak-normalised signal)) [frames, 4], before zero-rms frames are deleted
  <case>/rdc_out, /rdc_tar                get_rms_dynamic_crest [3, frames]
  <case>/low_out, /low_tar                get_low_freq_weighting [frames]
  noise_pan/sps_mean, /phi_mean           get_SPS's means over the frames of the target (unsmoothed) [bins]
Inputs are the recipes of mixfeat_ref.case_inputs: nothing but these results is stored.  Printed beside them: the restatement's values,
the reference's own error (rounded - exact) and, for the broadband cases, the largest bound / value of the per-frame sequences."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference/mixing_style_transfer"
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

import mixfeat_ref as R  # noqa: E402

LOUDNESS_KEYS = ("d_lufs", "d_peak")


def load_reference():
    import make_golden
    from oracle import normalizer_ref as N
    make_golden.install_stubs()
    pyln = types.ModuleType("pyloudnorm")

    class Meter:
        def __init__(self, rate):
            self.rate = rate

        def integrated_loudness(self, x):
            return N.integrated_loudness(x, self.rate)
    norm = types.ModuleType("pyloudnorm.normalize")
    norm.peak = lambda data, tgt: data * (np.float32(np.power(10.0, tgt / 20.0) / np.max(np.abs(data))) if data.dtype == np.float32
                                          else np.power(10.0, tgt / 20.0) / np.max(np.abs(data)))
    pyln.Meter, pyln.normalize = Meter, norm
    lib = types.ModuleType("librosa")
    lib.__path__ = []

    def stft(y, n_fft, hop_length, window, center):
        assert center is False
        n = 1 + (len(y) - n_fft) // hop_length
        return np.stack([np.fft.rfft(y[f * hop_length:f * hop_length + n_fft] * window) for f in range(n)], 1).astype(np.complex64)
    lib.stft = stft
    lib.util = types.ModuleType("librosa.util")
    lib.util.frame = lambda x, frame_length, hop_length: np.stack(
        [x[i * hop_length:i * hop_length + frame_length] for i in range(1 + (len(x) - frame_length) // hop_length)], 1)
    empty = types.ModuleType
    sys.modules.update({"pyloudnorm": pyln, "pyloudnorm.normalize": norm, "librosa": lib, "librosa.util": lib.util,
                        "librosa.display": empty("librosa.display"), "aubio": empty("aubio"), "soundfile": empty("soundfile")})
    if "psutil" not in sys.modules:
        try:
            import psutil  # noqa: F401
        except ImportError:
            sys.modules["psutil"] = empty("psutil")
    mm = os.path.join(REF, "mixing_manipulator")
    sys.path.insert(0, mm)
    spec = importlib.util.spec_from_file_location("ref_utils_data_normalization", os.path.join(mm, "utils_data_normalization.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    un = load_reference()
    peak = sys.modules["pyloudnorm"].normalize.peak
    out = {}
    for name in R.CASES:
        o, t, sr, n_fft, hop = R.case_inputs(name)
        args = (o, t, 0, sr, n_fft, hop)
        loud, pan, dyn = un.compute_loudness_features(args), un.compute_panning_features(args), un.compute_dynamic_features(args)
        out[f"{name}/loudness"] = np.asarray([loud[k][0] for k in LOUDNESS_KEYS], dtype=np.float64)
        out[f"{name}/panning"] = np.asarray([pan[k][0] for k in R.PANNING_KEYS + ("mape_mean",)], dtype=np.float64)
        out[f"{name}/dynamic"] = np.asarray([dyn[k][0] for k in R.DYNAMIC_KEYS], dtype=np.float64)
        freqs = [[0, sr // 2], [0, 250], [250, 2500], [2500, sr // 2]]
        for tag, x in (("out", o), ("tar", t)):
            xn = peak(x, -1.0)
            sps_mean, phi_mean, sps, _ = un.get_SPS(xn, n_fft=n_fft, hop_length=hop, smooth=False, frames=True)
            out[f"{name}/p_rms_{tag}"] = np.asarray(un.get_panning_rms(sps, freqs=freqs, sr=sr, n_fft=n_fft))
            out[f"{name}/rdc_{tag}"] = np.concatenate(un.get_rms_dynamic_crest(xn, n_fft, hop), axis=0)
            out[f"{name}/low_{tag}"] = un.get_low_freq_weighting(xn, sr, n_fft, hop, f0=1000)[0]
            if name == "noise_pan" and tag == "tar":
                out[f"{name}/sps_mean"], out[f"{name}/phi_mean"] = np.asarray(sps_mean), np.asarray(phi_mean)
        # the restatement beside it
        le, lb, lr = R.loudness_features(o, t, sr)
        pe, pb, pr, fo, ft = R.panning_features(o, t, sr, n_fft, hop)
        de, db, dr, (do_, lo_), (dt_, lt_) = R.dynamic_features(o, t, sr, n_fft, hop)
        print(f"{name}: T = {out[f'{name}/p_rms_tar'].shape[0]}")
        for title, keys, gold, ex, bd, rd in (("loudness", LOUDNESS_KEYS, loud, le, lb, lr), ("panning", R.PANNING_KEYS + ("mape_mean",), pan, pe, pb, pr),
                                              ("dynamic", R.DYNAMIC_KEYS, dyn, de, db, dr)):
            for k in keys:
                g = float(gold[k][0])
                print(f"    {title:8s} {k:18s} reference {g:.12g}  rounded {rd[k]:.12g}  exact {ex[k]:.12g}  own error {abs(g - ex[k]):.3g}  bound {bd[k]:.3g}")
        if name in R.BROADBAND or name == "real_bass":
            with np.errstate(divide="ignore", invalid="ignore"):
                rp = max(float(np.nanmax(f["dp"] / f["p_rms"])) for f in (fo, ft))
                rl = max(float(np.nanmax(f["d_ratio"] / f["ratio"])) for f in (lo_, lt_))
            print(f"    largest per-frame bound / value: p_rms {rp:.3g}, low ratio {rl:.3g}")
    np.savez_compressed(os.path.join(HERE, "mixfeat.npz"), **out)
    print("mixfeat.npz", os.path.getsize(os.path.join(HERE, "mixfeat.npz")), "bytes")


if __name__ == "__main__":
    main()
