"""Generate tests/golden/specfeat.npz: the reference's OWN compute_spectral_features on the cases of tests/specfeat_ref.py.

Run ONLY where the reference checkout is present:   python tests/golden/make_golden_specfeat.py
It imports the reference's mixing_manipulator/utils_data_normalization.py with the stand-ins make_golden_mixfeat.py installs (librosa.stft
as an rfft per frame rounded to complex64, pyloudnorm.normalize.peak, ...) and, because librosa itself is absent offline, with
librosa.feature.spectral_centroid / _bandwidth / _contrast / _rolloff / _flatness stand-ins that ARE the `rounded` restatement of
tests/specfeat_ref.py (the librosa 0.9.2 arithmetic, restated from its source).  sklearn is the real one.

So this file pins the reference's GLUE - the peak normalisation, compute_stft's layout, which arguments reach librosa, eps = 1, the
running means over 40 and 800 frames, which contrast band goes to which key, the means over channels and over the seven - and NOT
librosa: the definitions are pinned by the closed-form anchors of tests/test_specfeat_reference.py.

Per case the file holds
  <case>/spectral          the dictionary's values in the key order of specfeat_ref.KEYS + mape_mean
  <case>/seq_out, /seq_tar  what the reference's function got back for channel 0, every 4th frame: rows centroid, bandwidth, roll-off,
                            flatness, contrast bands 0 .. 4
Inputs are the recipes of specfeat_ref.case_inputs: nothing but these results is stored."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, HERE)

import make_golden_mixfeat  # noqa: E402
import specfeat_ref as R  # noqa: E402

STRIDE = 4


def main():
    un = make_golden_mixfeat.load_reference()
    calls = []

    def recording(name, fn):
        def wrapped(*a, **kw):
            r = fn(*a, **kw)
            calls.append((name, np.array(r)))
            return r
        return wrapped
    feature = types.ModuleType("librosa.feature")
    for name in ("spectral_centroid", "spectral_bandwidth", "spectral_contrast", "spectral_rolloff", "spectral_flatness"):
        setattr(feature, name, recording(name, getattr(R, name)))
    sys.modules["librosa"].feature = feature
    sys.modules["librosa.feature"] = feature
    out = {}
    for case in R.CASES:
        o, t, sr, n_fft, hop = R.case_inputs(case)
        del calls[:]
        d = un.compute_spectral_features((o, t, 0, sr, n_fft, hop, 2))
        assert list(d) == list(R.KEYS[:6]) + ["flatness_mean", "mape_mean"] and list(d)[:7] == list(R.KEYS)
        out[f"{case}/spectral"] = np.asarray([d[k][0] for k in list(R.KEYS) + ["mape_mean"]], dtype=np.float64)
        # channel 0's ten calls: tar then out of centroid, bandwidth, contrast, roll-off, flatness
        names = [c[0] for c in calls[:10]]
        assert names == [n for n in ("spectral_centroid", "spectral_bandwidth", "spectral_contrast", "spectral_rolloff", "spectral_flatness")
                         for _ in range(2)], names
        for tag, k in (("tar", 0), ("out", 1)):
            sc, bw, ct, ro, ft = (calls[2 * i + k][1] for i in range(5))
            out[f"{case}/seq_{tag}"] = np.concatenate([sc, bw, ro, ft.astype(np.float64), ct], axis=0)[:, ::STRIDE]
        vr = R.features_rounded(o, t, sr, n_fft, hop)[0]
        ve, be = R.features_exact(o, t, sr, n_fft, hop)[:2]
        print(f"{case}: T = {R.n_frames(len(o), n_fft, hop)}")
        for i, k in enumerate(list(R.KEYS) + ["mape_mean"]):
            g = out[f"{case}/spectral"][i]
            print(f"    {k:16s} reference {g:.12g}  rounded {vr[k]:.12g}  exact {ve[k]:.12g}  own error {abs(g - ve[k]):.3g}  bound {be[k]:.3g}")
    path = os.path.join(HERE, "specfeat.npz")
    np.savez_compressed(path, **out)
    print("specfeat.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
