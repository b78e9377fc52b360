"""Coefficient sets of tests/fx_pass_ref.py -> tests/golden/fx_pass_coefs.npz (rows b0 b1 b2 a0 a1 a2, float64), so that the GPU test needs
numpy alone.  Run from the repository root: python tests/golden/make_golden_fx_pass.py"""
import os
import sys

import numpy as np
import scipy.signal

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from music_mixing_style_transfer_amd.mixing_manipulator import fx_utils                      # noqa: E402
from music_mixing_style_transfer_amd.mixing_manipulator.common_audioeffects import rbj_coefficients  # noqa: E402
from oracle import fx_ref as F                                                                 # noqa: E402

SR = 44100
BANDS = ("low_shelf", "first_band", "second_band", "third_band", "high_shelf")


def config4(gains=None):
    rows = []
    for i, band in enumerate(BANDS):
        g, fc, q = F.CONFIG4["eq"][band]
        g = g if gains is None else gains[i]
        rows.append(rbj_coefficients(band if band.endswith("shelf") else "peaking", g, 0.707 if band.endswith("shelf") else q, fc, SR))
    return np.asarray(rows, dtype=np.float64)


def peaks(n):
    rows = []
    for k, f in enumerate((30, 60, 120, 500, 1000, 4000, 9000, 15000)[:n]):
        b, a = scipy.signal.iirpeak(f, 2.0 + k, fs=SR)
        rows.append([b[0], b[1], b[2], a[0], a[1], a[2]])
    return np.asarray(rows, dtype=np.float64)


def main():
    out = {"config4": config4(), "config4_p12": config4([12.0] * 5), "config4_m12": config4([-12.0] * 5),
           "config4_mixed12": config4([12.0, -12.0, 12.0, -12.0, 12.0]),
           "shelf": np.asarray([rbj_coefficients("low_shelf", 6.0, 0.707, 80.0, SR)], dtype=np.float64)}
    for n in range(1, 9):
        out[f"peaks{n}"] = peaks(n)
    kw = fx_utils.kweighting_coefficients(SR)
    out["kweighting"] = np.asarray([[*b, *a] for b, a in kw], dtype=np.float64)
    out["lowpass1000"] = scipy.signal.butter(4, 1000 / (SR / 2), "lowpass", output="sos").astype(np.float64)
    for n in range(1, 9):          # n sections with no pole near z = 1: the chunk states stay resolved over hundreds of chunks
        out[f"butter{2 * n}"] = scipy.signal.butter(2 * n, 0.25, "lowpass", output="sos").astype(np.float64)
    np.savez(os.path.join(HERE, "fx_pass_coefs.npz"), **out)
    for k, v in out.items():
        print(k, v.shape)


if __name__ == "__main__":
    main()
