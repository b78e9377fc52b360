"""The spectral-feature kernel (csrc/mixfeat_kernels.h, mixfeat_spectral_kernel) on the CPU SIMT emulator: all 16 slots against the
float64 restatement within the derived bounds (tests/specfeat_ref.py), the exact values of silent frames, ties counted once, bit
identity alone and in a batch, the Python function end to end at exactly 800 frames, the command line, every refusal."""
import ctypes as C
import io
import json
import os
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import real_audio as RA  # noqa: E402
import specfeat_ref as R  # noqa: E402
from specfeat_checks import check_bit_identity, check_function, check_kernel, check_ties  # noqa: E402

from music_mixing_style_transfer_amd.mixing_manipulator import _device_ops as D  # noqa: E402
from music_mixing_style_transfer_amd.mixing_manipulator import utils_data_normalization as U  # noqa: E402

_inputs = {}


def _signal(name, which):
    """`out` (0) or `tar` (1) of a case, computed once for the module"""
    if name not in _inputs:
        _inputs[name] = R.case_inputs(name)
    return _inputs[name][which], _inputs[name][2]


def _cut(n_fft, hop):
    return 12 * hop + n_fft + 321          # 13 frames and a remainder: T is no multiple of the frames a workgroup owns


# (case, out / tar, n_fft, hop, first sample): every frame length the handle accepts, hop = n_fft and a hop that does not divide it
KERNEL_CASES = [("noise_pan", 1, 2048, 1024, 0), ("mono", 0, 2048, 1024, 0), ("real_drums", 1, 2048, 512, R.DRUMS_DENSE), ("noise_4096", 1, 4096, 1024, 0),
                ("noise_512", 1, 512, 256, 0), ("noise_pan", 0, 1024, 300, 5000), ("noise_pan", 1, 4096, 4096, 0), ("noise_pan", 0, 512, 100, 777)]


@pytest.mark.parametrize("name,which,n_fft,hop,start", KERNEL_CASES)
def test_all_slots_within_the_bound(emu_default, name, which, n_fft, hop, start):
    x, sr = _signal(name, which)
    check_kernel(f"{name}[{which}]", x[start:start + _cut(n_fft, hop)], sr, n_fft, hop)


def test_silent_frames_ties_and_one_channel(emu_default):
    """the stretch around silence_gap's gap: frames of digital silence (exact values: every value of a band ties at 0) and frames half
    inside the gap; the same signal as C = 1; then non-zero ties, every one counted once"""
    tar, sr = _signal("silence_gap", 1)
    n_fft, hop = 2048, 1024
    lo = len(tar) // 3 - 4 * hop
    x = tar[lo:lo + 15 * hop + n_fft + 100]
    check_kernel("silence_gap", x, sr, n_fft, hop)
    silent = [not np.any(x[t * hop:t * hop + n_fft]) for t in range(R.n_frames(len(x), n_fft, hop))]
    assert sum(silent) >= 3
    check_kernel("one channel", x[:, :1], sr, n_fft, hop)
    check_ties(None)


def test_a_band_of_one_and_the_whole_spectrum(emu_default):
    x, sr = _signal("noise_pan", 1)
    for n_fft, hop in ((512, 256), (4096, 2048)):
        m = n_fft // 2
        for bands in ([(0, m + 1, m + 1), (0, m + 1, 1), (m, m + 1, 1), (0, 1, 1), (5, 70, 64)], [(m // 2, m + 1, 3), (1, m, m // 2), (7, 9, 2)], [(3, 4, 1)]):
            check_kernel(f"odd bands {n_fft}", x[:3 * n_fft + 55], sr, n_fft, hop, bands=bands)


def test_bit_identical_alone_in_a_batch_and_from_run_to_run(emu_default):
    out, sr = _signal("noise_pan", 0)
    tar, _ = _signal("noise_pan", 1)
    n = 9 * 1024 + 2048 + 5
    xs = np.stack([tar[:n], out[:n], _signal("compressed", 0)[0][:n], tar[1000:1000 + n]])
    a = check_bit_identity(xs, sr, 2048, 1024)
    assert a.shape == (4, 2, 10, 16)
    check_bit_identity(xs[:, :4 * 512 + 300], sr, 512, 128)


def test_function_end_to_end_at_exactly_800_frames(emu_default):
    out, sr = _signal("noise_512", 0)
    tar, _ = _signal("noise_512", 1)
    L = 512 + 799 * 16
    assert L == 13296
    got, worst = check_function("noise_512/16", out[:L], tar[:L], sr, 512, 16)
    assert all(np.isfinite(v[0]) for v in got.values())
    same, _ = check_function("identical", tar[:L], tar[:L], sr, 512, 16)
    assert all(v[0] == 0.0 for v in same.values())
    one, _ = check_function("one channel", out[:L], tar[:L], sr, 512, 16, channels=1)
    assert one["centroid_mean"][0] != got["centroid_mean"][0]
    with pytest.raises(ValueError, match="799 frames.*800"):
        U.compute_spectral_features((out[:L - 16], tar[:L - 16], 0, sr, 512, 16, 2))
    with pytest.raises(ValueError, match="channels = 3"):
        U.compute_spectral_features((out[:L], tar[:L], 0, sr, 512, 16, 3))


def _wavs(tmp_path, n):
    z = np.load(os.path.join(HERE, "golden", "real_audio.npz"))
    a, b = RA.unpack(z["pcm/input/drums"])[200000:200000 + n], RA.unpack(z["pcm/reference/drums"])[250000:250000 + n]
    RA.write_wav(tmp_path / "a.wav", a)
    RA.write_wav(tmp_path / "b.wav", b)
    return a, b


def _evaluate(argv):
    from music_mixing_style_transfer_amd.inference import evaluate
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert evaluate.main(argv) == 0
    return buf.getvalue()


def test_evaluate_takes_spectral_and_leaves_the_other_lines_alone(emu_default, tmp_path, capsys):
    from music_mixing_style_transfer_amd.inference import evaluate
    n_fft, hop = 2048, 512
    a, b = _wavs(tmp_path, n_fft + 799 * hop)
    base = ["--est", str(tmp_path / "a.wav"), "--target", str(tmp_path / "b.wav"), "--segment_length", "131072", "--device", "cpu",
            "--feature_fft", str(n_fft), "--feature_hop", str(hop)]
    line = _evaluate(base)
    # the parent's code path, in this process: score_pair with the default metric, and with the three feature functions called directly
    loss = evaluate.MultiScale_Spectral_Loss_MidSide_DDSP(mode="midside")
    f = evaluate.score_pair(str(tmp_path / "a.wav"), str(tmp_path / "b.wav"), loss, 131072, torch.device("cpu"))
    want = {"metric": "multi_scale_spectral_midside", "mean": sum(f["segments"]) / len(f["segments"]), "n_segments": len(f["segments"]),
            "segments": f["segments"], "segment_length": 131072, "sample_rate": 44100}
    assert line == json.dumps(want) + "\n"
    fa, fb = ((v.astype(np.float64) / 32768.0).astype(np.float32) for v in (a, b))
    args = (torch.from_numpy(fa), torch.from_numpy(fb), 0, 44100, n_fft, hop)
    old = {"loudness": U.compute_loudness_features(args), "panning": U.compute_panning_features(args), "dynamic": U.compute_dynamic_features(args)}
    want_old = dict(want, features={m: {k: float(v[0]) for k, v in d.items()} for m, d in old.items()})
    assert _evaluate(base + ["--metrics", "mss,loudness,panning,dynamic"]) == json.dumps(want_old) + "\n"
    exact, bound = R.features_exact(fa, fb, 44100, n_fft, hop)[:2]
    for metrics in ("mss,spectral", "mss,loudness,panning,dynamic,spectral"):
        full = json.loads(_evaluate(base + ["--metrics", metrics]))
        assert list(full)[-1] == "features" and list(full["features"])[-1] == "spectral"
        assert {k: v for k, v in full.items() if k != "features"} == want
        sp = full["features"]["spectral"]
        assert list(sp) == list(exact)
        for k in exact:
            assert abs(sp[k] - exact[k]) <= bound[k] + 64 * R.EPS64 * max(1.0, abs(exact[k])), (k, sp[k], exact[k], bound[k])
        if "loudness" in metrics:
            assert {m: full["features"][m] for m in old} == want_old["features"]
    # one frame short: a non-zero exit that names the frame count and the 800
    RA.write_wav(tmp_path / "a.wav", a[:-hop])
    RA.write_wav(tmp_path / "b.wav", b[:-hop])
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        evaluate.main(base + ["--metrics", "spectral"])
    assert e.value.code not in (0, None)
    err = capsys.readouterr().err
    assert "799 frames" in err and "800" in err


def _handle(emu, n_fft=2048, hop=1024):
    h = C.c_void_p()
    assert emu.mst_mixfeat_create(n_fft, hop, C.byref(h)) == 0
    return h


def test_refusals_name_the_offending_value(emu):
    assert emu.mst_version() >= 106
    h = _handle(emu)
    x = torch.zeros(1, 4096, 2)
    out = torch.zeros(1, 2, 3, 16, dtype=torch.float64)
    ints = lambda *v: (C.c_int * len(v))(*v)
    lo, hi, k = ints(0, 11), ints(11, 1025), ints(1, 20)
    call = lambda **kw: emu.mst_mixfeat_spectral(*[{**dict(h=h, x=x.data_ptr(), n=1, L=4096, C=2, s=None, lo=lo, hi=hi, k=k, nb=2,
                                                           out=out.data_ptr(), st=None), **kw}[a]
                                                   for a in ("h", "x", "n", "L", "C", "s", "lo", "hi", "k", "nb", "out", "st")])
    msg = lambda: (emu.mst_last_error() or b"").decode()
    assert call() == 0
    assert call(C=3) == -2 and "C = 3" in msg()
    assert call(C=0) == -2 and "C = 0" in msg()
    assert call(nb=0) == -2 and "n_bands = 0" in msg()
    assert call(nb=9) == -2 and "n_bands = 9" in msg()
    assert call(nb=6) == -2 and "n_bands = 6" in msg()          # 6 + 2 * 6 numbers would not fit a frame's 16
    assert call(hi=ints(11, 1026)) == -1 and "1026" in msg()
    assert call(lo=ints(-1, 11)) == -1 and "[-1, 11)" in msg()
    assert call(lo=ints(11, 11)) == -1 and "[11, 11)" in msg()          # an empty band
    assert call(k=ints(0, 20)) == -1 and "k = 0" in msg()
    assert call(k=ints(12, 20)) == -1 and "k = 12" in msg() and "1 .. 11" in msg()
    assert call(L=2000) == -2 and "L = 2000" in msg()
    assert call(n=70000) == -2 and "n_items = 70000" in msg()
    assert call(x=None) == -1 and call(out=None) == -1 and call(h=None) == -1 and call(lo=None) == -1 and call(k=None) == -1
    assert emu.mst_mixfeat_destroy(h) == 0


def test_refusals_of_the_python_layer(emu_default):
    with pytest.raises(ValueError, match="float32"):
        D.MixFeat.get(2048, 1024).spectral(torch.zeros(1, 8192, 2, dtype=torch.float64), [(0, 10, 1)])
    with pytest.raises(NotImplementedError, match="C = 3"):
        D.MixFeat.get(2048, 1024).spectral(torch.zeros(1, 8192, 3), [(0, 10, 1)])


def test_no_cpu_path_on_the_product_binding():
    with pytest.raises(RuntimeError, match="no CPU path"):
        D.MixFeat.get(2048, 1024).spectral(torch.zeros(1, 8192, 2), [(0, 10, 1)])


def test_the_case_list_launches_every_instantiation():
    """one instantiation per n_fft the handle accepts (mst_mixfeat_create: a power of two, 512 .. 4096)"""
    assert {c[2] for c in KERNEL_CASES} == {512, 1024, 2048, 4096}
