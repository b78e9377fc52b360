"""The spectral-feature kernel and compute_spectral_features on the MI355X: all 16 slots against the float64 restatement within the
derived bounds (tests/specfeat_ref.py), bit identity of a batch of 32, every golden case through the Python function against `exact`
and against the reference's own dictionary (tests/golden/specfeat.npz), device tensors, a second stream, the command line."""
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

from music_mixing_style_transfer_amd import _lib  # noqa: E402
from music_mixing_style_transfer_amd.mixing_manipulator import _device_ops as D  # noqa: E402
from music_mixing_style_transfer_amd.mixing_manipulator import utils_data_normalization as U  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = np.load(os.path.join(HERE, "golden", "specfeat.npz"))
_inputs = {}


def _signal(name, which):
    if name not in _inputs:
        _inputs[name] = R.case_inputs(name)
    return _inputs[name][which], _inputs[name][2]


def _cut(n_fft, hop):
    return 12 * hop + n_fft + 321          # 13 frames and a remainder: T is no multiple of the frames a workgroup owns


# (case, out / tar, n_fft, hop, first sample): every frame length the handle accepts, hop = n_fft and a hop that does not divide it
KERNEL_CASES = [("noise_pan", 1, 2048, 1024, 0), ("mono", 0, 2048, 1024, 0), ("real_drums", 1, 2048, 512, R.DRUMS_DENSE), ("noise_4096", 1, 4096, 1024, 0),
                ("noise_512", 1, 512, 256, 0), ("noise_pan", 0, 1024, 300, 5000), ("noise_pan", 1, 4096, 4096, 0), ("noise_pan", 0, 512, 100, 777)]


def test_the_product_library_is_bound():
    b = _lib.lib()
    assert b.path.endswith("libmst_hip.so") and b.mst_version() >= 106


@pytest.mark.parametrize("name,which,n_fft,hop,start", KERNEL_CASES)
def test_all_slots_within_the_bound(name, which, n_fft, hop, start):
    x, sr = _signal(name, which)
    check_kernel(f"{name}[{which}]", x[start:start + _cut(n_fft, hop)], sr, n_fft, hop, device=DEV)


def test_the_case_list_launches_every_instantiation():
    """one instantiation per n_fft the handle accepts (mst_mixfeat_create: a power of two, 512 .. 4096)"""
    assert {c[2] for c in KERNEL_CASES} == {512, 1024, 2048, 4096}


def test_silent_frames_ties_and_one_channel():
    tar, sr = _signal("silence_gap", 1)
    n_fft, hop = 2048, 1024
    lo = len(tar) // 3 - 4 * hop
    x = tar[lo:lo + 15 * hop + n_fft + 100]
    check_kernel("silence_gap", x, sr, n_fft, hop, device=DEV)
    check_kernel("one channel", x[:, :1], sr, n_fft, hop, device=DEV)
    check_ties(DEV)


def test_a_band_of_one_and_the_whole_spectrum():
    x, sr = _signal("noise_pan", 1)
    for n_fft, hop in ((512, 256), (4096, 2048)):
        m = n_fft // 2
        for bands in ([(0, m + 1, m + 1), (0, m + 1, 1), (m, m + 1, 1), (0, 1, 1), (5, 70, 64)], [(m // 2, m + 1, 3), (1, m, m // 2), (7, 9, 2)], [(3, 4, 1)]):
            check_kernel(f"odd bands {n_fft}", x[:3 * n_fft + 55], sr, n_fft, hop, device=DEV, bands=bands)


def test_a_batch_of_32_is_bit_identical_to_its_items_and_to_itself():
    tar, sr = _signal("noise_pan", 1)
    out, _ = _signal("noise_pan", 0)
    L = 131072
    xs = np.stack([(tar if i % 2 else out)[i * 20000:i * 20000 + L] for i in range(32)])
    a = check_bit_identity(xs, sr, 4096, 1024, device=DEV)
    assert a.shape == (32, 2, 125, 16) and np.all(np.isfinite(a))
    check_bit_identity(xs[:8, :20000], sr, 512, 256, device=DEV)


@pytest.mark.parametrize("name", R.CASES)
def test_function_against_exact_and_the_reference(name):
    out, tar, sr, n_fft, hop = R.case_inputs(name)
    got, worst = check_function(name, out, tar, sr, n_fft, hop, device=DEV, golden=GOLD[f"{name}/spectral"])
    if name == "identical":
        assert all(v[0] == 0.0 for v in got.values())


def test_device_tensors_stay_on_the_device_and_a_second_stream_agrees():
    out, tar, sr, n_fft, hop = R.case_inputs("noise_512")
    o, t = torch.from_numpy(out).to(DEV), torch.from_numpy(tar).to(DEV)
    # a float32 device tensor is taken as it is (no copy, none through the host), and the batch of the two is built on its device
    assert D.to_device(o).data_ptr() == o.data_ptr() and D.to_device(t).data_ptr() == t.data_ptr()
    pair = U._pair(o, t)
    assert pair.device == o.device and pair.shape == (2,) + tuple(o.shape) and torch.equal(pair[0], o) and torch.equal(pair[1], t)
    moved = []
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: (moved.append(tuple(self.shape)), real_cuda(self, *a, **k))[1]
    try:
        base = U.compute_spectral_features((o, t, 0, sr, n_fft, hop, 2))
    finally:
        torch.Tensor.cuda = real_cuda
    assert not any(len(sh) and max(sh) >= 1000 for sh in moved), moved          # nothing of the waveform's size travels host -> device
    host = U.compute_spectral_features((out, tar, 0, sr, n_fft, hop, 2))
    assert {k: v[0] for k, v in host.items()} == {k: v[0] for k, v in base.items()}
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        other = U.compute_spectral_features((o, t, 0, sr, n_fft, hop, 2))
    s.synchronize()
    assert {k: v[0] for k, v in other.items()} == {k: v[0] for k, v in base.items()}
    with pytest.raises(ValueError, match="frames.*800"):
        U.compute_spectral_features((o[:100000], t[:100000], 0, sr, n_fft, hop, 2))


def _evaluate(argv):
    from music_mixing_style_transfer_amd.inference import evaluate
    buf = io.StringIO()
    with redirect_stdout(buf):
        assert evaluate.main(argv) == 0
    return buf.getvalue()


def test_evaluate_takes_spectral_and_leaves_the_other_lines_alone(tmp_path, capsys):
    from music_mixing_style_transfer_amd.inference import evaluate
    n_fft, hop = 2048, 512
    z = np.load(os.path.join(HERE, "golden", "real_audio.npz"))
    n = n_fft + 899 * hop
    a, b = RA.unpack(z["pcm/input/drums"])[100000:100000 + n], RA.unpack(z["pcm/reference/drums"])[150000:150000 + n]
    RA.write_wav(tmp_path / "a.wav", a)
    RA.write_wav(tmp_path / "b.wav", b)
    base = ["--est", str(tmp_path / "a.wav"), "--target", str(tmp_path / "b.wav"), "--segment_length", "131072", "--device", DEV,
            "--feature_fft", str(n_fft), "--feature_hop", str(hop)]
    line = _evaluate(base)
    loss = evaluate.MultiScale_Spectral_Loss_MidSide_DDSP(mode="midside")
    f = evaluate.score_pair(str(tmp_path / "a.wav"), str(tmp_path / "b.wav"), loss, 131072, torch.device(DEV))
    want = {"metric": "multi_scale_spectral_midside", "mean": sum(f["segments"]) / len(f["segments"]), "n_segments": len(f["segments"]),
            "segments": f["segments"], "segment_length": 131072, "sample_rate": 44100}
    assert line == json.dumps(want) + "\n"
    fa, fb = ((v.astype(np.float64) / 32768.0).astype(np.float32) for v in (a, b))
    args = (torch.from_numpy(fa).to(DEV), torch.from_numpy(fb).to(DEV), 0, 44100, n_fft, hop)
    old = {"loudness": U.compute_loudness_features(args), "panning": U.compute_panning_features(args), "dynamic": U.compute_dynamic_features(args)}
    want_old = dict(want, features={m: {k: float(v[0]) for k, v in d.items()} for m, d in old.items()})
    assert _evaluate(base + ["--metrics", "mss,loudness,panning,dynamic"]) == json.dumps(want_old) + "\n"
    exact, bound = R.features_exact(fa, fb, 44100, n_fft, hop)[:2]
    for metrics in ("mss,spectral", "mss,loudness,panning,dynamic,spectral"):
        full = json.loads(_evaluate(base + ["--metrics", metrics]))
        assert {k: v for k, v in full.items() if k != "features"} == want and list(full["features"])[-1] == "spectral"
        sp = full["features"]["spectral"]
        assert list(sp) == list(exact)
        for k in exact:
            assert abs(sp[k] - exact[k]) <= bound[k] + 64 * R.EPS64 * max(1.0, abs(exact[k])), (k, sp[k], exact[k], bound[k])
    RA.write_wav(tmp_path / "a.wav", a[:n_fft + 798 * hop])
    RA.write_wav(tmp_path / "b.wav", b[:n_fft + 798 * hop])
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        evaluate.main(base + ["--metrics", "spectral"])
    assert e.value.code not in (0, None)
    err = capsys.readouterr().err
    assert "799 frames" in err and "800" in err


def test_a_cpu_tensor_has_no_path():
    with pytest.raises(RuntimeError, match="no CPU path"):
        D.MixFeat.get(2048, 1024).spectral(torch.zeros(1, 8192, 2), [(0, 10, 1)])
