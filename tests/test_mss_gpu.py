"""The fused multi-scale spectral kernel on the MI355X against the float64 restatement (tests/mss_ref.py), within the derived bound
whose constants are fixed against the reference alone; the module API on cuda; inference/evaluate.py end to end.

Recorded figure (not a gate), test_bf16_transfer_scored_against_the_fp32_transfer: the distance between the bf16-mode and the fp32-mode
transfer of the same stem, beside the distance between the transfer's input and its output - printed by the test, kept in DESIGN.md 5."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import mss_ref as R  # noqa: E402
import real_audio as RA  # noqa: E402

pytestmark = pytest.mark.gpu

from music_mixing_style_transfer_amd.modules import FrontEnd, MultiScale_Spectral_Loss_MidSide_DDSP  # noqa: E402
from mss_checks import _ratio, check_case, check_front_end  # noqa: E402

DEV = "cuda:0"


@pytest.mark.parametrize("name", R.CASES)
def test_golden_cases_at_full_length(name):
    """every golden case at its own length (2 x 2 x 131072, 131000, 2^19-sample stems): every term within the bound"""
    _, got, _ = check_case(name, None, DEV)
    if name == "identical":
        assert np.all(got == 0.0)


@pytest.mark.parametrize("mode", ["midside", "ori"])
def test_batch_of_32_segments(mode):
    """32 x 2 x 131072 (the bench shape): 32 different items, every term of every item within its bound; bit-identical from run to run
    and for an item scored alone"""
    rng = np.random.default_rng(7)
    tgt = rng.uniform(-1.0, 1.0, size=(32, 2, 131072)).astype(np.float32)
    tgt *= (10.0 ** rng.uniform(-3.0, 0.0, size=(32, 1, 1))).astype(np.float32)          # levels over 60 dB
    est = (tgt + np.float32(0.05) * rng.uniform(-1.0, 1.0, size=tgt.shape).astype(np.float32) * np.abs(tgt).max(axis=(1, 2), keepdims=True)).astype(np.float32)
    est[5] = tgt[5]
    est[6, 1] = est[6, 0]
    tgt[6, 1] = tgt[6, 0]
    loss = MultiScale_Spectral_Loss_MidSide_DDSP(mode=mode)
    e, t = torch.from_numpy(est).to(DEV), torch.from_numpy(tgt).to(DEV)
    got = loss.terms(e, t)
    assert torch.equal(got, loss.terms(e, t))
    for i in (0, 5, 17, 31):
        assert torch.equal(loss.terms(e[i:i + 1], t[i:i + 1])[0], got[i]), i
    got = got.cpu().numpy()
    worst = 0.0
    for i in range(0, 32, 4):
        val, bnd = R.terms(est[i:i + 4], tgt[i:i + 4], mode=mode)
        worst = max(worst, _ratio(np.abs(got[i:i + 4] - val), bnd))
    print(f"32 x 2 x 131072 {mode}: max term err / bound = {worst:.4f}")
    assert worst <= 1.0
    assert np.all(got[5] == 0.0)
    if mode == "midside":
        assert np.all(got[6, :, 1] == 0.0)
    tot, tot_bnd = R.total(R.terms(est[:4], tgt[:4], mode=mode)[0]), R.total(R.terms(est[:4], tgt[:4], mode=mode)[1])
    out = loss(e[:4], t[:4])
    assert out.dim() == 0 and out.dtype == torch.float32 and out.device.type == "cuda"
    assert abs(float(out) - tot) <= tot_bnd + 2.0 ** -23 * tot


@pytest.mark.parametrize("name", R.CASES)
def test_front_end_on_cuda(name):
    tgt, kw = R.case_inputs(name)[1:]
    for n_fft, hop, wl in kw["scales"][:2]:
        fe = FrontEnd(channel="stereo", n_fft=n_fft, hop_length=hop, win_length=wl, window=kw["kind"])
        check_front_end(fe(torch.from_numpy(tgt).to(DEV), mode=["mag"]).cpu().numpy(), tgt, n_fft, hop, wl, kw["kind"], f"{name} stereo {n_fft}")
    mono = FrontEnd(channel="mono", n_fft=1024)
    check_front_end(mono(torch.from_numpy(tgt[:, 0].copy()).to(DEV), mode=["mag"]).cpu().numpy(), tgt[:, :1], 1024, None, None, "hann", f"{name} mono 1024")


def test_module_api_on_cuda():
    loss = MultiScale_Spectral_Loss_MidSide_DDSP()
    x = torch.from_numpy(R.case_inputs("noise", 20000)[0]).to(DEV)
    with pytest.raises(NotImplementedError, match="requires grad"):
        loss(x.clone().requires_grad_(True), x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss(x.cpu(), x.cpu())
    with pytest.raises(NotImplementedError, match="L = 1000"):
        loss(x[:, :, :1000], x[:, :, :1000])
    v = loss.terms(x, x * 0.5)
    assert v.dtype == torch.float64 and v.is_cuda and tuple(v.shape) == (2, 4, 2, 2) and bool((v > 0).all())
    # a non-contiguous view and a side stream give the same bits
    wide = torch.zeros(2, 2, 40000, device=DEV)
    wide[:, :, ::2] = x
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        v2 = loss.terms(wide[:, :, ::2], x * 0.5)
    s.synchronize()
    assert torch.equal(v, v2)


def test_evaluate_cli_end_to_end(tmp_path):
    z = np.load(os.path.join(HERE, "golden", "real_audio.npz"))
    n = 300000                                        # two whole segments of 131072 and a remainder that is dropped
    a, b = RA.unpack(z["pcm/input/drums"])[:n], RA.unpack(z["pcm/reference/drums"])[:n]
    RA.write_wav(tmp_path / "a.wav", a)
    RA.write_wav(tmp_path / "b.wav", b)
    RA.write_wav(tmp_path / "short.wav", b[:1000])
    cmd = [sys.executable, "-m", "music_mixing_style_transfer_amd.inference.evaluate"]
    r = subprocess.run(cmd + ["--est", str(tmp_path / "a.wav"), "--target", str(tmp_path / "b.wav"), "--segment_length", "131072", "--json",
                              str(tmp_path / "out.json")], cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out == json.loads(open(tmp_path / "out.json").read()) and out["n_segments"] == 2 and out["segment_length"] == 131072
    fa, fb = (a.astype(np.float64) / 32768.0).astype(np.float32).T, (b.astype(np.float64) / 32768.0).astype(np.float32).T
    for i, got in enumerate(out["segments"]):
        sl = slice(i * 131072, (i + 1) * 131072)
        val, bnd = R.loss(fa[None, :, sl], fb[None, :, sl])
        print(f"evaluate segment {i}: {got:.9g} (float64 {val:.12g}, bound {bnd:.3g})")
        assert abs(got - val) <= bnd
    assert abs(out["mean"] - sum(out["segments"]) / 2) <= 1e-12
    # ori mode, a file shorter than one segment is one segment; files that differ are refused
    r = subprocess.run(cmd + ["--est", str(tmp_path / "a.wav"), "--target", str(tmp_path / "b.wav"), "--mode", "ori", "--segment_length", "1000000"],
                       cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    one = json.loads(r.stdout.strip())
    assert one["n_segments"] == 1 and one["segment_length"] == n
    val, bnd = R.loss(fa[None], fb[None], mode="ori")
    assert abs(one["mean"] - val) <= bnd
    r = subprocess.run(cmd + ["--est", str(tmp_path / "a.wav"), "--target", str(tmp_path / "short.wav")], cwd=REPO, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode != 0 and "differ in rate, channels or length" in r.stderr
    # directories of equally named files
    for d in ("est", "tgt"):
        os.makedirs(tmp_path / d)
    for nm, (pa, pb) in {"drums.wav": (a, b), "bass.wav": (RA.unpack(z["pcm/input/bass"])[:n], RA.unpack(z["pcm/reference/bass"])[:n])}.items():
        RA.write_wav(tmp_path / "est" / nm, pa)
        RA.write_wav(tmp_path / "tgt" / nm, pb)
    r = subprocess.run(cmd + ["--est", str(tmp_path / "est"), "--target", str(tmp_path / "tgt"), "--segment_length", "131072"], cwd=REPO,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    both = json.loads(r.stdout.strip())
    assert both["n_segments"] == 4 and len(both["files"]) == 2 and both["files"][1]["segments"] == out["segments"]


def test_bf16_transfer_scored_against_the_fp32_transfer():
    """what the measure is for: the perceptual cost of a precision mode on a real stem.  A recorded figure, not a gate: the value is
    finite and positive; it is printed beside the distance of the transfer's input to its output."""
    import yaml
    from music_mixing_style_transfer_amd.inference import StyleTransferEngine, build_models
    from music_mixing_style_transfer_amd.utils import synth
    with open(os.path.join(REPO, "music_mixing_style_transfer_amd", "networks", "configs.yaml")) as f:
        cfgs = yaml.full_load(f)
    enc_cfg, tcn_cfg = cfgs["Effects_Encoder"]["default"], cfgs["TCN"]["default"]
    dev = torch.device(DEV)
    enc, tcn = build_models({k: (list(v) if isinstance(v, list) else v) for k, v in enc_cfg.items()}, tcn_cfg, dev, "fp32")
    enc.load_state_dict(synth.fxencoder_state_dict(enc_cfg, seed=0))
    tcn.load_state_dict(synth.tcn_state_dict(seed=0))
    inp, ref = (torch.from_numpy(x).to(dev) for x in R.case_inputs("real_drums", 131072)[:2])
    with torch.no_grad():
        y32 = StyleTransferEngine(enc, tcn).step(ref, inp)[0].detach().clone()
        tcn.precision = "bf16"
        y16 = StyleTransferEngine(enc, tcn).step(ref, inp)[0].detach().clone()
    loss = MultiScale_Spectral_Loss_MidSide_DDSP()
    d_prec, d_io = float(loss(y16, y32)), float(loss(inp, y32))
    print(f"real drums, 131072 samples: distance(bf16 transfer, fp32 transfer) = {d_prec:.6g}; distance(input, fp32 transfer) = {d_io:.6g}; "
          f"ratio {d_prec / d_io:.4g}")
    assert np.isfinite(d_prec) and d_prec > 0.0 and np.isfinite(d_io) and d_io > 0.0
