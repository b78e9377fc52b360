"""The fused multi-scale spectral kernel (csrc/mss_kernels.h) on the CPU SIMT emulator: every golden case of tests/mss_ref.py at lengths
the emulator finishes, against the float64 restatement, within the derived bound (tests/mss_ref.py: C_FFT fixed against the reference
alone); determinism; the module API; every refusal."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import mss_ref as R  # noqa: E402
from mss_checks import check_case, check_front_end  # noqa: E402

from music_mixing_style_transfer_amd import _lib  # noqa: E402
from music_mixing_style_transfer_amd.modules import BackEnd, FrontEnd, MultiScale_Spectral_Loss_MidSide_DDSP  # noqa: E402

L_EMU = 12288          # a multiple of every n_fft / 4: the last frame is dropped


@pytest.mark.parametrize("name", R.CASES)
def test_golden_cases_within_the_bound(emu_default, name):
    length = {"noise_odd": 9001, "real_drums": 16384, "real_bass": 16384}.get(name, L_EMU)
    _, got, val = check_case(name, length)
    if name == "identical":
        assert np.all(got == 0.0)
    if name == "mono":
        assert np.all(got[:, :, 1, :] == 0.0) and np.all(val[:, :, 1, :] == 0.0)          # side of a mono signal: exactly nothing


@pytest.mark.parametrize("channel", ["mono", "stereo"])
@pytest.mark.parametrize("n_fft,hop,wl,kind", [(4096, None, None, "hann"), (2048, 512, 1200, "hamming"), (1024, 100, None, "hann"),
                                               (512, None, 400, "hann"), (256, 256, None, "hamming")])
def test_front_end_elementwise(emu_default, channel, n_fft, hop, wl, kind):
    x = R.case_inputs("noise", 7000 if hop == 100 else 8192)[0]
    x[1] *= np.float32(0.01)
    fe = FrontEnd(channel=channel, n_fft=n_fft, hop_length=hop, win_length=wl, window=kind)
    if channel == "mono":
        check_front_end(fe(torch.from_numpy(x[:, 0].copy()), mode=["mag"]).numpy(), x[:, :1], n_fft, hop, wl, kind, f"mono {n_fft} {hop} {wl} {kind}")
    else:
        check_front_end(fe(torch.from_numpy(x), mode=["mag"]).numpy(), x, n_fft, hop, wl, kind, f"stereo {n_fft} {hop} {wl} {kind}")


@pytest.mark.parametrize("name", R.CASES)
def test_front_end_elementwise_on_the_cases(emu_default, name):
    tgt, kw = R.case_inputs(name, 16384)[1:]
    n_fft, hop, wl = kw["scales"][0]
    got = FrontEnd(channel="stereo", n_fft=n_fft, hop_length=hop, win_length=wl, window=kw["kind"])(torch.from_numpy(tgt), mode=["mag"]).numpy()
    check_front_end(got, tgt, n_fft, hop, wl, kw["kind"], name)


def test_bit_identical_alone_in_a_batch_and_from_run_to_run(emu_default):
    est, tgt, kw = R.case_inputs("noise", 9001)
    est = np.concatenate([est, R.case_inputs("sine", 9001)[0], est[::-1]])
    tgt = np.concatenate([tgt, R.case_inputs("sine", 9001)[1], tgt])
    for mode in ("midside", "ori"):
        loss = MultiScale_Spectral_Loss_MidSide_DDSP(mode=mode)
        e, t = torch.from_numpy(est.copy()), torch.from_numpy(tgt.copy())
        a, b = loss.terms(e, t), loss.terms(e, t)
        assert torch.equal(a, b)
        for i in range(e.shape[0]):
            assert torch.equal(loss.terms(e[i:i + 1], t[i:i + 1])[0], a[i]), (mode, i)


def test_forward_is_the_mean_of_the_items_terms(emu_default):
    est, tgt, kw = R.case_inputs("noise", 9001)
    loss = MultiScale_Spectral_Loss_MidSide_DDSP()
    e, t = torch.from_numpy(est), torch.from_numpy(tgt)
    v = loss.terms(e, t)
    assert v.dtype == torch.float64 and tuple(v.shape) == (2, 4, 2, 2)
    m = v.mean(0)
    want = 0.9 * (0.5 * m[:, 0, 0] + 0.5 * m[:, 1, 0]).sum() + 0.1 * (0.5 * m[:, 0, 1] + 0.5 * m[:, 1, 1]).sum()
    out = loss(e, t)
    assert out.dim() == 0 and out.dtype == torch.float32 and float(out) == float(want.to(torch.float32))


def _create(emu, **over):
    args = dict(mode=0, n_fft=[1024], hop=[256], win_length=[1024], window=0, eps=1e-7)
    args.update(over)
    h = C.c_void_p()
    rc = emu.mst_mss_create(C.byref(_lib.MstMssDesc(**args)), C.byref(h))
    return rc, h, (emu.mst_last_error() or b"").decode()


@pytest.mark.parametrize("over,needle", [
    (dict(n_fft=[1000]), "n_fft = 1000"), (dict(n_fft=[128], hop=[32], win_length=[128]), "n_fft = 128"),
    (dict(n_fft=[8192], hop=[2048], win_length=[8192]), "n_fft = 8192"), (dict(hop=[0]), "hop = 0"), (dict(hop=[1025]), "hop = 1025"),
    (dict(win_length=[1025]), "win_length = 1025"), (dict(win_length=[0]), "win_length = 0"), (dict(mode=2), "mode = 2"),
    (dict(window=5), "window = 5"), (dict(eps=-1.0), "eps = -1"),
    (dict(n_fft=[512] * 9, hop=[128] * 9, win_length=[512] * 9), "n_scales = 9"), (dict(n_fft=[], hop=[], win_length=[]), "n_scales = 0")])
def test_unsupported_descriptors_name_the_offending_value(emu, over, needle):
    rc, _, msg = _create(emu, **over)
    assert rc == -2 and needle in msg, (rc, msg)


def test_unsupported_lengths_and_bad_arguments(emu):
    rc, h, _ = _create(emu, n_fft=[4096, 512], hop=[1024, 128], win_length=[4096, 512])
    assert rc == 0
    x = torch.zeros(1, 2, 2048)
    out = torch.zeros(1, 2, 2, 2, dtype=torch.float64)
    ws = torch.zeros(1 << 16, dtype=torch.uint8)
    assert emu.mst_mss_forward(h, x.data_ptr(), x.data_ptr(), 1, 2048, out.data_ptr(), ws.data_ptr(), ws.numel(), None) == -2
    assert b"L = 2048" in emu.mst_last_error() and b"2048" in emu.mst_last_error()
    mag = torch.zeros(1, 2, 256, 64)
    assert emu.mst_mss_spectrogram(h, 1, x.data_ptr(), 1, 2, 2048, mag.data_ptr(), None) == 0           # only the scale asked for must fit
    assert emu.mst_mss_spectrogram(h, 0, x.data_ptr(), 1, 2, 2048, mag.data_ptr(), None) == -2 and b"L = 2048" in emu.mst_last_error()
    assert emu.mst_mss_spectrogram(h, 1, x.data_ptr(), 70000, 2, 2048, mag.data_ptr(), None) == -2 and b"B = 70000" in emu.mst_last_error()
    assert emu.mst_mss_spectrogram(h, 1, x.data_ptr(), 1, 3, 4096, mag.data_ptr(), None) == -2 and b"C = 3" in emu.mst_last_error()
    assert emu.mst_mss_spectrogram(h, 2, x.data_ptr(), 1, 2, 4096, mag.data_ptr(), None) == -1
    assert emu.mst_mss_forward(h, None, x.data_ptr(), 1, 4096, out.data_ptr(), ws.data_ptr(), ws.numel(), None) == -1
    assert emu.mst_mss_forward(h, x.data_ptr(), x.data_ptr(), 1, 4096, out.data_ptr(), ws.data_ptr(), 8, None) == -5
    assert emu.mst_mss_frames(h, 0, 131072) == 128 and emu.mst_mss_frames(h, 1, 131000) == 1024
    assert emu.mst_mss_workspace_bytes(h, 32, 131072) >= 2 * 32 * 2 * 128 * 16
    d = _lib.MstMssDesc(0, [1024], [256], [1024])
    d.struct_size += 4
    h2 = C.c_void_p()
    assert emu.mst_mss_create(C.byref(d), C.byref(h2)) == -1
    # hop 4096 at L = 3072: L // hop = 0 and the one frame is the dropped one
    rc, h3, _ = _create(emu, n_fft=[4096], hop=[4096], win_length=[4096])
    x3 = torch.zeros(1, 2, 3072)
    assert emu.mst_mss_forward(h3, x3.data_ptr(), x3.data_ptr(), 1, 3072, out.data_ptr(), ws.data_ptr(), ws.numel(), None) == -2
    assert b"no frame" in emu.mst_last_error()
    for hh in (h, h3):
        assert emu.mst_mss_destroy(hh) == 0


def test_module_refusals_through_the_emulator(emu_default):
    loss = MultiScale_Spectral_Loss_MidSide_DDSP()
    x = torch.zeros(1, 2, 4096)
    with pytest.raises(NotImplementedError, match="L = 2000"):
        loss(torch.zeros(1, 2, 2000), torch.zeros(1, 2, 2000))
    with pytest.raises(NotImplementedError, match="n_fft = 3000"):
        MultiScale_Spectral_Loss_MidSide_DDSP(n_filters=[3000], windows_size=[3000], hops_size=[750])(x, x)
    with pytest.raises(NotImplementedError, match="cplx|mag"):
        FrontEnd()(x, mode=["cplx"])
    with pytest.raises(NotImplementedError):
        FrontEnd()(x, mode=["cplx", "mag"])
    with pytest.raises(NameError):
        FrontEnd()(x, mode=[])
    with pytest.raises(NotImplementedError):
        BackEnd()
    with pytest.raises(ValueError):
        loss(x, torch.zeros(1, 2, 4097))
    with pytest.raises(TypeError):
        loss(x.double(), x.double())


def test_refusals_on_the_product_binding():
    """forward only, and no CPU path: the product library refuses what it cannot do (no GPU is needed to be refused)"""
    assert not isinstance(_lib.lib(), type(None)) and _lib.lib().path == _lib.LIB_PATH
    with pytest.raises(NotImplementedError, match="reduce"):
        MultiScale_Spectral_Loss_MidSide_DDSP(reduce=False)
    loss = MultiScale_Spectral_Loss_MidSide_DDSP()
    x = torch.zeros(1, 2, 8192)
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss(x, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss.terms(x, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        FrontEnd()(x, mode=["mag"])


def test_requires_grad_is_refused(emu_default):
    loss = MultiScale_Spectral_Loss_MidSide_DDSP()
    x = torch.zeros(1, 2, 8192)
    g = torch.zeros(1, 2, 8192, requires_grad=True)
    with pytest.raises(NotImplementedError, match="requires grad"):
        loss(g, x)
    with pytest.raises(NotImplementedError, match="requires grad"):
        loss(x, g)
    with pytest.raises(NotImplementedError, match="requires grad"):
        FrontEnd()(g, mode=["mag"])
