"""Float64 restatement of the polyphase resampler (csrc/resample_kernels.h) and its per-element bound.

y[m] = sum_j h[m down - j up + half] x[j] over the float32 taps h the LIBRARY returns (mst_resample_taps) and float32 inputs x, zero
outside the signal; NumPy float64, vectorised over the outputs with a loop over the taps of a phase.  S[m] = sum |h x| comes with it.

Bound of one output: |y - y64| <= 2^-24 |y64| + 2^-149 + (T + 2) 2^-53 S, T = taps per phase - one float32 rounding of the sum, float32's
smallest step (a sum below the normal range), and float64 accumulation of T exact products in any order (the restatement's own order
included: hence T + 2, not T - 1)."""
import numpy as np

RATIOS = {(147, 160): (48000, 44100), (147, 320): (96000, 44100), (441, 320): (32000, 44100), (1, 2): (88200, 44100),
          (2, 1): (22050, 44100), (4, 1): (44100, 176400)}          # up / down -> a pair of rates that reduces to it


def design(up, down):
    """float32(up * scipy.signal.firwin(2 half + 1, fc, window=('kaiser', 12.0))) and half"""
    from scipy.signal import firwin
    mx = max(up, down)
    half = 64 * mx
    return (up * firwin(2 * half + 1, 0.945 / mx, window=("kaiser", 12.0))).astype(np.float32), half


def out_length(n_in, up, down):
    return -((-n_in * up) // down)


def resample64(x, taps, up, down, n_out=None, in_start=0, out_start=0):
    """x float32 [n_in, C] = inputs in_start .. of a signal that is zero elsewhere; taps float32 [2 half + 1] -> (y64, S) float64 [n_out, C] of
    outputs out_start .."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and taps.dtype == np.float32 and x.ndim == 2
    half = (len(taps) - 1) // 2
    n_in = x.shape[0]
    n_out = out_length(n_in, up, down) if n_out is None else n_out
    h = np.concatenate((taps.astype(np.float64), np.zeros(up)))
    xz = np.concatenate((x.astype(np.float64), np.zeros((1, x.shape[1]))))          # row n_in: the zero outside the buffer
    m = out_start + np.arange(n_out, dtype=np.int64)
    n = m * down + half
    q, r = n // up, n % up
    T = 2 * half // up + 1
    y, S = np.zeros((n_out, x.shape[1])), np.zeros((n_out, x.shape[1]))
    for t in range(T):
        j = q - t - in_start
        p = h[r + t * up][:, None] * xz[np.where((j >= 0) & (j < n_in), j, n_in)]
        y += p
        S += np.abs(p)
    return y, S


def bound(y64, S, T):
    return 2.0 ** -24 * np.abs(y64) + 2.0 ** -149 + (T + 2) * 2.0 ** -53 * S


def ratio(err, bnd):
    return float(np.max(err / bnd)) if err.size else 0.0


def noise(n, C, seed):
    return (0.3 * np.random.default_rng(seed).standard_normal((n, C))).astype(np.float32)


# ---- the checks both suites run (tests/test_resample_emu.py on the CPU emulator, tests/test_resample_gpu.py on the MI355X) -----------------
def _dev(a, device):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def get(D, up, down):
    ri, ro = RATIOS[(up, down)]
    rs = D.Resampler.get(ri, ro)
    info = rs.info()
    assert info[:2] == (up, down)
    return rs, rs.taps(), info[3]


def check_taps(D):
    import scipy.signal  # noqa: F401
    pairs = dict(RATIOS)
    pairs.update({("to 44.1 kHz", r): (r, 44100) for r in (8000, 11025, 16000, 24000, 192000)})
    for key, (ri, ro) in pairs.items():
        rs = D.Resampler.get(ri, ro)
        up, down, half, T = rs.info()
        g = int(np.gcd(ri, ro))
        assert (up, down, half, T) == (ro // g, ri // g, 64 * max(ro // g, ri // g), 2 * 64 * max(ro // g, ri // g) // (ro // g) + 1), key
        if ri == 48000:
            assert T == 140
        taps, (ref, _) = rs.taps(), design(up, down)
        assert taps.dtype == np.float32 and taps.shape == (2 * half + 1,)
        assert np.all(np.abs(taps.astype(np.float64) - ref) <= np.spacing(np.maximum(np.abs(taps), np.abs(ref)))), key
        lib = rs.lib
        for n in (0, 1, 7, 3001, 8_640_000, 691_200_000):          # the last: one hour at 192 kHz
            assert lib.mst_resample_length(rs._handle(), n) == out_length(n, up, down) == rs.length(n), (key, n)


def check_bound(D, device, up, down, n, C):
    """one item, then three items of different content: every element of every item within the bound"""
    rs, taps, T = get(D, up, down)
    xs = np.stack([noise(n, C, 100 * n + 10 * C + i) for i in range(3)])
    refs = [resample64(x, taps, up, down) for x in xs]          # once per item
    worst = 0.0
    for batch in (xs[:1], xs):
        y = rs.forward(_dev(batch, device)).cpu().numpy()
        assert y.shape == (len(batch), out_length(n, up, down), C) and y.dtype == np.float32
        for i in range(len(batch)):
            y64, S = refs[i]
            worst = max(worst, ratio(np.abs(y[i] - y64), bound(y64, S, T)))
    print(f"{up}/{down} n={n} C={C}: max err / bound = {worst:.4g}")
    assert worst <= 1.0
    return worst


def check_scipy(D, up, down):
    from scipy.signal import resample_poly
    rs, taps, T = get(D, up, down)
    x = noise(3001, 2, 5)
    y64, _ = resample64(x, taps, up, down)
    ind = resample_poly(x.astype(np.float64), up, down, axis=0, window=taps.astype(np.float64) / up)
    err = float(np.max(np.abs(ind - y64)))
    print(f"{up}/{down}: restatement against scipy.signal.resample_poly: {err:.3g}")
    assert ind.shape == y64.shape and err <= 1e-12


def check_impulse_and_silence(D, device, up, down):
    rs, taps, T = get(D, up, down)
    half, n = (len(taps) - 1) // 2, 300
    n_out = out_length(n, up, down)
    for j0 in (0, 137, n - 1):
        x = np.zeros((n, 2), np.float32)
        x[j0] = (1.0, -1.0)
        y = rs.forward(_dev(x[None], device)).cpu().numpy()[0]
        k = np.arange(n_out, dtype=np.int64) * down - j0 * up + half
        inside = (k >= 0) & (k <= 2 * half)
        want = np.where(inside, taps[np.clip(k, 0, 2 * half)], np.float32(0.0))
        assert inside.sum() > 0 and np.array_equal(y[:, 0], want) and np.array_equal(y[:, 1], -want), (up, down, j0)
        y1 = rs.forward(_dev(x[None, :, :1], device)).cpu().numpy()[0]
        assert np.array_equal(y1[:, 0], want)
    for C in (1, 2):
        y = rs.forward(_dev(np.zeros((2, n, C), np.float32), device)).cpu().numpy()
        assert y.shape == (2, n_out, C) and not np.any(y)


def check_determinism(D, device, up, down, n=3001):
    rs, taps, T = get(D, up, down)
    for C in (1, 2):
        xs = _dev(np.stack([noise(n, C, 40 + i) for i in range(3)]), device)
        a = rs.forward(xs)
        b = rs.forward(xs)
        assert bool((a == b).all())
        for i in range(3):
            assert bool((rs.forward(xs[i:i + 1])[0] == a[i]).all()), (up, down, C, i)


def input_span(m0, m1, up, down, half, n):
    """the input frames outputs m0 .. m1 - 1 read, inside a signal of n frames"""
    lo = max(0, -((half - m0 * down) // up))
    hi = min(n, ((m1 - 1) * down + half) // up + 1)
    return lo, max(lo + 1, hi)


def check_chunks(D, device, up, down, cuts=(0.26, 0.71), n=3001):
    """three calls with arbitrary out_start / n_out, each over an input buffer that just covers its span, against one call; and the same buffer
    2^30 periods further on"""
    rs, taps, T = get(D, up, down)
    half = (len(taps) - 1) // 2
    for C in (1, 2):
        x = noise(n, C, 77 + C)
        xd = _dev(x[None], device)
        whole = rs.forward(xd)
        n_out = whole.shape[1]
        edges = [0] + [int(c * n_out) | 1 for c in cuts] + [n_out]
        for m0, m1 in zip(edges[:-1], edges[1:]):
            lo, hi = input_span(m0, m1, up, down, half, n)
            part = rs.forward(xd[:, lo:hi], n_out=m1 - m0, in_start=lo, out_start=m0)
            assert bool((part == whole[:, m0:m1]).all()), (up, down, C, m0, m1)
        k = 1 << 30
        far = rs.forward(xd, n_out=n_out, in_start=k * down, out_start=k * up)
        assert bool((far == whole).all()), (up, down, C)


def check_refusals(lib, x_ptr, y_ptr, stream):
    """status codes straight from the C ABI; x_ptr / y_ptr: device buffers of at least 64 floats"""
    import ctypes as C
    h = C.c_void_p()
    assert lib.mst_resample_create(44100, 44101, C.byref(h)) == -2 and b"44101" in lib.mst_last_error()          # MST_ERR_UNSUPPORTED
    assert lib.mst_resample_create(44100, 44100, C.byref(h)) == -1                                               # MST_ERR_ARG
    assert lib.mst_resample_create(48000, 44100, None) == -1
    assert lib.mst_resample_create(0, 44100, C.byref(h)) == -1
    assert lib.mst_resample_create(48000, 44100, C.byref(h)) == 0
    try:
        assert lib.mst_resample_forward(h, x_ptr, 8, 0, y_ptr, 8, 0, 1, 3, stream) == -1 and b"C = 3" in lib.mst_last_error()
        assert lib.mst_resample_forward(h, None, 8, 0, y_ptr, 8, 0, 1, 2, stream) == -1
        assert lib.mst_resample_forward(h, x_ptr, 8, 0, None, 8, 0, 1, 2, stream) == -1
        assert lib.mst_resample_forward(None, x_ptr, 8, 0, y_ptr, 8, 0, 1, 2, stream) == -1
        assert lib.mst_resample_forward(h, x_ptr, 0, 0, y_ptr, 8, 0, 1, 2, stream) == -1
        assert lib.mst_resample_info(None, None, None, None, None) == -1
        assert lib.mst_resample_length(None, 5) == -1
        assert lib.mst_resample_taps(h, None, 20481) == -1
        buf = (C.c_float * 8)()
        assert lib.mst_resample_taps(h, buf, 8) == -1
    finally:
        assert lib.mst_resample_destroy(h) == 0
    assert lib.mst_resample_destroy(None) == 0


def check_tones(D, device):
    """48 -> 44.1 kHz, 6000 frames, interior outputs (300 dropped at each end)"""
    rs, taps, T = get(D, 147, 160)
    j, res = np.arange(6000), {}
    for f in (997.0, 19000.0, 23000.0):
        x = (0.5 * np.sin(2 * np.pi * f * j / 48000.0)).astype(np.float32)
        y = rs.forward(_dev(x[None, :, None], device)).cpu().numpy()[0, 300:-300, 0].astype(np.float64)
        m = np.arange(300, 300 + len(y))
        if f < 22050.0:
            res[f] = float(np.max(np.abs(y - 0.5 * np.sin(2 * np.pi * f * m / 44100.0))))
            print(f"{f:.0f} Hz: max deviation from the sine at 44.1 kHz {res[f]:.3g}")
            assert res[f] <= 1e-6
        else:
            res[f] = 20 * np.log10(np.sqrt(np.mean(y * y)) / np.sqrt(np.mean(x.astype(np.float64) ** 2)))
            print(f"{f:.0f} Hz: {res[f]:.1f} dB")
            assert res[f] <= -110.0
    return res


def check_true_peak(D, device):
    """4 / 1: a sine at a quarter of the sampling rate, phase 45 degrees - every sample sits 3.01 dB under the peak"""
    rs, taps, T = get(D, 4, 1)
    A = 0.5
    x = (A * np.sin(2 * np.pi * np.arange(1000) / 4.0 + np.pi / 4)).astype(np.float32)
    assert abs(20 * np.log10(np.abs(x).max() / A) + 3.0103) < 1e-3
    y = rs.forward(_dev(x[None, :, None], device)).cpu().numpy()[0, 300:-300, 0]
    rel = abs(float(np.abs(y).max()) - A) / A
    print(f"true peak at 4x: {rel:.3g} relative")
    assert rel <= 1e-5


# ---- files ----------------------------------------------------------------------------------------------------------------------------------
def write_wav(path, pcm, rate, width):
    """pcm int [L, nch] at `width` bytes per sample (2: int16, 3: 24-bit in int32, 4: int32)"""
    import wave
    pcm = np.asarray(pcm)
    if width == 3:
        raw = pcm.astype("<i4").reshape(-1, 1).view(np.uint8).reshape(-1, 4)[:, :3].tobytes()
    else:
        raw = pcm.astype("<i2" if width == 2 else "<i4").tobytes()
    with wave.open(str(path), "w") as w:
        w.setnchannels(pcm.shape[1])
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(raw)


def pcm_noise(n, width, seed, nch=2):
    full = 2 ** (8 * width - 1)
    v = np.random.default_rng(seed).standard_normal((n, nch)) * 0.2 * full
    return np.clip(np.rint(v), -full, full - 1).astype(np.int64)


def check_loaders(D, device, tmp_path):
    from music_mixing_style_transfer_amd.data_loader import load_wav_device, load_wav_segment
    import pytest
    cases = {"a48_16.wav": (48000, 2, 2501), "b96_24.wav": (96000, 3, 3333)}
    for name, (rate, width, n) in cases.items():
        pcm = pcm_noise(n, width, n)
        pcm[0], pcm[1] = -2 ** (8 * width - 1), 2 ** (8 * width - 1) - 1          # the ends of the range: the sign extension
        write_wav(tmp_path / name, pcm, rate, width)
        path = str(tmp_path / name)
        for fn in (lambda **k: load_wav_device(path, device, **k), lambda **k: load_wav_segment(path, axis=0, **k)):
            with pytest.raises(ValueError, match="sample rate should be 44100"):
                fn()
            with pytest.raises(ValueError, match="sample rate should be 44100"):
                fn(convert=False)
        rs = D.Resampler.get(rate, 44100)
        up, down, half, T = rs.info()
        dec = (pcm / float(2 ** (8 * width - 1))).astype(np.float32)
        y64, S = resample64(dec, rs.taps(), up, down)
        got = load_wav_device(path, device, convert=True)
        assert got.dtype.is_floating_point and tuple(got.shape) == (2, rs.length(n)) and got.is_contiguous()
        r = ratio(np.abs(got.cpu().numpy().T - y64), bound(y64, S, T))
        print(f"{name}: load_wav_device max err / bound = {r:.4g}")
        assert r <= 1.0
        host = load_wav_segment(path, axis=0, convert=True)
        assert host.dtype == np.float64 and np.array_equal(host, got.cpu().numpy().astype(np.float64))
        seg = load_wav_segment(path, start_point=100, duration=500, axis=1, convert=True)
        assert np.array_equal(seg, host.T[100:600])
    # 44.1 kHz: 16-bit gives the same bits either way; 24-bit needs the flag and is then exact
    pcm = pcm_noise(999, 2, 3)
    write_wav(tmp_path / "c441_16.wav", pcm, 44100, 2)
    p = str(tmp_path / "c441_16.wav")
    assert bool((load_wav_device(p, device) == load_wav_device(p, device, convert=True)).all())
    assert np.array_equal(load_wav_segment(p, axis=0), load_wav_segment(p, axis=0, convert=True))
    assert np.array_equal(load_wav_segment(p, 10, 50), load_wav_segment(p, 10, 50, convert=True))
    pcm = pcm_noise(777, 3, 4)
    pcm[5], pcm[6] = -2 ** 23, 2 ** 23 - 1
    write_wav(tmp_path / "d441_24.wav", pcm, 44100, 3)
    p = str(tmp_path / "d441_24.wav")
    for fn in (lambda **k: load_wav_device(p, device, **k), lambda **k: load_wav_segment(p, axis=0, **k)):
        with pytest.raises(ValueError, match="bit depth should be 16 or 32-bit"):
            fn()
    assert np.array_equal(load_wav_segment(p, axis=0, convert=True), (pcm / float(2 ** 23)).T)
    assert np.array_equal(load_wav_device(p, device, convert=True).cpu().numpy(), (pcm / float(2 ** 23)).astype(np.float32).T)


STEMS = ["drums", "bass", "other", "vocals"]


def write_song(root, L_in=30000, L_ref=40000, ref_rate=48000):
    """<root>/song0/separated/{input at 44.1 kHz, reference at ref_rate}/<stem>.wav, 16-bit; returns the reference stems' PCM"""
    from music_mixing_style_transfer_amd.utils import synth
    refs = {}
    for kind, L, rate in (("input", L_in, 44100), ("reference", L_ref, ref_rate)):
        d = root / "song0" / "separated" / kind
        d.mkdir(parents=True)
        for k, s in enumerate(STEMS):
            x = synth.synth_music(2, L, seed=10 * k + (0 if kind == "input" else 3), sr=rate).numpy()
            pcm = np.clip(np.rint(x.T * 32767), -32768, 32767).astype(np.int64)
            write_wav(d / (s + ".wav"), pcm, rate, 2)
            if kind == "reference":
                refs[s] = pcm
    return refs


def dataset_args(root, convert):
    import types
    return types.SimpleNamespace(target_dir=str(root) + "/", interpolation=False, instruments=list(STEMS), input_file_name="input",
                                 reference_file_name="reference", stem_level_directory_name="separated", do_not_separate=True,
                                 separation_model="mdx_extra", normalize_input=False, sample_rate=44100, workers=0, convert_input=convert)


def check_dataset(D, device, tmp_path):
    """44.1 kHz input stems stacked with 48 kHz reference stems; the device path and the host path give the same samples"""
    import pytest
    import torch
    from music_mixing_style_transfer_amd.data_loader import Song_Dataset_Inference
    refs = write_song(tmp_path / "data")
    n_ref = D.Resampler.get(48000, 44100).length(40000)
    items = []
    for dev in (device, None):
        ds = Song_Dataset_Inference(dataset_args(tmp_path / "data", True))
        ds.device = dev
        inputs, reference, name = ds[0]
        assert tuple(inputs.shape) == (4, 2, 30000) and tuple(reference.shape) == (4, 2, n_ref) and reference.dtype == torch.float32
        items.append(reference.cpu())
        path = str(tmp_path / "data" / "song0" / "separated" / "reference" / "bass.wav")
        assert ds._frames(path) == n_ref and ds._frames(path.replace("reference", "input")) == 30000
    assert torch.equal(items[0], items[1])
    want = D.resample(_dev((refs["bass"] / 32768.0).astype(np.float32), device), 48000, 44100).cpu().clamp(-1, 1).t()
    assert torch.equal(items[0][1], want)
    for dev in (device, None):
        ds = Song_Dataset_Inference(dataset_args(tmp_path / "data", False))
        ds.device = dev
        with pytest.raises(ValueError, match="sample rate should be 44100"):
            ds[0]
    ns = dataset_args(tmp_path / "data", False)
    del ns.convert_input
    assert Song_Dataset_Inference(ns).convert is False
    return refs
