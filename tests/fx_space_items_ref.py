"""Per-item panner, Haas and reverbs (mst_fx_panner_items, mst_fx_haas_items, mst_fx_convolve_items, mst_fx_algorithmic_reverb_items): the case
bodies of tests/test_fx_space_items_emu.py and tests/test_fx_space_items_gpu.py, written once.  Item i of a per-item call against the shared-parameter
call on the same batch with item i's settings, bit for bit; against float64 references; process_items against process(); and a whole
instrument chain through AugmentationChain.call_items against oracle.fx_ref composed as the items' plans say."""
import ctypes as C
import os
import random

import numpy as np
import torch

import fx_items_ref as I
from music_mixing_style_transfer_amd import _lib
from oracle import fx_ref as F

HERE = os.path.dirname(os.path.abspath(__file__))
same_bits = I.same_bits


def noise(shape, seed, amp=0.2):
    return (amp * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)


def stereo(x):
    """[n, L, c] -> [n, L, 2]: mono repeated"""
    return np.ascontiguousarray(np.repeat(x, 2, axis=2) if x.shape[2] == 1 else x)


# ---------------------------------------------------------------------------------------------------------- 1. panner
PAN_GAINS = np.array([[1.0, 0.0], [0.0, 1.0], [0.70710677, 0.70710677], [0.3, 0.95], [0.59460354, 0.59460354]], dtype=np.float32)


def check_panner(run, L, c_in, n=5):
    lib = run.lib
    x = noise((n, L, c_in), 21)
    xt, gt = run.t(x), run.t(PAN_GAINS[:n])
    yt = torch.full((n, L, 2), float("nan"), dtype=torch.float32, device=run.device)
    with lib.device_ctx(xt):
        lib.check(lib.mst_fx_panner_items(xt.data_ptr(), yt.data_ptr(), n, L, c_in, gt.data_ptr(), lib.stream_ptr(xt)), "mst_fx_panner_items")
        y = yt.cpu().numpy()
        for i in range(n):
            st = torch.empty_like(yt)
            lib.check(lib.mst_fx_panner(xt.data_ptr(), st.data_ptr(), n, L, c_in, float(PAN_GAINS[i, 0]), float(PAN_GAINS[i, 1]), lib.stream_ptr(xt)), "mst_fx_panner")
            assert same_bits(y[i], st.cpu().numpy()[i]), f"panner L={L} c_in={c_in} item {i}: the shared call's bits"
    assert np.array_equal(y, stereo(x) * PAN_GAINS[:n, None, :]), f"panner L={L} c_in={c_in}: x * gains in float32"


# ---------------------------------------------------------------------------------------------------------- 2. Haas
def check_haas(run, L, c_in, n=5):
    lib = run.lib
    x = noise((n, L, c_in), 22)
    delays = np.array([0, 37, -12, L, -3 * L - 5], dtype=np.int64)
    fbs = np.array([0.33, 0.41, 0.5, 0.58, 0.66], dtype=np.float64)
    chans = np.array([0, 1, 1, 0, 7], dtype=np.int32)
    xt, dt, ft, ct = run.t(x), run.t(delays), run.t(fbs), run.t(chans)
    yt = torch.full((n, L, 2), float("nan"), dtype=torch.float32, device=run.device)
    with lib.device_ctx(xt):
        lib.check(lib.mst_fx_haas_items(xt.data_ptr(), yt.data_ptr(), n, L, c_in, dt.data_ptr(), ft.data_ptr(), ct.data_ptr(), lib.stream_ptr(xt)), "mst_fx_haas_items")
        y = yt.cpu().numpy()
        xs = stereo(x)
        for i in range(n):
            what = f"haas L={L} c_in={c_in} item {i}"
            if chans[i] not in (0, 1):
                assert np.array_equal(y[i], xs[i]), what + ": an unknown wet channel leaves the stereo-expanded input"
                continue
            st = torch.empty_like(yt)
            lib.check(lib.mst_fx_haas(xt.data_ptr(), st.data_ptr(), n, L, c_in, int(delays[i]), float(fbs[i]), int(chans[i]), lib.stream_ptr(xt)), "mst_fx_haas")
            assert same_bits(y[i], st.cpu().numpy()[i]), what + ": the shared call's bits"
            assert np.array_equal(y[i], F.haas(xs[i], int(delays[i]), float(fbs[i]), "left" if chans[i] == 0 else "right")), what + ": oracle.fx_ref.haas"
        if c_in == 2:
            rc = lib.mst_fx_haas_items(xt.data_ptr(), xt.data_ptr(), n, L, c_in, dt.data_ptr(), ft.data_ptr(), ct.data_ptr(), lib.stream_ptr(xt))
            assert rc == -1 and b"in-place" in lib.mst_last_error()


# ---------------------------------------------------------------------------------------------------------- 3. / 4. convolution
def decaying_noise(frames, Cn, seed, tau):
    """seeded noise with an exponential decay, [frames, Cn] float32"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((frames, Cn)) * np.exp(-np.arange(frames) / tau)[:, None] * 0.5).astype(np.float32)


class Convolver:
    def __init__(self, lib, L, lh_max, n, Cn):
        self.lib, self.h = lib, C.c_void_p()
        lib.check(lib.mst_fx_convolver_create(L, lh_max, n, Cn, C.byref(self.h)), "mst_fx_convolver_create")

    def close(self):
        self.lib.mst_fx_convolver_destroy(self.h)


def conv_prepare(lib, cv, starts, lens, bank_frames, params, n_items=None, table_bytes=None):
    """-> (rc, table float64 array, first_bad_item)"""
    starts, lens = np.ascontiguousarray(starts, dtype=np.int64), np.ascontiguousarray(lens, dtype=np.int64)
    params = np.ascontiguousarray(params, dtype=np.float64)
    n = params.shape[0] if n_items is None else n_items
    nbytes = lib.mst_fx_convolve_items_table_bytes(n, len(lens))
    table = np.full(max(1, nbytes // 8), np.nan)
    bad = C.c_int(-7)
    rc = lib.mst_fx_convolve_items_prepare(cv.h, starts.ctypes.data, lens.ctypes.data, len(lens), bank_frames, params.ctypes.data, n, table.ctypes.data,
                                           nbytes if table_bytes is None else table_bytes, C.byref(bad))
    return rc, table, bad.value


def conv_items_call(run, cv, x, responses, params):
    """responses: list of [Lh_r, C] float32; params [n][4] = response index, offset, dry, wet -> y of one mst_fx_convolve_items call"""
    lib = run.lib
    n = x.shape[0]
    lens = [h.shape[0] for h in responses]
    starts = np.concatenate([[0], np.cumsum(lens)[:-1]])
    bank = np.concatenate(responses, axis=0)
    rc, table, bad = conv_prepare(lib, cv, starts, lens, bank.shape[0], params)
    assert rc == 0 and bad == -1 and np.isfinite(table).all(), (rc, bad, lib.mst_last_error())
    xt, bt, tt = run.t(x), run.t(bank), run.t(table)
    yt = torch.full(x.shape, float("nan"), dtype=torch.float32, device=run.device)
    nbytes = lib.mst_fx_convolver_items_workspace_bytes(cv.h, len(responses))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=run.device)
    with lib.device_ctx(xt):
        lib.check(lib.mst_fx_convolve_items(cv.h, xt.data_ptr(), bt.data_ptr(), tt.data_ptr(), n, len(responses), yt.data_ptr(), ws.data_ptr(), nbytes,
                                            lib.stream_ptr(xt)), "mst_fx_convolve_items")
    return yt.cpu().numpy()


def conv_shared_call(run, cv, x, h, offset, dry, wet):
    lib = run.lib
    xt, ht = run.t(x), run.t(h)
    yt = torch.full(x.shape, float("nan"), dtype=torch.float32, device=run.device)
    nbytes = lib.mst_fx_convolver_workspace_bytes(cv.h)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=run.device)
    with lib.device_ctx(xt):
        lib.check(lib.mst_fx_convolve(cv.h, xt.data_ptr(), ht.data_ptr(), h.shape[0], yt.data_ptr(), int(offset), float(dry), float(wet), ws.data_ptr(),
                                      nbytes, lib.stream_ptr(xt)), "mst_fx_convolve")
    return yt.cpu().numpy()


def conv_reference(x, h, offset, dry, wet, use_scipy):
    """dry * x + wet * full_convolution[offset : offset + L] in float64, per channel; wet == 0: x (ConvolutionalReverb.process returns its input)"""
    if wet == 0.0:
        return x.astype(np.float64)
    x64, h64 = x.astype(np.float64), h.astype(np.float64)
    if use_scipy:
        from scipy.signal import fftconvolve
        full = fftconvolve(x64, h64, mode="full", axes=0)
    else:
        full = np.stack([np.convolve(x64[:, c], h64[:, c]) for c in range(x.shape[1])], 1)
    return dry * x64 + wet * full[offset:offset + x.shape[0]]


def check_conv(run, x, responses, params, lh_max, use_scipy, log=print):
    """(a) item i = mst_fx_convolve on the SAME convolver and batch with item i's response and settings, bit for bit (an item with wet == 0: its
    input, bit for bit - process() never sends it to mst_fx_convolve); (b) within 5e-6 max|ref| of the float64 convolution"""
    n, L, Cn = x.shape
    cv = Convolver(run.lib, L, lh_max, n, Cn)
    try:
        y = conv_items_call(run, cv, x, responses, params)
        shared = {}
        for i, (r, off, dry, wet) in enumerate(params):
            what = f"convolve_items L={L} C={Cn} item {i} (response {r}, offset {off}, dry {dry}, wet {wet})"
            if wet == 0.0:
                assert same_bits(y[i], x[i]), what + ": wet == 0 returns the input"
            else:
                key = (r, off, dry, wet)
                if key not in shared:
                    shared[key] = conv_shared_call(run, cv, x, responses[r], off, dry, wet)
                assert same_bits(y[i], shared[key][i]), what + ": the shared call's bits"
            ref = conv_reference(x[i], responses[r], off, dry, wet, use_scipy)
            dev = float(np.abs(y[i] - ref).max() / np.abs(ref).max())
            log(f"{what}: deviation {dev:.2e} of max|ref|")
            assert dev <= 5e-6, what + f": {dev:.2e} of max|ref|"
    finally:
        cv.close()


def check_conv_one_block(run, Cn, log=print):
    """L = 1200: one transform block.  Three responses of 1, 50 and 400 frames in one bank; two items share the longest at offsets 0 and 399"""
    x = noise((6, 1200, Cn), 31)
    responses = [decaying_noise(1, Cn, 41, 1.0), decaying_noise(50, Cn, 42, 12.0), decaying_noise(400, Cn, 43, 90.0)]
    params = [(2, 0, 0.3, 0.7), (2, 399, 0.0, 1.0), (0, 0, 0.5, 0.5), (1, 10, 0.25, 0.0), (1, 49, 1.0, 0.2), (0, 0, 0.0, 1.0)]
    check_conv(run, x, responses, params, 400, False, log)


def check_conv_overlap_save(run, n, Cn, items, seed=51, log=print):
    """L = 262144 with Lh_max = 300: L + Lh_max - 1 > 2^18, blocks of 65536 samples, five per sequence, shift 299, step 65237; the offsets
    put the cut at different phases of the block boundaries"""
    L = 262144
    x = noise((n, L, Cn), seed)
    responses = [decaying_noise(300, Cn, seed + 1, 70.0), decaying_noise(7, Cn, seed + 2, 3.0)]
    check_conv(run, x, responses, [(r, off, dry, wet) for (r, off), (dry, wet) in zip(items, [(0.2, 0.8), (0.0, 1.0), (0.6, 0.4)])], 300, True, log)


def check_conv_refusals(run):
    """mst_fx_convolve_items_prepare names what it refuses; the sizes grow with n_resp; a short workspace is refused.  Nothing is launched."""
    lib = run.lib
    cv = Convolver(lib, 1200, 400, 4, 2)
    try:
        starts, lens, frames = [0, 400], [400, 50], 450
        ok = [(0, 0, 0.0, 1.0), (1, 49, 0.5, 0.5), (0, 399, 0.0, 1.0), (1, 0, 1.0, 0.0)]
        rc, table, bad = conv_prepare(lib, cv, starts, lens, frames, ok)
        assert rc == 0 and bad == -1
        assert table[:4].tolist() == [0, 400, 400, 50] and table[4:].reshape(4, 5)[:, 4].tolist() == [0, 0, 0, 1], "the wet == 0 item is flagged"

        def refused(params, want_rc, want_bad, *words, starts=starts, lens=lens, frames=frames, n_items=None):
            rc, _, bad = conv_prepare(lib, cv, starts, lens, frames, params, n_items=n_items)
            msg = lib.mst_last_error().decode()
            assert rc == want_rc and bad == want_bad and all(w in msg for w in words), (rc, bad, msg)

        refused(ok[:2] + [(1, 50, 0.0, 1.0)] + ok[3:], -1, 2, "item 2", "offset")                       # offset == len
        refused(ok[:1] + [(2, 0, 0.0, 1.0)] + ok[2:], -1, 1, "item 1", "response index")                # response index == n_resp
        refused(ok, -1, -1, "response 0", "401", starts=[0, 401], lens=[401, 50], frames=451)           # longer than Lh_max
        refused(ok, -1, -1, "response 1", "outside the bank", frames=449)                               # start + len > bank_frames
        refused(ok + [ok[0]], -1, 4, "item 4", "created for 4")                                         # more items than the convolver holds
        assert lib.mst_fx_convolve_items_table_bytes(4, 3) > lib.mst_fx_convolve_items_table_bytes(4, 2) > 0
        w2, w3 = lib.mst_fx_convolver_items_workspace_bytes(cv.h, 2), lib.mst_fx_convolver_items_workspace_bytes(cv.h, 3)
        n_fft = 2048
        assert w3 - w2 == 2 * (n_fft * 4 + (n_fft // 2 + 1) * 8) and w2 > lib.mst_fx_convolver_workspace_bytes(cv.h)
        t = torch.zeros(64, dtype=torch.float64, device=run.device)
        rc = lib.mst_fx_convolve_items(cv.h, t.data_ptr(), t.data_ptr(), t.data_ptr(), 4, 2, t.data_ptr(), t.data_ptr(), w2 - 1, lib.stream_ptr(t))
        assert rc == -5 and b"workspace" in lib.mst_last_error()
        big = Convolver(lib, 262144, 300, 4, 2)           # five blocks per sequence: (n_items * 5 + n_resp) * 2 <= 65535 is far away, the rule is the convolver's
        try:
            assert conv_prepare(lib, big, [0], [300], 300, [(0, 0, 0.0, 1.0)] * 4)[0] == 0
        finally:
            big.close()
    finally:
        cv.close()


# ---------------------------------------------------------------------------------------------------------- 6. algorithmic reverb
COMBS = (1422, 1491, 1557, 1617)
ALLPASS = (556, 556 + 23, 441, 441 + 23, 341, 341 + 23, 225, 255 + 23)
SPREAD, IN_GAIN = 23, 0.2
REVERB_ORACLE = dict(room_size=0.62, damping=0.35, dry_mix=0.7, wet_mix=0.45, width=0.8)


def reverb_rows():
    """[4][5] = damping, room_size, wet1, wet2, dry: damping 0; the largest room; a row without wet signal; the oracle's row"""
    o = REVERB_ORACLE
    return np.array([[0.0, 0.5, 0.085, 0.015, 0.9], [0.9, 0.85, 0.3, 0.1, 0.2], [0.4, 0.3, 0.0, 0.0, 0.75],
                     [o["damping"], o["room_size"], o["wet_mix"] * ((o["width"] / 2) + 0.5), o["wet_mix"] * ((1 - o["width"]) / 2), o["dry_mix"]]], dtype=np.float64)


def check_algorithmic_reverb(run, Cn, L=5000, n=4, log=print):
    lib = run.lib
    assert L > 1617 + 23
    x = noise((n, L, Cn), 61)
    rows = reverb_rows()
    combs, ap = (C.c_int * 4)(*COMBS), (C.c_int * 8)(*ALLPASS)
    xt, pt = run.t(x), run.t(rows)
    nbytes = lib.mst_fx_algorithmic_reverb_scratch_bytes(n, L, 4)
    new = lambda: (torch.full((n, L, 2), float("nan"), dtype=torch.float32, device=run.device),
                   torch.full(((nbytes + 7) // 8,), float("nan"), dtype=torch.float64, device=run.device))
    with lib.device_ctx(xt):
        yt, sc = new()
        lib.check(lib.mst_fx_algorithmic_reverb_items(xt.data_ptr(), yt.data_ptr(), n, L, Cn, combs, 4, ap, 4, SPREAD, IN_GAIN, pt.data_ptr(), sc.data_ptr(),
                                                      nbytes, lib.stream_ptr(xt)), "mst_fx_algorithmic_reverb_items")
        y = yt.cpu().numpy()
        assert np.isfinite(y).all()
        for i, (damp, room, w1, w2, dry) in enumerate(rows):
            st, sc = new()
            lib.check(lib.mst_fx_algorithmic_reverb(xt.data_ptr(), st.data_ptr(), n, L, Cn, combs, 4, ap, 4, SPREAD, damp, room, IN_GAIN, w1, w2, dry,
                                                    sc.data_ptr(), nbytes, lib.stream_ptr(xt)), "mst_fx_algorithmic_reverb")
            assert same_bits(y[i], st.cpu().numpy()[i]), f"algorithmic reverb C={Cn} item {i}: the shared call's bits"
        assert lib.mst_fx_algorithmic_reverb_items(xt.data_ptr(), yt.data_ptr(), n, L, Cn, combs, 4, ap, 4, SPREAD, IN_GAIN, pt.data_ptr(), sc.data_ptr(),
                                                   nbytes - 8, lib.stream_ptr(xt)) == -5
    ref = F.algorithmic_reverb(x[3], **REVERB_ORACLE)
    dev = float(np.abs(y[3] - ref).max() / np.abs(ref).max())
    log(f"algorithmic reverb C={Cn} item 3 against the oracle: {dev:.2e} of max|ref|")
    assert dev <= 2e-6, f"{dev:.2e} of max|ref|"


# ---------------------------------------------------------------------------------------------------------- 7. process_items
def golden_responses():
    g = np.load(os.path.join(HERE, "golden", "fx_reverb.npz"))
    return g, [("300-600", "roomA", g["h_stereo"][:400]), ("300-600", "roomB", g["h_mono"][:300]), ("3000-6000", "hall", g["h_stereo"][:500]),
               ("0-300", "ignored", g["h_mono"][:50])]


def _restore(fx, v):
    for k, val in v.items():
        getattr(fx.parameters, k).value = val
    fx.update(None)


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def check_process_items(device, kind, log=print):
    """a batch of 4 items with values drawn by randomize() under a fixed seed: process_items(x, values)[i] against process(x[i:i+1]) after
    restoring values[i] - bit for bit, the convolution reverb (whose single-item call may pick another transform size) within 5e-6 max|ref|"""
    from music_mixing_style_transfer_amd.mixing_manipulator import AlgorithmicReverb, ConvolutionalReverb, Haas, Panner
    from music_mixing_style_transfer_amd.mixing_manipulator.common_audioeffects import parameter_values
    g, irs = golden_responses()
    if kind == "conv":
        fx = ConvolutionalReverb([[{"impulse_response": (lambda h=h: h)} for _, _, h in irs[:2]], [{"impulse_response": (lambda h=irs[2][2]: h)}]], 44100)
        P = fx.parameters          # the ranges the reference pins to one value, opened: every host-side step of process() differs between the items
        (P.wet.min, P.wet.max), (P.dry.min, P.dry.max), (P.decay.min, P.decay.max), (P.pre_delay.min, P.pre_delay.max) = (0.3, 1.0), (0.0, 0.5), (0.4, 1.0), (0, 4)
    else:
        fx = {"panner": Panner, "haas": lambda: Haas(44100), "algo": AlgorithmicReverb}[kind]()
    L = 2000 if kind == "algo" else 1200
    x = torch.from_numpy(np.stack([g["x"][150 * i:150 * i + L] * np.float32(1.0 - 0.2 * i) for i in range(4)])).to(device)
    random.seed(17)
    np.random.seed(17)
    values = []
    for _ in range(4):
        fx.randomize()
        values.append(parameter_values(fx))
    assert len({tuple(sorted(v.items())) for v in values}) == 4
    keep = parameter_values(fx)
    y = _np(fx.process_items(x, values))
    assert parameter_values(fx) == keep and y.shape == (4, L, 2)
    for i, v in enumerate(values):
        _restore(fx, v)
        want = _np(fx.process(x[i:i + 1]))[0]
        if kind == "conv":
            dev = float(np.abs(y[i] - want).max() / np.abs(want).max())
            log(f"ConvolutionalReverb.process_items item {i} {v}: {dev:.2e} of max|ref|")
            assert dev <= 5e-6, (i, dev)
        else:
            assert same_bits(y[i], want), (kind, i, v)
    return fx, x, values, y


def check_conv_process_items_split(device, monkeypatch):
    """a block limit of 12 instead of 65535: the four stereo items, four distinct (faded) responses, go through two calls of two - the bits of the one call"""
    from music_mixing_style_transfer_amd.mixing_manipulator import ConvolutionalReverb
    fx, x, values, y = check_process_items(device, "conv", log=lambda s: None)
    calls = []
    lib = _lib.lib()
    real = lib.mst_fx_convolve_items
    monkeypatch.setattr(lib, "mst_fx_convolve_items", lambda *a: calls.append(a[4]) or real(*a))
    monkeypatch.setattr(ConvolutionalReverb, "MAX_TRANSFORM_BLOCKS", 12)
    y2 = _np(fx.process_items(x, values))
    assert calls == [2, 2] and same_bits(y, y2)


# ---------------------------------------------------------------------------------------------------------- 8. / 9. the instrument chains
PROBS = {"eq": 1, "comp": 1, "pan": 1, "imager": 1, "reverb": 100, "gain": 1}          # reverb * 0.01 = 1 on the drums' low branch
CHAIN_SEEDS = {"vocals": 5, "drums": 6, "bass": 7}
_chain_refs = {}


def write_ir_dir(tmp_path):
    from music_mixing_style_transfer_amd.data_loader import save_wav_pcm16
    for rt, name, h in golden_responses()[1]:
        d = tmp_path / "IR_set1" / "RT60_avg" / rt / name
        d.mkdir(parents=True, exist_ok=True)
        save_wav_pcm16(str(d / "impulse_response.wav"), h)
    return str(tmp_path / "IR_")


def oracle_plan_item(x, plan, comp_fn, rate=44100):
    """oracle.fx_ref's processors composed as one item's plan says: every processor of an instrument chain, the kept input and the mix of a
    parallel chain, rms-normalise where flagged"""
    y = np.asarray(x, dtype=np.float32)
    kept = []
    for op in plan:
        if op[0] == "begin":
            kept.append(y)
            continue
        if op[0] == "mix":
            w = op[1]
            y = (w * kept.pop() + (1 - w) * y).astype(np.float32)
            continue
        _, fx, v, rms, extra = op
        name = type(fx).__name__
        if name == "Equaliser":
            z = F.equaliser(y, {b: (v[b + "_gain"], v[b + "_freq"], v.get(b + "_q", 0.707)) for b in fx.bands}, rate, bands=tuple(fx.bands))
        elif name == "Compressor":
            z = comp_fn(y, v["threshold"], v["attack_time"], v["release_time"], v["ratio"], rate)
        elif name == "MidSideImager":
            z = F.midside_imager(y, v["bal"])
        elif name == "Gain":
            z = F.gain(y, v["gain"], v["invert"])
        elif name == "Panner":
            z = y * F.panner_gains(v["pan"], v["pan_law"])
        elif name == "ConvolutionalReverb":
            z = F.conv_reverb(y, extra, v["dry"], v["wet"], v["pre_delay"])
        elif name == "AlgorithmicReverb":
            z = F.algorithmic_reverb(y, room_size=v["room_size"], damping=v["damping"], dry_mix=v["dry_mix"], wet_mix=v["wet_mix"], width=v["width"])
        else:
            raise AssertionError(name)
        if rms:
            z = F.rms_normalize(y, z)
        y = np.asarray(z).astype(np.float32)
    return y


def chain_case(inst, ir_dir, comp_fn):
    """-> (x [6, 1200, 2] float32, build(): a fresh chain, seed, per-item oracle outputs); the oracle replay runs once per instrument"""
    from music_mixing_style_transfer_amd.mixing_manipulator.audio_effects_chain import create_inst_effects_augmentation_chain
    seed = CHAIN_SEEDS[inst]
    build = lambda: create_inst_effects_augmentation_chain(inst, PROBS, ir_dir_path=None if inst == "bass" else ir_dir)
    g = golden_responses()[0]
    x = np.stack([g["x"][200 * i:200 * i + 1200] * np.float32(1.0 - 0.1 * i) for i in range(6)]).astype(np.float32)
    if inst not in _chain_refs:
        random.seed(seed)
        np.random.seed(seed)
        plans = build().plan_items(6, 2)          # a twin chain: the draws of the run
        fxs = [[op for op in p if op[0] == "fx"] for p in plans]
        assert len({op[2]["pan"] for p in fxs for op in p if type(op[1]).__name__ == "Panner"}) == 6, "the items drew different pan values"
        if inst == "bass":
            assert len({op[2]["room_size"] for p in fxs for op in p if type(op[1]).__name__ == "AlgorithmicReverb"}) == 6
        else:
            hs = [op[4] for p in fxs for op in p if type(op[1]).__name__ == "ConvolutionalReverb"]
            assert len(hs) >= 6 and len({(h.shape, h.tobytes()) for h in hs}) > 1, "the items drew different responses"
        assert all(any(op[0] == "mix" for op in p) for p in plans)
        _chain_refs[inst] = [oracle_plan_item(x[i], plans[i], comp_fn) for i in range(6)]
    return x, build, seed, _chain_refs[inst]


def check_inst_chain(device, inst, ir_dir, comp_fn, log=print):
    """a seeded instrument chain, six items of [1200, 2] through call_items: every item within 2e-5 max(1e-3, max|ref|) of the oracle replay"""
    x, build, seed, refs = chain_case(inst, ir_dir, comp_fn)
    chain = build()
    random.seed(seed)
    np.random.seed(seed)
    out = chain.call_items(torch.from_numpy(x).to(device))
    out = _np(out)
    assert out.shape == (6, 1200, 2) and np.isfinite(out).all()
    for i in range(6):
        dev = float(np.abs(out[i] - refs[i]).max() / max(1e-3, np.abs(refs[i]).max()))
        log(f"call_items {inst} item {i}: deviation {dev:.2e} of max(1e-3, max|ref|)")
        assert dev <= 2e-5, f"call_items {inst} item {i}: {dev:.2e}"
    return out


def check_no_item_loop(device, inst, ir_dir, comp_fn, monkeypatch):
    """with process() of the panner, Haas and both reverbs raising, call_items still completes, with the results of check_inst_chain"""
    from music_mixing_style_transfer_amd.mixing_manipulator import AlgorithmicReverb, ConvolutionalReverb, Haas, Panner

    def refuse(self, *a, **kw):
        raise AssertionError(f"{type(self).__name__}.process called from call_items: the per-item loop is back")

    for cls in (Panner, Haas, ConvolutionalReverb, AlgorithmicReverb):
        monkeypatch.setattr(cls, "process", refuse)
    assert _lib.lib().mst_version() >= 105
    check_inst_chain(device, inst, ir_dir, comp_fn, log=lambda s: None)
