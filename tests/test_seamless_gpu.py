"""Seam-free conversion (StyleTransferEngine.convert_stem_seamless, `style_transfer --seamless True`) on the MI355X.

1. the 6-block net (context 441 a side), L = 5000, windows of 1024, passes of 4000 samples: first and last window clipped, the three interior
   ones (1906 samples) as a batch of two and a batch of one; against the float64 oracle's WHOLE-sequence forward at the project's tolerances;
2. the default 14-block net (context 114681 a side), L = 300001, windows of 100000: four windows with inputs of 214681 (clipped on the left),
   300001 (the second window's context reaches past BOTH ends), 214682 and 114682 samples (clipped on the right; the last window keeps ONE
   output sample) - lengths that are multiples of nothing - against the single-item product forward [1, 2, 300001]; each of the two runs is
   within the precision's tolerance of the exact result, so they get the sum: fp32 2e-4, bf16 2e-2.  L = 430001 beside it has an interior
   window of 100000 + 2 * 114681 = 329362 samples;
3. a host stem (pinned, streamed on the copy streams) gives the bits of a device stem;
4. the command line: --seamless True writes what the engine call gives, within one 16-bit step; without the flag it writes the bytes of the
   segment path (convert_stem), whatever --seamless_window says;
5. --interpolation True --seamless True against the oracle run piece by piece by the same definition.
"""
import os
import wave

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
TOL_ORACLE = {"fp32": 1e-4, "bf16x3": 1e-4, "bf16": 1e-2}


def _cfgs(nblocks=None):
    with open(os.path.join(REPO, "music_mixing_style_transfer_amd", "networks", "configs.yaml")) as f:
        cfgs = yaml.full_load(f)
    enc, tcn = cfgs["Effects_Encoder"]["default"], dict(cfgs["TCN"]["default"])
    if nblocks is not None:
        tcn["nblocks"] = nblocks
    return enc, tcn


def _tcn(nblocks, seed):
    from music_mixing_style_transfer_amd import _lib
    from music_mixing_style_transfer_amd.networks import TCNModel
    from music_mixing_style_transfer_amd.utils import synth
    assert _lib.lib().path.endswith("libmst_hip.so") and _lib.lib().mst_version() >= 107
    sd = synth.tcn_state_dict(nblocks=nblocks, seed=seed)
    m = TCNModel(nparams=2048, ninputs=2, noutputs=2, nblocks=nblocks, dilation_growth=2, kernel_size=15, channel_width=128, stack_size=15,
                 cond_dim=2048, causal=False).to(DEV)
    m.load_state_dict(sd)
    return m.eval(), sd


def _engine(tcn, **kw):
    from music_mixing_style_transfer_amd.inference import StyleTransferEngine
    return StyleTransferEngine(None, tcn, **kw)


def _cond(seed=9):
    from music_mixing_style_transfer_amd.utils import synth
    return synth.synth_audio((2048,), seed=seed, key="cond")


@pytest.fixture(scope="module")
def six():
    """The 6-block case: (model, state dict, stem [2, 5000], condition [2048], the float64 oracle's whole-sequence forward)."""
    from music_mixing_style_transfer_amd.utils import synth
    from oracle import networks_ref as R
    m, sd = _tcn(6, seed=2)
    x, e = synth.synth_audio((2, 5000), seed=5), _cond()
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    whole64 = R.tcn_forward(sd64, x.double()[None], e.double()[None], nblocks=6)[0]
    return m, sd, x, e, whole64


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
def test_six_blocks_against_the_whole_sequence_oracle(six, precision):
    import ctypes as C
    from music_mixing_style_transfer_amd import _lib
    from music_mixing_style_transfer_amd.inference import segmentation as seg
    m, _, x, e, whole64 = six
    m.precision = precision
    assert m.context() == (441, 441)
    lib, left, right = _lib.lib(), C.c_long(-1), C.c_long(-1)
    m._ensure(lib)
    lib.check(lib.mst_tcn_context(m._handle, C.byref(left), C.byref(right)), "mst_tcn_context")
    assert (left.value, right.value) == (441, 441)
    eng = _engine(m, pass_samples=4000)
    plan = seg.plan_windows(5000, 1024, 441, 441)
    assert [hi - lo for _, _, lo, hi in plan] == [1465, 1906, 1906, 1906, 1345]
    assert eng._window_passes(plan, 0, 5, 1906) == [(0, 1), (1, 3), (3, 4), (4, 5)]          # a batch of two interior windows
    y, rng = eng.convert_stem_seamless(x.to(DEV), e.to(DEV), window=1024)
    whole = m(x[None].to(DEV), e[None].to(DEV))[0]
    d_y, d_w = float((y.cpu().double() - whole64).abs().max()), float((whole.cpu().double() - whole64).abs().max())
    print(f"seam-free, 6 blocks, L 5000, W 1024, {precision}: windowed vs oracle {d_y:.3e}, whole vs oracle {d_w:.3e}, "
          f"windowed vs whole {float((y - whole).abs().max()):.3e} (bit-identical: {torch.equal(y, whole)})")
    assert rng == (0, 5000) and y.is_cuda and tuple(y.shape) == (2, 5000)
    assert float(whole64.abs().max()) > 0.1
    assert d_y <= TOL_ORACLE[precision]
    assert d_w <= TOL_ORACLE[precision]


def test_host_stem_gives_the_bits_of_a_device_stem(six):
    m, _, x, e, _ = six
    m.precision = "fp32"
    eng = _engine(m, pass_samples=4000)
    y_dev, _ = eng.convert_stem_seamless(x.to(DEV), e.to(DEV), window=1024)
    y_host, rng = eng.convert_stem_seamless(x.pin_memory(), e.to(DEV), window=1024)
    assert rng == (0, 5000) and not y_host.is_cuda and y_host.is_pinned()
    assert torch.equal(y_host, y_dev.cpu())
    out = torch.zeros(2, 5000).pin_memory()
    y_out, _ = eng.convert_stem_seamless(x, e.to(DEV), window=1024, out=out)          # pageable stem, caller's buffer
    assert y_out is out and torch.equal(out, y_host)


@pytest.fixture(scope="module")
def default_net():
    from music_mixing_style_transfer_amd.utils import synth
    m, _ = _tcn(14, seed=0)
    return m, synth.synth_audio((2, 430001), seed=5).to(DEV), _cond().to(DEV)


# (L, the window inputs' lengths): 300001 is the case of the file's header; 430001 adds an INTERIOR window, 329362 = W + 2 * 114681 samples
DEFAULT_NET_CASES = [(300001, [214681, 300001, 214682, 114682]), (430001, [214681, 314681, 329362, 244682, 144682])]


@pytest.mark.parametrize("precision,tol", [("fp32", 2e-4), ("bf16", 2e-2)])
@pytest.mark.parametrize("length,lengths", DEFAULT_NET_CASES)
def test_default_net_windows_clipped_at_both_ends(default_net, length, lengths, precision, tol):
    from music_mixing_style_transfer_amd.inference import segmentation as seg
    m, x, e = default_net
    x = x[:, :length].contiguous()
    m.precision = precision
    assert m.context() == (114681, 114681)
    plan = seg.plan_windows(length, 100000, 114681, 114681)
    assert [hi - lo for _, _, lo, hi in plan] == lengths and plan[-1][:2] == (100000 * (len(lengths) - 1), length)
    y, rng = _engine(m).convert_stem_seamless(x, e, window=100000)
    whole = m(x[None], e[None])[0]
    d = float((y - whole).abs().max())
    print(f"seam-free, default net, L {length}, W 100000, {precision}: windowed vs single-item forward {d:.3e} "
          f"(bit-identical: {torch.equal(y, whole)}), max|y| {float(whole.abs().max()):.3f}")
    assert rng == (0, length) and float(whole.abs().max()) > 0.1
    assert d <= tol


STEMS = ["drums", "bass"]
SEG, L_IN, L_REF, WIN = 16384, 40000, 50000, 8192


def _write_wav(path, x):
    pcm = np.clip(np.rint(x.T * 32767), -32768, 32767).astype("<i2")
    with wave.open(str(path), "w") as w:
        w.setnchannels(2)
        w.setsampwidth(2)
        w.setframerate(44100)
        w.writeframes(pcm.tobytes())


def _read_pcm(path):
    with wave.open(str(path)) as w:
        assert w.getnchannels() == 2 and w.getsampwidth() == 2
        return np.frombuffer(w.readframes(w.getnframes()), dtype="<i2").reshape(-1, 2).T.astype(np.int64)


@pytest.fixture(scope="module")
def song(tmp_path_factory):
    """Synthetic stems (input, reference, reference_B) and reference-format checkpoints of the default encoder and a 6-block converter."""
    from music_mixing_style_transfer_amd.utils import synth
    root = tmp_path_factory.mktemp("seamless")
    enc_cfg, _ = _cfgs()
    sds = synth.fxencoder_state_dict(enc_cfg, seed=0), synth.tcn_state_dict(nblocks=6, seed=2)
    synth.save_reference_format_checkpoint(str(root / "enc.pt"), sds[0])
    synth.save_reference_format_checkpoint(str(root / "tcn.pt"), sds[1])
    for kind, L, off in (("input", L_IN, 0), ("reference", L_REF, 3), ("reference_B", L_REF - 5000, 6)):
        d = root / "data" / "song0" / "separated" / kind
        d.mkdir(parents=True)
        for k, s in enumerate(STEMS):
            _write_wav(d / (s + ".wav"), synth.synth_music(2, L, seed=10 * k + off).numpy())
    return root, sds


def _runner(root, out, extra):
    from music_mixing_style_transfer_amd.inference import style_transfer as st
    args = st.build_parser().parse_args([
        "--target_dir", str(root / "data") + "/", "--output_dir", str(root / out) + "/", "--ckpt_path_enc", str(root / "enc.pt"),
        "--ckpt_path_conv", str(root / "tcn.pt"), "--do_not_separate", "True", "--normalize_input", "False", "--segment_length", str(SEG),
        "--segment_length_ref", str(SEG), "--save_each_inst", "True"] + extra)
    args.instruments = list(STEMS)
    args.cfg_encoder, args.cfg_converter = _cfgs(nblocks=6)
    return st.Mixing_Style_Transfer_Inference(args)


def _stem(root, kind, s):
    from music_mixing_style_transfer_amd.data_loader import load_wav_device
    wav = load_wav_device(str(root / "data" / "song0" / "separated" / kind / (s + ".wav")), torch.device(DEV))
    return torch.clamp(wav.float(), min=-1, max=1)          # what the runner's dataset hands the engine


def test_cli_seamless_writes_what_the_engine_gives_and_default_is_the_segment_path(song):
    root, _ = song
    run = _runner(root, "out_on", ["--seamless", "True", "--seamless_window", str(WIN)])
    run.inference()
    txt = open(root / "out_on" / "style_transfer_inference_configurations.txt").read()
    assert "- seamless            : True" in txt and f"- seamless_window     : {WIN}" in txt
    eng = run._engine()
    names = [f"{s}_output_notnormed.wav" for s in STEMS] + ["mixture_output_notnormed.wav"]
    assert sorted(os.listdir(root / "out_on" / "song0")) == sorted(names)
    on, off = [], []
    for s in STEMS:
        x, r = _stem(root, "input", s), _stem(root, "reference", s)
        on.append(eng.transfer_stem(x, r, SEG, SEG, "song0", seamless=True, window=WIN))
        off.append(eng.transfer_stem(x, r, SEG, SEG, "song0"))
        emb = eng.stem_embedding(r, SEG, SEG, "song0")
        assert torch.equal(off[-1], eng.convert_stem(x, emb, SEG, "song0")[0])
        assert torch.equal(on[-1], eng.convert_stem_seamless(x, emb, window=WIN)[0])
        assert float((on[-1] - off[-1]).abs().max()) > 1e-3          # the two modes are different audio
    for name, y in zip(names, on + [sum(on)]):
        pcm = _read_pcm(root / "out_on" / "song0" / name)
        assert pcm.shape == (2, L_IN)
        assert np.abs(pcm - y.cpu().double().numpy() * 32767.0).max() <= 1.0, name          # one 16-bit step
    # without --seamless (the window flag alone changes nothing): the bytes of the segment path
    from music_mixing_style_transfer_amd.data_loader import pcm16_device, save_wav_pcm16
    _runner(root, "out_off", ["--seamless_window", str(WIN)]).inference()
    for name, y in zip(names, off + [sum(off)]):
        want = str(root / ("want_" + name))
        save_wav_pcm16(want, pcm16_device(y.transpose(-1, -2).contiguous()).cpu().numpy(), 44100)
        assert open(root / "out_off" / "song0" / name, "rb").read() == open(want, "rb").read(), name


def test_cli_interpolation_seamless_against_the_per_piece_oracle(song):
    """Piece k of L // S + 1 samples is window k of the stem: the oracle runs samples [lo, hi) of the plan under piece k's blend of the two
    reference embeddings and keeps [a, b).  fp32: 1e-4 on the waveform, plus one 16-bit step of the written file."""
    from music_mixing_style_transfer_amd.data_loader import load_wav_segment
    from music_mixing_style_transfer_amd.inference import segmentation as seg
    from oracle import networks_ref as R
    from oracle import segmentation_ref as O
    root, (enc_sd, tcn_sd) = song
    enc_cfg, _ = _cfgs()
    S = 4
    _runner(root, "out_interp", ["--seamless", "True", "--interpolation", "True", "--interpolate_segments", str(S)]).inference_interpolation()
    mix = load_wav_segment(str(root / "out_interp" / "song0" / "mixture_output_notnormed_interpolation.wav"), axis=0)
    piece = L_IN // S + 1
    plan = seg.plan_windows(L_IN, piece, 441, 441)
    assert len(plan) == S
    ref_mix = 0
    for s in STEMS:
        rd = lambda kind: np.clip(load_wav_segment(str(root / "data" / "song0" / "separated" / kind / (s + ".wav")), axis=0), -1, 1).astype(np.float32)
        xin, emb = torch.from_numpy(rd("input")), {}
        for name, kind in (("a", "reference"), ("b", "reference_B")):
            batches = O.batchwise_segmentization(rd(kind), SEG, 1, SEG)
            emb[name] = torch.from_numpy(O.mean_embedding([R.fxencoder_forward(enc_sd, enc_cfg, torch.from_numpy(b)).numpy() for b in batches]))
        y = torch.empty(2, L_IN)
        for k, (a, b, lo, hi) in enumerate(plan):
            w = (S - 1 - k) / (S - 1)
            y[:, a:b] = R.tcn_forward(tcn_sd, xin[None, :, lo:hi], (w * emb["a"] + (1 - w) * emb["b"])[None], nblocks=6)[0][:, a - lo:a - lo + (b - a)]
        ref_mix = ref_mix + y.numpy()
    assert mix.shape == (2, L_IN)
    d = float(np.abs(mix - np.clip(ref_mix, -1, 1)).max())
    print(f"--interpolation --seamless, 6 blocks, fp32: mixture vs the per-piece oracle {d:.3e}")
    assert d <= 1e-4 + 1.0 / 32767
