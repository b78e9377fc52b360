"""Seam-free conversion (StyleTransferEngine.convert_stem_seamless) on the SIMT emulator build of the kernels, gloo for the two-rank run.

The case: the 3-block net (context 49 samples a side), a stem of 2300 samples, windows of 512 -> five windows: the first clipped on the left
(561 samples), three interior ones of 610, the last clipped on the right (301).  pass_samples = 1300 holds two interior windows, so the
interior ones run as a batch of two and a batch of one.  Two ranks own windows [0, 2) and [2, 5): uneven shards, and rank 1's batches are cut
differently from the single process's.

Tolerances: a windowed run and the whole-sequence product forward each sit within the project's tolerance of the float64 oracle (fp32 and
bf16x3 1e-4, bf16 1e-2), so against each other they get the sum, 2e-4 / 2e-4 / 2e-2; both are also held to the oracle directly.
(A host stem against a device stem needs a device: tests/test_seamless_gpu.py.)
"""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COND = 64
L, W, PASS = 2300, 512, 1300
TOL_ORACLE = {"fp32": 1e-4, "bf16x3": 1e-4, "bf16": 1e-2}


def _tcn(nblocks=3, causal=False, precision="fp32"):
    from music_mixing_style_transfer_amd.networks import TCNModel
    from music_mixing_style_transfer_amd.utils import synth
    m = TCNModel(nparams=COND, ninputs=2, noutputs=2, nblocks=nblocks, dilation_growth=2, kernel_size=15, channel_width=128, stack_size=15,
                 cond_dim=COND, causal=causal)
    sd = synth.tcn_state_dict(nblocks=nblocks, cond_dim=COND, seed=2)
    m.load_state_dict(sd)
    m.precision = precision
    return m.eval(), sd


def _engine(tcn, pass_samples=PASS):
    from music_mixing_style_transfer_amd.inference import StyleTransferEngine
    return StyleTransferEngine(None, tcn, pass_samples=pass_samples)


def _stem():
    from music_mixing_style_transfer_amd.utils import synth
    return synth.synth_audio((2, L), seed=5)


def _cond(seed=9):
    from music_mixing_style_transfer_amd.utils import synth
    return synth.synth_audio((COND,), seed=seed, key="cond")


def _oracle64(sd, x, e, nblocks=3):
    from oracle import networks_ref as R
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    return R.tcn_forward(sd64, x.double()[None], e.double()[None], nblocks=nblocks)[0]


@pytest.fixture(scope="module")
def whole64():
    """The float64 oracle's whole-sequence forward of the case: computed once, read by every test that needs it."""
    _, sd = _tcn()
    return _oracle64(sd, _stem(), _cond())


def test_context_entry_point(emu_default):
    emu = emu_default
    assert emu.mst_version() >= 107
    left, right = C.c_long(-1), C.c_long(-1)
    for causal, want in ((False, (49, 49)), (True, (98, 0))):
        m, _ = _tcn(causal=causal)
        m._ensure(emu)
        emu.check(emu.mst_tcn_context(m._handle, C.byref(left), C.byref(right)), "mst_tcn_context")
        assert (left.value, right.value) == want == m.context()
        emu.check(emu.mst_tcn_context(m._handle, None, C.byref(right)), "mst_tcn_context")
        emu.check(emu.mst_tcn_context(m._handle, C.byref(left), None), "mst_tcn_context")
    assert emu.mst_tcn_context(None, C.byref(left), C.byref(right)) == -1 and b"null handle" in emu.mst_last_error()


def test_the_case_is_what_the_header_says(emu_default):
    from music_mixing_style_transfer_amd.inference import segmentation as seg
    m, _ = _tcn()
    plan = seg.plan_windows(L, W, *m.context())
    assert [hi - lo for _, _, lo, hi in plan] == [561, 610, 610, 610, 301]
    assert _engine(m)._window_passes(plan, 0, 5, 610) == [(0, 1), (1, 3), (3, 4), (4, 5)]
    assert _engine(m)._window_passes(plan, 2, 5, 610) == [(2, 4), (4, 5)]
    assert [seg.shard_range(5, r, 2) for r in range(2)] == [(0, 2), (2, 5)]


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "bf16"])
def test_windowed_equals_whole_sequence(emu_default, whole64, precision):
    m, _ = _tcn(precision=precision)
    x, e = _stem(), _cond()
    whole = m(x[None], e[None])[0]
    y, rng = _engine(m).convert_stem_seamless(x, e, window=W)
    assert rng == (0, L) and tuple(y.shape) == (2, L)
    d = float((y - whole).abs().max())
    d_y, d_w = float((y.double() - whole64).abs().max()), float((whole.double() - whole64).abs().max())
    print(f"seam-free on the emulator, {precision}: windowed vs whole {d:.3e} (bit-identical: {torch.equal(y, whole)}), "
          f"windowed vs oracle {d_y:.3e}, whole vs oracle {d_w:.3e}")
    assert float(whole64.abs().max()) > 0.1
    assert d_w <= TOL_ORACLE[precision] and d_y <= TOL_ORACLE[precision]
    assert d <= 2 * TOL_ORACLE[precision]
    if precision != "bf16":          # (the emulator's fp32 and split-bf16 matrix instructions are slow: the plumbing below once, in bf16)
        return
    # one window for the whole stem is the whole-sequence forward itself
    y1, rng1 = _engine(m, pass_samples=1 << 23).convert_stem_seamless(x, e, window=L)
    assert rng1 == (0, L) and torch.equal(y1, whole)
    # `out` is filled and returned
    out = torch.full((2, L), 7.0)
    y2, _ = _engine(m).convert_stem_seamless(x, e, window=W, out=out)
    assert y2 is out and torch.equal(out, y)


def test_causal_net_on_the_generic_path(emu_default):
    """All the context on the left: windows [a - 98, b), only the first one clipped.  Symmetric halos would be 49 samples short on the left."""
    from music_mixing_style_transfer_amd.inference import segmentation as seg
    m, _ = _tcn(causal=True)
    assert m.context() == (98, 0)
    plan = seg.plan_windows(L, W, 98, 0)
    assert [hi - lo for _, _, lo, hi in plan] == [512, 610, 610, 610, 350]
    x, e = _stem(), _cond()
    whole = m(x[None], e[None])[0]
    y, rng = _engine(m).convert_stem_seamless(x, e, window=W)
    d = float((y - whole).abs().max())
    print(f"seam-free on the emulator, causal net: windowed vs whole {d:.3e} (bit-identical: {torch.equal(y, whole)})")
    assert rng == (0, L) and float(whole.abs().max()) > 0.1
    assert d <= 2e-4


def test_one_film_row_per_window(emu_default):
    """embedding = callable: window i runs, halo included, under condition i.  Against the float64 oracle run window by window by the same
    definition.  (bf16x3: the project's 1e-4 holds for it as for fp32, at a third of fp32's time on the emulator.)"""
    from music_mixing_style_transfer_amd.inference import segmentation as seg
    m, sd = _tcn(precision="bf16x3")
    x = _stem()
    conds = [_cond(seed=20 + i) for i in range(5)]
    asked = []
    y, _ = _engine(m).convert_stem_seamless(x, lambda i: (asked.append(i), conds[i])[1], window=W)
    assert asked == [0, 1, 2, 3, 4]
    want = torch.empty(2, L, dtype=torch.float64)
    for i, (a, b, lo, hi) in enumerate(seg.plan_windows(L, W, *m.context())):
        want[:, a:b] = _oracle64(sd, x[:, lo:hi], conds[i])[:, a - lo:a - lo + (b - a)]
    d = float((y.double() - want).abs().max())
    print(f"seam-free on the emulator, one condition per window: vs the per-window oracle {d:.3e}")
    assert d <= 1e-4
    one = torch.cat([_oracle64(sd, x[:, lo:hi], conds[0])[:, a - lo:a - lo + (b - a)] for a, b, lo, hi in seg.plan_windows(L, W, *m.context())], -1)
    assert float((one - want).abs().max()) > 1e-2          # (the conditions differ audibly: a run that gave every window condition 0 fails above)


def test_window_larger_than_a_pass(emu_default):
    m, _ = _tcn(precision="bf16")
    with pytest.raises(ValueError, match=r"window of 512 samples .* 49 \+ 49 samples is 610 samples, more than one pass of 609 samples"):
        _engine(m, pass_samples=609).convert_stem_seamless(_stem(), _cond(), window=W)
    y, _ = _engine(m, pass_samples=610).convert_stem_seamless(_stem(), _cond(), window=W)          # exactly one interior window per pass
    assert torch.equal(y, _engine(m).convert_stem_seamless(_stem(), _cond(), window=W)[0])
    with pytest.raises(ValueError, match="window"):
        _engine(m).convert_stem_seamless(_stem(), _cond(), window=0)


def test_only_tcn_kernels_launch(emu_default):
    """Dry-run launch trace of a seam-free call: FiLM table, block kernels, output head - nothing else of the library; one forward per pass."""
    emu = emu_default
    m, _ = _tcn(precision="bf16")
    x, e = _stem(), _cond()
    m(x[None], e[None])                              # (handle and weights exist before the trace)
    begin, end = emu.cdll.emu_trace_begin, emu.cdll.emu_trace_end
    begin.restype, end.restype, end.argtypes = None, C.c_long, [C.c_char_p, C.c_long]
    text = C.create_string_buffer(1 << 16)
    begin()
    try:
        _engine(m).convert_stem_seamless(x, e, window=W)
    finally:
        n = end(text, len(text))
    assert n < len(text)
    names = [ln.split()[0] for ln in text.value.decode().splitlines()]
    assert names and all("tcn_" in k for k in names), sorted(set(names))
    assert sum("tcn_film_kernel" in k for k in names) == 4          # four passes: 1 + 2 + 1 + 1 windows


def _worker(rank, world, port, out_path):
    sys.path.insert(0, REPO)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), MST_EMU_THREADS="2")
    torch.set_num_threads(1)
    from music_mixing_style_transfer_amd import _lib
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from emu_binding import bind_emulator
    _lib.set_default_binding(bind_emulator(build=False))
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    m, _ = _tcn(precision="bf16")          # (the emulator's fp32 matrix instruction is several times slower; the plumbing under test is the same)
    eng = _engine(m)
    x, e = _stem(), _cond()
    runs = [eng.convert_stem_seamless(x, e, window=W) for _ in range(2)]
    assert runs[0][1] == runs[1][1] and torch.equal(runs[0][0], runs[1][0])          # identical on repetition
    y, rng = runs[0]
    if world == 1:
        torch.save({"full": y, "ranges": [rng]}, out_path)
    else:
        ranges = [None] * world
        dist.all_gather_object(ranges, tuple(rng))
        full = eng.gather_stem(y, rng, L)
        if rank == 0:
            torch.save({"full": full, "ranges": ranges}, out_path)
        dist.destroy_process_group()


def test_two_ranks_equal_one(tmp_path, emu):
    from music_mixing_style_transfer_amd import _lib
    one, two = str(tmp_path / "one.pt"), str(tmp_path / "two.pt")
    prev = _lib._default
    try:
        _worker(0, 1, 0, one)
    finally:
        _lib.set_default_binding(prev)
    mp.spawn(_worker, args=(2, 29701, two), nprocs=2, join=True)
    a, b = torch.load(one, weights_only=False), torch.load(two, weights_only=False)
    assert a["ranges"] == [(0, L)] and b["ranges"] == [(0, 2 * W), (2 * W, L)]
    assert torch.equal(a["full"], b["full"])


def _runner(tcn, enc, out_dir, **over):
    import types
    from music_mixing_style_transfer_amd.inference import style_transfer as st
    runner = object.__new__(st.Mixing_Style_Transfer_Inference)
    runner.args = types.SimpleNamespace(normalize_input=False, instruments=["drums"], segment_length=512, segment_length_ref=512,
                                        batch_size=1, save_each_inst=True, sample_rate=44100, interpolate_segments=5, **over)
    runner.device = torch.device("cpu")
    runner.target_dir, runner.output_dir = "/data/", str(out_dir) + "/"
    runner.models = {"effects_encoder": enc, "mixing_converter": tcn}
    return runner


def test_runner_flags_route_and_default_off(tmp_path, emu_default):
    """The runner's inference() and inference_interpolation(): with `seamless` the stems go through convert_stem_seamless (window =
    --seamless_window, or the interpolation piece with one condition per piece); without the attribute the segment path runs as before.
    Same file names, different audio.  (One stem, bf16: the emulator's fast mode; what the files hold is checked on the GPU.)"""
    from test_distributed_gloo import _models
    from music_mixing_style_transfer_amd.data_loader import load_wav_segment
    from music_mixing_style_transfer_amd.inference import StyleTransferEngine
    from music_mixing_style_transfer_amd.inference import style_transfer as st
    from music_mixing_style_transfer_amd.utils import synth
    p = st.build_parser()
    assert p.parse_args([]).seamless is False and p.parse_args([]).seamless_window == 2 ** 21
    ns = p.parse_args(["--seamless", "True", "--seamless_window", "4096"])
    assert ns.seamless is True and ns.seamless_window == 4096
    inference_args = next(g for g in p._action_groups if g.title == "Inference args")          # what save_args records
    assert {"seamless", "seamless_window"} <= {act.dest for act in inference_args._group_actions}
    enc, tcn = _models()
    enc.precision = tcn.precision = "bf16"
    stem = lambda seed, n: synth.synth_audio((2, n), seed=seed)[None]
    calls, plain = [], StyleTransferEngine.convert_stem_seamless

    def recording(self, input_stem, embedding, window=None, out=None):
        calls.append((window, callable(embedding)))
        return plain(self, input_stem, embedding, window=window, out=out)
    StyleTransferEngine.convert_stem_seamless = recording
    try:
        wavs = {}
        for tag, over in (("plain", {}), ("on", {"seamless": True, "seamless_window": W})):
            runner = _runner(tcn, enc, tmp_path / tag, **over)
            runner.data_loader = [(stem(5, L), stem(6, 1100), "/data/song/")]
            runner.inference()
            d = tmp_path / tag / "song"
            assert sorted(os.listdir(d)) == ["drums_output_notnormed.wav", "mixture_output_notnormed.wav"]
            wavs[tag] = load_wav_segment(str(d / "drums_output_notnormed.wav"), axis=0)
        assert calls == [(W, False)]
        assert wavs["on"].shape == wavs["plain"].shape == (2, L) and abs(wavs["on"] - wavs["plain"]).max() > 1e-3
        runner = _runner(tcn, enc, tmp_path / "interp", seamless=True, seamless_window=4096)
        runner.data_loader = [(stem(5, L), stem(6, 1100), stem(16, 512 - 30), "/data/song/")]
        runner.inference_interpolation()
        assert calls[1:] == [(L // 5 + 1, True)]          # the piece is the window, one condition per piece
        d = tmp_path / "interp" / "song"
        assert sorted(os.listdir(d)) == ["drums_output_notnormed_interpolation.wav", "mixture_output_notnormed_interpolation.wav"]
        assert load_wav_segment(str(d / "drums_output_notnormed_interpolation.wav"), axis=0).shape == (2, L)
    finally:
        StyleTransferEngine.convert_stem_seamless = plain


