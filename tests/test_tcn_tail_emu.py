"""The last three bf16 TCN blocks as one launch (mst_tcn_set_fusion bit 0, tcn_tail_bf16_kernel), on the SIMT emulator.

Where the last three blocks of a full bf16 forward are the whole-sequence 256-time forms of four, eight and sixteen phases at dilations
d, 2d, 4d (L = 64 d) their tiles are the same samples, and one launch runs all three with the two activations between them kept in LDS.
The fused launch has to give the BITS of the three launches (same products, same fp32 order), has to run exactly where the conditions hold,
and has to leave every other launch table alone - a raw mst_tcn_create handle's included (tests/test_tcn_launch_plan.py pins those).

Shapes: the smallest that reach every path.  Five blocks at L = 256 (d = 4, 8, 16): B tiles, no multiple of 8 - the plain tile order.
Eight blocks at L = 2048 (d = 32, 64, 128): 8 B tiles - the XCD tile order.  B = 1 with one FiLM row; B = 3 with a row per item and with the
list-of-conditions branch.  tcn_block_ref.make_input puts digital silence and +-full-scale items (or stretches, B = 1) into every case.
"""
import ctypes as C
import re

import pytest
import torch

from tcn_block_ref import PlanTracer, make_cond, make_input

TCN_KERNEL = re.compile(r"^_Z\d+tcn_(block|block0|output|unpack|tail)_")
TAIL = "_Z20tcn_tail_bf16_kernel11TcnTailArgs"
COND_DIM = 64


def _tcn(nblocks, growth=2, seed=0):
    from music_mixing_style_transfer_amd.networks import TCNModel
    from music_mixing_style_transfer_amd.utils import synth
    sd = synth.tcn_state_dict(nblocks=nblocks, cond_dim=COND_DIM, seed=seed)
    m = TCNModel(nparams=COND_DIM, ninputs=2, noutputs=2, nblocks=nblocks, dilation_growth=growth, kernel_size=15,
                 channel_width=128, stack_size=15, cond_dim=COND_DIM, causal=False)
    m.load_state_dict(sd)
    m.precision = "bf16"
    return m


def _trace(emu, call):
    """(kernel symbol, grid x, y, z, block x) of every TCN kernel `call` launches; a dry run: no kernel body runs."""
    begin, end = emu.cdll.emu_trace_begin, emu.cdll.emu_trace_end
    begin.restype, end.restype, end.argtypes = None, C.c_long, [C.c_char_p, C.c_long]
    text = C.create_string_buffer(1 << 16)
    begin()
    try:
        call()
    finally:
        n = end(text, len(text))
    assert n < len(text)
    return [(f[0],) + tuple(int(v) for v in f[1:]) for f in (ln.split() for ln in text.value.decode().splitlines()) if TCN_KERNEL.match(f[0])]


def _fusion(emu, m):
    fl, ran = C.c_int(-1), C.c_int(-1)
    emu.check(emu.mst_tcn_get_fusion(m._handle, C.byref(fl), C.byref(ran)), "get_fusion")
    return fl.value, ran.value


def _set_fusion(emu, m, flags):
    emu.check(emu.mst_tcn_set_fusion(m._handle, flags), "set_fusion")


@pytest.mark.parametrize("nblocks,L,B,film", [(5, 256, 1, "1"), (5, 256, 3, "B"), (5, 256, 3, "list"), (8, 2048, 1, "1"), (8, 2048, 3, "B")])
def test_fused_tail_gives_the_bits_of_the_three_launches(emu_default, nblocks, L, B, film):
    from music_mixing_style_transfer_amd import _lib
    emu = emu_default
    m = _tcn(nblocks)
    x = make_input(B, L, seed=100 + nblocks)
    cond = make_cond(film, B, COND_DIM, nblocks, seed=7)
    m._ensure(emu)
    assert _lib.TCN_FUSION_DEFAULT == 1 and _fusion(emu, m)[0] == 1          # what TCNModel sets on its handle
    _set_fusion(emu, m, 0)
    y0 = m(x, cond)
    assert _fusion(emu, m) == (0, 0)
    t0 = _trace(emu, lambda: m(x, cond))
    _set_fusion(emu, m, 1)
    y1 = m(x, cond)
    assert _fusion(emu, m) == (1, 1)
    t1 = _trace(emu, lambda: m(x, cond))
    assert torch.equal(y1, y0)
    assert float(y0.abs().max()) > 0.0
    # one launch per block in front (block 0 rides in block 1's launch under the default tuning), then the tail on the four-phase block's grid
    d = 2 ** (nblocks - 3)
    assert len(t0) == nblocks - 1 and all(TAIL not in ln[0] for ln in t0)
    assert t0[-3][1:] == (B * d // 4, 1, 1, 256)
    assert t1 == t0[:-3] + [(TAIL,) + t0[-3][1:]]
    assert len(t1) - 1 == nblocks - 3 - 1


def test_tail_is_not_fused_where_the_conditions_do_not_hold(emu_default):
    """The launch table with fusion 1 IS the table with fusion 0: a step under in L, a ragged length, tuning without bit 7, the other precisions,
    the probe entry point, a net of three blocks."""
    from music_mixing_style_transfer_amd import _lib
    emu = emu_default
    cond = make_cond("1", 1, COND_DIM, 5, seed=7)
    cases = [(5, 255, 245, "bf16", None), (5, 250, 245, "bf16", None), (5, 256, 117, "bf16", None), (5, 256, 245, "fp32", None),
             (5, 256, 245, "bf16x3", None), (5, 256, 245, "bf16", 5), (3, 256, 245, "bf16", None), (3, 64, 245, "bf16", None)]
    models = {}
    for nblocks, L, tuning, prec, n_run in cases:
        m = models.setdefault(nblocks, _tcn(nblocks))
        m.precision = prec
        m._ensure(emu)
        emu.check(emu.mst_tcn_set_tuning(m._handle, tuning), "set_tuning")
        x = make_input(1, L, seed=3)
        run = (lambda: m(x, cond)) if n_run is None else (lambda: m.forward_blocks(x, cond, n_run))
        traces = {}
        for fusion in (0, 1):
            _set_fusion(emu, m, fusion)
            traces[fusion] = _trace(emu, run)
            assert _fusion(emu, m) == (fusion, 0), (nblocks, L, tuning, prec, n_run)
        assert traces[1] == traces[0] and traces[0], (nblocks, L, tuning, prec, n_run)
        assert all(TAIL not in ln[0] for ln in traces[1])
        emu.check(emu.mst_tcn_set_tuning(m._handle, _lib.TCN_TUNING_DEFAULT), "set_tuning")


def test_fusion_flags_and_the_raw_handle(emu):
    """Bits beyond bit 0 are refused; a handle from mst_tcn_create starts with fusion 0 and launches one kernel per block until it is asked."""
    tr = PlanTracer(emu)
    try:
        dil = (1, 2, 4, 8, 16)
        h = tr._handle(dil)
        fl, ran = C.c_int(-1), C.c_int(-1)
        emu.check(emu.mst_tcn_get_fusion(h, C.byref(fl), C.byref(ran)), "get_fusion")
        assert (fl.value, ran.value) == (0, 0)
        for bad in (2, 3, -1, 256):
            assert emu.mst_tcn_set_fusion(h, bad) != 0
        emu.check(emu.mst_tcn_get_fusion(h, C.byref(fl), None), "get_fusion")
        assert fl.value == 0
        assert emu.mst_tcn_set_fusion(None, 1) != 0 and emu.mst_tcn_get_fusion(None, None, None) != 0
        raw = tr.launches(dil, 245, 1, 256, "bf16")
        assert len(raw) == 4
        emu.check(emu.mst_tcn_get_fusion(h, None, C.byref(ran)), "get_fusion")
        assert ran.value == 0
        emu.check(emu.mst_tcn_set_fusion(h, 1), "set_fusion")
        assert tr.launches(dil, 245, 1, 256, "bf16") == raw[:-3]          # (PlanTracer keeps the pinned kernel families only: the tail is not one)
        emu.check(emu.mst_tcn_get_fusion(h, None, C.byref(ran)), "get_fusion")
        assert ran.value == 1
        emu.check(emu.mst_tcn_set_fusion(h, 0), "set_fusion")
    finally:
        tr.close()


def test_timing_hook_shares_the_fused_launch_among_its_blocks(emu_default):
    emu = emu_default
    nblocks = 5
    m = _tcn(nblocks)
    x, cond = make_input(1, 256, seed=5), make_cond("1", 1, COND_DIM, nblocks, seed=7)
    m._ensure(emu)
    emu.check(emu.mst_tcn_timing_begin(m._handle, 1), "timing_begin")
    m(x, cond)
    ms, nf = (C.c_float * (nblocks + 1))(), C.c_int(0)
    emu.check(emu.mst_tcn_timing_end(m._handle, ms, C.byref(nf)), "timing_end")
    assert nf.value == 1 and _fusion(emu, m) == (1, 1)
    assert ms[2] == ms[3] == ms[4] and ms[2] > 0.0
