"""The bf16 TCN forward over chunks of the batch (mst_tcn_set_chunk / mst_tcn_get_chunk), on the SIMT emulator.

A chunked forward runs, per chunk of c items, the launch table of a c-item batch - the same kernels, grids and tile order, the fused tail
where it qualifies - with x, y and the per-item FiLM rows offset by the chunk, every chunk of a chain on the same two activations.  Items are
independent through the whole net, so the output has to have the BITS of the whole-batch forward, and the launch trace has to be the
chunk-sized table repeated ceil(B / c) times, the last, short chunk with its own grids.  Automatic (0) leaves every shape here alone: the rule
asks for one activation larger than the 256 MiB Infinity Cache.

Shapes: those of tests/test_tcn_tail_emu.py.  Five blocks at L = 256: tile counts that are no multiple of 8, the plain tile order.  Eight
blocks at L = 2048: 8 tiles per item, the XCD tile order.  Both end in a qualifying tail.  B = 5: chunks of 1 (five, two chains), of 2 (2 + 2
+ 1: a short last chunk) and of 5 (no chunking), with a FiLM row per item and with one shared row.
"""
import ctypes as C
import re

import pytest
import torch

from tcn_block_ref import make_cond, make_input

TCN_KERNEL = re.compile(r"^_Z\d+tcn_(block|block0|output|unpack|tail)_")
TAIL = "_Z20tcn_tail_bf16_kernel11TcnTailArgs"
COND_DIM = 64
B = 5


def _tcn(nblocks, seed=0):
    from music_mixing_style_transfer_amd.networks import TCNModel
    from music_mixing_style_transfer_amd.utils import synth
    sd = synth.tcn_state_dict(nblocks=nblocks, cond_dim=COND_DIM, seed=seed)
    m = TCNModel(nparams=COND_DIM, ninputs=2, noutputs=2, nblocks=nblocks, dilation_growth=2, kernel_size=15, channel_width=128,
                 stack_size=15, cond_dim=COND_DIM, causal=False)
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


def _chunk(emu, m):
    items, ran = C.c_int(-1), C.c_int(-1)
    emu.check(emu.mst_tcn_get_chunk(m._handle, C.byref(items), C.byref(ran)), "get_chunk")
    return items.value, ran.value


def _set_chunk(emu, m, items):
    emu.check(emu.mst_tcn_set_chunk(m._handle, items), "set_chunk")


@pytest.mark.parametrize("nblocks,L,film", [(5, 256, "B"), (5, 256, "1"), (8, 2048, "B"), (8, 2048, "1")])
def test_chunked_forward_has_the_bits_and_the_launches_of_the_chunk_sized_tables(emu_default, nblocks, L, film):
    from music_mixing_style_transfer_amd import _lib
    emu = emu_default
    m = _tcn(nblocks)
    x = make_input(B, L, seed=200 + nblocks)
    cond = make_cond(film, B, COND_DIM, nblocks, seed=11)
    m._ensure(emu)
    assert _lib.TCN_CHUNK_DEFAULT == 0 and _chunk(emu, m)[0] == 0          # what TCNModel sets on its handle: automatic
    y0 = m(x, cond)
    assert _chunk(emu, m) == (0, 1)                                        # automatic: far below the threshold, the whole batch
    assert float(y0.abs().max()) > 0.0 and not torch.equal(y0[1], y0[2])
    t0 = _trace(emu, lambda: m(x, cond))
    # the unchunked table of an n-item batch, n = 1 .. B: what a chunk of n items has to launch
    _set_chunk(emu, m, _lib.TCN_CHUNK_WHOLE)
    table = {n: _trace(emu, lambda: m(x[:n], cond if film == "1" else cond[:n])) for n in (1, 2, B)}
    assert _chunk(emu, m) == (_lib.TCN_CHUNK_WHOLE, 1)
    assert t0 == table[B] and t0[-1][0] == TAIL and len(t0) == nblocks - 3          # chunk 0 left the trace untouched; the tail qualifies
    assert table[1] != table[2] != table[B]                                         # (the grids depend on the batch: the check below can fail)
    for c in (1, 2, B):
        _set_chunk(emu, m, c)
        y = m(x, cond)
        chunks = -(-B // c)
        assert _chunk(emu, m) == (c, chunks), c
        assert torch.equal(y, y0), (c, float((y - y0).abs().max()))
        want = []
        for k in range(chunks):
            want += table[min(c, B - k * c)]
        assert _trace(emu, lambda: m(x, cond)) == want, c
    # the other precisions and the probe keep the whole batch whatever is set
    _set_chunk(emu, m, 2)
    whole = {}
    for prec, n_run in (("fp32", None), ("bf16x3", None), ("bf16", nblocks)):
        m.precision = prec
        run = (lambda: m(x, cond)) if n_run is None else (lambda: m.forward_blocks(x, cond, n_run))
        whole[2] = _trace(emu, run)
        assert _chunk(emu, m) == (2, 1), prec
        _set_chunk(emu, m, _lib.TCN_CHUNK_WHOLE)
        whole[0] = _trace(emu, run)
        _set_chunk(emu, m, 2)
        assert whole[2] == whole[0] and whole[0], (prec, n_run)


def test_chunk_refusals_and_the_raw_handle(emu):
    """Negative items and a null handle are refused and change nothing; a handle from mst_tcn_create never chunks until it is asked."""
    from music_mixing_style_transfer_amd import _lib
    from tcn_block_ref import PlanTracer
    tr = PlanTracer(emu)
    try:
        dil = (1, 2, 4, 8, 16)
        h = tr._handle(dil)
        items, ran = C.c_int(-1), C.c_int(-1)
        emu.check(emu.mst_tcn_get_chunk(h, C.byref(items), C.byref(ran)), "get_chunk")
        assert (items.value, ran.value) == (_lib.TCN_CHUNK_WHOLE, 1)
        for bad in (-1, -5, -(1 << 31)):
            assert emu.mst_tcn_set_chunk(h, bad) != 0
        assert emu.mst_tcn_set_chunk(None, 2) != 0 and emu.mst_tcn_get_chunk(None, None, None) != 0
        emu.check(emu.mst_tcn_get_chunk(h, C.byref(items), None), "get_chunk")
        assert items.value == _lib.TCN_CHUNK_WHOLE
        raw = tr.launches(dil, 245, 4, 256, "bf16")
        emu.check(emu.mst_tcn_set_chunk(h, 2), "set_chunk")
        assert tr.launches(dil, 245, 4, 256, "bf16") == raw + raw          # (symbols only: two chunks of two items)
        emu.check(emu.mst_tcn_get_chunk(h, None, C.byref(ran)), "get_chunk")
        assert ran.value == 2
        # chunks of three in a batch of four: the second chain's buffers do not fit the workspace, the chunks still run (one chain)
        emu.check(emu.mst_tcn_set_chunk(h, 3), "set_chunk")
        assert tr.launches(dil, 245, 4, 256, "bf16") == raw + raw
        emu.check(emu.mst_tcn_set_chunk(h, 0), "set_chunk")
        assert tr.launches(dil, 245, 4, 256, "bf16") == raw
        # automatic at sizes that chunk (a dry run: nothing is computed).  32 x 131072: one activation is 1 GiB, chunks of 2.  8 x 131072: one
        # activation is exactly the cache, the whole batch.  32 x 2^19: a chunk of one item per chain would not fit, the whole batch.
        for Bn, L, chunks in ((32, 131072, 16), (9, 131072, 5), (8, 131072, 1), (32, 1 << 19, 1), (32, 65536, 8), (3, 2048, 1)):
            tr.launches(dil, 245, Bn, L, "bf16")
            emu.check(emu.mst_tcn_get_chunk(h, None, C.byref(ran)), "get_chunk")
            assert ran.value == chunks, (Bn, L, ran.value)
        emu.check(emu.mst_tcn_set_chunk(h, _lib.TCN_CHUNK_WHOLE), "set_chunk")
    finally:
        tr.close()


def test_timing_hook_sums_a_block_over_the_chunks(emu_default):
    emu = emu_default
    nblocks = 5
    m = _tcn(nblocks)
    x, cond = make_input(B, 256, seed=5), make_cond("B", B, COND_DIM, nblocks, seed=7)
    m._ensure(emu)
    _set_chunk(emu, m, 2)
    emu.check(emu.mst_tcn_timing_begin(m._handle, 1), "timing_begin")
    m(x, cond)
    m(x, cond)          # beyond max_forwards: not recorded
    ms, nf = (C.c_float * (nblocks + 1))(), C.c_int(0)
    emu.check(emu.mst_tcn_timing_end(m._handle, ms, C.byref(nf)), "timing_end")
    assert nf.value == 1 and _chunk(emu, m) == (2, 3)
    assert len(ms) == nblocks + 1 and all(v > 0.0 for v in ms), list(ms)
    assert ms[2] == ms[3] == ms[4]          # the fused tail's shares, chunk by chunk
