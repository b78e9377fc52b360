"""The bf16 TCN forward over chunks of the batch (mst_tcn_set_chunk) on the MI355X: two chains of chunks, the caller's stream and the
handle's side stream, have to give the bits of the whole-batch forward - with the caller on the default and on another stream, with a
dependent operation right behind two forwards (the join orders the side stream before the caller's stream goes on), with two handles on two
host threads, and at a size that really chunks (8 x 131072 of the 14-block net)."""
import ctypes as C
import threading

import pytest
import torch

from tcn_block_ref import make_cond, make_input

pytestmark = pytest.mark.gpu
COND_DIM = 64
NBLOCKS, B, L = 8, 6, 2048


def _tcn(nblocks, seed=0):
    from music_mixing_style_transfer_amd.networks import TCNModel
    from music_mixing_style_transfer_amd.utils import synth
    sd = synth.tcn_state_dict(nblocks=nblocks, cond_dim=COND_DIM, seed=seed)
    m = TCNModel(nparams=COND_DIM, ninputs=2, noutputs=2, nblocks=nblocks, dilation_growth=2, kernel_size=15,
                 channel_width=128, stack_size=15, cond_dim=COND_DIM, causal=False).to("cuda:0")
    m.load_state_dict(sd)
    m.precision = "bf16"
    return m


def _lib():
    from music_mixing_style_transfer_amd import _lib
    lib = _lib.lib()
    assert lib.path.endswith("libmst_hip.so") and lib.mst_version() >= 110
    return lib


def _run(lib, m, x, cond, items):
    """y of one forward with the handle's chunk setting `items`, and how many chunks that forward ran."""
    m._ensure(lib)
    lib.check(lib.mst_tcn_set_chunk(m._handle, items), "set_chunk")
    y = m(x, cond)
    ran = C.c_int(-1)
    lib.check(lib.mst_tcn_get_chunk(m._handle, None, C.byref(ran)), "get_chunk")
    return y, ran.value


@pytest.fixture(scope="module")
def small():
    """(model, x [6, 2, 2048], FiLM condition with a row per item, the whole-batch output): computed once, never changed."""
    lib, m = _lib(), _tcn(NBLOCKS)
    x = make_input(B, L, seed=31).to("cuda:0")
    cond = make_cond("B", B, COND_DIM, NBLOCKS, seed=7).to("cuda:0")
    y0, ran = _run(lib, m, x, cond, 0)
    torch.cuda.synchronize()
    assert ran == 1 and float(y0.abs().max()) > 0.0          # automatic at this size: the whole batch
    return m, x, cond, y0


@pytest.mark.parametrize("other_stream", [False, True])
def test_chunked_forward_bit_identical(small, other_stream):
    lib = _lib()
    m, x, cond, y0 = small
    s = torch.cuda.Stream() if other_stream else torch.cuda.current_stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for items, chunks in ((1, 6), (2, 3), (4, 2)):          # (4: 4 + 2 items; the second chain's buffers do not fit: one chain)
            y, ran = _run(lib, m, x, cond, items)
            s.synchronize()
            assert ran == chunks
            assert torch.equal(y, y0), (items, float((y - y0).abs().max()))
        y, ran = _run(lib, m, x, cond[:1], 2)                   # one shared FiLM row
        y1, ran1 = _run(lib, m, x, cond[:1], 0)
        s.synchronize()
        assert (ran, ran1) == (3, 1) and torch.equal(y, y1) and not torch.equal(y, y0)


def test_two_forwards_and_a_dependent_operation_behind_them(small):
    """Nothing waits on the host between the two forwards and the sum: if the join did not order the side stream's chunks before the caller's
    stream goes on, the sum would read items the side stream has not written yet."""
    lib = _lib()
    m, x, cond, y0 = small
    x2 = torch.flip(x, dims=(0,)).contiguous()
    cond2 = torch.flip(cond, dims=(0,)).contiguous()
    want = y0 + 2.0 * torch.flip(y0, dims=(0,))
    lib.check(lib.mst_tcn_set_chunk(m._handle, 1), "set_chunk")
    for _ in range(3):
        ya = m(x, cond)
        yb = m(x2, cond2)
        z = ya + 2.0 * yb
        assert torch.equal(z, want)
    lib.check(lib.mst_tcn_set_chunk(m._handle, 0), "set_chunk")


def test_two_handles_on_two_host_threads(small):
    lib = _lib()
    m, x, cond, y0 = small
    models = [m, _tcn(NBLOCKS)]
    xs = [x, torch.flip(x, dims=(0,)).contiguous()]
    conds = [cond, torch.flip(cond, dims=(0,)).contiguous()]
    wants = [y0, torch.flip(y0, dims=(0,))]
    for mm in models:
        mm._ensure(lib)
        lib.check(lib.mst_tcn_set_chunk(mm._handle, 2), "set_chunk")
    torch.cuda.synchronize()
    got, errors = [None, None], []

    def work(i):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                ys = [models[i](xs[i], conds[i]) for _ in range(4)]
            s.synchronize()
            got[i] = ys
        except Exception as e:          # noqa: BLE001 - reported below, in the test's thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(2):
        for y in got[i]:
            assert torch.equal(y, wants[i])
    lib.check(lib.mst_tcn_set_chunk(m._handle, 0), "set_chunk")


def test_headline_segment_length_in_chunks_bit_identical():
    """8 x 131072 of the 14-block net: one activation is exactly the Infinity Cache, so automatic keeps the whole batch; chunks of 2 - what
    automatic takes from 9 items on - run the size the schedule is for: 4 chunks, two chains, the fused tail per chunk."""
    lib, m = _lib(), _tcn(14)
    Bn = 8
    x = make_input(Bn, 131072, seed=9).to("cuda:0")
    cond = make_cond("B", Bn, COND_DIM, 14, seed=7).to("cuda:0")
    y_auto, ran_auto = _run(lib, m, x, cond, 0)
    y_whole, ran_whole = _run(lib, m, x, cond, Bn)
    y_c, ran_c = _run(lib, m, x, cond, 2)
    tail = C.c_int(-1)
    lib.check(lib.mst_tcn_get_fusion(m._handle, None, C.byref(tail)), "get_fusion")
    torch.cuda.synchronize()
    assert (ran_auto, ran_whole, ran_c, tail.value) == (1, 1, 4, 1)
    assert float(y_whole.abs().max()) > 0.0
    assert torch.equal(y_c, y_whole) and torch.equal(y_auto, y_whole)
