"""The last three bf16 TCN blocks as one launch (mst_tcn_set_fusion bit 0, tcn_tail_bf16_kernel) on the MI355X: the bits of the three
launches it replaces - on the two small nets of tests/test_tcn_tail_emu.py (plain and XCD tile order), on the real tail (14 blocks,
L = 131072: d = 2048, 4096, 8192) with one FiLM row and with a row per item, and with a fused and an unfused handle sharing the device on
two streams."""
import ctypes as C

import pytest
import torch

from tcn_block_ref import make_cond, make_input

pytestmark = pytest.mark.gpu
COND_DIM = 64


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
    assert lib.path.endswith("libmst_hip.so") and lib.mst_version() >= 104
    return lib


def _run(lib, m, x, cond, fusion):
    """y of one forward with the handle's fusion flags set to `fusion`, and whether that forward ran the fused tail."""
    m._ensure(lib)
    lib.check(lib.mst_tcn_set_fusion(m._handle, fusion), "set_fusion")
    y = m(x, cond)
    ran = C.c_int(-1)
    lib.check(lib.mst_tcn_get_fusion(m._handle, None, C.byref(ran)), "get_fusion")
    return y, ran.value


@pytest.fixture(scope="module")
def real_tail():
    """The 14-block net and its input, shared: (model, x [2, 2, 131072] with a silent and a full-scale item)."""
    return _tcn(14), make_input(2, 131072, seed=9).to("cuda:0")


def _cond(film, B, nblocks):
    c = make_cond(film, B, COND_DIM, nblocks, seed=7)
    return [t.to("cuda:0") for t in c] if isinstance(c, list) else c.to("cuda:0")


@pytest.mark.parametrize("nblocks,L,B,film", [(5, 256, 3, "B"), (5, 256, 1, "1"), (8, 2048, 3, "list"), (8, 2048, 1, "1")])
def test_fused_tail_small_nets_bit_identical(nblocks, L, B, film):
    lib, m = _lib(), _tcn(nblocks)
    x, cond = make_input(B, L, seed=100 + nblocks).to("cuda:0"), _cond(film, B, nblocks)
    y0, ran0 = _run(lib, m, x, cond, 0)
    y1, ran1 = _run(lib, m, x, cond, 1)
    torch.cuda.synchronize()
    assert (ran0, ran1) == (0, 1)
    assert torch.equal(y1, y0) and float(y0.abs().max()) > 0.0


@pytest.mark.parametrize("film", ["1", "B"])
def test_fused_tail_at_the_headline_segment_length_bit_identical(real_tail, film):
    lib = _lib()
    m, x = real_tail
    cond = _cond(film, 2, 14)
    y0, ran0 = _run(lib, m, x, cond, 0)
    y1, ran1 = _run(lib, m, x, cond, 1)
    torch.cuda.synchronize()
    assert (ran0, ran1) == (0, 1)
    assert torch.equal(y1, y0) and float(y0.abs().max()) > 0.0


def test_fused_and_unfused_handles_on_two_streams(real_tail):
    """Two handles of the same net share the device, one with the fused tail and one without: each gives the bits of its solo run."""
    lib = _lib()
    m_f, x = real_tail
    m_u = _tcn(14)
    cond = _cond("B", 2, 14)
    solo_f, ran_f = _run(lib, m_f, x, cond, 1)
    solo_u, ran_u = _run(lib, m_u, x, cond, 0)
    torch.cuda.synchronize()
    assert (ran_f, ran_u) == (1, 0) and torch.equal(solo_f, solo_u)
    s_f, s_u = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s_f):
        y_f = [m_f(x, cond) for _ in range(2)]
    with torch.cuda.stream(s_u):
        y_u = [m_u(x, cond) for _ in range(2)]
    s_f.synchronize()
    s_u.synchronize()
    for y in y_f:
        assert torch.equal(y, solo_f)
    for y in y_u:
        assert torch.equal(y, solo_u)
    ran = C.c_int(-1)
    lib.check(lib.mst_tcn_get_fusion(m_f._handle, None, C.byref(ran)), "get_fusion")
    assert ran.value == 1
    lib.check(lib.mst_tcn_get_fusion(m_u._handle, None, C.byref(ran)), "get_fusion")
    assert ran.value == 0
