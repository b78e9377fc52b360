"""Per-item FX parameters on the MI355X: the case bodies of tests/test_fx_items_emu.py (tests/fx_items_ref.py) through libmst_hip.so - the
device-built tables against mst_fx_biquad_tables bit for bit, _items calls against shared-parameter calls on the same batch, the pass-by-pass
longdouble checks of tests/fx_pass_ref.py through the per-item entry points.  The workgroups of a launch arrive in no fixed order here, so the
energy slots that several chunks add to are compared as fx_items_ref.same_energy says; everything else bit for bit."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fx_items_ref as I  # noqa: E402
import fx_pass_ref as R  # noqa: E402
from music_mixing_style_transfer_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
case_id = lambda c: f"{c[0]}-{c[1]}x{c[2]}x{c[3]}-forms{c[4]}"


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "needs the MI355X"
    b = _lib.lib()
    assert b.path.endswith("libmst_hip.so") and b.mst_version() >= 103
    return b


@pytest.fixture(scope="module")
def run(lib):
    return I.ItemsRunner(lib, DEV)


@pytest.fixture(scope="module")
def shared(lib):
    return R.Runner(lib, DEV)


@pytest.mark.parametrize("name", ["peaks1", "config4", "peaks8"])
@pytest.mark.parametrize("L,M", [(4099, 64), (64 * 511 + 1, 80)])
def test_device_built_tables_are_the_hosts_bits_gpu(run, name, L, M):
    I.check_tables(run, name, L, 5, 2, expect_M=lambda m: m == M)


@pytest.mark.parametrize("case", I.EQ_SAME, ids=case_id)
def test_equaliser_same_parameters_same_bits_gpu(run, shared, case):
    I.check_eq_same(run, shared, *case, ordered=False)


@pytest.mark.parametrize("case", I.EQ_DIFFERENT, ids=case_id)
def test_equaliser_different_parameters_gpu(run, shared, case):
    name, L, n, Cn, forms = case
    I.check_eq_different(run, shared, name, L, n, Cn, forms=forms, fused=L > 64, ordered=False)


def test_imager_and_gain_items_gpu(run):
    I.check_imager_gain(run)


@pytest.mark.parametrize("case", I.EQ_SAME, ids=case_id)
def test_equaliser_items_passes_against_longdouble_gpu(run, case):
    name, L, n, Cn, forms, fused = case
    kw = dict(scale=I.eq_fuse_kw(n, True)["in_scale"], sumsq=True, in_sumsq=True) if fused else {}
    R.check_equaliser(run, name, L, n, Cn, forms=forms, **kw)


@pytest.mark.parametrize("probs", [(1.0, 1.0, 1.0, 1.0), (0.5, 0.5, 0.5, 0.5)], ids=["p1", "p05"])
def test_call_items_random_chain_vs_oracle_gpu(lib, oracle_fx_lib, probs):
    """AugmentationChain.call_items: a seeded randomised EQ -> compressor -> imager -> gain chain with rms-normalise (BASELINE configs[3]'s
    processors), six items of [16384, 2] with their own draws, each within 2e-6 max|ref| of the oracle's processors composed with them"""
    I.check_random_chain(DEV, I.oracle_compressor_fn(oracle_fx_lib), probs)


@pytest.fixture(scope="module")
def crun(lib):
    return I.CompItemsRunner(lib, DEV)


comp_id = lambda c: f"{c[0]}x{c[1]}x{c[2]}-forms{c[3]}" + ("-fused" if c[4] else "")


@pytest.mark.parametrize("case", I.COMP_SAME, ids=comp_id)
def test_compressor_same_parameters_same_bits_gpu(crun, shared, case):
    I.check_comp_same(crun, shared, *case)


@pytest.mark.parametrize("L,Cn,forms", [(4133, 2, 0), (4133, 1, 0), (96, 2, 0), (9001, 2, 4), (200, 2, -1)])
def test_compressor_different_parameters_gpu(run, shared, L, Cn, forms):
    I.check_comp_different(run, shared, L, 6, Cn, forms=forms, fused=forms >= 0)


@pytest.mark.parametrize("case", [c for c in I.COMP_SAME if c[3] >= 0], ids=comp_id)
def test_compressor_items_passes_against_longdouble_gpu(crun, case):
    L, n, Cn, forms, fused = case
    kw = dict(scale=I.COMP_SCALE[:n], sumsq=True) if fused else {}
    R.check_compressor(crun, L, n, Cn, *I.BASE, forms=forms, **kw)


def test_compressor_items_prepare_refuses_the_ill_conditioned_item_gpu(run):
    I.check_comp_refusal(run)


def test_compressor_process_items_reroutes_the_refused_item_gpu(lib):
    I.check_comp_python_reroute(DEV)
