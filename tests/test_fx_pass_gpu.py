"""The time-parallel equaliser and compressor pass by pass on the MI355X: the case bodies of tests/test_fx_pass_emu.py (tests/fx_pass_ref.py)
through libmst_hip.so - chunk end / start states, chunk maps, chunk start values, carry, tile sums, every output sample and the energy
by-products against the longdouble reference, each within the bound computed beside it.  Needs numpy and the repository only.
Figures of one run: profiles/fx_pass_exact_mi355x.txt."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fx_pass_ref as R  # noqa: E402
from music_mixing_style_transfer_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def run():
    assert torch.cuda.is_available(), "needs the MI355X"
    lib = _lib.lib()
    assert lib.path.endswith("libmst_hip.so") and lib.mst_version() >= 102
    return R.Runner(lib, DEV)


@pytest.mark.parametrize("case", R.EQ_CASES, ids=R.eq_id)
def test_equaliser_passes_gpu(run, case):
    R.check_equaliser(run, **case)


@pytest.mark.parametrize("case", R.COMP_CASES, ids=R.comp_id)
def test_compressor_passes_gpu(run, case):
    R.check_compressor(run, **case)


@pytest.mark.parametrize("k", range(1, 9))
def test_equaliser_forms_stay_bit_identical_gpu(run, k):
    R.check_forms_identical(run, k)


def test_fast_attack_is_right_through_every_public_path_gpu(run):
    R.check_fast_attack_public_paths(run)


def test_ill_conditioned_fused_and_grid_calls_are_refused_gpu(run):
    R.check_refusals(run)
