"""Per-item panner, Haas and reverbs on the MI355X: the case bodies of tests/test_fx_space_items_emu.py (tests/fx_space_items_ref.py) through
libmst_hip.so - item i of a per-item call against the shared-parameter call on the same batch bit for bit, against float64 references,
process_items against process(), and the instrument chains through AugmentationChain.call_items without a per-item loop."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fx_items_ref as I  # noqa: E402
import fx_pass_ref as R  # noqa: E402
import fx_space_items_ref as S  # noqa: E402
from music_mixing_style_transfer_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def run():
    assert torch.cuda.is_available(), "needs the MI355X"
    b = _lib.lib()
    assert b.path.endswith("libmst_hip.so") and b.mst_version() >= 105
    return R.Runner(b, DEV)


@pytest.fixture(scope="module")
def ir_dir(tmp_path_factory):
    return S.write_ir_dir(tmp_path_factory.mktemp("irs"))


@pytest.mark.parametrize("c_in", [1, 2])
@pytest.mark.parametrize("L", [257, 1000])
def test_panner_items_gpu(run, L, c_in):
    S.check_panner(run, L, c_in)


@pytest.mark.parametrize("c_in", [1, 2])
@pytest.mark.parametrize("L", [257, 1000])
def test_haas_items_gpu(run, L, c_in):
    S.check_haas(run, L, c_in)


@pytest.mark.parametrize("Cn", [2, 1])
def test_convolve_items_one_block_gpu(run, Cn):
    S.check_conv_one_block(run, Cn)


def test_convolve_items_overlap_save_gpu(run):
    """three stereo items: the 300-frame response cut at its first and at its last frame, the 7-frame response at its last frame"""
    S.check_conv_overlap_save(run, 3, 2, [(0, 0), (0, 299), (1, 6)])


@pytest.mark.parametrize("Cn", [1, 2])
def test_algorithmic_reverb_items_gpu(run, Cn):
    S.check_algorithmic_reverb(run, Cn)


@pytest.mark.parametrize("kind", ["panner", "haas", "algo", "conv"])
def test_process_items_match_process_gpu(run, kind):
    S.check_process_items(DEV, kind)


def test_convolution_process_items_splits_a_batch_beyond_the_block_limit_gpu(run, monkeypatch):
    S.check_conv_process_items_split(DEV, monkeypatch)


@pytest.mark.parametrize("inst", ["vocals", "drums", "bass"])
def test_call_items_instrument_chain_vs_oracle_gpu(run, oracle_fx_lib, ir_dir, inst):
    S.check_inst_chain(DEV, inst, ir_dir, I.oracle_compressor_fn(oracle_fx_lib))


@pytest.mark.parametrize("inst", ["vocals", "drums", "bass"])
def test_call_items_runs_no_item_loop_gpu(run, oracle_fx_lib, ir_dir, inst, monkeypatch):
    S.check_no_item_loop(DEV, inst, ir_dir, I.oracle_compressor_fn(oracle_fx_lib), monkeypatch)
