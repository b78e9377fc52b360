"""Per-item panner, Haas and reverbs (mst_fx_panner_items, mst_fx_haas_items, mst_fx_convolve_items, mst_fx_algorithmic_reverb_items) on the CPU
emulator: item i of a per-item call against the shared-parameter call on the same batch with item i's settings bit for bit, against float64
references, the refusals of mst_fx_convolve_items_prepare, process_items against process(), and the whole instrument chains through
AugmentationChain.call_items without a per-item loop.  The same bodies (tests/fx_space_items_ref.py) run on the MI355X in
tests/test_fx_space_items_gpu.py."""
import pytest

import fx_items_ref as I
import fx_pass_ref as R
import fx_space_items_ref as S


@pytest.fixture(scope="module")
def run(emu):
    return R.Runner(emu, "cpu")


@pytest.fixture(scope="module")
def ir_dir(tmp_path_factory):
    return S.write_ir_dir(tmp_path_factory.mktemp("irs"))


def test_version(run):
    assert run.lib.mst_version() >= 105


@pytest.mark.parametrize("c_in", [1, 2])
@pytest.mark.parametrize("L", [257, 1000])
def test_panner_items(run, L, c_in):
    S.check_panner(run, L, c_in)


@pytest.mark.parametrize("c_in", [1, 2])
@pytest.mark.parametrize("L", [257, 1000])
def test_haas_items(run, L, c_in):
    S.check_haas(run, L, c_in)


@pytest.mark.parametrize("Cn", [2, 1])
def test_convolve_items_one_block(run, Cn):
    S.check_conv_one_block(run, Cn)


def test_convolve_items_overlap_save(run):
    """two mono items: the 300-frame response cut at its last frame, the 7-frame response at its last frame (the GPU test adds offset 0)"""
    S.check_conv_overlap_save(run, 2, 1, [(0, 299), (1, 6)])


def test_convolve_items_prepare_refusals(run):
    S.check_conv_refusals(run)


@pytest.mark.parametrize("Cn", [1, 2])
def test_algorithmic_reverb_items(run, Cn):
    S.check_algorithmic_reverb(run, Cn)


@pytest.mark.parametrize("kind", ["panner", "haas", "algo", "conv"])
def test_process_items_match_process(emu_default, kind):
    S.check_process_items("cpu", kind)


def test_convolution_process_items_splits_a_batch_beyond_the_block_limit(emu_default, monkeypatch):
    S.check_conv_process_items_split("cpu", monkeypatch)


@pytest.mark.parametrize("inst", ["vocals", "drums", "bass"])
def test_call_items_instrument_chain_vs_oracle(emu_default, oracle_fx_lib, ir_dir, inst):
    S.check_inst_chain("cpu", inst, ir_dir, I.oracle_compressor_fn(oracle_fx_lib))


@pytest.mark.parametrize("inst", ["vocals", "drums", "bass"])
def test_call_items_runs_no_item_loop(emu_default, oracle_fx_lib, ir_dir, inst, monkeypatch):
    S.check_no_item_loop("cpu", inst, ir_dir, I.oracle_compressor_fn(oracle_fx_lib), monkeypatch)
