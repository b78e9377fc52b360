"""Training batches on the CPU emulator: mst_batch_gather_pcm and mst_batch_finish bit for bit at every alignment and their refusals, the
resident stem bank, AugmentationChain.call_plans against the oracle replay, and whole batches of the two MUSDB datasets (get_batch against the
oracle replay of its own draws, without a per-item loop, and against the item loop).  The same bodies (tests/trainbatch_ref.py) run on the
MI355X in tests/test_trainbatch_gpu.py."""
import pytest

import fx_items_ref as I
import fx_pass_ref as R
import fx_space_items_ref as S
import trainbatch_ref as T


@pytest.fixture(scope="module")
def run(emu):
    return R.Runner(emu, "cpu")


@pytest.fixture(scope="module")
def ir_dir(tmp_path_factory):
    return S.write_ir_dir(tmp_path_factory.mktemp("irs"))


@pytest.fixture(scope="module")
def musdb(tmp_path_factory):
    return T.write_musdb_dir(tmp_path_factory.mktemp("musdb"))


def test_version(run):
    assert run.lib.mst_version() >= 108


@pytest.mark.parametrize("width", [2, 4])
def test_gather_pcm_bit_exact(run, width):
    T.check_gather(run, width)


def test_gather_pcm_refusals(run):
    T.check_gather_refusals(run)


@pytest.mark.parametrize("Cn", [1, 2])
def test_finish_bit_exact(run, Cn):
    T.check_finish(run, Cn)


def test_finish_refusals(run):
    T.check_finish_refusals(run)


def test_wrappers_raise_for_a_row_out_of_range(emu_default):
    T.check_wrappers("cpu")


@pytest.mark.parametrize("width", [2, 4])
def test_stem_bank_resident_and_host_banks(emu_default, tmp_path, width):
    T.check_stem_bank("cpu", tmp_path, width)


@pytest.mark.parametrize("inst", ["vocals", "drums", "bass"])
def test_call_plans_groups_of_two_vs_oracle(emu_default, oracle_fx_lib, ir_dir, inst):
    T.check_call_plans("cpu", inst, ir_dir, I.oracle_compressor_fn(oracle_fx_lib))


@pytest.mark.parametrize("inst", ["vocals", "drums", "bass"])
def test_call_items_is_call_plans_of_plan_items(emu_default, oracle_fx_lib, ir_dir, inst):
    T.check_call_items_unchanged("cpu", inst, ir_dir, I.oracle_compressor_fn(oracle_fx_lib))


@pytest.mark.parametrize("ir", [True, False])
@pytest.mark.parametrize("kind", ["fxenc", "style"])
def test_get_batch_vs_oracle_replay(emu_default, oracle_fx_lib, musdb, ir_dir, kind, ir):
    T.check_batch_vs_oracle("cpu", kind, musdb, ir_dir if ir else None, I.oracle_compressor_fn(oracle_fx_lib), T.BATCH_SEEDS[kind, ir])


@pytest.mark.parametrize("kind", ["fxenc", "style"])
def test_get_batch_runs_no_item_loop(emu_default, oracle_fx_lib, musdb, ir_dir, kind, monkeypatch):
    T.check_no_loop("cpu", kind, musdb, ir_dir, I.oracle_compressor_fn(oracle_fx_lib), T.BATCH_SEEDS[kind, True], monkeypatch)


@pytest.mark.parametrize("kind", ["fxenc", "style"])
def test_get_batch_vs_item_loop(emu_default, musdb, ir_dir, kind):
    T.check_batch_vs_items("cpu", kind, musdb, ir_dir, T.BATCH_SEEDS[kind, True])


@pytest.mark.parametrize("via", ["item", "batch"])
@pytest.mark.parametrize("kind,pad,neg", T.GOLDEN_CASES)
def test_items_vs_the_reference(emu_default, musdb, kind, pad, neg, via):
    T.check_golden_items("cpu", kind, pad, neg, musdb, via)


def test_behind_a_dataloader_without_workers(emu_default, musdb):
    T.check_dataloader("cpu", musdb)
