"""Training batches on the MI355X: the case bodies of tests/test_trainbatch_emu.py (tests/trainbatch_ref.py) through libmst_hip.so - the two
streaming kernels bit for bit at every alignment and at the training shape (64 rows of 135168 frames), the stem bank, grouped plans and whole
batches of both MUSDB datasets against the oracle replay, without a per-item loop, and against the item loop; the measurement tool runs once."""
import json
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fx_items_ref as I  # noqa: E402
import fx_pass_ref as R  # noqa: E402
import fx_space_items_ref as S  # noqa: E402
import trainbatch_ref as T  # noqa: E402
from music_mixing_style_transfer_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def run():
    assert torch.cuda.is_available(), "needs the MI355X"
    b = _lib.lib()
    assert b.path.endswith("libmst_hip.so") and b.mst_version() >= 108
    return R.Runner(b, DEV)


@pytest.fixture(scope="module")
def ir_dir(tmp_path_factory):
    return S.write_ir_dir(tmp_path_factory.mktemp("irs"))


@pytest.fixture(scope="module")
def musdb(tmp_path_factory):
    return T.write_musdb_dir(tmp_path_factory.mktemp("musdb"))


@pytest.mark.parametrize("width", [2, 4])
def test_gather_pcm_bit_exact_gpu(run, width):
    T.check_gather(run, width)


def test_gather_pcm_refusals_gpu(run):
    T.check_gather_refusals(run)


@pytest.mark.parametrize("Cn", [1, 2])
def test_finish_bit_exact_gpu(run, Cn):
    T.check_finish(run, Cn)


def test_finish_refusals_gpu(run):
    T.check_finish_refusals(run)


def test_wrappers_raise_for_a_row_out_of_range_gpu(run):
    T.check_wrappers(DEV)


@pytest.mark.parametrize("width", [2, 4])
def test_stem_bank_resident_and_host_banks_gpu(run, tmp_path, width):
    T.check_stem_bank(DEV, tmp_path, width)


@pytest.mark.parametrize("width", [2, 4])
def test_gather_pcm_training_shape_gpu(run, width):
    T.check_gather_large(run, width)


def test_finish_training_shape_gpu(run):
    T.check_finish_large(run)


@pytest.mark.parametrize("inst", ["vocals", "drums", "bass"])
def test_call_plans_groups_of_two_vs_oracle_gpu(run, oracle_fx_lib, ir_dir, inst):
    T.check_call_plans(DEV, inst, ir_dir, I.oracle_compressor_fn(oracle_fx_lib))


@pytest.mark.parametrize("inst", ["vocals", "drums", "bass"])
def test_call_items_is_call_plans_of_plan_items_gpu(run, oracle_fx_lib, ir_dir, inst):
    T.check_call_items_unchanged(DEV, inst, ir_dir, I.oracle_compressor_fn(oracle_fx_lib))


@pytest.mark.parametrize("ir", [True, False])
@pytest.mark.parametrize("kind", ["fxenc", "style"])
def test_get_batch_vs_oracle_replay_gpu(run, oracle_fx_lib, musdb, ir_dir, kind, ir):
    T.check_batch_vs_oracle(DEV, kind, musdb, ir_dir if ir else None, I.oracle_compressor_fn(oracle_fx_lib), T.BATCH_SEEDS[kind, ir])


@pytest.mark.parametrize("kind", ["fxenc", "style"])
def test_get_batch_runs_no_item_loop_gpu(run, oracle_fx_lib, musdb, ir_dir, kind, monkeypatch):
    T.check_no_loop(DEV, kind, musdb, ir_dir, I.oracle_compressor_fn(oracle_fx_lib), T.BATCH_SEEDS[kind, True], monkeypatch)


@pytest.mark.parametrize("kind", ["fxenc", "style"])
def test_get_batch_vs_item_loop_gpu(run, musdb, ir_dir, kind):
    T.check_batch_vs_items(DEV, kind, musdb, ir_dir, T.BATCH_SEEDS[kind, True])


def test_bench_trainbatch_tool_runs_gpu(run, tmp_path):
    """tools/bench_trainbatch.py at a small shape: one JSON result line with the figures the documents quote"""
    out = tmp_path / "bench.json"
    p = subprocess.run([sys.executable, os.path.join(REPO, "tools", "bench_trainbatch.py"), "--segment", "16384", "--seconds", "4", "--files", "2", "--batch", "4",
                        "--rounds", "2", "--warmup", "1", "--out", str(out)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    res = json.loads(out.read_text())
    assert res == json.loads(p.stdout.strip().splitlines()[-1])
    for key in ("get_batch_ms", "item_loop_ms", "gather_ms", "gather_gb_s", "finish_ms", "finish_gb_s", "host_plan_ms"):
        assert res[key] > 0, key


@pytest.mark.parametrize("via", ["item", "batch"])
@pytest.mark.parametrize("kind,pad,neg", T.GOLDEN_CASES)
def test_items_vs_the_reference_gpu(run, musdb, kind, pad, neg, via):
    T.check_golden_items(DEV, kind, pad, neg, musdb, via)


def test_behind_a_dataloader_without_workers_gpu(run, musdb):
    T.check_dataloader(DEV, musdb)
