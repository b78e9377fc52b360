"""Per-item FX parameters (mst_fx_biquad_cascade_items, mst_fx_compressor_items, mst_fx_midside_imager_items, mst_fx_gain_items) on the CPU emulator: the device-built
tables against mst_fx_biquad_tables bit for bit, an _items call against shared-parameter calls on the same batch bit for bit (same settings
for every item; different settings: n shared calls), the pass-by-pass longdouble checks of tests/fx_pass_ref.py through the per-item entry
points, and the launch coverage of the fxi_* kernels.  The same bodies run on the MI355X in tests/test_fx_items_gpu.py."""
import numpy as np
import pytest

import fx_items_ref as I
import fx_pass_ref as R


@pytest.fixture(autouse=True)
def one_emulator_worker(monkeypatch):
    """The equaliser's energy slots are float64 atomics: their bits depend on the order in which the workgroups arrive.  One emulator worker
    runs the workgroups in index order, the same chunk order in the shared and the per-item call - then every slot is compared bit for bit."""
    monkeypatch.setenv("MST_EMU_THREADS", "1")


@pytest.fixture(scope="module")
def run(emu):
    return I.ItemsRunner(emu, "cpu")


@pytest.fixture(scope="module")
def shared(emu):
    return R.Runner(emu, "cpu")


def test_version_and_plan(run):
    import ctypes as C
    from music_mixing_style_transfer_amd import _lib
    lib = run.lib
    assert lib.mst_version() >= 103
    p = _lib.MstFxBiquadItemsPlan()
    p.struct_size = 4
    assert lib.mst_fx_biquad_items_plan(5, 4099, 2, 5, C.byref(p)) == -1
    p = run.eq_items_plan(5, 4099, 2, 5)
    assert p.tables_offset == lib.mst_fx_biquad_scratch_bytes(5, 4099, 2, 5) and p.item_stride == 8 * (p.M * 10 + 9 * 100 + 40)
    assert p.total_bytes == lib.mst_fx_biquad_items_scratch_bytes(5, 4099, 2, 5) == p.tables_offset + 5 * p.item_stride


@pytest.mark.parametrize("name", ["peaks1", "config4", "peaks8"])
@pytest.mark.parametrize("L,M", [(4099, 64), (64 * 511 + 1, 80)])
def test_device_built_tables_are_the_hosts_bits(run, name, L, M):
    """five different coefficient sets; 1, 5 and 8 bands; M = 64 and the first M beyond it (the shortest signal that has it)"""
    assert R.coef_sets()[name].shape[0] == {"peaks1": 1, "config4": 5, "peaks8": 8}[name]
    I.check_tables(run, name, L, 5, 2, expect_M=lambda m: m == M)


@pytest.mark.parametrize("case", I.EQ_SAME, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}x{c[3]}-forms{c[4]}")
def test_equaliser_same_parameters_same_bits(run, shared, case):
    I.check_eq_same(run, shared, *case)


@pytest.mark.parametrize("case", I.EQ_DIFFERENT, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}x{c[3]}-forms{c[4]}")
def test_equaliser_different_parameters(run, shared, case):
    name, L, n, Cn, forms = case
    I.check_eq_different(run, shared, name, L, n, Cn, forms=forms, fused=L > 64)


def test_imager_and_gain_items(run):
    I.check_imager_gain(run)


@pytest.mark.parametrize("case", I.EQ_SAME, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}x{c[3]}-forms{c[4]}")
def test_equaliser_items_passes_against_longdouble(run, case):
    """fx_pass_ref.check_equaliser, unchanged, through the per-item entry point: the scratch layout is the shared call's"""
    name, L, n, Cn, forms, fused = case
    kw = dict(scale=I.eq_fuse_kw(n, True)["in_scale"], sumsq=True, in_sumsq=True) if fused else {}
    R.check_equaliser(run, name, L, n, Cn, forms=forms, **kw)


@pytest.fixture(scope="module")
def crun(emu):
    return I.CompItemsRunner(emu, "cpu")


comp_id = lambda c: f"{c[0]}x{c[1]}x{c[2]}-forms{c[3]}" + ("-fused" if c[4] else "")


@pytest.mark.parametrize("case", I.COMP_SAME, ids=comp_id)
def test_compressor_same_parameters_same_bits(crun, shared, case):
    from music_mixing_style_transfer_amd import _lib
    plan = I.check_comp_same(crun, shared, *case)
    L, forms = case[0], case[3]
    assert plan.form == (_lib.FX_COMP_SPLIT_SERIAL if L == 96 else _lib.FX_COMP_TIME_PARALLEL) and plan.nslices == (3 if forms > 0 else 1)


@pytest.mark.parametrize("L,Cn,forms", [(4133, 2, 0), (4133, 1, 0), (96, 2, 0), (9001, 2, 4), (200, 2, -1)])
def test_compressor_different_parameters(run, shared, L, Cn, forms):
    I.check_comp_different(run, shared, L, 6, Cn, forms=forms, fused=forms >= 0)


@pytest.mark.parametrize("case", [c for c in I.COMP_SAME if c[3] >= 0], ids=comp_id)
def test_compressor_items_passes_against_longdouble(crun, case):
    """fx_pass_ref.check_compressor, unchanged, through the per-item entry points"""
    L, n, Cn, forms, fused = case
    kw = dict(scale=I.COMP_SCALE[:n], sumsq=True) if fused else {}
    R.check_compressor(crun, L, n, Cn, *I.BASE, forms=forms, **kw)


def test_compressor_items_prepare_refuses_the_ill_conditioned_item(run):
    I.check_comp_refusal(run)


def test_compressor_process_items_reroutes_the_refused_item(emu_default):
    I.check_comp_python_reroute("cpu")


def test_every_items_kernel_is_launched_by_the_case_list(emu):
    from emu_binding import EMU_LIB
    seen = I.trace_items_cases(emu) | I.trace_comp_items_cases(emu)
    exported = I.exported_items_kernels(EMU_LIB)
    assert len(exported) >= 8 + 8 + 16 + 8 + 8 + 4 + 5, sorted(exported)          # ends, stereo ends, scans, two applies; tables, serial, imager, gain; five compressor kernels
    missing = sorted(exported - seen)
    assert not missing, "exported per-item FX kernels no case launches: " + ", ".join(missing)


# ---------------------------------------------------------------------------------------------------------- AugmentationChain.call_items
PROBS = {"eq": 0.7, "comp": 0.6, "pan": 0.5, "imager": 0.5, "reverb": 0.6, "gain": 0.8}


@pytest.mark.parametrize("inst", ["drums", "vocals"])
def test_call_items_plan_is_the_sequential_loops_draws(inst, monkeypatch):
    """No kernel runs.  The plan of call_items for n = 7 lists, per item, the processors, parameter values, rms flags and mix weights the loop
    `for i in range(7): chain([x[i]])` meets; afterwards both generators, the order of every fxs list and every parameter value are the loop's."""
    import random
    from music_mixing_style_transfer_amd.mixing_manipulator import common_audioeffects as A
    from music_mixing_style_transfer_amd.mixing_manipulator.audio_effects_chain import create_inst_effects_augmentation_chain
    build = lambda: I.tag_processors(create_inst_effects_augmentation_chain(inst, PROBS, algorithmic=True))
    a, b = build(), build()
    random.seed(123)
    np.random.seed(321)
    want = I.record_sequential_loop(a, 7, monkeypatch)
    state_a = (random.getstate(), np.random.get_state())
    random.seed(123)
    np.random.seed(321)
    got = I.plan_as_log(b.plan_items(7, 2))
    state_b = (random.getstate(), np.random.get_state())
    assert got == want
    assert sum(len(p) for p in want) > 14 and len({len(p) for p in want}) > 1, "the items took different routes"
    assert any(op[0] == "mix" for p in want for op in p)
    assert state_a[0] == state_b[0]
    assert state_a[1][0] == state_b[1][0] and np.array_equal(state_a[1][1], state_b[1][1]) and state_a[1][2:] == state_b[1][2:]
    assert I.fxs_order(a) == I.fxs_order(b)
    assert [A.parameter_values(f) for f in sorted(a._processors(), key=lambda f: f.tag)] == [A.parameter_values(f) for f in sorted(b._processors(), key=lambda f: f.tag)]


@pytest.mark.parametrize("probs", [(1.0, 1.0, 1.0, 1.0), (0.5, 0.5, 0.5, 0.5)], ids=["p1", "p05"])
def test_call_items_random_chain_vs_oracle(emu_default, oracle_fx_lib, probs):
    I.check_random_chain("cpu", I.oracle_compressor_fn(oracle_fx_lib), probs)


def test_process_items_match_process(emu_default):
    """Equaliser / Compressor / MidSideImager / Gain.process_items: item i is process() with item i's values on the same batch, bit for bit"""
    import torch
    from music_mixing_style_transfer_amd.mixing_manipulator import Compressor, Equaliser, Gain, MidSideImager
    from music_mixing_style_transfer_amd.mixing_manipulator.common_audioeffects import parameter_values
    import random
    random.seed(5)
    x = torch.from_numpy(I.stereo_input(4099, 3, 4))
    for fx in (Equaliser(2, 44100), MidSideImager(), Gain(), Compressor(44100)):
        values = []
        for _ in range(3):
            fx.randomize()
            values.append(parameter_values(fx))
        keep = parameter_values(fx)
        y = fx.process_items(x, values)
        assert parameter_values(fx) == keep
        for i, v in enumerate(values):
            for k, val in v.items():
                getattr(fx.parameters, k).value = val
            want = fx.process(x if not isinstance(fx, Compressor) else x[i:i + 1])
            assert I.same_bits(y[i].numpy(), want[i if not isinstance(fx, Compressor) else 0].numpy()), (type(fx).__name__, i)
