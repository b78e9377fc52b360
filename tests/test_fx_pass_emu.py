"""The time-parallel equaliser and compressor (csrc/fx_kernels.h fx_biquad_* / fx_comp_*) pass by pass on the CPU emulator against an
operand-exact longdouble reference: every float64 intermediate the passes leave in the caller's scratch buffer (chunk end / start states; chunk
maps, chunk start values, carry, tile sums), every output sample and the chain fusion's energy by-products, each within a bound computed
beside it (tests/fx_pass_ref.py; constants and measured ratios in DESIGN.md section 5).  The same cases run on the MI355X in
tests/test_fx_pass_gpu.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fx_pass_ref as R
from music_mixing_style_transfer_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def run(emu):
    return R.Runner(emu, "cpu")


def test_longdouble_is_extended_and_the_two_pass_reference_is_the_serial_one(run):
    """The reference runs chunk-parallel in longdouble (zero-state pass, serial scan with A^M, chunks from their true states) to keep the
    Python loop over M steps; against one serial longdouble run over the whole signal it differs by longdouble rounding only."""
    R.assert_longdouble()
    for name, L, n, Cn in (("config4", 1000, 2, 2), ("butter16", 1500, 1, 3)):
        plan = run.eq_plan(n, L, Cn, R.coef_sets()[name].shape[0])
        _, ref = R.eq_reference((name, L, n, Cn, None, 0, plan.M))
        s = ref.serial()
        assert float(np.abs(s - ref.v).max()) <= 2.0 ** -55 * float(np.abs(s).max())


@pytest.mark.parametrize("case", R.EQ_CASES, ids=R.eq_id)
def test_equaliser_passes(run, case):
    R.check_equaliser(run, **case)


@pytest.mark.parametrize("case", R.COMP_CASES, ids=R.comp_id)
def test_compressor_passes(run, case):
    R.check_compressor(run, **case)


@pytest.mark.parametrize("k", range(1, 9))
def test_equaliser_forms_stay_bit_identical(run, k):
    R.check_forms_identical(run, k)


def test_constants_cover_the_float64_restatement(run):
    """Every constant of the bounds is at least four times the worst err / bound of the float64 restatement of its pass over the whole case
    list (and a power of two, at least 1): the constants never come from a kernel's error."""
    worst = {}
    for c in R.EQ_CASES:
        for k, v in R.eq_restatement_ratios(run, c).items():
            worst["eq " + k] = max(worst.get("eq " + k, 0.0), v)
    for c in R.COMP_CASES:
        for k, v in R.comp_restatement_ratios(run, c).items():
            worst["comp " + k] = max(worst.get("comp " + k, 0.0), v)
    print("float64 restatement, worst err / bound at constant 1:", {k: round(v, 4) for k, v in worst.items()})
    for key, c in (("eq table", R.C_TAB), ("eq powers", R.C_POW), ("eq ends", R.C_ENDS), ("eq starts", R.C_STARTS), ("eq v", R.C_V), ("comp xl", R.C_XL), ("comp maps", R.C_MAP),
                   ("comp ystart", R.C_YL), ("comp yl", R.C_YL)):
        assert c >= 1.0 and np.log2(c) == int(np.log2(c)) and 4.0 * worst[key] <= c, (key, worst[key], c)


def test_fast_attack_is_right_through_every_public_path(emu_default):
    R.check_fast_attack_public_paths(R.Runner(emu_default, "cpu"))


def test_ill_conditioned_fused_and_grid_calls_are_refused(run):
    R.check_refusals(run)


def test_plan_queries(run):
    """host-only, refuse a struct of another layout, agree with the scratch sizes"""
    lib = run.lib
    assert lib.mst_version() >= 102
    import ctypes as C
    p = _lib.MstFxBiquadPlan()
    p.struct_size = 4
    assert lib.mst_fx_biquad_plan(1, 100, 2, 5, C.byref(p)) == -1
    q = _lib.MstFxCompressorPlan()
    q.struct_size = 4
    assert lib.mst_fx_compressor_plan(1, 100, 2, 1.0, 100.0, 44100.0, 0, C.byref(q)) == -1
    for n, L, Cn in ((1, 97, 2), (3, 5000, 1), (64, 131072, 2)):
        q = run.comp_plan(n, L, Cn, 2.0, 100.0)
        assert q.total_bytes == lib.mst_fx_compressor_scratch_bytes(n, L, Cn) and q.form == _lib.FX_COMP_TIME_PARALLEL
        p = run.eq_plan(n, L, Cn, 5)
        assert 2 * p.starts_offset + 9 * 4 * 64 * 8 == lib.mst_fx_biquad_scratch_bytes(n, L, Cn, 5)
    # the product's randomised ranges (1 .. 20 ms, 50 .. 500 ms) stay time-parallel at every rate the loaders accept
    for sr in (22050.0, 44100.0, 48000.0, 96000.0):
        for att in (1.0, 20.0):
            for rel in (50.0, 500.0):
                assert run.comp_plan(64, 131072, 2, att, rel, sr).form == _lib.FX_COMP_TIME_PARALLEL


def test_every_fx_pass_kernel_is_launched_by_the_case_list(emu):
    """Every exported instantiation of the equaliser / compressor kernels is launched by the case list (the emulator's dry-run launch trace):
    the GPU file runs the same list.  fx_log10_table_kernel runs once per process, in front of the first time-parallel compressor call: a
    fresh process shows it."""
    from emu_binding import EMU_LIB
    run = R.Runner(emu, "cpu")
    c = R.COMP_CASES[0]
    R.check_compressor(run, **c, log=lambda s: None)                                   # the log10 table of THIS process is built by a real launch first
    seen = R.trace_cases(emu)
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "import numpy as np, fx_pass_ref as R\nfrom emu_binding import bind_emulator\n"
            "emu = bind_emulator(build=False); tr = R.Tracer(emu); run = R.Runner(emu, 'cpu')\n"
            "with tr:\n    R._comp_call(run, np.zeros((1, 200, 2), np.float32), -30.0, 2.0, 100.0, 4.0, 44100.0, None, False, 0, True, False, False)\n"
            "print('\\n'.join(sorted(tr.seen)))\n") % (REPO, os.path.join(REPO, "tests"))
    first = subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True).stdout.split()
    seen.update(first)
    exported = R.exported_fx_kernels(EMU_LIB)
    assert len(exported) >= 60, sorted(exported)          # 4 x 8 band counts, 16 scans, 12 single kernels
    missing = sorted(exported - seen)
    assert not missing, "exported FX kernels no case launches: " + ", ".join(missing)
    assert any("fx_log10_table_kernel" in s for s in first)
    # every distinct template, all eight band counts of the biquad kernels
    for tmpl, count in (("fx_biquad_chunk_kernel", 8), ("fx_biquad_ends_kernel", 8), ("fx_biquad_stereo_ends_kernel", 8), ("fx_biquad_stereo_apply_kernel", 8),
                        ("fx_biquad_scan_kernel", 16), ("fx_biquad_stereo_ends_mfma_kernel", 1), ("fx_biquad_kernel", 1), ("fx_comp_map_kernel", 2),
                        ("fx_comp_apply_kernel", 2), ("fx_comp_chain_kernel", 1), ("fx_comp_gain_kernel", 1), ("fx_comp_smooth_kernel", 1),
                        ("fx_compressor_kernel", 1), ("fx_tile_sums_kernel", 1)):
        got = {s for s in seen if s.startswith(f"_Z{len(tmpl)}{tmpl}")}          # the mangled name carries the length: no longer name matches
        assert len(got) == count, (tmpl, sorted(got))
