"""The polyphase resampler (csrc/resample_kernels.h) on the CPU SIMT emulator: taps against scipy.signal.firwin, every output against the
float64 restatement within the derived bound (tests/resample_ref.py), exact impulse responses and zeros, bit identity alone / in a batch /
in chunks / 2^30 periods on, the refusals, the analytic anchors, and the loaders and the dataset with convert=True."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import resample_ref as R  # noqa: E402

from music_mixing_style_transfer_amd.mixing_manipulator import _device_ops as D  # noqa: E402

DEV = "cpu"          # the emulator's device memory is host memory
RATIOS = list(R.RATIOS)


def test_taps_info_and_length(emu_default):
    assert emu_default.mst_version() >= 101
    R.check_taps(D)


@pytest.mark.parametrize("up,down", RATIOS)
def test_every_output_within_the_bound(emu_default, up, down):
    for n in (1, 7, 129, 3001):
        for Cn in (1, 2):
            R.check_bound(D, DEV, up, down, n, Cn)


@pytest.mark.parametrize("up,down", RATIOS)
def test_restatement_against_scipy_resample_poly(emu_default, up, down):
    R.check_scipy(D, up, down)


@pytest.mark.parametrize("up,down", RATIOS)
def test_impulse_returns_the_taps_and_silence_zeros(emu_default, up, down):
    R.check_impulse_and_silence(D, DEV, up, down)


@pytest.mark.parametrize("up,down", RATIOS)
def test_bit_identical_alone_in_a_batch_and_from_run_to_run(emu_default, up, down):
    R.check_determinism(D, DEV, up, down)


@pytest.mark.parametrize("up,down", RATIOS)
def test_chunks_give_the_bits_of_one_call(emu_default, up, down):
    R.check_chunks(D, DEV, up, down)


def test_refusals(emu_default):
    x, y = torch.zeros(64), torch.zeros(64)
    R.check_refusals(emu_default, x.data_ptr(), y.data_ptr(), C.c_void_p(0))
    with pytest.raises(NotImplementedError, match="44101"):
        D.resample(torch.zeros(10, 2), 44100, 44101)
    with pytest.raises(ValueError, match="C = 3"):
        D.resample(torch.zeros(10, 3), 48000, 44100)


def test_python_wrapper_shapes(emu_default):
    x = torch.from_numpy(R.noise(500, 2, 9))
    y3, y2 = D.resample(x[None], 48000, 44100), D.resample(x, 48000, 44100)
    assert tuple(y3.shape) == (1, 460, 2) and tuple(y2.shape) == (460, 2) and torch.equal(y3[0], y2)
    assert torch.equal(D.resample(x.double(), 48000, 44100), y2)          # any float dtype in, float32 out
    assert torch.equal(D.resample(x, 44100, 44100), x)
    assert D.Resampler.get(48000, 44100) is D.Resampler.get(48000, 44100)


def test_tones_through_48_to_44k1(emu_default):
    R.check_tones(D, DEV)


def test_true_peak_of_the_4x_oversampler(emu_default):
    R.check_true_peak(D, DEV)


def test_loaders_convert(emu_default, tmp_path):
    R.check_loaders(D, DEV, tmp_path)


def test_dataset_stacks_stems_of_two_rates(emu_default, tmp_path):
    R.check_dataset(D, DEV, tmp_path)


def test_command_line_flag_defaults_off():
    from music_mixing_style_transfer_amd.inference import feature_extraction as fe
    from music_mixing_style_transfer_amd.inference import style_transfer as st
    for mod in (st, fe):
        p = mod.build_parser()
        assert p.parse_args([]).convert_input is False and p.parse_args(["--convert_input", "True"]).convert_input is True
