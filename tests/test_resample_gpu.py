"""The polyphase resampler on the MI355X: the checks of tests/test_resample_emu.py on the device (tests/resample_ref.py), the bound also at
65 537 frames, and the flag through the loaders, the dataset and the two command lines with tiny synthetic networks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import resample_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

from music_mixing_style_transfer_amd import _lib  # noqa: E402
from music_mixing_style_transfer_amd.mixing_manipulator import _device_ops as D  # noqa: E402

DEV = "cuda:0"
RATIOS = list(R.RATIOS)
ENC_CFG = {"channels": [4, 8, 16], "kernels": [5, 4, 3], "strides": [2, 2, 1], "dilation": [1, 1, 1], "bias": True, "norm": "batch",
           "conv_block": "res", "activation": "relu"}
TCN_CFG = {"condition_dimension": 16, "nblocks": 4, "dilation_growth": 2, "kernel_size": 5, "channel_width": 8, "stack_size": 15,
           "causal": False}


def test_taps_info_and_length():
    assert _lib.lib().path.endswith("libmst_hip.so") and _lib.lib().mst_version() >= 101
    R.check_taps(D)


@pytest.mark.parametrize("Cn", [1, 2])
@pytest.mark.parametrize("up,down", RATIOS)
def test_every_output_within_the_bound(up, down, Cn):
    for n in (1, 7, 129, 3001, 65537):
        R.check_bound(D, DEV, up, down, n, Cn)


@pytest.mark.parametrize("up,down", RATIOS)
def test_restatement_against_scipy_resample_poly(up, down):
    R.check_scipy(D, up, down)


@pytest.mark.parametrize("up,down", RATIOS)
def test_impulse_returns_the_taps_and_silence_zeros(up, down):
    R.check_impulse_and_silence(D, DEV, up, down)


@pytest.mark.parametrize("up,down", RATIOS)
def test_bit_identical_alone_in_a_batch_and_from_run_to_run(up, down):
    R.check_determinism(D, DEV, up, down)
    R.check_determinism(D, DEV, up, down, n=65537)


@pytest.mark.parametrize("up,down", RATIOS)
def test_chunks_give_the_bits_of_one_call(up, down):
    R.check_chunks(D, DEV, up, down)


def test_refusals():
    x, y = torch.zeros(64, device=DEV), torch.zeros(64, device=DEV)
    R.check_refusals(_lib.lib(), x.data_ptr(), y.data_ptr(), _lib.lib().stream_ptr(x))
    with pytest.raises(NotImplementedError, match="44101"):
        D.resample(torch.zeros(10, 2, device=DEV), 44100, 44101)
    with pytest.raises(RuntimeError, match="no CPU path"):
        D.Resampler.get(48000, 44100).forward(torch.zeros(1, 10, 2))


def test_python_wrapper_keeps_rank_and_place():
    x = torch.from_numpy(R.noise(500, 2, 9))
    yd, yh = D.resample(x.to(DEV), 48000, 44100), D.resample(x, 48000, 44100)          # a host tensor travels and comes back
    assert yd.is_cuda and not yh.is_cuda and tuple(yd.shape) == (460, 2) and torch.equal(yd.cpu(), yh)
    assert torch.equal(D.resample(x[None].to(DEV), 48000, 44100)[0], yd)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        other = D.resample(x.to(DEV), 48000, 44100)
    s.synchronize()
    assert torch.equal(other, yd)


def test_tones_through_48_to_44k1():
    R.check_tones(D, DEV)


def test_true_peak_of_the_4x_oversampler():
    R.check_true_peak(D, DEV)


def test_loaders_convert(tmp_path):
    R.check_loaders(D, DEV, tmp_path)


def test_dataset_stacks_stems_of_two_rates(tmp_path):
    R.check_dataset(D, DEV, tmp_path)


def _checkpoints(tmp_path):
    from music_mixing_style_transfer_amd.utils import synth
    synth.save_reference_format_checkpoint(str(tmp_path / "enc.pt"), synth.fxencoder_state_dict(ENC_CFG, seed=3))
    synth.save_reference_format_checkpoint(str(tmp_path / "tcn.pt"), synth.tcn_state_dict(nblocks=4, kernel_size=5, channel_width=8, cond_dim=16,
                                                                                          seed=5))


def test_style_transfer_cli_with_reference_stems_at_48k(tmp_path):
    import copy
    from music_mixing_style_transfer_amd.data_loader import load_wav_length
    from music_mixing_style_transfer_amd.inference import style_transfer as st
    from music_mixing_style_transfer_amd.inference.engine import StyleTransferEngine
    _checkpoints(tmp_path)
    refs = R.write_song(tmp_path / "data")
    seg_len = 16384

    def runner(extra):
        args = st.build_parser().parse_args([
            "--target_dir", str(tmp_path / "data") + "/", "--output_dir", str(tmp_path / "out") + "/", "--ckpt_path_enc", str(tmp_path / "enc.pt"),
            "--ckpt_path_conv", str(tmp_path / "tcn.pt"), "--do_not_separate", "True", "--normalize_input", "False", "--segment_length",
            str(seg_len), "--segment_length_ref", str(seg_len), "--save_each_inst", "True"] + extra)
        args.cfg_encoder, args.cfg_converter = copy.deepcopy(ENC_CFG), dict(TCN_CFG)
        return st.Mixing_Style_Transfer_Inference(args)

    with pytest.raises(ValueError, match="sample rate should be 44100"):
        runner([]).inference()
    seen, plain = [], StyleTransferEngine.stem_embedding

    def recording(self, reference_stem, *a, **k):
        emb = plain(self, reference_stem, *a, **k)
        seen.append(emb.clone())
        return emb
    run = runner(["--convert_input", "True"])
    StyleTransferEngine.stem_embedding = recording
    try:
        run.inference()
    finally:
        StyleTransferEngine.stem_embedding = plain
    names = sorted(os.listdir(tmp_path / "out" / "song0"))
    assert names == sorted([f"{s}_output_notnormed.wav" for s in R.STEMS] + ["mixture_output_notnormed.wav"])
    for k in names:
        assert load_wav_length(str(tmp_path / "out" / "song0" / k)) == 30000          # the input's length, at 44.1 kHz
    assert len(seen) == 4
    eng = run._engine()
    for s, emb in zip(R.STEMS, seen):
        stem = D.resample(torch.from_numpy((refs[s] / 32768.0).astype(np.float32)).to(DEV), 48000, 44100).clamp(-1, 1).t().contiguous()
        assert torch.equal(plain(eng, stem, seg_len, seg_len, "song0"), emb), s


def test_feature_extraction_cli_with_a_48k_file(tmp_path):
    import copy
    from music_mixing_style_transfer_amd.inference import feature_extraction as fe
    _checkpoints(tmp_path)
    d = tmp_path / "songs" / "a"
    d.mkdir(parents=True)
    pcm = R.pcm_noise(50001, 2, 8)
    R.write_wav(d / "mix.wav", pcm, 48000, 2)

    def runner(extra):
        args = fe.build_parser().parse_args(["--target_dir", str(tmp_path / "songs") + "/", "--ckpt_path_enc", str(tmp_path / "enc.pt"),
                                             "--segment_length", "20000", "--batch_size", "2"] + extra)
        args.cfg_encoder = copy.deepcopy(ENC_CFG)
        return fe.FXencoder_Inference(args)

    with pytest.raises(ValueError, match="sample rate should be 44100"):
        runner([]).save_averaged_embeddings()
    assert not os.path.exists(d / "mix_fx_embedding.npy")
    run = runner(["--convert_input", "True"])
    run.save_averaged_embeddings()
    emb = np.load(str(d / "mix_fx_embedding.npy"))
    song = D.resample(torch.from_numpy((pcm / 32768.0).astype(np.float32)), 48000, 44100).t().contiguous()
    assert emb.shape == (16,) and np.array_equal(emb, run.embed_song(song, "mix"))
