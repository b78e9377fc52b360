"""The training datasets' bookkeeping, no kernels (CPU only): against the real reference (tests/golden/trainbatch.npz: file names, start
points, parameter values and generator states of its own items), and the rules restated - both __len__ rules, the file globs, the
length-proportional file choice, the start points with the 2048-sample over-read, the seeding rule, the default probability tables with the
cumulative reverb weight, the output order, the refusal of worker processes and the file checks of the stem bank."""
import argparse
import os
import random

import numpy as np
import pytest
import torch

import trainbatch_ref as T


@pytest.fixture(scope="module")
def musdb(tmp_path_factory):
    return T.write_musdb_dir(tmp_path_factory.mktemp("musdb"))


def datasets():
    from music_mixing_style_transfer_amd import data_loader as D
    return D


@pytest.mark.parametrize("kind,pad,neg", T.GOLDEN_CASES)
def test_draws_equal_the_reference(musdb, kind, pad, neg):
    T.check_golden_bookkeeping(kind, pad, neg, musdb)


def test_names_are_exported_like_the_reference_star_import():
    D = datasets()
    for name in ("MUSDB_Dataset_Mixing_Manipulated_FXencoder", "MUSDB_Dataset_Mixing_Manipulated_Style_Transfer", "Collate_Variable_Length_Segments",
                 "Song_Dataset_Inference", "StemBank", "get_total_audio_length"):
        assert hasattr(D, name)
    from music_mixing_style_transfer_amd.mixing_manipulator.common_audioeffects import AugmentationChain
    assert callable(AugmentationChain.plan_one) and callable(AugmentationChain.call_plans)


def test_len_rules(musdb):
    D = datasets()
    args = T.make_args(musdb, batch_size_total=6, segment_length=2400)
    fx = D.MUSDB_Dataset_Mixing_Manipulated_FXencoder
    assert len(fx(args, "val", applying_effects="gain", device="cpu")) == 6
    os.makedirs(os.path.join(musdb, "train"), exist_ok=True)
    for inst in ("drums", "bass", "other", "vocals"):
        T.write_pcm_wav(os.path.join(musdb, "train", f"{inst}_normalized_{T.ORDER}_silence_trimmed_0.wav"), np.zeros((7000, 2)), 2)
    assert len(fx(args, "train", applying_effects="gain", device="cpu")) == 240
    st = D.MUSDB_Dataset_Mixing_Manipulated_Style_Transfer(args, "val", applying_effects="gain", device="cpu")
    assert len(st) == sum(T.FILE_FRAMES) // 2400          # the vocals files' frames over segment_length
    assert len(D.MUSDB_Dataset_Mixing_Manipulated_Style_Transfer(args, "train", applying_effects="gain", device="cpu")) == 7000 // 2400


def test_file_globs(tmp_path):
    """normalised: <inst>_normalized_<order>_silence_trimmed*.wav for both classes; otherwise <inst>_silence_trimmed*.wav (FXencoder) and
    <inst>_silence_trimmed.wav (Style_Transfer: no wildcard); sorted"""
    D = datasets()
    d = tmp_path / "val"
    d.mkdir()
    for inst in ("drums", "bass", "other", "vocals"):
        for name in (f"{inst}_silence_trimmed.wav", f"{inst}_silence_trimmed_b.wav", f"{inst}_silence_trimmed_a.wav", f"{inst}_normalized_{T.ORDER}_silence_trimmed_1.wav",
                     f"{inst}_normalized_other_silence_trimmed_1.wav", f"{inst}.wav"):
            T.write_pcm_wav(d / name, np.zeros((6000, 2)), 2)
    base = lambda ds, inst: [os.path.basename(p) for p in ds.data_paths[inst]]
    for use in (True, False):
        args = T.make_args(tmp_path, use_normalized=use)
        fx = D.MUSDB_Dataset_Mixing_Manipulated_FXencoder(args, "val", applying_effects="gain", device="cpu")
        st = D.MUSDB_Dataset_Mixing_Manipulated_Style_Transfer(args, "val", applying_effects="gain", device="cpu")
        for inst in ("drums", "vocals"):
            if use:
                assert base(fx, inst) == base(st, inst) == [f"{inst}_normalized_{T.ORDER}_silence_trimmed_1.wav"]
            else:
                assert base(fx, inst) == [f"{inst}_silence_trimmed.wav", f"{inst}_silence_trimmed_a.wav", f"{inst}_silence_trimmed_b.wav"]
                assert base(st, inst) == [f"{inst}_silence_trimmed.wav"]
    with pytest.raises(NotImplementedError):
        D.MUSDB_Dataset_Mixing_Manipulated_FXencoder(T.make_args(tmp_path, using_dataset="medleydb"), "val", applying_effects="gain", device="cpu")


@pytest.mark.parametrize("pad", [True, False])
def test_file_choice_and_start_points_restated(musdb, pad):
    """np.random.choice(paths, 2, p = length ratios), then torch.randint(0, frames - segment_length_ref [- 2 * 2048]) for A and for B"""
    D = datasets()
    args = T.make_args(musdb, pad_b4_manipulation=pad)
    ds = D.MUSDB_Dataset_Mixing_Manipulated_Style_Transfer(args, "val", applying_effects="gain", device="cpu")
    assert ds.pad_length == 2048 and ds.load_duration == 1200 + (4096 if pad else 0)
    total = sum(T.FILE_FRAMES)
    assert ds.data_length_ratio_list["bass"] == [n / total for n in T.FILE_FRAMES]
    for seed in range(5):
        np.random.seed(seed)
        torch.manual_seed(seed)
        got = ds._draw_segments("bass")
        np.random.seed(seed)
        torch.manual_seed(seed)
        chosen = np.random.choice(ds.data_paths["bass"], 2, p=ds.data_length_ratio_list["bass"])
        last = [T.FILE_FRAMES[ds.data_paths["bass"].index(p)] - 1200 - (4096 if pad else 0) for p in chosen]
        want = [int(torch.randint(low=0, high=last[0], size=(1,))[0]), int(torch.randint(low=0, high=last[1], size=(1,))[0])]
        assert got == ([str(p) for p in chosen], want)
        assert all(0 <= s <= n for s, n in zip(want, last))


def test_seeding_rule(musdb, monkeypatch):
    """outside train mode idx * random_seed; in train mode int(time.time()) * (idx + 1) % (2^32 - 1) - for all three generators"""
    D = datasets()
    from music_mixing_style_transfer_amd.data_loader import data_loader as DL

    def draws_after(seed):
        torch.manual_seed(seed)
        np.random.seed(seed)
        random.seed(seed)
        return T.next_draws()

    ds = D.MUSDB_Dataset_Mixing_Manipulated_FXencoder(T.make_args(musdb, random_seed=7), "val", applying_effects="gain", device="cpu")
    ds._seed(5)
    assert T.next_draws() == draws_after(35)
    ds.mode = "train"
    monkeypatch.setattr(DL.time, "time", lambda: 1700000123.9)
    ds._seed(5)
    assert T.next_draws() == draws_after(1700000123 * 6 % (2 ** 32 - 1))


def reverb_probabilities(chain):
    """the probability of every reverb entry of an instrument chain, in the order of the chain"""
    from music_mixing_style_transfer_amd.mixing_manipulator.common_audioeffects import AugmentationChain
    out = []
    for fx, p, _ in chain.fxs:
        if isinstance(fx, AugmentationChain):
            out.extend(reverb_probabilities(fx))
        elif "Reverb" in type(fx).__name__:
            out.append(p)
    return out


def top_probabilities(chain):
    from music_mixing_style_transfer_amd.mixing_manipulator.common_audioeffects import AugmentationChain
    out = {}
    for fx, p, _ in chain.fxs:
        if isinstance(fx, AugmentationChain):
            out.update(top_probabilities(fx))
        elif "Reverb" not in type(fx).__name__ and not (type(fx).__name__ == "Equaliser" and len(fx.bands) == 1):
            out[type(fx).__name__] = p
    return out


@pytest.mark.parametrize("kind", ["fxenc", "style"])
def test_default_probability_tables_and_cumulative_reverb_weight(musdb, kind):
    """defaults: eq 0.9, comp 0.9, pan 0.3, imager 0.8, gain 0.5; reverb: the drums' own 0.5, and from then on 'reverb' is in the dict and the
    weights multiply into it: bass 0.5 * 0.1, other and vocals * 1.0 (the reference as it stands).  A caller's dict is updated the same way."""
    cls = T.dataset_class(kind)
    ds = cls(T.make_args(musdb), "val", device="cpu")
    for inst in ds.instruments:
        assert top_probabilities(ds.mixing_manipulator[inst]) == {"Equaliser": 0.9, "Compressor": 0.9, "Panner": 0.3, "MidSideImager": 0.8, "Gain": 0.5}
    assert reverb_probabilities(ds.mixing_manipulator["drums"]) == [0.5 * 0.01, 0.5]          # below / above 100 Hz
    for inst in ("bass", "other", "vocals"):
        assert reverb_probabilities(ds.mixing_manipulator[inst]) == [0.5 * 0.1]
    mine = {"eq": 1.0, "comp": 0.5, "pan": 0.25, "imager": 0.125, "gain": 1.0, "reverb": 0.8}
    ds = cls(T.make_args(musdb), "val", apply_prob_dict=mine, device="cpu")
    assert reverb_probabilities(ds.mixing_manipulator["drums"]) == [0.8 * 0.5 * 0.01, 0.8 * 0.5]
    assert reverb_probabilities(ds.mixing_manipulator["vocals"]) == [0.8 * 0.5 * 0.1] and mine["reverb"] == 0.8 * 0.5 * 0.1
    assert top_probabilities(ds.mixing_manipulator["other"]) == {"Equaliser": 1.0, "Compressor": 0.5, "Panner": 0.25, "MidSideImager": 0.125, "Gain": 1.0}


def test_collate_orders_a_plain_list_like_the_reference():
    """items of labelled constants: the two collate methods pick the reference's rows, lengths and starts (restated)"""
    D = datasets()
    args = argparse.Namespace(segment_length=64, reference_length=64, num_strong_negatives=1, using_dataset="MUSDB18")
    c = D.Collate_Variable_Length_Segments(args)
    L, n = 64, 3
    ramp = torch.arange(L, dtype=torch.float32)
    item = lambda b, rows: [torch.stack([1000 * b + 10 * j + ramp / 100, -(1000 * b + 10 * j + ramp / 100)]) for j in range(rows)]
    batch = [item(b, 16) for b in range(n)]
    torch.manual_seed(11)
    out_a, out_b = c.random_duration_segments_strong_negatives(batch)
    torch.manual_seed(11)
    la, lb = (int(v) for v in torch.randint(low=L // 2, high=L, size=(2,)))
    for b in range(n):
        sa = int(torch.randint(low=0, high=L - la, size=(1,))[0])
        sb = int(torch.randint(low=0, high=L - lb, size=(1,))[0])
        for i in range(4):
            for neg in range(2):
                assert torch.equal(out_a[i][b * 2 + neg], batch[b][i * 4 + 2 * neg][:, sa:sa + la])
                assert torch.equal(out_b[i][b * 2 + neg], batch[b][i * 4 + 2 * neg + 1][:, sb:sb + lb])
    assert len(out_a) == len(out_b) == 4 and out_a[0].shape == (6, 2, la) and out_b[3].shape == (6, 2, lb)
    a1, a2, b2 = c.style_transfer_collate([item(b, 12) for b in range(n)])
    for i in range(4):
        for j, lst in enumerate((a1, a2, b2)):
            assert lst[i].shape == (n, 2, L) and [float(lst[i][b, 0, 0]) for b in range(n)] == [1000 * b + 10 * (3 * i + j) for b in range(n)]
    with pytest.raises(NotImplementedError):
        D.Collate_Variable_Length_Segments(argparse.Namespace(segment_length=1, reference_length=1, num_strong_negatives=0, using_dataset="other"))


def test_worker_processes_are_refused(musdb, monkeypatch):
    D = datasets()
    ds = D.MUSDB_Dataset_Mixing_Manipulated_FXencoder(T.make_args(musdb), "val", applying_effects="gain", device="cpu")
    monkeypatch.setattr(torch.utils.data, "get_worker_info", lambda: argparse.Namespace(id=1))
    for call in (lambda: ds[0], lambda: ds.get_batch([0]),
                 lambda: D.Collate_Variable_Length_Segments(T.make_args(musdb)).style_transfer_collate([[torch.zeros(2, 4)] * 12])):
        with pytest.raises(RuntimeError, match="num_workers=0"):
            call()


def test_stem_bank_file_checks(tmp_path):
    T.check_stem_bank_refuses_files(tmp_path)
