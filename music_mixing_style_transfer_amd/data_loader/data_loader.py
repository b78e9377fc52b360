"""The reference's datasets (data_loader/data_loader.py): the two MUSDB training datasets and their collate class (below the imports), and the
inference dataset (:545-603, Song_Dataset_Inference): for every song
directory <target_dir>/<song>/ load the 4 stems of the input and of the reference track(s) from
<song>/<stem_level_directory_name>[/<separation_model>]/<input|reference>/<stem>.wav, clamp to [-1, 1] and stack to
[4, 2, L] float32 tensors.

When args.normalize_input is set (the reference CLI's default) the INPUT stems go through the FX normaliser
(Audio_Effects_Normalizer, mixing_manipulator/data_normalization.py) with the features file
args.precomputed_normalization_feature and the effect order args.normalization_order (reference :559-563, :586-587).
"""
import os
import random
import time
from glob import glob

import numpy as np
import torch

from .loader_utils import (StemBank, batch_finish, get_total_audio_length, load_wav_device, load_wav_length, load_wav_segment,
                           read_wav_raw)

# ---------------------------------------------------------------------------------------------------------------------------------
# Training batches (reference data_loader/data_loader.py: Collate_Variable_Length_Segments :33-102,
# MUSDB_Dataset_Mixing_Manipulated_FXencoder :115-287, MUSDB_Dataset_Mixing_Manipulated_Style_Transfer :356-539).
#
# The datasets keep the reference's constructor arguments, file globs, length rules, seeding rule, probability tables, draws (from
# `random`, `np.random` and torch's CPU generator, in its order) and output order.  `ds[idx]` is the reference's item: two segments cut on
# the host, one chain call, a few torch ops - returned as device tensors.  `ds.get_batch(indices, collate)` builds what
# `collate([ds[i] for i in indices])` returns on the device: the draws of the whole loop first (no draw depends on the audio), then per
# instrument one gather out of the resident StemBank and one AugmentationChain.call_plans(group=2) over all rows of all negatives, then
# one finishing launch per output list (crop of the over-read, the collate's crop, transpose, clamp).
# Not here: the val-mode disk cache of manipulated wavs and generate_contents_w_effects; DataLoader worker processes (refused).
# ---------------------------------------------------------------------------------------------------------------------------------
INSTRUMENTS = ["drums", "bass", "other", "vocals"]


def _refuse_worker_process(what):
    info = torch.utils.data.get_worker_info()
    if info is not None:
        raise RuntimeError(f"{what}: called in DataLoader worker process {info.id}: the batches are built on the device by the process that "
                           "owns it - use num_workers=0 (or get_batch)")


class Collate_Variable_Length_Segments:
    """The reference's collate functions.  Both methods take the plain list of items (so that the class can stand behind a
    torch.utils.data.DataLoader with num_workers=0); handed to `dataset.get_batch(indices, collate=...)` their draws and crops become part of
    the batch's one finishing launch per output list."""

    def __init__(self, args):
        self.segment_length = args.segment_length
        self.random_length = args.reference_length
        self.num_strong_negatives = args.num_strong_negatives
        if "musdb" in args.using_dataset.lower():
            self.instruments = list(INSTRUMENTS)
        else:
            raise NotImplementedError

    def draw_random_durations(self, max_length, n_items):
        """the draws of random_duration_segments_strong_negatives for n_items items of max_length samples, in its order
        -> (length_a, length_b, [start_a per item], [start_b per item])"""
        min_length = max_length // 2
        length_a, length_b = (int(v) for v in torch.randint(low=min_length, high=max_length, size=(2,)))
        starts_a, starts_b = [], []
        for _ in range(n_items):
            starts_a.append(int(torch.randint(low=0, high=max_length - length_a, size=(1,))[0]))
            starts_b.append(int(torch.randint(low=0, high=max_length - length_b, size=(1,))[0]))
        return length_a, length_b, starts_a, starts_b

    def random_duration_segments_strong_negatives(self, batch):
        """trim segments A and B to two random durations (:46-75) -> [drums_A, bass_A, other_A, vocals_A], [drums_B, ...], each
        [len(batch) * (num_strong_negatives + 1), 2, length]"""
        _refuse_worker_process("Collate_Variable_Length_Segments")
        k = self.num_strong_negatives + 1
        la, lb, sa, sb = self.draw_random_durations(batch[0][0].shape[-1], len(batch))
        out_a, out_b = [[] for _ in self.instruments], [[] for _ in self.instruments]
        for item, a, b in zip(batch, sa, sb):
            for i in range(len(self.instruments)):
                for neg in range(k):
                    out_a[i].append(item[i * k * 2 + 2 * neg][:, a:a + la])
                    out_b[i].append(item[i * k * 2 + 1 + 2 * neg][:, b:b + lb])
        return [torch.stack(s, dim=0) for s in out_a], [torch.stack(s, dim=0) for s in out_b]

    def style_transfer_collate(self, batch):
        """(:79-102) -> [drums_A1, bass_A1, other_A1, vocals_A1], [..._A2], [..._B2], each [len(batch), 2, length]"""
        _refuse_worker_process("Collate_Variable_Length_Segments")
        out = [[[] for _ in self.instruments] for _ in range(3)]
        for item in batch:
            for i in range(len(self.instruments)):
                for j in range(3):
                    out[j][i].append(item[i * 3 + j])
        return tuple([torch.stack(s, dim=0) for s in lists] for lists in out)


class _MUSDB_Manipulated:
    """What the two training datasets share: paths, length ratios, the instrument chains, the resident stem banks, the draws of an item."""
    PAD_LENGTH = 2048

    def __init__(self, args, mode, applying_effects="full", apply_prob_dict=None, device=None):
        from ..mixing_manipulator.audio_effects_chain import create_effects_augmentation_chain, create_inst_effects_augmentation_chain
        self.args = args
        self.data_dir = args.data_dir + mode + "/"
        self.mode = mode
        self.applying_effects = applying_effects
        self.normalization_order = args.normalization_order
        self.fixed_random_seed = args.random_seed
        self.pad_b4_manipulation = args.pad_b4_manipulation
        self.pad_length = self.PAD_LENGTH
        self.device = torch.device("cuda" if device is None else device)
        if "musdb" in args.using_dataset.lower():
            self.instruments = list(INSTRUMENTS)
        else:
            raise NotImplementedError
        self.data_paths, self.data_length_ratio_list, self.banks, self._index, self._length = {}, {}, {}, {}, {}
        for inst in self.instruments:
            # sorted: the reference takes the order the file system returns
            self.data_paths[inst] = sorted(glob(self._pattern(inst)))
            total = get_total_audio_length(self.data_paths[inst])
            self._length.update({p: load_wav_length(p) for p in self.data_paths[inst]})
            self.data_length_ratio_list[inst] = [self._length[p] / total for p in self.data_paths[inst]]
            self._index[inst] = {p: i for i, p in enumerate(self.data_paths[inst])}
        self.mixing_manipulator = {}
        if applying_effects == "full":
            if apply_prob_dict is None:          # initial (default) applying probabilities of each FX
                apply_prob_dict = {"eq": 0.9, "comp": 0.9, "pan": 0.3, "imager": 0.8, "gain": 0.5}
                reverb_prob = {"drums": 0.5, "bass": 0.01, "vocals": 0.9, "other": 0.7}
            for inst in self.data_paths.keys():
                # the reference's rule as it stands: once 'reverb' is in the dict (from the second instrument on, with the default tables) the
                # weights multiply cumulatively into the caller's dict
                if "reverb" in apply_prob_dict.keys():
                    apply_prob_dict["reverb"] *= 0.5 if inst == "drums" else 0.1 if inst == "bass" else 1.0
                else:
                    apply_prob_dict["reverb"] = reverb_prob[inst]
                self.mixing_manipulator[inst] = create_inst_effects_augmentation_chain(inst, apply_prob_dict=apply_prob_dict,
                                                                                       ir_dir_path=args.ir_dir_path, sample_rate=args.sample_rate)
        else:                                    # single effects
            if not isinstance(applying_effects, list):
                applying_effects = [applying_effects]
            for inst in self.data_paths.keys():
                self.mixing_manipulator[inst] = create_effects_augmentation_chain(applying_effects, ir_dir_path=args.ir_dir_path)
        self.last_records = []                   # the draws of the last ds[idx] / get_batch, one record per index (see _draw_item)

    def _bank(self, inst):
        """the instrument's files as resident PCM, read at the first batch that needs them"""
        if inst not in self.banks:
            self.banks[inst] = StemBank(self.data_paths[inst], self.device, sample_rate=self.args.sample_rate,
                                        max_resident_bytes=getattr(self.args, "max_resident_bytes", None))
        return self.banks[inst]

    def _seed(self, idx):
        if self.mode == "train":
            torch.manual_seed(int(time.time()) * (idx + 1) % (2 ** 32 - 1))
            np.random.seed(int(time.time()) * (idx + 1) % (2 ** 32 - 1))
            random.seed(int(time.time()) * (idx + 1) % (2 ** 32 - 1))
        else:                                    # fixed random seed for evaluation
            torch.manual_seed(idx * self.fixed_random_seed)
            np.random.seed(idx * self.fixed_random_seed)
            random.seed(idx * self.fixed_random_seed)

    @property
    def load_duration(self):
        return self.args.segment_length_ref + self.pad_length * 2 if self.pad_b4_manipulation else self.args.segment_length_ref

    def _draw_segments(self, inst):
        """the file choice and the two start points of one instrument, the reference's draws -> (paths [2], starts [2])"""
        paths = self.data_paths[inst]
        chosen = np.random.choice(paths, 2, p=self.data_length_ratio_list[inst])
        last = [self._length[str(p)] - self.args.segment_length_ref for p in chosen]
        if self.pad_b4_manipulation:             # simply load more data to prevent artifacts likely to be caused by the manipulator
            last = [v - self.pad_length * 2 for v in last]
        start_a = int(torch.randint(low=0, high=last[0], size=(1,))[0])
        start_b = int(torch.randint(low=0, high=last[1], size=(1,))[0])
        return [str(p) for p in chosen], [start_a, start_b]

    def _draw_item(self, idx):
        """Every draw of ds[idx] without touching audio -> {inst: {"paths", "starts", "plans": one plan per chain call}}"""
        self._seed(idx)
        rec = {}
        for inst in self.data_paths.keys():
            paths, starts = self._draw_segments(inst)
            plans = [self.mixing_manipulator[inst].plan_one(2) for _ in range(self.n_chain_calls)]
            rec[inst] = {"paths": paths, "starts": starts, "plans": plans}
        return rec

    def _finish_item(self, seg):
        """[Lp, 2] on the device -> the reference's tail: crop the over-read, transpose, clamp"""
        if self.pad_b4_manipulation:
            seg = seg[self.pad_length:-self.pad_length]
        return torch.clamp(torch.transpose(seg.float(), 1, 0), min=-1, max=1)

    def _load_pair(self, paths, starts):
        return [torch.from_numpy(load_wav_segment(p, start_point=s, duration=self.load_duration, axis=1, sample_rate=self.args.sample_rate))
                .float().to(self.device) for p, s in zip(paths, starts)]

    def _chain_pair(self, inst, rec, seg_a, seg_b):
        """the reference's `chain([A, B])`: one set of draws for the two segments (kept in the record)"""
        chain = self.mixing_manipulator[inst]
        rec[inst]["plans"].append(chain.plan_one(2))
        return chain.call_plans(torch.stack([seg_a, seg_b], 0), rec[inst]["plans"][-1:], group=2).unbind(0)

    def _gather(self, records):
        """per instrument [2 len(records), Lp, 2]: rows 2b, 2b + 1 = segments A, B of record b - one launch per instrument"""
        out = {}
        for inst in self.data_paths.keys():
            files = [self._index[inst][p] for rec in records for p in rec[inst]["paths"]]
            starts = [s for rec in records for s in rec[inst]["starts"]]
            out[inst] = self._bank(inst).gather(files, starts, self.load_duration)
        return out

    def _manipulate(self, records, segments):
        """per instrument [len(records) * n_chain_calls * 2, Lp, 2]: rows ((b, call), A / B) - one call_plans over all rows of all calls"""
        out, k = {}, self.n_chain_calls
        for inst, x in segments.items():
            if k > 1:
                x = x.view(len(records), 1, 2, x.shape[1], 2).expand(-1, k, -1, -1, -1).reshape(-1, x.shape[1], 2)
            plans = [p for rec in records for p in rec[inst]["plans"]]
            out[inst] = self.mixing_manipulator[inst].call_plans(x, plans, group=2)
        return out

    def _finish(self, x, rows, starts, length, split):
        """one finishing launch -> `split` tensors [len(rows) / split, 2, length] (views of its output)"""
        return list(batch_finish(x, rows, starts, length).chunk(split, dim=0))


class MUSDB_Dataset_Mixing_Manipulated_FXencoder(_MUSDB_Manipulated):
    """Data for the contrastive training of the FXencoder (:115-287): two random segments A and B of every instrument, manipulated by
    1 + num_strong_negatives parameter sets.  Item: drums_A1, drums_B1, drums_A2, drums_B2, ..., bass_A1, ... - [2, segment_length_ref]
    float32 on the device, clamped to [-1, 1].  'full' calls create_inst_effects_augmentation_chain (the reference names a function that
    does not exist there)."""

    def _pattern(self, inst):
        return f"{self.data_dir}{inst}_normalized_{self.normalization_order}_silence_trimmed*.wav" if self.args.use_normalized \
            else f"{self.data_dir}{inst}_silence_trimmed*.wav"

    @property
    def n_chain_calls(self):
        return self.args.num_strong_negatives + 1

    def __len__(self):
        return self.args.batch_size_total * 40 if self.mode == "train" else self.args.batch_size_total

    def __getitem__(self, idx):
        _refuse_worker_process(type(self).__name__)
        self._seed(idx)
        rec, by_neg = {}, [{} for _ in range(self.n_chain_calls)]
        for inst in self.data_paths.keys():
            paths, starts = self._draw_segments(inst)
            seg_a, seg_b = self._load_pair(paths, starts)
            rec[inst] = {"paths": paths, "starts": starts, "plans": []}
            for neg in range(self.n_chain_calls):
                a, b = self._chain_pair(inst, rec, seg_a, seg_b)
                by_neg[neg][inst] = [self._finish_item(a), self._finish_item(b)]
        self.last_records = [rec]
        return [t for inst in self.data_paths.keys() for neg in range(self.n_chain_calls) for t in by_neg[neg][inst]]

    def get_batch(self, indices, collate=None):
        """What collate([self[i] for i in indices]) returns (collate None: the list of items), with that loop's draws, built on the device."""
        _refuse_worker_process(type(self).__name__)
        records = [self._draw_item(i) for i in indices]
        self.last_records = records
        n, k, n_inst, L = len(records), self.n_chain_calls, len(self.instruments), self.args.segment_length_ref
        pad = self.pad_length if self.pad_b4_manipulation else 0
        fused = getattr(collate, "__func__", None) is Collate_Variable_Length_Segments.random_duration_segments_strong_negatives
        if fused:
            if collate.__self__.num_strong_negatives + 1 != k:
                raise ValueError("get_batch: the collate's num_strong_negatives is not the dataset's")
            la, lb, sa, sb = collate.__self__.draw_random_durations(L, n)
        y = self._manipulate(records, self._gather(records))
        x = torch.cat([y[inst] for inst in self.data_paths.keys()], 0)              # rows (inst, b, neg, A / B)
        per = n * k * 2
        if fused:
            rows = lambda ab: [i * per + (b * k + neg) * 2 + ab for i in range(n_inst) for b in range(n) for neg in range(k)]
            starts = lambda s: [pad + s[b] for _ in range(n_inst) for b in range(n) for _ in range(k)]
            return self._finish(x, rows(0), starts(sa), la, n_inst), self._finish(x, rows(1), starts(sb), lb, n_inst)
        rows = [i * per + (b * k + neg) * 2 + ab for b in range(n) for i in range(n_inst) for neg in range(k) for ab in range(2)]
        out = batch_finish(x, rows, [pad] * len(rows), L)
        items = [list(t.unbind(0)) for t in out.chunk(n, dim=0)]
        return items if collate is None else collate(items)


class MUSDB_Dataset_Mixing_Manipulated_Style_Transfer(_MUSDB_Manipulated):
    """Data for training the MixFXcloner (:356-539): per instrument A1 (the input: segment A as it is), A2 (ground truth: A manipulated) and
    B2 (reference: segment B with the same parameters).  Item: drums_A1, drums_A2, drums_B2, bass_A1, ... - [2, segment_length_ref] float32
    on the device, clamped to [-1, 1]."""
    n_chain_calls = 1

    def _pattern(self, inst):
        return f"{self.data_dir}{inst}_normalized_{self.args.normalization_order}_silence_trimmed*.wav" if self.args.use_normalized \
            else f"{self.data_dir}{inst}_silence_trimmed.wav"

    def __len__(self):
        min_length = get_total_audio_length(glob(f"{self.data_dir}vocals_normalized_{self.args.normalization_order}*.wav"))
        return min_length // self.args.segment_length

    def __getitem__(self, idx):
        _refuse_worker_process(type(self).__name__)
        self._seed(idx)
        rec, out = {}, []
        for inst in self.data_paths.keys():
            paths, starts = self._draw_segments(inst)
            seg_a, seg_b = self._load_pair(paths, starts)
            rec[inst] = {"paths": paths, "starts": starts, "plans": []}
            a2, b2 = self._chain_pair(inst, rec, seg_a, seg_b)
            out.extend([self._finish_item(seg_a), self._finish_item(a2), self._finish_item(b2)])
        self.last_records = [rec]
        return out

    def get_batch(self, indices, collate=None):
        """What collate([self[i] for i in indices]) returns (collate None: the list of items), with that loop's draws, built on the device."""
        _refuse_worker_process(type(self).__name__)
        records = [self._draw_item(i) for i in indices]
        self.last_records = records
        n, n_inst, L = len(records), len(self.instruments), self.args.segment_length_ref
        pad = self.pad_length if self.pad_b4_manipulation else 0
        raw = self._gather(records)
        y = self._manipulate(records, raw)
        x = torch.cat([t for inst in self.data_paths.keys() for t in (raw[inst], y[inst])], 0)   # per instrument 2n raw rows, then 2n manipulated
        src = lambda i, b, j: i * 4 * n + (2 * b if j == 0 else 2 * n + 2 * b + (j - 1))             # j: A1, A2, B2
        if getattr(collate, "__func__", None) is Collate_Variable_Length_Segments.style_transfer_collate:
            return tuple(self._finish(x, [src(i, b, j) for i in range(n_inst) for b in range(n)], [pad] * (n_inst * n), L, n_inst) for j in range(3))
        rows = [src(i, b, j) for b in range(n) for i in range(n_inst) for j in range(3)]
        out = batch_finish(x, rows, [pad] * len(rows), L)
        items = [list(t.unbind(0)) for t in out.chunk(n, dim=0)]
        return items if collate is None else collate(items)


class Song_Dataset_Inference:
    def __init__(self, args):
        self.args = args
        self.data_dir = args.target_dir
        self.interpolate = args.interpolation
        self.instruments = args.instruments
        self.data_dir_paths = sorted(glob(f"{self.data_dir}*/"))
        self.input_name = args.input_file_name
        self.reference_name = args.reference_file_name
        self.stem_level_directory_name = args.stem_level_directory_name if args.do_not_separate \
            else os.path.join(args.stem_level_directory_name, args.separation_model)
        if self.interpolate:
            self.reference_name_B = args.reference_file_name_2interpolate
        if args.normalize_input:
            from ..mixing_manipulator.data_normalization import Audio_Effects_Normalizer
            self.normalization_chain = Audio_Effects_Normalizer(precomputed_feature_path=args.precomputed_normalization_feature,
                                                                STEMS=args.instruments, EFFECTS=args.normalization_order)
        # device: set by the runner (Mixing_Style_Transfer_Inference) to the GPU the stems are converted on - the stems are then decoded,
        # normalised and clamped THERE and returned as device tensors (the file's PCM bytes are what crosses PCIe); None = host arrays
        # like the reference.  workers (args.workers, the reference's DataLoader(num_workers=...)): > 0 = a background thread READS the next
        # song's wav files into memory while the current song is converted (file I/O only: decoding, normalising and everything else that
        # launches kernels stays on the consumer's thread and stream - see __iter__).
        self.device = None
        self.workers = int(getattr(args, "workers", 0) or 0)
        self._preread = None
        # convert (args.convert_input, off by default: the reference raises): stems at another sample rate are resampled on the device
        # (csrc/resample_kernels.h) and 24-bit PCM is accepted
        self.convert = bool(getattr(args, "convert_input", False))
        # dist (set by the runner when it runs on several ranks): the stems that need host / normaliser work are prepared by ONE rank each
        # (stem j by rank j % world) and broadcast - the normaliser, the expensive part of a song's preparation, is sharded by stems
        self.dist = None

    def _prepared_by_owner(self, idx, which, inst, j):
        """Input stem j of a multi-rank run: decoded + normalised by rank j % world, received by the others (one broadcast of [2, L])."""
        dist = self.dist
        rank, world = dist.get_rank(), dist.get_world_size()
        owner = j % world
        path = os.path.join(self.data_dir_paths[idx], self.stem_level_directory_name, which, inst + ".wav")
        if rank == owner:
            t = self._stem(idx, which, inst, normalize=True).contiguous()
        else:
            dev = self.device if (self.device is not None and dist.get_backend() == "nccl") else "cpu"
            t = torch.empty(2, self._frames(path), dtype=torch.float32, device=dev)
        if dist.get_backend() != "nccl" and t.is_cuda:          # test hook (gloo with several ranks on one GPU): through the host
            h = t.cpu()
            dist.broadcast(h, src=owner)
            return h.to(t.device)
        dist.broadcast(t, src=owner)
        return t.to(self.device) if self.device is not None else t

    def _frames(self, path):
        """frames of the stem as _stem returns it: the file's, or mst_resample_length of them when the file's rate is converted"""
        import wave
        with wave.open(path, "r") as w:
            rate, n = w.getframerate(), w.getnframes()
        if self.convert and rate != self.args.sample_rate:
            from ..mixing_manipulator._device_ops import Resampler
            return Resampler.get(rate, self.args.sample_rate).length(n)
        return n

    def __len__(self):
        return len(self.data_dir_paths)

    def _stem(self, idx, which, inst, normalize=False):
        path = os.path.join(self.data_dir_paths[idx], self.stem_level_directory_name, which, inst + ".wav")
        if self.device is not None:
            try:
                wav = load_wav_device(path, self.device, sample_rate=self.args.sample_rate, preread=self._preread, convert=self.convert)      # float32 [2, L] on the device
            except ValueError as e:
                if "stereo files only" not in str(e):
                    raise
                wav = None
            if wav is not None:
                if normalize:
                    wav = self.normalization_chain.normalize_audio(wav.t().contiguous(), src=inst).t().contiguous()
                return torch.clamp(wav.float(), min=-1, max=1)
        wav = load_wav_segment(path, axis=0, sample_rate=self.args.sample_rate, preread=self._preread, convert=self.convert)
        if normalize:           # only the input stems are normalised (:586-587)
            wav = self.normalization_chain.normalize_audio(wav.transpose(), src=inst).transpose()
        return torch.clamp(torch.from_numpy(wav).float(), min=-1, max=1)

    def __getitem__(self, idx):
        if self.dist is not None and self.args.normalize_input:
            inputs = [self._prepared_by_owner(idx, self.input_name, inst, j) for j, inst in enumerate(self.instruments)]
        else:
            inputs = [self._stem(idx, self.input_name, i, normalize=self.args.normalize_input) for i in self.instruments]
        refs = [self._stem(idx, self.reference_name, i) for i in self.instruments]
        dir_name = os.path.dirname(self.data_dir_paths[idx])
        if self.interpolate:
            refs_b = [self._stem(idx, self.reference_name_B, i) for i in self.instruments]
            return torch.stack(inputs, 0), torch.stack(refs, 0), torch.stack(refs_b, 0), dir_name
        return torch.stack(inputs, 0), torch.stack(refs, 0), dir_name

    def _song_paths(self, idx):
        kinds = [self.input_name, self.reference_name] + ([self.reference_name_B] if self.interpolate else [])
        return [os.path.join(self.data_dir_paths[idx], self.stem_level_directory_name, k, inst + ".wav") for k in kinds for inst in self.instruments]

    def _read_song(self, idx):
        out = {}
        for p in self._song_paths(idx):
            try:
                out[p] = read_wav_raw(p)
            except Exception:           # a missing / malformed file raises where the reference raises: in __getitem__, on the consumer's thread
                pass
        return out

    def __iter__(self):
        # Multi-rank runs prepare their songs INLINE whatever args.workers says (the loader's broadcasts must stay on the consumer's thread, in
        # its order: collectives of two threads on one process group pair up differently on different ranks).
        if self.workers <= 0 or len(self) < 2 or self.dist is not None:
            for i in range(len(self)):
                yield self[i]
            return
        # One song ahead, FILE I/O ONLY: a thread reads song i + 1's wav files into memory while song i is converted; decoding, the
        # normaliser and the stacking run here, on the consumer's thread and stream.  (Round 3 prepared the whole next song on a thread
        # with its own stream: its ~150 small kernels and ~70 host round trips per song queue behind the converter's 1.5 ms launches, the
        # prepared song arrived later than preparing it inline takes - measured 0.342 s per song against 0.324 s without the thread.)
        # The executor's context joins the thread when the generator is closed early (an exception in inference(), a break).
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=1, thread_name_prefix="mst-prefetch") as pool:
            nxt = pool.submit(self._read_song, 0)
            for i in range(len(self)):
                self._preread = nxt.result()
                nxt = pool.submit(self._read_song, i + 1) if i + 1 < len(self) else None
                try:
                    item = self[i]
                finally:
                    self._preread = None
                yield item
