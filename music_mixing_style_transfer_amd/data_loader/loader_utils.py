"""WAV I/O helpers of the inference data path (reference data_loader/loader_utils.py:40-70).

16/32-bit PCM -> float64 in [-1, 1) exactly like the reference (int16 / 2**15, int32 / 2**31), stereo
de-interleaved to [2, L] (axis=0) or [L, 2] (axis=1).  Same ValueErrors for a wrong sample rate / bit depth; with convert=True
(no counterpart in the reference) the loaders take 24-bit PCM and resample a file at another rate on the device instead.
soundfile is not a dependency: writing uses the standard `wave` module (PCM_16); `SlicedWavWriter` lets every rank of a
multi-GPU run write the time range it produced straight into the output file (no gather of the audio to one rank).
"""
import os
import struct
import wave

import numpy as np


def load_wav_length(audio_path):
    with wave.open(audio_path, "r") as w:
        return w.getnframes()


def read_wav_raw(audio_path):
    """(frame rate, bytes per sample, channels, frames, the raw PCM frames) of a wav file - the part of loading that is pure file I/O, which
    the dataset's prefetch thread does one song ahead (data_loader.py)."""
    with wave.open(audio_path, "r") as w:
        rate, width, nch, n = w.getframerate(), w.getsampwidth(), w.getnchannels(), w.getnframes()
        raw = w.readframes(n)
    return rate, width, nch, n, raw


def _resample(x, rate_in, rate_out):
    from ..mixing_manipulator._device_ops import resample
    return resample(x, rate_in, rate_out)


def pcm24_to_int32(raw):
    """24-bit PCM bytes (three per sample, little-endian) -> int32, sign-extended"""
    b = np.frombuffer(raw, dtype=np.uint8).reshape(-1, 3).astype(np.int32)
    v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
    return (v ^ 0x800000) - 0x800000


def load_wav_segment(audio_path, start_point=None, duration=None, axis=1, sample_rate=44100, preread=None, convert=False):
    """convert=True (off by default: the reference raises): 24-bit PCM is accepted (int / 2**23 in float64), and a file at another rate is
    decoded whole, resampled to sample_rate on the device (mixing_manipulator/_device_ops.resample: float32 in, float32 out) and returned as
    float64 like every other file; start_point and duration then count frames at sample_rate."""
    start_point = 0 if start_point is None else start_point
    if preread is not None and audio_path in preread:          # the whole file is in memory already
        rate, width, nch, n, raw = preread[audio_path]
    else:
        rate = None
    foreign = convert and (rate if rate is not None else _wav_rate(audio_path)) != sample_rate
    if foreign:                                                # another rate: the whole file, cut after the conversion
        if rate is None:
            rate, width, nch, n, raw = read_wav_raw(audio_path)
    elif rate is not None:
        duration = n if duration is None else duration
        if rate != sample_rate:
            raise ValueError(f"ValueError: input audio's sample rate should be {sample_rate}")
        a, b = min(max(0, start_point), n), min(n, max(0, start_point) + duration)
        raw = raw[a * width * nch:b * width * nch]
    else:
        with wave.open(audio_path, "r") as w:
            duration = w.getnframes() if duration is None else duration
            if w.getframerate() != sample_rate:
                raise ValueError(f"ValueError: input audio's sample rate should be {sample_rate}")
            w.setpos(start_point)
            raw = w.readframes(duration)
            width, nch = w.getsampwidth(), w.getnchannels()
    if width == 2:
        X = np.frombuffer(raw, dtype=np.int16) / float(2 ** 15)
    elif width == 4:
        X = np.frombuffer(raw, dtype=np.int32) / float(2 ** 31)
    elif width == 3 and convert:
        X = pcm24_to_int32(raw) / float(2 ** 23)
    else:
        raise ValueError("ValueError: input audio's bit depth should be 16 or 32-bit")
    if foreign:
        import torch
        Y = _resample(torch.from_numpy(X.reshape(-1, nch).astype(np.float32)), rate, sample_rate).cpu().numpy().astype(np.float64)
        a = min(max(0, start_point), len(Y))
        X = Y[a:len(Y) if duration is None else a + duration].reshape(-1)
    if nch == 2:
        X = np.concatenate((np.expand_dims(X[::2], axis=axis), np.expand_dims(X[1::2], axis=axis)), axis=axis)
    return X


def _wav_rate(audio_path):
    with wave.open(audio_path, "r") as w:
        return w.getframerate()


def load_wav_device(audio_path, device, sample_rate=44100, preread=None, convert=False):
    """The whole file as a float32 DEVICE tensor [2, L] (load_wav_segment(path, axis=0) followed by the dataset's `.float()`): the raw
    PCM frames are uploaded as they are (2 or 4 bytes per sample instead of a float64 array made on the host) and de-interleaved /
    scaled on the device - int / 2**15 (2**31) in float64, then rounded to float32, exactly the reference's two steps.  Stereo only
    (what the stems are); other channel counts go through load_wav_segment.  preread: {path: read_wav_raw(path)} of files already in memory.
    convert=True (off by default: the reference raises): 24-bit PCM is accepted (three bytes little-endian, sign-extended, / 2**23 in
    float64), and a file at another rate is resampled to sample_rate on the device (_device_ops.resample) before the final transpose."""
    import torch
    rate, width, nch, n, raw = preread[audio_path] if (preread is not None and audio_path in preread) else read_wav_raw(audio_path)
    if rate != sample_rate and not convert:
        raise ValueError(f"ValueError: input audio's sample rate should be {sample_rate}")
    if width not in ((2, 3, 4) if convert else (2, 4)):
        raise ValueError("ValueError: input audio's bit depth should be 16 or 32-bit")
    if nch != 2:
        raise ValueError("load_wav_device: stereo files only")
    import warnings
    with warnings.catch_warnings():          # the frames are only read (uploaded): no writable copy of the file's 30 MB
        warnings.simplefilter("ignore")
        host = torch.frombuffer(raw, dtype={2: torch.int16, 3: torch.uint8, 4: torch.int32}[width])
    dev = host.to(device, non_blocking=False)
    if width == 3:
        b = dev.view(-1, 3).to(torch.int32)
        dev = ((b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)) ^ 0x800000) - 0x800000
    x = (dev.view(-1, 2).to(torch.float64) / float(2 ** (8 * width - 1))).to(torch.float32)
    if rate != sample_rate:
        x = _resample(x, rate, sample_rate)
    return x.t().contiguous()


def get_total_audio_length(audio_paths):
    """frames of all the files together (reference loader_utils.py get_total_audio_length)"""
    return sum(load_wav_length(p) for p in audio_paths)


def _table(values, device):
    """int64 values as (host tensor, device tensor): the host copy is what the library checks, pinned and on its way to the device"""
    import torch
    from .._lib import lib
    host = torch.from_numpy(np.ascontiguousarray(values, dtype=np.int64))
    if torch.device(device).type == "cuda":
        host = host.pin_memory()
        return host, host.to(device, non_blocking=True)
    return host, lib().to_device(host)


def gather_pcm(bank, n_bank_frames, width, table, frames):
    """mst_batch_gather_pcm: bank, a uint8 device tensor of n_bank_frames interleaved stereo frames of `width` bytes per sample; table, the
    first frame of every row -> float32 [len(table), frames, 2], load_wav_device's arithmetic.  A row outside the bank is a ValueError that
    names it."""
    import torch
    from .._lib import lib as _binding
    lib = _binding()
    n = len(table)
    host, dev = _table(table, bank.device)
    out = torch.empty((n, int(frames), 2), dtype=torch.float32, device=bank.device)
    with lib.device_ctx(bank):
        lib.check(lib.mst_batch_gather_pcm(bank.data_ptr(), int(n_bank_frames), int(width), dev.data_ptr(), host.data_ptr(), n, int(frames),
                                           out.data_ptr(), lib.stream_ptr(bank)), "mst_batch_gather_pcm")
    return out


def batch_finish(x, rows, start, length):
    """mst_batch_finish: x float32 [n, Lp, C] on the device -> [len(rows), C, length],
    out[r] = clamp(x[rows[r], start[r]:start[r] + length].T, -1, 1) with torch.clamp's semantics, in one launch."""
    import torch
    from .._lib import lib as _binding
    lib = _binding()
    if x.dim() != 3 or x.dtype != torch.float32 or len(rows) != len(start):
        raise ValueError("batch_finish: x must be float32 [n, Lp, C] with one start per row")
    x = x.contiguous()
    m = len(rows)
    rows_host, rows_dev = _table(rows, x.device)
    start_host, start_dev = _table(start, x.device)
    out = torch.empty((m, x.shape[2], int(length)), dtype=torch.float32, device=x.device)
    with lib.device_ctx(x):
        lib.check(lib.mst_batch_finish(x.data_ptr(), x.shape[0], x.shape[1], x.shape[2], rows_dev.data_ptr(), rows_host.data_ptr(),
                                       start_dev.data_ptr(), start_host.data_ptr(), m, int(length), out.data_ptr(), lib.stream_ptr(x)),
                  "mst_batch_finish")
    return out


class StemBank:
    """The PCM frames of many stereo wav files, read once and kept back to back in ONE buffer, from which `gather` cuts a batch of segments
    with one launch (csrc/batch_kernels.h).  The files are 16- or 32-bit stereo at sample_rate, all of one bit depth (the reference's
    ValueErrors otherwise: its loaders raise the same way when a segment is read).  frame_offset[i] / length[i]: where file i starts in the
    bank and its frames (host arrays).  The buffer lives on the device; a bank larger than max_resident_bytes stays in pinned host memory
    instead, and gather copies just the chosen ranges into a per-call device slab and rebases its table - the same kernel, the same bits."""

    def __init__(self, paths, device, sample_rate=44100, max_resident_bytes=None):
        import torch
        self.paths, self.device, self.sample_rate = list(paths), torch.device(device), sample_rate
        self.width = None
        chunks, lengths = [], []
        for p in self.paths:
            rate, width, nch, n, raw = read_wav_raw(p)
            if rate != sample_rate:
                raise ValueError(f"ValueError: input audio's sample rate should be {sample_rate}")
            if width not in (2, 4):
                raise ValueError("ValueError: input audio's bit depth should be 16 or 32-bit")
            if nch != 2:
                raise ValueError(f"StemBank: {p}: stereo files only")
            if self.width is not None and width != self.width:
                raise ValueError(f"StemBank: {p}: {8 * width}-bit PCM in a bank of {8 * self.width}-bit files (one bit depth per bank)")
            self.width = width
            chunks.append(np.frombuffer(raw, dtype=np.uint8, count=n * 2 * width))
            lengths.append(n)
        if not chunks:
            raise ValueError("StemBank: no files")
        self.length = np.asarray(lengths, dtype=np.int64)
        self.frame_offset = np.concatenate([[0], np.cumsum(self.length)[:-1]]).astype(np.int64)
        self.n_frames = int(self.length.sum())
        self.frame_bytes = 2 * self.width
        host = torch.from_numpy(np.concatenate(chunks))
        self.resident = max_resident_bytes is None or host.numel() <= max_resident_bytes
        if self.device.type == "cuda":
            self.data = host.to(self.device) if self.resident else host.pin_memory()
        else:                                       # a test binding whose device memory is host memory
            self.data = host

    def gather(self, file_idx, start, frames):
        """Row r = frames start[r] .. start[r] + frames - 1 of file file_idx[r], float32 [n, frames, 2] on the device: int / 2^15 (2^31) in
        float64 rounded once to float32, bit for bit load_wav_device's values."""
        import torch
        file_idx, start, frames = np.asarray(file_idx, dtype=np.int64), np.asarray(start, dtype=np.int64), int(frames)
        if file_idx.shape != start.shape or file_idx.ndim != 1 or len(file_idx) < 1 or frames < 1:
            raise ValueError("StemBank.gather: one start per file index and at least one frame")
        for r, (i, s) in enumerate(zip(file_idx, start)):
            if not 0 <= i < len(self.paths):
                raise ValueError(f"StemBank.gather: row {r}: file index {i} outside [0, {len(self.paths)})")
            if s < 0 or s + frames > self.length[i]:
                raise ValueError(f"StemBank.gather: row {r}: frames {s} ... {s + frames} lie outside {self.paths[i]} ({self.length[i]} frames)")
        table = self.frame_offset[file_idx] + start
        if self.resident:
            return gather_pcm(self.data, self.n_frames, self.width, table, frames)
        fb, nb = self.frame_bytes, frames * self.frame_bytes
        slab = torch.empty(len(table) * nb, dtype=torch.uint8, device=self.device)
        for r, t in enumerate(table):
            slab[r * nb:(r + 1) * nb].copy_(self.data[int(t) * fb:int(t) * fb + nb], non_blocking=True)
        return gather_pcm(slab, len(table) * frames, self.width, np.arange(len(table), dtype=np.int64) * frames, frames)


def pcm16_device(x):
    """float device tensor [..., L, C] in [-1, 1] -> int16 tensor, the arithmetic of pcm16(): round-half-even(x * 32767), clipped."""
    import torch
    return torch.clamp(torch.round(x.to(torch.float32) * 32767.0), -32768, 32767).to(torch.int16)


def save_wav_pcm16(audio_path, data, sample_rate=44100):
    """data float [L, C] in [-1, 1] -> 16-bit PCM (what sf.write(..., 'PCM_16') is used for at
    inference/style_transfer.py:174,177): round(x * 32767), clipped."""
    data = np.asarray(data)
    if data.ndim == 1:
        data = data[:, None]
    pcm = data.astype("<i2") if data.dtype == np.int16 else pcm16(data)          # int16 in: already converted (on the device)
    with wave.open(audio_path, "w") as w:
        w.setnchannels(pcm.shape[1])
        w.setsampwidth(2)
        w.setframerate(sample_rate)
        w.writeframes(pcm.tobytes())


def pcm16(data):
    """float [-1, 1] -> little-endian int16 exactly like save_wav_pcm16 (elementwise: slices convert independently)."""
    return np.clip(np.rint(np.asarray(data) * 32767.0), -32768, 32767).astype("<i2")


class SlicedWavWriter:
    """A 16-bit PCM wav file of known length written in time slices, possibly by several processes of one node:
    `create()` (one process) writes the 44-byte RIFF header the `wave` module would write and sizes the file;
    `write(t0, data[L_slice, C])` (any process, after create) stores rows [t0, t0 + L_slice).  The finished file is
    byte-identical to save_wav_pcm16 of the whole signal."""

    def __init__(self, path, n_frames, n_channels=2, sample_rate=44100):
        self.path, self.n_frames, self.nch, self.sr = path, int(n_frames), int(n_channels), int(sample_rate)

    def create(self):
        nbytes = self.n_frames * self.nch * 2
        header = b"RIFF" + struct.pack("<L4s4sLHHLLHH4sL", 36 + nbytes, b"WAVE", b"fmt ", 16, 1, self.nch, self.sr,
                                       self.nch * self.sr * 2, self.nch * 2, 16, b"data", nbytes)
        with open(self.path, "wb") as f:
            f.write(header)
            f.truncate(44 + nbytes)

    def write(self, t0, data):
        data = np.asarray(data)
        if data.ndim == 1:
            data = data[:, None]
        if data.shape[1] != self.nch or t0 < 0 or t0 + data.shape[0] > self.n_frames:
            raise ValueError("SlicedWavWriter.write: slice outside the file")
        if data.shape[0] == 0:
            return
        fd = os.open(self.path, os.O_WRONLY)
        try:
            os.pwrite(fd, (data.astype("<i2") if data.dtype == np.int16 else pcm16(data)).tobytes(), 44 + int(t0) * self.nch * 2)
        finally:
            os.close(fd)
