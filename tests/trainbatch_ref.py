"""Training batches on the device (mst_batch_gather_pcm, mst_batch_finish, AugmentationChain.call_plans, StemBank and the MUSDB datasets): the
case bodies of tests/test_trainbatch_emu.py and tests/test_trainbatch_gpu.py, written once.  The two kernels bit for bit against numpy /
torch.clamp at every alignment; grouped plans against oracle.fx_ref composed as the plans say; whole batches of both datasets against the
oracle replay of their own draws; get_batch against the item loop."""
import argparse
import os
import random
import wave

import numpy as np
import torch

import fx_items_ref as I
import fx_space_items_ref as S
from music_mixing_style_transfer_amd import _lib

same_bits = I.same_bits
FILE_FRAMES = (9000, 12001, 20000)
TOL = 2e-5          # of max(1e-3, max|ref|): fx_space_items_ref.check_inst_chain's figure for call_items against the oracle replay


def deviation(y, ref):
    return float(np.abs(np.asarray(y, dtype=np.float64) - ref).max() / max(1e-3, np.abs(ref).max()))


# ---------------------------------------------------------------------------------------------------------- 1. gather
def pcm_bank(width, seed=3, frames=FILE_FRAMES):
    """-> (int array [sum(frames), 2] of dtype int16 / int32, file offsets): seeded values over the whole range with the extremes and zeros
    planted at both ends of every file and at odd positions"""
    dt = {2: np.int16, 4: np.int32}[width]
    lo, hi = np.iinfo(dt).min, np.iinfo(dt).max
    rng = np.random.default_rng(seed + width)
    files = []
    for n in frames:
        a = rng.integers(lo, hi, size=(n, 2), endpoint=True, dtype=np.int64).astype(dt)
        a[0], a[1], a[2] = (lo, hi), (hi, lo), (0, 0)
        a[-1], a[-2], a[-3] = (hi, lo), (lo, lo), (0, hi)
        a[1001], a[1002] = (lo, 0), (hi, hi)
        files.append(a)
    return np.concatenate(files), np.concatenate([[0], np.cumsum(frames)[:-1]]).astype(np.int64)


def gather_reference(bank, table, frames, width):
    raw = np.ascontiguousarray(bank, dtype={2: "<i2", 4: "<i4"}[width]).tobytes()
    dec = (np.frombuffer(raw, dtype={2: np.int16, 4: np.int32}[width]) / float(2 ** (8 * width - 1))).astype(np.float32).reshape(-1, 2)
    return np.stack([dec[o:o + frames] for o in table])


def gather_offsets(offs, frames, total):
    """0, odd offsets, the last valid offset of each file (the row ends with its file: nothing beyond it is read), repeats"""
    t = [0, 1, 4097, int(offs[1]) + 1, int(offs[1]) - frames, int(offs[2]) - frames, total - frames, 1, 0, int(offs[2]) + 7001, total - frames]
    assert all(0 <= o <= total - frames for o in t)
    return np.asarray(t, dtype=np.int64)


def gather_call(run, bank_t, n_bank_frames, width, table, frames, guard=True):
    """one mst_batch_gather_pcm into the middle of a NaN-filled buffer -> (rc, out [n, frames, 2]); the guard rows must stay untouched"""
    lib = run.lib
    n = len(table)
    host = torch.from_numpy(np.ascontiguousarray(table, dtype=np.int64))
    dev = run.t(np.asarray(table, dtype=np.int64))
    buf = torch.full(((n + 2) * frames * 2,), float("nan"), dtype=torch.float32, device=run.device)
    out = buf[frames * 2:(n + 1) * frames * 2]          # 8-byte aligned, 16-byte aligned only when frames is even
    with lib.device_ctx(buf):
        rc = lib.mst_batch_gather_pcm(bank_t.data_ptr(), n_bank_frames, width, dev.data_ptr(), host.data_ptr(), n, frames, out.data_ptr(), lib.stream_ptr(buf))
    res = buf.cpu().numpy()
    if rc == 0 and guard:
        assert np.isnan(res[:frames * 2]).all() and np.isnan(res[(n + 1) * frames * 2:]).all(), "a write outside the output rows"
    return rc, res[frames * 2:(n + 1) * frames * 2].reshape(n, frames, 2)


def check_gather(run, width, frames_list=(1, 3, 5, 1023, 1025, 5296)):
    bank, offs = pcm_bank(width)
    total = bank.shape[0]
    bank_t = run.t(np.frombuffer(np.ascontiguousarray(bank, dtype={2: "<i2", 4: "<i4"}[width]).tobytes(), dtype=np.uint8).copy())
    for frames in frames_list:
        table = gather_offsets(offs, frames, total)
        rc, y = gather_call(run, bank_t, total, width, table, frames)
        assert rc == 0, run.lib.mst_last_error()
        ref = gather_reference(bank, table, frames, width)
        assert same_bits(y, ref), f"gather width {width} frames {frames}: rows {[r for r in range(len(table)) if not same_bits(y[r], ref[r])]} differ"
    lim = float(2 ** (8 * width - 1))
    assert ref.min() == -1.0 and ref.max() == np.float32((lim - 1) / lim) and (ref == 0).any()


def check_gather_refusals(run):
    lib = run.lib
    bank, _ = pcm_bank(2)
    total = bank.shape[0]
    bank_t = run.t(np.frombuffer(bank.astype("<i2").tobytes(), dtype=np.uint8).copy())
    for table, row in (([0, 5, -1, 7], 2), ([0, total - 99, 3], 1), ([total, 0], 0)):
        rc, y = gather_call(run, bank_t, total, 2, table, 100, guard=False)
        msg = lib.mst_last_error().decode()
        assert rc == -1 and f"row {row}:" in msg, (rc, msg)
        assert np.isnan(y).all(), "a refused call launches nothing"
    assert gather_call(run, bank_t, total, 3, [0], 100, guard=False)[0] == -1 and b"width" in lib.mst_last_error()
    assert gather_call(run, bank_t, total, 2, [0], total, guard=False)[0] == 0          # the whole bank as one row


def write_pcm_wav(path, pcm, width, rate=44100):
    with wave.open(str(path), "w") as w:
        w.setnchannels(2)
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(pcm, dtype={2: "<i2", 4: "<i4"}[width]).tobytes())


def check_stem_bank(device, tmp_path, width):
    """the device-resident and the host-resident bank return the bits of load_wav_segment(...).astype(float32); a row beyond its file is refused"""
    from music_mixing_style_transfer_amd.data_loader import StemBank, load_wav_segment
    bank, offs = pcm_bank(width, seed=11)
    paths = []
    for i, n in enumerate(FILE_FRAMES):
        paths.append(str(tmp_path / f"f{width}_{i}.wav"))
        write_pcm_wav(paths[-1], bank[offs[i]:offs[i] + n], width)
    files, starts, frames = [0, 2, 1, 1, 0, 2, 1], [0, 333, 12001 - 5296, 1, 9000 - 5296, 20000 - 5296, 1], 5296
    ref = np.stack([load_wav_segment(paths[f], start_point=s, duration=frames, axis=1).astype(np.float32) for f, s in zip(files, starts)])
    res = StemBank(paths, device)
    host = StemBank(paths, device, max_resident_bytes=1000)
    assert res.resident and not host.resident and res.width == width
    assert res.frame_offset.tolist() == offs.tolist() and res.length.tolist() == list(FILE_FRAMES)
    y_res, y_host = res.gather(files, starts, frames), host.gather(files, starts, frames)
    assert str(y_res.device) == str(torch.device(device)) or y_res.device.type == torch.device(device).type
    assert same_bits(y_res.cpu().numpy(), ref) and same_bits(y_host.cpu().numpy(), ref)
    for bad in (([0], [9000 - 5295]), ([1], [-1]), ([3], [0])):
        try:
            res.gather(bad[0], bad[1], frames)
        except ValueError as e:
            assert "row 0" in str(e)
        else:
            raise AssertionError(f"StemBank.gather accepted {bad}")


def check_stem_bank_refuses_files(tmp_path):
    from music_mixing_style_transfer_amd.data_loader import StemBank, get_total_audio_length
    rng = np.random.default_rng(5)
    ok = str(tmp_path / "ok.wav")
    write_pcm_wav(ok, rng.integers(-99, 99, (50, 2)), 2)
    other_rate, deep = str(tmp_path / "rate.wav"), str(tmp_path / "deep.wav")
    write_pcm_wav(other_rate, rng.integers(-99, 99, (70, 2)), 2, rate=48000)
    write_pcm_wav(deep, rng.integers(-99, 99, (50, 2)), 4)
    assert get_total_audio_length([ok, other_rate, deep]) == 170
    for paths, words in (([ok, other_rate], "sample rate should be 44100"), ([ok, deep], "one bit depth")):
        try:
            StemBank(paths, "cpu")
        except ValueError as e:
            assert words in str(e)
        else:
            raise AssertionError(words)
    with wave.open(str(tmp_path / "b8.wav"), "w") as w:
        w.setnchannels(2)
        w.setsampwidth(1)
        w.setframerate(44100)
        w.writeframes(bytes(100))
    try:
        StemBank([str(tmp_path / "b8.wav")], "cpu")
    except ValueError as e:
        assert "bit depth should be 16 or 32-bit" in str(e)
    else:
        raise AssertionError("8-bit file accepted")


# ---------------------------------------------------------------------------------------------------------- 2. finish
SPECIALS = np.array([1.0000001, -1.5, 1.0, -1.0, -0.0, np.nan, 0.0, 3.0e38, -np.inf], dtype=np.float32)


def finish_input(n, Lp, Cn, seed=9):
    x = (0.7 * np.random.default_rng(seed).standard_normal((n, Lp, Cn))).astype(np.float32)          # a good part beyond +-1
    flat = x.reshape(n, -1)
    for i in range(n):
        for k, v in enumerate(SPECIALS):          # planted all over the row: every window of the cases holds some
            flat[i, (7 + 13 * k + 5 * i)::211][:] = v
    assert np.float32(1.0000001) > 1
    return x


def finish_reference(x, rows, start, length):
    xt = torch.from_numpy(x)
    return torch.stack([torch.clamp(xt[r, s:s + length].transpose(0, 1), -1, 1) for r, s in zip(rows, start)]).numpy()


def finish_call(run, xt, n, Lp, Cn, rows, start, length, shift=0):
    """one mst_batch_finish into a NaN-guarded buffer whose output starts `shift` floats beyond a 16-byte boundary -> (rc, out [m, C, len])"""
    lib = run.lib
    m = len(rows)
    rh, sh = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)) for a in (rows, start))
    rd, sd = run.t(np.asarray(rows, dtype=np.int64)), run.t(np.asarray(start, dtype=np.int64))
    size = m * Cn * length
    buf = torch.full((size + 16,), 12345.0, dtype=torch.float32, device=run.device)
    out = buf[4 + shift:4 + shift + size]
    with lib.device_ctx(buf):
        rc = lib.mst_batch_finish(xt.data_ptr(), n, Lp, Cn, rd.data_ptr(), rh.data_ptr(), sd.data_ptr(), sh.data_ptr(), m, length, out.data_ptr(), lib.stream_ptr(buf))
    res = buf.cpu().numpy()
    if rc == 0:
        assert (res[:4 + shift] == 12345.0).all() and (res[4 + shift + size:] == 12345.0).all(), "a write outside the output"
    return rc, res[4 + shift:4 + shift + size].reshape(m, Cn, length)


def check_finish(run, Cn, lengths=(1, 2, 3, 7, 1024, 1025, 1200)):
    n, Lp = 5, 1300
    x = finish_input(n, Lp, Cn)
    xt = run.t(x)
    rows, start = [3, 0, 0, 4, 1, 2, 2, 4], [0, 1, 2, 3, 17, 64, 99, 100]          # odd and even starts; repeated and permuted rows
    seen = set()
    for length in lengths:
        for shift in (0, 1, 2, 3):
            rc, y = finish_call(run, xt, n, Lp, Cn, rows, start, length, shift)
            assert rc == 0, run.lib.mst_last_error()
            ref = finish_reference(x, rows, start, length)
            assert same_bits(y, ref), f"finish C {Cn} len {length} shift {shift}"
        seen.update(I.bits(ref).reshape(-1).tolist())
    want = I.bits(np.array([1.0, -1.0, -0.0, np.nan], dtype=np.float32)).tolist()
    assert all(w in seen for w in want), "1, -1, -0.0 and NaN all appear in the outputs (bit patterns)"


def check_finish_refusals(run):
    lib = run.lib
    x = finish_input(3, 500, 2)
    xt = run.t(x)
    for rows, start, row, word in (([0, 3, 1], [0, 0, 0], 1, "source row 3"), ([0, 1, -1], [0, 0, 0], 2, "source row -1"), ([0, 1, 2], [0, 401, 0], 1, "samples 401"),
                                   ([2, 1, 0], [-2, 0, 0], 0, "samples -2")):
        rc, y = finish_call(run, xt, 3, 500, 2, rows, start, 100)
        msg = lib.mst_last_error().decode()
        assert rc == -1 and f"row {row}:" in msg and word in msg, (rc, msg)
        assert (y == 12345.0).all(), "a refused call launches nothing"
    assert finish_call(run, xt, 3, 500, 3, [0], [0], 100)[0] == -1 and b"C = 3" in lib.mst_last_error()
    assert finish_call(run, xt, 3, 500, 2, [0], [0], 501)[0] == -1
    assert finish_call(run, xt, 3, 500, 2, [2], [0], 500)[0] == 0


def check_wrappers(device):
    """loader_utils.gather_pcm / batch_finish: the library's refusal arrives as a ValueError that names the row"""
    from music_mixing_style_transfer_amd.data_loader import batch_finish, gather_pcm
    bank, _ = pcm_bank(2)
    bt = torch.from_numpy(np.frombuffer(bank.astype("<i2").tobytes(), dtype=np.uint8).copy()).to(device)
    y = gather_pcm(bt, bank.shape[0], 2, [5, 0], 40)
    assert same_bits(y.cpu().numpy(), gather_reference(bank, [5, 0], 40, 2))
    x = finish_input(3, 500, 2)
    z = batch_finish(torch.from_numpy(x).to(device), [2, 0], [3, 4], 77)
    assert same_bits(z.cpu().numpy(), finish_reference(x, [2, 0], [3, 4], 77))
    for call, word in ((lambda: gather_pcm(bt, bank.shape[0], 2, [5, bank.shape[0] - 39], 40), "row 1:"),
                       (lambda: batch_finish(torch.from_numpy(x).to(device), [2, 0], [3, 424], 77), "row 1:")):
        try:
            call()
        except ValueError as e:
            assert word in str(e)
        else:
            raise AssertionError("accepted")


# ---------------------------------------------------------------------------------------------------------- 3. grouped plans
def _chain_state(chain):
    from music_mixing_style_transfer_amd.mixing_manipulator.common_audioeffects import AugmentationChain, parameter_values

    def order(c):
        return [order(fx) if isinstance(fx, AugmentationChain) else type(fx).__name__ + ":" + str(sorted(fx.parameters.__dict__.keys())[:1]) for fx, _, _ in c.fxs]
    return order(chain), [sorted(parameter_values(fx).items(), key=lambda kv: kv[0]) for fx in chain._processors()]


def _generators():
    return random.getstate(), np.random.get_state()[1].tolist(), np.random.get_state()[2], torch.get_rng_state().tolist()


def check_call_plans(device, inst, ir_dir, comp_fn, log=print):
    """three plans for six rows: row r runs plans[r // 2] (oracle replay); a constant pair gives identical rows; generators, fxs orders and
    parameter values afterwards are those the planning loop alone leaves; call_items is call_plans of plan_items, bit for bit"""
    x, build, seed, _ = S.chain_case(inst, ir_dir, comp_fn)
    x = x.copy()
    x[3] = x[2]          # the second pair holds the same audio twice
    xt = torch.from_numpy(x).to(device)
    twin = build()
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    for _ in range(3):
        twin.plan_one(2)
    want_state, want_gen = _chain_state(twin), _generators()

    chain = build()
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    plans = [chain.plan_one(2) for _ in range(3)]
    assert plans[0] is not plans[1] and len({repr([(op[0], op[2] if op[0] == "fx" else op[1:]) for op in p]) for p in plans}) == 3, "three different sets of draws"
    out = S._np(chain.call_plans(xt, plans, group=2))
    assert _chain_state(chain) == want_state, "fxs orders and parameter values as after the planning loop alone"
    assert _generators() == want_gen, "call_plans draws nothing"
    assert out.shape == (6, 1200, 2) and np.isfinite(out).all()
    for r in range(6):
        ref = S.oracle_plan_item(x[r], plans[r // 2], comp_fn)
        dev = deviation(out[r], ref)
        log(f"call_plans {inst} row {r} (plan {r // 2}): deviation {dev:.2e} of max(1e-3, max|ref|)")
        assert dev <= TOL, f"call_plans {inst} row {r}: {dev:.2e}"
    assert same_bits(out[2], out[3]), "rows 2i and 2i + 1 of a constant pair"
    for bad in (lambda: chain.call_plans(xt, plans, group=3), lambda: chain.call_plans(xt[0], plans[:1])):
        try:
            bad()
        except ValueError:
            pass
        else:
            raise AssertionError("call_plans accepted a batch that does not fit its plans")


def check_call_items_unchanged(device, inst, ir_dir, comp_fn):
    """the helper's seeded case through call_items and through call_plans(x, plan_items(n, C)): the same bits, the same state afterwards"""
    x, build, seed, _ = S.chain_case(inst, ir_dir, comp_fn)
    xt = torch.from_numpy(x).to(device)
    outs, states = [], []
    for entry in ("items", "plans"):
        chain = build()
        random.seed(seed)
        np.random.seed(seed)
        outs.append(S._np(chain.call_items(xt) if entry == "items" else chain.call_plans(xt, chain.plan_items(6, 2))))
        states.append((_chain_state(chain), _generators()[:3]))
    assert same_bits(outs[0], outs[1]) and states[0] == states[1]


# ---------------------------------------------------------------------------------------------------------- 4. - 7. the datasets
ORDER = "eqcompimagegain"
PROCESSORS = ("Equaliser", "Compressor", "Panner", "MidSideImager", "Gain")
# random_seed per (dataset, impulse-response directory given): the smallest seed whose replay of indices 0, 1, 2 on write_musdb_dir's files
# meets check_batch_vs_oracle's coverage conditions (found on the CPU from the draws and the oracle alone)
BATCH_SEEDS = {("fxenc", True): 1, ("fxenc", False): 1, ("style", True): 1, ("style", False): 2}


def make_args(root, **kw):
    a = dict(data_dir=str(root) + "/", using_dataset="musdb", use_normalized=True, normalization_order=ORDER, random_seed=3, pad_b4_manipulation=True,
             ir_dir_path=None, sample_rate=44100, segment_length=2400, segment_length_ref=1200, num_strong_negatives=1, batch_size_total=4,
             reference_length=1200)
    a.update(kw)
    return argparse.Namespace(**a)


def write_musdb_dir(root, seed=1, mode="val", loud=("vocals", 2)):
    """a tiny MUSDB-shaped directory written from a seed: per instrument three 16-bit files of FILE_FRAMES frames of noise (a decaying
    envelope per 3000 frames so that the compressor has something to do); file `loud` is full-scale noise"""
    d = os.path.join(str(root), mode)
    os.makedirs(d, exist_ok=True)
    rng = np.random.default_rng(seed)
    for inst in ("drums", "bass", "other", "vocals"):
        for k, n in enumerate(FILE_FRAMES):
            env = 0.05 + 0.3 * np.exp(-(np.arange(n) % 3000) / 900.0)
            x = rng.standard_normal((n, 2)) * (0.6 if (inst, k) == loud else env[:, None])
            write_pcm_wav(os.path.join(d, f"{inst}_normalized_{ORDER}_silence_trimmed_{k}.wav"), np.clip(np.rint(x * 32767), -32768, 32767), 2)
    return str(root)


def dataset_class(kind):
    from music_mixing_style_transfer_amd import data_loader as D
    return {"fxenc": D.MUSDB_Dataset_Mixing_Manipulated_FXencoder, "style": D.MUSDB_Dataset_Mixing_Manipulated_Style_Transfer}[kind]


def replay_rows(ds, records, comp_fn, kind):
    """per record the reference's item from the oracle: load_wav_segment on the file, oracle_plan_item per chain call, crop / clamp / transpose
    in numpy -> (items: list of lists of [2, L] float32, clamped sample count)"""
    from music_mixing_style_transfer_amd.data_loader import load_wav_segment
    pad = ds.pad_length if ds.pad_b4_manipulation else 0
    clamped = 0

    def tail(y):
        nonlocal clamped
        y = y[pad:len(y) - pad] if pad else y
        clamped += int((np.abs(y) > 1).sum())
        return np.ascontiguousarray(np.clip(y, -1, 1).T.astype(np.float32))

    items = []
    for rec in records:
        item = []
        for inst in ds.instruments:
            a, b = (load_wav_segment(p, start_point=s, duration=ds.load_duration, axis=1).astype(np.float32) for p, s in zip(rec[inst]["paths"], rec[inst]["starts"]))
            if kind == "style":
                item.append(tail(a))
            for plan in rec[inst]["plans"]:
                item.extend([tail(S.oracle_plan_item(a, plan, comp_fn)), tail(S.oracle_plan_item(b, plan, comp_fn))])
        items.append(item)
    return items, clamped


def plan_coverage(records):
    """(processor type names applied anywhere, True when some chain call skipped a processor of its chain)"""
    seen, skipped = set(), False
    for rec in records:
        for inst, r in rec.items():
            for plan in r["plans"]:
                names = [type(op[1]).__name__ for op in plan if op[0] == "fx"]
                seen.update(names)
                skipped = skipped or not all(n in names for n in PROCESSORS)
    return seen, skipped


def record_summary(rec):
    """what of a record compares with ==: file names, start points and every drawn parameter value"""
    return {inst: ([os.path.basename(p) for p in r["paths"]], list(r["starts"]),
                   [[(type(op[1]).__name__, sorted(op[2].items(), key=lambda kv: kv[0]), op[3]) if op[0] == "fx" else op for op in plan] for plan in r["plans"]])
            for inst, r in rec.items()}


def check_batch_vs_oracle(device, kind, root, ir_dir, comp_fn, seed, indices=(0, 1, 2), log=print, expect_clamp=True):
    """'full' mode with the default probability tables: get_batch with the dataset's collate against the oracle replay of its own draws;
    shapes and order of the reference's collate; the collate's lengths and starts restated; the coverage conditions"""
    from music_mixing_style_transfer_amd.data_loader import Collate_Variable_Length_Segments
    args = make_args(root, random_seed=seed, ir_dir_path=ir_dir)
    ds = dataset_class(kind)(args, "val", device=device)
    collate = Collate_Variable_Length_Segments(args)
    n, k, L = len(indices), args.num_strong_negatives + 1, args.segment_length_ref
    if kind == "fxenc":
        out = ds.get_batch(list(indices), collate.random_duration_segments_strong_negatives)
    else:
        out = ds.get_batch(list(indices), collate.style_transfer_collate)
    gen_after = _generators()
    records = ds.last_records
    twin = dataset_class(kind)(args, "val", device=device)
    assert [record_summary(twin._draw_item(i)) for i in indices] == [record_summary(r) for r in records], "the draws of the batch are the item loop's"
    if kind == "fxenc":          # the reference's collate draws, restated (:49-61)
        la, lb = (int(v) for v in torch.randint(low=L // 2, high=L, size=(2,)))
        sa, sb = [], []
        for _ in indices:
            sa.append(int(torch.randint(low=0, high=L - la, size=(1,))[0]))
            sb.append(int(torch.randint(low=0, high=L - lb, size=(1,))[0]))
        assert la != lb, "the seed gives two different lengths"
    assert _generators() == gen_after, "the three generators end where collate([ds[i] for i in indices]) leaves them"
    seen, skipped = plan_coverage(records)
    reverb = "ConvolutionalReverb" if ir_dir else "AlgorithmicReverb"
    assert set(PROCESSORS) | {reverb} <= seen, f"every processor type is applied somewhere in the batch: {sorted(seen)}"
    assert skipped, "some chain call skips a processor"
    items, clamped = replay_rows(ds, records, comp_fn, kind)
    assert clamped > 0 or not expect_clamp, "the replay clamps at least one sample"
    worst = 0.0
    if kind == "fxenc":
        assert len(out) == 2 and all(len(lst) == 4 for lst in out)
        for ab, (lst, length, starts) in enumerate(zip(out, (la, lb), (sa, sb))):
            for i, t in enumerate(lst):
                assert tuple(t.shape) == (n * k, 2, length) and t.dtype == torch.float32 and t.device.type == torch.device(device).type
                y = t.cpu().numpy()
                for b in range(n):
                    for neg in range(k):
                        ref = items[b][i * k * 2 + 2 * neg + ab][:, starts[b]:starts[b] + length]
                        worst = max(worst, deviation(y[b * k + neg], ref))
                assert np.abs(y).max() <= 1
    else:
        assert len(out) == 3 and all(len(lst) == 4 for lst in out)
        for j, lst in enumerate(out):
            for i, t in enumerate(lst):
                assert tuple(t.shape) == (n, 2, L) and t.dtype == torch.float32 and t.device.type == torch.device(device).type
                y = t.cpu().numpy()
                for b in range(n):
                    ref = items[b][i * 3 + j]
                    if j == 0:
                        assert same_bits(y[b], ref), "A1 is the decoded segment, bit for bit"
                    worst = max(worst, deviation(y[b], ref))
    log(f"get_batch {kind} seed {seed} ir {bool(ir_dir)}: worst deviation {worst:.2e} of max(1e-3, max|ref|), {clamped} clamped samples in the replay")
    assert worst <= TOL, f"{worst:.2e}"
    return ds, out


EIGHT = ("Equaliser", "Compressor", "MidSideImager", "Gain", "ConvolutionalReverb", "Haas", "Panner", "AlgorithmicReverb")


def check_no_loop(device, kind, root, ir_dir, comp_fn, seed, monkeypatch):
    """process() of all eight processor classes and load_wav_segment raise: get_batch still completes with the results of check_batch_vs_oracle,
    in one gather launch per instrument and one finishing launch per output list"""
    from music_mixing_style_transfer_amd import mixing_manipulator as M
    from music_mixing_style_transfer_amd.data_loader import data_loader as DL
    from music_mixing_style_transfer_amd.data_loader import loader_utils as LU
    real_load = LU.load_wav_segment
    state = {"armed": False}
    counts = {"mst_batch_gather_pcm": 0, "mst_batch_finish": 0}

    def refuse(self, *a, **kw):
        raise AssertionError(f"{type(self).__name__}.process called from get_batch: the per-item loop is back")

    def guarded_load(*a, **kw):
        if state["armed"]:
            raise AssertionError("load_wav_segment called from get_batch: segments are cut on the host again")
        return real_load(*a, **kw)

    for name in EIGHT:
        monkeypatch.setattr(getattr(M.common_audioeffects, name), "process", refuse)
    monkeypatch.setattr(DL, "load_wav_segment", guarded_load)
    lib = _lib.lib()
    for name in counts:
        real = getattr(lib, name)
        monkeypatch.setattr(lib, name, lambda *a, _n=name, _f=real: (counts.__setitem__(_n, counts[_n] + (1 if state["armed"] else 0)), _f(*a))[1])
    cls = dataset_class(kind)
    real_get = cls.get_batch

    def armed_get(self, *a, **kw):
        state["armed"] = True
        try:
            return real_get(self, *a, **kw)
        finally:
            state["armed"] = False

    monkeypatch.setattr(cls, "get_batch", armed_get)
    check_batch_vs_oracle(device, kind, root, ir_dir, comp_fn, seed, log=lambda s: None)
    assert counts == {"mst_batch_gather_pcm": 4, "mst_batch_finish": 2 if kind == "fxenc" else 3}, counts


def check_batch_vs_items(device, kind, root, ir_dir, seed, indices=(0, 1, 2), log=print):
    """get_batch(indices) (no collate: the list of items) against [ds[i] for i in indices] of a twin dataset, row by row; the same draws; the
    three generators end in the same state"""
    args = make_args(root, random_seed=seed, ir_dir_path=ir_dir)
    cls = dataset_class(kind)
    ds = cls(args, "val", device=device)
    loop, loop_records = [], []
    for i in indices:
        loop.append(ds[i])
        loop_records.append(record_summary(ds.last_records[0]))
    gen_loop = _generators()
    ds = cls(args, "val", device=device)          # a fresh twin: a chain's shuffled `fxs` order carries over from item to item, as in the reference
    batch = ds.get_batch(list(indices))
    assert _generators() == gen_loop
    assert [record_summary(r) for r in ds.last_records] == loop_records
    per = 4 * (2 * (args.num_strong_negatives + 1) if kind == "fxenc" else 3)
    assert len(batch) == len(indices) and all(len(it) == per for it in batch) and all(len(it) == per for it in loop)
    worst = 0.0
    for a, b in zip(batch, loop):
        for j, (ta, tb) in enumerate(zip(a, b)):
            assert tuple(ta.shape) == tuple(tb.shape) == (2, args.segment_length_ref) and ta.dtype == tb.dtype == torch.float32
            assert float(ta.abs().max()) <= 1 and float(tb.abs().max()) <= 1
            if kind == "style" and j % 3 == 0:
                assert same_bits(ta.cpu().numpy(), tb.cpu().numpy()), "A1: the kernel's decode against load_wav_segment(...).float()"
            worst = max(worst, deviation(ta.cpu().numpy(), tb.cpu().numpy().astype(np.float64)))
    log(f"get_batch against the item loop, {kind}: worst deviation {worst:.2e}")
    assert worst <= TOL, f"{worst:.2e}"


# ---------------------------------------------------------------------------------------------------------- 8. the training shape
def check_gather_large(run, width=2, n=64, frames=135168):
    """64 rows of segment_length_ref + 2 * 2048 = 135168 frames out of a bank of a million frames: odd offsets, repeats, the bank's last row"""
    rng = np.random.default_rng(21)
    total = 1000003
    dt = {2: np.int16, 4: np.int32}[width]
    bank = rng.integers(np.iinfo(dt).min, np.iinfo(dt).max, size=(total, 2), endpoint=True, dtype=np.int64).astype(dt)
    table = rng.integers(0, total - frames, size=n, endpoint=True)
    table[:4] = (0, total - frames, 12345, 12345)
    bank_t = run.t(np.frombuffer(bank.tobytes(), dtype=np.uint8).copy())
    rc, y = gather_call(run, bank_t, total, width, table, frames)
    assert rc == 0, run.lib.mst_last_error()
    assert same_bits(y, gather_reference(bank, table, frames, width))


def check_finish_large(run, n=64, Lp=135168, length=131072):
    x = finish_input(n, Lp, 2, seed=23)
    rng = np.random.default_rng(24)
    rows = rng.permutation(n)
    rows[:2] = rows[2]
    start = rng.integers(0, Lp - length, size=n, endpoint=True)
    start[:3] = (2048, 0, Lp - length)
    rc, y = finish_call(run, run.t(x), n, Lp, 2, rows, start, length, shift=1)
    assert rc == 0, run.lib.mst_last_error()
    assert same_bits(y, finish_reference(x, rows.tolist(), start.tolist(), length))


# ---------------------------------------------------------------------------------------------------------- 4. against the real reference
GOLDEN_EFFECTS = ["comp", "imager", "gain"]
GOLDEN_CASES = [(kind, pad, neg) for kind in ("fxenc", "style") for pad in (0, 1) for neg in (0, 1)]
_golden = {}


def golden():
    """tests/golden/trainbatch.npz (make_golden_trainbatch.py): the reference's own datasets on write_musdb_dir's files, val mode, random_seed 3"""
    if not _golden:
        _golden.update(np.load(os.path.join(S.HERE, "golden", "trainbatch.npz")))
    return _golden


def golden_dataset(kind, pad, neg, root, device):
    args = make_args(root, random_seed=3, pad_b4_manipulation=bool(pad), num_strong_negatives=neg, ir_dir_path=None)
    return dataset_class(kind)(args, "val", applying_effects=list(GOLDEN_EFFECTS), device=device)


def record_arrays(ds, rec):
    """a record as the golden file lays it out: file names and start points in loading order, [chain calls][7] parameter values"""
    files = [os.path.basename(p) for inst in ds.instruments for p in rec[inst]["paths"]]
    starts = [s for inst in ds.instruments for s in rec[inst]["starts"]]
    params = [[float(v) for op in plan for v in op[2].values()] for inst in ds.instruments for plan in rec[inst]["plans"]]
    assert all([type(op[1]).__name__ for op in plan] == ["Compressor", "MidSideImager", "Gain"] for inst in ds.instruments for plan in rec[inst]["plans"])
    return files, starts, params


def next_draws():
    return [random.random(), float(np.random.rand()), float(torch.rand(1, dtype=torch.float64))]


def assert_record_is_golden(ds, rec, key):
    g = golden()
    files, starts, params = record_arrays(ds, rec)
    assert files == g[key + "/files"].tolist(), key
    assert starts == g[key + "/starts"].tolist(), key
    assert params == g[key + "/params"].tolist(), key


def check_golden_bookkeeping(kind, pad, neg, root):
    """no audio: __len__, and per index the draws of an item - file names, start points, parameter values, the generators afterwards - equal
    the reference's"""
    g = golden()
    case = f"{kind}/pad{pad}/neg{neg}"
    ds = golden_dataset(kind, pad, neg, root, "cpu")
    assert len(ds) == int(g[case + "/len"])
    for idx in range(4):
        rec = ds._draw_item(idx)
        assert next_draws() == g[f"{case}/{idx}/next"].tolist(), f"{case}/{idx}: the three generators after the item"
        assert_record_is_golden(ds, rec, f"{case}/{idx}")


def assert_audio_is_golden(item, key, kind, log):
    g = golden()
    probes = g["probes"]
    audio = np.stack([t.cpu().numpy() for t in item])
    assert list(audio.shape) == g[key + "/shape"].tolist() and audio.dtype == np.float32, key
    ref, ref_sum, ref_sumsq = g[key + "/audio"], g[key + "/sum"], g[key + "/sumsq"]
    worst = 0.0
    for r in range(audio.shape[0]):
        scale = max(1e-3, float(np.abs(ref[r]).max()))          # max|ref| over the stored probes: never above the row's
        if kind == "style" and r % 3 == 0:
            assert same_bits(audio[r][:, probes], ref[r]) and np.array_equal(audio[r].astype(np.float64).sum(axis=1), ref_sum[r]), f"{key} row {r}: A1"
        dev = float(np.abs(audio[r][:, probes].astype(np.float64) - ref[r]).max() / scale)
        worst = max(worst, dev)
        assert dev <= TOL, f"{key} row {r}: {dev:.2e} of max(1e-3, max|ref|) at the probes"
        n = audio.shape[2]
        assert np.all(np.abs(audio[r].astype(np.float64).sum(axis=1) - ref_sum[r]) <= TOL * scale * n), f"{key} row {r}: sum"
        assert np.all(np.abs(np.square(audio[r].astype(np.float64)).sum(axis=1) - ref_sumsq[r]) <= 2 * TOL * scale * n), f"{key} row {r}: sum of squares"
    log(f"{key}: worst deviation {worst:.2e} of max(1e-3, max|ref|) at the probes")


def check_golden_items(device, kind, pad, neg, root, via, log=print):
    """ds[idx] (via 'item') / get_batch([0, 1, 2, 3]) (via 'batch') against the reference's items: the draws equal, the audio within TOL, A1 bit
    for bit, the generators afterwards equal"""
    g = golden()
    case = f"{kind}/pad{pad}/neg{neg}"
    ds = golden_dataset(kind, pad, neg, root, device)
    if via == "item":
        for idx in range(4):
            item = ds[idx]
            assert next_draws() == g[f"{case}/{idx}/next"].tolist()
            assert_record_is_golden(ds, ds.last_records[0], f"{case}/{idx}")
            assert_audio_is_golden(item, f"{case}/{idx}", kind, log)
    else:
        items = ds.get_batch([0, 1, 2, 3])
        assert next_draws() == g[f"{case}/3/next"].tolist()
        for idx in range(4):
            assert_record_is_golden(ds, ds.last_records[idx], f"{case}/{idx}")
            assert_audio_is_golden(items[idx], f"{case}/{idx}", kind, log)


def check_dataloader(device, root):
    """the Style_Transfer dataset and the collate class behind a torch DataLoader with num_workers=0: the reference's three lists"""
    from music_mixing_style_transfer_amd.data_loader import Collate_Variable_Length_Segments
    args = make_args(root)
    ds = dataset_class("style")(args, "val", applying_effects=list(GOLDEN_EFFECTS), device=device)
    loader = torch.utils.data.DataLoader(torch.utils.data.Subset(ds, [0, 1, 2]), batch_size=3, shuffle=False, num_workers=0,
                                         collate_fn=Collate_Variable_Length_Segments(args).style_transfer_collate)
    batches = list(loader)
    assert len(batches) == 1 and len(batches[0]) == 3
    twin = dataset_class("style")(args, "val", applying_effects=list(GOLDEN_EFFECTS), device=device)
    want = twin.get_batch([0, 1, 2], Collate_Variable_Length_Segments(args).style_transfer_collate)
    for got_list, want_list in zip(batches[0], want):
        assert len(got_list) == 4
        for a, b in zip(got_list, want_list):
            assert tuple(a.shape) == tuple(b.shape) == (3, 2, 1200) and a.device.type == torch.device(device).type
            assert deviation(a.cpu().numpy(), b.cpu().numpy().astype(np.float64)) <= TOL
