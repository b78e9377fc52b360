"""Per-item FX parameters (mst_fx_*_items): the calls of tests/test_fx_items_emu.py and tests/test_fx_items_gpu.py, written once.  A Runner
(tests/fx_pass_ref.py) whose equaliser, and one whose compressor, go through the per-item entry points - the pass-by-pass checks of
fx_pass_ref run through them unchanged, the scratch layouts are the shared calls' -, the bit-for-bit comparisons of an _items call against shared-parameter calls on the
same batch, and the plan / oracle checks of AugmentationChain.call_items."""
import ctypes as C
import re

import numpy as np
import torch

import fx_pass_ref as R
from music_mixing_style_transfer_amd import _lib

SLOTS = R.SLOTS
FXI_KERNEL = r"^_Z\d+fxi_\w*kernel"          # every kernel of the per-item paths, and nothing of the shared ones


def bits(a):
    """the bit pattern of a float array (NaN-safe, -0.0 != 0.0)"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def varied_coefs(name, n):
    """n different, stable coefficient sets of one band count: the named set with its numerators scaled and its poles pulled in a little more
    per item (a0 = 1 is not assumed: rows keep their a0)"""
    base = np.asarray(R.coef_sets()[name], dtype=np.float64)
    out = np.stack([base.copy() for _ in range(n)])
    for i in range(n):
        r = 1.0 - 0.01 * i
        out[i, :, 0:3] *= 1.0 + 0.125 * i
        out[i, :, 4] *= r
        out[i, :, 5] *= r * r
    return np.ascontiguousarray(out)


def fuse_struct(in_scale=None, sumsq=None, in_sumsq=None, post_rms=0, post_gain=1.0, out_in_sumsq=None, out_ms=None, in_ms=None, forms=0):
    p = lambda t: t.data_ptr() if t is not None else None
    return _lib.MstFxFuse(p(in_scale), p(sumsq), p(in_sumsq), post_rms, post_gain, p(out_in_sumsq), p(out_ms), p(in_ms), forms=forms)


class ItemsRunner(R.Runner):
    """fx_pass_ref.Runner through the per-item entry points: one coefficient set -> every item gets it."""

    def eq_items_plan(self, n, L, Cn, nb):
        p = _lib.MstFxBiquadItemsPlan()
        self.lib.check(self.lib.mst_fx_biquad_items_plan(n, L, Cn, nb, C.byref(p)), "mst_fx_biquad_items_plan")
        return p

    def equaliser_items(self, x, coefs, in_scale=None, sumsq=False, in_sumsq=False, forms=0, scratch=True, poison=None):
        """x float32 [n, L, C], coefs [n][n_bands][6] -> what Runner.equaliser returns, plus tables [n][M][S], powers [n][9][S][S], coefn"""
        lib = self.lib
        n, L, Cn = x.shape
        coefs = np.ascontiguousarray(coefs, dtype=np.float64)
        assert coefs.shape[0] == n and coefs.shape[2] == 6
        nb = coefs.shape[1]
        plan = self.eq_plan(n, L, Cn, nb)
        xt = self.t(x.astype(np.float32))
        yt = torch.empty_like(xt)
        ct = self.t(coefs)
        nbytes = lib.mst_fx_biquad_items_scratch_bytes(n, L, Cn, nb)
        sc = torch.full(((nbytes + 7) // 8,), float("nan"), dtype=torch.float64, device=self.device) if scratch else None
        st = self.t(np.asarray(in_scale, dtype=np.float64)) if in_scale is not None else None
        fill = float("nan") if poison is None else poison
        qs = torch.full((n * SLOTS,), fill, dtype=torch.float64, device=self.device) if sumsq else None
        qi = torch.full((n * SLOTS,), fill, dtype=torch.float64, device=self.device) if in_sumsq else None
        fuse = None
        if st is not None or sumsq or in_sumsq or forms:
            f = fuse_struct(in_scale=st, sumsq=qs, out_in_sumsq=qi, forms=forms)
            fuse = C.byref(f)
        with lib.device_ctx(xt):
            rc = lib.mst_fx_biquad_cascade_items(xt.data_ptr(), yt.data_ptr(), n, L, Cn, ct.data_ptr(), nb, sc.data_ptr() if scratch else None,
                                                 nbytes if scratch else 0, fuse, lib.stream_ptr(xt))
        lib.check(rc, "mst_fx_biquad_cascade_items")
        out = {"plan": plan, "y": yt.cpu().numpy(), "sumsq": qs.cpu().numpy().reshape(n, SLOTS) if sumsq else None,
               "in_sumsq": qi.cpu().numpy().reshape(n, SLOTS) if in_sumsq else None}
        if scratch and plan.time_parallel:
            s = sc.cpu().numpy()
            cnt = n * Cn * plan.nchunks * plan.record_doubles
            shape = (n * Cn, plan.nchunks, plan.record_doubles)
            out["ends"] = s[plan.ends_offset // 8:plan.ends_offset // 8 + cnt].reshape(shape)
            out["starts"] = s[plan.starts_offset // 8:plan.starts_offset // 8 + cnt].reshape(shape)
            ip = self.eq_items_plan(n, L, Cn, nb)
            assert ip.M == plan.M and ip.total_bytes == nbytes and ip.tables_offset == lib.mst_fx_biquad_scratch_bytes(n, L, Cn, nb)
            S, M = 2 * nb, plan.M
            blocks = s[ip.tables_offset // 8:ip.tables_offset // 8 + n * ip.item_stride // 8].reshape(n, ip.item_stride // 8)
            out["tables"] = blocks[:, :M * S].reshape(n, M, S).copy()
            out["powers"] = blocks[:, ip.powers_offset // 8:ip.powers_offset // 8 + 9 * S * S].reshape(n, 9, S, S).copy()
            out["coefn"] = blocks[:, ip.coef_offset // 8:ip.coef_offset // 8 + 40].reshape(n, 8, 5).copy()
        return out

    def equaliser(self, x, coef6, in_scale=None, sumsq=False, in_sumsq=False, forms=0, scratch=True, poison=None):
        coefs = np.repeat(np.asarray(coef6, dtype=np.float64)[None], x.shape[0], axis=0)
        return self.equaliser_items(x, coefs, in_scale=in_scale, sumsq=sumsq, in_sumsq=in_sumsq, forms=forms, scratch=scratch, poison=poison)


# ---------------------------------------------------------------------------------------------------------- imager and gain
def imager_call(run, x, bal, items, in_scale=None, sumsq=False, post=None, in_sumsq=None):
    """MidSideImager on x [n, L, 2].  items: bal is [n] (mst_fx_midside_imager_items), else one value.  post: None, or (post_gain, per_item):
    the tail folding with in_sumsq [n, SLOTS]; per_item uploads post_gain as [n] float32.  -> dict(y, sumsq)"""
    lib = run.lib
    n, L, _ = x.shape
    xt = run.t(x.astype(np.float32))
    yt = torch.empty_like(xt)
    sc = torch.full((n * 2 * SLOTS,), float("nan"), dtype=torch.float64, device=run.device)
    st = run.t(np.asarray(in_scale, dtype=np.float64)) if in_scale is not None else None
    qs = torch.full((n * SLOTS,), 1e30, dtype=torch.float64, device=run.device) if sumsq else None
    qi = run.t(np.asarray(in_sumsq, dtype=np.float64).reshape(-1)) if post is not None else None
    pg = None
    shared_gain = 1.0
    if post is not None:
        g, per_item = post
        if items and per_item:
            pg = run.t(np.asarray(g, dtype=np.float32))
        else:
            shared_gain = float(g)
    fuse = None
    if st is not None or sumsq or post is not None:
        f = fuse_struct(in_scale=st, sumsq=qs, in_sumsq=qi, post_rms=1 if post is not None else 0, post_gain=shared_gain)
        fuse = C.byref(f)
    with lib.device_ctx(xt):
        if items:
            bt = run.t(np.asarray(bal, dtype=np.float64))
            rc = lib.mst_fx_midside_imager_items(xt.data_ptr(), yt.data_ptr(), n, L, bt.data_ptr(), sc.data_ptr(), pg.data_ptr() if pg is not None else None,
                                                 fuse, lib.stream_ptr(xt))
        else:
            rc = lib.mst_fx_midside_imager(xt.data_ptr(), yt.data_ptr(), n, L, float(bal), sc.data_ptr(), fuse, lib.stream_ptr(xt))
    lib.check(rc, "mst_fx_midside_imager")
    return {"y": yt.cpu().numpy(), "sumsq": qs.cpu().numpy().reshape(n, SLOTS) if sumsq else None}


def gain_call(run, x, gain_db, invert, items, in_scale=None):
    lib = run.lib
    n, L, Cn = x.shape
    xt = run.t(x.astype(np.float32))
    yt = torch.empty_like(xt)
    st = run.t(np.asarray(in_scale, dtype=np.float64)) if in_scale is not None else None
    fuse = None
    if st is not None:
        f = fuse_struct(in_scale=st)
        fuse = C.byref(f)
    with lib.device_ctx(xt):
        if items:
            gt = run.t(np.asarray(gain_db, dtype=np.float64))
            it = run.t(np.asarray(invert, dtype=np.int32)) if invert is not None else None
            rc = lib.mst_fx_gain_items(xt.data_ptr(), yt.data_ptr(), n, L, Cn, gt.data_ptr(), it.data_ptr() if it is not None else None, fuse, lib.stream_ptr(xt))
        else:
            rc = lib.mst_fx_gain(xt.data_ptr(), yt.data_ptr(), n, L, Cn, float(gain_db), int(invert or 0), fuse, lib.stream_ptr(xt))
    lib.check(rc, "mst_fx_gain")
    return yt.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------- the checks
def check_tables(run, name, L, n, Cn, expect_M=None):
    """the device-built tables and powers of n different coefficient sets, read back through the plan offsets, against mst_fx_biquad_tables"""
    coefs = varied_coefs(name, n)
    x = R.eq_input(L, n, Cn, 3)
    got = run.equaliser_items(x, coefs)
    M = got["plan"].M
    if expect_M is not None:
        assert expect_M(M), f"{name} L={L}: M = {M}"
    for i in range(n):
        tab, pw = run.eq_tables(coefs[i], M)
        assert same_bits(got["tables"][i], tab), f"{name} M={M} item {i}: impulse-state table"
        assert same_bits(got["powers"][i], pw), f"{name} M={M} item {i}: powers"
        want = np.zeros((8, 5))
        want[:coefs.shape[1]] = coefs[i][:, [0, 1, 2, 4, 5]] / coefs[i][:, 3:4]          # IEEE division: numpy's is the device's
        assert same_bits(got["coefn"][i], want), f"{name} item {i}: normalised coefficients"
    return M


EQ_SAME = [  # name, L, n, C, forms, fused
    ("config4", 4099, 5, 2, 0, True),
    ("config4", 4099, 5, 2, R.VALU_LANE, True),
    ("config4", 4099, 5, 1, 0, True),
    ("peaks8", 4099, 5, 2, 0, False),
    ("config4", 50, 5, 2, 0, False),
    ("config4", 50, 5, 1, 0, False),
    ("config4", 131072, 2, 2, 0, True),
]


def eq_fuse_kw(n, fused):
    return dict(in_scale=tuple(0.37 + 0.31 * i for i in range(n)), sumsq=True, in_sumsq=True) if fused else {}


def same_energy(a, b, nchunks, ordered):
    """The energy slots of two equaliser calls.  Slot s of an item is the float64 sum of the partials of its chunks s, s + 64, ..., added with
    atomics in the order the workgroups get there: the shared call does not repeat its own bits from run to run once a slot has several chunks
    (it does not on the emulator with several worker threads, nor on the device).  ordered (the emulator with one worker: workgroups in index
    order, the same chunk order in both calls): every slot bit for bit.  Otherwise: bit for bit where a slot holds one chunk (its channels
    arrive in lane order from one instruction); the others within the rounding of a float64 sum of their k positive chunk partials taken in
    two different orders, 2 (k - 1) 2^-53 of the sum.  That the per-chunk partials themselves are the same bits is shown on the device only
    indirectly - by the one-chunk slots, and by the output samples they are sums of - and directly by the ordered emulator run."""
    if ordered:
        return same_bits(a, b)
    k = np.array([len(range(s, nchunks, SLOTS)) for s in range(SLOTS)])
    one = k <= 1
    if not same_bits(np.ascontiguousarray(a[:, one]), np.ascontiguousarray(b[:, one])):
        return False
    return bool(np.all(np.abs(a - b)[:, ~one] <= (2.0 * (k[~one] - 1) * R.U * np.maximum(a, b)[:, ~one])))


def check_eq_same(run_items, run_shared, name, L, n, Cn, forms, fused, ordered=True):
    """every item given one coefficient set: the bits of the shared call on the same batch"""
    coef6 = R.coef_sets()[name]
    x = R.eq_input(L, n, Cn, 5)
    kw = eq_fuse_kw(n, fused)
    a = run_items.equaliser(x, coef6, forms=forms, **kw)
    b = run_shared.equaliser(x, coef6, forms=forms, **kw)
    what = f"eq same {name} L={L} n={n} C={Cn} forms={forms}"
    assert same_bits(a["y"], b["y"]), what + ": y"
    if a["plan"].time_parallel:
        assert same_bits(a["ends"], b["ends"]) and same_bits(a["starts"], b["starts"]), what + ": chunk records"
    if fused:
        nch = a["plan"].nchunks
        assert same_energy(a["sumsq"], b["sumsq"], nch, ordered), what + ": out_sumsq"
        assert same_energy(a["in_sumsq"], b["in_sumsq"], nch, ordered), what + ": out_in_sumsq"


def check_eq_different(run_items, run_shared, name, L, n, Cn, forms=0, fused=True, ordered=True):
    """item i of one _items call = item i of the shared call on the same batch with item i's coefficients: n shared calls"""
    coefs = varied_coefs(name, n)
    x = R.eq_input(L, n, Cn, 7)
    kw = eq_fuse_kw(n, fused)
    a = run_items.equaliser_items(x, coefs, forms=forms, **kw)
    for i in range(n):
        b = run_shared.equaliser(x, coefs[i], forms=forms, **kw)
        what = f"eq different {name} L={L} n={n} C={Cn} item {i}"
        assert same_bits(a["y"][i], b["y"][i]), what + ": y"
        if fused:
            nch = a["plan"].nchunks
            assert same_energy(a["sumsq"][i:i + 1], b["sumsq"][i:i + 1], nch, ordered) and same_energy(a["in_sumsq"][i:i + 1], b["in_sumsq"][i:i + 1], nch, ordered), what + ": energies"


def stereo_input(L, n, seed):
    rng = np.random.default_rng(seed)
    x = (0.2 * rng.standard_normal((n, L, 2))).astype(np.float32)
    x[:, :, 1] = (0.6 * x[:, :, 0] + 0.1 * rng.standard_normal((n, L))).astype(np.float32)
    return x


def check_imager_gain(run, L=4099, n=5):
    x = stereo_input(L, n, 11)
    scale = [0.5 + 0.4 * i for i in range(n)]
    in_sumsq = np.zeros((n, SLOTS))
    in_sumsq[:, :3] = np.random.default_rng(2).uniform(10.0, 40.0, (n, 3))
    # same parameters: the bits of the shared call, with and without the tail folding
    for bal in (0.731, 1.6):
        for post in (None, (0.7071, False), (0.7071, True)):
            kw = dict(in_scale=scale, sumsq=True, post=post, in_sumsq=in_sumsq if post is not None else None)
            g = post[0] if post is not None else None
            if post is not None and post[1]:
                kw["post"] = ([g] * n, True)
            a = imager_call(run, x, [bal] * n, True, **kw)
            kw["post"] = (g, False) if post is not None else None
            b = imager_call(run, x, bal, False, **kw)
            assert same_bits(a["y"], b["y"]) and same_bits(a["sumsq"], b["sumsq"]), f"imager same bal={bal} post={post}"
    # different parameters: item i against the shared call with item i's balance (and tail gain)
    bals = [0.0, 0.4567, 1.0, 1.25, 1.9994][:n]
    gains = [0.5, 1.0, 1.4142, 0.25, 2.0][:n]
    for post in (None, True):
        kw = dict(in_scale=scale, sumsq=True)
        a = imager_call(run, x, bals, True, post=(gains, True) if post else None, in_sumsq=in_sumsq if post else None, **kw)
        for i in range(n):
            b = imager_call(run, x, bals[i], False, post=(gains[i], False) if post else None, in_sumsq=in_sumsq if post else None, **kw)
            assert same_bits(a["y"][i], b["y"][i]) and same_bits(a["sumsq"][i], b["sumsq"][i]), f"imager item {i} post={post}"
    for Cn in (2, 1):
        xg = x[:, :, :Cn]
        assert same_bits(gain_call(run, xg, [-3.5] * n, [1] * n, True, in_scale=scale), gain_call(run, xg, -3.5, 1, False, in_scale=scale)), "gain same"
        assert same_bits(gain_call(run, xg, [4.25] * n, None, True), gain_call(run, xg, 4.25, 0, False)), "gain same, no fusion"
        dbs, inv = [-12.0, -3.3, 0.0, 2.7, 11.9][:n], [0, 1, 0, 1, 1][:n]
        a = gain_call(run, xg, dbs, inv, True, in_scale=scale)
        for i in range(n):
            assert same_bits(a[i], gain_call(run, xg, dbs[i], inv[i], False, in_scale=scale)[i]), f"gain item {i}"


# ---------------------------------------------------------------------------------------------------------- launch coverage
class ItemsTracer(R.Tracer):
    def __exit__(self, *a):
        n = self.end(self.text, len(self.text))
        assert n < len(self.text)
        self.seen.update(ln.split()[0] for ln in self.text.value.decode().splitlines() if re.match(FXI_KERNEL, ln))


def exported_items_kernels(lib_path):
    import subprocess
    nm = subprocess.run(["nm", "-D", "--defined-only", lib_path], check=True, capture_output=True, text=True).stdout
    return {f[2] for f in (ln.split() for ln in nm.splitlines()) if len(f) == 3 and f[1] in "TW" and re.match(FXI_KERNEL, f[2])}


# every band count on every per-item kernel form: mono (four-lane ends, lane apply), stereo (slab ends, slab apply; lane apply by its form
# bit), both scan sizes; the serial kernel.  (name, L, n, C, forms)
EQ_DIFFERENT = ([(f"peaks{k}", 113, 2, Cn, forms) for k in range(1, 9) for Cn, forms in ((2, 0), (1, 0), (2, _lib.FX_FORM_EQ_LANE_APPLY))] +
                [(f"butter{2 * k}", 64 * 255 + 1, 2, 1, 0) for k in range(1, 9)] +
                [("config4", 4099, 5, 2, 0), ("config4", 4099, 5, 1, 0), ("config4", 50, 3, 2, 0)])


def trace_items_cases(emu):
    """the fxi_* kernel symbols the case lists of this file launch (dry run)"""
    run = ItemsRunner(emu, "cpu")
    tr = ItemsTracer(emu)
    for name, L, n, Cn, forms in EQ_DIFFERENT + [c[:5] for c in EQ_SAME]:
        with tr:
            run.equaliser(np.zeros((n, L, Cn), dtype=np.float32), R.coef_sets()[name], forms=forms)
    x = np.zeros((2, 100, 2), dtype=np.float32)
    with tr:
        imager_call(run, x, [0.5, 0.5], True)
        gain_call(run, x, [0.0, 0.0], None, True)
    return tr.seen


# ---------------------------------------------------------------------------------------------------------- AugmentationChain.call_items
def tag_processors(chain):
    """a stable label per processor of a freshly built chain tree (before any shuffle): two chains built alike get the same labels"""
    for k, fx in enumerate(chain._processors()):
        fx.tag = k
    return chain


def fxs_order(chain):
    """the order of every fxs list of the tree, by label"""
    from music_mixing_style_transfer_amd.mixing_manipulator import AugmentationChain
    return [fxs_order(fx) if isinstance(fx, AugmentationChain) else fx.tag for fx, _, _ in chain.fxs]


class _Probe:
    """stands in for an array in the sequential loop: `w * x + (1 - w) * y` of a parallel chain leaves ("mix", w) in the log"""

    def __init__(self, log):
        self.log = log

    def __rmul__(self, w):
        return _Scaled(self, w)


class _Scaled:
    def __init__(self, p, w):
        self.p, self.w = p, w

    def __add__(self, other):
        self.p.log.append(("mix", self.w))
        return self.p


class _Holder:
    def __init__(self, x):
        self.x = x

    def result(self):
        return self.x


def record_sequential_loop(chain, n, monkeypatch):
    """`for i in range(n): chain([x_i])` with the processors' audio work patched out: per item the applied processors (label, parameter
    values, rms flag) and the mix weights, in the order the loop meets them"""
    from music_mixing_style_transfer_amd.mixing_manipulator import common_audioeffects as A
    logs = []

    def apply_same(self, x_list, processor, rms_normalize):
        logs[-1].append(("fx", processor.tag, A.parameter_values(processor), rms_normalize))
        return x_list

    monkeypatch.setattr(A.AugmentationChain, "apply_same_processor", apply_same)
    monkeypatch.setattr(A._Pending, "wrap", staticmethod(lambda x: _Holder(x)))
    for _ in range(n):
        logs.append([])
        chain([_Probe(logs[-1])])
    monkeypatch.undo()
    return logs


def plan_as_log(plans):
    return [[("fx", op[1].tag, op[2], op[3]) if op[0] == "fx" else op for op in plan if op[0] != "begin"] for plan in plans]


def oracle_chain_item(x, plan, comp_fn, rate=44100):
    """oracle.fx_ref's processors composed as one item's plan says (equaliser, compressor, imager, gain; rms-normalise where flagged)"""
    from oracle import fx_ref as F
    y = np.asarray(x, dtype=np.float32)
    for op in plan:
        assert op[0] == "fx"
        _, fx, v, rms, _ = op
        name = type(fx).__name__
        if name == "Equaliser":
            params = {b: (v[b + "_gain"], v[b + "_freq"], v.get(b + "_q", 0.707)) for b in fx.bands}
            z = F.equaliser(y, params, rate, bands=tuple(fx.bands))
        elif name == "Compressor":
            z = comp_fn(y, v["threshold"], v["attack_time"], v["release_time"], v["ratio"], rate)
        elif name == "MidSideImager":
            z = F.midside_imager(y, v["bal"])
        elif name == "Gain":
            z = F.gain(y, v["gain"], v["invert"])
        else:
            raise AssertionError(name)
        if rms:
            z = F.rms_normalize(y, z)
        y = np.asarray(z).astype(np.float32)
    return y


def config4_random_chain(probs):
    from music_mixing_style_transfer_amd.mixing_manipulator import AugmentationChain, Compressor, Equaliser, Gain, MidSideImager
    fxs = [(Equaliser(2, 44100), probs[0], True), (Compressor(44100), probs[1], True), (MidSideImager(), probs[2], True), (Gain(), probs[3], False)]
    return AugmentationChain(fxs=fxs, randomize_param_value=True)


def check_random_chain(device, comp_fn, probs, n=6, L=16384, seed=7, log=print):
    """a seeded randomised EQ -> compressor -> imager -> gain chain with rms-normalise through call_items: every item within 2e-6 max|ref| of
    the oracle's processors composed with the parameters drawn for that item (the tolerance of test_config4_chain_at_64_segments_vs_oracle)"""
    import random
    x = (0.1 * torch.randn(n, L, 2, generator=torch.Generator().manual_seed(seed))).clamp_(-1, 1)
    random.seed(seed)
    np.random.seed(seed)
    plans = config4_random_chain(probs).plan_items(n, 2)            # a twin chain: the draws of the run below
    chain = config4_random_chain(probs)
    random.seed(seed)
    np.random.seed(seed)
    out = chain.call_items(x.to(device))
    out = out.cpu().numpy() if isinstance(out, torch.Tensor) else np.stack([o.cpu().numpy() for o in out])
    assert out.shape == (n, L, 2) and np.isfinite(out).all()
    assert len({tuple(sorted(op[2].items())) for p in plans for op in p if type(op[1]).__name__ == "Equaliser"}) > 1 or probs[0] < 1, "the items drew different settings"
    worst = 0.0
    for i in range(n):
        ref = oracle_chain_item(x[i].numpy(), plans[i], comp_fn)
        dev = float(np.abs(out[i] - ref).max() / max(np.abs(ref).max(), 1e-30))
        log(f"call_items probs={probs} item {i}: {[type(op[1]).__name__ for op in plans[i]]} deviation {dev:.2e} of max|ref|")
        worst = max(worst, dev)
    assert worst <= 2e-6, f"call_items probs={probs}: worst deviation {worst:.2e} of max|ref|"
    return worst


def oracle_compressor_fn(oracle_fx_lib):
    fp = C.POINTER(C.c_float)

    def c_comp(xx, threshold, attack_time, release_time, ratio, sample_rate):
        if threshold == 0.0 and ratio == 1.0:
            return xx
        xx = np.ascontiguousarray(xx, dtype=np.float32)
        yy = np.empty_like(xx)
        oracle_fx_lib.ref_compressor(xx.ctypes.data_as(fp), yy.ctypes.data_as(fp), C.c_long(xx.shape[0]), xx.shape[1], C.c_double(threshold),
                                     C.c_double(attack_time), C.c_double(release_time), C.c_double(ratio), C.c_double(0.0), C.c_double(sample_rate))
        return yy
    return c_comp


# ---------------------------------------------------------------------------------------------------------- the compressor per item
def _comp_items_call(run, x, params, sr, in_scale, sumsq, forms, scratch):
    """fx_pass_ref._comp_call through mst_fx_compressor_items_prepare + mst_fx_compressor_items; params [n][4] = threshold dB, attack ms,
    release ms, ratio -> (rc, y, scratch, sumsq, ms, first refused item)"""
    lib = run.lib
    n, L, Cn = x.shape
    params = np.ascontiguousarray(params, dtype=np.float64)
    assert params.shape == (n, 4)
    nb = lib.mst_fx_compressor_items_table_bytes(n)
    assert nb == n * (4 + 4 * 33) * 8
    table = np.full(nb // 8, np.nan)
    refused = C.c_int(-7)
    rc = lib.mst_fx_compressor_items_prepare(params.ctypes.data, n, L, Cn, float(sr), forms, table.ctypes.data, nb, C.byref(refused))
    if rc != 0:
        return rc, None, None, None, None, refused.value
    assert refused.value == -1 and np.isfinite(table).all()
    xt = run.t(x.astype(np.float32))
    yt = torch.empty_like(xt)
    tt = run.t(table)
    nbytes = lib.mst_fx_compressor_scratch_bytes(n, L, Cn)
    sc = torch.full(((nbytes + 7) // 8,), float("nan"), dtype=torch.float64, device=run.device) if scratch else None
    st = run.t(np.asarray(in_scale, dtype=np.float64)) if in_scale is not None else None
    qs = torch.full((n * SLOTS,), 1e30, dtype=torch.float64, device=run.device) if sumsq else None
    qm = torch.full((n * SLOTS * 2,), 1e30, dtype=torch.float64, device=run.device) if sumsq and Cn == 2 else None
    fuse = None
    if st is not None or sumsq or forms:
        f = fuse_struct(in_scale=st, sumsq=qs, out_ms=qm, forms=forms)
        fuse = C.byref(f)
    with lib.device_ctx(xt):
        rc = lib.mst_fx_compressor_items(xt.data_ptr(), yt.data_ptr(), n, L, Cn, tt.data_ptr(), sc.data_ptr() if scratch else None,
                                         nbytes if scratch else 0, fuse, lib.stream_ptr(xt))
    return rc, yt, sc, qs, qm, -1


def run_compressor_items(run, x, params, sr=44100.0, in_scale=None, sumsq=False, forms=0, scratch=True):
    """fx_pass_ref.run_compressor for a per-item call: the same dict (the scratch layout is mst_fx_compressor_plan's)"""
    n, L, Cn = x.shape
    plan = run.comp_plan(n, L, Cn, params[0][1], params[0][2], sr, forms)
    rc, yt, sc, qs, qm, refused = _comp_items_call(run, x, params, sr, in_scale, sumsq, forms, scratch)
    if rc != 0:
        return {"rc": rc, "message": run.lib.mst_last_error().decode(), "plan": plan, "refused": refused}
    out = {"rc": 0, "plan": plan, "y": yt.cpu().numpy(), "sumsq": qs.cpu().numpy().reshape(n, SLOTS) if qs is not None else None,
           "ms": qm.cpu().numpy().reshape(n, SLOTS, 2) if qm is not None else None}
    if scratch:
        s = sc.cpu().numpy()
        n_seq = n * Cn
        take = lambda off, cnt: s[off // 8:off // 8 + cnt]
        if plan.form == _lib.FX_COMP_TIME_PARALLEL:
            out["maps"] = take(plan.maps_offset, n_seq * plan.nchunks * plan.record_doubles).reshape(n_seq, plan.nchunks, plan.record_doubles)
            out["ystart"] = take(plan.ystart_offset, n_seq * plan.nchunks).reshape(plan.nchunks, n_seq)
            out["carry"] = take(plan.carry_offset, n_seq)
        elif plan.form == _lib.FX_COMP_SPLIT_SERIAL:
            out["xl"] = take(plan.xl_offset, n_seq * L).reshape(L, n_seq)
        if sumsq:
            out["tsums"] = take(plan.tsums_offset, plan.ntiles * (3 * n if Cn == 2 else n_seq)).reshape((plan.ntiles, n, 3) if Cn == 2 else (plan.ntiles, n_seq))
    return out


class _CompItemsLib:
    """the binding with mst_fx_compressor answered by the per-item entry points (every item gets the call's one setting)"""

    def __init__(self, lib, runner):
        self._lib, self._run = lib, runner

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def mst_fx_compressor(self, x, y, n, L, Cn, thr, attack, release, ratio, sr, scratch, scratch_bytes, fuse, stream):
        lib = self._lib
        params = np.ascontiguousarray(np.tile([thr, attack, release, ratio], (n, 1)), dtype=np.float64)
        nb = lib.mst_fx_compressor_items_table_bytes(n)
        table = np.zeros(nb // 8)
        forms = C.cast(fuse, C.POINTER(_lib.MstFxFuse)).contents.forms if fuse is not None else 0
        rc = lib.mst_fx_compressor_items_prepare(params.ctypes.data, n, L, Cn, float(sr), forms, table.ctypes.data, nb, None)
        if rc != 0:
            return rc
        self._table = self._run.t(table)
        return lib.mst_fx_compressor_items(x, y, n, L, Cn, self._table.data_ptr(), scratch, scratch_bytes, fuse, stream)


class CompItemsRunner(R.Runner):
    """fx_pass_ref.Runner whose compressor goes through mst_fx_compressor_items: check_compressor / run_compressor run through it unchanged"""

    def __init__(self, lib, device):
        super().__init__(lib, device)
        self.lib = _CompItemsLib(lib, self)


BASE = (-30.0, 1.5, 60.0, 8.0)
# L, n, C, forms, fused; the split-serial form needs fewer than four 32-sample chunks: 96
COMP_SAME = [(L, 6, Cn, forms, fused) for Cn in (2, 1) for L, forms in ((96, 0), (100, 0), (4133, 0), (9001, _lib.FX_FORM_COMP_SLICE_SMALL))
             for fused in (True,)] + [(4133, 6, 2, 0, False), (200, 6, 2, -1, False)]          # forms -1: no scratch buffer (the serial kernel)
# aA < aR, aA > aR (200 / 300 ms attacks), aA == aR; ratios 4, 0.5, 1, 8, 40
COMP_MIXED = [(-30.0, 1.5, 60.0, 4.0), (-25.0, 200.0, 60.0, 0.5), (-20.0, 2.0, 100.0, 1.0), (-40.0, 5.0, 5.0, 8.0), (-10.0, 20.0, 500.0, 40.0),
              (-35.0, 300.0, 50.0, 4.0)]
COMP_SCALE = (1.9, 0.8, 1.0, 0.37, 1.2, 0.6)
COMP_KEYS = ("y", "sumsq", "ms", "maps", "ystart", "carry", "xl", "tsums")


def comp_case_kw(n, forms, fused):
    kw = dict(forms=max(forms, 0), scratch=forms >= 0)
    if fused:
        kw.update(in_scale=COMP_SCALE[:n], sumsq=True)
    return kw


def check_comp_same(run_items, run_shared, L, n, Cn, forms, fused, expect_form=None):
    """every item given one setting: y, out_sumsq, out_ms and everything the call leaves in its scratch are the shared call's bits"""
    x = R.comp_input(L, n, Cn, 9)
    kw = comp_case_kw(n, forms, fused)
    a = R.run_compressor(run_items, x, *BASE, **kw)
    b = R.run_compressor(run_shared, x, *BASE, **kw)
    assert a["rc"] == 0 and b["rc"] == 0, (a.get("message"), b.get("message"))
    for k in COMP_KEYS:
        if b.get(k) is not None:
            assert same_bits(a[k], b[k]), f"comp same L={L} n={n} C={Cn} forms={forms}: {k}"
    return b["plan"]


def check_comp_different(run, run_shared, L, n, Cn, forms=0, fused=True):
    """one batch mixing convex and concave items and ratios above, below and equal to 1: item i = item i of the shared call on the same batch
    with item i's settings - n shared calls"""
    x = R.comp_input(L, n, Cn, 10)
    kw = comp_case_kw(n, forms, fused)
    params = COMP_MIXED[:n]
    aA = [R.comp_alphas(p[1], p[2]) for p in params]
    assert any(a > r for a, r in aA) and any(a < r for a, r in aA) and {4.0, 0.5, 1.0} <= {p[3] for p in params}
    a = run_compressor_items(run, x, params, **kw)
    assert a["rc"] == 0, a.get("message")
    Cs = Cn
    for i, p in enumerate(params):
        b = R.run_compressor(run_shared, x, *p, **kw)
        assert b["rc"] == 0, b.get("message")
        what = f"comp different L={L} C={Cn} forms={forms} item {i} {p}"
        assert same_bits(a["y"][i], b["y"][i]), what + ": y"
        if fused:
            assert same_bits(a["sumsq"][i], b["sumsq"][i]), what + ": out_sumsq"
            if Cn == 2:
                assert same_bits(a["ms"][i], b["ms"][i]), what + ": out_ms"
        if "maps" in b:
            assert same_bits(a["maps"][i * Cs:(i + 1) * Cs], b["maps"][i * Cs:(i + 1) * Cs]) and same_bits(np.ascontiguousarray(a["ystart"][:, i * Cs:(i + 1) * Cs]), np.ascontiguousarray(b["ystart"][:, i * Cs:(i + 1) * Cs])), what + ": maps / ystart"


def check_comp_refusal(run):
    """attack 0.01 ms against release 1000 ms on one item of a batch: prepare names it; below four chunks (split-serial) it is accepted"""
    params = [BASE, BASE, (-30.0, 0.01, 1000.0, 8.0), BASE]
    x = R.comp_input(4133, 4, 2, 3)
    got = run_compressor_items(run, x, params)
    assert got["rc"] == -2 and got["refused"] == 2, got
    plan = run.comp_plan(4, 4133, 2, 0.01, 1000.0)
    assert plan.form == _lib.FX_COMP_WAVE_SERIAL and plan.kappa > plan.kappa_limit
    msg = got["message"]
    assert "item 2" in msg and "kappa" in msg and f"{plan.kappa_limit:.3g}" in msg and f"{R.comp_alphas(0.01, 1000.0)[0]:.6g}" in msg, msg
    assert run_compressor_items(run, R.comp_input(96, 4, 2, 3), params)["rc"] == 0
    got = run_compressor_items(run, x, [BASE, (0.0, 2.0, 100.0, 1.0), BASE, BASE])
    assert got["rc"] == -2 and got["refused"] == 1 and "bypass" in got["message"]


def check_comp_python_reroute(device):
    """Compressor.process_items: the refused item runs alone through process(), the others as one per-item batch"""
    from music_mixing_style_transfer_amd.mixing_manipulator import Compressor
    names = ("threshold", "attack_time", "release_time", "ratio")
    params = [COMP_MIXED[0], (-30.0, 0.01, 1000.0, 8.0), COMP_MIXED[1], COMP_MIXED[2]]
    values = [dict(zip(names, p)) for p in params]
    x = torch.from_numpy(R.comp_input(4133, 4, 2, 12)).to(device)
    c = Compressor(44100)
    y = c.process_items(x, values)
    others = [0, 2, 3]
    for i in range(4):
        for k, v in values[i].items():
            getattr(c.parameters, k).value = v
        want = c.process(x[i:i + 1])[0] if i == 1 else c.process(x[others].contiguous())[others.index(i)]
        assert same_bits(y[i].cpu().numpy(), want.cpu().numpy()), f"process_items item {i}"


def trace_comp_items_cases(emu):
    run = CompItemsRunner(emu, "cpu")
    tr = ItemsTracer(emu)
    for L, n, Cn, forms, fused in COMP_SAME:
        with tr:
            R._comp_call(run, np.zeros((n, L, Cn), np.float32), *BASE, 44100.0, COMP_SCALE[:n] if fused else None, fused, max(forms, 0), forms >= 0, False, False)
    return tr.seen
