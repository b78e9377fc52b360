"""Each FXencoder kernel ALONE against an operand-exact float64 reference, element by element (tests/enc_block_ref.py) - the encoder's
counterpart of tests/test_tcn_block_exact.py.

The other numeric encoder tests run n blocks from the waveform against the fp32 oracle and accept a few per cent of the tensor's largest
element, or compare one product kernel with another.  With reductions of up to 10240 products a dropped (tap, channel-chunk) pair, a reflection
index off by one, a split-K slice left out, truncation instead of rounding or a lost x_lo w_hi term hides in that room.  Here block n reads
what the kernels themselves produced behind block n - 1 (forward_blocks), its reference is float64 on the very operands the kernels multiply,
and the bound is per element:

    bound = (1 + u_out) E1 + u_out |y|,    E = c U32 S + fold + dshift + 4 U32 (|z| + |x|) + In

(enc_block_ref.block_ref derives every term, the never-observable intermediate's sparse rounding flips among them.)  EVERY element of EVERY
block of every case is compared, twice: against the primary bound with c_acc = 4 sqrt(K + 8) and against the rigorous one (K + 8 + the split-K
slices; the sum of the absolute input uncertainties).  The pool is checked alone on the probe's bits (the forward's launch list has to be the
probe's plus the pool), embedding_mean on its rows, and the kernels no Res block reaches get cases of their own.

Completeness is asserted: the kernels the CPU case list executes and checks, and those the GPU case list does, each have to be the whole
exported enc_* / embedding_mean set.  Measured max err / bound per (kernel, precision): DESIGN.md, "Parity".
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import enc_block_ref as E  # noqa: E402

ALL = ("bf16", "bf16x3", "fp32")

NETS = {
    # blocks 1 / 2 are the default encoder's (16 / 32 channels, k = 25 / 15): the stereo kernel and both enc_block1_fused forms
    "b1": E.net_cfg([2, 16, 32, 64], [25, 25, 15], [4, 4, 2]),
    "b1l": E.net_cfg([2, 16, 32, 64], [25, 25, 15], [4, 4, 2], "lrelu"),
    # the raw-rows kernel's four instantiations (k = 5 / 10, stride 1 / 2), one to five channel blocks, ragged channel tiles (192, 320)
    "t1": E.net_cfg([2, 16, 64, 128, 256], [25, 10, 10, 5], [4, 2, 2, 1]),
    "t2": E.net_cfg([2, 16, 64, 128, 128, 256], [25, 10, 10, 5, 5], [4, 2, 1, 2, 1]),
    "t3": E.net_cfg([2, 16, 64, 192, 320], [25, 10, 5, 10], [4, 2, 2, 1]),
    # the LDS-resident rows form: strides 1 / 2 / 4, even kernels, mw 1 / 2
    "r": E.net_cfg([2, 16, 32, 32, 64], [25, 10, 15, 5], [4, 2, 1, 2]),
    # weight-heavy 128 / 256-channel layers: weight-major order, split-K
    "w": E.net_cfg([2, 16, 32, 128, 256], [25, 10, 5, 5], [4, 2, 2, 1]),
    # not enc_nlc_eligible: the NCL kernels in every mode, mw 1 / 2 / 4, even kernels
    "n": E.net_cfg([2, 4, 40, 72, 136], [5, 4, 3, 10], [2, 2, 1, 2]),
    # block 0 on enc_direct_kernel (no stereo form): 8 / 24 / 32 output channels, a 4-channel input, the shortest-input net
    "d8": E.net_cfg([2, 8, 16], [9, 5], [2, 2]),
    "d24": E.net_cfg([2, 24, 48], [25, 4], [4, 1]),
    "d32": E.net_cfg([2, 32, 64], [7, 15], [3, 2]),
    "d4": E.net_cfg([4, 16, 32], [25, 25], [4, 4]),
    "s": E.net_cfg([2, 16], [25], [4]),
    # wide layers (>= 512 channels): short lengths only on the emulator
    "wide": E.net_cfg([2, 16, 128, 512, 512], [25, 5, 5, 5], [4, 4, 2, 1]),
}
SEED = {k: 31 + i for i, k in enumerate(NETS)}


def _build_cpu_cases():
    """(net, B, L, precision, schedule, rows_min_tiles)."""
    cases = []

    def add(net, B, L, precisions=ALL, schedule=1, rmt=512):
        for p in precisions:
            c = (net, B, L, p, schedule, rmt)
            if c not in cases:
                cases.append(c)

    # one tile / many tiles / a last tile of one output (stereo: 240 outputs per tile; block1: 256; direct: 256), lengths that are no
    # multiples of the strides, the shortest input the reflection allows (13 samples at k = 25: the mirror at both ends reaches across the item)
    for B, L in ((1, 13), (2, 14), (1, 41), (2, 957), (1, 961), (1, 965), (3, 1000), (1, 4001)):
        add("s", B, L)
        add("s", B, L, ("bf16", "bf16x3"), 1 | 8)              # two enc_direct_kernel launches instead of the stereo kernel
    for B, L in ((2, 8150), (1, 16003), (3, 4000), (1, 200), (2, 3997), (1, 4097), (1, 16385)):
        add("b1", B, L)
    add("b1", 2, 3997, ("bf16",), 1 | 16)                       # blocks 1 / 2 as two launches each
    add("b1", 2, 8150, ("bf16",), 1 | 16, 0)                    # ... on the rows kernel
    add("b1", 1, 16385, ("bf16", "bf16x3"), 1, 0)
    add("b1", 1, 16385, ("bf16", "bf16x3"), 1 | 8, -1)
    add("b1l", 2, 3997)
    add("b1l", 1, 200, ALL, 1 | 8 | 16)
    # the raw-rows kernel: Lout % 32 on both sides, items of 32 columns (8 per 256-column tile), tiles that end inside the batch, B = 1,
    # its split-K at 1 / 2 / more slices, the four-wave im2col kernel in its place (bit 5), the weight-major order off (bit 0 clear), the
    # 64-bit gather fall-back of the exact-fp32 kernel (bit 2)
    for B, L in ((3, 4096), (1, 2048), (3, 512), (5, 1024), (2, 1000)):
        add("t1", B, L)
    add("t1", 3, 512, ("bf16",), 1 | 32)
    add("t1", 5, 1024, ("bf16", "bf16x3"), 0)
    add("t1", 2, 1000, ("fp32",), 1 | 4)
    add("t1", 1, 2048, ("bf16", "bf16x3"), 1, 0)                # the rows form on the 64- and 128-channel layers (mw 2 / 4), one tile per item
    add("t1", 3, 4100, ("bf16", "bf16x3"), 1, 0)                # ... several tiles, the last one ragged
    for B, L in ((2, 4096), (5, 1024), (1, 3000), (3, 512)):
        add("t2", B, L)
    add("t2", 2, 4096, ("bf16",), 1 | 32)
    for B, L in ((2, 2048), (3, 1024), (1, 1023)):
        add("t3", B, L)
    add("t3", 3, 1024, ("bf16", "bf16x3"), 0)
    add("t3", 3, 1024, ("bf16",), 32)
    # the rows form wherever it qualifies (rows_min_tiles 0), nowhere (-1), by its own threshold (512: not at these sizes in bf16)
    for B, L in ((2, 5000), (1, 4097), (1, 8192)):
        for rmt in (0, -1, 512):
            add("r", B, L, ALL if rmt == 512 else ("bf16", "bf16x3"), 1, rmt)
    for B, L in ((3, 3000), (1, 512), (8, 256)):
        add("w", B, L)
        add("w", B, L, ("bf16", "bf16x3"), 0)
    add("w", 3, 3000, ("fp32",), 1 | 4)
    for B, L in ((3, 333), (1, 40), (2, 2049), (5, 128)):
        add("n", B, L)
    add("n", 3, 333, ("fp32",), 1 | 4)
    for net, shapes in (("d8", ((2, 700), (1, 513), (3, 9))), ("d24", ((2, 1025), (1, 13))), ("d32", ((2, 770), (1, 64))), ("d4", ((2, 2037), (1, 1100)))):
        for B, L in shapes:
            add(net, B, L)
    add("wide", 2, 512)
    add("wide", 1, 1024, ("bf16",))
    add("wide", 3, 256, ("bf16", "bf16x3"), 0)
    return cases


CPU_CASES = _build_cpu_cases()

DEFAULT = "default"          # configs.yaml Effects_Encoder.default, read when a case needs it


def _net(key):
    if key == DEFAULT:
        import yaml
        from music_mixing_style_transfer_amd import networks
        with open(os.path.join(os.path.dirname(networks.__file__), "configs.yaml")) as f:
            c = yaml.safe_load(f)["Effects_Encoder"]["default"]
        return E.net_cfg([2] + list(c["channels"]), c["kernels"], c["strides"], c["activation"])
    return NETS[key]


# the default encoder, all 12 blocks, at the bench's shape, at 2^19 samples, at a ragged length, with tiles that end inside the batch; the
# schedule flags and rows thresholds at a short length; the ragged-channel net; the NCL and direct-kernel nets
GPU_CASES = ([(DEFAULT, B, L, p, 1, 512) for B, L in ((32, 131072), (2, 1 << 19), (2, 100003), (5, 131072)) for p in ALL] +
             [(DEFAULT, 2, 16384, p, f, 512) for f in (1 | 8, 1 | 16, 1 | 32, 0) for p in ("bf16", "bf16x3")] +
             [(DEFAULT, 2, 16384, "fp32", 1 | 4, 512)] +
             [(DEFAULT, 2, 16384, p, 1, rmt) for rmt in (0, -1) for p in ("bf16", "bf16x3")] +
             [("t3", 3, 4096, p, 1, 512) for p in ALL] + [("t2", 5, 1024, p, 1, 512) for p in ALL] + [("r", 2, 5000, p, 1, 0) for p in ("bf16", "bf16x3")] +
             [(net, 3, 2049, p, 1, 512) for net in ("n", "d8", "d24", "d32", "d4") for p in ALL] + [("b1l", 2, 3997, p, 1, 512) for p in ALL])

# Conv1d_layer alone (mst_enc_forward_conv: exact-fp32 kernel, no split-K): (cin, cout, k, stride, padding, B, L)
SINGLE_CONVS = [(3, 20, 7, 2, "VALID", 2, 301), (24, 64, 4, 1, "VALID", 3, 130), (40, 136, 10, 3, "VALID", 1, 517), (8, 32, 5, 1, "SAME", 2, 64),
                (16, 16, 3, 2, "VALID", 2, 3)]
# mst_enc_zero_stuff: (rows, L, stride, pad_left, Lu)
ZERO_STUFF = [(6, 100, 2, 3, 3 + 99 * 2 + 1 + 4), (1, 1, 1, 0, 1), (5, 333, 4, 0, 1329), (3, 257, 3, 7, 7 + 256 * 3 + 1), (2, 64, 1, 2, 70)]
MEAN_ROWS = [(1, 40), (7, 40), (33, 2048), (400, 513)]


def _case_id(c):
    return "-".join(str(v) for v in c)


@pytest.fixture(scope="module")
def tracer(emu):
    t = E.EncTracer(emu)
    yield t
    t.close()


def _run_case(lib, tracer, case, dev=None, s_dtype=torch.float64):
    net, B, L, prec, schedule, rmt = case
    cfg = _net(net)
    _, per_block, fwd, same = tracer.checked_kernels(cfg, B, L, prec, schedule, rmt)
    # the forward runs the very launches of the probe, then the pool: its last activation has the probe's bits, and the embedding may be held
    # to the pool's own summation bound on them
    assert same, (per_block, fwd)
    m, sd = E.make_model(cfg, seed=0 if net == DEFAULT else SEED[net])
    x = E.make_enc_input(B, cfg["channels"][0], L, seed=100 + L)
    if dev is not None:
        m, x = m.to(dev), x.to(dev)
    m.precision = prec
    E.set_flags(m, lib, schedule, rmt)
    return E.check_model(m, sd, cfg, x, prec, per_block + [[fwd[-1]]], same, s_dtype=s_dtype, label=_case_id(case))


TEETH_FACTOR = 8.0
"""The bound must keep its teeth: the median over the non-tiny |y| of bound / |y| may be at most this multiple of its irreducible parts
(enc_block_ref.teeth_unit): the rounding of the output at the mode's precision and the accumulation / fold terms the check is defined with,
u + (c_acc(K) + fold) U32 median(S / |y|).  Everything else in the bound is the never-observable intermediate: its own accumulation bound
and its roundings and flips, propagated at IN_LAMBDA = 4 standard deviations through the second conv - a second term of the size of the
first times 4 / sqrt(the number of contributing elements), worst where K is small - and the epilogue's few ulps.  8 = 4 (IN_LAMBDA), doubled;
measured on the reference alone <= 5.6, on wide layers (K >= 1000) <= 3.7.  In bf16 mode the unit is UBF = 2^-8 plus an accumulation term of
at most the same size up to K = 10240; in fp32 / bf16x3 mode the accumulation term IS the unit: u_out is 6e-8 / 1.5e-5, c_acc(K) U32 S / |y|
measures 4e-5 ... 1e-3 (S / |y| of sums of K random-sign products grows like sqrt(K)) - DESIGN.md section 5."""


@pytest.mark.parametrize("case", CPU_CASES, ids=_case_id)
def test_every_block_of_the_case_within_its_derived_bound_emulated(emu_default, tracer, case):
    ratios, infos = _run_case(emu_default, tracer, case)
    for (kname, p), (r1, r2) in sorted(ratios.items()):
        print(f"RATIO\t{kname}\t{p}\t{r1:.4f}\t{r2:.5f}")
    for info in infos:
        assert not info["teeth"] > TEETH_FACTOR, info


def _reached(tracer, cases):
    seen = set()
    for net, B, L, prec, schedule, rmt in cases:
        seen |= tracer.checked_kernels(_net(net), B, L, prec, schedule, rmt)[0]
    return seen


def _direct_reach(tracer):
    """What the direct cases execute and check: Conv1d_layer alone, mst_enc_zero_stuff, mst_embedding_mean (the names asserted from a trace)."""
    emu = tracer.emu
    seen = set()
    for cin, cout, k, stride, padding, B, L in SINGLE_CONVS:
        cfg = E.net_cfg([cin, cout], [k], [stride])
        if padding == "VALID":
            seen |= set(tracer.conv_launches(cfg, B, L))
    d = tracer.dummy
    seen |= {f[0] for f in tracer.traced(lambda: emu.mst_enc_zero_stuff(d, d, 2, 8, 2, 0, 15, None))}
    seen |= {f[0] for f in tracer.traced(lambda: emu.mst_embedding_mean(d, 3, 5, d, None))}
    seen |= {f[0] for f in tracer.traced(lambda: emu.mst_global_avgpool(d, d, 4, 9, None))}
    return seen


def _assert_complete(emu, tracer, cases):
    exported = E.exported_enc_kernels(emu.path)
    in_sources = E.launched_in_sources()
    assert len(in_sources) >= 30 and len(exported) >= len(in_sources), (len(exported), sorted(in_sources))
    seen = _reached(tracer, cases) | _direct_reach(tracer)
    assert sorted(E.kernel_name(s) for s in exported - seen) == [], "exported kernels no case of the list executes and checks"
    assert sorted(seen - exported) == []
    return exported


def test_the_cpu_cases_execute_and_check_every_exported_encoder_kernel(emu, tracer):
    exported = _assert_complete(emu, tracer, CPU_CASES)
    # (the assertion has teeth: without the cases of the default schedule value, or of the rows threshold 0, kernels go unreached)
    direct = _direct_reach(tracer)
    assert exported - (_reached(tracer, [c for c in CPU_CASES if c[4] != 1]) | direct)
    assert exported - (_reached(tracer, [c for c in CPU_CASES if c[5] != 0]) | direct)


def test_the_gpu_cases_reach_every_exported_encoder_kernel_at_their_real_sizes(emu, tracer):
    _assert_complete(emu, tracer, GPU_CASES)


FLIP_CAP = 0.20
"""The near-tie allowance has to stay SPARSE.  A float64 t within E0 of a rounding tie is granted a flip; ties are one bf16 ulp apart, so the
expected share of such elements is mean(min(1, 2 E0 / ulp(t))) (a value's position inside its cell is uniform for all practical purposes).
Per block and item the measured share may exceed that expectation by half plus one point (the cells of small |t| are few and unevenly
filled; items whose input is constant - digital silence - are left out: every time step of a channel is the same number there, near a tie
or not); and no block of the CPU cases may come to more than FLIP_CAP = 0.15: E0 = c_acc(K) U32 S0 against ulp >= 2^-8 |t| gives
2 c_acc(K) U32 2^8 S0 / |t| = 0.005 ... 0.08 for K = 400 ... 2560 at the measured S0 / |t| of 3 ... 12, times the margin."""


def test_the_reference_alone_is_inside_a_quarter_of_the_primary_bound():
    """The constants are fixed against the REFERENCE, never against the kernels.  On the operands of every conv of the CPU case list:
    torch-CPU conv1d in fp32 (its own summation order) against float64 has to stay under sqrt(K + 8) U32 S, a quarter of the primary
    accumulation term; two fp32 evaluations of the intermediate in different summation orders (conv1d; tap by tap), each rounded as the mode
    stores it, through the float64 second conv, differ by at most IN_LAMBDA / 4 of sqrt(sum (d w)^2), the unit of the primary input term;
    the share of intermediate elements granted a flip stays under its cap (FLIP_CAP); the bound keeps its teeth (TEETH_FACTOR).
    The chain runs without any kernel: block n + 1 reads the fp32 reference result of block n, stored as the mode stores it."""
    F = torch.nn.functional
    worst_acc, worst_in, worst_flip, worst_teeth = {}, 0.0, (0.0, 0.0, None), {}
    done = set()
    for net, B, L, prec, _, _ in CPU_CASES:
        if (net, B, L, prec) in done:
            continue
        done.add((net, B, L, prec))
        cfg = NETS[net]
        nlc = E.nlc_eligible(cfg)
        _, sd = E.make_model(cfg, seed=SEED[net])
        a = E.make_enc_input(B, cfg["channels"][0], L, seed=100 + L)
        for n in range(len(cfg["kernels"])):
            mode = E.block_mode(prec, nlc, n)
            y, b1, _, info = E.block_ref(sd, cfg, n, a, prec, nlc)
            big = y.abs() > 1e-3 * float(y.abs().max().clamp_min(1e-30))
            if bool(big.any()):
                teeth = float((b1[big] / y[big].abs()).median()) / E.teeth_unit(info, y, big)
                if teeth > worst_teeth.get(mode, (0.0, None))[0]:
                    worst_teeth[mode] = (teeth, (net, B, L, prec, n))
            if "flip_share" in info:
                assert info["flip_share"] <= FLIP_CAP, (net, B, L, prec, n, info["flip_share"], info["flip_expected"])
                for share, expected in info["flip_items"]:
                    assert share <= 1.5 * expected + 0.01, (net, B, L, prec, n, share, expected)
                if info["flip_share"] > worst_flip[0]:
                    worst_flip = (info["flip_share"], info["flip_expected"], (net, B, L, prec, n))
            # the two convs on fp32-representable operands (bf16 modes: the rounded ones; split mode: wh + wl needs more than 24 bits - its
            # accumulation is the bf16 modes' with three exact products per term)
            xin, skip, t_pair = a.double(), a.double(), None
            for which in (0, 1):
                g = E.geometry(cfg["kernels"][n], cfg["strides"][n] if which else 1)
                wp, shift, _ = E.folded(sd, f"encoder.{n}.conv{which + 1}.conv1d.")
                K = wp.shape[1] * wp.shape[2]
                w16 = mode in ("ncl16", "nlc16", "nlc3")
                wq = E.bf16_rne(wp) if w16 else wp.double()
                X = E.bf16_rne(xin) if w16 else xin
                pad = X[:, :, E.reflect_index(X.shape[2], g["pad_l"], g["pad_r"], X.device)]
                acc64, S = E.conv(X, wq, g), E.conv(X.abs(), wq.abs(), g)
                acc32 = F.conv1d(pad.float(), wq.float(), None, stride=g["stride"])
                r = float(((acc32.double() - acc64).abs() / (E.U32 * S).clamp_min(1e-300)).max())
                worst_acc[K] = max(worst_acc.get(K, 0.0), r)
                assert r <= math.sqrt(K + 8), (net, n, which, K, r)
                if which == 0:
                    acc32b = E.conv(X.float(), wq.float(), g)
                    store = (lambda v: E.bf16_rne(v)) if mode in ("ncl16", "nlc16") else (lambda v: v.double())
                    t_pair = [store(E.act(acc.double() + shift[None, :, None], cfg["slope"]).float() + skip.float()) for acc in (acc32, acc32b)]
                    xin = E.act(acc64 + shift[None, :, None], cfg["slope"]) + skip
                elif "in_unit" in info and mode != "nlc3":
                    d = (E.conv(t_pair[0], wq, g) - E.conv(t_pair[1], wq, g)).abs()
                    worst_in = max(worst_in, float((d / info["in_unit"].clamp_min(1e-300))[d > 0].max()) if bool((d > 0).any()) else 0.0)
            a = {"fp32": y.float(), "ncl16": y.float(), "nlc16": E.bf16_rne(y).float(), "stereo": E.bf16_rne(y).float(), "nlc3": y.float()}[mode]
            if prec == "bf16x3" and mode in ("stereo", "nlc3"):
                hi = E.bf16_rne(y)
                a = (hi + E.bf16_rne(y - hi)).float()
    ks = sorted(worst_acc)
    print("reference alone: max |acc32 - acc64| / (U32 S) per K (sqrt(K + 8)): " + ", ".join(f"{k}: {worst_acc[k]:.2f} ({math.sqrt(k + 8):.1f})" for k in ks))
    print(f"reference alone: two fp32 evaluations of the intermediate through the float64 second conv: max difference / sqrt(sum (d w)^2) = {worst_in:.3f} "
          f"(IN_LAMBDA / 4 = {E.IN_LAMBDA / 4})")
    print(f"reference alone: largest near-tie share {worst_flip[0]:.4f} (expected {worst_flip[1]:.4f}) at {worst_flip[2]}, cap {FLIP_CAP}")
    for mode, (teeth, where) in sorted(worst_teeth.items()):
        print(f"reference alone: {mode}: largest median bound / |y| in units of (u + (c_acc + fold) U32 median S / |y|): {teeth:.2f} at {where} (allowed {TEETH_FACTOR})")
    assert worst_in <= E.IN_LAMBDA / 4 * (1.0 + 1e-9)          # (a lone flip through one weight is exactly 1 of the unit)
    assert all(teeth <= TEETH_FACTOR for teeth, _ in worst_teeth.values())


# ---- the kernels no Res block reaches ----

def _single_conv(lib, cin, cout, k, stride, padding, B, L, dev):
    from music_mixing_style_transfer_amd.networks.network_utils import Conv1d_layer
    from music_mixing_style_transfer_amd.utils import synth
    layer = Conv1d_layer(cin, cout, k, stride=stride, padding=padding, activation="lrelu").eval()
    sd = synth.fxencoder_state_dict({"channels": [cin, cout], "kernels": [k]}, seed=cin + k)
    layer.load_state_dict({key[len("encoder.0.conv2."):]: v for key, v in sd.items() if key.startswith("encoder.0.conv2.")})
    x = E.make_enc_input(B, cin, L, seed=L)
    if dev is not None:
        layer, x = layer.to(dev), x.to(dev)
    got = layer(x)
    g = E.geometry(k, stride, valid=padding == "VALID")
    y, b1, b2 = E.single_conv_ref(sd, "encoder.0.conv2.conv1d.", g, float(torch.tensor(0.01, dtype=torch.float32)), x)
    assert got.shape == y.shape
    err = (got.double() - y).abs()
    r1, r2 = float((err / b1).max()), float((err / b2).max())
    assert r1 <= 1.0 and r2 <= 1.0 and bool(torch.isfinite(err).all()), E.worst_report(err, b1 if r1 > 1.0 else b2, stride, f"Conv1d_layer {cin}->{cout} k={k}")
    return r1, r2


def _zero_stuff(lib, rows, L, stride, pad_left, Lu, dev):
    x = E.make_enc_input(1, rows, L, seed=L)[0].contiguous()
    if dev is not None:
        x = x.to(dev)
    y = torch.full((rows, Lu), float("nan"), dtype=torch.float32, device=x.device)
    lib.check(lib.mst_enc_zero_stuff(x.data_ptr(), y.data_ptr(), rows, L, stride, pad_left, Lu, lib.stream_ptr(x)), "mst_enc_zero_stuff")
    want = torch.zeros_like(y)
    want[:, pad_left:pad_left + (L - 1) * stride + 1:stride] = x
    assert torch.equal(y, want)          # a copy: bit for bit


def _embedding_mean(lib, n_rows, dim, dev):
    from music_mixing_style_transfer_amd.inference import embedding_mean
    from music_mixing_style_transfer_amd.utils import synth
    e = synth.synth_audio((n_rows, dim), seed=n_rows) * 3.0
    e[0] = 0.0
    if dev is not None:
        e = e.to(dev)
    m, p1, p2 = E.mean_ref(e, 0)
    err = (embedding_mean(e).double() - m).abs()
    r1, r2 = float((err / p1).max()), float((err / p2).max())
    assert r1 <= 1.0 and r2 <= 1.0, (n_rows, dim, r1, r2)
    return r1, r2


@pytest.mark.parametrize("conv", SINGLE_CONVS, ids=_case_id)
def test_a_conv_layer_alone_within_its_derived_bound_emulated(emu_default, tracer, conv):
    cin, cout, k, stride, padding, B, L = conv
    if padding == "VALID":
        ls = tracer.conv_launches(E.net_cfg([cin, cout], [k], [stride]), B, L)
        assert len(ls) == 1 and "enc_conv_kernel" in ls[0], ls
    _single_conv(emu_default, *conv, None)


def test_zero_stuff_pool_and_embedding_mean_alone_emulated(emu_default):
    for z in ZERO_STUFF:
        _zero_stuff(emu_default, *z, None)
    for n_rows, dim in MEAN_ROWS:
        _embedding_mean(emu_default, n_rows, dim, None)
    _pool_alone(emu_default, None)


def _pool_alone(lib, dev):
    """mst_global_avgpool (enc_avgpool_kernel) on rows of 1 ... 1000 steps: FXencoder's conv_block='conv' path calls it directly."""
    out = []
    for rows, Lf in ((3, 1), (5, 63), (8, 64), (130, 65), (4, 1000)):
        x = E.make_enc_input(1, rows, Lf, seed=Lf)[0].contiguous()
        if dev is not None:
            x = x.to(dev)
        y = torch.empty(rows, dtype=torch.float32, device=x.device)
        lib.check(lib.mst_global_avgpool(x.data_ptr(), y.data_ptr(), rows, Lf, lib.stream_ptr(x)), "mst_global_avgpool")
        m, p1, p2 = E.mean_ref(x, 1)
        err = (y.double() - m).abs()
        r1, r2 = float((err / p1).max()), float((err / p2).max())
        assert r1 <= 1.0 and r2 <= 1.0, (rows, Lf, r1, r2)
        out.append((r1, r2))
    return max(out)


# ---- on the MI355X ----

def _gpu_lib():
    from music_mixing_style_transfer_amd import _lib
    assert torch.cuda.is_available() and _lib.lib().path.endswith("libmst_hip.so")
    return _lib.lib(), torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_CASES, ids=_case_id)
def test_every_block_of_the_case_within_its_derived_bound_on_the_gpu(emu, tracer, case):
    """The reference runs in float64 ON THE GPU (torch matmul = DGEMM) for these sizes - it is still float64 of the same operands, S included.
    The launch lists come from the emulator build's dry run (its split-K slice counts are those of a 4-CU device: the symbols are the same,
    a finalize kernel apart where the real chip needs no slices).  Measured ("Parity"; profiles/enc_block_exact_mi355x.txt): channel-minor bf16
    blocks 0.48 - 0.99 of the primary bound (the output rounding itself), bf16x3 <= 0.34, fp32 <= 0.19; every case inside both bounds at the first run."""
    lib, dev = _gpu_lib()
    ratios, infos = _run_case(lib, tracer, case, dev)
    for (kname, p), (r1, r2) in sorted(ratios.items()):
        print(f"RATIO\t{kname}\t{p}\t{r1:.4f}\t{r2:.5f}")
    for info in infos:
        print(f"TEETH\t{_case_id(case)}\tblock {info['n']}\t{info['mode']}\tK {info['K'][1]}\tmedian bound/|y| {info['median']:.3e}\t{info['teeth']:.2f}\t"
              f"flip share {info.get('flip_share', 0.0):.4f}\texpected {info.get('flip_expected', 0.0):.4f}")
        assert not info["teeth"] > TEETH_FACTOR, info


@pytest.mark.gpu
def test_the_kernels_no_res_block_reaches_on_the_gpu():
    lib, dev = _gpu_lib()
    for conv in SINGLE_CONVS + [(64, 256, 10, 2, "VALID", 4, 20001)]:
        r1, r2 = _single_conv(lib, *conv, dev)
        print(f"RATIO\tenc_conv_kernel alone {_case_id(conv)}\tfp32\t{r1:.4f}\t{r2:.5f}")
    for z in ZERO_STUFF + [(64, 32768, 2, 4, 4 + 32767 * 2 + 1 + 5)]:
        _zero_stuff(lib, *z, dev)
    print("RATIO\tenc_zero_stuff_kernel\tfp32\t0.0000\t0.00000")
    for n_rows, dim in MEAN_ROWS:
        r1, r2 = _embedding_mean(lib, n_rows, dim, dev)
        print(f"RATIO\tembedding_mean_kernel {n_rows}x{dim}\tfp32\t{r1:.4f}\t{r2:.5f}")
    r1, r2 = _pool_alone(lib, dev)
    print(f"RATIO\tenc_avgpool_kernel alone\tfp32\t{r1:.4f}\t{r2:.5f}")
