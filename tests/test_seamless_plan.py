"""Seam-free conversion, the part that needs no kernel: the window plan (inference/segmentation.py plan_windows), the net's context
(TCNModel.context) and - the test with teeth for the halo - the plan driving the float64 oracle.

A halo one sample short changes the result by 5.9e-6 on the case below: under every GPU tolerance of the project (1e-4 at best), so only
float64 on the CPU can tell a right halo from an off-by-one.  Clipped windows reproduce the whole-sequence forward exactly in float64 (the
same products in the same order per output sample: measured 0.0); the bound 1e-12 is a few thousand float64 roundings of values below 1,
room for a convolution backend that picks another summation order for another length."""
import pytest
import torch

W = 1024


def _brute(L, window, h_l, h_r):
    """The definition, sample by sample: output sample t belongs to window t // window; the window reads every sample within the halo of any
    of its outputs, as far as the stem has them."""
    plan = {}
    for t in range(L):
        i = t // window
        first, last = max(0, t - h_l), min(L - 1, t + h_r)          # the samples output t reads, as far as the stem has them
        a, b, lo, hi = plan.get(i, (t, t + 1, first, last + 1))
        plan[i] = (min(a, t), max(b, t + 1), min(lo, first), max(hi, last + 1))
    return [plan[i] for i in sorted(plan)]


@pytest.mark.parametrize("halos", [(441, 441), (882, 0), (0, 0), (3000, 3000)], ids=["noncausal", "causal", "none", "longer-than-window"])
@pytest.mark.parametrize("L", [1, W - 1, W, W + 1, 5000, 3 * W])
def test_plan_windows_against_the_definition(L, halos):
    from music_mixing_style_transfer_amd.inference import segmentation as seg
    h_l, h_r = halos
    plan = seg.plan_windows(L, W, h_l, h_r)
    assert plan == _brute(L, W, h_l, h_r)
    assert all(isinstance(v, int) for w in plan for v in w)
    # the output ranges tile [0, L) in order, a_i = i W
    assert plan[0][0] == 0 and plan[-1][1] == L
    assert all(w[0] == i * W and w[1] == min(L, (i + 1) * W) for i, w in enumerate(plan))
    assert all(plan[i][1] == plan[i + 1][0] for i in range(len(plan) - 1))
    assert len(plan) == (L + W - 1) // W                      # L <= W: one item
    for a, b, lo, hi in plan:
        assert lo == max(0, a - h_l) and hi == min(L, b + h_r) and 0 <= lo <= a < b <= hi <= L      # clipped, never past the stem
    # at most three window shapes: first, interior, last; interior windows are all W + h_l + h_r long
    interior = [w for w in plan if w[2] == w[0] - h_l and w[3] == w[1] + h_r and w[1] - w[0] == W]
    assert all(hi - lo == W + h_l + h_r for _, _, lo, hi in interior)
    # sharding cuts the LIST of windows: whatever the world size, the ranks' runs put together are the one plan
    for world in (1, 2, 3, 8):
        runs = [plan[slice(*seg.shard_range(len(plan), r, world))] for r in range(world)]
        assert [w for run in runs for w in run] == plan


def test_plan_windows_refuses_bad_arguments():
    from music_mixing_style_transfer_amd.inference import segmentation as seg
    for bad in (0, -1):
        with pytest.raises(ValueError, match="window"):
            seg.plan_windows(5000, bad, 441, 441)
    with pytest.raises(ValueError):
        seg.plan_windows(5000, W, -1, 441)
    assert seg.plan_windows(0, W, 441, 441) == []


def _windowed(forward, x, plan):
    y = torch.empty(2, x.shape[-1], dtype=x.dtype)
    for a, b, lo, hi in plan:
        y[:, a:b] = forward(x[None, :, lo:hi])[0][:, a - lo:a - lo + (b - a)]
    return y


def test_plan_reproduces_the_whole_sequence_forward_in_float64():
    """6 blocks (H = 441), L = 5000, W = 1024: five windows, first and last clipped.  Right halo: <= 1e-12.  Both halos one short: > 1e-9
    (measured 5.9e-6) - an off-by-one in the halo, in the clipping or in the kept range cannot pass both."""
    from music_mixing_style_transfer_amd.inference import segmentation as seg
    from music_mixing_style_transfer_amd.networks import TCNModel
    from music_mixing_style_transfer_amd.utils import synth
    from oracle import networks_ref as R
    nblocks, L = 6, 5000
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in synth.tcn_state_dict(nblocks=nblocks, seed=2).items()}
    x = synth.synth_audio((2, L), seed=5).double()
    e = synth.synth_audio((1, 2048), seed=9, key="cond").double()
    forward = lambda xi: R.tcn_forward(sd, xi, e, nblocks=nblocks)
    whole = forward(x[None])[0]
    m = TCNModel(nparams=2048, ninputs=2, noutputs=2, nblocks=nblocks, dilation_growth=2, kernel_size=15, channel_width=128, stack_size=15,
                 cond_dim=2048, causal=False)
    h_l, h_r = m.context()
    assert (h_l, h_r) == (441, 441) == ((R.tcn_receptive_field(nblocks) - 1) // 2,) * 2
    right = float((_windowed(forward, x, seg.plan_windows(L, W, h_l, h_r)) - whole).abs().max())
    short = float((_windowed(forward, x, seg.plan_windows(L, W, h_l - 1, h_r - 1)) - whole).abs().max())
    rms = float(whole.pow(2).mean().sqrt())
    print(f"float64 oracle, 6 blocks, L {L}, W {W}: windowed vs whole {right:.3e}, halo one short {short:.3e}, output rms {rms:.3f}")
    assert rms > 0.05
    assert right <= 1e-12
    assert short > 1e-9
    # the alternative the definition rules out: windows extended with ZEROS past the stem's ends instead of clipped
    def zero_extended(a, b):
        xp = torch.zeros(1, 2, (b - a) + h_l + h_r, dtype=x.dtype)
        s0, s1 = max(0, a - h_l), min(L, b + h_r)
        xp[0, :, s0 - (a - h_l):s0 - (a - h_l) + (s1 - s0)] = x[:, s0:s1]
        return forward(xp)[0][:, h_l:h_l + (b - a)]
    ext = torch.cat([zero_extended(a, b) for a, b, _, _ in seg.plan_windows(L, W, h_l, h_r)], -1)
    assert float((ext - whole).abs().max()) > 1e-3


def test_context_of_the_net():
    """(rf - 1) / 2 on each side for a non-causal net - 114681 for the default configuration -, also where stack_size restarts the dilations;
    (rf - 1, 0) for a causal one."""
    import os
    import yaml
    from music_mixing_style_transfer_amd.networks import TCNModel
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(here, "music_mixing_style_transfer_amd", "networks", "configs.yaml")) as f:
        c = yaml.full_load(f)["TCN"]["default"]

    def net(**over):
        kw = dict(nparams=c["condition_dimension"], ninputs=2, noutputs=2, nblocks=c["nblocks"], dilation_growth=c["dilation_growth"],
                  kernel_size=c["kernel_size"], channel_width=c["channel_width"], stack_size=c["stack_size"],
                  cond_dim=c["condition_dimension"], causal=c["causal"])
        kw.update(over)
        if "small" in over:
            kw.pop("small")
            kw.update(nparams=16, cond_dim=16, channel_width=8)
        return TCNModel(**kw)
    m = net(small=True)
    rf = m.compute_receptive_field()
    assert rf == 229363 and m.context() == ((rf - 1) // 2, (rf - 1) // 2) == (114681, 114681)
    m = net(small=True, nblocks=7, stack_size=3)            # dilations 1 2 4 1 2 4 1
    rf = m.compute_receptive_field()
    assert rf == 1 + 14 * (1 + 2 + 4 + 1 + 2 + 4 + 1) and m.context() == ((rf - 1) // 2, (rf - 1) // 2)
    m = net(small=True, nblocks=5, causal=True)
    rf = m.compute_receptive_field()
    assert rf == 1 + 14 * 31 and m.context() == (rf - 1, 0)
