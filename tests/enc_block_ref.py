"""TEST INFRASTRUCTURE: the teacher-forced, operand-exact, element-wise check of ONE FXencoder Res_ConvBlock (tests/test_enc_block_exact.py),
the encoder's counterpart of tests/tcn_block_ref.py, whose constants, accumulation bounds, reports and trace plumbing it reuses.

forward_blocks(x, n) returns the kernels' own activation behind block n - in bf16 mode the unpacked bf16 values, in bf16x3 mode hi + lo, both
exact in fp32 - so block n is checked alone: its input is what its kernels really read (forward_blocks(x, n); the waveform for block 0), its
reference is float64 of conv -> shift -> act -> + x -> conv -> shift -> act on the operands the kernels multiply, and no error compounds across
blocks.  The bound is per element and derived - see block_ref.  Everything runs on the device of its inputs (float64 on the CPU; float64 on
the GPU for the full-size segments), the strided reflection-padded conv written as k tap-wise matrix products so that both do it alike.
"""
import ctypes as C
import math
import os
import re

import torch

from tcn_block_ref import (FOLD_ULPS, PRECISION_ID, U32, UBF, PlanTracer, bf16_rne, c_acc, c_acc_rigorous, demangle_hint,  # noqa: F401
                           make_input, worst_report)

KERNEL_SYMBOL = re.compile(r"^_Z\d+(enc_[a-z0-9_]+_kernel|embedding_mean_kernel)")
MAX_SLICES = 16       # the largest split-K slice count any heuristic of mst_enc.hip returns (enc_splitk_f32: 16; enc_splitk, enc_splitk_taps: 8)
IN_LAMBDA = 4.0       # standard deviations granted to the propagated, element-wise independent uncertainty of the intermediate (block_ref)
C_POOL = 4.0          # the primary constant of a fp32 sum of n terms, c sqrt(n + 2): the factor of c_acc
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the convolution, as the kernels index it ----

def reflect_index(L, pad_l, pad_r, device):
    """Input positions of the reflection-padded signal: t < 0 -> -t, t >= L -> 2 (L - 1) - t (every kernel's `if (ti < 0) ti = -ti; ...`)."""
    t = torch.arange(-pad_l, L + pad_r, device=device).abs()
    return torch.where(t >= L, 2 * (L - 1) - t, t)


def out_length(L, g):
    return (L + g["pad_l"] + g["pad_r"] - (g["k"] - 1) * g["dil"] - 1) // g["stride"] + 1


def conv(x, w, g):
    """x [B, Cin, L], w [Cout, Cin, k] (same dtype) -> [B, Cout, Lout]: reflection padding pad_l / pad_r (none for VALID), dilation, stride."""
    L = x.shape[2]
    xp = x[:, :, reflect_index(L, g["pad_l"], g["pad_r"], x.device)] if g["pad_l"] or g["pad_r"] else x
    Lo = out_length(L, g)
    out = torch.zeros(x.shape[0], w.shape[0], Lo, dtype=x.dtype, device=x.device)
    for j in range(g["k"]):
        s = j * g["dil"]
        out += torch.matmul(w[:, :, j], xp[:, :, s:s + (Lo - 1) * g["stride"] + 1:g["stride"]])
    return out


def geometry(k, stride, dil=1, valid=False):
    """mst_enc_create: 'SAME' = total (k - 1) d of reflection padding, left = total // 2 (even kernels pad one more sample on the right)."""
    pad = 0 if valid else (k - 1) * dil
    return {"k": k, "stride": stride, "dil": dil, "pad_l": pad // 2, "pad_r": pad - pad // 2}


# ---- the host's BN fold ----

def folded(sd, prefix, eps=1e-5):
    """(W', shift, dshift) of one Conv1d_layer as mst_enc_load_conv computes them in fp32 (csrc/mst_host.h bn_fold):
    scale = gamma / sqrt(var + eps), W' = w * scale, shift = (beta - mean * scale) + bias * scale; one correctly rounded fp32 operation each
    in torch.  dshift [Cout] float64: what FOLD_ULPS fp32 ulps of every term of the shift come to (block_ref, "The fold")."""
    f = lambda k: sd[prefix + k].detach().to("cpu", torch.float32)
    scale = f("batch_norm.weight") / torch.sqrt(f("batch_norm.running_var") + torch.tensor(eps, dtype=torch.float32))
    ms, bs = f("batch_norm.running_mean") * scale, f("conv1d.bias") * scale
    shift = (f("batch_norm.bias") - ms) + bs
    dshift = 2.0 * FOLD_ULPS * U32 * (f("batch_norm.bias").abs() + ms.abs() + bs.abs() + shift.abs()).double()
    return (f("conv1d.weight") * scale[:, None, None]).to(torch.float32), shift.double(), dshift


def bf16_ulp(v):
    """One bf16 ulp at |v| (float64 tensor): |v| = m 2^e with m in [0.5, 1) -> 2^(e - 8); 0 at 0."""
    e = torch.frexp(v.abs())[1]
    return torch.where(v != 0, torch.ldexp(torch.ones_like(v), e - 8), torch.zeros_like(v))


def near_tie_fp32(wp, ulps):
    """One bf16 ulp of the fp32 tensor wp where it lies within `ulps` fp32 ulps of a bf16 rounding tie (low half 0x8000), 0 elsewhere."""
    low = (wp.contiguous().view(torch.int32) & 0xffff) - 0x8000
    return torch.where((low.abs() <= ulps) & (wp != 0), bf16_ulp(wp.double()), torch.zeros_like(wp, dtype=torch.float64))


def flip_allowance(t, e):
    """By how much bf16(t~) may differ from bf16(t) when |t~ - t| <= e (float64 tensors), and where.

    Both roundings fall into the same cell, and so agree bit for bit, unless rounding ties (the midpoints of neighbouring bf16 numbers) lie
    between t and t~, i.e. within e of t; every tie crossed moves the rounded value by one ulp.  The ties of a binade are (k + 1/2) u, so
    with u_lo the bf16 ulp at |t| - e and u_hi the one at |t| + e the allowance is
        n u_hi,   n = floor((|t| + e) / u_lo - 1/2) - ceil((|t| - e) / u_lo - 1/2) + 1   ties in [|t| - e, |t| + e]
    (counted on the finer grid, weighed with the coarser ulp where the interval straddles a binade border): 0 for most elements while
    e << u, one ulp for the share 2 e / u of them that sit near a tie.  Where |t| <= e or e > 4 u_hi (tiny |t|: a cell structure is no help)
    the dense e + 2 u_hi stands in.  Returns (sparse, dense, flag): the tie-counted allowances, the dense ones, where either is non-zero."""
    at = t.abs()
    lo = at - e
    u_hi, u_lo = bf16_ulp(at + e), bf16_ulp(lo.clamp_min(0.0))
    zero = torch.zeros_like(t)
    ok = (lo > 0) & (e <= 4 * u_hi) & (e > 0)
    ul = u_lo.clamp_min(1e-300)
    n = (torch.floor((at + e) / ul - 0.5) - torch.ceil(lo / ul - 0.5) + 1.0).clamp_min(0.0)
    sparse = torch.where(ok, n * u_hi, zero)
    dense = torch.where(~ok & (e > 0), e + 2 * u_hi, zero)
    return sparse, dense, (sparse > 0) | (dense > 0)


def act(z, slope):
    return torch.where(z > 0, z, slope * z)


def block_mode(precision, nlc, n):
    """Which arithmetic block n runs in (mst_enc.hip enc_run): 'fp32' - exact-fp32 NCL kernels (fp32 mode; bf16x3 on nets that are not
    enc_nlc_eligible); 'ncl16' - bf16 mode on such nets: enc_conv_bf16_kernel rounds fp32 NCL activations to bf16 while staging;
    'stereo' - block 0 of the channel-minor pipeline: fp32 operands on enc_stereo_block_kernel / enc_direct_kernel, the result stored as
    bf16 (bf16 mode) or hi + lo (bf16x3); 'nlc16' / 'nlc3' - blocks >= 1 of the pipeline in bf16 / split mode."""
    if precision == "fp32" or (precision == "bf16x3" and not nlc):
        return "fp32"
    if not nlc:
        return "ncl16"
    if n == 0:
        return "stereo"
    return "nlc16" if precision == "bf16" else "nlc3"


def block_ref(sd, cfg, n, a_in, precision, nlc, s_dtype=torch.float64):
    """float64 result of Res_ConvBlock n on the operands the kernels multiply, and two per-element bounds of |kernel - result|.

    a_in: the block's input as the kernels hold it - forward_blocks(x, n), or the waveform for n = 0.  cfg: channels (input first), kernels,
    strides, slope (c.slope as the kernels hold it: relu 0, lrelu float32(0.01)).  nlc: enc_nlc_eligible(net).
    Returns (y, bound, bound_rigorous, info); info: K of both convs, the share of intermediate elements granted a rounding flip and the
    share expected from E0 / ulp.

    One conv, input X (the operand values, exact), weights Wq (what the kernel multiplies), S = conv(|X|, |Wq|):
        z = conv(X, Wq) + shift,   v = act(z) (+ x for conv 0: the skip reads the block's input itself, in fp32 / bf16 / hi + lo as it lies)
        Ez = c U32 S                fp32 accumulation of K = Cin k exact products (bf16 x bf16 is exact in fp32; fp32 MFMA / fmaf round once per
                                    step) in ANY order: c = c_acc(K) = 4 sqrt(K + 8) primary, K + 8 + MAX_SLICES rigorous (split-K adds S <= 16 partial sums)
          + fold + dshift           the fold (below)
          + 2 U32 |z|               acc + shift
          + In                      what the uncertainty of the INPUT operand does (only conv 1 and split mode have one: below)
        E  = (z < -Ez ? slope Ez : Ez) + 2 U32 (|v| + |x|)
    act is 1-Lipschitz for every slope in [0, 1], so an error of z is at most that error behind it (the argument of
    tcn_block_ref.clamp_excess); where z is negative for certain (z < -Ez) the kernel multiplies by the slope like the reference and the
    error shrinks with it - relu: act is exactly 0 on both sides and the error ENDS there, which is what keeps the flips of the intermediate
    sparse.  2 U32 (|v| + |x|): the roundings of slope * z, of + x and of r_hi + r_lo.
    Output: bound = (1 + u_out) E1 + u_out |y| - one rounding of the stored value - with u_out = U32 (fp32 store), UBF (bf16 store) or
    UBF^2 + U32 (split store hi = bf16(v), lo = bf16(v - hi): |v - hi - lo| <= UBF |v - hi| <= UBF^2 |v|; the probe adds hi + lo in fp32).

    Operands per mode (block_mode; read from the kernels, not from their comments):
      fp32    X = a, Wq = W' (fp32).  t = fl32(v0) in HBM: the dense Et = E0 + U32 |t| goes through conv(Et, |W1'|) = In of conv 1.
      stereo  as fp32 (enc_stereo_block_kernel / enc_direct_kernel multiply fp32 waveform samples by fp32 W', fmaf chain; t in LDS / HBM as
              fp32); only the store differs.
      ncl16   X = bf16(a) (enc_conv_bf16_kernel rounds while staging; RNE, deterministic), Wq = bf16(W'); the skip adds the fp32 a; t is stored
              in fp32 and rounded when conv 1 stages it: X1 = bf16(t), flips (below) within E0 + U32 |t| of a tie.
      nlc16   X = a (bf16 exact), Wq = bf16(W'), X1 = bf16(t).  The kernel rounds ITS t~, |t~ - t| <= E0, and the two roundings differ only
              where a rounding tie lies within E0 of t: there by one bf16 ulp per tie, elsewhere by NOTHING (flip_allowance).  In of conv 1 is that
              sparse allowance through conv(f, |bf16(W1')|) - not a blanket UBF |t|, which at K in the thousands would swallow a dropped product.
      nlc3    W' = wh + wl + ew, wh = bf16(W'), wl = bf16(W' - wh) as mst_enc_load_conv splits it; a = ah + al as the producing kernel split
              it.  The kernels sum ah wh + ah wl + al wh = a wh + ah wl: the reference is conv(a, wh) + conv(bf16(a), wl), and the dropped
              al wl is no error of the kernel - it is absent from both.  ah is bf16(a) except where a = hi + lo sits exactly on a tie (lo was
              rounded up to half an ulp of hi): there ah may be either neighbour, one bf16 ulp of a times |wl|: In of conv 0, sparse.
              t = hi + lo of v0: dense Et = E0 + (UBF^2 + U32) |t| through |wh| + |wl|, and the flips of t_hi = bf16(t) within Et of a tie
              through |wl| alone (the sum t_hi + t_lo moves by Et only).  S = conv(|a|, |wh| + |wl|).

    The fold.  W' and the shift are a few fp32 operations away from the parameters, done once by the host code and once here by torch; on the
    MI355X hosts the two differed by one or two ulps (tcn_block_ref.block_ref, "The fold itself").  FOLD_ULPS ulps: fp32 / stereo / nlc3
    2 FOLD_ULPS U32 S; bf16 modes: invisible except for the weights within FOLD_ULPS ulps of a bf16 tie, which may be packed as either
    neighbour: conv(|X|, A), A one bf16 ulp there; nlc3 likewise for wl (a W' - wh within FOLD_ULPS ulps of W' of a tie of wl's grid: one
    bf16 ulp of wl) and for wh (either neighbour, wl follows: the sum moves by at most 4 UBF^2 |W'|).  dshift: the same for the shift's terms.
    """
    dev = a_in.device
    mode = block_mode(precision, nlc, n)
    slope = float(cfg["slope"])
    a = a_in.to(torch.float64)
    info = {"mode": mode, "K": []}
    x_dense = x_flip = x_lin = None          # [primary, rigorous] uncertainty of conv 1's input: per-element dense (through |W|), one-ulp flips (through the flip weights), and the flips' dense fall-back
    xin, skip = a, a
    S = z = E = None
    for which_conv in (0, 1):
        g = geometry(cfg["kernels"][n], cfg["strides"][n] if which_conv else 1)
        wp, shift, dshift = folded(sd, f"encoder.{n}.conv{which_conv + 1}.conv1d.")
        K = wp.shape[1] * wp.shape[2]
        info["K"].append(K)
        shift, dshift = shift.to(dev)[None, :, None], dshift.to(dev)[None, :, None]
        w64 = wp.double()
        if mode in ("fp32", "stereo"):
            wq, wabs, wflip = w64, w64.abs(), None
            X = xin
            fold_w = None
        elif mode in ("ncl16", "nlc16"):
            wq = bf16_rne(wp)
            wabs = wflip = wq.abs()
            X = bf16_rne(xin)          # nlc16 conv 0: the identity (a is bf16 exact)
            fold_w = near_tie_fp32(wp, FOLD_ULPS)
        else:
            wh = bf16_rne(wp)
            rest = (wp - wh.float())          # exact in fp32
            wl = bf16_rne(rest)
            wq, wabs, wflip = wh + wl, wh.abs() + wl.abs(), wl.abs()
            X = xin
            fold_w = near_tie_scaled(rest, wp) * bf16_ulp(wl) + 4.0 * UBF * UBF * w64.abs() * (near_tie_fp32(wp, FOLD_ULPS) > 0)
        to = lambda t: t.to(dev)
        if mode == "nlc3":
            acc = conv(X, to(wh), g) + conv(bf16_rne(X), to(wl), g)
        else:
            acc = conv(X, to(wq), g)
        S = conv(X.abs().to(s_dtype), to(wabs).to(s_dtype), g).to(torch.float64)
        if s_dtype != torch.float64:
            S = S * (1.0 + 2.0 * (K + 8) * U32)
        fold = 2.0 * FOLD_ULPS * U32 * S if mode in ("fp32", "stereo", "nlc3") else torch.zeros_like(S)
        if fold_w is not None and bool((fold_w != 0).any()):
            fold = fold + conv(X.abs(), to(fold_w), g)
        inp = torch.zeros_like(S)
        if which_conv == 0 and mode == "nlc3":
            tie = (a_in.to(torch.float32).contiguous().view(torch.int32) & 0xffff) == 0x8000
            if bool(tie.any()):
                inp = conv(torch.where(tie, bf16_ulp(a), torch.zeros_like(a)), to(wflip), g)
        # the input's uncertainty: each element's own, independent of its neighbours' - a rounding of t, a flip of its bf16 cell.  Rigorous:
        # the sum of the absolute terms.  Primary: IN_LAMBDA standard deviations of a sum of independent terms, sqrt(sum (d w)^2) - the rule of
        # c_acc, and like it fixed against the reference alone (test_the_reference_alone_...)
        if x_dense is not None or x_flip is not None:
            sq, lin = torch.zeros_like(S), torch.zeros_like(S)
            for d, wd in ((x_dense, wabs), (x_flip, wflip)):
                if d is not None:
                    sq = sq + conv(d[0] * d[0], to(wd * wd), g)
                    lin = lin + conv(d[1], to(wd), g)
            info["in_unit"] = torch.sqrt(sq)
            inp = [inp + IN_LAMBDA * torch.sqrt(sq) + (conv(x_lin[0], to(wflip), g) if x_lin is not None else 0.0),
                   inp + lin + (conv(x_lin[1], to(wflip), g) if x_lin is not None else 0.0)]
        else:
            inp = [inp, inp]
        z = acc + shift
        del acc
        # the error of z in front of the activation, then behind it: where z is negative for certain (z < -Ez) the activation multiplies it
        # by the slope - relu: the kernel's act is exactly 0 like the reference's and the error ends there - elsewhere act is 1-Lipschitz;
        # then the roundings of slope * z, of + x and of r_hi + r_lo
        v = act(z, slope)
        Ez = [c * U32 * S + fold + dshift + 2.0 * U32 * z.abs() + i for c, i in zip((c_acc(K), c_acc_rigorous(K) + MAX_SLICES), inp)]
        res = skip.abs() if which_conv == 0 else 0.0
        E = [torch.where(z < -e, slope * e, e) + 2.0 * U32 * (v.abs() + res) for e in Ez]
        if which_conv == 0:
            t = act(z, slope) + skip
            ut = {"fp32": U32, "stereo": U32, "ncl16": U32, "nlc16": 0.0, "nlc3": UBF * UBF + U32}[mode]
            # (relu clamped for certain: t~ is the block's input x itself, which the store represents exactly - fp32, bf16 or hi + lo as it came)
            Et = [torch.where((z < -ez) & (slope == 0.0), torch.zeros_like(e), (1.0 + ut) * e + ut * t.abs()) for e, ez in zip(E, Ez)]
            if mode in ("fp32", "stereo"):
                x_dense, xin = Et, t
            else:
                fl = [flip_allowance(t, e) for e in Et]          # the primary check with the primary E0, the rigorous one with the rigorous
                x_flip = [fl[0][0], fl[1][0]]
                x_lin = [fl[0][1], fl[1][1]]
                x_dense, xin = (Et, t) if mode == "nlc3" else (None, bf16_rne(t))
                info["flip_share"], info["flip_share_rigorous"] = float(fl[0][2].double().mean()), float(fl[1][2].double().mean())
                expect = (2.0 * Et[0] / bf16_ulp(t).clamp_min(1e-300)).clamp_max(1.0)
                info["flip_expected"] = float(expect.mean())
                # per item, for the items whose input is a signal: a constant input (digital silence) makes every time step of a channel the
                # same number, which sits near a tie or does not - no distribution to expect anything of
                live = ((a.amax(2) - a.amin(2)) > 0).any(1)
                info["flip_items"] = [(float(fl[0][2][b].double().mean()), float(expect[b].mean())) for b in range(a.shape[0]) if bool(live[b])]
            skip = None
    y = v
    u_out = {"fp32": U32, "ncl16": U32, "stereo": UBF if precision == "bf16" else UBF * UBF + U32, "nlc16": UBF, "nlc3": UBF * UBF + U32}[mode]
    info["u_out"], info["S"] = u_out, S
    bounds = [(1.0 + u_out) * e + u_out * y.abs() + 1e-37 for e in E]
    return y, bounds[0], bounds[1], info


def near_tie_scaled(rest, wp):
    """Where rest = W' - wh (fp32, exact) lies within FOLD_ULPS fp32 ulps OF W' of a rounding tie of its own bf16 grid: 1.0 there, 0 elsewhere."""
    r = rest.double()
    u = bf16_ulp(r)
    q = r.abs() / u.clamp_min(1e-300)
    dist = ((q - torch.floor(q)) - 0.5).abs() * u
    ulp32 = torch.ldexp(torch.ones_like(r), torch.frexp(wp.double().abs())[1] - 24)
    return ((dist <= FOLD_ULPS * ulp32) & (r != 0)).double()


def single_conv_ref(sd, prefix, g, slope, x, s_dtype=torch.float64):
    """One Conv1d_layer alone in exact-fp32 mode (mst_enc_forward_conv: enc_conv_kernel, no split-K): float64 act(conv(x, W') + shift) and
    its two bounds - block_ref's single-conv E with fp32 operands and an fp32 store."""
    wp, shift, dshift = folded(sd, prefix)
    K = wp.shape[1] * wp.shape[2]
    dev = x.device
    a = x.to(torch.float64)
    w64 = wp.double().to(dev)
    z = conv(a, w64, g) + shift.to(dev)[None, :, None]
    S = conv(a.abs(), w64.abs(), g)
    y = act(z, slope)
    out = [y]
    for c in (c_acc(K), c_acc_rigorous(K)):
        E = (c + 2.0 * FOLD_ULPS) * U32 * S + dshift.to(dev)[None, :, None] + 4.0 * U32 * z.abs()
        out.append((1.0 + U32) * E + U32 * y.abs() + 1e-37)
    return tuple(out)


def mean_ref(a, dim):
    """float64 mean over `dim` of the fp32 tensor a and the two bounds of a fp32 sum of n terms followed by one division:
    (n + 2) U32 mean|a| for any summation order (gamma_n and the division), C_POOL sqrt(n + 2) U32 mean|a| primary.
    The primary bound takes the n roundings for independent.  Over a CONSTANT row they are not: the same addend meets a partial sum of the
    same binade step after step and rounds the same way for whole stretches, a drift of up to a quarter ulp per step (measured on the silent
    item, whose activation is one number per channel: 0.25 of the rigorous bound at n = 313, 1.11 of the primary).  Such rows are held to the
    rigorous bound alone."""
    a64 = a.to(torch.float64)
    n = a.shape[dim]
    m, ma = a64.mean(dim), a64.abs().mean(dim)
    rigorous = (n + 2) * U32 * ma + 1e-37
    constant = (a64.amax(dim) - a64.amin(dim)) == 0
    return m, torch.where(constant, rigorous, C_POOL * math.sqrt(n + 2) * U32 * ma + 1e-37), rigorous


# ---- which kernel runs ----

def net_cfg(channels, kernels, strides, activation="relu"):
    """channels: WITH the input channel count in front (2 for an FXencoder)."""
    slope = {"relu": 0.0, "lrelu": float(torch.tensor(0.01, dtype=torch.float32))}[activation]
    return {"channels": list(channels), "kernels": list(kernels), "strides": list(strides), "activation": activation, "slope": slope}


def nlc_eligible(cfg):
    """mst_enc.hip enc_nlc_eligible, restated: asserted against the trace by EncTracer.checked_kernels (a bf16 run of an eligible net launches no
    NCL kernel and the other way round)."""
    ch, k, s = cfg["channels"], cfg["kernels"], cfg["strides"]
    if ch[0] > 4 or ch[1] > 32 or ch[1] % 8 or k[0] > 64 or 255 * s[0] + (k[0] - 1) + 1 > 256 * 8 + 64:
        return False
    return all(c % 8 == 0 for c in ch[1:])


class EncTracer(PlanTracer):
    """Dry-runs mst_enc_forward_blocks / mst_enc_forward / mst_enc_forward_conv of a constant-weight handle on the emulator build.  The trace
    plumbing (emu_trace_begin / emu_trace_end, the text buffer, the dummy pointer, the handle cache) is tcn_block_ref.PlanTracer's, inherited
    as it stands; the handles, what is dry-run and the symbols kept are the encoder's."""

    def traced(self, call, what="dry run"):
        """[[symbol, gx, gy, gz, bx], ...] of every launch `call()` (which returns the library's status) makes."""
        self.begin()
        rc = call()
        n = self.end(self.text, len(self.text))
        self.emu.check(rc, what)
        assert n < len(self.text)
        return [ln.split() for ln in self.text.value.decode().splitlines() if ln.strip()]

    def _handle(self, cfg, valid=False):
        import numpy as np
        from music_mixing_style_transfer_amd import _lib
        key = (tuple(cfg["channels"]), tuple(cfg["kernels"]), tuple(cfg["strides"]), cfg["slope"], valid)
        if key in self.handles:
            return self.handles[key]
        emu, nb = self.emu, len(cfg["kernels"])
        d = _lib.MstEncDesc()
        d.nblocks, d.act_slope, d.valid_padding = nb, cfg["slope"], int(valid)
        d.channels[0] = cfg["channels"][0]
        for i in range(nb):
            d.channels[i + 1], d.kernels[i], d.strides[i], d.dilations[i] = cfg["channels"][i + 1], cfg["kernels"][i], cfg["strides"][i], 1
        h = C.c_void_p()
        emu.check(emu.mst_enc_create(C.byref(d), C.byref(h)), "create")
        for i in range(nb):
            for which, cout in enumerate((cfg["channels"][i], cfg["channels"][i + 1])):
                if valid and which == 0:
                    continue
                w = np.full((cout, cfg["channels"][i], cfg["kernels"][i]), 1e-3, np.float32)
                one, zero = np.ones(cout, np.float32), np.zeros(cout, np.float32)
                emu.check(emu.mst_enc_load_conv(h, i, which, w.ctypes.data, zero.ctypes.data, one.ctypes.data, zero.ctypes.data, zero.ctypes.data,
                                                one.ctypes.data, 1e-5, None), "load_conv")
        self.handles[key] = h
        return h

    def close(self):
        for h in self.handles.values():
            self.emu.mst_enc_destroy(h)
        self.handles = {}

    def launches(self, cfg, B, L, precision, schedule=1, rows_min_tiles=512, n_run=None):
        """Launches of one call, in order, as (symbol, grid z): forward (n_run None) or forward_blocks(n_run)."""
        emu, h = self.emu, self._handle(cfg)
        prec = PRECISION_ID[precision]
        emu.check(emu.mst_enc_set_schedule(h, schedule), "set_schedule")
        emu.check(emu.mst_enc_set_tuning(h, rows_min_tiles), "set_tuning")
        need = emu.mst_enc_workspace_bytes(h, B, L)
        if n_run is None:
            call = lambda: emu.mst_enc_forward(h, self.dummy, self.dummy, B, L, prec, self.dummy, need, None)
        else:
            call = lambda: emu.mst_enc_forward_blocks(h, self.dummy, self.dummy, B, L, prec, n_run, self.dummy, need, None)
        return [(f[0], int(f[3])) for f in self.traced(call) if KERNEL_SYMBOL.match(f[0])]

    def conv_launches(self, cfg, B, L):
        """mst_enc_forward_conv of a one-layer VALID handle (Conv1d_layer alone)."""
        emu, h = self.emu, self._handle(cfg, valid=True)
        return [f[0] for f in self.traced(lambda: emu.mst_enc_forward_conv(h, 0, 1, self.dummy, self.dummy, B, L, None)) if KERNEL_SYMBOL.match(f[0])]

    def checked_kernels(self, cfg, B, L, precision, schedule=1, rows_min_tiles=512):
        """What the per-block check of one case executes AND checks: per block n the launches forward_blocks(n + 1) adds to those of
        forward_blocks(n) (the probe's unpack kernel apart), the unpack kernel where there is one, and the forward's pool.
        Returns ({symbol}, [[symbols of block n]], [symbols of the forward], same: the forward runs the probe's launches and then the pool)."""
        nb = len(cfg["kernels"])
        seen, per_block, prev = set(), [], []
        for n in range(1, nb + 1):
            ls = [s for s, _ in self.launches(cfg, B, L, precision, schedule, rows_min_tiles, n)]
            if "enc_unpack_nlc_kernel" in ls[-1]:
                seen.add(ls[-1])
                ls = ls[:-1]
            assert ls[:len(prev)] == prev and len(ls) > len(prev), (ls, prev)
            per_block.append(ls[len(prev):])
            seen.update(ls[len(prev):])
            prev = ls
        fwd = [s for s, _ in self.launches(cfg, B, L, precision, schedule, rows_min_tiles, None)]
        assert "avgpool" in fwd[-1], fwd
        seen.add(fwd[-1])
        ncl = any("enc_conv_bf16_kernel" in s or "enc_conv_kernel" in s for s in prev)
        assert ncl == (block_mode(precision, nlc_eligible(cfg), 1) in ("fp32", "ncl16")), (prev, precision)
        return seen, per_block, fwd, fwd[:-1] == prev


def kernel_name(sym):
    """'enc_conv_nlc_kernel<4, true>' of a mangled symbol: tcn_block_ref.demangle_hint without the argument list; the bare kernel name where
    c++filt does not know a type (__bf16 arguments)."""
    out = demangle_hint(sym)
    if out.startswith("_Z"):
        return KERNEL_SYMBOL.match(sym).group(1)
    return re.sub(r"\(.*\)$", "", out)


def exported_enc_kernels(lib_path):
    import subprocess
    nm = subprocess.run(["nm", "-D", "--defined-only", lib_path], check=True, capture_output=True, text=True).stdout
    return {f[2] for f in (ln.split() for ln in nm.splitlines()) if len(f) == 3 and f[1] in "TW" and KERNEL_SYMBOL.match(f[2])}


def launched_in_sources():
    """The distinct encoder kernel instantiations csrc/mst_enc.hip launches: 'enc_conv_kernel<1>', 'enc_avgpool_kernel', ..."""
    src = open(os.path.join(REPO, "music_mixing_style_transfer_amd", "csrc", "mst_enc.hip")).read()
    return set(re.findall(r"MST_LAUNCH\(\(?((?:enc_\w+_kernel|embedding_mean_kernel)(?:<[^>]*>)?)", src))


# ---- one case ----

class Stack:
    """Res_ConvBlocks on one encoder handle with FXencoder's probe interface, for the stacks FXencoder does not build (it always puts a stereo
    input in front): block 0 with 4 input channels is the only way to enc_direct_kernel<false, 4>."""

    def __init__(self, cfg):
        from music_mixing_style_transfer_amd.networks.architectures import _EncoderRunner
        from music_mixing_style_transfer_amd.networks.network_utils import Res_ConvBlock
        ch = cfg["channels"]
        self.encoder = torch.nn.Sequential(*[Res_ConvBlock(1, ch[i], ch[i + 1], cfg["kernels"][i], stride=cfg["strides"][i], padding="SAME",
                                                           dilation=1, norm="batch", activation=cfg["activation"],
                                                           last_activation=cfg["activation"]) for i in range(len(cfg["kernels"]))])
        self.encoder.eval()
        self._runner = _EncoderRunner(list(self.encoder))
        self.precision = "fp32"

    def load_state_dict(self, sd):
        self.encoder.load_state_dict({k[len("encoder."):]: v for k, v in sd.items()})

    def to(self, dev):
        self.encoder.to(dev)
        return self

    def _get_runner(self):
        return self._runner

    def forward_blocks(self, x, n):
        return self._runner.run(x, pooled=False, n_run=n, precision=self.precision)

    def __call__(self, x):
        return self._runner.run(x, pooled=True, precision=self.precision)


def make_model(cfg, seed):
    """(model, state dict) of the net; an FXencoder where it can build it."""
    from music_mixing_style_transfer_amd.networks import FXencoder
    from music_mixing_style_transfer_amd.utils import synth
    sd = synth.fxencoder_state_dict({"channels": list(cfg["channels"]), "kernels": cfg["kernels"]}, seed=seed)
    if cfg["channels"][0] == 2:
        m = FXencoder({"channels": list(cfg["channels"][1:]), "kernels": list(cfg["kernels"]), "strides": list(cfg["strides"]),
                       "dilation": [1] * len(cfg["kernels"]), "bias": True, "norm": "batch", "conv_block": "res", "activation": cfg["activation"]})
    else:
        m = Stack(cfg)
    m.load_state_dict(sd)
    return m, sd


def make_enc_input(B, C0, L, seed):
    """tcn_block_ref.make_input's waveform (item 0 digital silence, last item full scale, synthetic audio between) for C0 input channels."""
    if C0 == 2:
        return make_input(B, L, seed)
    return torch.cat([make_input(B, L, seed + c) for c in range((C0 + 1) // 2)], dim=1)[:, :C0].contiguous()


def set_flags(model, lib, schedule, rows_min_tiles):
    run = model._get_runner()
    run._ensure(lib)
    lib.check(lib.mst_enc_set_schedule(run.handle, schedule), "schedule")
    lib.check(lib.mst_enc_set_tuning(run.handle, rows_min_tiles), "tuning")


def teeth_unit(info, y, big):
    """The irreducible parts of the primary bound relative to |y|, over the non-tiny elements `big`: one rounding at the mode's working
    precision - the output's own (u_out), or in 'ncl16' mode, whose fp32 store hides it, the bf16 rounding of the operands (UBF) - and the
    terms the check is defined with, accumulation and (where it is dense) fold: (c_acc(K) + 2 FOLD_ULPS) U32 median(S / |y|)."""
    u = UBF if info["mode"] == "ncl16" else info["u_out"]
    c = c_acc(info["K"][1]) + (2.0 * FOLD_ULPS if info["mode"] in ("fp32", "stereo", "nlc3") else 0.0)
    return u + c * U32 * float((info["S"][big] / y[big].abs()).median())


def check_model(model, sd, cfg, x, precision, names=None, fwd_same=True, s_dtype=torch.float64, ref_device=None, log=print, label="", blocks=None):
    """Every block of `model`, the pool alone on the probe's bits and the embedding, element by element.  names[n]: the kernel symbols of
    block n (report only).  Returns ({(kernel, precision): (max err / bound, max err / rigorous bound)}, [info per block]); raises
    AssertionError naming the worst elements on a miss."""
    model.precision = precision
    dev = ref_device or x.device
    nb = len(cfg["kernels"])
    nlc = nlc_eligible(cfg)
    ratios, failures, infos = {}, [], []
    a_prev = x
    a = None
    for n in range(nb):
        a = model.forward_blocks(x, n + 1)
        if blocks is not None and n not in blocks:
            a_prev = a
            continue
        y, b1, b2, info = block_ref(sd, cfg, n, a_prev.to(dev), precision, nlc, s_dtype=s_dtype)
        assert a.shape == y.shape, (a.shape, y.shape)
        err = (a.to(dev, torch.float64) - y).abs()
        r1, r2 = float((err / b1).max()), float((err / b2).max())
        kname = " + ".join(dict.fromkeys(kernel_name(s) for s in names[n])) if names else f"block {n}"
        what = f"{label} {precision} block {n} {kname}"
        ratios[(kname, precision)] = max(ratios.get((kname, precision), (0.0, 0.0)), (r1, r2))
        big = y.abs() > 1e-3 * float(y.abs().max().clamp_min(1e-30))
        med = float((b1[big] / y[big].abs()).median()) if bool(big.any()) else float("nan")
        info.update(n=n, median=med, r1=r1, r2=r2, kname=kname)
        teeth = med / teeth_unit(info, y, big) if bool(big.any()) else float("nan")
        info["teeth"] = teeth
        del info["S"]
        info.pop("in_unit", None)
        infos.append(info)
        log(f"{what}: max err/bound {r1:.3f}, max err/rigorous bound {r2:.4f}, median bound/|y| {med:.2e} = {teeth:.2f} x (u + (c_acc + fold) U32 median S/|y|), "
            f"flip share {info.get('flip_share', 0.0):.4f} (expected {info.get('flip_expected', 0.0):.4f})")
        if not (r1 <= 1.0 and r2 <= 1.0) or not bool(torch.isfinite(err).all()):
            failures.append(worst_report(err, b1 if r1 > 1.0 else b2, cfg["strides"][n], what + (": PRIMARY bound" if r1 > 1.0 else ": RIGOROUS bound")))
        del err, y, b1, b2
        a_prev = a
    # the pool alone on the probe's own activation; the forward runs the probe's launches, so its last activation has the probe's bits
    emb = model(x)
    pname = kernel_name(names[nb][0]) if names and len(names) > nb else "pool"
    if fwd_same:
        m, p1, p2 = mean_ref(a.to(dev), 2)
        err = (emb.to(dev, torch.float64) - m).abs()
        r1, r2 = float((err / p1).max()), float((err / p2).max())
        ratios[(pname, precision)] = (r1, r2)
        log(f"{label} {precision} {pname} alone on the probe's activation: max err/bound {r1:.3f}, max err/rigorous bound {r2:.4f}")
        if not (r1 <= 1.0 and r2 <= 1.0) or not bool(torch.isfinite(err).all()):
            failures.append(worst_report(err[:, :, None], (p1 if r1 > 1.0 else p2)[:, :, None], 1, f"{label} {precision} {pname}"))
    assert not failures, "\n".join(failures)
    return ratios, infos
