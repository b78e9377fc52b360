"""TEST INFRASTRUCTURE: the time-parallel FX passes (csrc/fx_kernels.h fx_biquad_* / fx_comp_*) one by one against an operand-exact
np.longdouble reference, element by element, each value with a bound computed beside it ("FX passes").

Plain numpy, vectorised over sequences (and chunks), the Python loop over time only.  Operands are exactly what the kernels multiply: inputs
float64(float32(x * float32(in_scale))), coefficients the five a0-normalised float64 values per band (mst_fx.hip biquad_coefs).  The float64
intermediates of a call (chunk end / start states; chunk maps, chunk start values, carry, tile sums) are read from the caller's scratch buffer
through the layouts mst_fx_biquad_plan / mst_fx_compressor_plan report.

Shared by tests/test_fx_pass_emu.py (CPU emulator) and tests/test_fx_pass_gpu.py (MI355X): `Runner` hides which of the two a case runs on."""
import ctypes as C
import functools
import os

import numpy as np
import torch

from music_mixing_style_transfer_amd import _lib

LD = np.longdouble
U = 2.0 ** -53
LN10_20 = 0.11512925464970228420
SLOTS = 64
MAXB = 8
COMP_T = 32
NEVER = 1e300
TINY = 2.0 ** -960          # a decayed state far below anything audible may underflow: the relative bounds get this floor
HERE = os.path.dirname(os.path.abspath(__file__))

# Constants of the bounds: four times the worst ratio (float64 restatement of the pass - no fma, one association order - against the
# longdouble reference, over the whole CPU case list, tests/test_fx_pass_emu.py::test_constants_cover_the_float64_restatement), rounded up to a
# power of two, at least 1.  Never from a kernel's own error.  DESIGN.md section 5 lists the measured ratios.
C_TAB = 4.0        # equaliser: the host's impulse-state table against the true impulse states (worst restatement ratio 0.51)
C_POW = 1.0        # the host's powers (A^M)^(2^l) against the true powers (0.064)
C_ENDS = 1.0       # zero-state end states against the longdouble sum on the table in use (0.10)
C_STARTS = 1.0     # chunk start states against the longdouble scan on the powers in use (0.082)
C_V = 8.0          # the output before its float32 rounding (1.51: numpy rounds every product and every sum, the kernels' fma once)
C_XL = 2.0         # compressor: level differences (0.35)
C_MAP = 2.0        # chunk records b_0, lb (0.33)
C_YL = 8.0         # the smoother: chunk start values, carry, y_l (1.92); FX_COMP_C_START of mst_fx.hip is this value (the dispatch limit follows from it)


def assert_longdouble():
    assert np.finfo(LD).eps <= 2.0 ** -63, "np.longdouble is not an extended type here: the reference would be no better than the kernels"


@functools.lru_cache(maxsize=None)
def coef_sets():
    g = np.load(os.path.join(HERE, "golden", "fx_pass_coefs.npz"))
    return {k: g[k] for k in g.files}


def norm_coefs(coef6):
    """[nb][6] (b0 b1 b2 a0 a1 a2) -> [nb][5] (b0 b1 b2 a1 a2) / a0, float64: mst_fx.hip biquad_coefs"""
    c = np.asarray(coef6, dtype=np.float64)
    a0 = c[:, 3]
    return np.stack([c[:, 0] / a0, c[:, 1] / a0, c[:, 2] / a0, c[:, 4] / a0, c[:, 5] / a0], 1)


def operands(x, in_scale):
    """x float32 [n, L, C], in_scale float64 [n] or None -> the float32 values the kernels convert, [n * C, L] float64 (sequence = item * C + c)"""
    x = np.asarray(x, dtype=np.float32)
    if in_scale is not None:
        x = x * np.asarray(in_scale, dtype=np.float64).astype(np.float32)[:, None, None]
    n, L, Cn = x.shape
    return np.ascontiguousarray(x.transpose(0, 2, 1).reshape(n * Cn, L)).astype(np.float64)


# =========================================================================================================== equaliser
def cascade_step(v, z, cf, local=None):
    """One sample through every band (transposed direct form II, fx_biquad_band): v [...], z [..., 2 nb] updated in place; returns the output.
    local = (Lz, u): also the first-order bound of the rounding THIS step adds, given exact incoming state and input - Lz [..., 2 nb] for
    the new state, returned second for the output (each operation rounds by u * sum of |operand products|, carried through the later bands
    of the same step by |coefficients|)."""
    dv = None
    if local is not None:
        Lz, u = local
        dv = np.zeros(v.shape, dtype=np.float64)
    for b in range(cf.shape[0]):
        b0, b1, b2, a1, a2 = cf[b]
        z1, z2 = z[..., 2 * b], z[..., 2 * b + 1]
        y = b0 * v + z1
        p1 = b1 * v + z2
        p2 = b2 * v
        if local is not None:
            av, ay = np.abs(v).astype(np.float64), np.abs(y).astype(np.float64)
            fb0, fb1, fb2, fa1, fa2 = (abs(float(t)) for t in (b0, b1, b2, a1, a2))
            dy = fb0 * dv + u * (fb0 * av + np.abs(z1).astype(np.float64))
            dp1 = fb1 * dv + u * (fb1 * av + np.abs(z2).astype(np.float64))
            dp2 = fb2 * dv + u * fb2 * av
            Lz[..., 2 * b] = fa1 * dy + dp1 + u * (fa1 * ay + np.abs(p1).astype(np.float64))
            Lz[..., 2 * b + 1] = fa2 * dy + dp2 + u * (fa2 * ay + np.abs(p2).astype(np.float64))
            dv = dy
        z[..., 2 * b] = p1 - a1 * y
        z[..., 2 * b + 1] = p2 - a2 * y
        v = y
    return (v, dv) if local is not None else v


def system_matrices(cf, M, dtype=LD):
    """A^d for d = 0 .. M ([M + 1][S][S], A^d[:, c] = the state d steps after unit state c, zero input) and the output row (v = crow . s + d x)"""
    S = 2 * cf.shape[0]
    cfd = cf.astype(dtype)
    z = np.eye(S, dtype=dtype)             # row c = the run started from unit state c
    out = np.zeros((M + 1, S, S), dtype=dtype)
    out[0] = np.eye(S, dtype=dtype)
    crow = None
    for d in range(1, M + 1):
        v = cascade_step(np.zeros(S, dtype=dtype), z, cfd)
        if d == 1:
            crow = v.copy()
        out[d] = z.T
    return out, crow


def impulse_table(cf, M, dtype=LD, track=False):
    """h_m, m = 0 .. M - 1: the state m steps after a unit impulse went in ([M][S]); track: also the local rounding bound of every step (float64)"""
    S = 2 * cf.shape[0]
    cfd = cf.astype(dtype)
    z = np.zeros(S, dtype=dtype)
    tab = np.zeros((M, S), dtype=dtype)
    loc = np.zeros((M, S))
    for m in range(M):
        v = np.asarray(1.0 if m == 0 else 0.0, dtype=dtype)
        if track:
            Lz = np.zeros(S)
            cascade_step(v, z, cfd, (Lz, U))
            loc[m] = Lz
        else:
            cascade_step(v, z, cfd)
        tab[m] = z
    return (tab, loc) if track else tab


def run_chunks(X, starts, cf, dtype, track=False):
    """X [..., M] operands, starts [..., S] -> (v [..., M], end states [..., S]); track: and (Lstate [..., M, S], Lv [..., M])"""
    M, S = X.shape[-1], 2 * cf.shape[0]
    cfd = cf.astype(dtype)
    z = starts.astype(dtype).copy()
    v = np.zeros(X.shape, dtype=dtype)
    Ls = np.zeros(X.shape + (S,)) if track else None
    Lv = np.zeros(X.shape) if track else None
    Xd = X.astype(dtype)
    for t in range(M):
        if track:
            Lz = np.zeros(X.shape[:-1] + (S,))
            v[..., t], Lv[..., t] = cascade_step(Xd[..., t], z, cfd, (Lz, U))
            Ls[..., t, :] = Lz
        else:
            v[..., t] = cascade_step(Xd[..., t], z, cfd)
    return (v, z, Ls, Lv) if track else (v, z)


def matvec(Mx, v):
    """[S][S] x [..., S] -> [..., S]"""
    return np.einsum("rc,...c->...r", Mx, v)


class EqRef:
    """Reference values and bounds of one equaliser call: x64 [n_seq, L] operands, cf [nb][5], chunk length M (from the plan query)."""

    def __init__(self, x64, cf, M):
        assert_longdouble()
        self.x64, self.cf, self.M = x64, cf, M
        n_seq, L = x64.shape
        self.n_seq, self.L, self.S = n_seq, L, 2 * cf.shape[0]
        self.nchunks, self.nfull = (L + M - 1) // M, L // M
        S, nchunks, nfull = self.S, self.nchunks, self.nfull
        self.Apow, self.crow = system_matrices(cf, M)
        self.absA = np.abs(self.Apow).astype(np.float64)
        self.h, h_loc = impulse_table(cf, M, track=True)                              # true impulse states, local bounds of the float64 recursion
        self.bound_h = np.zeros((M, S))                                               # of the float64 table: every local error carried by |A^d|
        for m in range(M):
            for d in range(m + 1):
                self.bound_h[m] += self.absA[d] @ h_loc[m - d]
        Xp = np.zeros((n_seq, nchunks * M))
        Xp[:, :L] = x64
        self.Xp = Xp.reshape(n_seq, nchunks, M)
        # zero-state end state of every full chunk
        _, e = run_chunks(self.Xp[:, :nfull], np.zeros((n_seq, nfull, S)), cf, LD)
        self.ends = e
        # serial state at every chunk boundary: s_(k+1) = A^M s_k + e_k
        P = self.Apow[M]
        st = np.zeros((n_seq, nchunks, S), dtype=LD)
        for k in range(1, nchunks):
            st[:, k] = matvec(P, st[:, k - 1]) + e[:, k - 1]
        self.starts = st
        # every chunk from its true start state: the output before its float32 rounding, and the rounding each step adds
        v, _, self.Ls, self.Lv = run_chunks(self.Xp, st, cf, LD, track=True)
        self.v = v.reshape(n_seq, nchunks * M)[:, :L]

    def serial(self):
        """The same output by one serial longdouble run over the whole signal (checks the two-pass reference itself)"""
        v, _ = run_chunks(self.x64, np.zeros((self.n_seq, self.S)), self.cf, LD)
        return v

    def power_bounds(self, P0, nlev, absQ):
        """|error| of the float64 powers the scan multiplies by, level l = P^(2^l): A^M by the float64 recursion (D0), squared up level by
        level (rounding R_j of squaring number j).  An error E in P^(2^j) sits in P^(2^l) as sum_k (P^(2^j))^k E (P^(2^j))^(2^(l-j) - 1 - k):
        bounded with |.| of the TRUE powers it travels through (absQ[n] = |P^n|), not with powers of |P|."""
        M, S = self.M, self.S
        z = np.eye(S)
        hist = []
        for d in range(M):
            Lz = np.zeros((S, S))
            cascade_step(np.zeros(S), z, self.cf, (Lz, U))
            hist.append(Lz)                                                            # [start state c][state]
        d0 = np.zeros((S, S))
        for d in range(M):
            d0 += self.absA[M - 1 - d] @ hist[d].T                                     # column c of the error matrix
        src, cur, out = [d0], P0, [d0]
        for l in range(1, nlev):
            if (1 << l) >= absQ.shape[0]:
                break
            a = np.abs(cur)
            src.append(S * U * (a @ a))                                                # rounding of squaring number l
            cur = cur @ cur
            tot = np.zeros((S, S))
            for j, e in enumerate(src):
                w, cnt = 1 << j, 1 << (l - j)
                for k in range(cnt):
                    tot += absQ[k * w] @ e @ absQ[(cnt - 1 - k) * w]
            out.append(tot)
        return out

    def true_powers(self, nq):
        """P^n, P = A^M, n = 0 .. nq - 1 (longdouble)"""
        Q = np.zeros((nq, self.S, self.S), dtype=LD)
        Q[0] = np.eye(self.S, dtype=LD)
        for n in range(1, nq):
            Q[n] = self.Apow[self.M] @ Q[n - 1]
        return Q

    def scan(self, ends, pw, nb_threads, bound_in=None, dtype=np.float64):
        """fx_biquad_scan_kernel restated: blocks of nb_threads - 1 chunks, element 0 the carry, Hillis-Steele levels with the powers pw[l]
        the call multiplies by; dtype longdouble: the same network on the same tables without the float64 rounding.  bound_in [n_seq, nchunks,
        S] (the rounding bound of `ends`): also returns the rounding bound of the start states - every input error and every level's rounding
        carried to the elements it reaches by |P^n| of the TRUE power it travels through."""
        n_seq, nchunks, S, M = self.n_seq, self.nchunks, self.S, self.M
        nlev = 9 if nb_threads == 512 else 8
        pw = [np.asarray(pw[l]).astype(dtype) for l in range(nlev)]
        starts = np.zeros((n_seq, nchunks, S), dtype=dtype)
        bound = np.zeros((n_seq, nchunks, S)) if bound_in is not None else None
        if bound_in is not None:
            absQ = np.abs(self.true_powers(min(nb_threads, nchunks + 1))).astype(np.float64)
        carry = np.zeros((n_seq, S), dtype=dtype)
        bcarry = np.zeros((n_seq, S))
        for k0 in range(0, nchunks, nb_threads - 1):
            nel = min(nb_threads, nchunks - k0 + 1)                                    # elements that matter: carry + the chunks before each start
            t = np.zeros((n_seq, nel, S), dtype=dtype)
            t[:, 0] = carry
            t[:, 1:] = ends[:, k0:k0 + nel - 1]
            if bound_in is not None:
                b = np.zeros((n_seq, nel, S))
                b[:, 0] = bcarry
                b[:, 1:] = bound_in[:, k0:k0 + nel - 1]
                fin = np.zeros((n_seq, nel, S))
                for n in range(nel):
                    fin[:, n:] += matvec(absQ[n], b[:, :nel - n])
            for l in range(nlev):
                d = 1 << l
                if d >= nel:
                    break
                add = matvec(pw[l], t[:, :nel - d])
                if bound_in is not None:
                    loc = (S + 1) * U * (np.abs(t[:, d:]) + matvec(np.abs(pw[l]), np.abs(t[:, :nel - d])))
                    step = 2 * d                                                        # reaches i + m * 2^(l+1) through the later levels
                    for m in range(0, (nel - d + step - 1) // step + 1):
                        sft = m * step
                        if d + sft >= nel:
                            break
                        fin[:, d + sft:] += matvec(absQ[sft], loc[:, :nel - d - sft]) if sft else loc
                t = t.copy()
                t[:, d:] += add
            take = min(nb_threads - 1, nchunks - k0)
            starts[:, k0:k0 + take] = t[:, :take]
            if bound_in is not None:
                bound[:, k0:k0 + take] = fin[:, :take]
            if nel == nb_threads:
                carry = t[:, nb_threads - 1]
                if bound_in is not None:
                    bcarry = fin[:, nb_threads - 1]
        return (starts, bound) if bound_in is not None else starts

    def restated_tables(self):
        """the host's tables restated in numpy float64 (no fma): impulse states by recursion, A^M by recursion, squared up level by level"""
        tab = impulse_table(self.cf, self.M, np.float64)
        pw = [system_matrices(self.cf, self.M, np.float64)[0][self.M]]
        for _ in range(1, 9):
            pw.append(pw[-1] @ pw[-1])
        return tab, np.stack(pw)

    def table_bounds(self, pw):
        """(bound of the float64 impulse table, bounds of the float64 powers): the tables are intermediates of their own"""
        nlev = pw.shape[0]
        absQ = np.abs(self.true_powers((1 << (nlev - 1)) + 1)).astype(np.float64)
        return self.bound_h, self.power_bounds(pw[0], nlev, absQ)

    def bounds(self, nb_threads, tab=None, pw=None):
        """Everything the checks of one call need, for the float64 tables the checked code multiplies by (tab [M][S], pw [9][S][S]: the
        library's own, mst_fx_biquad_tables; default: the numpy restatement's) and the scan block size it takes.  The tables are checked
        against longdouble as intermediates of their own; what they are is then KNOWN, so the passes behind them are held to the longdouble
        evaluation of the same sums on those tables (ends_exp, starts_exp) within the rounding of the float64 arithmetic alone (be_r, bs_r),
        and the distance of that evaluation from the true values is a known number, not a bound.
        Returns a dict: ends64 / starts64 (the numpy float64 restatement), ends_exp / starts_exp, be_r / bs_r, be / bs (against the TRUE end /
        start states: known table effect + rounding, constants applied), bv [n_seq, L] (bound of the output before its float32 rounding)."""
        cf, M, S = self.cf, self.M, self.S
        if tab is None:
            tab, pw = self.restated_tables()
        nf = self.nfull
        ends64 = np.zeros((self.n_seq, self.nchunks, S))
        ends_exp = np.zeros((self.n_seq, self.nchunks, S), dtype=LD)
        tl = tab.astype(LD)
        for n in range(M):                                                             # dot product in time order
            ends64[:, :nf] += tab[M - 1 - n] * self.Xp[:, :nf, n, None]
            ends_exp[:, :nf] += tl[M - 1 - n] * self.Xp[:, :nf, n, None].astype(LD)
        be_r = np.zeros((self.n_seq, self.nchunks, S))
        be_r[:, :nf] = np.einsum("skn,nj->skj", np.abs(self.Xp[:, :nf, ::-1]), M * U * np.abs(tab))      # M terms in any association order
        starts64, bs_r = self.scan(ends64, pw, nb_threads, C_ENDS * be_r)
        starts_exp = self.scan(ends_exp, pw, nb_threads, dtype=LD)
        f = lambda a: np.abs(a).astype(np.float64)
        be = f(ends_exp[:, :nf] - self.ends) + C_ENDS * be_r[:, :nf]
        bs = f(starts_exp - self.starts) + C_STARTS * bs_r
        # inside a chunk: the start state's bound and every step's rounding, carried by |A^d|
        sb = np.zeros((self.n_seq, self.nchunks, M, S))                                # bound of the state BEFORE step t
        for t in range(M):
            sb[:, :, t] = matvec(self.absA[t], bs)
        for d in range(M - 1):
            sb[:, :, d + 1:] += matvec(self.absA[d], self.Ls[:, :, :M - 1 - d])
        bv = np.einsum("c,skmc->skm", np.abs(self.crow).astype(np.float64), sb) + self.Lv
        return dict(ends64=ends64, starts64=starts64, ends_exp=ends_exp[:, :nf], starts_exp=starts_exp, be_r=be_r[:, :nf], bs_r=bs_r, be=be, bs=bs,
                    bv=bv.reshape(self.n_seq, self.nchunks * M)[:, :self.L])


# =========================================================================================================== running a call
class Runner:
    """One binding (the emulator's or the product's) and the device its tensors live on."""

    def __init__(self, lib, device):
        self.lib, self.device = lib, torch.device(device)

    def t(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def eq_plan(self, n, L, Cn, nb):
        p = _lib.MstFxBiquadPlan()
        self.lib.check(self.lib.mst_fx_biquad_plan(n, L, Cn, nb, C.byref(p)), "mst_fx_biquad_plan")
        return p

    def eq_tables(self, coef6, M):
        """the library's own float64 tables for this coefficient set and chunk length: (impulse states [M][S], powers [9][S][S])"""
        coef = np.ascontiguousarray(coef6, dtype=np.float64)
        S = 2 * coef.shape[0]
        tab, pw = np.zeros((M, S)), np.zeros((9, S, S))
        dp = C.POINTER(C.c_double)
        self.lib.check(self.lib.mst_fx_biquad_tables(coef.ctypes.data_as(dp), coef.shape[0], M, tab.ctypes.data_as(dp), pw.ctypes.data_as(dp)), "mst_fx_biquad_tables")
        return tab, pw

    def comp_plan(self, n, L, Cn, attack, release, sr=44100.0, forms=0):
        p = _lib.MstFxCompressorPlan()
        self.lib.check(self.lib.mst_fx_compressor_plan(n, L, Cn, float(attack), float(release), float(sr), forms, C.byref(p)), "mst_fx_compressor_plan")
        return p

    def equaliser(self, x, coef6, in_scale=None, sumsq=False, in_sumsq=False, forms=0, scratch=True, poison=None):
        """x float32 [n, L, C] -> dict(y, ends, starts, sumsq, in_sumsq, plan): numpy; ends / starts [n_seq, nchunks, 16] as the call left them"""
        lib = self.lib
        n, L, Cn = x.shape
        coef = np.ascontiguousarray(coef6, dtype=np.float64)
        nb = coef.shape[0]
        plan = self.eq_plan(n, L, Cn, nb)
        xt = self.t(x.astype(np.float32))
        yt = torch.empty_like(xt)
        nbytes = lib.mst_fx_biquad_scratch_bytes(n, L, Cn, nb)
        sc = torch.full(((nbytes + 7) // 8,), float("nan"), dtype=torch.float64, device=self.device) if scratch else None
        st = self.t(np.asarray(in_scale, dtype=np.float64)) if in_scale is not None else None
        fill = float("nan") if poison is None else poison                              # the call clears its energy slots itself
        qs = torch.full((n * SLOTS,), fill, dtype=torch.float64, device=self.device) if sumsq else None
        qi = torch.full((n * SLOTS,), fill, dtype=torch.float64, device=self.device) if in_sumsq else None
        fuse = None
        if st is not None or sumsq or in_sumsq or forms:
            f = _lib.MstFxFuse(st.data_ptr() if st is not None else None, qs.data_ptr() if sumsq else None, None, 0, 1.0,
                               qi.data_ptr() if in_sumsq else None, forms=forms)
            fuse = C.byref(f)
        with lib.device_ctx(xt):
            rc = lib.mst_fx_biquad_cascade(xt.data_ptr(), yt.data_ptr(), n, L, Cn, coef.ctypes.data_as(C.POINTER(C.c_double)), nb,
                                           sc.data_ptr() if scratch else None, nbytes if scratch else 0, fuse, lib.stream_ptr(xt))
        lib.check(rc, "mst_fx_biquad_cascade")
        out = {"plan": plan, "y": yt.cpu().numpy(), "sumsq": qs.cpu().numpy().reshape(n, SLOTS) if sumsq else None,
               "in_sumsq": qi.cpu().numpy().reshape(n, SLOTS) if in_sumsq else None}
        if scratch and plan.time_parallel:
            s = sc.cpu().numpy()
            cnt = n * Cn * plan.nchunks * plan.record_doubles
            shape = (n * Cn, plan.nchunks, plan.record_doubles)
            out["ends"] = s[plan.ends_offset // 8:plan.ends_offset // 8 + cnt].reshape(shape)
            out["starts"] = s[plan.starts_offset // 8:plan.starts_offset // 8 + cnt].reshape(shape)
        return out


def seq_to_audio(a, n, Cn):
    """[n * C, L] -> [n, L, C]"""
    return a.reshape(n, Cn, -1).transpose(0, 2, 1)


def worst_ratio(err, bound):
    """max err / bound over all elements (0 / 0 = 0; anything / 0 = inf)"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


def f32_bound(v, bv):
    return 2.0 ** -24 * np.abs(v) * (1 + 2.0 ** -20) + bv + 2.0 ** -149


@functools.lru_cache(maxsize=None)
def eq_reference(key):
    """key = (coef name, L, n, C, in_scale tuple or None, seed, M) -> (x, EqRef): built once per case and shared"""
    name, L, n, Cn, scale, seed, M = key
    x = eq_input(L, n, Cn, seed)
    return x, EqRef(operands(x, None if scale is None else np.asarray(scale)), norm_coefs(coef_sets()[name]), M)


def eq_input(L, n, Cn, seed):
    """white noise at 0.2 with a quiet stretch (x 1e-3), a run of exact zeros and a full-scale sample"""
    rng = np.random.default_rng(seed)
    x = (0.2 * rng.standard_normal((n, L, Cn))).astype(np.float32)
    q = max(1, L // 5)
    x[:, q:2 * q] *= np.float32(1e-3)
    x[:, 3 * q:3 * q + max(1, q // 3)] = 0.0
    x[0, L - 1] = 1.0
    return x


def check_equaliser(run, name, L, n, Cn, scale=None, seed=0, forms=0, sumsq=False, in_sumsq=False, expect=None, log=print, conditions=True):
    """One equaliser call, every intermediate and every output sample against the reference.  expect: dict of plan fields the case is there
    to reach (asserted).  Returns {quantity: max err / bound}."""
    coef6 = coef_sets()[name]
    nb = coef6.shape[0]
    plan = run.eq_plan(n, L, Cn, nb)
    for k, v in (expect or {}).items():
        assert getattr(plan, k) == v, f"{name} {(L, n, Cn)}: plan.{k} = {getattr(plan, k)}, the case is there for {v}"
    x, ref = eq_reference((name, L, n, Cn, None if scale is None else tuple(scale), seed, plan.M))
    got = run.equaliser(x, coef6, in_scale=scale, sumsq=sumsq, in_sumsq=in_sumsq, forms=forms)
    if sumsq or in_sumsq:                                                              # a second call clears the slots of the first
        got = run.equaliser(x, coef6, in_scale=scale, sumsq=sumsq, in_sumsq=in_sumsq, forms=forms, poison=1e30)
    out, S = {}, ref.S
    what = f"eq {name} L={L} n={n} C={Cn} forms={forms}"
    if plan.time_parallel:
        assert plan.nchunks == ref.nchunks
        tab, pw = run.eq_tables(coef6, plan.M)
        bh, bp = ref.table_bounds(pw)                                                  # the host's tables first: intermediates of their own
        out["table"] = worst_ratio(np.abs(tab - ref.h).astype(np.float64), C_TAB * bh + TINY)
        out["powers"] = max(worst_ratio(np.abs(pw[l] - ref.true_powers((1 << l) + 1)[1 << l]).astype(np.float64), C_POW * bp[l] + TINY) for l in range(len(bp)))
        B = ref.bounds(plan.scan_threads, tab, pw)
        bv = B["bv"]
        ends, starts = got["ends"][:, :, :S], got["starts"][:, :, :S]
        out["ends"] = worst_ratio(np.abs(ends[:, :ref.nfull] - B["ends_exp"]).astype(np.float64), C_ENDS * B["be_r"] + TINY)
        if ref.nfull < ref.nchunks:
            assert np.all(ends[:, ref.nfull:] == 0.0), what + ": the short last chunk's record is zeros"
        out["starts"] = worst_ratio(np.abs(starts - B["starts_exp"]).astype(np.float64), C_STARTS * B["bs_r"] + TINY)
        out["ends true"] = worst_ratio(np.abs(ends[:, :ref.nfull] - ref.ends).astype(np.float64), B["be"] + TINY)
        out["starts true"] = worst_ratio(np.abs(starts - ref.starts).astype(np.float64), B["bs"] + TINY)
        if conditions:
            eq_conditions(ref, B, what)
    else:
        bv = np.zeros((ref.n_seq, L))                                                  # one chunk from rest: only the steps' own rounding
        sb = np.zeros((ref.n_seq, 1, ref.M, S))
        for d in range(ref.M - 1):
            sb[:, :, d + 1:] += matvec(ref.absA[d], ref.Ls[:, :, :ref.M - 1 - d])
        bv = (np.einsum("c,skmc->skm", np.abs(ref.crow).astype(np.float64), sb) + ref.Lv).reshape(ref.n_seq, -1)[:, :L]
    y = operands(got["y"], None)
    out["y"] = worst_ratio(np.abs(y - ref.v).astype(np.float64), f32_bound(np.abs(ref.v).astype(np.float64), C_V * bv))
    if sumsq or in_sumsq:
        out.update(check_eq_energies(got, x, plan, n, Cn, sumsq, in_sumsq, what))
    log(f"{what} M={plan.M} nchunks={plan.nchunks} scan={plan.scan_threads}: " + ", ".join(f"{k} {v:.3f}" for k, v in out.items()))
    bad = {k: v for k, v in out.items() if not v <= 1.0}
    assert not bad, f"{what}: err / bound {bad}"
    return out, got


def eq_conditions(ref, B, what):
    """every checked float64 intermediate is resolved to 2^-30 of the largest value of its sequence: bound against the TRUE value (the known
    effect of the float64 tables + the rounding bound)"""
    for nm, b, val in (("ends", B["be"], ref.ends), ("starts", B["bs"], ref.starts)):
        if val.shape[1]:
            top = np.abs(val).astype(np.float64).max(axis=(1, 2), keepdims=True)
            assert np.all(b <= 2.0 ** -30 * top), f"{what}: the bound of {nm} is 2^{np.log2(float((b / top).max())):.1f} of its sequence's largest value, not below 2^-30"


def check_eq_energies(got, x, plan, n, Cn, sumsq, in_sumsq, what):
    """slot s of an item = its chunks s, s + 64, ... (all channels), float64 sums of the call's OWN float32 output (exact operands);
    out_in_sumsq: float32 squares of the raw input, float64 sums"""
    out = {}
    M, L = plan.M, x.shape[1]
    slot_of = (np.arange(L) // M) % SLOTS
    for nm, on, vals in (("sumsq", sumsq, got["y"].astype(np.float64) ** 2), ("in_sumsq", in_sumsq, (x * x).astype(np.float64))):
        if not on:
            continue
        want = np.zeros((n, SLOTS))
        terms = np.zeros((n, SLOTS))
        for s in range(SLOTS):
            sel = slot_of == s
            want[:, s] = vals[:, sel].sum((1, 2))
            terms[:, s] = sel.sum() * Cn
        assert np.all(got[nm][terms == 0] == 0.0), what + f": {nm} slots without a chunk are cleared"
        out[nm] = worst_ratio(np.abs(got[nm] - want), (terms + 1) * U * want)
    return out


# =========================================================================================================== compressor
def comp_alphas(attack_ms, release_ms, sr=44100.0):
    return float(np.exp(-1.0 / (0.001 * sr * attack_ms))), float(np.exp(-1.0 / (0.001 * sr * release_ms)))


def curve(ratio):
    """(mode, mul) per sequence as fx_comp_curve: 1 compressor (mul = 1 / ratio), 2 expander (mul = ratio), 0 ratio == 1"""
    ratio = np.asarray(ratio, dtype=np.float64)
    mode = np.where(ratio > 1.0, 1, np.where(ratio < 1.0, 2, 0))
    with np.errstate(divide="ignore"):
        mul = np.where(ratio > 1.0, 1.0 / ratio, ratio)
    return mode, mul


def level_diff(xs32, thr, ratio, dtype=LD, log10=None):
    """x_l = x_g - y_g per sample: xs32 float32 [n_seq, L], thr / ratio [n_seq].  The -120 dB floor is decided on the float32 |x| like the
    kernel does.  Returns (x_l, bound of a float64 evaluation)."""
    ax = np.abs(xs32.astype(np.float32))
    floor = ax.astype(np.float64) < 0.000001
    safe = np.where(floor, np.float32(1.0), ax)
    lg = np.log10(safe.astype(dtype)) if log10 is None else log10(safe)
    xg = np.where(floor, dtype(-120.0), dtype(20.0) * lg)
    mode, mul = curve(ratio)
    thr_c, mul_c, mode_c = np.asarray(thr, dtype=np.float64)[:, None].astype(dtype), mul[:, None].astype(dtype), mode[:, None]
    bent = thr_c + (xg - thr_c) * mul_c
    yg = np.where(mode_c == 1, np.where(xg >= thr_c, bent, xg), np.where(mode_c == 2, np.where(xg <= thr_c, bent, xg), dtype(0.0)))
    xl = xg - yg
    # float64 evaluation: the logarithm's terms (e log10 2 + table + polynomial) round by 4 u each at their own size, then the curve's fma
    expo = np.where(floor, 0.0, np.abs(np.floor(np.log2(safe.astype(np.float64)))))
    bxg = np.where(floor, 0.0, 20.0 * 4.0 * U * (0.30103 * expo + 1.0))
    f = lambda a: np.abs(a).astype(np.float64)
    bxl = bxg * (1.0 + mul[:, None]) + U * (2.0 * f(xg - thr_c) * mul[:, None] + f(thr_c) + f(yg) + f(xl))
    return xl, bxl


def log10_f32_restated(ax32):
    """fx_log10_f32 in numpy float64 (no fma): exponent, the 7-bit table, log1p of the remainder to r^7"""
    bits = ax32.astype(np.float32).view(np.uint32)
    e = (bits >> 23).astype(np.int64) - 127
    i = ((bits >> 16) & 127).astype(np.int64)
    m = ((bits & 0x007fffff) | 0x3f800000).astype(np.uint32).view(np.float32).astype(np.float64)
    mh = ((bits & 0x007f0000) | 0x3f800000).astype(np.uint32).view(np.float32).astype(np.float64)
    grid = 1.0 + np.arange(128) / 128.0
    r = (m - mh) * (1.0 / grid)[i]
    p = r * (1.0 / 7.0) - 1.0 / 6.0
    for cst in (1.0 / 5.0, -1.0 / 4.0, 1.0 / 3.0, -0.5):
        p = r * p + cst
    l1p = (r * r) * p + r
    return l1p * 0.43429448190325182765 + (e.astype(np.float64) * 0.30102999566398119521 + np.log10(grid)[i])


def smooth(xl, aA, aR, dtype=LD, y0=None):
    """the serial smoother y <- y + c (x - y), c = 1 - aA when x > y else 1 - aR, from 0: [n_seq, L]"""
    n_seq, L = xl.shape
    cA, cR = dtype(1.0) - dtype(aA), dtype(1.0) - dtype(aR)
    y = np.zeros(n_seq, dtype=dtype) if y0 is None else y0.astype(dtype)
    out = np.zeros((n_seq, L), dtype=dtype)
    xl = xl.astype(dtype)
    for n in range(L):
        d = xl[:, n] - y
        y = y + np.where(d > 0, cA, cR) * d
        out[:, n] = y
    return out


def chunk_records(xl, aA, aR, dtype=LD):
    """Per 32-step chunk: b_0 (intercept of the all-attack piece) and lb_1 .. lb_n, the sorted values f_(x_n) o ... o f_(x_(t+1)) (x_t), t = 1 .. n
    (n = steps of the chunk), NEVER beyond: [n_seq, nchunks, 34] as fx_comp_map_kernel stores them (last double a pad, not compared)"""
    n_seq, L = xl.shape
    T = COMP_T
    nch = (L + T - 1) // T
    X = np.zeros((n_seq, nch * T), dtype=dtype)
    X[:, :L] = xl
    X = X.reshape(n_seq, nch, T)
    steps = np.minimum(T, L - np.arange(nch) * T)                                      # [nch]
    cA, cR = dtype(1.0) - dtype(aA), dtype(1.0) - dtype(aR)
    vals = np.full((n_seq, nch, T), np.inf, dtype=dtype)
    b0 = np.zeros((n_seq, nch), dtype=dtype)
    with np.errstate(invalid="ignore"):                                                # the unused slots of a short chunk hold inf
        for t in range(T):
            on = (t < steps)[None, :]
            x = X[:, :, t]
            b0 = np.where(on, dtype(aA) * b0 + cA * x, b0)
            if t:
                cur = vals[:, :, :t]
                d = x[:, :, None] - cur
                vals[:, :, :t] = np.where(on[:, :, None], cur + np.where(d > 0, cA, cR) * d, cur)
            vals[:, :, t] = np.where(on, x, np.inf)
    vals = np.sort(vals, axis=2)
    rec = np.full((n_seq, nch, T + 2), NEVER, dtype=dtype)
    rec[:, :, 0] = b0
    rec[:, :, 1:T + 1] = np.where(np.isfinite(vals), vals, dtype(NEVER))
    return rec


def restate_map_and_walk(xl64, aA, aR):
    """The time-parallel smoother restated in numpy float64 (no fma): chunk maps by sorted insertion (fx_comp_map_kernel), the walk by piece
    lookup over rebuilt intercepts and crossing inputs (fx_comp_chain_kernel).  Returns (records [n_seq, nch, 34], ystart [nch, n_seq])."""
    n_seq, L = xl64.shape
    T = COMP_T
    nch = (L + T - 1) // T
    cA, cR = 1.0 - aA, 1.0 - aR
    pick = np.minimum if aA > aR else np.maximum
    rec = np.full((n_seq, nch, T + 2), NEVER)
    ystart = np.zeros((nch, n_seq))
    y = np.zeros(n_seq)
    for k in range(nch):
        n = min(T, L - k * T)
        lb = np.zeros((n_seq, T + 2))
        b0 = np.zeros(n_seq)
        for t in range(n):
            x = xl64[:, k * T + t]
            oA, oR = cA * x, cR * x
            b0 = aA * b0 + oA
            m = x.copy()
            for s in range(t + 1, 0, -1):
                if s > 1:
                    v = lb[:, s - 1]
                    g = pick(aA * v + oA, aR * v + oR)
                    lb[:, s] = np.maximum(g, m)
                    m = np.minimum(g, x)
                else:
                    lb[:, 1] = m
        rec[:, k, 0] = b0
        rec[:, k, 1:n + 1] = lb[:, 1:n + 1]
        slope = np.array([aA ** (n - p) * aR ** p for p in range(n + 1)])
        inv = 1.0 / slope
        d = np.zeros((n_seq, n + 1))
        d[:, 1] = (lb[:, 1] - b0) * inv[0]
        for p in range(2, n + 1):
            d[:, p] = (lb[:, p] - lb[:, p - 1]) * inv[p - 1]
        u = np.cumsum(d, axis=1)
        u[:, 0] = -NEVER
        bp = lb[:, :n + 1] - slope * u
        bp[:, 0] = b0
        ystart[k] = y
        idx = (u <= y[:, None]).sum(1) - 1                                             # the highest piece whose crossing input y has reached
        y = slope[idx] * y + bp[np.arange(n_seq), idx]
    return rec, ystart, y


class CompRef:
    """Reference values and bounds of one compressor call.  xs32 [n_seq, L]: the float32 operands (x * float32(in_scale)); thr / ratio per sequence."""

    def __init__(self, xs32, thr, ratio, aA, aR):
        assert_longdouble()
        self.n_seq, self.L = xs32.shape
        self.aA, self.aR = aA, aR
        self.xs = xs32.astype(np.float32)
        self.xl, self.bxl = level_diff(self.xs, thr, ratio)
        self.thr, self.ratio = thr, ratio
        self.yl = smooth(self.xl, aA, aR)
        T = COMP_T
        self.nchunks = (self.L + T - 1) // T
        idx = np.arange(1, self.nchunks) * T - 1
        self.ystart = np.zeros((self.nchunks, self.n_seq), dtype=LD)
        self.ystart[1:] = self.yl[:, idx].T
        # the carry: the kernels keep ONE value per sequence and every time slice overwrites it, so only the last survives the call; the value
        # handed across a slice boundary is the start value of the next slice's first chunk and is checked there (ystart)
        self.carry = self.yl[:, -1]
        self.records = chunk_records(self.xl, aA, aR)
        self.v = self.xs.astype(LD) * np.exp(-self.yl * np.log(LD(10.0)) / LD(20.0))
        self.X = np.abs(self.xl).astype(np.float64).max(axis=1)                       # max |x_l| per sequence
        self.dxl = C_XL * self.bxl.max(axis=1)
        amax, amin = max(aA, aR), min(aA, aR)
        self.reach = 1.0 / (1.0 - amax) if amax < 1.0 else float("inf")
        self.kappa = (amax / amin) ** T if amin > 0 else float("inf")

    def bound_yl(self, n, time_parallel, c=None):
        """of the smoother's value behind n samples (n an array or a number), per sequence [n_seq, ...]: the recursion's own rounding reaches
        back min(n, 1 / (1 - max alpha)) steps; the time-parallel form adds kappa_T, the slope spread of a chunk map; x_l's own error passes
        through a convex combination (never amplified)"""
        c = C_YL if c is None else c
        n = np.asarray(n, dtype=np.float64)
        grow = np.minimum(n, self.reach) + (self.kappa if time_parallel else 0.0)
        return c * U * self.X.reshape((-1,) + (1,) * n.ndim) * grow[None] + self.dxl.reshape((-1,) + (1,) * n.ndim)

    def bound_map(self, c=None):
        """of b_0 and every lb: at most 32 smoother steps from a sample"""
        return (C_MAP if c is None else c) * U * self.X * (COMP_T + 1) + self.dxl


def comp_input(L, n, Cn, seed):
    """Noise at 0.2 with a 200-sample burst at full scale, a stretch scaled by 1e-3, a run of exact zeros, the two float32 neighbours of
    1e-6 (the -120 dB floor decides between them), one 1e-40 and +-1.0"""
    rng = np.random.default_rng(seed)
    x = (0.2 * rng.standard_normal((n, L, Cn))).astype(np.float32)
    q = max(1, L // 6)
    b = min(200, q)
    x[:, q:q + b] = np.clip(5.0 * x[:, q:q + b], -1.0, 1.0)
    x[:, 2 * q:3 * q] *= np.float32(1e-3)
    x[:, 4 * q:4 * q + max(1, q // 2)] = 0.0
    e = np.float32(1e-6)
    for i, v in enumerate((np.nextafter(e, np.float32(0)), np.nextafter(e, np.float32(1)), np.float32(1e-40), np.float32(1.0), np.float32(-1.0))):
        x[:, min(L - 1, 5 * q + 1 + i), i % Cn] = v
    return x


def _comp_call(run, x, thr, attack, release, ratio, sr, in_scale, sumsq, forms, scratch, grid, peak):
    lib = run.lib
    n, L, Cn = (len(thr) if grid else x.shape[0]), x.shape[1], x.shape[2]
    xt = run.t(x.astype(np.float32))
    yt = torch.empty((n, L, Cn), dtype=torch.float32, device=run.device)
    nbytes = lib.mst_fx_compressor_scratch_bytes(n, L, Cn)
    sc = torch.full(((nbytes + 7) // 8,), float("nan"), dtype=torch.float64, device=run.device) if scratch else None
    keep = [xt, yt, sc]
    qs = qm = None
    with lib.device_ctx(xt):
        if grid:
            th, ra = run.t(np.asarray(thr, dtype=np.float64)), run.t(np.asarray(ratio, dtype=np.float64))
            pk = torch.full((n * 64,), float("nan"), dtype=torch.float64, device=run.device) if peak else None
            rc = lib.mst_fx_compressor_grid(xt.data_ptr(), yt.data_ptr(), n, L, Cn, th.data_ptr(), ra.data_ptr(), float(attack), float(release),
                                            float(sr), sc.data_ptr(), nbytes, pk.data_ptr() if peak else None, lib.stream_ptr(xt))
        else:
            st = run.t(np.asarray(in_scale, dtype=np.float64)) if in_scale is not None else None
            qs = torch.full((n * SLOTS,), 1e30, dtype=torch.float64, device=run.device) if sumsq else None
            qm = torch.full((n * SLOTS * 2,), 1e30, dtype=torch.float64, device=run.device) if sumsq and Cn == 2 else None
            fuse = None
            if st is not None or sumsq or forms:
                f = _lib.MstFxFuse(st.data_ptr() if st is not None else None, qs.data_ptr() if sumsq else None, None, 0, 1.0, None,
                                   qm.data_ptr() if qm is not None else None, forms=forms)
                keep.append(f)
                fuse = C.byref(f)
            rc = lib.mst_fx_compressor(xt.data_ptr(), yt.data_ptr(), n, L, Cn, float(thr), float(attack), float(release), float(ratio), float(sr),
                                       sc.data_ptr() if scratch else None, nbytes if scratch else 0, fuse, lib.stream_ptr(xt))
    return rc, yt, sc, qs, qm, (pk if grid and peak else None)


def run_compressor(run, x, thr, attack, release, ratio, sr=44100.0, in_scale=None, sumsq=False, forms=0, scratch=True, grid=False, peak=False):
    """-> dict(rc, y, plan, maps, ystart, carry, tsums, xl, sumsq, ms) as numpy; a refused call returns only rc and the message"""
    n, L, Cn = (len(thr) if grid else x.shape[0]), x.shape[1], x.shape[2]
    plan = run.comp_plan(n, L, Cn, attack, release, sr, forms)
    rc, yt, sc, qs, qm, pk = _comp_call(run, x, thr, attack, release, ratio, sr, in_scale, sumsq, forms, scratch, grid, peak)
    if rc != 0:
        return {"rc": rc, "message": run.lib.mst_last_error().decode(), "plan": plan}
    out = {"rc": 0, "plan": plan, "y": yt.cpu().numpy(), "sumsq": qs.cpu().numpy().reshape(n, SLOTS) if qs is not None else None,
           "ms": qm.cpu().numpy().reshape(n, SLOTS, 2) if qm is not None else None,
           "peak": pk.cpu().numpy().reshape(n, 64).max(axis=1) if pk is not None else None}
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
        if sumsq and plan.form != _lib.FX_COMP_WAVE_SERIAL:
            out["tsums"] = take(plan.tsums_offset, plan.ntiles * (3 * n if Cn == 2 else n_seq)).reshape((plan.ntiles, n, 3) if Cn == 2 else (plan.ntiles, n_seq))
    return out


@functools.lru_cache(maxsize=None)
def comp_reference(key):
    """key = (L, n, C, thr tuple, ratio tuple, attack, release, in_scale tuple or None, shared, seed) -> (x, CompRef); built once and shared"""
    L, n, Cn, thr, ratio, attack, release, scale, shared, seed = key
    x = comp_input(L, 1 if shared else n, Cn, seed)
    xs = np.repeat(x, n, axis=0) if shared else x
    xs32 = operands(xs, None if scale is None else np.asarray(scale)).astype(np.float32)
    aA, aR = comp_alphas(attack, release)
    return x, CompRef(xs32, np.repeat(np.asarray(thr, dtype=np.float64), Cn), np.repeat(np.asarray(ratio, dtype=np.float64), Cn), aA, aR)


def check_compressor(run, L, n, Cn, thr, attack, release, ratio, scale=None, sumsq=False, forms=0, scratch=True, grid=False, seed=1,
                     expect=None, log=print):
    """One compressor call (grid: n candidates (thr[i], ratio[i]) over one shared input, with the peak / clip by-product), every
    intermediate the form leaves behind and every output sample.  expect: plan fields the case is there to reach (asserted)."""
    thr_t = tuple(np.broadcast_to(np.asarray(thr, dtype=np.float64), (n,)).tolist())
    ratio_t = tuple(np.broadcast_to(np.asarray(ratio, dtype=np.float64), (n,)).tolist())
    x, ref = comp_reference((L, n, Cn, thr_t, ratio_t, float(attack), float(release), None if scale is None else tuple(scale), bool(grid), seed))
    got = run_compressor(run, x, list(thr_t) if grid else thr, attack, release, list(ratio_t) if grid else ratio, in_scale=scale, sumsq=sumsq,
                         forms=forms, scratch=scratch, grid=grid, peak=grid)
    plan = got["plan"]
    what = f"comp L={L} n={n} C={Cn} thr={thr} att={attack} rel={release} ratio={ratio} forms={forms}{' grid' if grid else ''}{'' if scratch else ' no scratch'}"
    for k, v in (expect or {}).items():
        assert getattr(plan, k) == v, f"{what}: plan.{k} = {getattr(plan, k)}, the case is there for {v}"
    assert got["rc"] == 0, what + ": " + got.get("message", "")
    tp = scratch and plan.form == _lib.FX_COMP_TIME_PARALLEL
    out = {}
    f64 = lambda a: np.asarray(a).astype(np.float64)
    nidx = np.arange(1, L + 1)
    byl = ref.bound_yl(nidx, tp)                                                      # [n_seq, L]
    if tp:
        assert plan.nchunks == ref.nchunks
        rec = got["maps"]
        sent = f64(ref.records[:, :, :COMP_T + 1]) >= 0.5 * NEVER
        assert np.array_equal(rec[:, :, :COMP_T + 1] >= 0.5 * NEVER, sent) and np.all(rec[:, :, :COMP_T + 1][sent] == NEVER), what + ": 1e300 exactly beyond the chunk's pieces"
        bm = ref.bound_map()[:, None, None]
        err = np.where(sent, 0.0, np.abs(rec[:, :, :COMP_T + 1] - ref.records[:, :, :COMP_T + 1]).astype(np.float64))
        out["maps"] = worst_ratio(err, np.broadcast_to(bm, err.shape))
        bys = ref.bound_yl(np.arange(ref.nchunks) * COMP_T, True).T                   # [nchunks, n_seq]
        out["ystart"] = worst_ratio(f64(np.abs(got["ystart"] - ref.ystart)), bys)
        out["ycarry"] = worst_ratio(f64(np.abs(got["carry"] - ref.carry)), ref.bound_yl(L, True))
        if plan.kappa <= plan.kappa_limit:                                            # conditions (not for a fast attack run before its dispatch), per sequence
            live = np.where(sent, 0.0, f64(np.abs(ref.records[:, :, :COMP_T + 1])))
            top_y = f64(np.abs(ref.yl)).max(axis=1)
            for nm, b, top in (("maps", ref.bound_map(), live.max(axis=(1, 2))), ("ystart", bys.max(axis=0), f64(np.abs(ref.ystart)).max(axis=0)),
                               ("ycarry", ref.bound_yl(L, True), top_y)):
                ok = top > 0                                                           # a sequence that never leaves 0 dB of level difference has nothing to resolve
                assert np.all(b[ok] <= 2.0 ** -30 * top[ok]), f"{what}: the bound of {nm} is 2^{np.log2(float(np.max(b[ok] / top[ok]))):.1f} of its sequence's largest value, not below 2^-30"
    elif scratch and plan.form == _lib.FX_COMP_SPLIT_SERIAL:
        out["yl"] = worst_ratio(f64(np.abs(got["xl"].T - ref.yl)), byl)
        top_y = f64(np.abs(ref.yl)).max(axis=1)
        assert np.all(byl.max(axis=1)[top_y > 0] <= 2.0 ** -30 * top_y[top_y > 0]), what + ": the bound of y_l is not below 2^-30 of its sequence's largest value"
    v = f64(ref.v)
    y = operands(got["y"], None)
    if grid:                                                                           # a candidate whose peak reaches 1 is clipped
        peakv = np.abs(v).reshape(n, -1).max(axis=1)
        assert np.all(np.abs(peakv - 1.0) > 1e-3), what + ": a candidate's peak too close to 1 to tell which side the device took"
        v = np.where(np.repeat(peakv >= 1.0, Cn)[:, None], np.clip(v, -1.0, 1.0), v)
        # the peak by-product itself: max |y| before the clip - of an unclipped candidate the maximum of the observed output, bit for bit; of a
        # clipped one the reference's peak within a float32 rounding and the gain's bound there
        seen = np.abs(got["y"]).reshape(n, -1).max(axis=1).astype(np.float64)
        assert np.array_equal(got["peak"][peakv < 1.0], seen[peakv < 1.0]), what + ": peak of the unclipped candidates"
        tol = f32_bound(peakv, peakv * LN10_20 * byl.reshape(n, -1).max(axis=1))
        assert np.all(np.abs(got["peak"] - peakv)[peakv >= 1.0] <= tol[peakv >= 1.0]) and np.all(seen[peakv >= 1.0] == 1.0), what + ": peak of the clipped candidates"
    out["y"] = worst_ratio(np.abs(y - v), f32_bound(v, np.abs(v) * LN10_20 * byl))
    if sumsq:
        out.update(check_comp_energies(got, n, Cn, L, what))
    log(f"{what} form={plan.form} nchunks={plan.nchunks} nbatch={plan.nbatch} slices={plan.nslices} kappa={plan.kappa:.3g}: " + ", ".join(f"{k} {v:.3f}" for k, v in out.items()))
    bad = {k: v for k, v in out.items() if not v <= 1.0}
    assert not bad, f"{what}: err / bound {bad}"
    return out, got


def check_comp_energies(got, n, Cn, L, what):
    """the per-tile partials, the 64 slots per item (slot s = tiles s, s + 64, ...) and, stereo, the mid / side energies - against float64 sums
    of the call's OWN float32 output (exact operands; the mid / side squares float32 like the kernel's)"""
    out = {}
    y = got["y"]
    ntiles = (L + 63) // 64
    yp = np.zeros((n, ntiles * 64, Cn), dtype=np.float32)
    yp[:, :L] = y
    yt = yp.reshape(n, ntiles, 64, Cn)
    sq = yt.astype(np.float64) ** 2
    slot = np.arange(ntiles) % SLOTS
    fold = lambda a: np.stack([a[:, slot == s].sum(1) for s in range(SLOTS)], 1)      # [n, ntiles, ...] -> [n, SLOTS, ...]
    per_tile = sq.sum((2, 3))                                                          # [n, ntiles]
    cnt = np.stack([(slot == s).sum() for s in range(SLOTS)]) * 64 * Cn
    out["sumsq"] = worst_ratio(np.abs(got["sumsq"] - fold(per_tile)), (cnt + 1) * U * fold(per_tile) + 1e-300)
    if "tsums" in got:
        if Cn == 2:
            m, s = yt[..., 0] + yt[..., 1], yt[..., 0] - yt[..., 1]
            em, es = (m * m).astype(np.float64).sum(2), (s * s).astype(np.float64).sum(2)
            want = np.stack([per_tile, em, es], 2).transpose(1, 0, 2)                  # [tile, item, 3]
            out["tsums"] = worst_ratio(np.abs(got["tsums"] - want), 129 * U * want + 1e-300)
            assert np.all(129 * U * want <= 2.0 ** -30 * want.max(axis=0, keepdims=True)), what + ": tile sums resolved to 2^-30"
            wm = np.stack([fold(em), fold(es)], 2)
            out["ms"] = worst_ratio(np.abs(got["ms"] - wm), (cnt[None, :, None] + 1) * U * wm + 1e-300)
        else:
            want = sq.sum(2).transpose(1, 0, 2).reshape(ntiles, n * Cn)
            out["tsums"] = worst_ratio(np.abs(got["tsums"] - want), 65 * U * want + 1e-300)
            assert np.all(65 * U * want <= 2.0 ** -30 * np.maximum(want.max(axis=0, keepdims=True), 1e-300)), what + ": tile sums resolved to 2^-30"
    return out


# =========================================================================================================== the case lists
# Every shape is the smallest that reaches its branch; `expect` names the plan fields the branch shows in (asserted before the call).
# The sets with a pole near z = 1 (the 80 Hz shelf, the 30 Hz peak, the K-weighting 38 Hz high-pass: A^64 has entries of 40 to 60 and the
# transposed-direct-form states cancel) run through the many-chunk shapes like the well-conditioned ones (the mix-feature low-pass, Butterworth
# low-passes at a quarter of the rate, butter2 .. butter16 = one to eight sections).
VALU_LANE = _lib.FX_FORM_EQ_VALU_ENDS | _lib.FX_FORM_EQ_LANE_APPLY


def _eq_cases():
    cs = []
    add = lambda name, L, n, Cn, **kw: cs.append(dict(name=name, L=L, n=n, Cn=Cn, **kw))
    add("config4", 64, 1, 2, expect=dict(time_parallel=0, nchunks=1))                 # one chunk: serial fx_biquad_kernel
    add("config4", 65, 1, 2, expect=dict(time_parallel=1, nchunks=2, M=64))           # two chunks, tail of 1
    add("kweighting", 128, 1, 1, expect=dict(nchunks=2))                              # exact multiple, mono four-lane ends kernel
    for name in ("config4_p12", "config4_m12", "config4_mixed12", "shelf"):
        add(name, 1000, 2, 2, expect=dict(nchunks=16))
    for name in ("lowpass1000", "kweighting", "peaks4"):
        add(name, 1000, 3, 1, expect=dict(nchunks=16))                                # mono, several items
    for name in ("butter16", "peaks7"):
        add(name, 1000, 2, 3, expect=dict(nchunks=16))                                # C = 3: generic path
    for name in ("lowpass1000", "config4", "peaks5"):
        add(name, 2049, 33, 2, expect=dict(nchunks=33))                               # chunk pairs cross a 128-pair workgroup, idle lanes in the last wave
    for name in ("lowpass1000", "config4"):
        add(name, 64 * 255, 1, 2, expect=dict(nchunks=255, scan_threads=256))
    for name in ("lowpass1000", "shelf", "peaks8"):
        add(name, 64 * 255 + 1, 1, 2, expect=dict(nchunks=256, scan_threads=512))
    for name in ("lowpass1000", "kweighting"):
        add(name, 64 * 256 + 1, 2, 2, expect=dict(nchunks=257, scan_threads=512))
    for k in range(1, 9):                                                              # every band count through the 512-thread scan (eight: stereo)
        add(f"butter{2 * k}", 64 * 255 + 1, 1, 2 if k == 8 else 1, expect=dict(nchunks=256, scan_threads=512))
    for name in ("lowpass1000", "config4", "kweighting"):
        add(name, 50021, 1, 2, expect=dict(M=64, nchunks=782, scan_threads=512))      # more chunks than a scan block: the carry
    for r in (1, 15, 16, 17, 63):                                                      # tails at one M
        add("butter4", 3 * 64 + r, 2, 2, expect=dict(M=64, nchunks=4))
        add("config4", 3 * 64 + r, 2, 2, expect=dict(M=64, nchunks=4))
    add("peaks6", 3 * 64 + 17, 2, 2, expect=dict(M=64, nchunks=4))
    for k in range(1, 9):                                                              # every band count on every pass form, and mono
        add(f"peaks{k}", 113, 2, 2, expect=dict(nchunks=2))                           # MFMA ends, slab apply
        add(f"peaks{k}", 64 * 5 + 17, 3, 2, forms=VALU_LANE, expect=dict(nchunks=6))  # VALU ends, lane apply
        add(f"peaks{k}", 113, 2, 1, expect=dict(nchunks=2))
        add(f"butter{2 * k}", 64 * 5 + 17, 3, 2, forms=VALU_LANE, expect=dict(nchunks=6))
    fused = dict(scale=(0.37, 1.9), sumsq=True, in_sumsq=True)                         # chain fusion, stereo and mono, called twice
    add("lowpass1000", 1000, 2, 2, expect=dict(time_parallel=1, nchunks=16), **fused)
    add("config4", 1000, 2, 2, expect=dict(time_parallel=1, nchunks=16), **fused)
    add("lowpass1000", 1000, 2, 1, expect=dict(time_parallel=1, nchunks=16), **fused)
    add("butter10", 64 * 70 + 5, 2, 2, forms=VALU_LANE, expect=dict(time_parallel=1, nchunks=71), **fused)      # more chunks than slots
    return cs


def _comp_cases():
    cs = []
    add = lambda L, n, Cn, p, **kw: cs.append(dict(L=L, n=n, Cn=Cn, thr=p[0], attack=p[1], release=p[2], ratio=p[3], **kw))
    TP, SS, WS = _lib.FX_COMP_TIME_PARALLEL, _lib.FX_COMP_SPLIT_SERIAL, _lib.FX_COMP_WAVE_SERIAL
    base = (-30.0, 1.5, 60.0, 8.0)
    for thr in (-80.0, -5.0):                                                          # the corners of the product's ranges
        for att in (1.0, 20.0):
            for rel in (50.0, 500.0):
                for ra in (4.0, 40.0):
                    add(1025, 1, 2, (thr, att, rel, ra), expect=dict(form=TP))
    add(1025, 1, 2, (-30.0, 2.0, 100.0, 0.5), expect=dict(form=TP))                    # expander
    add(1025, 1, 2, (-30.0, 2.0, 100.0, 1.0), expect=dict(form=TP))                    # ratio exactly 1: y_g stays 0
    add(1025, 1, 2, (-25.0, 200.0, 60.0, 6.0), expect=dict(form=TP))                   # attack slower than release: the min form
    add(1025, 1, 2, (-25.0, 5.0, 5.0, 3.0), expect=dict(form=TP))                      # equal: linear maps
    add(1500, 1, 2, (-30.0, 0.07, 100.0, 8.0), expect=dict(form=TP))                   # the fast attacks: kappa 3e4 stays time-parallel ...
    for att in (0.03, 0.02, 0.005):                                                    # ... beyond the limit the serial form
        add(1500, 1, 2, (-30.0, att, 100.0, 8.0), expect=dict(form=WS))
    add(1500, 1, 2, (-30.0, 0.01, 0.02, 8.0), expect=dict(form=WS))
    add(96, 1, 2, base, expect=dict(form=SS, nchunks=3))                               # split serial form; xl then holds y_l
    add(96, 2, 2, (-30.0, 0.02, 100.0, 8.0), scale=(1.9, 0.8), sumsq=True, expect=dict(form=SS))      # short and fast: the split form serves fusion
    add(97, 1, 2, base, expect=dict(form=TP, nchunks=4))                               # four chunks, the last of 1
    for L in (128, 1024, 1025, 1056, 2049):                                            # chunk and chain-batch boundaries
        add(L, 1, 2, base, expect=dict(form=TP, nbatch=(L + 1023) // 1024))
    add(9 * 1024 + 517, 1, 2, base, forms=_lib.FX_FORM_COMP_SLICE_SMALL, expect=dict(form=TP, nslices=3, nbatch=10))
    add(9 * 1024 + 517, 2, 1, base, forms=_lib.FX_FORM_COMP_SLICE_SMALL, sumsq=True, expect=dict(form=TP, nslices=3))
    for n, Cn in ((1, 1), (1, 2), (32, 2), (65, 1), (65, 2)):                          # 1, 2, 64, 65, 130 sequences: around the 64-lane wave
        add(200, n, Cn, base, expect=dict(form=TP))
    add(200, 1, 2, base, scratch=False)                                                # fx_compressor_kernel
    add(2049, 6, 2, ((-30.0, -20.0, -10.0, -40.0, -25.0, -15.0), 2.0, 100.0, (8.0, 0.5, 1.0, 40.0, 0.7, 4.0)), grid=True, expect=dict(form=TP))
    add(1025, 2, 2, (-20.0, 2.0, 100.0, 4.0), scale=(1.9, 0.8), sumsq=True, expect=dict(form=TP))      # fused: in_scale, out_sumsq, out_ms
    add(1056, 3, 1, (-20.0, 2.0, 100.0, 4.0), scale=(1.9, 0.8, 1.0), sumsq=True, expect=dict(form=TP))
    return cs


EQ_CASES = _eq_cases()
COMP_CASES = _comp_cases()


def eq_id(c):
    return f"{c['name']}-{c['L']}x{c['n']}x{c['Cn']}" + (f"-forms{c['forms']}" if c.get("forms") else "") + ("-fused" if c.get("sumsq") else "")


def comp_id(c):
    tag = "grid" if c.get("grid") else f"thr{c['thr']:g}-att{c['attack']:g}-rel{c['release']:g}-ratio{c['ratio']:g}"
    return (f"{c['L']}x{c['n']}x{c['Cn']}-{tag}" + (f"-forms{c['forms']}" if c.get("forms") else "") + ("-fused" if c.get("sumsq") else "") +
            ("" if c.get("scratch", True) else "-noscratch"))


# =========================================================================================================== launch coverage
FX_KERNEL = r"^_Z\d+(fx_biquad_\w*kernel|fx_comp_\w*kernel|fx_compressor_kernel|fx_tile_sums_kernel|fx_log10_table_kernel)"


class Tracer:
    """The emulator's dry-run launch trace around one C-ABI call: the kernels are recorded, not run."""

    def __init__(self, emu):
        self.begin, self.end = emu.cdll.emu_trace_begin, emu.cdll.emu_trace_end
        self.begin.restype, self.end.restype, self.end.argtypes = None, C.c_long, [C.c_char_p, C.c_long]
        self.text = C.create_string_buffer(1 << 16)
        self.seen = set()

    def __enter__(self):
        self.begin()
        return self

    def __exit__(self, *a):
        import re
        n = self.end(self.text, len(self.text))
        assert n < len(self.text)
        self.seen.update(ln.split()[0] for ln in self.text.value.decode().splitlines() if re.match(FX_KERNEL, ln))


def trace_cases(emu):
    """The FX kernel symbols the two case lists launch (dry run: no kernel body runs, the buffers are never read)"""
    import contextlib
    run = Runner(emu, "cpu")
    tr = Tracer(emu)
    for c in EQ_CASES:
        x = np.zeros((c["n"], c["L"], c["Cn"]), dtype=np.float32)
        with tr:
            run.equaliser(x, coef_sets()[c["name"]], in_scale=c.get("scale"), sumsq=c.get("sumsq", False), in_sumsq=c.get("in_sumsq", False),
                          forms=c.get("forms", 0))
    for c in COMP_CASES:
        grid = c.get("grid", False)
        x = np.zeros((1 if grid else c["n"], c["L"], c["Cn"]), dtype=np.float32)
        with tr:
            _comp_call(run, x, list(c["thr"]) if grid else c["thr"], c["attack"], c["release"], list(c["ratio"]) if grid else c["ratio"], 44100.0,
                       c.get("scale"), c.get("sumsq", False), c.get("forms", 0), c.get("scratch", True), grid, grid)
    return tr.seen


def exported_fx_kernels(lib_path):
    import re
    import subprocess
    nm = subprocess.run(["nm", "-D", "--defined-only", lib_path], check=True, capture_output=True, text=True).stdout
    return {f[2] for f in (ln.split() for ln in nm.splitlines()) if len(f) == 3 and f[1] in "TW" and re.match(FX_KERNEL, f[2])}


# =========================================================================================================== the constants
def eq_restatement_ratios(run, c):
    """err / (bound with every constant 1) of the float64 restatement of one equaliser case against the longdouble reference"""
    nb = coef_sets()[c["name"]].shape[0]
    plan = run.eq_plan(c["n"], c["L"], c["Cn"], nb)
    if not plan.time_parallel:
        return {}
    scale = c.get("scale")
    _, ref = eq_reference((c["name"], c["L"], c["n"], c["Cn"], None if scale is None else tuple(scale), 0, plan.M))
    tab, pw = ref.restated_tables()
    bh, bp = ref.table_bounds(pw)
    B = ref.bounds(plan.scan_threads, tab, pw)
    v64, _ = run_chunks(ref.Xp, B["starts64"], ref.cf, np.float64)
    v64 = v64.reshape(ref.n_seq, -1)[:, :ref.L]
    f = lambda a: np.abs(a).astype(np.float64)
    return {"table": worst_ratio(f(tab - ref.h), bh + TINY),
            "powers": max(worst_ratio(f(pw[l] - ref.true_powers((1 << l) + 1)[1 << l]), bp[l] + TINY) for l in range(len(bp))),
            "ends": worst_ratio(f(B["ends64"][:, :ref.nfull] - B["ends_exp"]), B["be_r"] + TINY),
            "starts": worst_ratio(f(B["starts64"] - B["starts_exp"]), B["bs_r"] + TINY), "v": worst_ratio(f(v64 - ref.v), B["bv"] + TINY)}


def _unit_dxl(ref):
    """a copy of the reference whose x_l allowance carries constant 1"""
    import copy
    r = copy.copy(ref)
    r.dxl = ref.dxl / C_XL
    return r


def comp_restatement_ratios(run, c):
    """the same for one compressor case: level differences by the table logarithm, chunk maps by sorted insertion, the walk by piece lookup
    (time-parallel cases) or the serial recursion"""
    n, Cn, grid = c["n"], c["Cn"], c.get("grid", False)
    thr_t = tuple(np.broadcast_to(np.asarray(c["thr"], dtype=np.float64), (n,)).tolist())
    ratio_t = tuple(np.broadcast_to(np.asarray(c["ratio"], dtype=np.float64), (n,)).tolist())
    scale = c.get("scale")
    _, ref = comp_reference((c["L"], n, Cn, thr_t, ratio_t, float(c["attack"]), float(c["release"]), None if scale is None else tuple(scale), bool(grid), 1))
    plan = run.comp_plan(n, c["L"], Cn, c["attack"], c["release"], 44100.0, c.get("forms", 0))
    f = lambda a: np.abs(a).astype(np.float64)
    xl64, _ = level_diff(ref.xs, ref.thr, ref.ratio, dtype=np.float64, log10=lambda a: log10_f32_restated(a))
    out = {"xl": worst_ratio(f(xl64 - ref.xl), ref.bxl)}
    ref = _unit_dxl(ref)
    if plan.form == _lib.FX_COMP_TIME_PARALLEL and c.get("scratch", True):
        rec, ys, carry = restate_map_and_walk(xl64, ref.aA, ref.aR)
        sent = f(ref.records[:, :, :COMP_T + 1]) >= 0.5 * NEVER
        err = np.where(sent, 0.0, f(rec[:, :, :COMP_T + 1] - ref.records[:, :, :COMP_T + 1]))
        out["maps"] = worst_ratio(err, np.broadcast_to(ref.bound_map(c=1.0)[:, None, None], err.shape))
        out["ystart"] = worst_ratio(f(ys - ref.ystart), ref.bound_yl(np.arange(ref.nchunks) * COMP_T, True, c=1.0).T)
    else:
        yl64 = smooth(xl64, ref.aA, ref.aR, dtype=np.float64)
        out["yl"] = worst_ratio(f(yl64 - ref.yl), ref.bound_yl(np.arange(1, c["L"] + 1), False, c=1.0))
    return out


# =========================================================================================================== further case bodies
def check_forms_identical(run, k, log=print):
    """k bands, stereo: MFMA ends + slab apply (default) against VALU ends + lane apply, and each alone - the same start states, the same
    output bits; with a short last chunk and with whole chunks only"""
    for name, L, n in ((f"peaks{k}", 113, 2), (f"butter{2 * k}", 64 * 5, 3)):
        x = eq_input(L, n, 2, 3)
        base = run.equaliser(x, coef_sets()[name])
        for forms in (_lib.FX_FORM_EQ_VALU_ENDS, _lib.FX_FORM_EQ_LANE_APPLY, VALU_LANE):
            got = run.equaliser(x, coef_sets()[name], forms=forms)
            assert np.array_equal(got["y"], base["y"]), (name, L, forms)
            assert np.array_equal(got["starts"][:, :, :2 * k], base["starts"][:, :, :2 * k]) and np.array_equal(got["ends"][:, :, :2 * k], base["ends"][:, :, :2 * k]), (name, L, forms)
    log(f"eq forms, {k} bands: identical bits")


FAST = (-30.0, 0.02, 100.0, 8.0)          # threshold, attack ms, release ms, ratio: kappa 6e15, 70 % wrong through the time-parallel form


def check_fast_attack_public_paths(run, log=print):
    """Attack 0.02 ms, release 100 ms through Compressor.process, a chain that arrives at the compressor with a pending rms factor (the fused
    call is refused by the library: the chain must take the unfused path, not raise), compress() and the normaliser's candidate grid: every
    output sample within the serial form's bound.  The module API must be routed through run.lib by the caller."""
    from music_mixing_style_transfer_amd.mixing_manipulator import AugmentationChain, Compressor, Gain
    from music_mixing_style_transfer_amd.mixing_manipulator import _device_ops as D
    from music_mixing_style_transfer_amd.mixing_manipulator import utils_data_normalization as UN
    thr, att, rel, ra = FAST
    L, Cn = 1500, 2
    x = comp_input(L, 1, Cn, 7)[0]
    aA, aR = comp_alphas(att, rel)

    def within(y, xin, thr_v, ra_v, what, clip=False):
        n = xin.shape[0]
        ref = CompRef(operands(xin, None).astype(np.float32), np.repeat(np.asarray(thr_v, dtype=np.float64), Cn), np.repeat(np.asarray(ra_v, dtype=np.float64), Cn), aA, aR)
        v = np.asarray(ref.v).astype(np.float64)
        if clip:
            pk = np.abs(v).reshape(n, -1).max(1)
            assert np.all(np.abs(pk - 1.0) > 1e-3), pk
            v = np.where(np.repeat(pk >= 1.0, Cn)[:, None], np.clip(v, -1.0, 1.0), v)
        r = worst_ratio(np.abs(operands(np.asarray(y), None) - v), f32_bound(v, np.abs(v) * LN10_20 * ref.bound_yl(np.arange(1, L + 1), False)))
        log(f"fast attack through {what}: y {r:.3f}")
        assert r <= 1.0, (what, r)

    plan = run.comp_plan(1, L, Cn, att, rel)
    assert plan.form == _lib.FX_COMP_WAVE_SERIAL and plan.kappa > plan.kappa_limit
    c = Compressor(44100)
    c.parameters.threshold.value, c.parameters.attack_time.value, c.parameters.release_time.value, c.parameters.ratio.value = thr, att, rel, ra
    within(c.process(x.copy())[None], x[None], [thr], [ra], "Compressor.process")
    g = Gain()
    g.parameters.gain.value = 3.0
    staged = AugmentationChain([(g, 1.0, True)], randomize_param_value=False)([x.copy()])[0]      # what the compressor sees: gain, rms-normalised
    y = AugmentationChain([(g, 1.0, True), (c, 1.0, False)], randomize_param_value=False)([x.copy()])[0]
    within(y[None], staged[None], [thr], [ra], "a chain with a pending rms factor")
    y = AugmentationChain([(g, 1.0, True), (c, 1.0, True)], randomize_param_value=False)([x.copy()])[0]
    assert np.isfinite(y).all()
    within(UN.compress(c, x.copy(), 44100, thr, ra, att, rel)[None], x[None], [thr], [ra], "compress()", clip=True)
    ths, ras = [-30.0, 6.0, -40.0], [8.0, 0.5, 40.0]          # the expander lifts everything below +6 dB: its peak passes 1 and it is clipped
    yg = D.compressor_grid(D.to_device(x.copy()), ths, ras, att, rel, 44100, clip=True)
    within(yg.cpu().numpy(), np.repeat(x[None], 3, axis=0), ths, ras, "compressor_grid", clip=True)
    # ratio exactly 1 never reads its threshold; (0 dB, 1) must not be taken for the bypass setting.  Its peak sits at 1: without the clip
    ths, ras = [0.0, -10.0], [1.0, 1.0]
    yg = D.compressor_grid(D.to_device(x.copy()), ths, ras, att, rel, 44100, clip=False)
    within(yg.cpu().numpy(), np.repeat(x[None], 2, axis=0), ths, ras, "compressor_grid, ratio 1")


def check_refusals(run):
    """beyond the conditioning limit a fused call and a grid call return MST_ERR_UNSUPPORTED and say why; nothing is written silently"""
    thr, att, rel, ra = FAST
    x = comp_input(1500, 2, 2, 7)
    got = run_compressor(run, x, thr, att, rel, ra, in_scale=(1.9, 0.8), sumsq=True)
    assert got["rc"] == -2 and "attack" in got["message"] and "release" in got["message"] and "limit" in got["message"], got
    got = run_compressor(run, x[:1], [-30.0, -20.0], att, rel, [8.0, 0.5], grid=True, peak=True)
    assert got["rc"] == -2 and "mst_fx_compressor_grid" in got["message"] and "limit" in got["message"], got
    got = run_compressor(run, x, thr, 0.07, rel, ra, in_scale=(1.9, 0.8), sumsq=True)           # kappa 3e4: served
    assert got["rc"] == 0
