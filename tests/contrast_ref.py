"""TEST INFRASTRUCTURE: the reference's contrastive and gain losses (modules/loss.py: NT_Xent :24-71, RMSLoss :77-93, infoNCE :228-238) and
their gradients in float64 numpy, in this project's own words, each with an error bound derived from the operands.

The arithmetic (the closed form of the reference's autograd graph):
  zh_i = z_i / max(|z_i|, eps)       S_ij = zh_i . zh_j / tau
  NT-Xent   p(i) = i +- N / 2, term_i = -S_i,p(i) + log sum_{j != i} exp S_ij, loss = mean term_i     (eps 1e-8: nn.CosineSimilarity)
  infoNCE   S = A B^T / tau, A = normalize(nn), B = normalize(p), label i -> i, nothing masked        (eps 1e-12: F.normalize)
  G_ij  = (softmax_j(S_i.) - [j = p(i)]) dloss / rows
  dZh   = (G + G^T) Zh / tau          (infoNCE: dA = G B / tau, dB = G^T A / tau)
  dz_i  = (dzh_i - zh_i (zh_i . dzh_i)) / |z_i|
  RMSLoss   rms = sqrt(mean_t x^2) per [B C] row, w = wf max(|rms_t - rms_e|, 1 / wf), loss = mean(w^1.5) mean((rms_e - rms_t)^2)
            (nn.MSELoss(reduce=None) is the mean reduction), d loss / d est[r, t] = c_r est[r, t].
Two departures from the reference's autograd, both in the backward only: a row whose norm is below eps gets a gradient of exact zeros (the
reference's is dzh / eps, 1e8-scale numbers), and a row of est without energy gets zeros where the reference gives NaN.

The bounds (u = 2^-24).  A normalised value carries two roundings; a Gram entry is one k-ordered float32 chain over D:
  bS_ij   = 4 sqrt(D + 8) u sum_k |zh_ik zh_jk| / tau + u |S_ij|             (the project's accumulation term, plus one rounding)
  term_i    bS_i,p(i) + sum_j softmax_ij expm1(bS_ij)                          (log-sum-exp moves by at most log sum_j softmax_j e^(b_j))
  loss      the mean of those + u |loss|                                       (the value is returned as float32)
  softmax   bp_ij = softmax_ij e^(2 max_j bS_ij) (bS_ij + sum_m softmax_im bS_im)
  G         bG_ij = (bp_ij + u |softmax_ij - [j = p]|) |dloss| / rows          (G is stored as float32)
  P = G + G^T: bP = bG + bG^T + u |P|
  dZh_id    sum_j (bP_ij + (2 + 4 sqrt(rows + 8)) u |P_ij|) |zh_jd| / tau + u |dzh_id|      (operand roundings, the chain over j, one rounding)
  r_i = zh_i . dzh_i:  br_i = sum_d |zh_id| (bdZh_id + 2 u |dzh_id|)
  dz_id     (bdZh_id + |zh_id| br_i + 2 u |zh_id r_i|) / |z_i| + 3 u |dz_id|
  RMS       a float32 mean square of T values errs by (2 + log2 T) u relatively, its root by half of that plus u: e = (2 + log2(T) / 2) u;
            bd = e (rms_e + rms_t) + u |d|, bw = wf bd + u w, b(w^1.5) = 1.5 sqrt(w) bw + 2 u w^1.5, b(d^2) = 2 |d| bd + u d^2; the two
            means add u each; loss W Q: bW Q + W bQ + u |loss|; c_r likewise, product rule term by term, and a row within bd of the clamp's
            edge |d| = 1 / wf is charged the whole w-branch (a float32 run may legitimately land on either side).
Each bound is multiplied by ONE constant per quantity, fixed by the project's rule against the reference ALONE:
tests/golden/make_golden_contrast.py runs the reference's own code under autograd in float32 and in float64 and records the largest
|fp32 - float64| / bound(c = 1); the constant is twice that, rounded up.
"""
import math

import numpy as np

U32 = 2.0 ** -24
NTX_EPS, NCE_EPS = 1e-8, 1e-12
WEIGHT_FACTOR = 100.0

# Reference alone, max |fp32 autograd - float64 autograd| / bound(c = 1) over the cases of tests/golden/contrast.npz (printed by the generator):
#   NT-Xent loss      0.0077 (flat)           gradient 0.0207 (flat; sharp 0.0041, strips 0.0009)
#   infoNCE           0.1202 (sharp, gradient; its loss 0.0004 at most)
#   RMS               0.0916 (clamped, gradient; loss 0.0841 on silent_row)
# The bounds add absolute values where the errors carry signs, and the reference's float32 dot products are pairwise sums, not chains: a run
# shows far less than they allow.
MEASURED_MAX_RATIO = {"ntx_loss": 0.0077, "ntx_grad": 0.0207, "nce": 0.1202, "rms": 0.0916}
# twice that, rounded up (the generator prints ceil(2 x)):
C_NTX_LOSS = 1.0
C_NTX_GRAD = 1.0
C_NCE = 1.0
C_RMS = 1.0


# ---- the cases: integer recipes, nothing stored ---------------------------------------------------------------------------------------------
def _noise(seed, shape):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=shape).astype(np.float32)


# name -> (rows per view, D, tau)
NTX_CASES = {
    "tiny1": (1, 1, 0.1),
    "tiny3": (3, 7, 0.1),
    "ragged": (17, 130, 0.1),
    "strips": (40, 2048, 0.1),
    "sharp": (17, 64, 0.01),
    "flat": (17, 64, 0.5),
    "scales": (17, 130, 0.1),
    "same": (17, 64, 0.1),
    "zero_row": (17, 64, 0.1),
}
NCE_CASES = {"ragged": (17, 130, 0.1), "sharp": (17, 64, 0.01), "zero_row": (17, 64, 0.1)}
ZERO_ROW = 5          # of the first view


def ntx_case_inputs(name, D=None):
    """(z_i, z_j, tau) of an NT-Xent case, float32 [B, D]; `D` overrides the width (the emulator runs `strips` narrower)"""
    B, D0, tau = NTX_CASES[name]
    D = D0 if D is None else D
    seed = 300 + sorted(NTX_CASES).index(name)
    zi = _noise(seed, (B, D))
    zj = (np.float32(0.7) * zi + np.float32(0.5) * _noise(seed + 50, (B, D))).astype(np.float32)      # a positive pair is correlated
    if name == "sharp":          # two duplicated rows: ties in the max at logits of 100
        zi[3] = zi[2]
        zj[9] = zi[8]
    elif name == "scales":
        s = (10.0 ** np.linspace(-3.0, 3.0, B)).astype(np.float32)[:, None]
        zi, zj = (zi * s).astype(np.float32), (zj * s[::-1]).astype(np.float32)
    elif name == "same":
        zj = zi.copy()
    elif name == "zero_row":
        zi[ZERO_ROW] = 0.0
    return np.ascontiguousarray(zi), np.ascontiguousarray(zj), tau


def nce_case_inputs(name):
    """(nn, p, tau) of an infoNCE case: two distinct views"""
    B, D, tau = NCE_CASES[name]
    seed = 400 + sorted(NCE_CASES).index(name)
    a = _noise(seed, (B, D))
    b = (np.float32(0.6) * a + np.float32(0.6) * _noise(seed + 50, (B, D))).astype(np.float32)
    if name == "sharp":
        a[3] = a[2]
        b[9] = b[8]
    elif name == "zero_row":
        a[ZERO_ROW] = 0.0
    return np.ascontiguousarray(a), np.ascontiguousarray(b), tau


# name -> (B, C, T)
RMS_CASES = {"short": (2, 2, 16), "odd": (3, 2, 1000), "real": (2, 2, 131072), "clamped": (2, 2, 1000), "silent_row": (2, 2, 1000)}
SILENT_ROW = 1


def rms_case_inputs(name):
    """(est, tgt) float32 [B, C, T]; the row levels differ by far more than 1 / wf except in `clamped`, whose row 2 differs by about 0.003"""
    shape = RMS_CASES[name]
    seed = 500 + sorted(RMS_CASES).index(name)
    rows = shape[0] * shape[1]
    le = np.linspace(0.2, 0.6, rows, dtype=np.float32).reshape(shape[0], shape[1], 1)
    lt = le[::-1, ::-1] * np.float32(0.5) + np.float32(0.05)
    est, tgt = _noise(seed, shape) * le, _noise(seed + 50, shape) * lt
    if name == "clamped":
        tgt[1, 0] = est[1, 0] * np.float32(1.01)
    elif name == "silent_row":
        est[SILENT_ROW // shape[1], SILENT_ROW % shape[1]] = 0.0
    return np.ascontiguousarray(est.astype(np.float32)), np.ascontiguousarray(tgt.astype(np.float32))


# ---- NT-Xent / infoNCE ---------------------------------------------------------------------------------------------------------------------
def _normalize(z, eps):
    z = np.asarray(z, dtype=np.float64)
    norm = np.sqrt((z * z).sum(axis=1))
    inv_fwd = 1.0 / np.maximum(norm, eps)
    inv_bwd = np.where(norm < eps, 0.0, inv_fwd)          # the first departure
    return z * inv_fwd[:, None], inv_bwd


def _softmax_rows(S, masked):
    X = np.where(masked, -np.inf, S)
    mx = X.max(axis=1, keepdims=True)
    if not np.all(np.isfinite(mx)):          # no row is empty in any mode: N = 2 leaves the positive
        raise ValueError("a row without logits")
    e = np.exp(X - mx)
    tot = e.sum(axis=1, keepdims=True)
    return e / tot, (mx + np.log(tot))[:, 0]


def _contrast(X, Y, inv_x, inv_y, tau, masked, pos, dloss, c_loss, c_grad, symmetric):
    """the shared body: X [M, D], Y [Nc, D] normalised; returns loss, its bound, (dX, dY) or dZ and the bounds"""
    M, D = X.shape
    rows = np.arange(M)
    S = X @ Y.T / tau
    bS = 4.0 * math.sqrt(D + 8) * U32 * (np.abs(X) @ np.abs(Y).T) / tau + U32 * np.abs(S)
    bS = np.where(masked, 0.0, bS)
    P, lse = _softmax_rows(S, masked)
    term = lse - S[rows, pos]
    bterm = bS[rows, pos] + (P * np.expm1(bS)).sum(axis=1)
    loss = term.mean()
    bloss = c_loss * (bterm.mean() + U32 * abs(loss))
    onehot = np.zeros_like(S)
    onehot[rows, pos] = 1.0
    G = (P - onehot) * dloss / M
    bp = P * np.exp(2.0 * bS.max(axis=1, keepdims=True)) * (bS + (P * bS).sum(axis=1, keepdims=True))
    bG = (bp + U32 * np.abs(P - onehot)) * abs(dloss) / M

    def through(Pm, bPm, Yh, Xh, inv):
        K = Pm.shape[1]
        dZh = Pm @ Yh / tau
        bdZh = ((bPm + (2.0 + 4.0 * math.sqrt(K + 8)) * U32 * np.abs(Pm)) @ np.abs(Yh)) / tau + U32 * np.abs(dZh)
        r = (Xh * dZh).sum(axis=1, keepdims=True)
        br = (np.abs(Xh) * (bdZh + 2.0 * U32 * np.abs(dZh))).sum(axis=1, keepdims=True)
        dz = (dZh - Xh * r) * inv[:, None]
        bdz = (bdZh + np.abs(Xh) * br + 2.0 * U32 * np.abs(Xh * r)) * inv[:, None] + 3.0 * U32 * np.abs(dz)
        return dz, c_grad * bdz

    if symmetric:
        Pm = G + G.T
        return loss, bloss, through(Pm, bG + bG.T + U32 * np.abs(Pm), Y, X, inv_x)
    return loss, bloss, through(G, bG, Y, X, inv_x), through(G.T, bG.T, X, Y, inv_y)


def ntxent(z_i, z_j, tau, dloss=1.0, c_loss=None, c_grad=None):
    """-> loss, its bound, grad [2 B, D] (rows of z_i, then of z_j), its bound"""
    z = np.concatenate([np.asarray(z_i, dtype=np.float64), np.asarray(z_j, dtype=np.float64)], axis=0)
    N = z.shape[0]
    Zh, inv = _normalize(z, NTX_EPS)
    pos = (np.arange(N) + N // 2) % N
    loss, bloss, (g, bg) = _contrast(Zh, Zh, inv, inv, tau, np.eye(N, dtype=bool), pos, dloss, C_NTX_LOSS if c_loss is None else c_loss,
                                     C_NTX_GRAD if c_grad is None else c_grad, True)
    return loss, bloss, g, bg


def infonce(a, b, tau, dloss=1.0, c=None):
    """-> loss, its bound, (grad_nn, bound), (grad_p, bound)"""
    c = C_NCE if c is None else c
    A, inv_a = _normalize(a, NCE_EPS)
    B, inv_b = _normalize(b, NCE_EPS)
    n = A.shape[0]
    return _contrast(A, B, inv_a, inv_b, tau, np.zeros((n, n), dtype=bool), np.arange(n), dloss, c, c, False)


def mask_correlated_samples(batch_size, world_size=1):
    N = 2 * batch_size * world_size
    mask = np.ones((N, N), dtype=bool)
    np.fill_diagonal(mask, False)
    for i in range(batch_size * world_size):
        mask[i, batch_size + i] = False
        mask[batch_size + i, i] = False
    return mask


# ---- RMSLoss -------------------------------------------------------------------------------------------------------------------------------
def rms_loss(est, tgt, dloss=1.0, c=None, wf=WEIGHT_FACTOR):
    """-> loss, its bound, grad [B, C, T] with respect to est, its bound"""
    c = C_RMS if c is None else c
    shape = np.asarray(est).shape
    e = np.asarray(est, dtype=np.float64).reshape(-1, shape[-1])
    t = np.asarray(tgt, dtype=np.float64).reshape(-1, shape[-1])
    R, T = e.shape
    re, rt = np.sqrt((e * e).mean(axis=1)), np.sqrt((t * t).mean(axis=1))
    d = re - rt
    a = np.abs(d)
    w = wf * np.maximum(a, 1.0 / wf)
    W, Q = (w ** 1.5).mean(), (d * d).mean()
    loss = W * Q
    rel = (2.0 + math.log2(T) / 2.0) * U32
    bd = rel * (re + rt) + U32 * a
    bw = wf * bd + U32 * w
    bW = (1.5 * np.sqrt(w) * bw + 2.0 * U32 * w ** 1.5).mean() + U32 * W
    bQ = (2.0 * a * bd + U32 * d * d).mean() + U32 * Q
    bloss = c * (bW * Q + W * bQ + U32 * abs(loss))
    dw = np.where(a >= 1.0 / wf, wf * np.sign(d), 0.0)
    x1 = 1.5 * np.sqrt(w) * dw * Q
    x2 = 2.0 * W * d
    edge = np.abs(a - 1.0 / wf) <= bd
    bx1 = np.where(dw != 0.0, 1.5 * wf * (0.5 * bw / np.sqrt(w) * Q + np.sqrt(w) * bQ), 0.0) + 3.0 * U32 * np.abs(x1) + edge * 1.5 * np.sqrt(w) * wf * Q
    bx2 = 2.0 * (bW * a + W * bd) + 2.0 * U32 * np.abs(x2)
    live = re > 0.0          # the second departure
    den = np.where(live, T * re, 1.0)
    coef = np.where(live, dloss * (x1 + x2) / R / den, 0.0)
    bcoef = np.where(live, abs(dloss) * (bx1 + bx2) / R / den + (rel + 3.0 * U32) * np.abs(coef), 0.0)
    grad = coef[:, None] * e
    bgrad = c * (bcoef[:, None] * np.abs(e) + U32 * np.abs(grad))
    return loss, bloss, grad.reshape(shape), bgrad.reshape(shape)


def ratio(err, bnd):
    """max err / bound; an error where the bound is zero counts as infinite"""
    err, bnd = np.asarray(err, dtype=np.float64), np.asarray(bnd, dtype=np.float64)
    r = np.divide(err, bnd, out=np.zeros_like(err), where=bnd > 0)
    r = np.where((bnd == 0) & (err > 0), np.inf, r)
    return float(r.max())
