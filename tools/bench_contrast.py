#!/usr/bin/env python
"""Value + gradient of NT_Xent (modules/loss.py on csrc/contrast_kernels.h) at N = 2 B rows of a D-wide embedding on one MI355X, against two
torch formulations on the same device:
  (a) "reference": the reference's own NT_Xent.forward - the broadcast nn.CosineSimilarity(dim=2) over [N, N, D], the boolean mask, a
      CrossEntropyLoss - under autograd.  Skipped where N N D 4 3 bytes exceed 64 GB (noted in the record).
  (b) "mm": the fair competitor - F.normalize, one mm, a masked cross_entropy - under autograd.
and of RMSLoss at [32, 2, 131072] against its torch form.  The compared forms run in one process, alternating, after all have been warmed;
each round is `--steps` value + gradient calls between two events; medians with min and max.  Peak memory is torch's allocator peak over
one call of each, above what was allocated before it.  Prints ONE JSON line per size and writes them to --out.

    python tools/bench_contrast.py [--rows 512 1024 2048] [--dim 2048] [--tau 0.1] [--rounds 7] [--steps 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BROADCAST_LIMIT = 64e9


class ReferenceNTXent(torch.nn.Module):
    """the reference's formulation, statement for statement (world_size = 1)"""

    def __init__(self, batch_size, temperature):
        super().__init__()
        self.batch_size, self.temperature = batch_size, temperature
        N = 2 * batch_size
        mask = torch.ones((N, N), dtype=bool).fill_diagonal_(0)
        for i in range(batch_size):
            mask[i, batch_size + i] = 0
            mask[batch_size + i, i] = 0
        self.mask = mask
        self.criterion = torch.nn.CrossEntropyLoss(reduction="sum")
        self.similarity_f = torch.nn.CosineSimilarity(dim=2)

    def forward(self, z_i, z_j):
        N = 2 * self.batch_size
        z = torch.cat((z_i, z_j), dim=0)
        sim = self.similarity_f(z.unsqueeze(1), z.unsqueeze(0)) / self.temperature
        sim_i_j, sim_j_i = torch.diag(sim, self.batch_size), torch.diag(sim, -self.batch_size)
        positive = torch.cat((sim_i_j, sim_j_i), dim=0).reshape(N, 1)
        negative = sim[self.mask.to(sim.device)].reshape(N, -1)
        logits = torch.cat((positive, negative), dim=1)
        return self.criterion(logits, torch.zeros(N, device=sim.device).long()) / N


def mm_ntxent(z_i, z_j, tau, eye, labels):
    z = F.normalize(torch.cat((z_i, z_j), dim=0), dim=1, eps=1e-8)
    return F.cross_entropy((z @ z.T / tau).masked_fill(eye, float("-inf")), labels)


def torch_rms(est, tgt, wf=100.0):
    e, t = est.reshape(-1, est.shape[2]), tgt.reshape(-1, tgt.shape[2])
    re, rt = torch.sqrt(torch.mean(e ** 2, dim=-1)), torch.sqrt(torch.mean(t ** 2, dim=-1))
    w = torch.clamp(torch.abs(rt - re), min=1 / wf) * wf
    return torch.mean(w ** 1.5 * F.mse_loss(re, rt))


def compare(forms, leaves, a):
    """forms: name -> callable returning the loss; every call is value + gradient.  -> per form (median ms, [min, max], peak bytes, value)"""
    def step(fn):
        for x in leaves:
            x.grad = None
        v = fn()
        v.backward()
        return v

    for _ in range(3):
        for fn in forms.values():
            step(fn)
    torch.cuda.synchronize()
    times = {k: [] for k in forms}
    for _ in range(a.rounds):          # alternating: a drift of the clock or a neighbour on the host hits every form
        for k, fn in forms.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(a.steps):
                step(fn)
            e.record()
            torch.cuda.synchronize()
            times[k].append(s.elapsed_time(e) / a.steps)
    out = {}
    for k, fn in forms.items():
        for x in leaves:
            x.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        v = step(fn)
        torch.cuda.synchronize()
        out[k] = {"ms": statistics.median(times[k]), "ms_min_max": [min(times[k]), max(times[k])],
                  "peak_bytes": torch.cuda.max_memory_allocated() - before, "value": float(v.detach()),
                  "grad": [x.grad.clone() for x in leaves]}
    return out


def measure_ntx(a, N):
    from music_mixing_style_transfer_amd.modules import NT_Xent
    dev = torch.device("cuda:0")
    B = N // 2
    g = torch.Generator().manual_seed(N)
    zi = torch.randn(B, a.dim, generator=g).to(dev)
    zj = (0.7 * zi + 0.5 * torch.randn(B, a.dim, generator=g).to(dev)).requires_grad_(True)
    zi.requires_grad_(True)
    ours = NT_Xent(B, a.tau, 1, differentiable=True)
    eye = torch.eye(N, dtype=torch.bool, device=dev)
    labels = (torch.arange(N, device=dev) + B) % N
    forms = {"hip": lambda: ours(zi, zj), "torch_mm": lambda: mm_ntxent(zi, zj, a.tau, eye, labels)}
    broadcast_bytes = N * N * a.dim * 4 * 3
    if broadcast_bytes <= BROADCAST_LIMIT:
        ref = ReferenceNTXent(B, a.tau)
        forms["torch_reference_broadcast"] = lambda: ref(zi, zj)
    r = compare(forms, [zi, zj], a)
    rec = {"metric": "NT_Xent, value + gradient, ms per call", "N": N, "D": a.dim, "tau": a.tau, "rounds": a.rounds, "steps": a.steps,
           "operand_bytes": N * a.dim * 4}
    gm = torch.cat(r["torch_mm"]["grad"])
    for k, v in r.items():
        gk = torch.cat(v.pop("grad"))
        rec[k] = dict(v, grad_max_abs_diff_vs_torch_mm_over_max_abs=float((gk - gm).abs().max() / gm.abs().max()))
    rec["speedup_vs_torch_mm"] = r["torch_mm"]["ms"] / r["hip"]["ms"]
    rec["peak_ratio_torch_mm_over_hip"] = r["torch_mm"]["peak_bytes"] / max(r["hip"]["peak_bytes"], 1)
    if "torch_reference_broadcast" in r:
        rec["speedup_vs_torch_reference_broadcast"] = r["torch_reference_broadcast"]["ms"] / r["hip"]["ms"]
        rec["peak_ratio_torch_reference_broadcast_over_hip"] = r["torch_reference_broadcast"]["peak_bytes"] / max(r["hip"]["peak_bytes"], 1)
    else:
        rec["torch_reference_broadcast"] = f"skipped: N N D 4 3 = {broadcast_bytes / 1e9:.1f} GB of broadcast operands exceed {BROADCAST_LIMIT / 1e9:.0f} GB"
    return rec


def measure_rms(a):
    from music_mixing_style_transfer_amd.modules import RMSLoss
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7)
    tgt = (0.3 * torch.randn(32, 2, 131072, generator=g)).to(dev)
    est = (0.5 * tgt + 0.02 * torch.randn(32, 2, 131072, generator=g).to(dev)).requires_grad_(True)
    ours = RMSLoss(True, differentiable=True)
    r = compare({"hip": lambda: ours(est, tgt), "torch": lambda: torch_rms(est, tgt)}, [est], a)
    rec = {"metric": "RMSLoss, value + gradient, ms per call", "shape": [32, 2, 131072], "rounds": a.rounds, "steps": a.steps,
           "waveform_bytes": 2 * 32 * 2 * 131072 * 4}
    gt = r["torch"]["grad"][0]
    for k, v in r.items():
        gk = v.pop("grad")[0]
        rec[k] = dict(v, grad_max_abs_diff_vs_torch_over_max_abs=float((gk - gt).abs().max() / gt.abs().max()))
    rec["speedup_vs_torch"] = r["torch"]["ms"] / r["hip"]["ms"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[512, 1024, 2048], help="N = rows of cat(z_i, z_j)")
    ap.add_argument("--dim", type=int, default=2048)
    ap.add_argument("--tau", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "contrast_bench_mi355x.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_contrast.py measures on the MI355X; no GPU is visible and there is no CPU path")
    results = []
    for N in a.rows:
        results.append(measure_ntx(a, N))
        print(json.dumps(results[-1]), flush=True)
        torch.cuda.empty_cache()
    results.append(measure_rms(a))
    print(json.dumps(results[-1]), flush=True)
    with open(a.out, "w") as f:
        json.dump(results, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
