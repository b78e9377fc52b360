#!/usr/bin/env python
"""Does the bf16 TCN forward get faster when the batch walks through the block chain in chunks of c items whose two ping-pong activations
stay in the 256 MiB Infinity Cache?  TCNModel.forward on slices of the headline batch (c items per call, the model's one workspace, so every
chunk reuses the same ping-pong addresses) against the full-batch forward, the two alternating in one process, HIP events around each;
`2xc`: two model handles on two streams, each walking every other chunk.  Default tuning and fusion; the chunked outputs are compared
bit for bit with the full-batch output before anything is timed.

    python tools/bench_tcn_chunks.py [--batch 32] [--steps 5] [--pairs 6] [--settings 1,2,3,4,8,16,2x1,2x2,2x4] [--out tcn_chunks.json]
    rocprofv3 --pmc FETCH_SIZE -d DIR -o pmc --output-format csv -- python tools/bench_tcn_chunks.py --pmc-run 2     (0 = the full batch; with --native: the library's own chunked schedule)
    python tools/bench_tcn_chunks.py --pmc-summary FETCH_DIR WRITE_DIR [--out FILE]        (per kernel name: launches, mean HBM bytes)
"""
import argparse
import csv
import glob
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
SEG = 131072


def pmc_summary(fetch_dir, write_dir, out):
    """Mean FETCH_SIZE / WRITE_SIZE per launch of every kernel name, as bytes (tools/pmc_traffic.py's correction: FETCH_SIZE x 2 on gfx950)."""
    def table(d, counter):
        acc = {}
        for path in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            for r in csv.DictReader(open(path)):
                if r["Counter_Name"] == counter:
                    k = acc.setdefault(r["Kernel_Name"], [0.0, 0, int(r["Grid_Size"]) // 256 if "Grid_Size" in r else 0])
                    k[0] += float(r["Counter_Value"])
                    k[1] += 1
        return acc
    f, w = table(fetch_dir, "FETCH_SIZE"), table(write_dir, "WRITE_SIZE")
    res = {}
    for name in sorted(set(f) | set(w)):
        if "tcn_" not in name:
            continue
        fs, fn, grid = f.get(name, [0.0, 0, 0])
        ws, wn, _ = w.get(name, [0.0, 0, 0])
        res[name] = {"launches": [fn, wn], "workgroups": grid, "read_bytes_per_launch": 2.0 * 1024.0 * fs / max(fn, 1),
                     "write_bytes_per_launch": 1024.0 * ws / max(wn, 1), "read_bytes_total": 2.0 * 1024.0 * fs, "write_bytes_total": 1024.0 * ws}
        print(f"{name[:70]:70s} launches {fn:4d} read {res[name]['read_bytes_per_launch'] / 1e9:8.4f} GB write "
              f"{res[name]['write_bytes_per_launch'] / 1e9:8.4f} GB per launch", flush=True)
    tot = {"read_bytes_total": sum(v["read_bytes_total"] for v in res.values()), "write_bytes_total": sum(v["write_bytes_total"] for v in res.values())}
    print(f"all TCN launches of the run: read {tot['read_bytes_total'] / 1e9:.3f} GB, write {tot['write_bytes_total'] / 1e9:.3f} GB", flush=True)
    if out:
        os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
        json.dump({"kernels": res, "total": tot, "note": "read = 2 x FETCH_SIZE x 1024, write = WRITE_SIZE x 1024; separate --pmc passes"},
                  open(out, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=6)
    ap.add_argument("--settings", default="1,2,3,4,8,16,2x1,2x2,2x4")
    ap.add_argument("--segment", type=int, default=131072)
    ap.add_argument("--pmc-run", default=None, help="one warm-up and one forward of this setting and nothing else (for rocprofv3 --pmc); 0 = full batch")
    ap.add_argument("--pmc-summary", nargs=2, default=None, metavar=("FETCH_DIR", "WRITE_DIR"))
    ap.add_argument("--native", action="store_true", help="leave the handles' automatic chunking on: setting 0 is then the library's own schedule "
                                                          "(two chains of 2 items at 32 x 131072), the other settings slices of it")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.pmc_summary:
        return pmc_summary(args.pmc_summary[0], args.pmc_summary[1], args.out)
    global SEG
    SEG = args.segment
    import torch
    import yaml
    from music_mixing_style_transfer_amd import _lib
    from music_mixing_style_transfer_amd.networks import TCNModel
    from music_mixing_style_transfer_amd.utils import synth

    dev = torch.device("cuda", 0)
    with open(os.path.join(REPO, "music_mixing_style_transfer_amd", "networks", "configs.yaml")) as f:
        cfg = yaml.full_load(f)["TCN"]["default"]
    sd = synth.tcn_state_dict(seed=0)

    def model():
        m = TCNModel(nparams=cfg["condition_dimension"], ninputs=2, noutputs=2, nblocks=cfg["nblocks"], dilation_growth=cfg["dilation_growth"],
                     kernel_size=cfg["kernel_size"], channel_width=cfg["channel_width"], stack_size=cfg["stack_size"],
                     cond_dim=cfg["condition_dimension"], causal=cfg["causal"]).to(dev)
        m.load_state_dict(sd)
        m.precision = "bf16"
        return m

    tcn = [model(), model()]
    lib = _lib.lib()
    for m in tcn:
        m._ensure(lib)
        if not args.native:      # the gate's question: every call here is ONE launch table, the library's own chunking (mst_tcn_set_chunk) off
            lib.check(lib.mst_tcn_set_chunk(m._handle, _lib.TCN_CHUNK_WHOLE), "set_chunk")
    side = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    B = args.batch
    x = synth.synth_audio((B, 2, SEG), seed=200).to(dev)
    cond = synth.synth_audio((1, cfg["condition_dimension"]), seed=3).to(dev)

    def forward(setting):
        """One forward of the whole batch under `setting` ('0' full batch, 'c' chunks of c on the current stream, '2xc' two handles on two
        side streams forked from and joined into the current stream); returns the list of (first item, y) per call."""
        if setting == "0":
            return [(0, tcn[0](x, cond))]
        two = setting.startswith("2x")
        c = int(setting[2:] if two else setting)
        ys = []
        if not two:
            for i in range(0, B, c):
                ys.append((i, tcn[0](x[i:i + c], cond)))
            return ys
        cur = torch.cuda.current_stream(dev)
        for s in side:
            s.wait_stream(cur)
        for k, i in enumerate(range(0, B, c)):
            with torch.cuda.stream(side[k & 1]):
                ys.append((i, tcn[k & 1](x[i:i + c], cond)))
        for s in side:
            cur.wait_stream(s)
        return ys

    if args.pmc_run is not None:
        for _ in range(2):
            forward(args.pmc_run)
            torch.cuda.synchronize()
        return

    settings = args.settings.split(",")
    y_full = forward("0")[0][1].clone()
    torch.cuda.synchronize()
    out = {"batch": B, "segment": SEG, "steps": args.steps, "settings": {}}
    for s in settings:
        ys = forward(s)
        torch.cuda.synchronize()
        same = all(bool(torch.equal(y, y_full[i:i + y.shape[0]])) for i, y in ys)
        out["settings"][s] = {"bit_identical": same, "calls": len(ys), "pairs": []}
        print(f"setting {s}: {len(ys)} calls, bit identical to the full batch: {same}", flush=True)
        if not same:
            sys.exit("a chunked forward does not give the bits of the full batch: nothing timed")
        del ys

    def timed(setting):
        for _ in range(2):
            forward(setting)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            forward(setting)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / args.steps

    for s in settings:
        rec = out["settings"][s]
        for r in range(args.pairs):
            full, chunked = timed("0"), timed(s)
            rec["pairs"].append({"full_ms": full, "chunked_ms": chunked})
            print(f"setting {s} pair {r}: full {full:.4f} ms, chunked {chunked:.4f} ms ({100.0 * (chunked - full) / full:+.2f} %)", flush=True)
        gains = [100.0 * (p["full_ms"] - p["chunked_ms"]) / p["full_ms"] for p in rec["pairs"]]
        rec["min_gain_percent"], rec["median_gain_percent"] = min(gains), sorted(gains)[len(gains) // 2]
        print(f"setting {s}: gain over the full batch min {min(gains):+.2f} %, median {rec['median_gain_percent']:+.2f} %", flush=True)
        if args.out:
            os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
            json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
