"""Device time of one block of the navigation graph (dllm_neighbor_rows: `block` stored rows against the
whole store on the int8 matrix cores) next to what the library offered for the same job before it:
``decompress_vectors`` of the block, then ``search_vectors`` with the f32 rows as queries.

Store: rows x dim (default 64 Ki x 768) N(0,1) vectors compressed at 8 bits; k = 10; blocks of 256 query
rows; the search table and the pair table prebuilt (neither arm pays for them).  One process, both arms
in every round (interleaved), 0.3 s warm-up per arm, HIP events around `reps` back-to-back calls through
the Python wrappers (both arms allocate their outputs and workspace per call, as a user's call does);
the block moves through the store from call to call.  The baseline asks for k + 1 rows, since it has no
way to leave the query's own row out; the own row is removed on the host for the agreement figure only
(outside the timed window).  The two arms follow different pinned rules (8g rounds f32 strand sums, 8l
is exact to the last cast), so near-ties may rank differently: the share of query rows whose id lists
agree is informational.

The kernel split comes from a separate profiler pass (the tracer slows the host, so no wall-clock
figure is taken from it):
    rocprofv3 --kernel-trace -d DIR -o trace --output-format csv -- \\
        python scripts/neighbors_time.py --trace-run
    python scripts/neighbors_time.py --merge-stats DIR --out profiles/neighbors/times.json
--trace-run makes 10 calls of the new arm at the timed shape and 10 at dim 64 with the same rows and
block: the scan at dim 64 is one MFMA step per tile, i.e. the epilogue (the f64 rule per pair and the
score write) with almost no matrix work, an upper estimate of the epilogue's share of the full scan.

Usage: python scripts/neighbors_time.py [--rows 65536] [--dim 768] [--k 10] [--block 256] [--rounds 7]
                                        [--reps 10] [--out profiles/neighbors/times.json]"""
import argparse
import csv
import json
import re
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def merge_stats(folder, out):
    """Adds the kernels' average times from rocprofv3's *kernel_trace.csv under `folder` to `out`: per
    kernel the calls in start order, the first half made at the timed shape, the second half at dim 64."""
    files = sorted(Path(folder).rglob("*kernel_trace.csv"))
    assert files, f"no *kernel_trace.csv under {folder}"
    calls = {}
    for row in csv.DictReader(files[-1].open()):
        m = re.search(r"(neighbor_\w+|search_select_kernel)(<[^>]*>)?", row["Kernel_Name"])
        if m:
            calls.setdefault(m.group(0), []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    kernels = {}
    for name, spans in calls.items():
        us = [(e - b) / 1e3 for b, e in sorted(spans)]
        h = len(us) // 2
        kernels[name] = {"calls": len(us), "timed_shape_avg_us": round(statistics.mean(us[:h]), 1),
                         "dim64_avg_us": round(statistics.mean(us[h:]), 1)}
    path = Path(out)
    res = json.loads(path.read_text()) if path.exists() else {}
    res["kernel_trace"] = {"source": "rocprofv3 --kernel-trace, a run of its own (--trace-run): 10 calls at the timed "
                                     "shape, then 10 at dim 64", "kernels": kernels}
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res["kernel_trace"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 16)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--block", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--merge-stats", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.merge_stats:
        return merge_stats(args.merge_stats, args.out or "profiles/neighbors/times.json")

    import torch
    import __graft_entry__ as g
    d = g.load_package()
    assert torch.cuda.is_available(), "needs a GPU: a timing taken elsewhere says nothing"
    rows, dim, k, block = args.rows, args.dim, args.k, args.block
    gen = torch.Generator(device="cuda").manual_seed(0)

    def make_store(dm):
        x = torch.randn(rows, dm, device="cuda", generator=gen)
        codes, scales, zps = d.compress_vectors(x, 8)
        return codes, scales, zps

    codes, scales, zps = make_store(dim)
    pairs = d.neighbor_table(codes, scales, zps)
    stab = d.search_table(codes, scales, zps)
    turn = [0]

    def nxt():
        turn[0] = (turn[0] + block) % (rows - block + 1)
        return turn[0]

    def new_arm(r0=None, c=codes, p=pairs):
        r0 = nxt() if r0 is None else r0
        return d.neighbor_rows(c[r0:r0 + block], None, None, c, None, None, k, self_base=r0, qtable=p[r0:r0 + block], table=p)

    def old_arm(r0=None):
        r0 = nxt() if r0 is None else r0
        Q = d.decompress_vectors(codes[r0:r0 + block], scales[r0:r0 + block], zps[r0:r0 + block])
        return d.search_vectors(Q, codes, scales, zps, k + 1, table=stab)

    if args.trace_run:
        small = make_store(64)
        psmall = d.neighbor_table(*small)
        for _ in range(10):
            new_arm()
        for _ in range(10):
            new_arm(c=small[0], p=psmall)
        torch.cuda.synchronize()
        return

    # what the arms compute, before they are timed: the share of query rows with the same id list
    agree = total = 0
    for r0 in (0, rows // 2, rows - block):
        a = new_arm(r0)[0].cpu().tolist()
        b = old_arm(r0)[0].cpu().tolist()
        for j in range(block):
            total += 1
            agree += a[j] == [t for t in b[j] if t != r0 + j][:k]
    ops = {"neighbor_rows": new_arm, "decompress_then_search_vectors": old_arm}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in ops.values():
        t0 = time.time()
        while time.time() - t0 < 0.3:
            fn()
        torch.cuda.synchronize()
    times = {name: [] for name in ops}
    for _ in range(args.rounds):
        for name, fn in ops.items():
            a.record()
            for _ in range(args.reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) / args.reps * 1e3)

    res = {"rows": rows, "dim": dim, "k": k, "block": block, "rounds": args.rounds, "reps": args.reps, "bits": 8,
           "us_per_call": {n: [round(t, 1) for t in ts] for n, ts in times.items()}, "us": {}}
    for name, ts in times.items():
        res["us"][name] = {"median": round(statistics.median(ts), 1), "min": round(min(ts), 1), "max": round(max(ts), 1)}
    new, old = times["neighbor_rows"], times["decompress_then_search_vectors"]
    res["every_new_round_below_every_baseline_round"] = max(new) < min(old)
    res["baseline_over_new_median"] = round(statistics.median(old) / statistics.median(new), 2)
    res["pairs_per_call"] = block * rows
    res["G_pairs_per_s"] = round(block * rows / statistics.median(new) / 1e3, 1)
    res["G_int8_mac_per_s"] = round(block * rows * dim / statistics.median(new) / 1e3, 1)
    res["id_lists_agree_share"] = round(agree / total, 4)
    res["whole_graph_s_estimate"] = round(statistics.median(new) * 1e-6 * rows / block, 3)
    print(json.dumps(res), flush=True)
    if args.out:
        path = Path(args.out)
        prev = json.loads(path.read_text()) if path.exists() else {}
        if "kernel_trace" in prev:
            res["kernel_trace"] = prev["kernel_trace"]
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
