"""Device time of the store deduplication (dllm_hash_rows, dllm_dedup_rows, dllm_gather_rows) on the
search record's store, rows x dim codes (default 1 Mi x 768 u8, 0.8 GB), against two yardsticks:

* the hash pass's byte rate next to the nq = 1 scan's (profiles/search/times.json,
  scan_codes_TB_per_s): that kernel makes one read of the same bytes;
* what a user can do today: ``(codes.long() * powers).sum(1)`` on the device (the same wrapping
  sum in int64), the hashes copied to the host and numpy's first-occurrence filter there.

Timed separately: the hash pass; the one-shot filter (which empties its own 2 Mi-slot table inside
the call) on hashes with 0 % duplicates, 50 % with every duplicate far from its original (scattered),
50 % with every duplicate right behind its original (adjacent: the layout the insert kernel's
left-neighbour skip removes), ~100 % (1024 distinct values) and one value repeated (the all-zero
prefill: every thread on one slot); the stateful form on a warm table that has seen every row (no
table init in the call); the gather of the 50 % case; hash + filter + gather chained on one stream,
on stores whose duplicates are scattered.  One process, every arm in
every round (interleaved), 0.2 s warm-up per arm, HIP events around `reps` back-to-back calls straight
into the C-ABI.  The arms that read the codes rotate over `sets` stores, each three times the 256 MiB
Infinity Cache, so the figures are HBM figures.

Usage: python scripts/dedup_time.py [--rows 1048576] [--dim 768] [--rounds 7] [--reps 20] [--sets 2]
                                    [--out profiles/dedup/times.json]"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch-reps", type=int, default=2)
    ap.add_argument("--sets", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import __graft_entry__ as g
    d = g.load_package()
    L = d._lib.load()
    assert torch.cuda.is_available(), "needs a GPU: a timing taken elsewhere says nothing"
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())
    rows, dim = args.rows, args.dim
    gen = torch.Generator(device="cuda").manual_seed(0)

    # stores: random codes, the second half copies of the first half's rows in a random order (50 %
    # duplicates, none next to its original)
    half = rows // 2
    stores = []
    for _ in range(args.sets):
        codes = torch.randint(0, 256, (rows, dim), dtype=torch.uint8, device="cuda", generator=gen)
        codes[rows - half:] = codes[torch.randperm(half, device="cuda", generator=gen)]
        stores.append(codes)
    hashes = torch.empty(rows, dtype=torch.int64, device="cuda")
    keep = torch.empty(rows, dtype=torch.uint8, device="cuda")
    first = torch.empty(rows, dtype=torch.int64, device="cuda")
    kept = torch.empty(rows, dtype=torch.int32, device="cuda")
    n_kept = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.empty(rows, dim, dtype=torch.uint8, device="cuda")
    wsb = L.dllm_dedup_workspace(rows)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")

    uniq = torch.randint(-2 ** 62, 2 ** 62, (rows,), dtype=torch.int64, device="cuda", generator=gen)
    idx = torch.arange(rows, device="cuda")
    scattered = uniq.clone()
    scattered[rows - half:] = uniq[torch.randperm(half, device="cuda", generator=gen)]
    hsets = {"dup_0": uniq.clone(), "dup_50": scattered, "dup_50_adjacent": uniq[idx // 2].clone(),
             "dup_100": uniq[idx % 1024].clone(), "one_value": torch.zeros(rows, dtype=torch.int64, device="cuda")}
    # the stateful form: a table that has seen every row of dup_0 once; each timed call offers them again
    slots = 4
    while slots < 4 * rows:
        slots *= 2
    table = torch.empty(L.dllm_dedup_table_bytes(slots) // 8, dtype=torch.int64, device="cuda")
    turn = [0]

    def nxt():
        turn[0] = (turn[0] + 1) % args.sets
        return stores[turn[0]]

    def hash_pass(codes=None, into=hashes):
        assert L.dllm_hash_rows(P(codes if codes is not None else nxt()), rows, dim, dim, P(into), st) == 0

    def filt(h):
        assert L.dllm_dedup_rows(P(h), rows, 0, None, 0, P(keep), P(first), P(kept), P(n_kept), P(ws), wsb, st) == 0

    def filt_warm():
        assert L.dllm_dedup_rows(P(hsets["dup_0"]), rows, rows, P(table), slots, P(keep), P(first), P(kept), P(n_kept),
                                 P(ws), wsb, st) == 0

    def gather(codes=None):
        assert L.dllm_gather_rows(P(codes if codes is not None else nxt()), dim, dim, P(kept50), P(n50), P(out), dim, st) == 0

    def chained():
        codes = nxt()
        hash_pass(codes)
        filt(hashes)
        assert L.dllm_gather_rows(P(codes), dim, dim, P(kept), P(n_kept), P(out), dim, st) == 0

    powers = None

    def torch_hash(codes=None):
        return (codes if codes is not None else nxt()).long().mul_(powers).sum(1)

    def torch_arm():
        h = torch_hash().cpu().numpy()
        _, where = np.unique(h, return_index=True)        # first occurrences, on the host
        k = np.zeros(rows, bool)
        k[where] = True
        return k

    # what the arms compute, checked before they are timed
    p = np.ones(dim, np.uint64)
    with np.errstate(over="ignore"):
        p[1:] = np.cumprod(np.full(dim - 1, 31, np.uint64))
    powers = torch.tensor(p[::-1].copy().view(np.int64), device="cuda")
    hash_pass(stores[0])
    assert torch.equal(hashes, torch_hash(stores[0])), "the two hashes differ"
    filt(hsets["dup_50"])
    kept50, n50 = kept.clone(), n_kept.clone()
    torch.cuda.synchronize()
    counts = {}
    for name, h in hsets.items():
        filt(h)
        counts[name] = int(n_kept.item())
    assert counts["dup_0"] == rows and counts["dup_50"] == rows - half == counts["dup_50_adjacent"]
    assert counts["one_value"] == 1
    assert L.dllm_dedup_table_init(P(table), slots, st) == 0
    assert L.dllm_dedup_rows(P(hsets["dup_0"]), rows, 0, P(table), slots, P(keep), P(first), P(kept), P(n_kept),
                             P(ws), wsb, st) == 0
    assert int(n_kept.item()) == rows
    filt_warm()          # base stays at `rows` in every timed call: every row is a duplicate, nothing is stored
    assert int(n_kept.item()) == 0
    counts["warm_table"] = 0

    ops = {"hash": (hash_pass, args.reps), "gather_50": (gather, args.reps), "chained_50": (chained, args.reps),
           "torch_hash": (torch_hash, args.torch_reps)}
    for name, h in hsets.items():
        ops["filter_" + name] = ((lambda h=h: filt(h)), args.reps)
    ops["filter_warm_table"] = (filt_warm, args.reps)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn, _ in ops.values():
        t0 = time.time()
        while time.time() - t0 < 0.2:
            fn()
        torch.cuda.synchronize()
    times = {name: [] for name in ops}
    times["torch_hash_copy_host_filter_wall"] = []
    for _ in range(args.rounds):
        for name, (fn, reps) in ops.items():
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b) / reps * 1e3)
        t0 = time.perf_counter()                         # host work included: wall time, synchronous by its .cpu()
        torch_arm()
        times["torch_hash_copy_host_filter_wall"].append((time.perf_counter() - t0) * 1e6)

    res = {"rows": rows, "dim": dim, "rounds": args.rounds, "reps": args.reps, "sets": args.sets,
           "store_bytes": rows * dim, "kept": counts, "us": {}}
    for name, ts in times.items():
        res["us"][name] = {"median": round(statistics.median(ts), 1), "min": round(min(ts), 1), "max": round(max(ts), 1)}
    med = lambda n: res["us"][n]["median"]
    res["hash_TB_per_s"] = round(rows * dim / (med("hash") * 1e-6) / 1e12, 3)
    for name in list(hsets) + ["warm_table"]:
        res["filter_%s_Mrows_per_s" % name] = round(rows / med("filter_" + name), 1)
    res["gather_50_TB_per_s_read_plus_written"] = round(2 * counts["dup_50"] * dim / (med("gather_50") * 1e-6) / 1e12, 3)
    res["torch_hash_over_hash"] = round(med("torch_hash") / med("hash"), 1)
    res["torch_arm_wall_over_chained"] = round(med("torch_hash_copy_host_filter_wall") / med("chained_50"), 1)
    ref = ROOT / "profiles" / "search" / "times.json"
    if ref.exists():
        scan = [c for c in json.loads(ref.read_text())["cases"] if c["nq"] == 1][0].get("scan_codes_TB_per_s")
        if scan:
            res["search_scan_nq1_TB_per_s"] = scan
            res["hash_rate_over_scan_rate"] = round(res["hash_TB_per_s"] / scan, 3)
    print(json.dumps(res), flush=True)
    if args.out:
        out_path = Path(args.out)
        out_path.parent.mkdir(parents=True, exist_ok=True)
        out_path.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
