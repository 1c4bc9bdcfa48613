"""Device time of the p_losses reduction (dllm_noise_mse) next to dllm_p_sample on the same element
count, the existing kernel nearest in work (12 B per element + the same generator, against 4-8 B).

B = 1, n = 2048 x 4096 and 4096 x 4096, f32 pred, explicit noise and stream noise.  One process, the
four ops interleaved in every round, 0.2 s warm-up per op, HIP events around `reps` back-to-back
calls straight into the C-ABI.  Every op rotates over `sets` buffer sets so that the bytes between
two uses of a line exceed the 256 MiB Infinity Cache: the figures are HBM figures.

Usage: python scripts/p_losses_time.py [--rounds 10] [--reps 100] [--sets 4] [--out profiles/p_losses/times.json]"""
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
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import __graft_entry__ as g
    d = g.load_package()
    L = d._lib.load()
    assert torch.cuda.is_available(), "needs a GPU: a timing taken elsewhere says nothing"
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())
    coef = torch.tensor([[0.9, 0.1, 0.05]], device="cuda")
    results = []
    for n in (2048 * 4096, 4096 * 4096):
        bufs = [[torch.randn(n, device="cuda") for _ in range(4)] for _ in range(args.sets)]   # pred/x, noise, eps, out
        wsb = L.dllm_noise_mse_workspace(1, n)
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
        loss = torch.empty(4, device="cuda")
        k = [0]

        def nxt():
            k[0] = (k[0] + 1) % args.sets
            return bufs[k[0]]

        def mse(explicit):
            a, z, _, _ = nxt()
            rc = L.dllm_noise_mse(P(a), 0, P(z) if explicit else None, 1, n, 7, 0, P(loss), P(ws), wsb, st)
            assert rc == 0

        def psample(explicit):
            a, z, e, o = nxt()
            rc = L.dllm_p_sample(P(a), P(e), P(z) if explicit else None, P(coef), 1, n, 1, 7, 0, P(o), st)
            assert rc == 0

        ops = {"noise_mse_explicit": lambda: mse(True), "p_sample_explicit": lambda: psample(True),
               "noise_mse_stream": lambda: mse(False), "p_sample_stream": lambda: psample(False)}
        for fn in ops.values():
            t0 = time.time()
            while time.time() - t0 < 0.2:
                fn()
            torch.cuda.synchronize()
        times = {name: [] for name in ops}
        for _ in range(args.rounds):
            for name, fn in ops.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.reps):
                    fn()
                b.record()
                torch.cuda.synchronize()
                times[name].append(a.elapsed_time(b) / args.reps * 1e3)
        row = {"n": n, "rounds": args.rounds, "reps": args.reps, "sets": args.sets}
        for name, ts in times.items():
            row[name] = {"median_us": round(statistics.median(ts), 2), "min_us": round(min(ts), 2),
                         "max_us": round(max(ts), 2)}
        row["noise_mse_explicit"]["TB_per_s"] = round(8 * n / (row["noise_mse_explicit"]["median_us"] * 1e-6) / 1e12, 3)
        for kind in ("explicit", "stream"):
            ps, ms = row[f"p_sample_{kind}"], row[f"noise_mse_{kind}"]
            spread = ps["max_us"] - ps["min_us"]
            row[f"{kind}_p_sample_spread_us"] = round(spread, 2)
            row[f"{kind}_within_expectation"] = bool(ms["median_us"] <= ps["median_us"] + 3 * spread)
        print(json.dumps(row), flush=True)
        results.append(row)
        del bufs
    if args.out:
        out = Path(args.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
