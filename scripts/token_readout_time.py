"""Device time of the token readout (dllm_token_readout) at the real vocabulary, V = 50257, for
M in {1, 64, 2048} rows of f16 and f32 logits, against two baselines: the logits' bytes over the HBM
peak (8.0 TB/s spec; 6.3 TB/s is what a float4 copy reaches on this part), and torch.softmax(dim=-1)
followed by torch.argmax on the same logits -- what a caller had before.

Arms, interleaved in every round of one process: `readout` (tokens + stats, one read of the logits),
`readout_probs` (the same plus the probabilities), `torch` (softmax + argmax).  The readout runs on
two layouts: `dense` (ld = V: odd, so rows start off 16-byte alignment and groups of four straddle
cache lines; what a QuantLinear with N = V writes) and `padded` (ld = 50260: every group aligned).  0.2 s warm-up per
arm, HIP events around `reps` back-to-back calls straight into the C-ABI.  Every arm rotates over
enough buffer sets that the bytes between two uses of a line exceed the 256 MiB Infinity Cache where
that takes at most `max_sets` sets; at M = 1 (a 100-200 KB row) it cannot, and the figures there are
launch-latency figures, not HBM figures.

Usage: python scripts/token_readout_time.py [--rounds 7] [--reps 20] [--out profiles/token_readout/times.json]"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

V = 50257
LD_PADDED = 50260
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--max-sets", type=int, default=96)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import __graft_entry__ as g
    d = g.load_package()
    L = d._lib.load()
    assert torch.cuda.is_available(), "needs a GPU: a timing taken elsewhere says nothing"
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P = lambda t: C.c_void_p(t.data_ptr())
    results = []
    for dtype, code, esize in ((torch.float16, 1, 2), (torch.float32, 0, 4)):
        for M in (1, 64, 2048):
            nbytes = M * V * esize
            sets = max(2, min(args.max_sets, -(-(512 << 20) // nbytes)))
            gen = torch.Generator(device="cuda").manual_seed(M)
            padded = [(2.0 * torch.randn(M, LD_PADDED, device="cuda", generator=gen)).to(dtype) for _ in range(sets)]
            dense = [p[:, :V].contiguous() for p in padded]
            tokens = torch.empty(M, dtype=torch.int32, device="cuda")
            stats = torch.empty(M, 2, device="cuda")
            probs = torch.empty(M, V, device="cuda")
            wsb = L.dllm_token_readout_workspace(M, V)
            ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
            k = [0]

            def nxt(bufs):
                k[0] = (k[0] + 1) % sets
                return bufs[k[0]]

            def readout(bufs, ld, with_probs):
                rc = L.dllm_token_readout(P(nxt(bufs)), code, M, V, ld, P(tokens), P(stats),
                                          P(probs) if with_probs else None, P(ws), wsb, st)
                assert rc == 0

            def torch_arm():
                x = nxt(dense)
                p = torch.softmax(x, dim=-1)
                return p, torch.argmax(x, dim=-1)

            ops = {"readout_dense": lambda: readout(dense, V, False),
                   "readout_padded": lambda: readout(padded, LD_PADDED, False),
                   "readout_probs_dense": lambda: readout(dense, V, True),
                   "readout_probs_padded": lambda: readout(padded, LD_PADDED, True),
                   "torch_softmax_argmax": torch_arm}
            # the arms compute the same thing: greedy tokens agree where the row has no tie
            readout(dense, V, False)
            want = torch.argmax(dense[k[0]], dim=-1)
            torch.cuda.synchronize()
            agree = float((tokens.long() == want).float().mean())
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
            row = {"M": M, "V": V, "dtype": "f16" if code else "f32", "logits_bytes": nbytes, "sets": sets,
                   "rounds": args.rounds, "reps": args.reps, "hbm_peak_floor_us": round(nbytes / HBM_PEAK * 1e6, 2),
                   "tokens_agree_with_torch_argmax": agree}
            for name, ts in times.items():
                med = statistics.median(ts)
                row[name] = {"median_us": round(med, 2), "min_us": round(min(ts), 2), "max_us": round(max(ts), 2)}
                if name.startswith("readout") and "probs" not in name:
                    row[name]["logits_TB_per_s"] = round(nbytes / (med * 1e-6) / 1e12, 3)
            for name in ("readout_dense", "readout_padded", "readout_probs_dense", "readout_probs_padded"):
                row[name]["torch_over_this"] = round(row["torch_softmax_argmax"]["median_us"] / row[name]["median_us"], 2)
            print(json.dumps(row), flush=True)
            results.append(row)
            del padded, dense, probs
            torch.cuda.empty_cache()
    if args.out:
        out = Path(args.out)
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(json.dumps(results, indent=1) + "\n")


if __name__ == "__main__":
    main()
