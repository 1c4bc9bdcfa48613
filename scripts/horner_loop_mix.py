"""Instruction mix of the main loop of a wq_horner16_kernel instance, from the device assembly hipcc
writes with ``--cuda-device-only -S`` (the Makefile's flags for linear_horner.hip).  The main loop is
the backward branch that encloses the most MFMAs; on the 4-slot ring it holds two k-steps (one group,
one s_barrier each), so the counts are printed per loop body and per k-step.  The counts are static:
with the skew the body holds the second half k-step twice (waves 0-3 run it behind the first half,
waves 4-7 in front of it: 96 MFMAs per k-step in the code, 64 executed), while the weight words, the
dequant and the rescale sit in the first half that every wave runs once.  No GPU needed.

Usage: python scripts/horner_loop_mix.py FILE.s [substring of the kernel's mangled name ...]"""
import collections
import json
import re
import sys

# (mnemonic prefixes: the assembler's _e32 / _e64 encodings count together)
WATCH = ("v_mfma_f32_16x16x32_f16", "v_permlane16_swap_b32", "ds_read2_b32", "ds_read_b128", "v_mul_f32",
         "v_and_or_b32", "v_pk_add_f16", "v_lshrrev_b32", "s_barrier")


def functions(text):
    """name -> list of lines of every kernel body in the file."""
    out, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name is not None:
            if line.startswith("\t.end_amdhsa_kernel") or line.startswith(".Lfunc_end"):
                name = None
            else:
                out[name].append(line)
    return out


def main_loop(lines):
    """(first, last) line indices of the backward branch whose body holds the most MFMAs."""
    labels = {m.group(1): i for i, l in enumerate(lines) if (m := re.match(r"^(\.LBB\w+):", l))}
    best = None
    for i, l in enumerate(lines):
        m = re.match(r"\s+s_cbranch_\w+\s+(\.LBB\w+)", l) or re.match(r"\s+s_branch\s+(\.LBB\w+)", l)
        if not m or labels.get(m.group(1), i) >= i:
            continue
        lo = labels[m.group(1)]
        n = sum("v_mfma" in x for x in lines[lo:i])
        if best is None or n > best[0]:
            best = (n, lo, i)
    return best[1], best[2]


def mix(lines):
    lo, hi = main_loop(lines)
    ops = collections.Counter(l.split()[0] for l in lines[lo:hi] if l.startswith("\t") and not l.startswith("\t."))
    ksteps = ops["s_barrier"] or 1
    valu = sum(n for op, n in ops.items() if op.startswith("v_") and not op.startswith("v_mfma"))
    body = {w: sum(n for op, n in ops.items() if op.startswith(w)) for w in WATCH}
    body["valu_without_mfma"] = valu
    return {"k_steps_in_loop": ksteps, "loop_body": body, "per_k_step": {k: v / ksteps for k, v in body.items()}}


if __name__ == "__main__":
    fns = functions(open(sys.argv[1]).read())
    for name, lines in fns.items():
        if "wq_horner16_kernel" in name and all(s in name for s in sys.argv[2:]):
            print(json.dumps({"kernel": name, **mix(lines)}))
