"""The one recipe for the stand-alone host checks: tests/cpp/<name>.cpp (its own main) with the HIP-free
modules of csrc, compiled by g++ alone under the address and undefined-behaviour sanitizers and run on
the CPU.  No hipcc, no include path into ROCm and no library: that it links is the proof that the
modules are host-only."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "diffusion-llm-rs_amd" / "csrc"
RULES = ("host_rules.cpp", "error.cpp")   # the *_host mirrors of 8g - 8l and dllm_last_error


def run_host_check(name, tmp_path, sources=RULES, timeout=300):
    """Builds tests/cpp/<name>.cpp with csrc's `sources`, runs it and asserts a clean exit with "0 failed"."""
    exe = tmp_path / name
    # the sanitizer runtimes linked statically: the program runs as it is, in any environment
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                    "-static-libubsan", f"-I{ROOT / 'include'}", f"-I{CSRC}", str(ROOT / "tests" / "cpp" / f"{name}.cpp"),
                    *(str(CSRC / s) for s in sources), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=timeout)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failed" in r.stdout
