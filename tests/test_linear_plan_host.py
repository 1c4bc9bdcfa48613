"""The linear layer's kernel selection is host-only: tests/cpp/plan_host_check.cpp and
csrc/linear_plan.cpp alone compile and link with g++ (no hipcc, no library) and the check's boundary
sweep runs clean under the address and undefined-behaviour sanitizers."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "diffusion-llm-rs_amd" / "csrc"
SRC = ROOT / "tests" / "cpp" / "plan_host_check.cpp"


def test_plan_module_links_and_sweeps_with_gxx(tmp_path):
    exe = tmp_path / "plan_host_check"
    # the sanitizer runtimes linked statically: the program runs as it is, in any environment
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                    f"-I{ROOT / 'include'}", f"-I{CSRC}", str(SRC),
                    str(CSRC / "linear_plan.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failed" in r.stdout
