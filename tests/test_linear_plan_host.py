"""The linear layer's kernel selection is host-only: tests/cpp/plan_host_check.cpp and
csrc/linear_plan.cpp alone compile and link with g++ (no hipcc, no library) and the check's boundary
sweep runs clean under the address and undefined-behaviour sanitizers."""
from tests.host_check import run_host_check


def test_plan_module_links_and_sweeps_with_gxx(tmp_path):
    run_host_check("plan_host_check", tmp_path, sources=("linear_plan.cpp",), timeout=120)
