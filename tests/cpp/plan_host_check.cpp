// The linear layer's kernel selection (csrc/linear_plan.cpp) called directly: no library, no HIP,
// no Python.  Built by tests/test_linear_plan_host.py with g++ and the address / undefined-behaviour
// sanitizers against linear_plan.cpp alone; that it links is the proof that the module is host-only.
//
// Walks the anchor shapes of tests/test_linear_plan_cpu.py and M +- 1 around every multiple of 32
// (hence of 64 and 128) up to 8200 at K = 4096, N in {512, 1024, 2048, 4096, 32768}, for every code
// width, group, precision, Horner validity and layout flag, and asserts the invariants that need no
// library.  Cross-product invariants (coverage of the GPU test matrix) stay in the Python test.
#include <cstdio>
#include <initializer_list>
#include <set>

#include "linear_plan.hpp"

using namespace dllm;

static long g_checked = 0, g_failed = 0;

static void check_one(size_t K, size_t N, int bits, size_t group, int flags, int horner_ok, size_t M) {
    const PlanError se = check_shape(K, N, static_cast<uint8_t>(bits), group, flags);
    const PlanError ae = check_plan_args(N, M, 0);
    if (se.code != DLLM_OK || ae.code != DLLM_OK) {
        std::printf("FAIL arguments rejected: K %zu N %zu bits %d group %zu flags %d M %zu: %s\n", K, N, bits, group,
                    flags, M, se.code ? se.msg : ae.msg);
        ++g_failed;
        return;
    }
    const PlanShape s = plan_shape_for(K, N, static_cast<uint8_t>(bits), group, flags, horner_ok);
    dllm_linear_plan_t p{};
    select_plan(&s, M, 0, &p);
    const bool tiles_npad = p.tile_n > 0 && s.Npad % static_cast<size_t>(p.tile_n) == 0;
    const bool decode_iff = (p.kernel == DLLM_KERNEL_DECODE) == (M <= 64 && s.decode_layout);
    const bool splitk_iff = ((p.flags & DLLM_PLAN_SPLITK) != 0) == (p.nsplit > 1);
    ++g_checked;
    if (tiles_npad && decode_iff && splitk_iff) return;
    ++g_failed;
    std::printf("FAIL K %zu N %zu bits %d group %zu flags %d horner_ok %d M %zu -> kernel %d tile %d x %d kgroups %d "
                "nsplit %d flags %d (%s%s%s)\n", K, N, bits, group, flags, horner_ok, M, p.kernel, p.tile_m, p.tile_n,
                p.kgroups, p.nsplit, p.flags, tiles_npad ? "" : " Npad % tile_n", decode_iff ? "" : " decode iff M <= 64",
                splitk_iff ? "" : " SPLITK iff nsplit > 1");
}

int main() {
    // (M, K, N, bits, horner_ok) of ANCHORS in tests/test_linear_plan_cpu.py; int4 / int2 g128 EXACT
    static const size_t anchors[][5] = {
        {4096, 4096, 4096, 4, 1}, {4096, 4096, 4096, 2, 1}, {8000, 4096, 4096, 4, 1}, {3001, 4096, 4096, 4, 1},
        {2048, 4096, 4096, 4, 1}, {1800, 4096, 4096, 4, 1}, {4300, 4096, 4096, 4, 1}, {4096, 4096, 2048, 4, 1},
        {4096, 4096, 1024, 4, 1}, {1024, 4096, 4096, 4, 1}, {700, 4096, 4096, 4, 1},  {512, 4096, 4096, 4, 1},
        {384, 4096, 4096, 4, 1},  {4096, 4096, 512, 4, 1},  {256, 4096, 4096, 4, 1},  {65, 4096, 4096, 4, 1},
        {2048, 4096, 4096, 2, 1}, {4096, 4096, 4096, 4, 0}, {384, 4096, 4096, 4, 0},  {100, 512, 32768, 4, 1},
    };
    for (const auto &a : anchors)
        check_one(a[1], a[2], static_cast<int>(a[3]), 128, DLLM_PRECISION_EXACT, static_cast<int>(a[4]), a[0]);

    std::set<size_t> ms;
    for (size_t b = 32; b <= 8200; b += 32)
        for (size_t m : {b - 1, b, b + 1})
            if (m <= 8200) ms.insert(m);
    const size_t ns[] = {512, 1024, 2048, 4096, 32768};
    for (size_t N : ns)
        for (int bits : {2, 4, 8})
            for (size_t group : {64, 128, 256})
                for (int precision : {int(DLLM_PRECISION_EXACT), int(DLLM_PRECISION_F16W)})
                    for (int prefill_only : {0, int(DLLM_LINEAR_PREFILL_ONLY)})
                        for (int horner_ok : {1, 0})
                            for (size_t M : ms) check_one(4096, N, bits, group, precision | prefill_only, horner_ok, M);

    std::printf("%ld plans checked, %ld failed\n", g_checked, g_failed);
    return g_failed == 0 && g_checked > 100000 ? 0 : 1;
}
