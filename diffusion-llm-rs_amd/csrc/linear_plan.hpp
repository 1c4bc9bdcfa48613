// linear_plan.hpp -- the kernel selection of the linear layer: which of the kernel families and
// tile classes a (layer, M) runs.  dllm_linear_plan(_shape) report select_plan's answer and the
// launchers of linear_wq.hip / linear_exact.hip switch on it.  Host integer arithmetic only: this
// header and linear_plan.cpp include dllm_quant.h and the C++ standard library, nothing from HIP
// (tests/cpp/plan_host_check.cpp links the module with g++ alone).
#pragma once

#include <cstddef>
#include <cstdint>

#include "dllm_quant.h"
#include "plan_consts.hpp"

#ifndef DLLM_LAB
#define DLLM_LAB 0
#endif

#pragma GCC visibility push(hidden)   // internal to the library, as the launchers that call it
namespace dllm {

// What the kernel selection reads of a layer: a handle's facts (plan_shape_of, linear_wq.hip) or the
// arguments of dllm_linear_plan_shape (plan_shape_for).  horner_ok = the create's check of the Horner
// ratios passed (hstate == 1).
struct PlanShape {
    size_t K = 0, N = 0, Npad = 0, group = 0;
    int bits = 0, precision = DLLM_PRECISION_EXACT;
    bool horner_ok = false, decode_layout = false;
#if DLLM_LAB
    int variant = -1;   // lab A/B: the handle's schedule variant
#endif
};

// A failed argument check: the DLLM_ERR_* code and the text for dllm_last_error() (code == DLLM_OK:
// passed).  The C API hands both to fail().
struct PlanError {
    int code = DLLM_OK;
    const char *msg = nullptr;
};
// The layer arguments of create and dllm_linear_plan_shape (`flags`: precision | DLLM_LINEAR_PREFILL_ONLY).
PlanError check_shape(size_t K, size_t N, uint8_t bits, size_t group, int flags);
// The call arguments of dllm_linear_plan and dllm_linear_plan_shape.
PlanError check_plan_args(size_t N, size_t M, int fused);
// The shape of a layer created with these (checked) arguments.
PlanShape plan_shape_for(size_t K, size_t N, uint8_t bits, size_t group, int flags, int horner_ok);

bool exact_gemm_supported(int M, int K, int Npad, int group);
bool use_exact(const PlanShape *h);
bool horner_shape(const PlanShape *h);
size_t xl_lds_bytes(int M, int K, int group);

// The plan of one (layer, M); `fused`: of dllm_linear_forward_psample(_ex).
void select_plan(const PlanShape *h, size_t M, int fused, dllm_linear_plan_t *p);
// Its parts, for the launchers that re-plan under a lab override or switch on one family.
void decode_plan(const PlanShape *h, int M, dllm_linear_plan_t *p, int nt0 = 0, int nsplit0 = 0);
void rounded_plan(const PlanShape *h, int M, dllm_linear_plan_t *p);
void exact_plan(int bits, int M, int K, int Npad, int group, dllm_linear_plan_t *p);

// Tile counts of the fold-form grids and the thresholds exact_plan decides by (the lab launcher of
// linear_exact.hip asks the same questions).
struct ExactGrids {
    int tiles, t64, t32;   // 128 x 128, 64 x 128 and 32 x 128 tiles
    int ngroups;           // K / group
    bool full256;          // 128 x 256 tiles fill a round
    bool mid;              // mid M: the 32 x 128 tiles' range (int4 g128 only)
    bool one_round;        // 128 x 128 tiles give one to two rounds and K halves by groups
};
ExactGrids exact_grids(int M, int K, int Npad, int group);
// K slices of the 64 x 128 one-k-group tiles on a grid short of two rounds.
int exact_split64(const ExactGrids &g, int K);

#if DLLM_LAB
bool lab_horner128();                             // DLLM_LAB_HORNER128 set: Horner form on 128 x 256 tiles
int horner_rows(const PlanShape *hc, int M);      // variant 323: the Horner kernel's 128-row tiles
#endif

}  // namespace dllm
#pragma GCC visibility pop
