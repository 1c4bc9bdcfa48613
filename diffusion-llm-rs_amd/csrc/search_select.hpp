// search_select.hpp -- the top-k select passes of search.hip (score matrix f32 [nq][rows] -> idx /
// scores [nq][k] by 8g's key), for the other producer of such a matrix: neighbors.hip.
#pragma once

#include "common.hpp"

namespace dllm {

// Bytes of the two candidate-key buffers the passes alternate between (0 when one slice holds a row).
struct SelectPlan {
    size_t keys_a = 0, keys_b = 0;
};
SelectPlan select_plan(size_t nq, size_t rows, size_t k);
// nq * ceil(rows / slice) is the first pass's grid: false when it exceeds the grid limit.
bool select_grid_ok(size_t nq, size_t rows);
// The select passes on `st`.  drop_nan: a NaN score is "no row" (key 0: index -1, score -inf, ranked
// past every row) instead of a row that ranks below -inf.  rows >= 1, 1 <= k <= 256.
int select_topk(const float *sc, size_t nq, size_t rows, size_t k, uint64_t *keys_a, uint64_t *keys_b, int32_t *idx,
                float *scores, bool drop_nan, hipStream_t st);
// idx = -1, scores = -inf for n outputs.
int select_fill_empty(size_t n, int32_t *idx, float *scores, hipStream_t st);

}  // namespace dllm
