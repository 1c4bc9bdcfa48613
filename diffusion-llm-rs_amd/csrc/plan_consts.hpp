// plan_consts.hpp -- the constants the kernels share with the host-side kernel selection
// (linear_plan.hpp).  Standard C++ only: included by common.hpp for the device translation units and
// by linear_plan.hpp for the host-only one, so each value is defined once.
#pragma once

#include <cstddef>

namespace dllm {

constexpr int kWave = 64;      // CDNA wavefront width
constexpr int kCUs = 256;      // MI355X compute units (8 XCDs x 32)
constexpr int kXCDs = 8;

// Linear layer: Npad is a multiple of kBN columns, K of the kBK-deep k-step (one LDS stage).
constexpr int kBN = 128, kBK = 64;

// Decode GEMM (wq_decode_kernel): waves per block, and the largest M it takes.
constexpr int kDecWaves = 8;
constexpr int kDecodeMaxM = 64;

// XL decode (M <= 16): dynamic LDS of X rows + zero row (2K + 16 B each) + pair and scale rows
// (256 B per 4 groups each), within the CU's 160 KiB beside the 8 KiB partial-sum buffer.
constexpr size_t kXlLdsMax = 160 * 1024 - kDecWaves * 64 * 4 * 4;

}  // namespace dllm
