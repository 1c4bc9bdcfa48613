// dedup_mirror_check.cpp -- a stand-alone driver (its own main) of the C++ mirror's
// dllm::io_dedup::DedupBuffer (include/dllm_quant.hpp): compute_hash on known values, the reference's
// collision rule, and a second call on the same buffer.  Host entry points only; no device.
#include <cstdio>

#include "dllm_quant.hpp"

static int failed = 0, checked = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        ++checked;                                                    \
        if (!(cond)) {                                                \
            ++failed;                                                 \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                             \
    } while (0)

int main() {
    using dllm::diffusion_prefill::CompressedVector;
    using dllm::io_dedup::DedupBuffer;
    CHECK(DedupBuffer::compute_hash({}) == 0);
    CHECK(DedupBuffer::compute_hash({7}) == 7);
    CHECK(DedupBuffer::compute_hash({1, 0, 0}) == 961);
    CHECK(DedupBuffer::compute_hash({1, 31}) == 62 && DedupBuffer::compute_hash({2, 0}) == 62);
    CHECK(DedupBuffer::compute_hash(std::vector<uint8_t>(768, 0)) == 0);

    auto rec = [](const char *id, std::vector<uint8_t> data) {
        CompressedVector v{};
        v.id = id;
        v.data = std::move(data);
        return v;
    };
    DedupBuffer buf(8);
    // {1, 31} and {2, 0} differ and collide: the later one is dropped, as the reference drops it
    std::vector<CompressedVector> a = {rec("a", {1, 31}), rec("b", {2, 0}), rec("c", {2, 1}), rec("d", {1, 31})};
    auto ua = buf.deduplicate(a);
    CHECK(ua.size() == 2 && ua[0].id == "a" && ua[1].id == "c");
    // a second call on the same buffer: what the first saw stays seen, in whatever order it comes back
    std::vector<CompressedVector> b = {rec("e", {2, 1}), rec("f", {9, 9}), rec("g", {2, 0}), rec("h", {9, 9})};
    auto ub = buf.deduplicate(b);
    CHECK(ub.size() == 1 && ub[0].id == "f" && ub[0].data == std::vector<uint8_t>({9, 9}));
    CHECK(buf.deduplicate({}).empty());
    bool threw = false;
    try {
        buf.deduplicate(a);   // 8 offered + 4 exceeds the capacity of 8
    } catch (const dllm::QuantizationError &) {
        threw = true;
    }
    CHECK(threw);
    // an all-zero prefill: one record survives
    DedupBuffer zeros(96);
    std::vector<CompressedVector> z(48, rec("z", std::vector<uint8_t>(64, 0)));
    CHECK(zeros.deduplicate(z).size() == 1 && zeros.deduplicate(z).empty());
    std::printf("%d checked, %d failed\n", checked, failed);
    return failed ? 1 : 0;
}
