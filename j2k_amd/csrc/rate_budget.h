// rate_budget.h -- a sequence to a byte budget (j2k_hip.h: j2k_hip_encode_sequence_budget_device): the
// search for the per-frame caps and the shared index on the public slope grid (rate_block.h: rate_slope_grid).  Host only and
// free of the device: it sees the call through two interfaces -- the rate curve (in the library: rate_curve_kernel) and the exact
// price of a frame at an index (in the library: the cut and the packet planner) -- and under test both are CPU stand-ins.
//
// The curve gives an estimate, body + ceil(header bits / 8) + fixed bytes of the frame (+ what the first exact prices showed
// the estimate to lack), and a K-ary descent over it proposes an index: three launches at strides 256, 16 and 1 cover the
// 4097 candidates.  Nothing depends on the estimate for correctness: every boundary is established by the exact walk, which
// moves one way, one index at a time, on real lengths, and ends at an index c that fits while c - 1 does not (or c = ALL), or
// past the coarsest candidate with an overflow.
#pragma once

#include <cstdint>
#include <map>
#include <utility>
#include <vector>

namespace j2k_hip {

struct BudgetCurve {
    virtual ~BudgetCurve() {}
    // sums[(f * K + j) * 2 + {0, 1}] = body bytes, header bits of frame f at max(min(base + j * step, K_MAX), cap[f])
    virtual void curve(int32_t base, uint32_t step, uint32_t K, const int32_t *cap, uint64_t *sums) = 0;
    virtual uint64_t fixed_bytes(uint32_t f) = 0; // of frame f's file whatever the cut: headers, markers, empty packets
};

struct BudgetPricer {
    virtual ~BudgetPricer() {}
    // len[i] = the exact length of frame frames[i]'s file at grid index index[i] (a whole-frame plan each)
    virtual void lengths(const uint32_t *frames, const int32_t *index, uint32_t n, uint64_t *len) = 0;
};

struct BudgetOutcome {
    enum { OK = 0, OVER_TOTAL = 1, OVER_FRAME = 2 } status = OK;
    uint32_t over_frame = 0;       // OVER_FRAME: the frame
    uint64_t smallest = 0;         // on overflow: the length at the coarsest candidate (of that frame, or of all together)
    int32_t shared = 0;            // c*
    std::vector<int32_t> cap;      // cap_f
    std::vector<int32_t> index;    // c_f(c*) = max(c*, cap_f)
    std::vector<uint64_t> len;     // len_f(index[f])
    uint64_t total = 0;
    uint32_t capped = 0;           // frames with cap_f > c*
    uint32_t curve_launches = 0;
    uint32_t exact_plans = 0;      // lengths asked of the pricer beyond one per frame
};

class BudgetSearch {
public:
    BudgetSearch(uint32_t nframes, BudgetCurve &curve, BudgetPricer &pricer) : F(nframes), cv(curve), px(pricer), adj(nframes, 0) {}
    BudgetOutcome run(uint64_t total_bytes, uint64_t frame_max_bytes);

private:
    uint32_t F;
    BudgetCurve &cv;
    BudgetPricer &px;
    std::vector<int64_t> adj; // per frame: exact - estimate where both were last known
    std::map<std::pair<uint32_t, int32_t>, uint64_t> known; // exact lengths by (frame, index)
    uint32_t launches = 0, priced = 0;

    void price(const std::vector<std::pair<uint32_t, int32_t>> &want);
    uint64_t len(uint32_t f, int32_t c) const { return known.at({f, c}); }
    uint64_t estimate(uint32_t f, const uint64_t *s) const;
    void launch(int32_t base, uint32_t step, uint32_t K, const std::vector<int32_t> &cap, std::vector<uint64_t> &sums);
    std::vector<int32_t> descend_caps(uint64_t limit, std::vector<uint64_t> *est_at);
    int32_t descend_shared(uint64_t limit, const std::vector<int32_t> &cap, std::vector<uint64_t> *est_at);
};

} // namespace j2k_hip
