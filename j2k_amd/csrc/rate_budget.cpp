// rate_budget.cpp -- the search of rate_budget.h.
#include "rate_budget.h"

#include <algorithm>
#include <set>

#include "rate_block.h"

namespace j2k_hip {

namespace {
constexpr uint32_t kFan = 16;                 // candidates per stage beyond the bracket's start
constexpr uint32_t kStrides[3] = {256, 16, 1}; // 16 x 256 = 4096 = kSlopeKMax - kSlopeAll

// One walk along the grid on exact lengths: from `c` finer while c - 1 also fits, or coarser until something fits.
struct Walker {
    int32_t c = kSlopeAll;
    int dir = 0;
    bool done = false, over = false;
};

// missing(c): true when a length the value at c needs is not known yet (it has been put on the list to price);
// value(c): that value, from known lengths.  Returns when the walk has ended or has to wait for prices.
template <class Missing, class Value> void advance(Walker &w, uint64_t limit, Missing &&missing, Value &&value)
{
    while (!w.done) {
        if (missing(w.c)) return;
        if (w.dir == 0) w.dir = value(w.c) <= limit ? -1 : 1;
        if (w.dir < 0) {
            if (w.c == kSlopeAll) { w.done = true; break; }
            if (missing(w.c - 1)) return;
            if (value(w.c - 1) <= limit) --w.c;
            else w.done = true;
        } else {
            if (value(w.c) <= limit) { w.done = true; break; }
            if (w.c == kSlopeKMax) { w.over = w.done = true; break; }
            ++w.c;
        }
    }
}
} // namespace

void BudgetSearch::price(const std::vector<std::pair<uint32_t, int32_t>> &want)
{
    std::set<std::pair<uint32_t, int32_t>> todo;
    for (const auto &w : want)
        if (!known.count(w)) todo.insert(w);
    if (todo.empty()) return;
    std::vector<uint32_t> fr;
    std::vector<int32_t> ix;
    for (const auto &w : todo) { fr.push_back(w.first); ix.push_back(w.second); }
    std::vector<uint64_t> ln(fr.size());
    px.lengths(fr.data(), ix.data(), (uint32_t)fr.size(), ln.data());
    for (size_t i = 0; i < fr.size(); ++i) known[{fr[i], ix[i]}] = ln[i];
    priced += (uint32_t)fr.size();
}

uint64_t BudgetSearch::estimate(uint32_t f, const uint64_t *s) const
{
    const int64_t e = (int64_t)(s[0] + (s[1] + 7) / 8 + cv.fixed_bytes(f)) + adj[f];
    return e > 0 ? (uint64_t)e : 0;
}

void BudgetSearch::launch(int32_t base, uint32_t step, uint32_t K, const std::vector<int32_t> &cap, std::vector<uint64_t> &sums)
{
    sums.assign((size_t)F * K * 2, 0);
    cv.curve(base, step, K, cap.data(), sums.data());
    ++launches;
}

// Per frame the first candidate whose estimate fits `limit`: one launch at stride 256 for all, then one per distinct bracket.
std::vector<int32_t> BudgetSearch::descend_caps(uint64_t limit, std::vector<uint64_t> *est_at)
{
    const std::vector<int32_t> none(F, kSlopeAll);
    std::vector<int32_t> at(F, kSlopeAll); // the bracket's start; in the end the index
    std::vector<bool> closed(F, false);
    est_at->assign(F, 0);
    std::vector<uint64_t> sums;
    for (int stage = 0; stage < 3; ++stage) {
        const uint32_t step = kStrides[stage], K = kFan + 1;
        std::set<int32_t> bases;
        for (uint32_t f = 0; f < F; ++f)
            if (!closed[f]) bases.insert(at[f]);
        for (int32_t base : bases) {
            launch(base, step, K, none, sums);
            for (uint32_t f = 0; f < F; ++f) {
                if (closed[f] || at[f] != base) continue;
                uint32_t j = stage == 0 ? 0 : 1; // (a later stage's first candidate is the bracket's start: it did not fit)
                while (j < kFan && estimate(f, &sums[((size_t)f * K + j) * 2]) > limit) ++j;
                (*est_at)[f] = estimate(f, &sums[((size_t)f * K + j) * 2]);
                if (stage == 0 && j == 0) { closed[f] = true; continue; } // everything fits
                at[f] = stage < 2 ? base + (int32_t)((j - 1) * step) : base + (int32_t)j;
            }
        }
    }
    return at;
}

// The first shared candidate at which the frames' estimates, each at max(candidate, its cap), fit `limit` together.
int32_t BudgetSearch::descend_shared(uint64_t limit, const std::vector<int32_t> &cap, std::vector<uint64_t> *est_at)
{
    int32_t base = kSlopeAll;
    est_at->assign(F, 0);
    std::vector<uint64_t> sums;
    for (int stage = 0; stage < 3; ++stage) {
        const uint32_t step = kStrides[stage], K = kFan + 1;
        launch(base, step, K, cap, sums);
        auto all = [&](uint32_t j) {
            uint64_t t = 0;
            for (uint32_t f = 0; f < F; ++f) t += estimate(f, &sums[((size_t)f * K + j) * 2]);
            return t;
        };
        uint32_t j = stage == 0 ? 0 : 1;
        while (j < kFan && all(j) > limit) ++j;
        for (uint32_t f = 0; f < F; ++f) (*est_at)[f] = estimate(f, &sums[((size_t)f * K + j) * 2]);
        if (stage == 0 && j == 0) return kSlopeAll;
        base = stage < 2 ? base + (int32_t)((j - 1) * step) : base + (int32_t)j;
    }
    return base;
}

BudgetOutcome BudgetSearch::run(uint64_t total_bytes, uint64_t frame_max_bytes)
{
    BudgetOutcome out;
    out.cap.assign(F, kSlopeAll);
    std::vector<std::pair<uint32_t, int32_t>> want;
    std::vector<uint64_t> est_at;
    bool calibrated = false;
    // what the estimate lacked where it was last compared with a real length; true when that moved
    auto calibrate = [&](const std::vector<int32_t> &at) {
        bool moved = false;
        for (uint32_t f = 0; f < F; ++f) {
            const int64_t a = (int64_t)len(f, at[f]) - ((int64_t)est_at[f] - adj[f]);
            if (a != adj[f]) { adj[f] = a; moved = true; }
        }
        calibrated = true;
        return moved;
    };
    auto finish = [&]() -> BudgetOutcome & {
        out.curve_launches = launches;
        out.exact_plans = priced > F ? priced - F : 0;
        return out;
    };

    // the frames' walks to a boundary of frame_max_bytes, side by side (one list of prices per round); false: overflow
    auto walk_caps = [&](std::vector<Walker> &ws) {
        for (;;) {
            want.clear();
            for (uint32_t f = 0; f < F; ++f)
                advance(ws[f], frame_max_bytes,
                        [&](int32_t c) { if (known.count({f, c})) return false; want.push_back({f, c}); return true; },
                        [&](int32_t c) { return len(f, c); });
            if (want.empty()) break;
            price(want);
        }
        for (uint32_t f = 0; f < F; ++f) {
            if (ws[f].over) {
                out.status = BudgetOutcome::OVER_FRAME; out.over_frame = f; out.smallest = len(f, kSlopeKMax);
                return false;
            }
            out.cap[f] = ws[f].c;
        }
        return true;
    };

    // ---- the caps, frame by frame
    if (frame_max_bytes) {
        std::vector<int32_t> at = descend_caps(frame_max_bytes, &est_at);
        want.clear();
        for (uint32_t f = 0; f < F; ++f) want.push_back({f, at[f]});
        price(want);
        if (calibrate(at)) at = descend_caps(frame_max_bytes, &est_at);
        std::vector<Walker> ws(F);
        for (uint32_t f = 0; f < F; ++f) ws[f].c = at[f];
        if (!walk_caps(ws)) return finish();
    }

    // ---- the shared index
    auto at_shared = [&](int32_t c) {
        std::vector<int32_t> v(F);
        for (uint32_t f = 0; f < F; ++f) v[f] = std::max(c, out.cap[f]);
        return v;
    };
    auto price_shared = [&](int32_t c) {
        want.clear();
        const std::vector<int32_t> v = at_shared(c);
        for (uint32_t f = 0; f < F; ++f) want.push_back({f, v[f]});
        price(want);
    };
    out.shared = kSlopeAll;
    if (total_bytes) {
        int32_t c0 = descend_shared(total_bytes, out.cap, &est_at);
        price_shared(c0);
        if (!calibrated && calibrate(at_shared(c0))) c0 = descend_shared(total_bytes, out.cap, &est_at);
        Walker w;
        w.c = c0;
        for (;;) {
            for (;;) {
                want.clear();
                advance(w, total_bytes,
                        [&](int32_t c) {
                            bool miss = false;
                            for (uint32_t f = 0; f < F; ++f) {
                                const std::pair<uint32_t, int32_t> k{f, std::max(c, out.cap[f])};
                                if (!known.count(k)) { want.push_back(k); miss = true; }
                            }
                            return miss;
                        },
                        [&](int32_t c) {
                            uint64_t t = 0;
                            for (uint32_t f = 0; f < F; ++f) t += len(f, std::max(c, out.cap[f]));
                            return t;
                        });
                if (want.empty()) break;
                price(want);
            }
            if (w.over) {
                out.status = BudgetOutcome::OVER_TOTAL;
                for (uint32_t f = 0; f < F; ++f) out.smallest += len(f, kSlopeKMax);
                return finish();
            }
            // Lengths need not fall with the index: a frame whose cap lies below the shared index may be above frame_max_bytes
            // there.  Its cap then moves up to the next boundary at or above the shared index -- as valid a cap as the one it
            // had -- and the shared walk starts again from where it stands, under the new caps.  Caps only rise: this ends.
            if (!frame_max_bytes) break;
            std::vector<Walker> ws(F);
            bool moved = false;
            for (uint32_t f = 0; f < F; ++f) {
                ws[f].c = out.cap[f]; ws[f].done = true;
                if (out.cap[f] < w.c && len(f, w.c) > frame_max_bytes) { ws[f] = Walker{}; ws[f].c = w.c; ws[f].dir = 1; moved = true; }
            }
            if (!moved) break;
            if (!walk_caps(ws)) return finish();
            const int32_t c = w.c;
            w = Walker{};
            w.c = c;
        }
        out.shared = w.c;
    } else
        price_shared(kSlopeAll);

    out.index = at_shared(out.shared);
    out.len.resize(F);
    for (uint32_t f = 0; f < F; ++f) {
        out.len[f] = len(f, out.index[f]);
        out.total += out.len[f];
        if (out.cap[f] > out.shared) ++out.capped;
    }
    return finish();
}

} // namespace j2k_hip
