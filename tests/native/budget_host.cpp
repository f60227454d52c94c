// budget_host.cpp -- the search for a sequence's byte budget (j2k_amd/csrc/rate_budget.h) as a stand-alone host program, built
// with the address and undefined-behaviour sanitizers by tests/test_budget_host.py.  The curve provider is a CPU implementation
// over a case file's pass tables through rate_block.h (what rate_curve_kernel runs per thread); the exact pricer is the
// estimate itself, the estimate plus a constant per frame, or the estimate plus a wobble of +-40 bytes keyed by frame and index.
//   budget_host <case file> [tables]
// prints, for the test to judge against tests/budget_model.py:
//   L f len(ALL) .. len(K_MAX)        with `tables`: the pricer's lengths of frame f at all 4097 candidates
//   C f index body bits               the curve at every 64th candidate
//   R setting run status total frame_max shared launches plans smallest | cap_0 .. cap_F-1 index_0 .. index_F-1
// Every setting is run twice on fresh searches.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../j2k_amd/csrc/rate_block.h"
#include "../../j2k_amd/csrc/rate_budget.h"

using namespace j2k_hip;

namespace {

[[noreturn]] void die(const char *what)
{
    std::fprintf(stderr, "budget_host: %s\n", what);
    std::exit(2);
}

struct Reader {
    FILE *f;
    template <class T> T get()
    {
        T v;
        if (std::fread(&v, sizeof v, 1, f) != 1) die("case file cut short");
        return v;
    }
    template <class T> void get(T *p, size_t n)
    {
        if (n && std::fread(p, sizeof(T), n, f) != n) die("case file cut short");
    }
};

constexpr int kCand = kSlopeKMax - kSlopeAll + 1;
constexpr uint64_t kFixed = 100;

struct Frames {
    uint32_t F = 0, pricer = 0;
    std::vector<uint64_t> body, bits; // [F][kCand]
    uint64_t estimate(uint32_t f, int32_t c) const
    {
        const size_t at = (size_t)f * kCand + (size_t)(c - kSlopeAll);
        return body[at] + (bits[at] + 7) / 8 + kFixed;
    }
    uint64_t price(uint32_t f, int32_t c) const
    {
        const uint64_t e = estimate(f, c);
        if (pricer == 0) return e;
        if (pricer == 1) return e + 1000 + 377 * (uint64_t)f;
        uint32_t h = (uint32_t)f * 2654435761u ^ (uint32_t)(c - kSlopeAll) * 40503u;
        h ^= h >> 13; h *= 2246822519u; h ^= h >> 16;
        return e + 40 + (uint64_t)(h % 81) - 40; // (e + [0, 80]: a wobble of +-40 about e + 40)
    }
};

struct CpuCurve : BudgetCurve {
    const Frames &fr;
    explicit CpuCurve(const Frames &f) : fr(f) {}
    void curve(int32_t base, uint32_t step, uint32_t K, const int32_t *cap, uint64_t *sums) override
    {
        if (!K || K > 64 || !step || base < kSlopeAll || base > kSlopeKMax) die("the search asked for a curve outside the kernel's limits");
        for (uint32_t f = 0; f < fr.F; ++f) {
            if (cap[f] < kSlopeAll || cap[f] > kSlopeKMax) die("the search passed a cap outside the grid");
            for (uint32_t j = 0; j < K; ++j) {
                const long long c = (long long)base + (long long)j * step;
                int32_t idx = c > kSlopeKMax ? kSlopeKMax : (int32_t)c;
                if (idx < cap[f]) idx = cap[f];
                const size_t at = (size_t)f * kCand + (size_t)(idx - kSlopeAll);
                sums[((size_t)f * K + j) * 2] += fr.body[at];
                sums[((size_t)f * K + j) * 2 + 1] += fr.bits[at];
            }
        }
    }
    uint64_t fixed_bytes(uint32_t) override { return kFixed; }
};

struct CpuPricer : BudgetPricer {
    const Frames &fr;
    explicit CpuPricer(const Frames &f) : fr(f) {}
    void lengths(const uint32_t *frames, const int32_t *index, uint32_t n, uint64_t *len) override
    {
        for (uint32_t i = 0; i < n; ++i) {
            if (frames[i] >= fr.F || index[i] < kSlopeAll || index[i] > kSlopeKMax) die("the search priced outside the call");
            len[i] = fr.price(frames[i], index[i]);
        }
    }
};

} // namespace

int main(int argc, char **argv)
{
    if (argc < 2) die("usage: budget_host <case file> [tables]");
    const bool tables = argc > 2 && !std::strcmp(argv[2], "tables");
    FILE *fp = std::fopen(argv[1], "rb");
    if (!fp) die("cannot open the case file");
    Reader r{fp};
    char magic[4];
    r.get(magic, 4);
    if (std::memcmp(magic, "RBG1", 4)) die("not a case file");
    const uint32_t n = r.get<uint32_t>(), F = r.get<uint32_t>(), pricer = r.get<uint32_t>();
    if (!F || n % F) die("frames do not divide the blocks");
    const uint32_t nb1 = n / F;
    Frames fr;
    fr.F = F; fr.pricer = pricer;
    fr.body.assign((size_t)F * kCand, 0);
    fr.bits.assign((size_t)F * kCand, 0);
    for (uint32_t b = 0; b < n; ++b) {
        const double w = r.get<double>();
        const uint32_t numbps = r.get<uint32_t>(), np = r.get<uint32_t>();
        if (np > (uint32_t)kRatePasses) die("too many passes");
        std::vector<uint32_t> rate(np);
        std::vector<int32_t> dist(np);
        r.get(rate.data(), np);
        r.get(dist.data(), np);
        std::vector<double> disto(np);
        rate_block_disto(w, numbps, np, dist.data(), disto.data(), nullptr);
        const uint32_t f = b / nb1;
        for (int p = 0; p < kCand; ++p) {
            const uint32_t k = rate_block_choose(rate.data(), disto.data(), np, 0, 0.0, false, rate_slope_grid(kSlopeAll + p), nullptr);
            const uint32_t bytes = k ? rate[k - 1] : 0u;
            fr.body[(size_t)f * kCand + p] += bytes;
            fr.bits[(size_t)f * kCand + p] += rate_block_header_bits(k, bytes);
        }
    }
    const uint32_t nset = r.get<uint32_t>();
    std::vector<std::pair<uint64_t, uint64_t>> settings(nset);
    for (auto &s : settings) { s.first = r.get<uint64_t>(); s.second = r.get<uint64_t>(); }
    std::fclose(fp);

    if (tables)
        for (uint32_t f = 0; f < F; ++f) {
            std::string line = "L " + std::to_string(f);
            for (int p = 0; p < kCand; ++p) line += " " + std::to_string(fr.price(f, kSlopeAll + p));
            std::puts(line.c_str());
        }
    for (uint32_t f = 0; f < F; ++f)
        for (int p = 0; p < kCand; p += 64)
            std::printf("C %u %d %llu %llu\n", f, kSlopeAll + p, (unsigned long long)fr.body[(size_t)f * kCand + p], (unsigned long long)fr.bits[(size_t)f * kCand + p]);

    for (uint32_t k = 0; k < nset; ++k)
        for (int run = 0; run < 2; ++run) {
            CpuCurve cv(fr);
            CpuPricer px(fr);
            BudgetSearch search(F, cv, px);
            const BudgetOutcome o = search.run(settings[k].first, settings[k].second);
            std::string line = "R " + std::to_string(k) + " " + std::to_string(run) + " " + std::to_string((int)o.status) + " " +
                               std::to_string(settings[k].first) + " " + std::to_string(settings[k].second) + " " + std::to_string(o.shared) + " " +
                               std::to_string(o.curve_launches) + " " + std::to_string(o.exact_plans) + " " + std::to_string(o.smallest) + " |";
            if (o.status == BudgetOutcome::OK) {
                if (o.cap.size() != F || o.index.size() != F || o.len.size() != F) die("an outcome without its frames");
                uint64_t total = 0;
                for (uint32_t f = 0; f < F; ++f) {
                    if (o.index[f] != (o.cap[f] > o.shared ? o.cap[f] : o.shared)) die("a frame's index is not max(shared, cap)");
                    if (o.len[f] != fr.price(f, o.index[f])) die("a frame's length is not the pricer's");
                    total += o.len[f];
                }
                if (total != o.total) die("the total is not the sum of the lengths");
                for (uint32_t f = 0; f < F; ++f) line += " " + std::to_string(o.cap[f]);
                for (uint32_t f = 0; f < F; ++f) line += " " + std::to_string(o.index[f]);
            } else if (o.status == BudgetOutcome::OVER_TOTAL) { // (the caps stand; no frame has an index)
                if (o.cap.size() != F) die("an outcome without its caps");
                for (int twice = 0; twice < 2; ++twice)
                    for (uint32_t f = 0; f < F; ++f) line += " " + std::to_string(o.cap[f]);
            }
            std::puts(line.c_str());
        }
    return 0;
}
