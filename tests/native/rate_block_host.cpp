// rate_block_host.cpp -- j2k_amd/csrc/rate_block.h on the host, alone: reads a case file (tests/test_rate_model.py writes it)
// and prints every number it computes as hexadecimal bit patterns, for the Python model (tests/rate_model.py) to be held
// to bit for bit.  Built by the test with the address and undefined-behaviour sanitizers and run as a child process.
//
// Case file, little endian:  "RBH1"  u32 nblocks, then per block  f64 weight, u32 comp, u32 numbps, u32 npasses,
//   u32 rate[npasses], i32 nmsedec[npasses];  u32 first, u32 count, u32 has_done, u8 done[count] (if has_done);
//   u32 K, f64 ahead[K];  u32 nthresh, f64 thresh[nthresh];  u32 nheader, (u32 n, u32 bytes)[nheader].
// Output, one record per line:
//   D <block> <disto bits>...      R <block> <reach bits>...      B <block> <bmin> <bmax> <steepest>
//   A <component> <body>...        (the running sums of the walk's changes, as RateDevice::ahead returns them)
//   S <threshold index> <sums x 8> (as rate_scan_kernel adds them up)
//   T <threshold index> <block> <n> <lo> <hi> <bytes> <n without the shortcut>
//   H <n> <bytes> <bits>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rate_block.h"

using namespace j2k_hip;

namespace {

struct Reader {
    FILE *f;
    template <class T> T get()
    {
        T v;
        if (std::fread(&v, sizeof(T), 1, f) != 1) { std::fprintf(stderr, "case file cut short\n"); std::exit(2); }
        return v;
    }
};

uint64_t bits(double v) { uint64_t u; std::memcpy(&u, &v, 8); return u; }
uint32_t bits(float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; }

struct Block {
    double weight;
    uint32_t comp, numbps, np;
    uint32_t rate[kRatePasses];
    int32_t nmsedec[kRatePasses];
    double disto[kRatePasses];
    float reach[kRatePasses];
    double bmin, bmax, steepest;
};

} // namespace

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: rate_block_host <case file>\n"); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    Reader r{f};
    char magic[4];
    if (std::fread(magic, 1, 4, f) != 4 || std::memcmp(magic, "RBH1", 4) != 0) { std::fprintf(stderr, "not a case file\n"); return 2; }
    const uint32_t nb = r.get<uint32_t>();
    std::vector<Block> blocks(nb);
    for (uint32_t i = 0; i < nb; ++i) {
        Block &b = blocks[i];
        b.weight = r.get<double>(); b.comp = r.get<uint32_t>(); b.numbps = r.get<uint32_t>(); b.np = r.get<uint32_t>();
        if (b.np > (uint32_t)kRatePasses || b.comp > 3) { std::fprintf(stderr, "block %u outside the tables\n", i); return 2; }
        for (uint32_t p = 0; p < b.np; ++p) b.rate[p] = r.get<uint32_t>();
        for (uint32_t p = 0; p < b.np; ++p) b.nmsedec[p] = r.get<int32_t>();
        rate_block_disto(b.weight, b.numbps, b.np, b.nmsedec, b.disto, nullptr);
        b.steepest = 0.0;
        rate_block_bounds(b.rate, b.disto, b.np, &b.bmin, &b.bmax, b.reach, &b.steepest);
        std::printf("D %u", i);
        for (uint32_t p = 0; p < b.np; ++p) std::printf(" %016" PRIx64, bits(b.disto[p]));
        std::printf("\nR %u", i);
        for (uint32_t p = 0; p < b.np; ++p) std::printf(" %08x", bits(b.reach[p]));
        std::printf("\nB %u %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", i, bits(b.bmin), bits(b.bmax), bits(b.steepest));
    }
    const uint32_t first = r.get<uint32_t>(), count = r.get<uint32_t>(), has_done = r.get<uint32_t>();
    if (first > nb || count > nb - first) { std::fprintf(stderr, "range outside the blocks\n"); return 2; }
    std::vector<uint8_t> done(count, 0);
    for (uint32_t i = 0; has_done && i < count; ++i) done[i] = r.get<uint8_t>();
    const uint32_t K = r.get<uint32_t>();
    std::vector<double> ahead(K);
    for (double &a : ahead) a = r.get<double>();
    if (K) {
        std::vector<int64_t> delta(4 * (size_t)K, 0);
        for (uint32_t i = 0; i < count; ++i) {
            const Block &b = blocks[first + i];
            int64_t *dc = delta.data() + (size_t)b.comp * K;
            rate_block_ahead(b.rate, b.reach, b.np, done[i], ahead.data(), K, [&](uint32_t k, int64_t change) { dc[k] += change; });
        }
        for (uint32_t c = 0; c < 4; ++c) {
            std::printf("A %u", c);
            int64_t run = 0;
            for (uint32_t k = 0; k < K; ++k) { run += delta[(size_t)c * K + k]; std::printf(" %" PRIx64, (uint64_t)run); }
            std::printf("\n");
        }
    }
    const uint32_t nt = r.get<uint32_t>();
    for (uint32_t t = 0; t < nt; ++t) {
        const double thresh = r.get<double>();
        uint64_t sums[kRateSums] = {};
        for (uint32_t i = 0; i < count; ++i) {
            const Block &b = blocks[first + i];
            Taken tk;
            const uint32_t n = rate_block_choose(b.rate, b.disto, b.np, done[i], b.steepest, true, thresh, &tk);
            const uint32_t plain = rate_block_choose(b.rate, b.disto, b.np, done[i], b.steepest, false, thresh, nullptr);
            const uint32_t bytes = n ? b.rate[n - 1] : 0u, dn = done[i];
            const uint32_t before = dn ? b.rate[dn - 1] : 0u;
            const uint64_t body = n > dn ? bytes - before : 0u;
            sums[2 * b.comp] += body;
            sums[2 * b.comp + 1] += rate_block_header_bits(n - dn, (uint32_t)body);
            std::printf("T %u %u %u %" PRIx64 " %x %u %u\n", t, i, n, tk.lo, tk.hi, bytes, plain);
        }
        std::printf("S %u", t);
        for (uint64_t s : sums) std::printf(" %" PRIx64, s);
        std::printf("\n");
    }
    const uint32_t nh = r.get<uint32_t>();
    for (uint32_t i = 0; i < nh; ++i) {
        const uint32_t n = r.get<uint32_t>(), bytes = r.get<uint32_t>();
        std::printf("H %u %u %u\n", n, bytes, rate_block_header_bits(n, bytes));
    }
    std::fclose(f);
    return 0;
}
