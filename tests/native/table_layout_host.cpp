// The two table layouts of j2k_amd/csrc/table_layout.h on the host, the header included alone: T1Tables (the Tier-1 result
// tables) and GatherPlan (the gather plan), over real buffers of the sizes they report, so that the sanitizers see every access.
// Prints "ok <checks>" and returns 0, or names what failed and returns 1.  Driven by tests/test_table_layout_host.py.
#include "table_layout.h"

#include <cstdio>
#include <vector>

using namespace j2k_hip;

static int failures = 0, checks = 0;
#define CHECK(cond)                                                                                              \
    do {                                                                                                         \
        ++checks;                                                                                                \
        if (!(cond)) { ++failures; std::printf("line %d: %s  [%s]\n", __LINE__, #cond, what); }                  \
    } while (0)

// stand-ins for the launch structs of kernels.h (which needs HIP): the fields the fillers set, with the kernels' types
struct T1ArgsLike { unsigned int *numbps, *npasses, *nsym, *len, *err, *pass_nsym; int *pass_nmsedec; unsigned int *pass_rate; };
struct GatherArgsLike {
    const uint8_t *blob; const unsigned long long *hdr_dst, *cblk_dst, *seg_dst, *seg_src; const unsigned int *hdr_src, *hdr_len, *seg_len;
    int nhdr, nseg;
};

static void t1_tables(size_t nb)
{
    char what[64];
    std::snprintf(what, sizeof what, "T1Tables nb=%zu", nb);
    const T1Tables t(nb);
    std::vector<uint32_t> meta(t.meta_bytes() / 4), passes(t.passes_bytes() / 4);
    uint32_t *m = meta.data(), *p = passes.data();
    CHECK(t.meta_bytes() % 4 == 0 && t.passes_bytes() % 4 == 0);
    // the columns are nb words apart, in the documented order, the error word at 4 nb inside the arena and inside what a reader copies
    CHECK(t.numbps(m) == m && t.npasses(m) == m + nb && t.len(m) == m + 2 * nb && t.nsym(m) == m + 3 * nb && t.err(m) == m + 4 * nb);
    CHECK((4 * nb + 1) * 4 <= t.meta_bytes() && t.meta_words() == 4 * nb + 1);
    CHECK(T1Tables::kColumns * t.column_bytes() == 4 * nb * 4);
    const uint32_t *cm = m; // (a host image is read through const pointers)
    CHECK(t.err(cm) == cm + 4 * nb);
    // passes: three columns of nb rows of kMaxPasses words
    CHECK(t.row(0) == 0 && t.row(1) == (size_t)kMaxPasses && t.row(nb) == nb * kMaxPasses);
    for (size_t i = 0; i + 1 <= nb; ++i) CHECK(t.row(i + 1) - t.row(i) == (size_t)kMaxPasses);
    CHECK(t.pass_nsym(p) == p && t.pass_nmsedec(p) == p + t.row(nb) && t.pass_rate(p) == p + 2 * t.row(nb));
    CHECK(t.passes_words() == 3 * t.row(nb) && t.passes_words() * 4 <= t.passes_bytes());
    // the host image: the two columns behind the decisions in one copy, or the rate column alone
    CHECK(t.h_passes_bytes() == (t.passes_words() - t.row(nb)) * 4 && t.h_rates_bytes() == t.row(nb) * 4);
    CHECK(t.h_rate(p) - p == t.pass_rate(p) - t.pass_nmsedec(p));
    T1ArgsLike a{};
    t.fill(a, m, p);
    CHECK(a.numbps == t.numbps(m) && a.npasses == t.npasses(m) && a.len == t.len(m) && a.nsym == t.nsym(m) && a.err == t.err(m));
    CHECK(a.pass_nsym == t.pass_nsym(p) && (void *)a.pass_nmsedec == (void *)t.pass_nmsedec(p) && a.pass_rate == t.pass_rate(p));
    // every word the accessors name is inside the arenas
    *a.err = 7;
    for (size_t i = 0; i < nb; ++i) {
        a.numbps[i] = a.npasses[i] = a.len[i] = a.nsym[i] = (uint32_t)i;
        a.pass_nsym[t.row(i) + kMaxPasses - 1] = 1; a.pass_nmsedec[t.row(i) + kMaxPasses - 1] = -1; a.pass_rate[t.row(i) + kMaxPasses - 1] = 1;
    }
    CHECK(*t.err(cm) == 7);
}

static void gather_plan(size_t blob_bytes, size_t nh, size_t nbd, size_t nseg)
{
    char what[96];
    std::snprintf(what, sizeof what, "GatherPlan blob=%zu nh=%zu nbd=%zu nseg=%zu", blob_bytes, nh, nbd, nseg);
    const GatherPlan g(blob_bytes, nh, nbd, nseg);
    std::vector<unsigned long long> store(g.total / 8 + 1); // (an 8-byte aligned base, as the arenas are)
    uint8_t *base = reinterpret_cast<uint8_t *>(store.data());
    const GatherTables t = g.tables(base);
    // today's rounding: the blob to 16 after + 8, the total to 64 after + 64
    CHECK(g.blob_sz == (blob_bytes + 8 + 15) / 16 * 16);
    CHECK(g.total == (g.blob_sz + nh * 16 + nbd * 8 + nseg * 20 + 64 + 63) / 64 * 64);
    // the tables in the documented order, each starting where the one before ends: no overlap, no gap
    const uint8_t *at = base + g.blob_sz;
    const struct { const void *p; size_t n, width; } order[7] = {{t.hdr_dst, nh, 8}, {t.cblk_dst, nbd, 8}, {t.seg_dst, nseg, 8}, {t.seg_src, nseg, 8},
                                                                 {t.hdr_src, nh, 4}, {t.hdr_len, nh, 4}, {t.seg_len, nseg, 4}};
    CHECK(blob_bytes <= g.blob_sz);
    for (const auto &o : order) {
        CHECK(o.p == at);
        CHECK((reinterpret_cast<uintptr_t>(o.p) - reinterpret_cast<uintptr_t>(base)) % o.width == 0 && reinterpret_cast<uintptr_t>(o.p) % o.width == 0);
        at += o.n * o.width;
    }
    CHECK(at <= base + g.total); // the last table ends inside the reported total
    GatherArgsLike a{};
    g.fill(a, base);
    CHECK(a.blob == base && a.hdr_dst == t.hdr_dst && a.cblk_dst == t.cblk_dst && a.seg_dst == t.seg_dst && a.seg_src == t.seg_src);
    CHECK(a.hdr_src == t.hdr_src && a.hdr_len == t.hdr_len && a.seg_len == t.seg_len && a.nhdr == (int)nh && a.nseg == (int)nseg);
    for (size_t i = 0; i < nh; ++i) { t.hdr_dst[i] = 1; t.hdr_src[i] = 2; t.hdr_len[i] = 3; }
    for (size_t i = 0; i < nbd; ++i) t.cblk_dst[i] = 4;
    for (size_t i = 0; i < nseg; ++i) { t.seg_dst[i] = 5; t.seg_src[i] = 6; t.seg_len[i] = 7; }
    for (size_t i = 0; i < nh; ++i) CHECK(a.hdr_dst[i] == 1 && a.hdr_src[i] == 2 && a.hdr_len[i] == 3);
    for (size_t i = 0; i < nbd; ++i) CHECK(a.cblk_dst[i] == 4);
    for (size_t i = 0; i < nseg; ++i) CHECK(a.seg_dst[i] == 5 && a.seg_src[i] == 6 && a.seg_len[i] == 7);
}

int main()
{
    for (size_t nb : {0, 1, 64, 65}) t1_tables(nb);
    for (size_t blob : {0, 1, 8, 15, 16})
        for (size_t nh : {0, 1, 3})
            for (size_t nbd : {0, 1, 3})
                for (size_t nseg : {0, 1, 3}) gather_plan(blob, nh, nbd, nseg);
    if (failures) { std::printf("%d of %d checks failed\n", failures, checks); return 1; }
    std::printf("ok %d\n", checks);
    return 0;
}
