// The buffer planner and the offsets check of syzkaller_amd/csrc/sg_plan.h, on
// the CPU: alignment, no overlap, the total, the region-count overflow, and
// the three largest staging layouts against the byte counts their entry points
// summed by hand before they used the planner; grow_cap, the capacity policy
// of the grow-only buffers; bits_below, the sorts' mask over keys below n; and
// band_plan, the launch arithmetic of k_prio_band.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "sg_plan.h"

using sg::WsPlan;

static int fails = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      fails++;                                                \
    }                                                         \
  } while (0)

// adds raw[i] bytes per region and expects region i at the sum of want[0 .. i),
// `want` being the aligned byte counts of the hand-written layout
static void layout(const char* name, const std::vector<size_t>& raw, const std::vector<size_t>& want, size_t total) {
  WsPlan p;
  size_t at = 0;
  CHECK(raw.size() == want.size());
  for (size_t i = 0; i < raw.size(); i++) {
    const size_t o = p.add(raw[i]);
    if (o != at) {
      printf("FAIL %s: region %zu at %zu, expected %zu\n", name, i, o, at);
      fails++;
    }
    CHECK(o == p.off[i]);
    at += want[i];
  }
  CHECK(at == total);
  CHECK(p.total == total);
  CHECK(!p.overflow);
}

int main() {
  {  // alignment, no overlap, the total; a zero-byte region costs nothing
    const size_t sizes[] = {0, 1, 255, 256, 257, 0, 1};
    WsPlan p;
    size_t prev_end = 0;
    for (size_t b : sizes) {
      const size_t before = p.total, o = p.add(b);
      CHECK(o % 256 == 0);
      CHECK(o >= prev_end);  // starts at or after the end of every earlier region
      CHECK(o == before);
      if (b == 0) CHECK(p.total == before);
      prev_end = o + b;
      CHECK(p.total == sg::align256(prev_end));  // the end of the last region, rounded up
      CHECK(p.total >= prev_end && p.total - prev_end < 256);
    }
    CHECK(p.n == 7 && !p.overflow);
    CHECK(p.total == 0 + 256 + 256 + 256 + 512 + 0 + 256);
    CHECK(sg::align256(0) == 0 && sg::align256(1) == 256 && sg::align256(256) == 256 && sg::align256(257) == 512);
  }
  {  // one region past the capacity: reported, laid out, nothing written past off[]
    struct {
      WsPlan p;
      size_t guard[4];
    } g;
    for (size_t& x : g.guard) x = 0xA5A5A5A5u;
    for (int i = 0; i < WsPlan::kMaxRegions; i++) {
      CHECK(g.p.add(1) == (size_t)i * 256);
      CHECK(!g.p.overflow);
    }
    CHECK(g.p.n == WsPlan::kMaxRegions);
    const size_t last = g.p.off[WsPlan::kMaxRegions - 1];
    CHECK(g.p.add(1) == (size_t)WsPlan::kMaxRegions * 256);
    CHECK(g.p.overflow);
    CHECK(g.p.n == WsPlan::kMaxRegions);
    CHECK(g.p.off[WsPlan::kMaxRegions - 1] == last);
    CHECK(g.p.total == (size_t)(WsPlan::kMaxRegions + 1) * 256);
    for (size_t x : g.guard) CHECK(x == 0xA5A5A5A5u);
    CHECK(WsPlan::kMaxRegions >= 29);  // sg_triage_runs_from_kcov's host form
  }
  {  // offsets_ok
    const uint64_t empty[] = {0}, nonzero[] = {1, 2, 3}, ok[] = {0, 2, 2, 5, 5}, first[] = {3, 2, 4, 6, 8},
                   d_first[] = {0, 4, 3, 6, 8}, d_mid[] = {0, 2, 5, 4, 8}, d_last[] = {0, 2, 4, 6, 5};
    CHECK(sg::offsets_ok(empty, 0));
    CHECK(!sg::offsets_ok(nonzero, 2));
    CHECK(!sg::offsets_ok(nonzero, 0));
    CHECK(sg::offsets_ok(ok, 4));  // equal neighbours
    CHECK(!sg::offsets_ok(first, 4));
    CHECK(!sg::offsets_ok(d_first, 4));
    CHECK(!sg::offsets_ok(d_mid, 4));
    CHECK(!sg::offsets_ok(d_last, 4));
    CHECK(sg::offsets_ok(d_last, 3));  // the decreasing step lies past n
  }
  {  // sg_ipc_parse: 131 words, 37 programs, 71 calls
    const size_t nwords = 131, nprog = 37, nrec = 71;
    layout("sg_ipc_parse",
           {nwords * 4 + 4, nwords * 4 + 4, nwords * 4 + 4, (nprog + 1) * 8, (nprog + 1) * 8, (nrec + 1) * 8,
            (nrec + 1) * 8, (nrec + 1) * 8, nrec * 4 + 4, nrec + 1, nprog * 4 + 4},
           {768, 768, 768, 512, 512, 768, 768, 768, 512, 256, 256}, 6656);
  }
  {  // sg_triage_runs_from_kcov's host form: 67 candidates x 3 runs, 45 calls,
     // 301 PCs, 77 signals, new_cap >= 77, cov_cap 99: 12 staged regions, then
     // the body's 17
    const size_t n = 67, nexec = 201, ncalls = 45, npcs = 301, nsig = 77, ncap = 77, ccap = 99;
    layout("sg_triage_runs_from_kcov",
           {nsig * 4 + 4, (n + 1) * 8,      (n + 1) * 8,  (n + 1) * 8,  n * 4,        n,           (nexec + 1) * 8,
            (ncalls + 1) * 8, npcs * 8 + 8, n * 4,        ncap * 4 + 4, ccap * 4 + 4,
            npcs * 4 + 4, ncalls + 1,       nexec * 4 + 4, (ncalls + 1) * 8, npcs * 4 + 4, (ncalls + 1) * 8,
            npcs * 4 + 4, nsig * 4 + 4,     (n + 1) * 8,  n * 4 + 4,    n * 8 + 8,    n * 4 + 4,   n * 4 + 4,
            n * 4 + 4,    n + 1,            npcs * 4 + 4, npcs * 4 + 4},
           {512,  768, 768,  768, 512,  256, 1792, 512, 2560, 512, 512, 512,
            1280, 256, 1024, 512, 1280, 512, 1280, 512, 768,  512, 768, 512, 512, 512, 256, 1280, 1280},
           23040);
  }
  {  // sg_hints_from_kcov's host form: 21 records, 45 calls, 77 value slots: 6
     // staged regions, then the body's 3
    const size_t nrecs = 21, ncalls = 45, nvals = 77;
    layout("sg_hints_from_kcov",
           {nrecs * 32 + 32, (ncalls + 1) * 8, (ncalls + 1) * 8, nvals * 8 + 8, ncalls * 4 + 4, (nvals + 1) * 8,
            (ncalls + 1) * 8, (ncalls + 1) * 8, 2 * nrecs * 16 + 16},
           {768, 512, 512, 768, 256, 768, 512, 512, 768}, 5376);
  }
  {  // grow_cap: the capacity a grow-only buffer takes
    const size_t MiB = size_t(1) << 20;
    const struct {
      size_t cap, need, floor, want;
    } cases[] = {{0, 0, 1024, 0},
                 {0, 1, 1024, 1024},
                 {0, 1024, 1024, 1024},
                 {0, 1025, 1024, 2048},
                 {1024, 1024, 1024, 1024},
                 {1024, 1025, 1024, 2048},
                 {1024, 5000, 1024, 8192},
                 {2048, 2049, 1024, 4096},
                 {0, 1, 64 * MiB, 64 * MiB},
                 {64 * MiB, 64 * MiB + 1, 64 * MiB, 128 * MiB},
                 {0, 16 * MiB + 1, 16 * MiB, 32 * MiB}};
    for (const auto& c : cases) {
      const size_t got = sg::grow_cap(c.cap, c.need, c.floor);
      if (got != c.want) {
        printf("FAIL grow_cap(%zu, %zu, %zu) = %zu, expected %zu\n", c.cap, c.need, c.floor, got, c.want);
        fails++;
      }
    }
    for (size_t cap : {size_t(0), size_t(1024), size_t(3000)})
      for (size_t need = 0; need <= 10000; need++) {
        const size_t got = sg::grow_cap(cap, need, 1024);
        CHECK(got >= need);
        if (need <= cap) CHECK(got == cap);
        // the loop the key store's reserve ran before the policy was shared
        size_t nc = cap;
        if (need > cap) {
          nc = cap * 2 > 1024 ? cap * 2 : 1024;
          while (nc < need) nc *= 2;
        }
        CHECK(got == nc);
      }
  }
  {  // bits_below: 0 for n <= 1, else the smallest 2^k - 1 that is >= n - 1, on 0 .. 9; 2^k - 1, 2^k, 2^k + 1
     // for k in {8, 31, 32, 33, 63}; 2^64 - 1
    const struct {
      uint64_t n, want;
    } cases[] = {{0x0ull, 0x0ull},
                 {0x1ull, 0x0ull},
                 {0x2ull, 0x1ull},
                 {0x3ull, 0x3ull},
                 {0x4ull, 0x3ull},
                 {0x5ull, 0x7ull},
                 {0x6ull, 0x7ull},
                 {0x7ull, 0x7ull},
                 {0x8ull, 0x7ull},
                 {0x9ull, 0xfull},
                 {0xffull, 0xffull},
                 {0x100ull, 0xffull},
                 {0x101ull, 0x1ffull},
                 {0x7fffffffull, 0x7fffffffull},
                 {0x80000000ull, 0x7fffffffull},
                 {0x80000001ull, 0xffffffffull},
                 {0xffffffffull, 0xffffffffull},
                 {0x100000000ull, 0xffffffffull},
                 {0x100000001ull, 0x1ffffffffull},
                 {0x1ffffffffull, 0x1ffffffffull},
                 {0x200000000ull, 0x1ffffffffull},
                 {0x200000001ull, 0x3ffffffffull},
                 {0x7fffffffffffffffull, 0x7fffffffffffffffull},
                 {0x8000000000000000ull, 0x7fffffffffffffffull},
                 {0x8000000000000001ull, 0xffffffffffffffffull},
                 {0xffffffffffffffffull, 0xffffffffffffffffull}};
    for (const auto& c : cases) {
      const uint64_t got = sg::bits_below(c.n);
      if (got != c.want) {
        printf("FAIL bits_below(0x%llx) = 0x%llx, expected 0x%llx\n", (unsigned long long)c.n, (unsigned long long)got,
               (unsigned long long)c.want);
        fails++;
      }
      CHECK((got & (got + 1)) == 0);            // 2^k - 1
      CHECK(c.n <= 1 || got >= c.n - 1);        // covers 0 .. n - 1
      CHECK(got == 0 || (got >> 1) < c.n - 1);  // and no shorter mask does
    }
  }
  {  // band_plan: k_prio_band's launch for every matrix size and the id counts about its thresholds, against
     // the expressions sg_prio_table_add computed inline before (div_up returned uint32_t there), and what
     // the kernel relies on, in 64-bit arithmetic.  The digest and the table pin tests/call_prios_cases.py's
     // band_plan to this one (tests/test_call_prios_edges.py reads them).
    const uint32_t kCells = 40960, kT = 1024;
    const uint64_t kPart = 1ull << 26;
    const auto div_up = [](uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); };
    const auto up64 = [](uint64_t a, uint64_t b) { return (a + b - 1) / b; };
    const uint64_t nids_set[] = {1, 4095, 4096, 4097, kPart - 1, kPart, kPart + 1, (1ull << 32) - 1};
    uint64_t h = 14695981039346656037ull;
    int bad = 0;
    for (uint32_t ncalls = 1; ncalls <= 8192; ncalls++)
      for (uint64_t nids : nids_set) {
        const sg::BandPlan p = sg::band_plan(ncalls, nids, kCells, kT, kPart);
        // as sg_prio_table_add had it
        const uint32_t rows = std::max(1u, std::min(kCells / ncalls, ncalls));
        const uint32_t nbands = div_up(ncalls, rows);
        uint64_t nparts = std::min<uint64_t>(div_up(2048, nbands), div_up(nids, 4 * kT));
        nparts = std::max<uint64_t>(nparts, div_up(nids, kPart));
        const uint64_t part = (uint64_t)div_up(div_up(nids, nparts), kT) * kT;
        const uint32_t gridy = div_up(nids, part);
        bool ok = p.rows == rows && p.nbands == nbands && p.nparts == nparts && p.part == part && p.gridy == gridy;
        // what the kernel relies on
        ok = ok && p.rows >= 1 && (uint64_t)p.rows * ncalls <= kCells;  // (ncalls <= kCells throughout)
        ok = ok && (uint64_t)p.nbands * p.rows >= ncalls && ncalls > (uint64_t)(p.nbands - 1) * p.rows;
        ok = ok && p.part % kT == 0 && p.part >= kT && p.part <= kPart;
        ok = ok && (uint64_t)p.gridy * p.part >= nids && nids > (uint64_t)(p.gridy - 1) * p.part;
        // nothing truncated: every intermediate of the old form, in 64 bits, is its 32-bit value
        ok = ok && up64(ncalls, rows) == nbands && up64(2048, nbands) == div_up(2048, nbands);
        ok = ok && up64(nids, 4 * kT) == div_up(nids, 4 * kT) && up64(nids, kPart) == div_up(nids, kPart);
        ok = ok && up64(nids, nparts) == div_up(nids, nparts) && up64(up64(nids, nparts), kT) * kT == part;
        ok = ok && up64(nids, part) == gridy && gridy <= 65535;  // (a grid's y extent)
        if (!ok && bad++ < 5) printf("FAIL band_plan(%u, %llu)\n", ncalls, (unsigned long long)nids);
        for (uint64_t v : {(uint64_t)p.rows, (uint64_t)p.nbands, p.nparts, p.part, (uint64_t)p.gridy})
          h = (h ^ v) * 1099511628211ull;
      }
    fails += bad;
    printf("band_plan digest %016llx\n", (unsigned long long)h);
    for (uint32_t ncalls : {1u, 8u, 70u, 202u, 203u, 256u, 257u, 300u, 320u, 512u, 513u, 1025u, 1541u, 8191u, 8192u})
      for (uint64_t nids : {uint64_t(1), uint64_t(4097), uint64_t(45056), kPart + 1}) {
        const sg::BandPlan p = sg::band_plan(ncalls, nids, kCells, kT, kPart);
        printf("band_plan %u %llu %u %u %llu %llu %u\n", ncalls, (unsigned long long)nids, p.rows, p.nbands,
               (unsigned long long)p.nparts, (unsigned long long)p.part, p.gridy);
      }
    // ncalls past the band (not reachable: SG_PRIO_MAX_CALLS is 8192): a one-row band is still planned
    CHECK(sg::band_plan(kCells + 1, 1, kCells, kT, kPart).rows == 1);
  }
  if (fails) return 1;
  printf("PASS\n");
  return 0;
}
