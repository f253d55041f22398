// The share planner of the int8 scan's long passes (csrc/ehx_balance.h) on the CPU: includes nothing but that header, is built
// by the plain host compiler (tests/test_i8_balance_host.py) and checks, over random factors, tile counts from 0 to 40 000
// and chunk counts of 8, 64 and 256:
//   the cover is exact and the bounds are monotone; every XCD's range is proportional to its factor (to the rounding of
//   whole tiles) and split evenly over its chunks; zero-tile XCDs are allowed;
//   the clamp holds; the first update is applied in full and later ones with gain 1/4; XCDs without a rate keep their factor;
//   a corrupted table is refused and inconsistent factors fall back to the uniform split, which is the kernel's own arithmetic;
//   forced factors are used as they are and freeze the state.
#include "ehx_balance.h"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace ehx;

static int g_fail = 0;
#define CHECK(cond, ...)                         \
  do {                                           \
    if (!(cond)) {                               \
      if (++g_fail <= 20) {                      \
        printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        printf(__VA_ARGS__);                     \
        printf("\n");                            \
      }                                          \
    }                                            \
  } while (0)

static const uint32_t kChunkCounts[3] = {8, 64, 256};

// the kernel's arithmetic without a table (k_flati8.hip): chunk c takes [c tpc, (c + 1) tpc) cut at n_tiles
static void kernel_uniform(uint32_t n_tiles, uint32_t n_chunks, std::vector<uint32_t>* lo, std::vector<uint32_t>* hi) {
  const uint32_t tpc = (n_tiles + n_chunks - 1) / n_chunks;
  for (uint32_t c = 0; c < n_chunks; ++c) {
    const uint32_t b = c * tpc;
    uint32_t e = b + tpc;
    if (e > n_tiles) e = n_tiles;
    lo->push_back(e > b ? b : e);
    hi->push_back(e);
  }
}

static void check_cover(const uint32_t* b, uint32_t n_tiles, uint32_t n_chunks, const char* what) {
  CHECK(b[0] == 0, "%s: bounds[0] = %u", what, b[0]);
  CHECK(b[n_chunks] == n_tiles, "%s: bounds[%u] = %u, not %u", what, n_chunks, b[n_chunks], n_tiles);
  uint64_t total = 0;
  for (uint32_t c = 0; c < n_chunks; ++c) {
    CHECK(b[c] <= b[c + 1], "%s: bounds[%u] = %u > bounds[%u] = %u", what, c, b[c], c + 1, b[c + 1]);
    total += b[c + 1] >= b[c] ? b[c + 1] - b[c] : 0;
  }
  CHECK(total == n_tiles, "%s: the chunks hold %llu tiles of %u", what, (unsigned long long)total, n_tiles);
  CHECK(balance_valid(b, n_tiles, n_chunks), "%s: balance_valid refuses it", what);
}

static void test_bounds(std::mt19937_64& rng) {
  std::uniform_real_distribution<double> u01(0.0, 1.0);
  std::vector<uint32_t> b(kBalanceMaxChunks + 2);
  for (int it = 0; it < 6000; ++it) {
    const uint32_t n_chunks = kChunkCounts[it % 3];
    uint32_t n_tiles = (uint32_t)(rng() % 40001);
    if (it % 50 == 0) n_tiles = (uint32_t)(it / 50 % 20);   // (0 .. 19 tiles: fewer tiles than chunks)
    if (it % 50 == 1) n_tiles = 40000;
    double f[kXcds];
    const int kind = it % 5;
    for (uint32_t x = 0; x < kXcds; ++x) {
      if (kind == 0) f[x] = kBalanceLo + (kBalanceHi - kBalanceLo) * u01(rng);   // what the planner itself produces
      else if (kind == 1) f[x] = u01(rng) < 0.4 ? 0.0 : 3.0 * u01(rng);          // zero-tile XCDs
      else if (kind == 2) f[x] = 1e-6 + 1e6 * u01(rng) * u01(rng) * u01(rng);    // any scale
      else if (kind == 3) f[x] = x == (uint32_t)(it / 5 % 8) ? 1.0 : 0.0;        // all tiles on one XCD
      else f[x] = (x & 1u) ? 1.5 : 0.5;                                          // alternating
    }
    double sum = 0.0;
    for (double v : f) sum += v;
    if (!(sum > 0.0)) f[it % 8] = sum = 1.0;
    b[n_chunks + 1] = 0xDEADBEEFu;
    const bool ok = balance_bounds(f, n_tiles, n_chunks, b.data());
    CHECK(ok, "balance_bounds refused valid factors (it %d)", it);
    CHECK(b[n_chunks + 1] == 0xDEADBEEFu, "balance_bounds wrote past bounds[n_chunks]");
    check_cover(b.data(), n_tiles, n_chunks, "planned");
    uint32_t tiles[kXcds];
    balance_xcd_tiles(b.data(), n_chunks, tiles);
    const uint32_t cpx = n_chunks / kXcds;
    double cum = 0.0;
    for (uint32_t x = 0; x < kXcds; ++x) {
      // proportional: the XCD's range ends within one tile of its share of the cumulated factors
      cum += f[x];
      const double want_end = (double)n_tiles * cum / sum;
      CHECK(std::fabs((double)b[(x + 1) * cpx] - want_end) <= 1.0, "XCD %u ends at %u, its share at %.2f", x, b[(x + 1) * cpx], want_end);
      if (f[x] == 0.0) CHECK(tiles[x] == 0, "XCD %u has factor 0 and %u tiles", x, tiles[x]);
      // even inside: the chunks of an XCD differ by at most one tile
      uint32_t mn = ~0u, mx = 0;
      for (uint32_t j = 0; j < cpx; ++j) {
        const uint32_t len = b[x * cpx + j + 1] - b[x * cpx + j];
        mn = std::min(mn, len);
        mx = std::max(mx, len);
      }
      CHECK(mx - mn <= 1, "XCD %u: chunks of %u and %u tiles", x, mn, mx);
    }
  }
}

static void test_fallback(std::mt19937_64& rng) {
  std::vector<uint32_t> b(kBalanceMaxChunks + 1), lo, hi;
  for (int it = 0; it < 600; ++it) {
    const uint32_t n_chunks = kChunkCounts[it % 3], n_tiles = (uint32_t)(rng() % 40001);
    // the uniform split IS the kernel's arithmetic
    balance_uniform(n_tiles, n_chunks, b.data());
    check_cover(b.data(), n_tiles, n_chunks, "uniform");
    lo.clear();
    hi.clear();
    kernel_uniform(n_tiles, n_chunks, &lo, &hi);
    for (uint32_t c = 0; c < n_chunks; ++c)
      CHECK(b[c + 1] - b[c] == hi[c] - lo[c] && (hi[c] == lo[c] || b[c] == lo[c]), "uniform chunk %u: [%u, %u) against the kernel's [%u, %u)",
            c, b[c], b[c + 1], lo[c], hi[c]);
    // inconsistent factors: refused, and the uniform split in their place
    double f[kXcds] = {1, 1, 1, 1, 1, 1, 1, 1};
    const int kind = it % 4;
    if (kind == 0) f[it % 8] = -0.5;
    else if (kind == 1) f[it % 8] = std::nan("");
    else if (kind == 2) f[it % 8] = INFINITY;
    else for (double& v : f) v = 0.0;
    std::vector<uint32_t> g(kBalanceMaxChunks + 1, 7u);
    CHECK(!balance_bounds(f, n_tiles, n_chunks, g.data()), "balance_bounds accepted bad factors (kind %d)", kind);
    for (uint32_t c = 0; c <= n_chunks; ++c) CHECK(g[c] == b[c], "fallback bounds[%u] = %u, uniform %u", c, g[c], b[c]);
    // chunk counts the kernel's XCD mapping does not cover
    const double one[kXcds] = {1, 1, 1, 1, 1, 1, 1, 1};
    std::vector<uint32_t> h(kBalanceMaxChunks + 1, 7u);
    CHECK(!balance_bounds(one, n_tiles, 12, h.data()), "12 chunks accepted");
    check_cover(h.data(), n_tiles, 12, "12 chunks, uniform");
    // a corrupted table is refused
    if (n_tiles >= 2) {
      CHECK(balance_bounds(one, n_tiles, n_chunks, g.data()), "uniform factors refused");
      std::vector<uint32_t> bad = g;
      const uint32_t c = 1 + (uint32_t)(rng() % n_chunks);
      switch (it % 3) {
        case 0: bad[c] = n_tiles + 1 + (uint32_t)(rng() % 1000); break;   // past the pass (or a non-monotone step at the end)
        case 1: bad[0] = 1; break;
        default: bad[n_chunks] = n_tiles - 1; break;
      }
      CHECK(!balance_valid(bad.data(), n_tiles, n_chunks), "corrupted table accepted (it %d)", it);
    }
  }
}

static void test_updates(std::mt19937_64& rng) {
  std::uniform_real_distribution<double> u(0.5, 1.5);
  for (int it = 0; it < 300; ++it) {
    BalanceState st;
    const uint64_t key = BalanceState::key_of(4, 64, 465), other = BalanceState::key_of(4, 64, 128);
    CHECK(key != other && key != 0 && other != 0, "keys");
    CHECK(BalanceState::key_of(4, 64, 465) == BalanceState::key_of(4, 64, 470), "appended rows change the shape's key");
    double f[kXcds], want[kXcds];
    st.factors(key, f);
    for (double v : f) CHECK(v == 1.0, "factors before any measurement: %g", v);
    for (int round = 0; round < 12; ++round) {
      double r[kXcds];
      for (uint32_t x = 0; x < kXcds; ++x) r[x] = u(rng);
      const uint32_t skip = (uint32_t)(rng() % 8);
      if (round % 3 == 2) r[skip] = 0.0;   // an XCD without tiles: no rate
      st.factors(key, f);
      for (uint32_t x = 0; x < kXcds; ++x) {
        double v = round == 0 ? r[x] : f[x] + 0.25 * (r[x] - f[x]);
        if (!(r[x] > 0.0)) v = f[x];
        want[x] = std::min(kBalanceHi, std::max(kBalanceLo, v));
      }
      st.update(key, r);
      st.factors(key, f);
      for (uint32_t x = 0; x < kXcds; ++x) {
        CHECK(std::fabs(f[x] - want[x]) < 1e-12, "round %d XCD %u: factor %.6f, expected %.6f", round, x, f[x], want[x]);
        CHECK(f[x] >= kBalanceLo && f[x] <= kBalanceHi, "factor %.4f outside the clamp", f[x]);
      }
      double g[kXcds];
      st.factors(other, g);
      for (double v : g) CHECK(v == 1.0, "another shape's factors moved: %g", v);
    }
    // forced: used as they are, for every shape, and nothing moves underneath
    const double forced[kXcds] = {1, 0, 0, 0, 0, 0, 0, 9};
    double before[kXcds], r[kXcds] = {2, 2, 2, 2, 2, 2, 2, 2};
    st.factors(key, before);
    st.force(forced);
    CHECK(st.is_forced(), "force");
    st.update(key, r);
    st.factors(other, f);
    for (uint32_t x = 0; x < kXcds; ++x) CHECK(f[x] == forced[x], "forced factor %u: %g", x, f[x]);
    st.force(nullptr);
    st.factors(key, f);
    for (uint32_t x = 0; x < kXcds; ++x) CHECK(f[x] == before[x], "factor %u moved while forced: %g -> %g", x, before[x], f[x]);
    // more shapes than slots: the oldest is forgotten, nothing breaks
    for (uint32_t q = 1; q <= 7; ++q) st.update(BalanceState::key_of(q, 8 * q, 100), r);
    st.factors(BalanceState::key_of(7, 56, 100), f);
    CHECK(f[0] == kBalanceHi, "latest shape: %g", f[0]);
    st.reset();
    st.factors(key, f);
    for (double v : f) CHECK(v == 1.0, "after reset: %g", v);
  }
}

static void test_rates() {
  // 16 workgroups, two per XCD; XCD x finishes after 100 + 10 x ticks with 10 tiles: rate ~ 1 / (100 + 10 x)
  const uint32_t grid = 16;
  std::vector<uint64_t> st(2 * grid);
  uint32_t tiles[kXcds];
  for (uint32_t b = 0; b < grid; ++b) {
    st[2 * b] = 1000 + b;
    st[2 * b + 1] = 1000 + 100 + 10 * (b & 7u) - (b >> 3);   // (the later workgroup of an XCD finishes first: the latest counts)
  }
  for (uint32_t& t : tiles) t = 10;
  tiles[5] = 0;
  double rate[kXcds];
  uint64_t t0, fin[kXcds];
  CHECK(balance_rates(st.data(), grid, tiles, rate, &t0, fin), "rates");
  CHECK(t0 == 1000, "earliest start %llu", (unsigned long long)t0);
  double mean = 0.0;
  for (uint32_t x = 0; x < kXcds; ++x) {
    CHECK(fin[x] == 1100 + 10 * x, "finish of XCD %u: %llu", x, (unsigned long long)fin[x]);
    if (x != 5) mean += 10.0 / (100.0 + 10.0 * x) / 7.0;
  }
  for (uint32_t x = 0; x < kXcds; ++x)
    CHECK(std::fabs(rate[x] - (x == 5 ? 0.0 : 10.0 / (100.0 + 10.0 * x) / mean)) < 1e-12, "rate of XCD %u: %g", x, rate[x]);
  for (uint32_t& t : tiles) t = 0;
  CHECK(!balance_rates(st.data(), grid, tiles, rate), "rates of a pass without tiles");
}

int main() {
  std::mt19937_64 rng(20250211);
  test_bounds(rng);
  test_fallback(rng);
  test_updates(rng);
  test_rates();
  if (g_fail) {
    printf("balance_check: %d checks failed\n", g_fail);
    return 1;
  }
  printf("balance_check ok\n");
  return 0;
}
