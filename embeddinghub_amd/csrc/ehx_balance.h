// The share planner of the int8 scan's long passes (ehx_flat.cpp, flat_pass8): how many row tiles every XCD of the chip gets.
// A scan pass runs one persistent workgroup per CU and ends when the slowest one ends; the kernel maps chunks
// [x * n_chunks / 8, (x + 1) * n_chunks / 8) to XCD x (k_flati8.hip), and under a power-limited kernel the eight XCDs do not
// run at one clock.  Every workgroup of a stamped pass records when it started and when it finished (ScanArgsI8::stamps);
// from those the planner keeps, per space and per pass shape, eight rate factors — tiles per unit of time of every XCD,
// relative to their mean — and from the factors it builds the table the kernel reads its tile range from
// (ScanArgsI8::bounds): a contiguous range per XCD proportional to its factor, split evenly over the XCD's chunks.
// The partition cannot change an answer (thresholds are fixed per pass, the pools are unordered sets).
// Pure host arithmetic over the standard library: tests/host/balance_check.cpp builds it with the plain host compiler.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>

namespace ehx {

constexpr uint32_t kXcds = 8;
constexpr uint32_t kBalanceMaxChunks = 256;   // (the int8 scan's plans have at most 256 chunks)
constexpr double kBalanceLo = 0.85, kBalanceHi = 1.15;   // a factor's clamp, as a multiple of the uniform share
constexpr double kBalanceGain = 0.25;         // weight of a new measurement in the running average (the first: 1)

// today's split, as the kernel computes it without a table: chunk c takes [c * tpc, (c + 1) * tpc) cut at n_tiles, tpc =
// ceil(n_tiles / n_chunks)
inline void balance_uniform(uint32_t n_tiles, uint32_t n_chunks, uint32_t* bounds) {
  const uint64_t tpc = n_chunks ? ((uint64_t)n_tiles + n_chunks - 1) / n_chunks : 0;
  for (uint32_t c = 0; c <= n_chunks; ++c) bounds[c] = (uint32_t)std::min<uint64_t>((uint64_t)c * tpc, n_tiles);
}

// bounds[0] = 0, bounds[n_chunks] = n_tiles, monotone: every tile belongs to exactly one chunk
inline bool balance_valid(const uint32_t* bounds, uint32_t n_tiles, uint32_t n_chunks) {
  if (n_chunks == 0 || n_chunks > kBalanceMaxChunks || bounds[0] != 0u || bounds[n_chunks] != n_tiles) return false;
  for (uint32_t c = 0; c < n_chunks; ++c)
    if (bounds[c] > bounds[c + 1]) return false;
  return true;
}

// bounds[n_chunks + 1] from eight factors (any non-negative scale; an XCD's factor may be 0: it gets no tile).  n_chunks must
// be a multiple of 8 (the kernel's XCD mapping).  false — and the uniform split in bounds — on anything inconsistent.
inline bool balance_bounds(const double* f, uint32_t n_tiles, uint32_t n_chunks, uint32_t* bounds) {
  bool ok = n_chunks > 0 && n_chunks <= kBalanceMaxChunks && n_chunks % kXcds == 0;
  double sum = 0.0;
  for (uint32_t x = 0; ok && x < kXcds; ++x) {
    ok = std::isfinite(f[x]) && f[x] >= 0.0;
    sum += f[x];
  }
  ok = ok && std::isfinite(sum) && sum > 0.0;
  if (ok) {
    const uint32_t cpx = n_chunks / kXcds;
    double cum = 0.0;
    uint32_t lo = 0;
    for (uint32_t x = 0; x < kXcds; ++x) {
      cum += f[x];
      // (the last XCD ends at n_tiles exactly, whatever the rounding of the sum did)
      uint32_t hi = x + 1 == kXcds ? n_tiles : (uint32_t)std::min<double>((double)n_tiles, std::floor((double)n_tiles * (cum / sum) + 0.5));
      if (hi < lo) hi = lo;
      const uint64_t len = hi - lo;
      for (uint32_t j = 0; j < cpx; ++j) bounds[x * cpx + j] = lo + (uint32_t)(len * j / cpx);
      lo = hi;
    }
    bounds[n_chunks] = n_tiles;
    ok = balance_valid(bounds, n_tiles, n_chunks);
  }
  if (!ok) balance_uniform(n_tiles, n_chunks, bounds);
  return ok;
}

// tiles of every XCD under a table
inline void balance_xcd_tiles(const uint32_t* bounds, uint32_t n_chunks, uint32_t* tiles) {
  const uint32_t cpx = n_chunks / kXcds;
  for (uint32_t x = 0; x < kXcds; ++x) tiles[x] = bounds[(x + 1) * cpx] - bounds[x * cpx];
}

// One stamped pass of one batch -> the relative rates of the XCDs that had tiles: rate_x = tiles_x / (latest finish in XCD x -
// earliest start of the pass), divided by the mean over those XCDs; 0 for an XCD without tiles or without a usable time.
// stamps[2 b] / stamps[2 b + 1]: start / finish of workgroup b (any unit, one time base); workgroup b runs on XCD b & 7.
// *t0 / finish[8] (optional): the earliest start and every XCD's latest finish.  false: nothing usable.
inline bool balance_rates(const uint64_t* stamps, uint32_t grid, const uint32_t* tiles, double* rate, uint64_t* t0_out = nullptr,
                          uint64_t* finish_out = nullptr) {
  uint64_t t0 = ~0ull, fin[kXcds] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (uint32_t b = 0; b < grid; ++b) {
    t0 = std::min(t0, stamps[2 * b]);
    fin[b & 7u] = std::max(fin[b & 7u], stamps[2 * b + 1]);
  }
  if (t0_out) *t0_out = t0;
  double sum = 0.0;
  uint32_t n = 0;
  for (uint32_t x = 0; x < kXcds; ++x) {
    if (finish_out) finish_out[x] = fin[x];
    rate[x] = 0.0;
    if (tiles[x] == 0 || fin[x] <= t0) continue;
    rate[x] = (double)tiles[x] / (double)(fin[x] - t0);
    sum += rate[x];
    ++n;
  }
  if (n == 0 || !(sum > 0.0)) return false;
  for (uint32_t x = 0; x < kXcds; ++x) rate[x] *= (double)n / sum;
  return true;
}

// The factors of a space, per pass shape; a few shapes at a time (a space's cascade has two stamped passes; appends move the
// shape slowly), the least recently used one replaced.  Everything under one small mutex: with two pipelined callers batch
// i + 1 is planned before batch i is measured and simply uses older factors.
struct BalanceState {
  static constexpr int kShapes = 4;
  struct Shape {
    uint64_t key = 0;            // 0: free
    double f[kXcds];
    uint64_t updates = 0, used = 0;
  };

  // the shape of a pass: query tiles, chunks and the size class of a chunk (factors carry over while rows are appended)
  static uint64_t key_of(uint32_t q_tiles, uint32_t n_chunks, uint32_t tiles_per_chunk) {
    uint32_t cls = 0;
    while ((tiles_per_chunk >> cls) > 1u) ++cls;
    return 1ull | ((uint64_t)q_tiles << 8) | ((uint64_t)n_chunks << 24) | ((uint64_t)cls << 40);
  }

  // the factors a pass of this shape is planned with (uniform until a measurement exists; the forced ones while forced)
  void factors(uint64_t key, double* out) {
    std::lock_guard<std::mutex> l(mu);
    if (forced) {
      std::copy(forced_f, forced_f + kXcds, out);
      return;
    }
    const Shape* s = find(key);
    for (uint32_t x = 0; x < kXcds; ++x) out[x] = s && s->updates ? s->f[x] : 1.0;
  }
  // one measurement (balance_rates): the first is applied in full, later ones with kBalanceGain; an XCD without a rate keeps
  // its factor; every factor stays inside the clamp.  Nothing moves while the factors are forced.
  void update(uint64_t key, const double* rate) {
    std::lock_guard<std::mutex> l(mu);
    if (forced) return;
    Shape* s = find(key);
    if (!s) {
      s = &shape[0];
      for (Shape& c : shape)
        if (c.key == 0 || (s->key != 0 && c.used < s->used)) s = &c;
      s->key = key;
      s->updates = 0;
      for (double& v : s->f) v = 1.0;
    }
    for (uint32_t x = 0; x < kXcds; ++x) {
      if (!(rate[x] > 0.0) || !std::isfinite(rate[x])) continue;
      const double v = s->updates ? s->f[x] + kBalanceGain * (rate[x] - s->f[x]) : rate[x];
      s->f[x] = std::min(kBalanceHi, std::max(kBalanceLo, v));
    }
    ++s->updates;
    s->used = ++tick;
  }
  // tests: eight factors of any non-negative size, used as they are for every shape until released (f == nullptr)
  void force(const double* f) {
    std::lock_guard<std::mutex> l(mu);
    forced = f != nullptr;
    if (f) std::copy(f, f + kXcds, forced_f);
  }
  bool is_forced() {
    std::lock_guard<std::mutex> l(mu);
    return forced;
  }
  void reset() {
    std::lock_guard<std::mutex> l(mu);
    for (Shape& c : shape) c = Shape();
    forced = false;
  }

 private:
  Shape* find(uint64_t key) {
    for (Shape& c : shape)
      if (c.key == key) {
        c.used = ++tick;
        return &c;
      }
    return nullptr;
  }
  std::mutex mu;
  Shape shape[kShapes];
  uint64_t tick = 0;
  bool forced = false;
  double forced_f[kXcds] = {1, 1, 1, 1, 1, 1, 1, 1};
};

}  // namespace ehx
