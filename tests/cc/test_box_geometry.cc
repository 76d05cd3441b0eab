// Standalone C++ unit tests for the shared box-geometry header (the N-d
// box normalizer and the 32-bit multiply-shift divisor that the planner,
// the CPU reference op and the CDNA4 box kernel compile). No torch
// dependency: built and run by tests/test_box_geometry_cc.py with a plain
// g++.

#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../torchdistx_amd/csrc/core/box_geometry.h"

static int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      if (failures < 20) {                                              \
        std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      }                                                                 \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

using tdx::BoxGeometry;
using tdx::BoxStatus;
using tdx::MagicDiv32;
using tdx::magicDiv;
using tdx::makeMagicDiv32;
using tdx::normalizeBox;

constexpr uint32_t kMaxDividend = 0x7fffffffu;  // 2^31 - 1

static void checkDivisor(uint32_t d, const std::vector<uint32_t>& randoms) {
  const MagicDiv32 m = makeMagicDiv32(d);
  auto one = [&](uint32_t n) {
    const uint32_t q = magicDiv(m, n);
    if (q != n / d || n - q * d != n % d) {
      if (failures < 20) {
        std::printf("FAIL divisor d=%u n=%u: got %u want %u\n", d, n, q,
                    n / d);
      }
      ++failures;
    }
  };
  one(0);
  one(1);
  one(d - 1);
  one(d);
  if (d + 1 <= kMaxDividend) {
    one(d + 1);
  }
  one(kMaxDividend);
  for (uint32_t n : randoms) {
    one(n);
  }
}

static void testDivisor() {
  std::mt19937 rng(20240607u);
  std::vector<uint32_t> randoms(100000);
  for (uint32_t& n : randoms) {
    n = rng() & kMaxDividend;
  }
  for (uint32_t d = 1; d <= 4096; ++d) {
    checkDivisor(d, randoms);
  }
  for (int k = 0; k <= 31; ++k) {
    const uint64_t p = uint64_t{1} << k;
    for (uint64_t d : {p - 1, p, p + 1}) {
      if (d >= 1 && d <= kMaxDividend) {
        checkDivisor(static_cast<uint32_t>(d), randoms);
      }
    }
  }
}

// Every box of `sizes`: enumerating the shard's flat indices through the
// normalized geometry must visit the global indices of the brute-force
// row-major walk over the box, in the same order.
static void sweepShape(const std::vector<int64_t>& sizes) {
  const int rank = static_cast<int>(sizes.size());
  std::vector<int64_t> strides(rank, 1);
  for (int d = rank - 2; d >= 0; --d) {
    strides[d] = strides[d + 1] * sizes[d + 1];
  }
  std::vector<int64_t> lo(rank, 0), hi(rank, 0);
  // Odometer over all (lo, hi) pairs with lo <= hi per dim.
  while (true) {
    BoxGeometry geo;
    const BoxStatus st =
        normalizeBox(sizes.data(), lo.data(), hi.data(), rank, &geo);
    CHECK(st == BoxStatus::kOk);
    std::vector<int64_t> want;
    std::vector<int64_t> idx(lo);
    bool empty = false;
    for (int d = 0; d < rank; ++d) {
      empty = empty || lo[d] == hi[d];
    }
    if (!empty) {
      while (true) {
        int64_t g = 0;
        for (int d = 0; d < rank; ++d) {
          g += idx[d] * strides[d];
        }
        want.push_back(g);
        int d = rank - 1;
        for (; d >= 0; --d) {
          if (++idx[d] < hi[d]) {
            break;
          }
          idx[d] = lo[d];
        }
        if (d < 0) {
          break;
        }
      }
    }
    CHECK(geo.numel() == static_cast<int64_t>(want.size()));
    CHECK(geo.levels >= 0 && geo.levels <= tdx::kMaxBoxLevels);
    if (geo.numel() == static_cast<int64_t>(want.size())) {
      bool same = true;
      for (int64_t i = 0; i < geo.numel(); ++i) {
        same = same && geo.globalIndex(i) == want[i];
      }
      CHECK(same);
      if (!want.empty()) {
        CHECK(geo.footprintEnd() == want.back() + 1);
        // Normal form: no extent-1 level, nothing left to fold.
        for (int l = 0; l < geo.levels; ++l) {
          CHECK(geo.extent[l] > 1);
          const int64_t inner_span =
              l + 1 < geo.levels ? geo.extent[l + 1] * geo.g_stride[l + 1]
                                 : geo.run_len;
          CHECK(geo.g_stride[l] > inner_span);
        }
      } else {
        CHECK(geo.footprintEnd() == 0);
      }
    }
    // Next box.
    int d = rank - 1;
    for (; d >= 0; --d) {
      if (++hi[d] <= sizes[d]) {
        break;
      }
      if (++lo[d] <= sizes[d]) {
        hi[d] = lo[d];
        break;
      }
      lo[d] = 0;
      hi[d] = 0;
    }
    if (d < 0) {
      break;
    }
  }
}

static BoxGeometry norm(const std::vector<int64_t>& sizes,
                        const std::vector<int64_t>& lo,
                        const std::vector<int64_t>& hi,
                        BoxStatus want = BoxStatus::kOk) {
  BoxGeometry geo;
  const BoxStatus st = normalizeBox(sizes.data(), lo.data(), hi.data(),
                                    static_cast<int>(sizes.size()), &geo);
  CHECK(st == want);
  return geo;
}

static void testCoalescing() {
  // Whole tensor, and a 0-d tensor: flat ranges.
  BoxGeometry g = norm({4, 6, 8}, {0, 0, 0}, {4, 6, 8});
  CHECK(g.levels == 0 && g.run_len == 192 && g.g_off == 0);
  g = norm({}, {}, {});
  CHECK(g.levels == 0 && g.run_len == 1 && g.g_off == 0 && g.numel() == 1);

  // dim-0 slice: a flat range.
  g = norm({4, 6, 8}, {1, 0, 0}, {3, 6, 8});
  CHECK(g.levels == 0 && g.run_len == 96 && g.g_off == 48);

  // Single-dim boxes: one level with the ShardWindow numbers
  // (n_blocks = prod(sizes[:dim]), block_len = len * inner,
  //  g_stride = size * inner, g_off = start * inner).
  g = norm({4, 6, 8}, {0, 2, 0}, {4, 5, 8});
  CHECK(g.levels == 1 && g.extent[0] == 4 && g.run_len == 24 &&
        g.g_stride[0] == 48 && g.g_off == 16);
  g = norm({4, 6, 8}, {0, 0, 3}, {4, 6, 7});
  CHECK(g.levels == 1 && g.extent[0] == 24 && g.run_len == 4 &&
        g.g_stride[0] == 8 && g.g_off == 3);
  // ... and a flat range when there is one block.
  g = norm({1, 6, 8}, {0, 2, 0}, {1, 5, 8});
  CHECK(g.levels == 0 && g.run_len == 24 && g.g_off == 16);

  // A full middle dim merges into its outer neighbour.
  g = norm({4, 6, 8}, {1, 0, 2}, {3, 6, 6});
  CHECK(g.levels == 1 && g.extent[0] == 12 && g.g_stride[0] == 8 &&
        g.run_len == 4 && g.g_off == 48 + 2);
  // Every dim partial: one level per outer dim.
  g = norm({4, 6, 8}, {1, 2, 2}, {3, 5, 6});
  CHECK(g.levels == 2 && g.extent[0] == 2 && g.g_stride[0] == 48 &&
        g.extent[1] == 3 && g.g_stride[1] == 8 && g.run_len == 4 &&
        g.g_off == 48 + 16 + 2);

  // An extent-1 dim is dropped, its offset folded into g_off.
  g = norm({4, 6, 8}, {1, 3, 2}, {3, 4, 6});
  CHECK(g.levels == 1 && g.extent[0] == 2 && g.g_stride[0] == 48 &&
        g.run_len == 4 && g.g_off == 48 + 24 + 2);
  // Single row / single column.
  g = norm({5, 7}, {2, 1}, {3, 6});
  CHECK(g.levels == 0 && g.run_len == 5 && g.g_off == 15);
  g = norm({5, 7}, {1, 3}, {4, 4});
  CHECK(g.levels == 1 && g.extent[0] == 3 && g.g_stride[0] == 7 &&
        g.run_len == 1 && g.g_off == 10);

  // Empty boxes.
  g = norm({4, 6, 8}, {1, 3, 2}, {3, 3, 6});
  CHECK(g.numel() == 0 && g.levels == 0);

  // Five partial dims: four levels. Six: unsupported.
  g = norm({3, 3, 3, 3, 3}, {1, 1, 1, 1, 1}, {3, 3, 3, 3, 3});
  CHECK(g.levels == 4 && g.run_len == 2 && g.numel() == 32);
  norm({3, 3, 3, 3, 3, 3}, {1, 1, 1, 1, 1, 1}, {3, 3, 3, 3, 3, 3},
       BoxStatus::kTooManyLevels);
  // Bad ranges.
  norm({4, 6}, {2, 0}, {1, 6}, BoxStatus::kBadRange);
  norm({4, 6}, {0, 0}, {4, 7}, BoxStatus::kBadRange);
  norm({4, 6}, {-1, 0}, {4, 6}, BoxStatus::kBadRange);
}

int main() {
  testDivisor();
  testCoalescing();
  sweepShape({7});
  sweepShape({3, 4});
  sweepShape({2, 3, 4});
  sweepShape({3, 1, 2, 3});
  sweepShape({2, 2, 3, 2, 2});

  if (failures == 0) {
    std::printf("box geometry unit tests: all passed\n");
    return 0;
  }
  std::printf("box geometry unit tests: %d failures\n", failures);
  return 1;
}
