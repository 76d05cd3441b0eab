// Standalone C++ unit tests for rowsMeeting (box_geometry.h): the rows of
// a box that meet a flat element range, which tdx::patch_box_ walks instead
// of the whole box. Compared exhaustively against brute force over every
// box of a few small tensor shapes and every [lo, hi), ranges outside the
// footprint and empty boxes included. No torch dependency: built and run by
// tests/test_patch_geometry_cc.py with a plain g++.

#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../torchdistx_amd/csrc/core/box_geometry.h"

static long failures = 0;
static long checked = 0;
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
using tdx::RowRange;
using tdx::normalizeBox;
using tdx::rowsMeeting;

// Brute force: the rows r with [rowStart(r), rowStart(r) + run_len)
// meeting [lo, hi), which must be exactly [first, last).
static void checkRange(const BoxGeometry& geo, int64_t lo, int64_t hi) {
  const RowRange got = rowsMeeting(geo, lo, hi);
  const int64_t rows = geo.numel() == 0 ? 0 : geo.rows();
  int64_t first = -1;
  int64_t last = -1;
  int64_t count = 0;
  for (int64_t r = 0; r < rows; ++r) {
    const int64_t rs = geo.rowStart(r);
    bool meets = false;
    for (int64_t e = rs; e < rs + geo.run_len; ++e) {
      meets = meets || (lo <= e && e < hi);
    }
    if (meets) {
      if (first < 0) {
        first = r;
      }
      last = r + 1;
      ++count;
    }
  }
  ++checked;
  if (count == 0) {
    CHECK(got.count() == 0);
    return;
  }
  // One contiguous range, and the one the helper found.
  CHECK(count == last - first);
  CHECK(got.first == first && got.last == last);
  CHECK(0 <= got.first && got.last <= rows);
}

static void sweepShape(const std::vector<int64_t>& sizes) {
  const int rank = static_cast<int>(sizes.size());
  int64_t numel = 1;
  for (int64_t s : sizes) {
    numel *= s;
  }
  std::vector<int64_t> lo(rank, 0), hi(rank, 0);
  while (true) {
    BoxGeometry geo;
    const BoxStatus st =
        normalizeBox(sizes.data(), lo.data(), hi.data(), rank, &geo);
    CHECK(st == BoxStatus::kOk);
    // Every range of the tensor, the empty ones and a margin past both
    // ends of the footprint included.
    for (int64_t a = -1; a <= numel + 1; ++a) {
      for (int64_t b = a; b <= numel + 2; ++b) {
        checkRange(geo, a, b);
      }
    }
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

static void testHandMade() {
  // Geometries as the ops receive them, extent-1 levels included.
  BoxGeometry g;
  g.g_off = 5;
  g.run_len = 3;
  g.levels = 1;
  g.extent[0] = 1;
  g.g_stride[0] = 3;
  RowRange r = rowsMeeting(g, 0, 5);
  CHECK(r.count() == 0);
  r = rowsMeeting(g, 7, 100);
  CHECK(r.first == 0 && r.last == 1);
  r = rowsMeeting(g, 8, 100);
  CHECK(r.count() == 0);
  // Empty shard: run_len 0.
  g.run_len = 0;
  r = rowsMeeting(g, 0, 100);
  CHECK(r.count() == 0);
  // Rows far apart, far out.
  g = BoxGeometry{};
  g.g_off = (int64_t{1} << 40) + 3;
  g.run_len = 29;
  g.levels = 2;
  g.extent[0] = 5;
  g.g_stride[0] = int64_t{1} << 20;
  g.extent[1] = 7;
  g.g_stride[1] = 64;
  for (int64_t row = 0; row < 35; ++row) {
    const int64_t rs = g.rowStart(row);
    r = rowsMeeting(g, rs + 28, rs + 29);
    CHECK(r.first == row && r.last == row + 1);
    r = rowsMeeting(g, rs + 29, rs + 30);
    CHECK(r.count() == 0);
    r = rowsMeeting(g, rs, g.rowStart(34) + 1);
    CHECK(r.first == row && r.last == 35);
  }

  CHECK(tdx::checkPatchArgs(0, 4, 4, 3, false, false) == nullptr);
  CHECK(tdx::checkPatchArgs(1, 4, 4, 3, false, false) != nullptr);
  CHECK(tdx::checkPatchArgs(-1, 2, 4, 3, false, false) != nullptr);
  CHECK(tdx::checkPatchArgs(0, -1, 4, 3, false, false) != nullptr);
  CHECK(tdx::checkPatchArgs(INT64_MAX, 2, INT64_MAX, 4, false, false) !=
        nullptr);
  CHECK(tdx::checkPatchArgs(0, 4, 4, 5, true, true) != nullptr);
  CHECK(tdx::checkPatchArgs(0, 4, 4, 1, true, false) != nullptr);
  CHECK(tdx::checkPatchArgs(0, 4, 4, 1, true, true) == nullptr);
}

int main() {
  testHandMade();
  sweepShape({7});
  sweepShape({3, 4});
  sweepShape({3, 4, 5});
  sweepShape({2, 3, 2, 3});

  if (failures == 0) {
    std::printf("patch geometry unit tests: all passed (%ld ranges)\n",
                checked);
    return 0;
  }
  std::printf("patch geometry unit tests: %ld failures\n", failures);
  return 1;
}
