// N-d box geometry shared between the planner, the CPU reference ops and
// the CDNA4 kernels. Header-only and host/device-compilable, with no torch
// includes (tests/cc/test_box_geometry.cc builds it with plain g++).
//
// A box full[lo_0:hi_0, ..., lo_{r-1}:hi_{r-1}] of a contiguous tensor,
// flattened in row-major order, is a nest of equally long contiguous runs
// of the full tensor's element space. BoxGeometry is that nest in its
// smallest form; the windowed slice of one dim (ShardWindow in
// deferred_init.cc) is its one-level case and a flat range its zero-level
// case.

#pragma once

#include <cstddef>
#include <cstdint>

#include "philox.h"  // TDX_HD, philox::mulhi32

namespace tdx {

constexpr int kMaxBoxLevels = 4;
// Highest tensor rank normalizeBox accepts.
constexpr int kMaxBoxRank = 64;

// Shard flat index i splits into within = i % run_len and row = i / run_len;
// row is decomposed innermost-first (level levels-1 first) over extent[]
// into coordinates c_l, and the element of the full tensor is
//   g_off + sum_l c_l * g_stride[l] + within.
// Levels are stored outermost first.
struct BoxGeometry {
  int64_t g_off = 0;
  int64_t run_len = 0;
  int32_t levels = 0;
  int64_t extent[kMaxBoxLevels] = {1, 1, 1, 1};
  int64_t g_stride[kMaxBoxLevels] = {0, 0, 0, 0};

  TDX_HD int64_t rows() const {
    int64_t n = 1;
    for (int l = 0; l < levels; ++l) {
      n *= extent[l];
    }
    return n;
  }

  TDX_HD int64_t numel() const { return rows() * run_len; }

  // First full-tensor element of run `row`.
  TDX_HD int64_t rowStart(int64_t row) const {
    int64_t g = g_off;
    for (int l = levels - 1; l >= 0; --l) {
      const int64_t q = row / extent[l];
      g += (row - q * extent[l]) * g_stride[l];
      row = q;
    }
    return g;
  }

  TDX_HD int64_t globalIndex(int64_t i) const {
    const int64_t row = i / run_len;
    return rowStart(row) + (i - row * run_len);
  }

  // One past the last full-tensor element the box touches (0 when empty).
  TDX_HD int64_t footprintEnd() const {
    if (numel() == 0) {
      return 0;
    }
    int64_t last = g_off + run_len;
    for (int l = 0; l < levels; ++l) {
      last += (extent[l] - 1) * g_stride[l];
    }
    return last;
  }
};

enum class BoxStatus {
  kOk,
  kBadRank,        // rank < 0 or rank > kMaxBoxRank
  kBadRange,       // not 0 <= lo <= hi <= size on some dim
  kTooManyLevels,  // more than kMaxBoxLevels levels after normalizing
};

// Normalizes the box [lo, hi) of a contiguous tensor of `sizes`:
//  * trailing fully covered dims and the innermost partly covered dim fold
//    into the run;
//  * a level folds into its outer neighbour when the two are one strided
//    sequence (the inner one covers its whole dim);
//  * extent-1 levels are dropped, their offset living in g_off.
// An empty box gives levels == 0 and run_len == 0.
inline BoxStatus normalizeBox(const int64_t* sizes, const int64_t* lo,
                              const int64_t* hi, int rank, BoxGeometry* out) {
  *out = BoxGeometry{};
  if (rank < 0 || rank > kMaxBoxRank) {
    return BoxStatus::kBadRank;
  }
  int64_t ext[kMaxBoxRank + 1];
  int64_t str[kMaxBoxRank + 1];
  int n = 0;
  bool empty = false;
  int64_t g_off = 0;
  {
    int64_t stride = 1;
    // Innermost dim first while the strides are built; reversed below.
    for (int d = rank - 1; d >= 0; --d) {
      if (!(0 <= lo[d] && lo[d] <= hi[d] && hi[d] <= sizes[d])) {
        return BoxStatus::kBadRange;
      }
      const int64_t e = hi[d] - lo[d];
      empty = empty || e == 0;
      g_off += lo[d] * stride;
      if (e != 1) {  // extent-1 dims only move g_off
        ext[n] = e;
        str[n] = stride;
        ++n;
      }
      stride *= sizes[d];
    }
  }
  if (empty) {
    return BoxStatus::kOk;
  }
  // ext/str are innermost first. Fold into the run every level that
  // continues it, then fold level pairs that form one strided sequence.
  int64_t run_len = 1;
  int first = 0;
  while (first < n && str[first] == run_len) {
    run_len *= ext[first];
    ++first;
  }
  int64_t m_ext[kMaxBoxRank + 1];
  int64_t m_str[kMaxBoxRank + 1];
  int m = 0;
  for (int i = first; i < n; ++i) {
    if (m > 0 && str[i] == m_ext[m - 1] * m_str[m - 1]) {
      m_ext[m - 1] *= ext[i];
    } else {
      m_ext[m] = ext[i];
      m_str[m] = str[i];
      ++m;
    }
  }
  if (m > kMaxBoxLevels) {
    return BoxStatus::kTooManyLevels;
  }
  out->g_off = g_off;
  out->run_len = run_len;
  out->levels = m;
  for (int l = 0; l < m; ++l) {  // outermost first
    out->extent[l] = m_ext[m - 1 - l];
    out->g_stride[l] = m_str[m - 1 - l];
  }
  return BoxStatus::kOk;
}

// Validates the geometry arguments of tdx::rng_box_ (shared by its CPU and
// CDNA4 implementations). Returns nullptr when they describe a box of
// `shard_numel` elements inside a tensor of `full_numel`, else what is
// wrong with them.
inline const char* checkBoxArgs(const int64_t* extents, size_t n_extents,
                                const int64_t* g_strides, size_t n_strides,
                                int64_t run_len, int64_t g_off,
                                int64_t shard_numel, int64_t full_numel) {
  if (n_extents < 1 || n_extents > static_cast<size_t>(kMaxBoxLevels)) {
    return "expected 1 to 4 levels";
  }
  if (n_strides != n_extents) {
    return "extents and g_strides differ in length";
  }
  if (run_len < 0 || g_off < 0 || full_numel < 0) {
    return "run_len, g_off and full_numel must be >= 0";
  }
  int64_t rows = 1;
  int64_t inner_span = run_len;  // elements one step of the next level spans
  int64_t last = g_off;          // last element touched, when non-empty
  for (size_t i = n_extents; i-- > 0;) {
    if (extents[i] < 0) {
      return "extents must be >= 0";
    }
    if (g_strides[i] < inner_span) {
      return "a stride is smaller than what the level inside it spans";
    }
    int64_t reach = 0;
    if (__builtin_mul_overflow(extents[i], g_strides[i], &inner_span) ||
        __builtin_mul_overflow(rows, extents[i], &rows) ||
        __builtin_mul_overflow(extents[i] > 0 ? extents[i] - 1 : 0,
                               g_strides[i], &reach) ||
        __builtin_add_overflow(last, reach, &last)) {
      return "the box overflows 64-bit indexing";
    }
  }
  int64_t numel = 0;
  if (__builtin_mul_overflow(rows, run_len, &numel) ||
      __builtin_add_overflow(last, run_len, &last)) {
    return "the box overflows 64-bit indexing";
  }
  if (numel != shard_numel) {
    return "shard numel must equal prod(extents) * run_len";
  }
  if (numel == 0 ? g_off > full_numel : last > full_numel) {
    return "the box does not fit in full_numel";
  }
  return nullptr;
}

// Rows [first, last) of a box.
struct RowRange {
  int64_t first = 0;
  int64_t last = 0;

  TDX_HD int64_t count() const { return last - first; }
};

// The rows of `box` that hold at least one element of the full-tensor
// range [lo, hi). rowStart is strictly increasing in the row index (every
// stride is at least what the level inside it spans), so these rows are
// one contiguous range, found by two binary searches: the first row that
// ends after lo, and the first row that starts at or after hi. Empty boxes
// and ranges give {0, 0}. Used by tdx::patch_box_, which walks only these
// rows.
TDX_HD RowRange rowsMeeting(const BoxGeometry& box, int64_t lo,
                                   int64_t hi) {
  RowRange out;
  const int64_t rows = box.rows();
  if (box.run_len <= 0 || rows <= 0 || lo >= hi) {
    return out;
  }
  int64_t a = 0;
  int64_t b = rows;
  while (a < b) {  // first row with rowStart + run_len > lo
    const int64_t mid = a + (b - a) / 2;
    if (box.rowStart(mid) + box.run_len > lo) {
      b = mid;
    } else {
      a = mid + 1;
    }
  }
  const int64_t first = a;
  b = rows;
  while (a < b) {  // first row with rowStart >= hi
    const int64_t mid = a + (b - a) / 2;
    if (box.rowStart(mid) >= hi) {
      b = mid;
    } else {
      a = mid + 1;
    }
  }
  if (a > first) {
    out.first = first;
    out.last = a;
  }
  return out;
}

// Validates the patch arguments of tdx::patch_box_ that checkBoxArgs does
// not cover. Returns nullptr when they are sound.
inline const char* checkPatchArgs(int64_t patch_lo, int64_t patch_len,
                                  int64_t full_numel, int64_t dist,
                                  bool has_seed, bool has_offset) {
  int64_t end = 0;
  if (patch_lo < 0 || patch_len < 0 ||
      __builtin_add_overflow(patch_lo, patch_len, &end) || end > full_numel) {
    return "the patch does not fit in full_numel";
  }
  if (dist < 0 || dist > 4) {
    return "dist must be 0 (uniform), 1 (normal), 2 (bernoulli), 3 (fill) "
           "or 4 (zero)";
  }
  if (dist <= 2 && !(has_seed && has_offset)) {
    return "an RNG patch needs a seed and an offset";
  }
  return nullptr;
}

// Unsigned division by a fixed 32-bit divisor as a multiply-high, an add
// and a shift (Granlund & Montgomery, "Division by invariant integers
// using multiplication", PLDI'94): with s = ceil(log2 d) and
// magic = floor(2^32 * (2^s - d) / d) + 1,
//   n / d == (mulhi(n, magic) + n) >> s
// for every n < 2^31 (the bound keeps the 32-bit add from wrapping). The
// magic and shift are computed once on the host; the kernels that walk a
// box use this for their per-level row decomposition instead of the
// hardware's multi-instruction integer divide.
struct MagicDiv32 {
  uint32_t d = 1;
  uint32_t magic = 1;
  uint32_t shift = 0;
};

inline MagicDiv32 makeMagicDiv32(uint32_t d) {
  MagicDiv32 m;
  if (d == 0) {
    d = 1;  // never divided by: callers return early on empty boxes
  }
  uint32_t s = 0;
  while (s < 32 && (uint64_t{1} << s) < d) {
    ++s;
  }
  m.d = d;
  m.shift = s;
  m.magic = static_cast<uint32_t>(
      ((uint64_t{1} << 32) * ((uint64_t{1} << s) - d)) / d + 1);
  return m;
}

// n / m.d for n < 2^31.
TDX_HD uint32_t magicDiv(const MagicDiv32& m, uint32_t n) {
  return (philox::mulhi32(n, m.magic) + n) >> m.shift;
}

}  // namespace tdx
