// Deferred module initialization: record every op performed on fake tensors
// on an in-memory tape, then replay the tape to materialize real tensors.
//
// Capability parity with the reference deferred-init core
// (/root/reference/src/cc/torchdistx/deferred_init.{h,cc}): a boxed fallback
// on the pre-autograd `DeferredInit` dispatch key, an Op/OpNode tape with
// chronological (op_nr) ordering, storage-alias-aware in-place replay,
// view keep-alives, external-tensor version-counter checks, a
// VariableHooks proxy recording `.data` reads/writes, and identity-stable
// repeated materialization.

#pragma once

#include <ATen/ATen.h>

namespace tdx {

// TLS-scoped deferred-init mode; nestable.
void enterDeferredInit();
void leaveDeferredInit();
bool isDeferredInitActive() noexcept;

// RAII: temporarily disable deferred-init recording on this thread.
class NoDeferredInit {
 public:
  NoDeferredInit();
  ~NoDeferredInit();
  NoDeferredInit(const NoDeferredInit&) = delete;
  NoDeferredInit& operator=(const NoDeferredInit&) = delete;

 private:
  bool prev_;
};

// True when `tensor` is a fake tensor carrying a deferred-init record (i.e.
// materializeTensor can reconstruct it).
bool canMaterialize(const at::Tensor& tensor) noexcept;

// Replays the relevant tape segment and returns the real tensor. Identity
// rules: a non-fake input is returned as-is; repeated calls (and aliased
// fakes) yield the same underlying TensorImpl. Raises c10::ValueError for a
// fake tensor with no record.
at::Tensor materializeTensor(const at::Tensor& tensor);

// Introspection of a deferred tensor's tape record (observability beyond
// the reference, which exposes nothing). All fields are cheap to compute
// except pending_ops, which runs the same call-stack analysis
// materialization would.
struct RecordInfo {
  uint64_t op_nr = 0;          // tape position of the producing op
  size_t output_index = 0;     // which output of that op
  bool materialized = false;   // producer already replayed?
  std::string op_name;         // producer op (empty once replayed)
  size_t pending_ops = 0;      // ops a materialize call would replay now
};

// std::nullopt when `tensor` carries no deferred-init record.
std::optional<RecordInfo> recordInfo(const at::Tensor& tensor);

// Reduced replay plan of a simple init chain (see tensorInitPlan).
struct InitPlan {
  enum class Kind { kFactory, kUniform, kNormal, kBernoulli, kFill, kZero };
  Kind kind = Kind::kFactory;
  double p0 = 0.0;
  double p1 = 0.0;
  uint64_t seed = 0;
  uint64_t offset = 0;
  std::vector<int64_t> sizes;
  c10::ScalarType dtype = c10::ScalarType::Float;
  // Set when the chain ends in a dtype conversion behind an RNG value
  // step (`empty(..).normal_().to(bf16)`, `Module.to(dtype)` in the
  // builder): the values are drawn, and the tail applied, at src_dtype and
  // stored as `dtype` (tdx::rng_chain_cast_). Both are then one of
  // float32/bf16/f16. A converted fill/zero is a plain fill at `dtype`
  // with p0 already rounded through the source dtype, and has no
  // src_dtype.
  std::optional<c10::ScalarType> src_dtype;
  c10::Device device{c10::DeviceType::CPU};
  bool requires_grad = false;
};

std::optional<InitPlan> tensorInitPlan(const at::Tensor& tensor);

// One step of a fused pointwise-scalar tail (see tensorChainPlan). The
// opcode numbering is shared with the tdx::rng_chain_ ops and the CDNA4
// kernels (csrc/hip/init_kernels.hip applyTail). s0/s1 hold the recorded
// scalars as doubles; the kernels narrow them to float the way ATen
// narrows a scalar operand to opmath_t.
struct TailOp {
  enum Code : int32_t {
    kErfinv = 0,
    kMul = 1,       // s0
    kAdd = 2,       // s0 (alpha == 1 only)
    kSub = 3,       // s0 (alpha == 1 only)
    kClamp = 4,     // s0 = min, s1 = max
    kClampMin = 5,  // s0
    kClampMax = 6,  // s0
    kNeg = 7,
    kAbs = 8,
  };
  int32_t op = kErfinv;
  double s0 = 0.0;
  double s1 = 0.0;
};

constexpr size_t kMaxTailOps = 8;

// Name of a TailOp code ("erfinv", "mul", ...).
const char* tailOpName(int32_t op);

// InitPlan plus the fusable pointwise tail that follows the plan's value
// step (empty for chains tensorInitPlan already reduces).
struct ChainPlan : InitPlan {
  std::vector<TailOp> tail;
};

// Like tensorInitPlan, but a chain whose last whole-tensor value step is
// a pinned-Philox RNG step followed only by fusable pointwise-scalar ops
// (erfinv_/mul_/add_/sub_/clamp*_/neg_/abs_ with Scalar or wrapped-number
// operands, alpha == 1, at most kMaxTailOps of them) is plannable too:
// the tail runs in registers inside the RNG kernel. Pointwise steps
// before the last value step are dead and dropped. With
// fusedInitChainsEnabled() off, any pointwise step makes the chain
// unplannable, as in tensorInitPlan.
std::optional<ChainPlan> tensorChainPlan(const at::Tensor& tensor);

// A value step recorded on a contiguous proper sub-range of the tensor
// (`w[i].zero_()`, `w[:k].normal_(std=s)`): it sets flat elements
// [lo, lo + len) to what element k - lo of a contiguous len-element tensor
// gets from the whole-tensor op, and leaves the rest alone.
struct PatchStep {
  int64_t lo = 0;
  int64_t len = 0;
  InitPlan::Kind kind = InitPlan::Kind::kZero;  // never kFactory
  double p0 = 0.0;
  double p1 = 0.0;
  uint64_t seed = 0;
  uint64_t offset = 0;
};

// ChainPlan of the base value step plus the live patches behind it, in
// application order (later ones overwrite earlier ones).
struct PatchPlan : ChainPlan {
  std::vector<PatchStep> patches;
};

// tensorChainPlan for chains that also hold live patches. tensorInitPlan
// and tensorChainPlan return nullopt for those (their callers rely on
// "one value step"); this returns the base plan and the patches. nullopt
// whenever the chain is unplannable for any other reason, and when an RNG
// patch coexists with a dtype conversion (it draws at the dtype it was
// recorded at; slice materialization serves that, a batched plan does
// not). A constant patch recorded before a conversion carries its value
// already rounded through the source dtype.
std::optional<PatchPlan> tensorPatchPlan(const at::Tensor& tensor);

// Slice materialization: materializes indices [start_row, end_row) of
// the deferred tensor along `dim` WITHOUT materializing the rest,
// bitwise-equal to the corresponding slice of a full materialization
// (per device type). dim 0 serves FSDP `Shard(0)` and column-parallel
// weights; dim 1 serves row-parallel (Megatron-style TP) weights.
// Requires the tensor's tape to be a "simple init chain" — a factory
// (empty/zeros/ones/full) followed by in-place init ops
// (uniform_/normal_/bernoulli_/fill_/zero_) on the whole tensor or on a
// contiguous sub-range of it reached through view ops (select/slice/
// narrow/view/reshape/flatten/unflatten/squeeze/unsqueeze), aliasing
// pass-throughs (detach/variable_data) and same-device dtype conversions (`to`, and
// the `p.data = p.to(dtype)` that `Module.to(dtype)` records) — which is
// exactly what module constructors record; throws a descriptive error
// otherwise so callers can fall back to full materialization. The shard
// is generated at the chain's first dtype and converted shard-sized; an
// RNG step (and fusable tail) followed by one conversion between
// float32/bf16/f16 is a single launch that stores the final dtype. This
// is the FSDP/TP init primitive: N ranks materialize disjoint slices of a
// model larger than any single device, with zero communication.
at::Tensor materializeTensorShard(const at::Tensor& tensor,
                                  int64_t start_row,
                                  int64_t end_row,
                                  int64_t dim = 0);

// N-d form of materializeTensorShard: materializes the block
// full[starts[0]:ends[0], ..., starts[r-1]:ends[r-1]] alone (one entry per
// tensor dim; a 0-d tensor takes empty lists), bitwise-equal to that
// block of a full materialization. This is the 2-D mesh primitive (FSDP x
// TP, or EP x TP on stacked expert weights): a rank generates exactly the
// elements it keeps. The block is normalized into nested contiguous runs
// (csrc/core/box_geometry.h); flat ranges and single-dim windows launch
// the ops materializeTensorShard launches, deeper nests tdx::rng_box_.
// Same supported tapes and errors as materializeTensorShard; a block that
// needs more than kMaxBoxLevels (4) nested levels throws the same
// "slice materialization" error.
at::Tensor materializeTensorBlock(const at::Tensor& tensor,
                                  at::IntArrayRef starts,
                                  at::IntArrayRef ends);

}  // namespace tdx
