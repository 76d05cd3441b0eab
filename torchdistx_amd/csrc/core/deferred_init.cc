// See deferred_init.h. Reference behavior map (file:line into
// /root/reference/src/cc/torchdistx/deferred_init.cc):
//   recording fallback + stack copy      — :732-862, :88-100
//   Op / OpNode / TensorRecord tape      — :157-462
//   view keep-alives                     — :126-154, :431-462
//   materialization (call-stack build)   — :506-667
//   VariableHooks proxy                  — :889-948, :1050-1128
//
// The tape is re-designed rather than translated: one mutable TensorRecord
// per fake impl (restamped in place), per-storage AliasGroups owning the
// family's writer nodes (an acyclic replacement for the reference's view
// keep-alives), record-time history snapshots for cross-family reads, and
// a replay collection that takes a family's full writer set, closes over
// dependencies + each writer's chronological prefix, and pulls in (to
// fixpoint) readers whose inputs a collected later writer would clobber.
// Validated differentially against eager execution by tests/test_tape_fuzz
// (thousands of random aliasing programs).

#include "deferred_init.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>
#include <mutex>
#include <optional>
#include <unordered_set>
#include <vector>

#include <ATen/CPUGeneratorImpl.h>
#include <ATen/Context.h>
#include <ATen/ThreadLocalState.h>
#include <c10/core/GradMode.h>
#include <ATen/core/dispatch/Dispatcher.h>
#include <ATen/core/VariableHooksInterface.h>
#include <c10/core/DefaultDtype.h>
#include <c10/core/impl/LocalDispatchKeySet.h>
#include <torch/library.h>

#include "box_geometry.h"
#include "fake.h"
#include "native_redirect.h"
#include "stack_utils.h"

namespace tdx {
namespace {

constexpr c10::DispatchKey kDeferredKey = c10::DispatchKey::DeferredInit;
constexpr c10::DispatchKey kFakeKey = c10::DispatchKey::Fake;

struct OpNode;

// Producer edge: which output of which node materializes a given fake.
struct OpOutputDescriptor {
  std::shared_ptr<OpNode> node;
  size_t index = 0;  // tensor-visit-order index into the node's outputs
};

// All tensors sharing one (meta) storage share one AliasGroup, which owns
// every node that wrote to that storage. Any surviving member of the alias
// family therefore keeps the whole family's tape segments alive — a view
// can outlive its base (and vice versa) without losing in-place writes —
// and, unlike record<->record keep-alive edges, the ownership graph is
// acyclic: groups own nodes, nodes own dependency nodes, records own their
// group. When the last fake of the family dies, the group and its nodes
// (including any materialized outputs they cache) are released.
struct AliasGroup {
  std::vector<std::shared_ptr<OpNode>> writers;
};

// Per-fake-tensor record, stored in the impl's dispatch-key side table.
// Mutable: an in-place op restamps `desc` in place, so aliased tensors
// observe the rewrite through their shared group.
struct TensorRecord {
  OpOutputDescriptor desc;
  std::shared_ptr<AliasGroup> group;
};

// One recorded call frame.
struct RecordedOp {
  std::string name;
  // Contract: consumes the arguments from the stack and leaves exactly the
  // op's return values on it (OperatorHandle::callBoxed semantics).
  std::function<void(torch::jit::Stack&)> run;
  std::vector<c10::IValue> args;  // deep-copied; fake slots -> undefined
  at::ThreadLocalState tls;       // captured with DeferredInit excluded
  // Pinned Philox (seed, counter offset) for RNG ops; also consumed by the
  // slice-materialization fast path (materializeTensorShard).
  std::optional<std::pair<uint64_t, uint64_t>> philox;
  // The dispatcher op, for ops recorded by the boxed fallback (not the
  // tdx:: pseudo-ops): the chain model reads argument names off its schema.
  std::optional<c10::OperatorHandle> handle;
};

// Pinned Philox state for recorded RNG ops: derived from the default
// generator's seed and the op's tape position at RECORD time, so replaying
// ANY subset of the tape on ANY rank produces identical bits
// (partition-invariant initialization — the property that makes sharded /
// broadcast materialization bitwise-equal to local materialization when
// the native CDNA4 kernels run the replay).
constexpr uint64_t kPhiloxStridePerOp = 4;

// RNG session, one per outermost deferred_init on each thread (sessions
// are per-thread by construction: deferred_level is thread_local).
//
// A session is partitioned into SEGMENTS by the mutations the user makes
// to the default CPU generator. Recording never consumes the generator,
// so at record time of each RNG op the full generator state is hashed:
// an unchanged hash means "same segment, next slot", a changed hash
// means the user re-seeded (or otherwise perturbed) the generator mid
// construction and a new segment begins there. Each segment derives:
//
//   * a 64-bit Philox nonce = the state hash. Pins are therefore a pure
//     function of the generator state in effect when the op was
//     recorded: torch.manual_seed(S) — before deferred_init OR inside
//     the module builder — fixes the native init bits, exactly like
//     eager init is a function of the generator state at construction,
//     and independently of any ambient (e.g. per-rank) seeding that the
//     in-builder seed overrides. Within one tape, replaying any subset
//     on any rank gives identical bits (partition-invariant sharded
//     materialization).
//   * a state snapshot. CPU stock replay draws from a cursor initialized
//     to the segment snapshot (not from the ambient generator), so a
//     full in-tape-order CPU materialization is bitwise-equal to eager
//     construction, and replay never perturbs the ambient stream.
//
// Session EXIT advances the live CPU generator by one 64-bit draw, the
// way eager construction consumes it: a second session without
// re-seeding hashes a different state and draws an independent stream
// (two unseeded models never collide), while a session entered right
// after torch.manual_seed(S) still sees the pristine state S — so its
// pins and cursors match an eager construction from S bitwise.
struct RngSession {
  bool has_segment = false;
  uint64_t segment_hash = 0;   // raw state hash of the current segment
  uint64_t nonce = 0;          // collision-salted Philox seed in use
  uint64_t next_slot = 1;      // Philox slot within the current segment
  std::vector<uint64_t> raw_hashes;  // for registry release at session end
  // Default CPU generator state; seeded from segment snapshots and
  // advanced only by this session's CPU stock replay, in tape order.
  // Guarded by cursor_mutex: node execution runs without the tape lock,
  // and the swap-draw-swap of the process-global default generator must
  // be atomic per op (stock-CPU RNG replay therefore serializes per
  // session — it consumes one generator stream by definition; the
  // pinned-Philox native paths parallelize freely).
  at::Tensor replay_cursor;
  std::mutex cursor_mutex;
};

thread_local std::shared_ptr<RngSession> current_rng_session;

// Live-segment registry: two sessions OPEN AT THE SAME TIME (concurrent
// threads) that hash the same generator state would otherwise pin the
// same stream — recording consumes nothing, so the shared state cannot
// tell them apart. Concurrent collisions get a salted nonce (and a
// salted replay snapshot); sequential sessions release their entries at
// exit, so re-seeding to the same state later still reproduces exactly.
std::mutex segment_registry_mutex;
std::unordered_map<uint64_t, uint64_t> live_segment_uses;

uint64_t mixSalt(uint64_t h, uint64_t salt) {
  for (int b = 0; b < 8; ++b) {
    h = (h ^ ((salt >> (8 * b)) & 0xff)) * 1099511628211ull;
  }
  return h;
}

bool isRngOpName(const std::string& name) {
  return name == "aten::uniform_" || name == "aten::normal_" ||
         name == "aten::bernoulli_";
}

// Word-at-a-time mix over a generator-state blob (splitmix-style):
// change detection + nonce derivation, not cryptography. Runs once per
// recorded RNG op over the ~5 KB Mersenne state, so byte-at-a-time FNV
// (~5 us per op) would be a measurable recording cost.
uint64_t hashStateBytes(const uint8_t* bytes, int64_t n) {
  uint64_t h = 0x9E3779B97F4A7C15ull ^ static_cast<uint64_t>(n);
  int64_t i = 0;
  for (; i + 8 <= n; i += 8) {
    uint64_t w;
    std::memcpy(&w, bytes + i, 8);
    h ^= w;
    h *= 0xBF58476D1CE4E5B9ull;
    h ^= h >> 29;
  }
  uint64_t tail = 0;
  for (int j = 0; i < n; ++i, ++j) {
    tail |= static_cast<uint64_t>(bytes[i]) << (8 * j);
  }
  h ^= tail;
  h *= 0x94D049BB133111EBull;
  h ^= h >> 32;
  return h;
}

void beginRngSession() {
  current_rng_session = std::make_shared<RngSession>();
}

void endRngSession() {
  // Registry release and the exit-advance must be ONE atomic step with
  // respect to other threads opening segments: otherwise a concurrent
  // thread can snapshot the pre-advance generator state, lose the race
  // to this release, and register the same state hash with salt 0 —
  // pinning the stream this session already used.
  std::lock_guard<std::mutex> reg_lock(segment_registry_mutex);
  if (current_rng_session != nullptr) {
    for (uint64_t h : current_rng_session->raw_hashes) {
      auto it = live_segment_uses.find(h);
      if (it != live_segment_uses.end() && --(it->second) == 0) {
        live_segment_uses.erase(it);
      }
    }
  }
  current_rng_session = nullptr;
  // Consume one draw so the next unseeded session sees a new state
  // (recorded ops keep the session alive through their own references).
  auto gen = at::globalContext().defaultGenerator(c10::DeviceType::CPU);
  std::lock_guard<std::mutex> lock(gen.mutex());
  gen.get<at::CPUGeneratorImpl>()->random64();
}

// Pins (seed, counter-offset) for every recorded RNG op. The pins drive
// the tdx Philox kernels on GPU replay and the slice-materialization fast
// path on any device; plain CPU replay ignores them (it draws from the
// segment's replay cursor for eager bit-parity). When this op opens a new
// segment, `segment_start` receives the segment's generator-state
// snapshot (undefined otherwise).
std::optional<std::pair<uint64_t, uint64_t>> pinPhiloxForOp(
    const std::string& name, at::Tensor* segment_start) {
  if (!isRngOpName(name) || current_rng_session == nullptr) {
    return std::nullopt;
  }
  RngSession& session = *current_rng_session;
  // The registry lock brackets the state snapshot AND the segment
  // registration, and session exit advances the generator under the
  // same lock — so "state hash is live in the registry" and "state has
  // been advanced past" are mutually exclusive, with no window where a
  // second thread can re-pin a just-closed session's stream (gen.mutex
  // nests inside it, same order as endRngSession).
  std::lock_guard<std::mutex> reg_lock(segment_registry_mutex);
  auto gen = at::globalContext().defaultGenerator(c10::DeviceType::CPU);
  at::Tensor state;
  {
    std::lock_guard<std::mutex> lock(gen.mutex());
    state = gen.get_state();  // returns a fresh copy
  }
  const uint64_t h =
      hashStateBytes(state.const_data_ptr<uint8_t>(), state.numel());
  if (!session.has_segment || h != session.segment_hash) {
    session.has_segment = true;
    session.segment_hash = h;
    session.next_slot = 1;
    const uint64_t salt = live_segment_uses[h]++;
    session.raw_hashes.push_back(h);
    session.nonce = salt == 0 ? h : mixSalt(h, salt);
    if (salt != 0) {
      // Concurrent collision: give the CPU stock path a distinct stream
      // too, by snapshotting a generator seeded with the salted nonce.
      auto salted = at::make_generator<at::CPUGeneratorImpl>(session.nonce);
      state = salted.get_state();
    }
    *segment_start = std::move(state);
  }
  return std::make_pair(session.nonce,
                        session.next_slot++ * kPhiloxStridePerOp);
}

struct InputSlot {
  std::optional<OpOutputDescriptor> desc;  // set when the arg was fake
  std::optional<uint32_t> external_version;  // set for real tensor args
  // For fake inputs read from a *different* storage family than this op
  // writes: a record-time snapshot of that family's writers so far. Replay
  // of this op must first replay these (they produced the value the op
  // observed), and holding them here keeps cross-family history alive even
  // after the other family's fakes are gone. Acyclic by construction:
  // every held node has a smaller op_nr.
  std::vector<std::shared_ptr<OpNode>> history;
  // Inference tensors have no version counter, so their mutations cannot
  // be tracked; replay rejects them with a clear error.
  bool inference = false;
};

struct AliasGroup;

struct OpNode {
  uint64_t op_nr = 0;
  std::optional<RecordedOp> op;          // dropped after replay
  std::vector<InputSlot> input_slots;    // tensor visit order over args
  std::vector<c10::Storage> output_storages;  // meta storages, visit order
  // What each output looked like at record time (dtype Undefined for a
  // non-fake output). Survives replay; the chain model needs the dtype a
  // step runs at, which a later set_data or cast hides from the final
  // tensor's metadata.
  struct OutputMeta {
    c10::ScalarType dtype = c10::ScalarType::Undefined;
    c10::Device device{c10::DeviceType::CPU};
    bool contiguous = false;
    // Where the output sits in its storage, in elements: what locates a
    // view (and an in-place op's target) inside the tensor it was taken
    // from.
    int64_t storage_offset = 0;
    int64_t numel = 0;
  };
  std::vector<OutputMeta> output_metas;
  // tdx::set_data only: the producer `self` had BEFORE the assignment.
  // set_data swaps the impl's record for the new value's, so by the time
  // the op is recorded both input slots name the new value's producer;
  // this is what is left of the old lineage. Weak: it lives on only while
  // something else (a `to` that read it, say) still depends on it, which
  // is exactly when it matters.
  std::weak_ptr<OpNode> set_data_prior;
  std::vector<std::weak_ptr<OpNode>> dependents;
  // The storage families this node writes (weak: groups own nodes, never
  // the reverse). Replay collection closes over each collected writer's
  // chronological prefix in these families, so a writer forced into a
  // replay set (e.g. by the clobber rule) can never run before an earlier
  // writer of the same storage.
  std::vector<std::weak_ptr<AliasGroup>> write_groups;
  std::vector<at::Tensor> outputs;  // real tensors after replay
  bool materialized = false;  // Done: outputs valid, frame freed
  // Another thread is executing this node's op with tape_mutex released;
  // threads whose call stacks share the node wait on tape_cv instead of
  // double-replaying. All transitions happen under tape_mutex.
  bool running = false;
};

std::atomic<uint64_t> next_op_nr{1};

// Serializes tape STRUCTURE access: recording (recordOp), call-stack
// construction, node state transitions and recordInfo. Materialization
// runs with the GIL released, so without this a second thread could
// record into or replay from the same node graph mid-walk. The lock is
// NOT held while a node's op actually executes — replay releases it
// around the kernel/compute work and marks the node `running`, so
// disjoint subgraphs materialize concurrently on multiple threads (and
// multiple HIP streams) while threads whose closures share a node wait
// on tape_cv for its single execution. Recursive because a terminal op
// (aten::item) can materialize while a recording is on the stack.
std::recursive_mutex tape_mutex;
std::condition_variable_any tape_cv;

std::shared_ptr<TensorRecord> getRecord(FakeTensorImpl* fake) {
  return std::static_pointer_cast<TensorRecord>(fake->getData(kDeferredKey));
}

void setRecord(FakeTensorImpl* fake, std::shared_ptr<TensorRecord> rec) {
  fake->setData(kDeferredKey, std::move(rec));
}

uint32_t tensorVersion(const at::Tensor& t) {
  return t.unsafeGetTensorImpl()->version_counter().current_version();
}

bool storagesAlias(const c10::Storage& a, const c10::Storage& b) {
  return a && b && a.is_alias_of(b);
}

// ---------------------------------------------------------------------------
// Recording.
// ---------------------------------------------------------------------------

thread_local size_t deferred_level = 0;

bool shouldRecordHere() {
  return deferred_level > 0 &&
         !c10::impl::tls_is_dispatch_key_excluded(kDeferredKey);
}

// Creates an OpNode out of a recorded call frame. `args` is the deep-copied
// pre-execution argument region; `stack`/`rets_begin` point at the
// post-execution return values, whose fake tensors get stamped with this
// node's records.
void recordOp(std::string name,
              std::function<void(torch::jit::Stack&)> run,
              std::vector<c10::IValue> args,
              at::ThreadLocalState tls,
              torch::jit::Stack& stack,
              size_t rets_begin,
              std::optional<std::pair<uint64_t, uint64_t>> philox =
                  std::nullopt,
              std::optional<c10::OperatorHandle> handle = std::nullopt,
              std::weak_ptr<OpNode> set_data_prior = {}) {
  std::lock_guard<std::recursive_mutex> lock{tape_mutex};
  auto node = std::make_shared<OpNode>();
  node->set_data_prior = std::move(set_data_prior);
  node->op_nr = next_op_nr.fetch_add(1, std::memory_order_relaxed);

  // Input pass: capture producer descriptors for fake args (replacing them
  // with undefined placeholders in the saved frame) and version counters
  // for external (real) tensor args.
  std::vector<std::shared_ptr<TensorRecord>> input_records;
  std::vector<c10::Storage> input_storages;
  std::vector<size_t> fake_slot_idx;  // input_slots index per fake input
  {
    torch::jit::Stack args_stack{args.begin(), args.end()};
    mapTensors(args_stack, 0, args_stack.size(),
               [&](const at::Tensor& t) -> at::Tensor {
                 if (auto* fake = asFake(t)) {
                   auto rec = getRecord(fake);
                   TORCH_CHECK(
                       rec != nullptr,
                       "A fake tensor constructed outside of a deferred-init "
                       "context (or stripped of its record) was used in `",
                       name, "` and cannot be recorded.");
                   fake_slot_idx.push_back(node->input_slots.size());
                   node->input_slots.push_back(InputSlot{rec->desc, {}, {}});
                   rec->desc.node->dependents.emplace_back(node);
                   input_records.push_back(std::move(rec));
                   input_storages.push_back(fake->meta_tensor().storage());
                   return at::Tensor{};
                 }
                 if (t.defined() && t.is_inference()) {
                   InputSlot slot;
                   slot.inference = true;
                   node->input_slots.push_back(std::move(slot));
                 } else if (t.defined()) {
                   node->input_slots.push_back(
                       InputSlot{{}, tensorVersion(t), {}});
                 } else {
                   node->input_slots.push_back(InputSlot{});
                 }
                 return t;
               });
    args.assign(args_stack.begin(), args_stack.end());
  }

  node->op = RecordedOp{std::move(name), std::move(run), std::move(args),
                        std::move(tls), philox, std::move(handle)};

  // Output pass: stamp (or restamp) each fake output's record.
  visitTensors(stack, rets_begin, stack.size(), [&](const at::Tensor& t) {
    size_t out_idx = node->output_storages.size();
    auto* fake = asFake(t);
    if (fake == nullptr) {
      node->output_storages.emplace_back();
      node->output_metas.emplace_back();
      return;
    }
    const c10::Storage& out_storage = fake->meta_tensor().storage();
    node->output_storages.push_back(out_storage);
    node->output_metas.push_back(OpNode::OutputMeta{
        fake->meta_tensor().scalar_type(), fake->fake_device(),
        fake->meta_tensor().is_contiguous(),
        fake->meta_tensor().storage_offset(), fake->meta_tensor().numel()});

    auto rec = getRecord(fake);
    if (rec == nullptr) {
      rec = std::make_shared<TensorRecord>();
      setRecord(fake, rec);
    }
    // Restamp IN PLACE: aliased records observe the rewrite through the
    // shared group (fills the role of the reference's view_records_,
    // deferred_init.cc:126-154).
    rec->desc = OpOutputDescriptor{node, out_idx};

    // Alias-group wiring: adopt the group of any aliased fake input (a
    // view adopts its base's family), else keep/create our own, and
    // register this node as a writer of the family's storage.
    if (rec->group == nullptr) {
      for (size_t i = 0; i < input_records.size(); ++i) {
        if (storagesAlias(out_storage, input_storages[i]) &&
            input_records[i]->group != nullptr) {
          rec->group = input_records[i]->group;
          break;
        }
      }
      if (rec->group == nullptr) {
        rec->group = std::make_shared<AliasGroup>();
      }
    }
    if (rec->group->writers.empty() ||
        rec->group->writers.back() != node) {
      rec->group->writers.push_back(node);
      node->write_groups.emplace_back(rec->group);
    }
  });

  // History snapshots: for every fake input whose storage this op does NOT
  // write (a pure read from another family), capture that family's writer
  // list as of now.
  for (size_t i = 0; i < input_records.size(); ++i) {
    bool writes_it = false;
    for (const c10::Storage& out : node->output_storages) {
      if (storagesAlias(out, input_storages[i])) {
        writes_it = true;
        break;
      }
    }
    if (!writes_it && input_records[i]->group != nullptr) {
      node->input_slots[fake_slot_idx[i]].history =
          input_records[i]->group->writers;
    }
  }
}

bool isTerminalOp(const c10::OperatorHandle& op) {
  const auto& name = op.schema().operator_name().name;
  return name == "aten::item" || name == "aten::_local_scalar_dense";
}

// Whole-tensor in-place init ops `(Tensor(a!) self, ...scalars...) ->
// Tensor(a!)`: on a fake self they change no metadata and produce no new
// tensor, so recording can skip the fake-layer walk AND the meta
// redispatch entirely. This matters enormously for throughput: PyTorch
// has no C++ meta kernels for uniform_/normal_ — the Meta key lands in
// the Python-dispatcher _refs decomposition at ~0.5 ms per op, which
// made these two ops ~85% of the host-side cost of recording a 70B tape.
bool isInPlaceInitOp(const c10::OperatorName& name) {
  if (name.name == "aten::uniform_" || name.name == "aten::normal_" ||
      name.name == "aten::zero_") {
    return name.overload_name.empty();
  }
  if (name.name == "aten::fill_") {
    return name.overload_name == "Scalar";
  }
  if (name.name == "aten::bernoulli_") {
    return name.overload_name == "float";
  }
  return false;
}

void deferredInitHandler(const c10::OperatorHandle& op,
                         c10::DispatchKeySet ks,
                         torch::jit::Stack* stack) {
  c10::impl::ExcludeDispatchKeyGuard no_reentry{kDeferredKey};

  const auto& schema = op.schema();
  size_t num_args = schema.arguments().size();
  size_t args_begin = stack->size() - num_args;

  bool has_fake_arg = false;
  visitTensors(*stack, args_begin, args_begin + num_args,
               [&](const at::Tensor& t) {
                 if (auto* fake = asFake(t)) {
                   has_fake_arg = true;
                   TORCH_CHECK(
                       getRecord(fake) != nullptr,
                       "A fake tensor without a deferred-init record was "
                       "passed to `", schema.operator_name(),
                       "`. Only tensors constructed inside `deferred_init()` "
                       "can be used here.");
                 }
               });

  const auto below =
      ks & c10::DispatchKeySet{c10::DispatchKeySet::FULL_AFTER, kDeferredKey};

  // Terminal ops need real data (e.g. aten::item): materialize the fake
  // arguments eagerly and run for real (reference deferred_init.cc:813-815).
  if (has_fake_arg && isTerminalOp(op)) {
    mapTensors(*stack, args_begin, args_begin + num_args,
               [&](const at::Tensor& t) -> at::Tensor {
                 return isFake(t) ? materializeTensor(t) : t;
               });
    op.redispatchBoxed(below, stack);
    return;
  }

  auto saved = copyStackRegion(*stack, args_begin, args_begin + num_args);
  at::ThreadLocalState tls;  // DeferredInit is excluded in this snapshot

  // Fast path for whole-tensor in-place init on a fake self: the op
  // neither changes metadata nor creates tensors, so skip the fake-layer
  // redispatch (and with it the expensive Python-dispatcher meta
  // decompositions of uniform_/normal_). Validation that eager would do
  // on entry is performed here so errors still surface at record time.
  bool fast_inplace = false;
  if (has_fake_arg && isInPlaceInitOp(schema.operator_name()) &&
      (*stack)[args_begin].isTensor()) {
    const at::Tensor& self = (*stack)[args_begin].toTensor();
    // Autograd-visible mutations (in-place on a requires_grad tensor
    // under grad mode) must keep going through the autograd layer so
    // eager's semantics — the leaf-mutation error, version bumps —
    // surface at record time exactly as they would eagerly.
    if (isFake(self) &&
        (!self.requires_grad() || !c10::GradMode::is_enabled())) {
      const auto& opname = schema.operator_name().name;
      if (opname == "aten::uniform_" || opname == "aten::normal_") {
        TORCH_CHECK(c10::isFloatingType(self.scalar_type()), "`", opname,
                    "` expects a floating-point tensor, got ",
                    self.scalar_type());
      }
      if (opname == "aten::normal_" && num_args >= 3 &&
          (*stack)[args_begin + 2].isDouble()) {
        const double std = (*stack)[args_begin + 2].toDouble();
        TORCH_CHECK(std >= 0.0,
                    "normal_ expects std >= 0.0, but found std=", std);
      }
      if (opname == "aten::bernoulli_" && num_args >= 2 &&
          (*stack)[args_begin + 1].isDouble()) {
        const double p = (*stack)[args_begin + 1].toDouble();
        TORCH_CHECK(0.0 <= p && p <= 1.0,
                    "bernoulli_ expects 0 <= p <= 1, but found p=", p);
      }
      fast_inplace = true;
    }
  }

  if (fast_inplace) {
    c10::IValue self_iv = (*stack)[args_begin];
    stack->resize(args_begin);
    stack->push_back(std::move(self_iv));
  } else {
    // Factory calls (no tensor inputs) with dtype=None resolve the dtype
    // at execution time from the process-global default. Pin the default
    // that is in effect NOW into the recorded frame, so replay is
    // faithful even after torch.set_default_dtype() changes (for
    // non-factories None means "follow the input tensor" and must stay
    // None).
    bool has_tensor_arg = false;
    visitTensors(*stack, args_begin, args_begin + num_args,
                 [&](const at::Tensor& t) {
                   has_tensor_arg = has_tensor_arg || t.defined();
                 });
    if (!has_tensor_arg) {
      const auto& schema_args = schema.arguments();
      for (size_t i = 0; i < schema_args.size(); ++i) {
        if (schema_args[i].name() == "dtype" && saved[i].isNone()) {
          // NB: schema .type() erases ScalarType to int; the semantic
          // type lives in .real_type().
          const auto* type = schema_args[i].real_type().get();
          if (type->kind() == c10::TypeKind::OptionalType &&
              type->castRaw<c10::OptionalType>()->getElementType()->kind() ==
                  c10::TypeKind::ScalarTypeType) {
            saved[i] = c10::IValue{c10::get_default_dtype_as_scalartype()};
          }
        }
      }
    }

    // Execute through the fake layer: shape/dtype work happens on the
    // meta backend and fake tensors come back.
    op.redispatchBoxed(below.add(kFakeKey), stack);
  }

  size_t rets_begin = stack->size() - schema.returns().size();
  bool has_fake_ret = false;
  visitTensors(*stack, rets_begin, stack->size(), [&](const at::Tensor& t) {
    has_fake_ret = has_fake_ret || isFake(t);
  });

  if (has_fake_arg || has_fake_ret) {
    at::Tensor segment_start;
    auto philox = pinPhiloxForOp(schema.operator_name().name, &segment_start);
    // RNG ops additionally carry their session (and, for the first op of
    // a segment, the segment's generator-state snapshot) for the CPU
    // replay cursor.
    std::shared_ptr<RngSession> session =
        philox.has_value() ? current_rng_session : nullptr;
    recordOp(
        schema.operator_name().name,
        [handle = op, philox, session,
         segment_start](torch::jit::Stack& s) {
          // Replay hot path: recorded init ops whose target lives on the
          // GPU run through the hand-written CDNA4 kernels (tdx::) when
          // the _K extension is loaded. The pinned Philox state makes the
          // result independent of which rank replays which subset.
          if (tryNativeInitRedirect(handle, s, philox)) {
            return;
          }
          if (session != nullptr && !s.empty() && s.front().isTensor()) {
            // CPU stock replay of a session RNG op: draw from the
            // segment's replay cursor instead of the ambient generator,
            // so in-tape-order materialization reproduces eager bits and
            // the ambient stream is left untouched. Ops recorded with an
            // explicit generator keep consuming that generator.
            const at::Tensor& self = s.front().toTensor();
            bool explicit_gen = false;
            for (const c10::IValue& v : s) {
              explicit_gen = explicit_gen || v.isGenerator();
            }
            if (self.defined() && self.is_cpu() && !explicit_gen) {
              std::lock_guard<std::mutex> cursor_lock{session->cursor_mutex};
              if (segment_start.defined()) {
                session->replay_cursor = segment_start;
              }
              if (session->replay_cursor.defined()) {
                auto gen = at::globalContext().defaultGenerator(
                    c10::DeviceType::CPU);
                auto swap_state = [&gen](const at::Tensor& st) {
                  std::lock_guard<std::mutex> lock(gen.mutex());
                  at::Tensor prev = gen.get_state();
                  gen.set_state(st);
                  return prev;
                };
                at::Tensor ambient = swap_state(session->replay_cursor);
                handle.callBoxed(s);
                session->replay_cursor = swap_state(ambient);
                return;
              }
              // Out-of-tape-order replay reached a mid-segment op before
              // its segment head: CPU bits for such partial replays are
              // unspecified; draw from the ambient generator.
            }
          }
          handle.callBoxed(s);
        },
        std::move(saved), std::move(tls), *stack, rets_begin, philox, op);
  }
}

TORCH_LIBRARY_IMPL(_, DeferredInit, m) {
  m.fallback(torch::CppFunction::makeFromBoxedFunction<&deferredInitHandler>());
}

// ---------------------------------------------------------------------------
// VariableHooks proxy: `.data` reads and writes bypass the dispatcher, so a
// recording proxy is swapped in for the duration of deferred-init
// (reference deferred_init.cc:889-948, 1050-1128; design note in the
// reference docs fake_tensor_and_deferred_init.rst:153-188).
// ---------------------------------------------------------------------------

class ProxyVariableHooks final : public at::impl::VariableHooksInterface {
 public:
  explicit ProxyVariableHooks(at::impl::VariableHooksInterface* inner)
      : inner_{inner} {}

  at::TensorBase variable_data(const at::TensorBase& self) const override;
  void set_data(const at::TensorBase& self,
                const at::TensorBase& new_data) const override;
  at::TensorBase data(const at::TensorBase& self) const override {
    // Route through variable_data so `.data` reads are recorded too.
    return variable_data(self);
  }

  at::TensorBase tensor_data(const at::TensorBase& t) const override {
    return inner_->tensor_data(t);
  }
  const std::shared_ptr<torch::autograd::Node>& grad_fn(
      const at::TensorBase& t) const override {
    return inner_->grad_fn(t);
  }
  unsigned _register_hook(
      const at::TensorBase& t,
      std::function<at::TensorBase(const at::TensorBase&)> hook)
      const override {
    return inner_->_register_hook(t, std::move(hook));
  }
  void remove_hook(const at::TensorBase& t, unsigned pos) const override {
    inner_->remove_hook(t, pos);
  }
  bool is_view(const at::TensorBase& t) const override {
    return inner_->is_view(t);
  }
  const at::TensorBase& base(const at::TensorBase& t) const override {
    return inner_->base(t);
  }
  const std::string& name(const at::TensorBase& t) const override {
    return inner_->name(t);
  }
  bool is_leaf(const at::TensorBase& t) const override {
    return inner_->is_leaf(t);
  }
  int64_t output_nr(const at::TensorBase& t) const override {
    return inner_->output_nr(t);
  }
  int64_t _version(const at::TensorBase& t) const override {
    return inner_->_version(t);
  }
  void retain_grad(const at::TensorBase& t) const override {
    inner_->retain_grad(t);
  }
  bool retains_grad(const at::TensorBase& t) const override {
    return inner_->retains_grad(t);
  }
  void _backward(const at::Tensor& t,
                 at::TensorList inputs,
                 const std::optional<at::Tensor>& gradient,
                 std::optional<bool> keep_graph,
                 bool create_graph) const override {
    inner_->_backward(t, inputs, gradient, keep_graph, create_graph);
  }
  void requires_grad_(const at::TensorBase& t, bool value) const override {
    inner_->requires_grad_(t, value);
  }
  void basic_autograd_not_implemented_fallback(
      const c10::OperatorHandle& op,
      c10::DispatchKeySet dispatch_keys,
      torch::jit::Stack* stack) const override {
    inner_->basic_autograd_not_implemented_fallback(op, dispatch_keys, stack);
  }
  std::optional<c10::ScalarType> grad_dtype(
      const at::TensorBase& t) const override {
    return inner_->grad_dtype(t);
  }
  void set_grad_dtype(
      const at::TensorBase& t,
      const std::optional<c10::ScalarType>& dtype) const override {
    inner_->set_grad_dtype(t, dtype);
  }

  at::impl::VariableHooksInterface* inner() const noexcept {
    return inner_;
  }

  void setInner(at::impl::VariableHooksInterface* inner) noexcept {
    inner_ = inner;
  }

 private:
  at::impl::VariableHooksInterface* inner_;
};

std::mutex hooks_mutex;
size_t hooks_refcount = 0;
at::impl::VariableHooksInterface* saved_hooks = nullptr;
// Never freed: a thread that fetched the global hooks pointer just
// before the last session left (e.g. replaying a recorded
// tdx::variable_data op, which calls through the hooks) may still be
// mid-call when the stock hooks are restored — deleting the proxy there
// is a use-after-free. The proxy forwards to the real hooks and records
// nothing outside an active session, so keeping the one object alive
// for the process lifetime is both safe and semantically inert.
ProxyVariableHooks* proxy_hooks = nullptr;

void installProxyHooks() {
  std::lock_guard<std::mutex> lock{hooks_mutex};
  if (hooks_refcount++ == 0) {
    at::impl::VariableHooksInterface* current = at::impl::GetVariableHooks();
    TORCH_INTERNAL_ASSERT(current != proxy_hooks);
    saved_hooks = current;
    if (proxy_hooks == nullptr) {
      proxy_hooks = new ProxyVariableHooks{saved_hooks};
    } else {
      proxy_hooks->setInner(saved_hooks);
    }
    at::impl::SetVariableHooks(proxy_hooks);
  }
}

void removeProxyHooks() {
  std::lock_guard<std::mutex> lock{hooks_mutex};
  TORCH_INTERNAL_ASSERT(hooks_refcount > 0);
  if (--hooks_refcount == 0) {
    at::impl::SetVariableHooks(saved_hooks);
  }
}

at::TensorBase ProxyVariableHooks::variable_data(
    const at::TensorBase& self) const {
  at::TensorBase out_base = inner_->variable_data(self);
  at::Tensor self_t{self};
  if (!shouldRecordHere() || !isFake(self_t)) {
    return out_base;
  }
  auto* self_fake = asFake(self_t);
  if (getRecord(self_fake) == nullptr) {
    return out_base;
  }
  at::Tensor out{out_base};
  torch::jit::Stack rets{c10::IValue{out}};
  std::vector<c10::IValue> args{c10::IValue{self_t}};
  recordOp(
      "tdx::variable_data",
      [](torch::jit::Stack& s) {
        at::Tensor in = s.back().toTensor();
        s.pop_back();
        s.emplace_back(in.variable_data());
      },
      std::move(args), at::ThreadLocalState{}, rets, 0);
  return out;
}

void ProxyVariableHooks::set_data(const at::TensorBase& self,
                                  const at::TensorBase& new_data) const {
  at::Tensor self_t{self};
  at::Tensor new_t{new_data};
  bool record = shouldRecordHere() && isFake(self_t) &&
                getRecord(asFake(self_t)) != nullptr;
  std::vector<c10::IValue> args;
  std::weak_ptr<OpNode> prior;
  if (record) {
    // Capture the pre-mutation producer of `self` before the impl swap.
    args = {c10::IValue{self_t}, c10::IValue{new_t}};
    std::lock_guard<std::recursive_mutex> lock{tape_mutex};
    prior = getRecord(asFake(self_t))->desc.node;
  }
  inner_->set_data(self, new_data);
  if (!record) {
    return;
  }
  torch::jit::Stack rets{c10::IValue{self_t}};
  recordOp(
      "tdx::set_data",
      [](torch::jit::Stack& s) {
        at::Tensor nd = s.back().toTensor();
        s.pop_back();
        at::Tensor slf = s.back().toTensor();
        s.pop_back();
        slf.set_data(nd);
        s.emplace_back(slf);
      },
      std::move(args), at::ThreadLocalState{}, rets, 0, std::nullopt,
      std::nullopt, std::move(prior));
}

// ---------------------------------------------------------------------------
// Materialization.
// ---------------------------------------------------------------------------

// Does `node` produce (as one of its outputs) a tensor aliasing `storage`?
bool outputsAlias(const OpNode& node, const c10::Storage& storage) {
  for (const c10::Storage& s : node.output_storages) {
    if (storagesAlias(s, storage)) {
      return true;
    }
  }
  return false;
}

// The ordered replay set for the tensor behind `rec` (fills the role of
// the reference's buildCallStack + getLastInPlaceOpNode,
// deferred_init.cc:506-622, but is driven by the alias group instead of a
// dependents walk — a dependents walk cannot reach in-place writes made to
// a *base* after a view was taken, since those hang off the base's
// producer, not the view node):
//   1. every writer of the target's storage family (from the AliasGroup),
//      with their dependency closures and cross-family history snapshots;
//   2. to fixpoint, dependents of collected nodes whose inputs a collected
//      later writer would clobber — they must replay now, in chronological
//      position, or they would later observe post-overwrite values.
struct CallStack {
  std::vector<std::shared_ptr<OpNode>> nodes;
  std::unordered_set<OpNode*> members;

  void addWithDeps(const std::shared_ptr<OpNode>& n) {
    if (!members.insert(n.get()).second) {
      return;
    }
    nodes.push_back(n);
    for (const InputSlot& slot : n->input_slots) {
      if (slot.desc.has_value()) {
        addWithDeps(slot.desc->node);
      }
      for (const auto& h : slot.history) {
        addWithDeps(h);
      }
    }
    // Chronological-prefix closure: every earlier writer of every family
    // this node writes must replay before it.
    for (const auto& wg : n->write_groups) {
      if (auto group = wg.lock()) {
        for (const auto& w : group->writers) {
          if (w->op_nr < n->op_nr) {
            addWithDeps(w);
          }
        }
      }
    }
  }
};

std::vector<std::shared_ptr<OpNode>> buildCallStack(const TensorRecord& rec) {
  CallStack cs;
  uint64_t horizon = 0;
  if (rec.group != nullptr) {
    for (const auto& w : rec.group->writers) {
      horizon = std::max(horizon, w->op_nr);
      cs.addWithDeps(w);
    }
  } else {
    cs.addWithDeps(rec.desc.node);
    horizon = rec.desc.node->op_nr;
  }

  bool changed = true;
  while (changed) {
    changed = false;
    // Snapshot: addWithDeps mutates cs.nodes.
    std::vector<std::shared_ptr<OpNode>> snapshot = cs.nodes;
    for (const auto& n : snapshot) {
      for (const auto& wd : n->dependents) {
        auto d = wd.lock();
        if (!d || cs.members.count(d.get()) != 0 || d->materialized ||
            d->op_nr > horizon) {
          continue;
        }
        // Clobber rule: `d` reads an output of a collected node whose
        // storage a collected later op overwrites.
        bool include = false;
        for (const InputSlot& slot : d->input_slots) {
          if (!slot.desc.has_value() ||
              cs.members.count(slot.desc->node.get()) == 0) {
            continue;
          }
          const c10::Storage& s =
              slot.desc->node->output_storages[slot.desc->index];
          if (!s) {
            continue;
          }
          for (const auto& w : cs.nodes) {
            if (w->op_nr > d->op_nr && w.get() != slot.desc->node.get() &&
                outputsAlias(*w, s)) {
              include = true;
              break;
            }
          }
          if (include) {
            break;
          }
        }
        if (include) {
          cs.addWithDeps(d);
          changed = true;
        }
      }
    }
  }

  std::sort(cs.nodes.begin(), cs.nodes.end(),
            [](const auto& a, const auto& b) { return a->op_nr < b->op_nr; });
  return cs.nodes;
}

// Rebuilds a replay stack for `node` from its saved frame, substituting
// materialized dependency outputs for fake placeholders and validating
// external tensors (reference materializeArguments,
// deferred_init.cc:640-667).
torch::jit::Stack materializeArguments(OpNode& node) {
  torch::jit::Stack stack{node.op->args.begin(), node.op->args.end()};
  size_t visit = 0;
  mapTensors(stack, 0, stack.size(), [&](const at::Tensor& t) -> at::Tensor {
    const InputSlot& slot = node.input_slots.at(visit++);
    if (slot.desc.has_value()) {
      const OpOutputDescriptor& dep = *slot.desc;
      TORCH_INTERNAL_ASSERT(dep.node->materialized,
                            "deferred-init replay ordering bug: dependency "
                            "not yet materialized");
      return dep.node->outputs.at(dep.index);
    }
    TORCH_CHECK(!slot.inference,
                "An inference tensor was used while recording `",
                node.op->name,
                "`; in-place updates to inference tensors cannot be "
                "tracked, so the tape cannot be replayed faithfully.");
    if (t.defined() && slot.external_version.has_value()) {
      TORCH_CHECK(tensorVersion(t) == *slot.external_version,
                  "The external tensor used by the recorded op `",
                  node.op->name,
                  "` was modified in place after recording; the tape can no "
                  "longer be replayed faithfully.");
    }
    return t;
  });
  return stack;
}

// Ensures `node` is Done before returning. Called with `lock` held (at
// recursion depth 1); releases the tape lock around the op execution so
// other threads can build call stacks, record, and run disjoint nodes
// concurrently. If another thread is already executing the node, waits
// for it instead of double-replaying.
void replayNode(std::unique_lock<std::recursive_mutex>& lock,
                const std::shared_ptr<OpNode>& node) {
  while (node->running) {
    tape_cv.wait(lock);
  }
  if (node->materialized) {
    return;
  }
  TORCH_CHECK(node->op.has_value(),
              "This deferred-init tape segment has already been freed and "
              "cannot be replayed again.");
  // Dependencies are Done (the caller replays in chronological order and
  // waits on in-flight nodes), so the argument stack can be built now.
  torch::jit::Stack stack = materializeArguments(*node);
  node->running = true;
  lock.unlock();
  try {
    at::ThreadLocalStateGuard tls_guard{node->op->tls};
    // Replay must run for real regardless of any ambient fake/deferred
    // mode captured in the snapshot or active on this thread.
    c10::impl::ExcludeDispatchKeyGuard no_deferred{kDeferredKey};
    c10::impl::ExcludeDispatchKeyGuard no_fake{kFakeKey};
    node->op->run(stack);
  } catch (...) {
    lock.lock();
    node->running = false;
    tape_cv.notify_all();
    throw;
  }
  lock.lock();
  node->running = false;
  node->outputs.clear();
  visitTensors(stack, 0, stack.size(),
               [&](const at::Tensor& t) { node->outputs.push_back(t); });
  node->materialized = true;
  // Free the tape incrementally: drop the call frame and the dependency
  // edges (reference detachDependencies, deferred_init.cc:524).
  node->op.reset();
  node->input_slots.clear();
  node->input_slots.shrink_to_fit();
  tape_cv.notify_all();
}

}  // namespace

void enterDeferredInit() {
  if (deferred_level++ == 0) {
    beginRngSession();
    c10::impl::tls_set_dispatch_key_included(kDeferredKey, true);
    installProxyHooks();
  }
}

void leaveDeferredInit() {
  TORCH_CHECK(deferred_level > 0, "Not in a deferred-init context.");
  if (--deferred_level == 0) {
    c10::impl::tls_set_dispatch_key_included(kDeferredKey, false);
    removeProxyHooks();
    endRngSession();
  }
}

bool isDeferredInitActive() noexcept {
  return deferred_level > 0;
}

NoDeferredInit::NoDeferredInit()
    : prev_{c10::impl::tls_is_dispatch_key_excluded(kDeferredKey)} {
  c10::impl::tls_set_dispatch_key_excluded(kDeferredKey, true);
}

NoDeferredInit::~NoDeferredInit() {
  c10::impl::tls_set_dispatch_key_excluded(kDeferredKey, prev_);
}

bool canMaterialize(const at::Tensor& tensor) noexcept {
  auto* fake = asFake(tensor);
  return fake != nullptr && getRecord(fake) != nullptr;
}

std::optional<RecordInfo> recordInfo(const at::Tensor& tensor) {
  std::lock_guard<std::recursive_mutex> lock{tape_mutex};
  auto* fake = asFake(tensor);
  if (fake == nullptr) {
    return std::nullopt;
  }
  auto rec = getRecord(fake);
  if (rec == nullptr) {
    return std::nullopt;
  }
  RecordInfo info;
  const auto& node = rec->desc.node;
  info.op_nr = node->op_nr;
  info.output_index = rec->desc.index;
  info.materialized = node->materialized;
  if (node->op.has_value()) {
    info.op_name = node->op->name;
  }
  if (!node->materialized) {
    for (const auto& n : buildCallStack(*rec)) {
      if (!n->materialized) {
        ++info.pending_ops;
      }
    }
  }
  return info;
}

namespace {

bool chainNameIs(const std::string& name, const char* prefix) {
  return name.rfind(prefix, 0) == 0;
}

// One value-affecting step of a simple init chain.
struct ChainStep {
  enum class Kind {
    kFactory,
    kUniform,
    kNormal,
    kBernoulli,
    kFill,
    kZero,
    kPass,
    // Elementwise op with only scalar parameters (erfinv_/mul_/add_/
    // clamp_/...): slicing commutes with it, so a shard just applies the
    // same op. This is what makes trunc_normal_-style init chains
    // (uniform_ -> erfinv_ -> mul_ -> add_ -> clamp_) slice-
    // materializable.
    kPointwise,
    // Out-of-place dtype conversion on the same device (aten::to /
    // aten::_to_copy, strided, contiguous source): elementwise, so slicing
    // commutes with it. The steps before it run at `dtype`, the steps
    // after it at `cast_to`.
    kCast,
  } kind;
  // The dtype the step runs at: its output's for everything but kCast,
  // whose `dtype` is the SOURCE dtype and `cast_to` the result's.
  c10::ScalarType dtype = c10::ScalarType::Undefined;
  c10::ScalarType cast_to = c10::ScalarType::Undefined;
  // The step's result lives in a new storage (kCast, or a same-dtype
  // copying `to`, which is a kPass): the lineage continues, towards the
  // factory, in `in_storage`.
  bool out_of_place = false;
  c10::Storage in_storage;
  bool is_set_data = false;
  double p0 = 0.0;  // from / mean / fill value
  double p1 = 0.0;  // to / std
  std::optional<std::pair<uint64_t, uint64_t>> philox;
  std::vector<c10::IValue> pointwise_args;  // non-self args for kPointwise
  // Replay closure of the recorded op (boxed call), for kPointwise.
  std::function<void(torch::jit::Stack&)> pointwise_run;
  // Set for a kPointwise step the RNG kernels can apply in registers
  // (fusableTailOp below).
  std::optional<TailOp> tail_op;
  // In-place value and pointwise steps: the extent of the tensor they ran
  // on, as recorded (OpNode::OutputMeta). buildChainSteps compares it with
  // the lineage tensor's own extent.
  bool in_place = false;
  bool target_contiguous = false;
  int64_t target_offset = 0;
  int64_t target_numel = 0;
  // kCast / copying kPass: the extent of the SOURCE tensor in in_storage.
  int64_t in_offset = 0;
  int64_t in_numel = 0;
  // Set by buildChainSteps for a value step on a contiguous proper
  // sub-range of the tensor: it writes flat elements
  // [patch_lo, patch_lo + patch_len) and leaves the rest alone.
  bool patch = false;
  int64_t patch_lo = 0;
  int64_t patch_len = 0;
  std::string name;  // the recorded op, for error messages
};

// A recorded scalar operand of a fusable tail step. Only what ATen turns
// into an opmath_t immediate qualifies: Scalar IValues and wrapped-number
// 0-dim CPU tensors (python scalars). Any other 0-dim tensor operand
// takes part in type promotion differently and is left to ATen.
struct TailOperand {
  bool present = false;  // false: None
  double value = 0.0;
};

std::optional<TailOperand> tailOperand(const c10::IValue& v) {
  TailOperand out;
  if (v.isNone()) {
    return out;
  }
  out.present = true;
  if (v.isDouble()) {
    out.value = v.toDouble();
    return out;
  }
  if (v.isInt()) {
    out.value = static_cast<double>(v.toInt());
    return out;
  }
  if (v.isTensor()) {
    const at::Tensor& t = v.toTensor();
    if (!t.defined() || isFake(t) || t.dim() != 0 || !t.is_cpu() ||
        !t.unsafeGetTensorImpl()->is_wrapped_number()) {
      return std::nullopt;
    }
    // Wrapped python numbers are double or int64 (bool and complex ones
    // are not immediates of these ops). Read in place: no dispatch.
    if (t.scalar_type() == at::kDouble) {
      out.value = *t.const_data_ptr<double>();
    } else if (t.scalar_type() == at::kLong) {
      out.value = static_cast<double>(*t.const_data_ptr<int64_t>());
    } else {
      return std::nullopt;
    }
    return out;
  }
  return std::nullopt;  // bool, complex, symbolic, lists, ...
}

// Maps a kPointwise step to its TailOp when the fused kernels reproduce
// ATen's bits for it. div_/sqrt_/reciprocal_ are excluded (ATen divides
// by a scalar through a host-computed reciprocal), as is any add_/sub_
// with alpha != 1 (ATen may or may not contract a + alpha * b).
std::optional<TailOp> fusableTailOp(const std::string& name,
                                    const std::vector<c10::IValue>& args) {
  std::vector<TailOperand> a;
  for (const c10::IValue& v : args) {
    auto operand = tailOperand(v);
    if (!operand.has_value() ||
        (operand->present && std::isnan(operand->value))) {
      return std::nullopt;
    }
    a.push_back(*operand);
  }
  auto unary = [&](TailOp::Code code) -> std::optional<TailOp> {
    if (!a.empty()) {
      return std::nullopt;
    }
    return TailOp{code, 0.0, 0.0};
  };
  auto one = [&](TailOp::Code code) -> std::optional<TailOp> {
    if (a.size() != 1 || !a[0].present) {
      return std::nullopt;
    }
    return TailOp{code, a[0].value, 0.0};
  };
  if (name == "aten::erfinv_") {
    return unary(TailOp::kErfinv);
  }
  if (name == "aten::neg_") {
    return unary(TailOp::kNeg);
  }
  if (name == "aten::abs_") {
    return unary(TailOp::kAbs);
  }
  if (name == "aten::mul_") {
    // mul_.Tensor with a wrapped number only (what `t.mul_(2.0)`
    // records): mul_.Scalar puts the scalar first, and ATen's CPU kernel
    // then rounds it to a 16-bit tensor dtype before multiplying.
    if (args.size() != 1 || !args[0].isTensor()) {
      return std::nullopt;
    }
    return one(TailOp::kMul);
  }
  if (name == "aten::clamp_min_") {
    return one(TailOp::kClampMin);
  }
  if (name == "aten::clamp_max_") {
    return one(TailOp::kClampMax);
  }
  if (name == "aten::add_" || name == "aten::sub_") {
    if (a.size() != 2 || !a[0].present || !a[1].present ||
        a[1].value != 1.0) {
      return std::nullopt;
    }
    return TailOp{name == "aten::add_" ? TailOp::kAdd : TailOp::kSub,
                  a[0].value, 0.0};
  }
  if (name == "aten::clamp_") {
    if (a.size() != 2 || (!a[0].present && !a[1].present)) {
      return std::nullopt;
    }
    // A one-sided clamp_ is ATen's clamp_min/clamp_max kernel.
    if (!a[1].present) {
      return TailOp{TailOp::kClampMin, a[0].value, 0.0};
    }
    if (!a[0].present) {
      return TailOp{TailOp::kClampMax, a[1].value, 0.0};
    }
    return TailOp{TailOp::kClamp, a[0].value, a[1].value};
  }
  return std::nullopt;
}

// In-place elementwise ops whose only parameters are scalars; slicing
// commutes with all of them.
bool isPointwiseScalarOpName(const std::string& name) {
  static const char* kNames[] = {
      "aten::erfinv_",    "aten::mul_",       "aten::add_",
      "aten::sub_",       "aten::div_",       "aten::clamp_",
      "aten::clamp_min_", "aten::clamp_max_", "aten::neg_",
      "aten::abs_",       "aten::sqrt_",      "aten::reciprocal_",
  };
  for (const char* n : kNames) {
    if (name == n) {
      return true;
    }
  }
  return false;
}

bool isScalarLikeArg(const c10::IValue& v) {
  if (v.isNone() || v.isScalar() || v.isDouble() || v.isInt() ||
      v.isBool()) {
    return true;
  }
  // Python scalars often reach the dispatcher as wrapped-number 0-dim
  // tensors (`t.mul_(2.0)` -> mul_.Tensor). A real 0-dim tensor operand
  // commutes with slicing just like a Scalar; an UNDEFINED tensor here
  // is a nulled-out fake placeholder (a tensor dependency the shard path
  // cannot substitute) and must be rejected.
  if (v.isTensor()) {
    const at::Tensor& t = v.toTensor();
    return t.defined() && t.dim() == 0 && !isFake(t);
  }
  return false;
}

// The op names behind the out-of-place `to` step and the aliasing kPass
// steps; classifyChainNode and setDataFollowsLineage both go by these.
bool isToOpName(const std::string& name) {
  return name == "aten::to" || name == "aten::_to_copy";
}

bool isAliasPassOpName(const std::string& name) {
  return name == "aten::detach" || name == "tdx::variable_data" ||
         name == "aten::alias";
}

// View ops that keep their output inside the input's storage. They are
// pass steps: what matters is the extent of the tensor a later in-place op
// ran on, which that op's own record holds.
bool isViewPassOpName(const std::string& name) {
  static const char* kNames[] = {
      "aten::select",    "aten::slice",   "aten::narrow",
      "aten::view",      "aten::_unsafe_view", "aten::reshape",
      "aten::flatten",   "aten::unflatten",    "aten::squeeze",
      "aten::unsqueeze",
  };
  for (const char* n : kNames) {
    if (name == n) {
      return true;
    }
  }
  return false;
}

bool isFloat3(c10::ScalarType t) {
  return t == at::kFloat || t == at::kBFloat16 || t == at::kHalf;
}

// aten::to (every overload) / aten::_to_copy as a chain step: a kPass when
// it returned its input or copied it at the same dtype, a kCast when the
// dtype changed. Anything that moves the data elsewhere or lays it out
// differently is not a simple chain.
void classifyToNode(const OpNode& node, ChainStep& step) {
  const RecordedOp& op = *node.op;
  auto reject = [&](const char* why) {
    TORCH_CHECK(false, "slice materialization: `", op.name, "` ", why,
                " is not a whole-tensor init op; materialize the tensor "
                "fully instead.");
  };
  if (!op.handle.has_value() || node.input_slots.empty() ||
      !node.input_slots[0].desc.has_value() || node.output_metas.empty() ||
      !node.output_storages[0]) {
    reject("recorded without its schema or source");
  }
  const auto& schema_args = op.handle->schema().arguments();
  for (size_t i = 0; i < schema_args.size() && i < op.args.size(); ++i) {
    const std::string& arg = schema_args[i].name();
    const c10::IValue& v = op.args[i];
    if (arg == "layout") {
      if (!v.isNone() &&
          !(v.isInt() &&
            static_cast<c10::Layout>(v.toInt()) == c10::kStrided)) {
        reject("to a non-strided layout");
      }
    } else if (arg == "pin_memory") {
      if (!v.isNone() && !(v.isBool() && !v.toBool())) {
        reject("into pinned memory");
      }
    } else if (arg == "memory_format") {
      if (!v.isNone()) {
        if (!v.isInt()) {
          reject("to another memory format");
        }
        const auto mf = static_cast<c10::MemoryFormat>(v.toInt());
        if (mf != c10::MemoryFormat::Preserve &&
            mf != c10::MemoryFormat::Contiguous) {
          reject("to another memory format");
        }
      }
    } else if (arg == "other") {
      // to.other: a real tensor only lends its dtype and device; a fake
      // one (nulled out in the frame) would be a second lineage.
      if (!v.isTensor() || !v.toTensor().defined() || isFake(v.toTensor())) {
        reject("to the dtype of another deferred tensor");
      }
    }
  }
  const OpOutputDescriptor& src = *node.input_slots[0].desc;
  if (src.index >= src.node->output_metas.size()) {
    reject("of a source recorded without metadata");
  }
  const OpNode::OutputMeta& in = src.node->output_metas[src.index];
  const OpNode::OutputMeta& out = node.output_metas[0];
  if (in.device != out.device) {
    reject("to another device");
  }
  if (!in.contiguous || !out.contiguous) {
    reject("of a non-contiguous tensor");
  }
  step.dtype = in.dtype;
  const c10::Storage& in_storage = src.node->output_storages[src.index];
  if (storagesAlias(node.output_storages[0], in_storage)) {
    step.kind = ChainStep::Kind::kPass;  // nothing to convert: returned self
    return;
  }
  step.out_of_place = true;
  step.in_storage = in_storage;
  step.in_offset = in.storage_offset;
  step.in_numel = in.numel;
  if (in.dtype == out.dtype) {
    step.kind = ChainStep::Kind::kPass;  // copy=True
    return;
  }
  step.kind = ChainStep::Kind::kCast;
  step.cast_to = out.dtype;
}

ChainStep classifyChainNode(const OpNode& node) {
  TORCH_CHECK(node.op.has_value(),
              "slice materialization: the tape segment for `",
              (node.materialized ? "an already-materialized op"
                                 : "a freed op"),
              "` is gone; materialize the tensor fully instead.");
  const RecordedOp& op = *node.op;
  ChainStep step;
  auto scalarArg = [&](size_t i) -> double {
    const c10::IValue& v = op.args.at(i);
    if (v.isDouble()) {
      return v.toDouble();
    }
    if (v.isInt()) {
      return static_cast<double>(v.toInt());
    }
    if (v.isScalar()) {
      return v.toScalar().toDouble();
    }
    TORCH_CHECK(false, "slice materialization: unexpected argument type `",
                v.tagKind(), "` in `", op.name, "`");
  };
  step.name = op.name;
  if (!node.output_metas.empty()) {
    step.dtype = node.output_metas[0].dtype;
    step.target_offset = node.output_metas[0].storage_offset;
    step.target_numel = node.output_metas[0].numel;
  }
  auto markInPlace = [&] {
    TORCH_CHECK(!node.output_metas.empty() && node.output_storages[0],
                "slice materialization: `", op.name,
                "` was recorded without its target; materialize the tensor "
                "fully instead.");
    const OpNode::OutputMeta& out = node.output_metas[0];
    step.in_place = true;
    step.target_contiguous = out.contiguous;
    step.target_offset = out.storage_offset;
    step.target_numel = out.numel;
  };
  if (isToOpName(op.name)) {
    classifyToNode(node, step);
  } else if (op.name == "tdx::set_data") {
    // `p.data = t`: p continues t's lineage. Whether t is this lineage's
    // own latest value is checked where the whole chain is known
    // (buildChainSteps).
    step.kind = ChainStep::Kind::kPass;
    step.is_set_data = true;
  } else if (chainNameIs(op.name, "aten::empty")) {
    step.kind = ChainStep::Kind::kFactory;
  } else if (chainNameIs(op.name, "aten::zeros")) {
    step.kind = ChainStep::Kind::kZero;
  } else if (chainNameIs(op.name, "aten::ones")) {
    step.kind = ChainStep::Kind::kFill;
    step.p0 = 1.0;
  } else if (chainNameIs(op.name, "aten::full")) {
    step.kind = ChainStep::Kind::kFill;
    step.p0 = scalarArg(1);
  } else if (op.name == "aten::uniform_" || op.name == "aten::normal_" ||
             op.name == "aten::bernoulli_") {
    for (size_t i = 1; i < op.args.size(); ++i) {
      TORCH_CHECK(!op.args[i].isGenerator(),
                  "slice materialization: `", op.name,
                  "` was recorded with an explicit generator, which the "
                  "counter-based shard path cannot honor; materialize the "
                  "tensor fully instead.");
    }
    if (op.name == "aten::bernoulli_") {
      step.kind = ChainStep::Kind::kBernoulli;
      step.p0 = scalarArg(1);
    } else {
      step.kind = op.name == "aten::uniform_" ? ChainStep::Kind::kUniform
                                              : ChainStep::Kind::kNormal;
      step.p0 = scalarArg(1);
      step.p1 = scalarArg(2);
    }
    step.philox = op.philox;
    markInPlace();
  } else if (op.name == "aten::fill_") {
    step.kind = ChainStep::Kind::kFill;
    step.p0 = scalarArg(1);
    markInPlace();
  } else if (op.name == "aten::zero_") {
    step.kind = ChainStep::Kind::kZero;
    markInPlace();
  } else if (isAliasPassOpName(op.name)) {
    step.kind = ChainStep::Kind::kPass;
  } else if (isViewPassOpName(op.name) && !node.input_slots.empty() &&
             node.input_slots[0].desc.has_value() &&
             !node.output_storages.empty() &&
             storagesAlias(
                 node.output_storages[0],
                 node.input_slots[0].desc->node->output_storages.at(
                     node.input_slots[0].desc->index))) {
    step.kind = ChainStep::Kind::kPass;
  } else if (isPointwiseScalarOpName(op.name) &&
             std::all_of(op.args.begin() + 1, op.args.end(),
                         isScalarLikeArg)) {
    step.kind = ChainStep::Kind::kPointwise;
    step.pointwise_args.assign(op.args.begin() + 1, op.args.end());
    step.pointwise_run = op.run;
    step.tail_op = fusableTailOp(op.name, step.pointwise_args);
    markInPlace();
  } else {
    TORCH_CHECK(false, "slice materialization: `", op.name,
                "` is not a whole-tensor init op; materialize the tensor "
                "fully instead.");
  }
  return step;
}

// A dim-d slice of a contiguous tensor, flattened: n_blocks contiguous
// global element ranges of block_len elements, block r starting at
// g_off + r * g_stride. dim 0 is the n_blocks == 1 case and takes the
// flat shard ops (whose boundary handling is tuned for it); dim > 0
// takes the windowed ops.
struct ShardWindow {
  int64_t n_blocks;
  int64_t block_len;
  int64_t g_stride;
  int64_t g_off;
  // Set for an N-d box of two or more levels (materializeTensorBlock),
  // which takes tdx::rng_box_; the four fields above are then unused.
  std::optional<BoxGeometry> box = std::nullopt;
};

int64_t rngDistCode(ChainStep::Kind kind) {
  return kind == ChainStep::Kind::kUniform
             ? 0
             : (kind == ChainStep::Kind::kNormal ? 1 : 2);
}

// One tdx::rng_box_ launch: the RNG step over the box, with `tail` (may
// be empty) applied before the store.
void applyBoxStep(const ChainStep& rng, const std::vector<TailOp>& tail,
                  at::Tensor& shard, const BoxGeometry& box,
                  int64_t full_numel) {
  static const auto rng_box =
      c10::Dispatcher::singleton()
          .findSchemaOrThrow("tdx::rng_box_", "")
          .typed<at::Tensor&(at::Tensor&, at::IntArrayRef, at::IntArrayRef,
                             int64_t, int64_t, int64_t, double, double,
                             at::IntArrayRef, at::ArrayRef<double>,
                             at::ArrayRef<double>, int64_t, int64_t,
                             int64_t)>();
  std::vector<int64_t> ops;
  std::vector<double> s0;
  std::vector<double> s1;
  for (const TailOp& t : tail) {
    ops.push_back(t.op);
    s0.push_back(t.s0);
    s1.push_back(t.s1);
  }
  rng_box.call(shard, at::IntArrayRef(box.extent, box.levels),
               at::IntArrayRef(box.g_stride, box.levels), box.run_len,
               box.g_off, rngDistCode(rng.kind), rng.p0, rng.p1, ops, s0, s1,
               full_numel, static_cast<int64_t>(rng.philox->first),
               static_cast<int64_t>(rng.philox->second));
}

// dist code of a value step in the _DIST_CODE numbering of the batched
// planner and tdx::patch_box_: 0 uniform, 1 normal, 2 bernoulli, 3 fill,
// 4 zero.
int64_t valueDistCode(ChainStep::Kind kind) {
  switch (kind) {
    case ChainStep::Kind::kUniform:
      return 0;
    case ChainStep::Kind::kNormal:
      return 1;
    case ChainStep::Kind::kBernoulli:
      return 2;
    case ChainStep::Kind::kFill:
      return 3;
    default:
      return 4;
  }
}

// One tdx::patch_box_ call: the value step (dist, p0, p1, philox) on flat
// elements [lo, lo + len) of the full tensor, applied to what the window
// (or box) `w` holds of them, at the shard's dtype.
void applyPatchOp(at::Tensor& shard, const ShardWindow& w, int64_t full_numel,
                  int64_t lo, int64_t len, int64_t dist, double p0, double p1,
                  const std::optional<std::pair<uint64_t, uint64_t>>& philox) {
  static const auto patch_box =
      c10::Dispatcher::singleton()
          .findSchemaOrThrow("tdx::patch_box_", "")
          .typed<at::Tensor&(at::Tensor&, at::IntArrayRef, at::IntArrayRef,
                             int64_t, int64_t, int64_t, int64_t, int64_t,
                             int64_t, double, double, std::optional<int64_t>,
                             std::optional<int64_t>)>();
  TORCH_CHECK(dist > 2 || philox.has_value(),
              "slice materialization: this RNG op carries no pinned "
              "Philox state (was it recorded by an older build?)");
  std::optional<int64_t> seed;
  std::optional<int64_t> offset;
  if (philox.has_value()) {
    seed = static_cast<int64_t>(philox->first);
    offset = static_cast<int64_t>(philox->second);
  }
  if (w.box.has_value()) {
    const BoxGeometry& box = *w.box;
    patch_box.call(shard, at::IntArrayRef(box.extent, box.levels),
                   at::IntArrayRef(box.g_stride, box.levels), box.run_len,
                   box.g_off, full_numel, lo, len, dist, p0, p1, seed, offset);
    return;
  }
  // A flat range or single-dim window is the one-level box it is.
  const int64_t extent = w.n_blocks;
  const int64_t stride = std::max(w.g_stride, w.block_len);
  patch_box.call(shard, at::IntArrayRef(&extent, 1),
                 at::IntArrayRef(&stride, 1), w.block_len, w.g_off,
                 full_numel, lo, len, dist, p0, p1, seed, offset);
}

void applyShardStep(const ChainStep& step, at::Tensor& shard,
                    const ShardWindow& w, int64_t full_numel) {
  if (step.patch) {
    applyPatchOp(shard, w, full_numel, step.patch_lo, step.patch_len,
                 valueDistCode(step.kind), step.p0, step.p1, step.philox);
    return;
  }
  switch (step.kind) {
    case ChainStep::Kind::kFactory:
    case ChainStep::Kind::kPass:
      return;
    case ChainStep::Kind::kCast:
      // Replaces the shard; replayChainOnShard splits the chain there.
      TORCH_INTERNAL_ASSERT(false, "kCast is not an in-place shard step");
      return;
    case ChainStep::Kind::kPointwise: {
      torch::jit::Stack s;
      s.emplace_back(shard);
      for (const c10::IValue& a : step.pointwise_args) {
        s.push_back(a);
      }
      c10::impl::ExcludeDispatchKeyGuard no_deferred{kDeferredKey};
      c10::impl::ExcludeDispatchKeyGuard no_fake{kFakeKey};
      step.pointwise_run(s);
      shard = s.back().toTensor();
      return;
    }
    case ChainStep::Kind::kZero:
      shard.zero_();
      return;
    case ChainStep::Kind::kFill:
      shard.fill_(step.p0);
      return;
    case ChainStep::Kind::kUniform:
    case ChainStep::Kind::kNormal:
    case ChainStep::Kind::kBernoulli: {
      TORCH_CHECK(step.philox.has_value(),
                  "slice materialization: this RNG op carries no pinned "
                  "Philox state (was it recorded by an older build?)");
      if (w.box.has_value()) {
        applyBoxStep(step, {}, shard, *w.box, full_numel);
        return;
      }
      static const auto uniform_shard =
          c10::Dispatcher::singleton()
              .findSchemaOrThrow("tdx::uniform_shard_", "")
              .typed<at::Tensor&(at::Tensor&, int64_t, int64_t, double,
                                 double, int64_t, int64_t)>();
      static const auto normal_shard =
          c10::Dispatcher::singleton()
              .findSchemaOrThrow("tdx::normal_shard_", "")
              .typed<at::Tensor&(at::Tensor&, int64_t, int64_t, double,
                                 double, int64_t, int64_t)>();
      static const auto bernoulli_shard =
          c10::Dispatcher::singleton()
              .findSchemaOrThrow("tdx::bernoulli_shard_", "")
              .typed<at::Tensor&(at::Tensor&, int64_t, int64_t, double,
                                 int64_t, int64_t)>();
      static const auto uniform_shard_win =
          c10::Dispatcher::singleton()
              .findSchemaOrThrow("tdx::uniform_shard_win_", "")
              .typed<at::Tensor&(at::Tensor&, int64_t, int64_t, int64_t,
                                 int64_t, double, double, int64_t,
                                 int64_t)>();
      static const auto normal_shard_win =
          c10::Dispatcher::singleton()
              .findSchemaOrThrow("tdx::normal_shard_win_", "")
              .typed<at::Tensor&(at::Tensor&, int64_t, int64_t, int64_t,
                                 int64_t, double, double, int64_t,
                                 int64_t)>();
      static const auto bernoulli_shard_win =
          c10::Dispatcher::singleton()
              .findSchemaOrThrow("tdx::bernoulli_shard_win_", "")
              .typed<at::Tensor&(at::Tensor&, int64_t, int64_t, int64_t,
                                 int64_t, double, int64_t, int64_t)>();
      const auto& [seed, offset] = *step.philox;
      const auto s64 = static_cast<int64_t>(seed);
      const auto o64 = static_cast<int64_t>(offset);
      if (w.n_blocks == 1) {
        const int64_t start = w.g_off;
        const int64_t end = w.g_off + w.block_len;
        if (step.kind == ChainStep::Kind::kUniform) {
          uniform_shard.call(shard, start, end, step.p0, step.p1, s64, o64);
        } else if (step.kind == ChainStep::Kind::kNormal) {
          normal_shard.call(shard, start, end, step.p0, step.p1, s64, o64);
        } else {
          bernoulli_shard.call(shard, start, end, step.p0, s64, o64);
        }
      } else if (step.kind == ChainStep::Kind::kUniform) {
        uniform_shard_win.call(shard, w.n_blocks, w.block_len, w.g_stride,
                               w.g_off, step.p0, step.p1, s64, o64);
      } else if (step.kind == ChainStep::Kind::kNormal) {
        normal_shard_win.call(shard, w.n_blocks, w.block_len, w.g_stride,
                              w.g_off, step.p0, step.p1, s64, o64);
      } else {
        bernoulli_shard_win.call(shard, w.n_blocks, w.block_len, w.g_stride,
                                 w.g_off, step.p0, s64, o64);
      }
      return;
    }
  }
}

// One launch for an RNG step and the fusable tail after it: the window
// (or box) op draws the values and applies the tail before its single
// store.
void applyFusedShardStep(const ChainStep& rng, const std::vector<TailOp>& tail,
                         at::Tensor& shard, const ShardWindow& w,
                         int64_t full_numel) {
  TORCH_CHECK(rng.philox.has_value(),
              "slice materialization: this RNG op carries no pinned "
              "Philox state (was it recorded by an older build?)");
  if (w.box.has_value()) {
    applyBoxStep(rng, tail, shard, *w.box, full_numel);
    return;
  }
  static const auto chain_shard_win =
      c10::Dispatcher::singleton()
          .findSchemaOrThrow("tdx::rng_chain_shard_win_", "")
          .typed<at::Tensor&(at::Tensor&, int64_t, int64_t, int64_t, int64_t,
                             int64_t, double, double, at::IntArrayRef,
                             at::ArrayRef<double>, at::ArrayRef<double>,
                             int64_t, int64_t, int64_t)>();
  std::vector<int64_t> ops;
  std::vector<double> s0;
  std::vector<double> s1;
  for (const TailOp& t : tail) {
    ops.push_back(t.op);
    s0.push_back(t.s0);
    s1.push_back(t.s1);
  }
  chain_shard_win.call(shard, w.n_blocks, w.block_len, w.g_stride, w.g_off,
                       rngDistCode(rng.kind), rng.p0, rng.p1, ops, s0, s1,
                       full_numel, static_cast<int64_t>(rng.philox->first),
                       static_cast<int64_t>(rng.philox->second));
}

// applyFusedShardStep for a chain that ends in a conversion: `shard` has
// the FINAL dtype, the values are drawn (and the tail applied) at
// `src_dtype`. Windows only; boxes convert a temporary (replayChainOnShard).
void applyFusedCastShardStep(const ChainStep& rng,
                             const std::vector<TailOp>& tail,
                             c10::ScalarType src_dtype, at::Tensor& shard,
                             const ShardWindow& w, int64_t full_numel) {
  TORCH_CHECK(rng.philox.has_value(),
              "slice materialization: this RNG op carries no pinned "
              "Philox state (was it recorded by an older build?)");
  static const auto chain_cast_shard_win =
      c10::Dispatcher::singleton()
          .findSchemaOrThrow("tdx::rng_chain_cast_shard_win_", "")
          .typed<at::Tensor&(at::Tensor&, at::ScalarType, int64_t, int64_t,
                             int64_t, int64_t, int64_t, double, double,
                             at::IntArrayRef, at::ArrayRef<double>,
                             at::ArrayRef<double>, int64_t, int64_t,
                             int64_t)>();
  std::vector<int64_t> ops;
  std::vector<double> s0;
  std::vector<double> s1;
  for (const TailOp& t : tail) {
    ops.push_back(t.op);
    s0.push_back(t.s0);
    s1.push_back(t.s1);
  }
  chain_cast_shard_win.call(shard, src_dtype, w.n_blocks, w.block_len,
                            w.g_stride, w.g_off, rngDistCode(rng.kind),
                            rng.p0, rng.p1, ops, s0, s1, full_numel,
                            static_cast<int64_t>(rng.philox->first),
                            static_cast<int64_t>(rng.philox->second));
}

// The shard converted to `dtype`: tdx::copy_ (bitwise ATen's conversion)
// between two of {f32, bf16, f16}, ATen's `to` for anything else (an fp8
// destination, a double source).
at::Tensor castShard(const at::Tensor& shard, c10::ScalarType dtype) {
  c10::impl::ExcludeDispatchKeyGuard no_deferred{kDeferredKey};
  c10::impl::ExcludeDispatchKeyGuard no_fake{kFakeKey};
  if (!isFloat3(shard.scalar_type()) || !isFloat3(dtype)) {
    return shard.to(dtype);
  }
  static const auto copy =
      c10::Dispatcher::singleton()
          .findSchemaOrThrow("tdx::copy_", "")
          .typed<at::Tensor&(at::Tensor&, const at::Tensor&, bool)>();
  at::Tensor out = at::empty(shard.sizes(), shard.options().dtype(dtype));
  copy.call(out, shard, false);
  return out;
}

// Whether `op` on a tensor of `dtype` and `numel` elements may fuse in
// the current switch state: everything in the fusable set, except the
// steps that are NOT bitwise equal to ATen's kernels on gfx950, which
// need the explicit opt-in (fusedInitChainsExplicit):
//  * erfinv_ on float32: 1-2 ulp on about half of all inputs.
//  * mul_ on float16 tensors of 2^31 elements or more. ATen's f16
//    multiply rounds differently in the last, partial block of its
//    elementwise kernel; the fused kernels reproduce that from the
//    tensor's element count (csrc/hip/init_kernels.hip tailMul), but
//    ATen splits tensors too large for 32-bit indexing into several
//    launches, whose block boundaries are not reproduced.
bool tailOpAdmitted(const TailOp& op, c10::ScalarType dtype, int64_t numel) {
  const bool inexact =
      (op.op == TailOp::kErfinv && dtype == at::kFloat) ||
      (op.op == TailOp::kMul && dtype == at::kHalf &&
       numel > std::numeric_limits<int32_t>::max());
  return !inexact || fusedInitChainsExplicit();
}

// The steps that set every element they run on, whatever it held before.
bool isValueStep(const ChainStep& step) {
  return step.kind == ChainStep::Kind::kUniform ||
         step.kind == ChainStep::Kind::kNormal ||
         step.kind == ChainStep::Kind::kBernoulli ||
         step.kind == ChainStep::Kind::kFill ||
         step.kind == ChainStep::Kind::kZero;
}

bool isRngStep(const ChainStep& step) {
  return step.kind == ChainStep::Kind::kUniform ||
         step.kind == ChainStep::Kind::kNormal ||
         step.kind == ChainStep::Kind::kBernoulli;
}

// `p.data = t` keeps a chain simple only when t is this lineage's own
// latest value: walking back from t's producer through conversions and
// aliasing pass-throughs (producer edges, not tape positions) must arrive
// at the producer p had before it was assigned (OpNode::set_data_prior),
// and nothing but pass steps may sit between t's producer and the
// assignment. After `p.data = other` p shares other's record, so without
// this check it would silently plan and slice as other's lineage.
bool setDataFollowsLineage(const std::vector<std::shared_ptr<OpNode>>& nodes,
                           const std::vector<ChainStep>& steps, size_t i) {
  const OpNode& node = *nodes[i];
  const std::shared_ptr<OpNode> prior = node.set_data_prior.lock();
  if (prior == nullptr || node.input_slots.size() != 2 ||
      !node.input_slots[1].desc.has_value()) {
    return false;
  }
  const OpNode* self_producer = prior.get();
  const OpNode* data_producer = node.input_slots[1].desc->node.get();
  size_t at = i;
  while (at > 0 && nodes[at - 1].get() != data_producer) {
    --at;
    if (steps[at].kind != ChainStep::Kind::kPass || steps[at].out_of_place) {
      return false;
    }
  }
  if (at == 0) {
    return false;
  }
  // A producer is always recorded before its consumer, so op_nr falls
  // with every hop and the walk ends at, or passes, self_producer.
  const OpNode* cur = data_producer;
  while (cur != self_producer) {
    if (cur->op_nr < self_producer->op_nr || !cur->op.has_value() ||
        !(isToOpName(cur->op->name) || isAliasPassOpName(cur->op->name)) ||
        cur->input_slots.empty() || !cur->input_slots[0].desc.has_value()) {
      return false;
    }
    cur = cur->input_slots[0].desc->node.get();
  }
  return true;
}

// The tensor's replay set as chain steps, in tape order, reduced to its
// own lineage. Throws (c10::Error, "slice materialization: ...") when the
// tape is not a simple init chain.
//
// Until a conversion enters the picture every step acts on one storage
// and the replay set IS the lineage. A `to` makes a second storage: the
// walk goes backwards from the final tensor's storage, crosses a
// conversion into its source's storage, and drops conversions that
// produced some OTHER tensor (the replay set pulls in `h = p.half()` when
// p is overwritten afterwards; h is no part of p).
//
// In-place steps are placed by the extent of the tensor they ran on,
// relative to the lineage tensor's own [offset, offset + numel) in the
// storage the step acts on:
//  * the whole tensor, contiguously: a whole-tensor step, as recorded on
//    the tensor itself (`w.view(-1).normal_()` is `w.normal_()`);
//  * a contiguous proper sub-range, for a value step: a PATCH
//    (`w[i].zero_()`, `w[:k].normal_()`), honoured in tape order;
//  * nothing of the tensor (a sibling view of a shared buffer): dropped;
//  * anything else (a strided view, a pointwise op on a sub-view, a
//    range that only partly covers the tensor) throws.
// A whole-tensor value step makes every earlier patch dead (it becomes a
// pass step); a whole-tensor pointwise step behind a live patch throws.
std::vector<ChainStep> buildChainSteps(const TensorRecord& rec,
                                       const at::Tensor& final_meta) {
  auto nodes = buildCallStack(rec);
  std::vector<ChainStep> all;
  all.reserve(nodes.size());
  for (const auto& n : nodes) {
    all.push_back(classifyChainNode(*n));
  }
  std::vector<char> keep(all.size(), 1);
  std::vector<char> in_lineage(all.size(), 1);
  bool crosses = false;
  c10::Storage cur = final_meta.storage();
  int64_t cur_off = final_meta.storage_offset();
  int64_t cur_numel = final_meta.numel();
  for (size_t i = all.size(); i-- > 0;) {
    const bool in = outputsAlias(*nodes[i], cur);
    in_lineage[i] = in;
    ChainStep& step = all[i];
    if (step.out_of_place) {
      if (!in) {
        keep[i] = 0;
        continue;
      }
      crosses = true;
      cur = step.in_storage;
      cur_off = step.in_offset;
      cur_numel = step.in_numel;
    } else if (step.is_set_data) {
      TORCH_CHECK(in && setDataFollowsLineage(nodes, all, i),
                  "slice materialization: `tdx::set_data` assigns a tensor "
                  "of another lineage, which is not a whole-tensor init op; "
                  "materialize the tensor fully instead.");
    } else if (step.in_place && in) {
      TORCH_CHECK(step.target_contiguous,
                  "slice materialization: `", step.name,
                  "` ran on a non-contiguous view, which is not a "
                  "whole-tensor init op; materialize the tensor fully "
                  "instead.");
      const int64_t lo = step.target_offset - cur_off;
      const int64_t hi = lo + step.target_numel;
      if (lo == 0 && hi == cur_numel) {
        continue;  // the whole tensor
      }
      if (hi <= 0 || lo >= cur_numel || step.target_numel == 0) {
        keep[i] = 0;  // touches nothing of this tensor
        continue;
      }
      TORCH_CHECK(0 <= lo && hi <= cur_numel,
                  "slice materialization: `", step.name,
                  "` ran on a tensor that only partly overlaps this one, "
                  "which is not a whole-tensor init op; materialize the "
                  "tensor fully instead.");
      TORCH_CHECK(step.kind != ChainStep::Kind::kPointwise,
                  "slice materialization: `", step.name,
                  "` on a sub-view is not a whole-tensor init op; "
                  "materialize the tensor fully instead.");
      step.patch = true;
      step.patch_lo = lo;
      step.patch_len = hi - lo;
    }
  }
  std::vector<ChainStep> steps;
  steps.reserve(all.size());
  for (size_t i = 0; i < all.size(); ++i) {
    if (!keep[i]) {
      continue;
    }
    TORCH_CHECK(!crosses || in_lineage[i],
                "slice materialization: the tape mixes a dtype conversion "
                "with ops on another tensor; materialize the tensor fully "
                "instead.");
    steps.push_back(std::move(all[i]));
  }
  // Liveness: patches before the last whole-tensor value step are dead.
  size_t last_whole = 0;
  bool have_whole = false;
  for (size_t i = 0; i < steps.size(); ++i) {
    if (isValueStep(steps[i]) && !steps[i].patch) {
      last_whole = i;
      have_whole = true;
    }
  }
  bool live_patch = false;
  for (size_t i = 0; i < steps.size(); ++i) {
    ChainStep& step = steps[i];
    if (step.patch && have_whole && i < last_whole) {
      ChainStep pass;
      pass.kind = ChainStep::Kind::kPass;
      pass.dtype = step.dtype;
      pass.name = step.name;
      step = std::move(pass);
    } else if (step.patch) {
      live_patch = true;
    } else if (step.kind == ChainStep::Kind::kPointwise) {
      TORCH_CHECK(!live_patch, "slice materialization: `", step.name,
                  "` follows a partial-tensor write, which is not a "
                  "whole-tensor init chain; materialize the tensor fully "
                  "instead.");
    }
  }
  return steps;
}

// A trailing run [RNG step, fusable tail..., pass steps...] of
// steps[lo, hi) that one fused launch can serve. With `allow_cast` the
// run may also hold exactly one kCast between two of {f32, bf16, f16}
// behind the tail (pass steps on either side of it), and the tail may
// then be empty: that is one launch of tdx::rng_chain_cast_shard_win_.
// The tail rules are evaluated at the dtype the tail runs at — the
// cast's SOURCE dtype.
struct FusedRun {
  size_t rng;         // index of the RNG step
  size_t tail_begin;  // [tail_begin, tail_end): the kPointwise steps
  size_t tail_end;
  std::optional<size_t> cast;
};

std::optional<FusedRun> fusedRunStart(const std::vector<ChainStep>& steps,
                                      size_t lo, size_t hi, int64_t numel,
                                      bool allow_cast) {
  if (!fusedInitChainsEnabled()) {
    return std::nullopt;
  }
  size_t end = hi;
  while (end > lo && steps[end - 1].kind == ChainStep::Kind::kPass) {
    --end;
  }
  std::optional<size_t> cast;
  if (allow_cast && end > lo &&
      steps[end - 1].kind == ChainStep::Kind::kCast) {
    cast = --end;
    if (!isFloat3(steps[*cast].cast_to)) {
      return std::nullopt;
    }
    while (end > lo && steps[end - 1].kind == ChainStep::Kind::kPass) {
      --end;
    }
  }
  if (end == lo) {
    return std::nullopt;
  }
  const c10::ScalarType dtype = steps[end - 1].dtype;
  if (!isFloat3(dtype)) {
    return std::nullopt;
  }
  size_t first_tail = end;
  while (first_tail > lo &&
         steps[first_tail - 1].kind == ChainStep::Kind::kPointwise &&
         steps[first_tail - 1].tail_op.has_value() &&
         tailOpAdmitted(*steps[first_tail - 1].tail_op, dtype, numel)) {
    --first_tail;
  }
  const size_t n_tail = end - first_tail;
  if ((n_tail == 0 && !cast.has_value()) || n_tail > kMaxTailOps ||
      first_tail == lo || !isRngStep(steps[first_tail - 1]) ||
      !steps[first_tail - 1].philox.has_value()) {
    return std::nullopt;
  }
  return FusedRun{first_tail - 1, first_tail, end, cast};
}

// double -> `dtype` -> double, the way tdx::fill_ / ATen narrow a Scalar
// into a tensor of that dtype (through float for the 16-bit types).
std::optional<double> roundScalarThrough(double v, c10::ScalarType dtype) {
  switch (dtype) {
    case at::kDouble:
      return v;
    case at::kFloat:
      return static_cast<double>(static_cast<float>(v));
    case at::kBFloat16:
      return static_cast<double>(
          static_cast<float>(c10::BFloat16(static_cast<float>(v))));
    case at::kHalf:
      return static_cast<double>(
          static_cast<float>(c10::Half(static_cast<float>(v))));
    default:
      return std::nullopt;
  }
}

// Shared body of tensorInitPlan (allow_tail == false) and tensorChainPlan.
// With `patches` set, live patches are collected there in application
// order (tensorPatchPlan); without it a chain with a live patch has no
// plan.
std::optional<ChainPlan> chainPlanImpl(const at::Tensor& tensor,
                                       bool allow_tail,
                                       std::vector<PatchStep>* patches =
                                           nullptr) {
  auto* fake = asFake(tensor);
  if (fake == nullptr) {
    return std::nullopt;
  }
  auto rec = getRecord(fake);
  if (rec == nullptr) {
    return std::nullopt;
  }
  const at::Tensor& meta = fake->meta_tensor();
  if (!meta.is_contiguous()) {
    return std::nullopt;
  }
  std::lock_guard<std::recursive_mutex> lock{tape_mutex};
  ChainPlan plan;
  try {
    const std::vector<ChainStep> steps =
        buildChainSteps(*rec, meta);
    // The plan stands for a tensor with a storage of its own: a view of a
    // larger buffer keeps its aliasing only through ordinary replay.
    if (!steps.empty() && !steps.front().in_place &&
        (steps.front().kind == ChainStep::Kind::kFactory ||
         steps.front().kind == ChainStep::Kind::kZero ||
         steps.front().kind == ChainStep::Kind::kFill) &&
        (meta.storage_offset() != 0 ||
         steps.front().target_numel != meta.numel())) {
      return std::nullopt;
    }
    bool have_value = false;
    std::vector<char> patch_before_cast;
    bool tail_unfusable = false;  // a live pointwise step we cannot fuse
    // At most one conversion, and nothing that changes values behind it:
    // the kernels generate at one dtype and store at another, once.
    std::optional<c10::ScalarType> cast_src;
    for (const ChainStep& step : steps) {
      if (step.patch) {
        // Live by construction (buildChainSteps), and behind the tail.
        if (patches == nullptr ||
            (isRngStep(step) && !step.philox.has_value())) {
          return std::nullopt;
        }
        PatchStep ps;
        ps.lo = step.patch_lo;
        ps.len = step.patch_len;
        ps.kind = step.kind == ChainStep::Kind::kUniform
                      ? InitPlan::Kind::kUniform
                      : (step.kind == ChainStep::Kind::kNormal
                             ? InitPlan::Kind::kNormal
                             : (step.kind == ChainStep::Kind::kBernoulli
                                    ? InitPlan::Kind::kBernoulli
                                    : (step.kind == ChainStep::Kind::kFill
                                           ? InitPlan::Kind::kFill
                                           : InitPlan::Kind::kZero)));
        ps.p0 = step.p0;
        ps.p1 = step.p1;
        if (step.philox.has_value()) {
          ps.seed = step.philox->first;
          ps.offset = step.philox->second;
        }
        patches->push_back(ps);
        patch_before_cast.push_back(!cast_src.has_value());
        continue;
      }
      if (cast_src.has_value() && step.kind != ChainStep::Kind::kPass &&
          step.kind != ChainStep::Kind::kFactory) {
        return std::nullopt;
      }
      switch (step.kind) {
        case ChainStep::Kind::kFactory:
        case ChainStep::Kind::kPass:
          break;
        case ChainStep::Kind::kCast:
          cast_src = step.dtype;
          break;
        case ChainStep::Kind::kPointwise:
          if (!allow_tail) {
            return std::nullopt;  // needs sequential application
          }
          if (step.tail_op.has_value() &&
              tailOpAdmitted(*step.tail_op, step.dtype, meta.numel())) {
            plan.tail.push_back(*step.tail_op);
          } else {
            tail_unfusable = true;
          }
          break;
        case ChainStep::Kind::kZero:
          plan.kind = InitPlan::Kind::kZero;
          have_value = true;
          plan.tail.clear();
          tail_unfusable = false;
          break;
        case ChainStep::Kind::kFill:
          plan.kind = InitPlan::Kind::kFill;
          plan.p0 = step.p0;
          have_value = true;
          plan.tail.clear();
          tail_unfusable = false;
          break;
        case ChainStep::Kind::kUniform:
        case ChainStep::Kind::kNormal:
        case ChainStep::Kind::kBernoulli:
          if (!step.philox.has_value()) {
            return std::nullopt;
          }
          plan.kind = step.kind == ChainStep::Kind::kUniform
                          ? InitPlan::Kind::kUniform
                          : (step.kind == ChainStep::Kind::kNormal
                                 ? InitPlan::Kind::kNormal
                                 : InitPlan::Kind::kBernoulli);
          plan.p0 = step.p0;
          plan.p1 = step.p1;
          plan.seed = step.philox->first;
          plan.offset = step.philox->second;
          have_value = true;
          // Everything before a whole-tensor value step is dead.
          plan.tail.clear();
          tail_unfusable = false;
          break;
      }
    }
    if (!have_value) {
      plan.kind = InitPlan::Kind::kFactory;  // allocate-only (empty)
    }
    if (tail_unfusable || !plan.tail.empty()) {
      // A live tail fuses only into a pinned-Philox RNG kernel.
      const bool rng_head = plan.kind == InitPlan::Kind::kUniform ||
                            plan.kind == InitPlan::Kind::kNormal ||
                            plan.kind == InitPlan::Kind::kBernoulli;
      if (tail_unfusable || !rng_head || plan.tail.size() > kMaxTailOps) {
        return std::nullopt;
      }
    }
    if (cast_src.has_value() && patches != nullptr) {
      for (size_t i = 0; i < patches->size(); ++i) {
        PatchStep& ps = (*patches)[i];
        // An RNG patch draws at the dtype it was recorded at; only the
        // segment replay serves that next to a conversion.
        if (ps.kind != InitPlan::Kind::kFill &&
            ps.kind != InitPlan::Kind::kZero) {
          return std::nullopt;
        }
        if (patch_before_cast[i]) {
          auto rounded = roundScalarThrough(ps.p0, *cast_src);
          if (!rounded.has_value()) {
            return std::nullopt;
          }
          ps.p0 = *rounded;
        }
      }
    }
    if (cast_src.has_value()) {
      switch (plan.kind) {
        case InitPlan::Kind::kUniform:
        case InitPlan::Kind::kNormal:
        case InitPlan::Kind::kBernoulli:
          // The values depend on the dtype they were drawn at (group
          // size, tail arithmetic): the cast kernels take both dtypes.
          if (!isFloat3(*cast_src) || !isFloat3(meta.scalar_type())) {
            return std::nullopt;
          }
          plan.src_dtype = *cast_src;
          break;
        case InitPlan::Kind::kFill: {
          // A constant converts on the host: a plain fill at the final
          // dtype with the value as the source tensor held it.
          auto rounded = roundScalarThrough(plan.p0, *cast_src);
          if (!rounded.has_value()) {
            return std::nullopt;
          }
          plan.p0 = *rounded;
          break;
        }
        case InitPlan::Kind::kZero:
        case InitPlan::Kind::kFactory:
          break;
      }
    }
  } catch (const c10::Error&) {
    return std::nullopt;  // not a simple chain
  }
  plan.sizes.assign(meta.sizes().begin(), meta.sizes().end());
  plan.dtype = meta.scalar_type();
  plan.device = fake->fake_device();
  plan.requires_grad = tensor.requires_grad();
  return plan;
}

// Allocates the shard and applies the tensor's init chain to it over the
// window (or box) `w` of the full tensor.
at::Tensor replayChainOnShard(FakeTensorImpl* fake,
                              const std::vector<int64_t>& shard_sizes,
                              const ShardWindow& w) {
  const at::Tensor& meta = fake->meta_tensor();
  std::lock_guard<std::recursive_mutex> lock{tape_mutex};
  auto rec = getRecord(fake);
  const std::vector<ChainStep> steps = buildChainSteps(*rec, meta);
  TORCH_CHECK(!steps.empty() &&
                  (steps.front().kind == ChainStep::Kind::kFactory ||
                   steps.front().kind == ChainStep::Kind::kZero ||
                   steps.front().kind == ChainStep::Kind::kFill),
              "slice materialization: the tape does not start with a "
              "factory op");
  const auto options = at::TensorOptions().device(fake->fake_device());
  auto tailOf = [&](const FusedRun& run) {
    std::vector<TailOp> tail;
    for (size_t i = run.tail_begin; i < run.tail_end; ++i) {
      tail.push_back(*steps[i].tail_op);
    }
    return tail;
  };

  // Live patches sit behind the tail (buildChainSteps); with them read as
  // pass steps the fused runs below are found as for a patch-free chain.
  std::vector<ChainStep> plain = steps;
  bool rng_patch = false;
  for (ChainStep& step : plain) {
    if (step.patch) {
      rng_patch = rng_patch || isRngStep(step);
      step.kind = ChainStep::Kind::kPass;
      step.patch = false;
    }
  }

  // [RNG step, tail..., one cast] at the end of the chain is one launch
  // that draws at the source dtype and stores the final one; everything
  // before the RNG step is overwritten by it. A box of two or more levels
  // has no cast kernel: it takes the segments below (the box op at the
  // source dtype into a block-sized temporary, then the conversion).
  // Constant patches go on afterwards at the final dtype, a patch from
  // before the conversion with its value rounded through the source dtype
  // first; an RNG patch draws at the dtype it was recorded at, so a chain
  // with one takes the segments.
  if (!w.box.has_value() && !rng_patch) {
    const auto run = fusedRunStart(plain, 0, plain.size(), meta.numel(),
                                   /*allow_cast=*/true);
    if (run.has_value() && run->cast.has_value()) {
      std::vector<double> values;
      bool representable = true;
      for (size_t i = run->tail_end; i < steps.size(); ++i) {
        if (!steps[i].patch) {
          continue;
        }
        std::optional<double> v = steps[i].p0;
        if (i < *run->cast) {
          v = roundScalarThrough(steps[i].p0, steps[*run->cast].dtype);
        }
        representable = representable && v.has_value();
        values.push_back(v.value_or(0.0));
      }
      if (representable) {
        at::Tensor shard =
            at::empty(shard_sizes, options.dtype(steps[*run->cast].cast_to));
        applyFusedCastShardStep(steps[run->rng], tailOf(*run),
                                steps[*run->cast].dtype, shard, w,
                                meta.numel());
        size_t n = 0;
        for (size_t i = run->tail_end; i < steps.size(); ++i) {
          if (steps[i].patch) {
            applyPatchOp(shard, w, meta.numel(), steps[i].patch_lo,
                         steps[i].patch_len, valueDistCode(steps[i].kind),
                         values[n++], 0.0, std::nullopt);
          }
        }
        return shard;
      }
    }
  }

  // Otherwise the chain runs in segments of one dtype each, split at its
  // conversions. The shard starts at the chain's FIRST dtype; within a
  // segment a [RNG step, fusable tail...] run followed only by pass steps
  // and patches is one fused launch and any other arrangement applies step
  // by step; a patch is one tdx::patch_box_ call at the segment's dtype; a
  // conversion replaces the shard by its converted copy. Only shard-sized
  // tensors exist at any point.
  at::Tensor shard = at::empty(shard_sizes, options.dtype(steps.front().dtype));
  size_t lo = 0;
  while (lo < steps.size()) {
    size_t hi = lo;
    while (hi < steps.size() && steps[hi].kind != ChainStep::Kind::kCast) {
      ++hi;
    }
    const auto run =
        fusedRunStart(plain, lo, hi, meta.numel(), /*allow_cast=*/false);
    for (size_t i = lo; i < hi; ++i) {
      if (run.has_value() && i == run->rng) {
        applyFusedShardStep(steps[i], tailOf(*run), shard, w, meta.numel());
        i = run->tail_end - 1;  // pass steps and patches remain
        continue;
      }
      applyShardStep(steps[i], shard, w, meta.numel());
    }
    if (hi < steps.size()) {
      shard = castShard(shard, steps[hi].cast_to);
    }
    lo = hi + 1;
  }
  return shard;
}

}  // namespace

const char* tailOpName(int32_t op) {
  static const char* kNames[] = {"erfinv",    "mul",       "add",
                                 "sub",       "clamp",     "clamp_min",
                                 "clamp_max", "neg",       "abs"};
  TORCH_CHECK(0 <= op && op < 9, "bad tail opcode ", op);
  return kNames[op];
}

// Reduces a deferred tensor's tape chain to its final whole-tensor value
// step, when the chain is that simple. Every simple-chain value step
// (uniform/normal/bernoulli/fill/zero) overwrites the whole tensor, so
// only the LAST one determines the bits: batched replay can then fill
// many tensors with ONE kernel launch. Returns nullopt for anything
// else (pointwise tails, live partial-tensor writes — see
// tensorPatchPlan —, strided views, cross-tensor deps, explicit
// generators); callers fall back to ordinary materialization.
std::optional<InitPlan> tensorInitPlan(const at::Tensor& tensor) {
  auto plan = chainPlanImpl(tensor, /*allow_tail=*/false);
  if (!plan.has_value()) {
    return std::nullopt;
  }
  return static_cast<const InitPlan&>(*plan);
}

std::optional<ChainPlan> tensorChainPlan(const at::Tensor& tensor) {
  return chainPlanImpl(tensor, fusedInitChainsEnabled());
}

std::optional<PatchPlan> tensorPatchPlan(const at::Tensor& tensor) {
  std::vector<PatchStep> patches;
  auto plan = chainPlanImpl(tensor, fusedInitChainsEnabled(), &patches);
  if (!plan.has_value()) {
    return std::nullopt;
  }
  PatchPlan out;
  static_cast<ChainPlan&>(out) = std::move(*plan);
  out.patches = std::move(patches);
  return out;
}

at::Tensor materializeTensorShard(const at::Tensor& tensor,
                                  int64_t start_row,
                                  int64_t end_row,
                                  int64_t dim) {
  auto* fake = asFake(tensor);
  TORCH_CHECK_VALUE(fake != nullptr && getRecord(fake) != nullptr,
                    "`tensor` is not a deferred tensor.");
  const at::Tensor& meta = fake->meta_tensor();
  TORCH_CHECK(meta.is_contiguous(),
              "slice materialization requires a contiguous tensor");
  TORCH_CHECK(0 <= dim && (dim < meta.dim() || (dim == 0 && meta.dim() == 0)),
              "invalid slice dim ", dim, " for a ", meta.dim(),
              "-d tensor");
  const int64_t dim_len = meta.dim() == 0 ? 1 : meta.size(dim);
  TORCH_CHECK(0 <= start_row && start_row <= end_row && end_row <= dim_len,
              "invalid slice range [", start_row, ", ", end_row,
              ") for size ", dim_len, " along dim ", dim);
  // full.narrow(dim, start, end - start) flattened = a strided window
  // over the full element space: prod(sizes[:dim]) blocks of
  // (end - start) * prod(sizes[dim+1:]) contiguous elements each.
  int64_t inner = 1;  // prod(sizes[dim+1:])
  for (int64_t d = dim + 1; d < meta.dim(); ++d) {
    inner *= meta.size(d);
  }
  int64_t n_blocks = 1;  // prod(sizes[:dim])
  for (int64_t d = 0; d < dim; ++d) {
    n_blocks *= meta.size(d);
  }
  const ShardWindow w{n_blocks, (end_row - start_row) * inner,
                      dim_len * inner, start_row * inner};

  std::vector<int64_t> shard_sizes(meta.sizes().begin(), meta.sizes().end());
  if (!shard_sizes.empty()) {
    shard_sizes[dim] = end_row - start_row;
  }
  return replayChainOnShard(fake, shard_sizes, w);
}

at::Tensor materializeTensorBlock(const at::Tensor& tensor,
                                  at::IntArrayRef starts,
                                  at::IntArrayRef ends) {
  auto* fake = asFake(tensor);
  TORCH_CHECK_VALUE(fake != nullptr && getRecord(fake) != nullptr,
                    "`tensor` is not a deferred tensor.");
  const at::Tensor& meta = fake->meta_tensor();
  TORCH_CHECK(meta.is_contiguous(),
              "slice materialization requires a contiguous tensor");
  const int64_t rank = meta.dim();
  TORCH_CHECK(static_cast<int64_t>(starts.size()) == rank &&
                  static_cast<int64_t>(ends.size()) == rank,
              "block materialization takes one start and one end per dim: "
              "got ", starts.size(), " and ", ends.size(), " for a ", rank,
              "-d tensor");
  std::vector<int64_t> shard_sizes(rank);
  for (int64_t d = 0; d < rank; ++d) {
    TORCH_CHECK(0 <= starts[d] && starts[d] <= ends[d] &&
                    ends[d] <= meta.size(d),
                "invalid slice range [", starts[d], ", ", ends[d],
                ") for size ", meta.size(d), " along dim ", d);
    shard_sizes[d] = ends[d] - starts[d];
  }
  BoxGeometry box;
  const BoxStatus status = normalizeBox(meta.sizes().data(), starts.data(),
                                        ends.data(), static_cast<int>(rank),
                                        &box);
  TORCH_CHECK(status == BoxStatus::kOk,
              "slice materialization: the block needs more than ",
              kMaxBoxLevels, " nested strided levels; materialize the "
              "tensor fully instead.");
  // 0 and 1 levels are the flat range and the single-dim window, served
  // by the ops materializeTensorShard launches; deeper nests take the box
  // op.
  ShardWindow w{1, box.run_len, box.run_len, box.g_off};
  if (box.levels == 1) {
    w = ShardWindow{box.extent[0], box.run_len, box.g_stride[0], box.g_off};
  } else if (box.levels >= 2) {
    w.box = box;
  }
  return replayChainOnShard(fake, shard_sizes, w);
}

at::Tensor materializeTensor(const at::Tensor& tensor) {
  auto* fake = asFake(tensor);
  if (fake == nullptr) {
    return tensor;  // identity for real tensors
  }
  auto rec = getRecord(fake);
  TORCH_CHECK_VALUE(rec != nullptr,
                    "`tensor` is fake but carries no deferred-init record, "
                    "so it cannot be materialized.");

  std::unique_lock<std::recursive_mutex> lock{tape_mutex};
  // Capture the producer descriptor while holding the lock: a concurrent
  // recording thread may restamp `rec->desc` while this thread's replay
  // runs unlocked, and the pre-restamp value is the one this call stack
  // materializes (a legal serialization of the two racing calls).
  OpOutputDescriptor desc = rec->desc;
  for (const auto& n : buildCallStack(*rec)) {
    replayNode(lock, n);
  }

  at::Tensor out = desc.node->outputs.at(desc.index);
  // requires_grad_() is untraceable on purpose; re-apply the fake tensor's
  // final autograd flag explicitly (reference deferred_init.cc:713-729).
  if (out.is_leaf() && out.requires_grad() != tensor.requires_grad()) {
    out.set_requires_grad(tensor.requires_grad());
  }
  return out;
}

}  // namespace tdx
