# Deferred-initialization Python API.
#
# Capability parity with the reference
# (/root/reference/src/python/torchdistx/deferred_init.py:19-124):
# deferred_init / is_deferred / materialize_tensor / materialize_module with
# identical semantics, including recursive child-first module
# materialization, buffers_only / check_fn filtering, object identity for
# repeated and aliased materializations, and in-place swapping of
# module._parameters / module._buffers entries.
#
# Design difference vs the reference binding layer: the reference allocates
# the materialized Python object with the original's class in C++
# (_C/deferred_init.cc:33-94); here the C++ core returns the canonical
# Tensor wrapper (stable per TensorImpl) and the original's Python class —
# Parameter, a Parameter subclass, or a plain Tensor subclass — is restored
# in Python (Parameter re-wrap / Tensor.as_subclass, neither of which runs
# the subclass constructor, mirroring the reference's tp_alloc), memoized
# per materialized tensor so aliased parameters still materialize to one
# object.

from typing import Callable, Dict, Optional, TypeVar, Union


from torch import Tensor
from torch.nn import Module, Parameter
from torch.utils.weak import WeakTensorKeyDictionary

# Imported for its Tensor.__repr__ patch.
from torchdistx_amd import fake  # noqa: F401
from torchdistx_amd import _C

T = TypeVar("T", bound=Module)

# materialized base tensor -> class-restored wrapper, so aliased parameters
# (and repeated materializations) map to a single wrapper object.
_wrapper_memo: "WeakTensorKeyDictionary" = WeakTensorKeyDictionary()

# Stable per-slot HIP streams for materialize_module_parallel (see there).
_worker_streams: list = []


def deferred_init(module_fn: Callable[..., T], *args, **kwargs) -> T:
    """Runs ``module_fn`` with tensor construction deferred: every tensor it
    creates is fake, and every operation on those tensors is recorded on an
    in-memory tape. The result can later be turned into a real module with
    :func:`materialize_module` (or tensor-by-tensor with
    :func:`materialize_tensor`) — including on a different device, sharded
    across ranks, or through the CDNA4 HIP init kernels on an MI355X.

    Args:
        module_fn: a callable returning a ``Module``.
        args, kwargs: forwarded to ``module_fn``.

    .. warning::
        Only operations performed *inside* ``deferred_init()`` are recorded.
        Mutating the returned module afterwards (outside another deferred
        context) cannot be replayed and will make materialization
        incorrect or impossible.
    """
    _C.enter_deferred_init()
    try:
        return module_fn(*args, **kwargs)
    finally:
        _C.leave_deferred_init()


def is_deferred(obj: Union[Tensor, Module]) -> bool:
    """Whether ``obj`` (a tensor, or any parameter/buffer of a module) still
    awaits materialization."""
    if isinstance(obj, Tensor):
        return _C.can_materialize(obj)

    if isinstance(obj, Module):
        return any(
            _C.can_materialize(t)
            for t in list(obj.parameters()) + list(obj.buffers())
        )

    raise ValueError("`obj` must be of type `Tensor` or `Module`.")


def materialize_tensor(tensor: Tensor) -> Tensor:
    """Materializes ``tensor`` by replaying the relevant part of its
    recording tape. Real tensors pass through unchanged; repeated calls and
    aliased fakes return the same object.

    .. warning::
        A materialized fake keeps a reference to its materialized value;
        drop the fake once it is no longer needed to release memory.
    """
    materialized = _C.materialize_tensor(tensor)
    if materialized is tensor:
        return tensor
    return _restore_class(tensor, materialized)


def _restore_class(original: Tensor, materialized: Tensor) -> Tensor:
    cls = type(original)
    if cls is type(materialized):
        return materialized
    wrapper = _wrapper_memo.get(materialized)
    if wrapper is None or type(wrapper) is not cls:
        if cls is Parameter:
            wrapper = Parameter(
                materialized, requires_grad=original.requires_grad
            )
        else:
            # Parameter subclass or plain Tensor subclass: re-class the
            # materialized tensor without running the subclass constructor
            # (the Python analog of the reference's tp_alloc class
            # preservation, _C/deferred_init.cc:33-94).
            wrapper = materialized.as_subclass(cls)
            if (
                wrapper.is_leaf
                and wrapper.requires_grad != original.requires_grad
            ):
                wrapper.requires_grad_(original.requires_grad)
        _wrapper_memo[materialized] = wrapper
    return wrapper


def materialize_module(
    module: Module,
    buffers_only: bool = False,
    check_fn: Optional[Callable[[Module], bool]] = None,
) -> None:
    """Materializes ``module`` in place: children first, then this module's
    parameters and buffers.

    Args:
        module: the deferred module to materialize.
        buffers_only: only materialize buffers.
        check_fn: optional per-module predicate; modules for which it
            returns ``False`` are skipped (their children are still
            visited).
    """

    def swap(tensors: Dict[str, Optional[Tensor]]) -> None:
        for key, tensor in tensors.items():
            if tensor is None:
                continue
            try:
                tensors[key] = materialize_tensor(tensor)
            except ValueError:
                raise ValueError(
                    f"'{key}' has already been materialized."
                ) from None

    for child in module.children():
        materialize_module(child, buffers_only, check_fn)

    if check_fn is None or check_fn(module):
        if not buffers_only:
            swap(module._parameters)  # type: ignore[arg-type]
        swap(module._buffers)  # type: ignore[arg-type]


_DIST_CODE = {"uniform": 0, "normal": 1, "bernoulli": 2, "fill": 3,
              "zero": 4, "factory": -1}

# Tail opcodes of the fused chain kernels (TailOp::Code in
# csrc/core/deferred_init.h), keyed by the names tensor_chain_plan reports.
_TAIL_CODE = {"erfinv": 0, "mul": 1, "add": 2, "sub": 3, "clamp": 4,
              "clamp_min": 5, "clamp_max": 6, "neg": 7, "abs": 8}


def materialize_module_batched(
    module: Module,
    buffers_only: bool = False,
    check_fn: Optional[Callable[[Module], bool]] = None,
    device=None,
) -> None:
    """Materializes ``module`` through the batched replay planner: every
    parameter/buffer whose tape is a simple init chain collapses to its
    final whole-tensor value step, and ALL of them fill in ONE CDNA4
    kernel launch (bitwise-identical to the per-tensor replay — each
    tensor keeps its pinned Philox stream). An RNG step followed by a
    fusable pointwise-scalar tail (``trunc_normal_``'s ``uniform_ ->
    erfinv_ -> mul_ -> add_ -> clamp_``) is part of that launch: the
    kernel applies the tail in registers before the store. Tensors with
    richer tapes (views, cross-tensor dependencies, tails outside the
    fusable set such as ``div_`` or ``add_(alpha != 1)``, any tail while
    ``_C.set_fused_init_chains(False)`` is in effect) fall back to
    ordinary replay. A chain that ends in one dtype conversion between
    float32/bf16/fp16 — ``Model(cfg).to(torch.bfloat16)`` inside the
    builder, ``Parameter(empty(..).normal_().to(bf16))`` — is plannable
    too: its tensors fill in a second launch that draws at the recorded
    dtype and stores the final one, without a full-precision copy.
    GPU-only; CPU targets use :func:`materialize_module`.

    Launch count for a Llama-3-70B replica drops from ~560 to ~3.

    ``device`` retargets materialization: plans allocate and fill
    directly on that device (e.g. a tape recorded with device="cpu"
    lands straight in HBM; the pinned counters make uniform/bernoulli/
    fill bits identical across devices, normals equivalent but
    per-device-transformed). Fallback tensors replay on their recorded
    device and are then moved; a chain with a pointwise tail recorded on
    another device is one of them (erfinv bits are per device)."""
    import torch

    from torchdistx_amd import _kernels

    entries = []
    for submodule in module.modules():
        if check_fn is not None and not check_fn(submodule):
            continue
        if not buffers_only:
            for key, p in submodule._parameters.items():
                if p is not None and _C.can_materialize(p):
                    entries.append((submodule, key, p, True))
        for key, b in submodule._buffers.items():
            if b is not None and _C.can_materialize(b):
                entries.append((submodule, key, b, False))

    for entry in _batched_fill(entries, device=device):
        submodule, key, tensor, is_param = entry
        mat = materialize_tensor(tensor)
        if device is not None and mat.device != torch.device(device):
            moved = mat.detach().to(device)
            moved.requires_grad_(mat.requires_grad)
            mat = _restore_class(tensor, moved)
        if is_param:
            submodule._parameters[key] = mat
        else:
            submodule._buffers[key] = mat


def _same_device(a, b) -> bool:
    """Device equality where a missing index matches any ("cuda" is
    "cuda:0" for this purpose)."""
    return a.type == b.type and (
        a.index is None or b.index is None or a.index == b.index
    )


def _batched_fill(entries, device=None) -> list:
    """Fills every plannable (simple-chain, GPU, f32/bf16/f16) entry with
    one batched kernel launch and swaps the module slots; returns the
    entries that must go through ordinary replay instead. Used by
    :func:`materialize_module_batched` and the distributed shard path.
    ``device`` overrides the plans' target device (retargeting).

    A chain whose init also overwrites contiguous sub-ranges of the tensor
    (``nn.Embedding(padding_idx=i)``, a fused weight initialized by parts)
    has no chain plan; ``_C.tensor_patch_plan`` gives its base value step,
    which joins the batch like any other plan, and its patches. After the
    batched launch each patch is one ``tdx::patch_box_`` call on the flat
    output, on the same stream. Patches are rare (one or two per model), so
    a launch each is cheaper than teaching the batched kernel about them.
    Under retargeting a normal patch recorded for another device sends the
    tensor to ordinary replay, as a tail does (the normal transform is per
    device); uniform, bernoulli and constant patches do not."""
    import torch

    from torchdistx_amd import _kernels

    if device is not None:
        device = torch.device(device)
    target_cuda = (
        device.type == "cuda"
        if device is not None
        else bool(entries) and entries[0][2].is_cuda
    )
    gpu = (
        bool(entries)
        and target_cuda
        and torch.cuda.is_available()
        and getattr(_kernels, "_K", None) is not None
        and _kernels._K.has_batched_init()
    )
    if not gpu:
        return list(entries)

    fused = (
        hasattr(_kernels._K, "has_fused_chains")
        and _kernels._K.has_fused_chains()
    )
    # Chains that end in a dtype conversion (Module.to(dtype) inside the
    # builder) need the kernels that draw at one dtype and store another.
    cast = (
        hasattr(_kernels._K, "has_cast_chains")
        and _kernels._K.has_cast_chains()
    )
    patch_kernel = (
        hasattr(_kernels._K, "has_patch_kernel")
        and _kernels._K.has_patch_kernel()
    )
    batch = {"t": [], "dist": [], "p0": [], "p1": [], "seed": [],
             "offset": [], "tail": [], "src": [], "entry": []}
    patched = []  # (out, patches): applied after the batched launches
    fallback = []
    seen = {}  # id(fake) -> out: tied params must share ONE allocation
    for entry in entries:
        tensor = entry[2]
        if id(tensor) in seen:
            batch["entry"].append((entry, seen[id(tensor)]))
            continue
        if fused:
            plan = _C.tensor_chain_plan(tensor)
        else:
            plan = _C.tensor_init_plan(tensor)
        patches = []
        if plan is None and patch_kernel:
            plan = _C.tensor_patch_plan(tensor)
            if plan is not None and plan["tail"] and not fused:
                plan = None
            patches = plan["patches"] if plan is not None else []
        tail = plan.get("tail", []) if plan is not None else []
        src_dtype = plan.get("src_dtype") if plan is not None else None
        if (
            plan is None
            or (src_dtype is not None and not cast)
            or plan["dtype"] not in (
                torch.float32, torch.bfloat16, torch.float16
            )
            # One batched launch targets one device; stray tensors of a
            # mixed-device module replay normally.
            or (device is None and plan["device"] != entries[0][2].device)
            # A tail recorded on another device replays there: the
            # uniform bits match across devices, erfinv's need not.
            or (
                (tail or any(p["kind"] == "normal" for p in patches))
                and device is not None
                and not _same_device(plan["device"], device)
            )
        ):
            fallback.append(entry)
            continue
        out = torch.empty(
            plan["sizes"],
            dtype=plan["dtype"],
            device=device if device is not None else plan["device"],
        )
        seen[id(tensor)] = out
        code = _DIST_CODE[plan["kind"]]
        if code >= 0:
            batch["t"].append(out)
            batch["dist"].append(code)
            batch["p0"].append(plan["p0"])
            batch["p1"].append(plan["p1"])
            batch["seed"].append(plan["seed"])
            batch["offset"].append(plan["offset"])
            batch["tail"].append(tail)
            batch["src"].append(src_dtype)
        # kind == "factory": allocate-only, matching aten::empty replay.
        batch["entry"].append((entry, out))
        if patches:
            patched.append((out, patches))

    if batch["t"] and any(d is not None for d in batch["src"]):
        # Tensors with a conversion fill in a second launch of their own
        # kernel; the others launch as in the branches below.
        _kernels._K.batched_init_(
            batch["t"], batch["dist"], batch["p0"], batch["p1"],
            batch["seed"], batch["offset"],
            [[_TAIL_CODE[name] for name, _, _ in t] for t in batch["tail"]],
            [[s0 for _, s0, _ in t] for t in batch["tail"]],
            [[s1 for _, _, s1 in t] for t in batch["tail"]],
            batch["src"],
        )
    elif batch["t"] and any(batch["tail"]):
        _kernels._K.batched_init_(
            batch["t"], batch["dist"], batch["p0"], batch["p1"],
            batch["seed"], batch["offset"],
            [[_TAIL_CODE[name] for name, _, _ in t] for t in batch["tail"]],
            [[s0 for _, s0, _ in t] for t in batch["tail"]],
            [[s1 for _, _, s1 in t] for t in batch["tail"]],
        )
    elif batch["t"]:
        _kernels._K.batched_init_(
            batch["t"], batch["dist"], batch["p0"], batch["p1"],
            batch["seed"], batch["offset"],
        )
    for out, patches in patched:
        n = out.numel()
        flat = out.view(-1)
        for p in patches:
            rng = p["kind"] in ("uniform", "normal", "bernoulli")
            torch.ops.tdx.patch_box_(
                flat, [1], [n], n, 0, n, p["lo"], p["len"],
                _DIST_CODE[p["kind"]], p["p0"], p["p1"],
                p["seed"] if rng else None, p["offset"] if rng else None,
            )
    for (submodule, key, tensor, is_param), out in batch["entry"]:
        if is_param:
            if out.is_leaf and out.requires_grad != tensor.requires_grad:
                out.requires_grad_(tensor.requires_grad)
            out = _restore_class(tensor, out)
            submodule._parameters[key] = out
        else:
            submodule._buffers[key] = out
    return fallback


def materialize_module_parallel(
    module: Module,
    num_threads: int = 4,
    buffers_only: bool = False,
    check_fn: Optional[Callable[[Module], bool]] = None,
) -> None:
    """Materializes ``module`` with ``num_threads`` worker threads, each
    replaying its share of the parameters on its own HIP stream. The tape
    releases its lock while ops execute, so host-side launch work and the
    init kernels of different tensors genuinely overlap — on GPU targets
    with the pinned-Philox native kernels the result is bitwise identical
    to :func:`materialize_module` (replay order cannot change the pinned
    streams). On CPU targets it falls back to the sequential path, whose
    tape-order stock-generator replay is the documented eager-parity
    contract."""
    import threading

    entries = []  # (submodule, key, tensor, is_param)
    for submodule in module.modules():
        if check_fn is not None and not check_fn(submodule):
            continue
        if not buffers_only:
            for key, p in submodule._parameters.items():
                if p is not None and _C.can_materialize(p):
                    entries.append((submodule, key, p, True))
        for key, b in submodule._buffers.items():
            if b is not None and _C.can_materialize(b):
                entries.append((submodule, key, b, False))

    gpu = bool(entries) and entries[0][2].is_cuda
    if num_threads <= 1 or not gpu or len(entries) < 2:
        materialize_module(module, buffers_only, check_fn)
        return

    # Greedy size balancing: the embedding/lm-head tensors are an order
    # of magnitude larger than a block's projections, so round-robin
    # alone would leave one thread with most of the bytes.
    loads = [0] * num_threads
    chunks = [[] for _ in range(num_threads)]
    for i in sorted(
        range(len(entries)), key=lambda j: -entries[j][2].numel()
    ):
        w = min(range(num_threads), key=lambda r: loads[r])
        chunks[w].append(entries[i])
        loads[w] += entries[i][2].numel()

    import torch

    # One stable stream per worker slot, created once per process: the
    # caching allocator tags blocks with their allocation stream, so
    # fresh Stream objects every call would orphan the previous call's
    # cached blocks and turn each step into a full hipFree/hipMalloc
    # churn of the model's bytes (measured ~90x slowdown on a 141 GB
    # replicate step).
    global _worker_streams
    while len(_worker_streams) < num_threads:
        _worker_streams.append(torch.cuda.Stream())

    errors = []

    def worker(slot, chunk):
        try:
            stream = _worker_streams[slot]
            with torch.cuda.stream(stream):
                for submodule, key, tensor, is_param in chunk:
                    mat = materialize_tensor(tensor)
                    if is_param:
                        submodule._parameters[key] = mat
                    else:
                        submodule._buffers[key] = mat
            # A fresh thread's current stream is the shared default
            # stream: ordering it after the side stream makes the
            # materialized tensors safe for any later default-stream use.
            torch.cuda.current_stream().wait_stream(stream)
        except Exception as e:  # surfaced below
            errors.append(e)

    threads = [
        threading.Thread(target=worker, args=(slot, c))
        for slot, c in enumerate(chunks)
        if c
    ]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
