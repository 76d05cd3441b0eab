# Per-element oracle for tdx::patch_box_, shared by tests/test_patch_slice.py
# (CPU op) and tests/test_patch_slice_gpu.py (CDNA4 kernel). A plain helper
# module: it draws the patch VIEW with the full-tensor tdx:: op on the
# device under test (normals are per device), computes every shard
# element's full-tensor index from the box geometry, and scatters the view
# into a copy of the shard.

import torch

UNIFORM, NORMAL, BERNOULLI, FILL, ZERO = range(5)
KINDS = {"uniform": UNIFORM, "normal": NORMAL, "bernoulli": BERNOULLI,
         "fill": FILL, "zero": ZERO}


def box_geometry(shape, box):
    """(extents, g_strides, run_len, g_off) of full[box] for a contiguous
    tensor of ``shape`` (rank 1..5), unnormalized: the last dim is the run,
    every other dim a level. That is a valid geometry for the box ops,
    extent-1 and extent-0 levels included."""
    strides = [1] * len(shape)
    for d in range(len(shape) - 2, -1, -1):
        strides[d] = strides[d + 1] * shape[d + 1]
    g_off = sum(lo * s for (lo, _), s in zip(box, strides))
    run_len = box[-1][1] - box[-1][0]
    extents = [hi - lo for lo, hi in box[:-1]]
    g_strides = list(strides[:-1])
    if not extents:
        extents, g_strides = [1], [max(run_len, 1)]
    if run_len == 0 or 0 in extents:
        g_off = 0  # an empty box touches nothing, wherever it "starts"
    return extents, g_strides, run_len, g_off


def global_indices(extents, g_strides, run_len, g_off, device="cpu"):
    """Full-tensor index of every shard element, in shard order (int64)."""
    g = torch.full((1,), g_off, dtype=torch.int64, device=device)
    for e, s in zip(extents, g_strides):
        level = torch.arange(e, dtype=torch.int64, device=device) * s
        g = (g[:, None] + level[None, :]).reshape(-1)
    within = torch.arange(run_len, dtype=torch.int64, device=device)
    return (g[:, None] + within[None, :]).reshape(-1)


def draw_view(n, dtype, device, dist, p0, p1, seed, offset):
    """What the full-tensor tdx:: op gives a contiguous n-element tensor."""
    view = torch.empty(n, dtype=dtype, device=device)
    if dist == UNIFORM:
        torch.ops.tdx.uniform_(view, p0, p1, seed=seed, offset=offset)
    elif dist == NORMAL:
        torch.ops.tdx.normal_(view, p0, p1, seed=seed, offset=offset)
    elif dist == BERNOULLI:
        torch.ops.tdx.bernoulli_(view, p0, seed=seed, offset=offset)
    elif dist == FILL:
        torch.ops.tdx.fill_(view, p0)
    else:
        torch.ops.tdx.zero_(view)
    return view


def expected(shard, geometry, patch_lo, patch_len, dist, p0, p1, seed,
             offset):
    """``shard`` (any shape, contiguous) after the patch, by scatter."""
    g = global_indices(*geometry, device=shard.device)
    assert g.numel() == shard.numel()
    view = draw_view(patch_len, shard.dtype, shard.device, dist, p0, p1,
                     seed, offset)
    inside = (g >= patch_lo) & (g < patch_lo + patch_len)
    out = shard.clone().view(-1)
    out[inside] = view[g[inside] - patch_lo]
    return out.view(shard.shape), int(inside.sum())


def call(shard, geometry, full_numel, patch_lo, patch_len, dist, p0, p1,
         seed, offset):
    extents, g_strides, run_len, g_off = geometry
    rng = dist <= BERNOULLI
    return torch.ops.tdx.patch_box_(
        shard, list(extents), list(g_strides), run_len, g_off, full_numel,
        patch_lo, patch_len, dist, p0, p1,
        seed if rng else None, offset if rng else None)
