# Plain fp64 reference of the SlowMo kernels (csrc/hip/slowmo.hip): inputs
# widened to fp64, scalars kept in double, round_P by .to(dtype). A helper
# module for tests/test_slowmo_fused_gpu.py.

import torch


def reference_outer_step(a, prev, m, lr, slowmo_factor, slowmo_lr):
    """(m', q) in fp64 of one outer step; a is the averaged parameter as
    its dtype stores it. prev' = p' = q.to(a.dtype)."""
    a64, prev64, m64 = (t.to(torch.float64) for t in (a, prev, m))
    m_new = slowmo_factor * m64 + (prev64 - a64) / lr
    return m_new, prev64 - slowmo_lr * lr * m_new


def reference_pack(params, offsets, total, world_size):
    """The flat buffer after the pack: cat(params).div_(world_size), as
    the stock averager forms it, scattered into the padded layout."""
    packed = torch.cat([p.reshape(-1) for p in params]).div_(world_size)
    flat = torch.zeros(total, dtype=packed.dtype, device=packed.device)
    start = 0
    for p, off in zip(params, offsets):
        flat[off:off + p.numel()] = packed[start:start + p.numel()]
        start += p.numel()
    return flat
