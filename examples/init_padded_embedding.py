"""A Hugging Face style model with a pad token: `_init_weights` draws the
embedding table and then zeroes the padding row, a partial-tensor write in
the table's init chain. The builder also converts to bfloat16. Each rank
still materializes only its own rows: the padding row is written by
tdx::patch_box_ on whichever shard holds it, and no rank ever allocates the
full table.

    python examples/init_padded_embedding.py [world_size]

Runs on the GPU when there is one, else on the CPU, playing every rank in
turn and checking the shards against one full materialization.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
from torch import nn

from torchdistx_amd import _C, deferred_init
from torchdistx_amd.deferred_init import materialize_tensor
from torchdistx_amd.parallel import materialize_module_dim0_sharded

VOCAB, DIM, PAD = 4096, 256, 0


class PadTokenLM(nn.Module):
    def __init__(self, device) -> None:
        super().__init__()
        self.embed = nn.Embedding(VOCAB, DIM, padding_idx=PAD, device=device)
        self.head = nn.Linear(DIM, VOCAB, bias=False, device=device)
        self.apply(self._init_weights)

    @staticmethod
    def _init_weights(module: nn.Module) -> None:
        if isinstance(module, nn.Linear):
            module.weight.data.normal_(mean=0.0, std=0.02)
        elif isinstance(module, nn.Embedding):
            module.weight.data.normal_(mean=0.0, std=0.02)
            if module.padding_idx is not None:
                module.weight.data[module.padding_idx].zero_()


def main() -> None:
    world_size = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    device = "cuda" if torch.cuda.is_available() else "cpu"
    if device == "cpu":
        _C.set_native_init_cpu(True)  # counter-based init kernels on the CPU
    torch.manual_seed(0)
    model = deferred_init(lambda: PadTokenLM(device).to(torch.bfloat16))

    plan = _C.tensor_patch_plan(model.embed.weight)
    print(f"embed.weight: {plan['kind']} drawn at {plan['src_dtype']}, stored "
          f"as {plan['dtype']}, patches {plan['patches']}")

    shards = [
        materialize_module_dim0_sharded(model, rank, world_size)
        for rank in range(world_size)
    ]
    rows = VOCAB // world_size
    assert all(s["embed.weight"].shape == (rows, DIM) for s in shards)
    assert (shards[0]["embed.weight"][PAD] == 0).all()

    full = materialize_tensor(model.embed.weight).detach()
    got = torch.cat([s["embed.weight"].detach() for s in shards])
    assert torch.equal(got, full)
    print(f"{world_size} row shards of {rows} x {DIM} bf16 reassemble to the "
          f"full table on {device}; row {PAD} is zero")


if __name__ == "__main__":
    main()
