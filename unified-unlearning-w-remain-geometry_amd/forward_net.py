"""What the forward-only nets (vae._VAENet, resnet.ResNet, text.CLIPTextEncoder) share on the host, and the one statement of the 2 GiB
operand rule: the products take their operands through buffer resources sized by a 32-bit byte count, so the
library refuses an operand of 2 GiB or more, and every launch asserts its operands first so that the caller sees which tensor is too large.
"""
import numpy as np
import torch

from . import _lib

LIMIT = 1 << 31           # bytes: no operand of a launch may reach this (32-bit buffer-resource sizes, csrc/common.h)


def guard(*tensors):
    for t in tensors:
        if t is not None and not isinstance(t, int):
            nb = t.numel() * t.element_size()
            assert nb < LIMIT, f"operand of {nb} bytes: a launch may not read or write 2 GiB or more (chunk the batch)"


class ForwardNet:
    """A net that only runs forward: weights in one fp32 arena ``params`` with a bf16 shadow ``params_bf16`` of what the products read,
    ``index`` {arena name: element offset}, activations in workspaces reused by every later call.  The subclass fills the arena;
    constructing the base allocates nothing on the device."""

    _UNTILED = ""             # what chunk_size adds when one sample alone is too large, e.g. " (tiled encoding is not supported)"

    def __init__(self, device):
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise _lib.SfronError(f"{type(self).__name__} needs a GPU (no CPU fallback)")
        self._ws = {}

    def _buf(self, key, numel, dtype):
        """A view of the first numel elements of workspace `key` (grown, never shrunk; reused by every later call)."""
        t = self._ws.get(key)
        if t is None or t.numel() < numel:
            self._ws[key] = t = torch.empty(numel, dtype=dtype, device=self.dev)
        return t[:numel]

    def _p(self, name):
        return self.params.data_ptr() + 4 * self.index[name]

    def _w(self, name):
        return self.params_bf16.data_ptr() + 2 * self.index[name]

    def view(self, name):
        """The fp32 arena entry `name` in the shape ``specs`` gives it (for the nets whose arena holds the state dict's own tensors)."""
        shp = self.specs[name]
        return self.params[self.index[name]:self.index[name] + int(np.prod(shp))].view(shp)

    def chunk_size(self, H, W):
        """Samples per run such that the largest operand (``per_sample_bytes`` each) stays under ``max_chunk_bytes`` and under 2 GiB."""
        ps = self.per_sample_bytes(H, W)
        if ps >= LIMIT:
            raise ValueError(f"one {H}x{W} image needs a {ps}-byte operand: above 2 GiB{self._UNTILED}")
        return max(1, min(self.max_chunk_bytes, LIMIT - 1) // ps)
