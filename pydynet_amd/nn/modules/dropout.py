"""Inverted dropout (surface of pydynet/nn/modules/dropout.py); the mask is drawn on the host, or, with a
`pydynet_amd.Generator`, on the device (core/fused/dropout.py: no host random numbers, replayable from a `hipnp.Graph`)."""
from .module import Module
from ...special import rand


class Dropout(Module):
    def __init__(self, p: float = 0.5, generator=None) -> None:
        super().__init__()
        assert 0 <= p < 1
        self.p = p
        self.generator = generator

    def __repr__(self) -> str:
        return f"Dropout(p={self.p})" if self.generator is None else f"Dropout(p={self.p}, generator={self.generator})"

    def forward(self, x):
        if not self._train:
            return x
        if self.generator is not None:
            from ...core import fused
            return fused.dropout(x, self.p, self.generator)
        keep = 1 - self.p
        kept = (rand(*x.shape, device=x.device) < keep).astype(x.dtype)      # one host draw per element, as the reference
        return x * kept / keep
