"""Utilities over a model's parameters.  `clip_grad_norm_` is the stand-alone form of the clipping that
`optim.Adam(max_grad_norm=)` does inside its step: for SGD, Adagrad, Adadelta and hand-written loops."""
import numpy as np

from ..core import Tensor
from ..optim import clip as _clip

_CHUNK = 16384
_tables = {}          # (gradient address, size) per parameter -> (chunk table, partials, ctl) on the device


def _fused(params):
    return all(p.device.is_hip and p.device == params[0].device and p.grad.dtype == np.float32
               and p.grad.is_contiguous() for p in params)


def _buffers(params):
    from .. import hipnp
    key = tuple((p.grad._ptr, p.grad.size) for p in params)
    ent = _tables.get(key)
    if ent is None:
        if len(_tables) >= 8:                         # gradients were re-allocated a few times: forget the old tables
            _tables.clear()
        rows = [(0, p.grad._ptr + 4 * off, 0, 0, min(_CHUNK, p.grad.size - off))
                for p in params for off in range(0, p.grad.size, _CHUNK)]
        table = hipnp.from_numpy(np.asarray(rows, dtype=np.int64).reshape(-1, 5))
        ent = _tables[key] = (table, hipnp.empty((len(rows),), np.float64), hipnp.zeros((4,), np.float32))
    return ent


def clip_grad_norm_(parameters, max_norm, norm_type=2.0):
    """Scale the gradients of `parameters` IN PLACE so that their global 2-norm is at most `max_norm`
    (g *= min(1, max_norm / (norm + 1e-6)), optim/clip.py) and return the norm they had, as a 0-d `Tensor` on the
    gradients' device.  Unlike `Adam(max_grad_norm=)` this rewrites the gradients.  A non-finite norm leaves them
    untouched.  Float32 contiguous gradients on one HIP device take two launches (norm, scale: csrc/optim.hip)
    through a chunk table cached on the gradients' addresses, with no host round trip; everything else takes the
    array statement.  NOT capturable in a `hipnp.Graph` (the cached table is not owned by the graph): it raises
    there; inside a graph use `Adam(max_grad_norm=)`."""
    if float(norm_type) != 2.0:
        raise ValueError(f"clip_grad_norm_ supports norm_type 2 only, got {norm_type!r}")
    if not max_norm > 0:
        raise ValueError(f"max_norm must be positive, got {max_norm!r}")
    if isinstance(parameters, Tensor):
        parameters = [parameters]
    params = [p for p in parameters if p.grad is not None]
    if not params:
        return Tensor(np.zeros((), np.float32))
    dev = params[0].device
    if _fused(params):
        from .. import hipnp, _lib
        if hipnp.capturing() is not None:
            raise RuntimeError("clip_grad_norm_ cannot be captured in a hipnp.Graph; use Adam(max_grad_norm=)")
        with dev:
            table, partials, ctl = _buffers(params)
            L = _lib.lib()
            L.call("pdnx_grad_norm_multi_f32", table._ptr, table.shape[0], 1.0, float(max_norm), partials._ptr, ctl._ptr,
                   hipnp.stream())
            L.call("pdnx_grad_scale_multi_f32", table._ptr, table.shape[0], ctl._ptr, hipnp.stream())
            return Tensor(ctl[0], device=dev)         # (a copy: the next call overwrites ctl)
    norm = _clip.total_norm([p.grad for p in params])
    coef, finite = _clip.coefficient(norm, max_norm)
    if finite and coef != 1.0:
        for p in params:
            with p.device:
                p.grad *= coef
    return Tensor(np.array(norm, np.float32), device=dev)
