"""Optimizers (surface of pydynet/optim/optimizer.py).  They update the raw `param.data`
arrays in place, as the reference does.  `Adam` on HIP parameters is ONE multi-tensor kernel
launch per step (the reference runs 8 array expressions per parameter, optimizer.py:185-196);
SGD / Adagrad / Adadelta are plain array expressions through `xp`."""
from math import sqrt

import numpy as np

from ..core import Tensor


class Optimizer:
    def __init__(self, params) -> None:
        self.params = list(params)
        self._flat_grad = None
        # data parallel: gradients arrive as the SUM over ranks and every optimizer applies
        # `grad_scale` = 1 / world_size (Adam folds it into its kernel)
        self.grad_scale = 1.0

    def _grad(self, p, weight_decay):
        g = p.grad * self.grad_scale if self.grad_scale != 1.0 else p.grad
        return g + weight_decay * p.data

    def step(self):
        raise NotImplementedError

    def zero_grad(self):
        if self._flat_grad is not None and self._flat_ok():
            with self.params[0].device:
                self._flat_grad[...] = 0.          # one fill instead of one per parameter
            return
        for p in self.params:
            p.zero_grad()

    def flatten_grads(self):
        """Move all gradients into one flat buffer (see optim/flat.py); optional, HIP or CPU."""
        from .flat import flatten_gradients
        self._flat_grad, self._flat_offsets = flatten_gradients(self.params)
        self._flat_views = [p.grad for p in self.params]
        return self._flat_grad

    def _flat_ok(self):
        # user code may have re-assigned p.grad; fall back to per-parameter zeroing then
        for p, v in zip(self.params, self._flat_views):
            if p.grad is not v:
                return False
        return True

    def _state(self):
        out = []
        for p in self.params:
            with p.device:
                out.append(p.xp.zeros(p.shape, dtype=p.dtype))
        return out


class SGD(Optimizer):
    """Momentum SGD with optional Nesterov look-ahead (optimizer.py:32-74)."""

    def __init__(self, params, lr, momentum=.5, weight_decay=0., nesterov=True) -> None:
        super().__init__(params)
        self.lr, self.momentum, self.weight_decay, self.nesterov = lr, momentum, weight_decay, nesterov
        self.v = self._state()

    def step(self):
        for p, v in zip(self.params, self.v):
            with p.device:
                grad = self._grad(p, self.weight_decay)
                v *= self.momentum
                v += self.lr * grad
                p.data -= v
                if self.nesterov:
                    p.data -= self.lr * grad


class Adagrad(Optimizer):
    """optimizer.py:77-112 (eps inside the square root)."""

    def __init__(self, params, lr=1e-2, weight_decay=0, eps=1e-10) -> None:
        super().__init__(params)
        self.lr, self.weight_decay, self.eps = lr, weight_decay, eps
        self.G = self._state()

    def step(self):
        for p, G in zip(self.params, self.G):
            with p.device:
                grad = self._grad(p, self.weight_decay)
                G += grad ** 2
                p.data -= self.lr * grad / (self.eps + G) ** 0.5


class Adadelta(Optimizer):
    """optimizer.py:115-157 (as written there: an RMSprop-style update)."""

    def __init__(self, params, lr=1.0, rho=0.9, weight_decay=0, eps=1e-6) -> None:
        super().__init__(params)
        self.lr, self.rho, self.eps, self.weight_decay = lr, rho, eps, weight_decay
        self.G = self._state()

    def step(self):
        for i, p in enumerate(self.params):
            with p.device:
                grad = self._grad(p, self.weight_decay)
                self.G[i] = self.rho * self.G[i] + (1 - self.rho) * grad ** 2
                p.data -= self.lr * grad / (self.G[i] + self.eps) ** 0.5


class Adam(Optimizer):
    """Adam with the reference's exact arithmetic (optimizer.py:160-196): step counter starts at
    1, a_t = sqrt(1-b2^t)/(1-b1^t) is a host scalar, and eps is added to sqrt(v) WITHOUT the
    bias-correction divisor (this differs from PyTorch and is kept).

    Two extensions the reference lacks (statement: optim/clip.py, kernels: csrc/optim.hip); with both left at their
    defaults the step issues exactly the entry points it always did:

    `max_grad_norm=m` clips by the global 2-norm inside the step: the update uses g * grad_scale * coef with
    coef = min(1, m / (norm + 1e-6)); the gradients in memory are NOT rewritten.  On the fused HIP path norm and
    coef never leave the device, so the step stays capturable in a `hipnp.Graph`.  `last_grad_norm` is the norm of
    the latest step as a device scalar (read it with `hipnp.read_later` to avoid a sync).  A non-finite norm skips
    the whole update -- p, m and v keep their bits and `skipped_steps()` goes up by one -- but the step counter `t`
    STILL ADVANCES: the host cannot learn of the skip without a sync, and eager and replayed steps must agree.
    When clipping is set and some parameter does not qualify for the fused path (float64, non-contiguous), ALL
    parameters take the array path: a norm over half the model would be wrong.

    `decoupled_weight_decay=True` (what `AdamW` sets): p -= lr * weight_decay * p first (the plain rate, not
    lr * a_t), then the update without weight_decay * p in the gradient.  This is the reference's Adam with the decay
    decoupled, not a bit-copy of PyTorch's AdamW: the eps placement stays.

    Replayed steps read `lr` again at every replay: a changed rate is copied to the device (8 bytes, `pdn_memcpy_h2d`)
    ahead of the graph launch; a constant rate costs nothing.  That copy WAITS for the stream: a schedule that moves the
    rate at every step (CosineAnnealingLR) makes the host wait for the previous replay before it launches the next."""

    CHUNK = 16384

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, max_grad_norm=None,
                 decoupled_weight_decay=False) -> None:
        super().__init__(params)
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError(f"max_grad_norm must be positive or None, got {max_grad_norm!r}")
        self.lr = lr
        self.beta1, self.beta2 = betas
        self.eps, self.weight_decay = eps, weight_decay
        self.max_grad_norm, self.decoupled_weight_decay = max_grad_norm, bool(decoupled_weight_decay)
        self.m, self.v = self._state(), self._state()
        self.t = 1
        self._table = None
        self._table_key = None
        self.last_grad_norm = None          # set by every clipped step
        self._ctl = self._partials = None   # device float[4] {norm, coef, skip, skipped steps} / double[nchunks]
        self._skipped_host = 0              # skips counted by the array path

    def skipped_steps(self) -> int:
        """Updates skipped so far because the gradient norm was not finite (reads one device word: synchronises)."""
        return self._skipped_host + (int(self._ctl[3].item()) if self._ctl is not None else 0)

    # -- HIP multi-tensor path ------------------------------------------------------------
    def _hip_params(self):
        return [i for i, p in enumerate(self.params)
                if p.device.is_hip and p.dtype == np.float32 and p.grad is not None
                and p.grad.dtype == np.float32 and p.data.is_contiguous() and p.grad.is_contiguous()]

    def _chunk_table(self, idx):
        key = tuple((self.params[i].data._ptr, self.params[i].grad._ptr) for i in idx)
        if key != self._table_key:
            from .. import hipnp
            rows = []
            for i in idx:
                p = self.params[i]
                for off in range(0, p.size, self.CHUNK):
                    n = min(self.CHUNK, p.size - off)
                    rows.append((p.data._ptr + 4 * off, p.grad._ptr + 4 * off,
                                 self.m[i]._ptr + 4 * off, self.v[i]._ptr + 4 * off, n))
            self._table = hipnp.from_numpy(np.asarray(rows, dtype=np.int64).reshape(-1, 5))
            self._table_key = key
        return self._table

    def _clip_buffers(self, table):
        """(partials, ctl) for `table`: ctl is made once (its skip count persists), partials once per table."""
        from .. import hipnp
        if self._ctl is None:
            self._ctl = hipnp.zeros((4,), np.float32)
        if self._partials is None or self._partials.shape[0] != table.shape[0]:
            self._partials = hipnp.empty((table.shape[0],), np.float64)
        return self._partials, self._ctl

    def _seed_tick(self, words):
        """Warm-up run inside a graph's pool: {t, lr} go to the device, where replays find and advance them."""
        from .. import hipnp
        self._tick = (hipnp.from_numpy(np.array([float(self.t), float(self.lr)])), hipnp.empty((words,), np.float32))
        self._lr_pushed = self.lr
        self._lr_host = np.zeros(1, np.float64)      # source of the 8-byte copy below; lives as long as the optimizer

    def _replay_hook(self):
        from .. import hipnp, _lib
        state = self._tick[0]

        def advance(opt=self):
            opt.t += 1
            if opt.lr != opt._lr_pushed:             # a scheduler moved the rate since the last replay
                opt._lr_host[0] = opt.lr
                _lib.lib().call("pdn_memcpy_h2d", state._ptr + 8, opt._lr_host.ctypes.data, 8, hipnp.stream())
                opt._lr_pushed = opt.lr
        return advance

    def step(self):
        a_t = sqrt(1 - self.beta2 ** self.t) / (1 - self.beta1 ** self.t)
        clip, decoupled = self.max_grad_norm is not None, self.decoupled_weight_decay
        fast = self._hip_params() if self.params and self.params[0].device.is_hip else []
        if fast:
            from .. import hipnp, _lib
            graph = hipnp.capturing()
            if graph is not None and len(fast) != len(self.params):
                raise RuntimeError("Adam inside a hipnp.Graph needs all parameters on the fused HIP path")
            if clip and len(fast) != len(self.params):
                fast = []                                # one norm over ALL gradients: everything takes the array path
        if fast:
            with self.params[fast[0]].device:
                table = self._chunk_table(fast)
                partials, ctl = self._clip_buffers(table) if clip else (None, None)
                if clip:
                    self.last_grad_norm = ctl[0]
                if graph is not None:
                    graph.pin(table)                     # the captured launch holds the table's address
                    if clip:
                        graph.pin(partials), graph.pin(ctl)
                    # replayed steps cannot take a host scalar: {t, lr} live on the device, a one-thread
                    # kernel forms lr * a_t there and advances t (the host counter follows at every replay)
                    if graph.warming:                    # the eager run inside the graph's pool: seed the device state
                        self._seed_tick(2 if clip or decoupled else 1)
                    else:
                        graph.on_replay(self._replay_hook())
                        self.t -= 1                      # the captured run executes nothing; replay() counts it
                    if clip or decoupled:
                        _lib.lib().call("pdnx_adam_multi_clip_tick_f32", table._ptr, table.shape[0], self._tick[0]._ptr,
                                        self._tick[1]._ptr, self.beta1, self.beta2, self.eps, self.weight_decay,
                                        self.grad_scale, float(self.max_grad_norm) if clip else 0.0, int(decoupled),
                                        partials._ptr if clip else None, ctl._ptr if clip else None, hipnp.stream())
                    else:
                        _lib.lib().call("pdn_adam_multi_tick_f32", table._ptr, table.shape[0], self._tick[0]._ptr,
                                        self._tick[1]._ptr, self.beta1, self.beta2, self.eps, self.weight_decay,
                                        self.grad_scale, hipnp.stream())
                elif clip or decoupled:
                    if clip:
                        _lib.lib().call("pdnx_grad_norm_multi_f32", table._ptr, table.shape[0], self.grad_scale,
                                        float(self.max_grad_norm), partials._ptr, ctl._ptr, hipnp.stream())
                    _lib.lib().call("pdnx_adam_multi_clip_f32", table._ptr, table.shape[0], self.lr * a_t,
                                    self.lr * self.weight_decay, self.beta1, self.beta2, self.eps, self.weight_decay,
                                    self.grad_scale, int(decoupled), ctl._ptr if clip else None, hipnp.stream())
                else:
                    _lib.lib().call("pdn_adam_multi_f32", table._ptr, table.shape[0], self.lr * a_t,
                                    self.beta1, self.beta2, 1 - self.beta1, 1 - self.beta2, self.eps,
                                    self.weight_decay, self.grad_scale, hipnp.stream())
        done = set(fast)
        if clip or decoupled:
            self._array_step([i for i in range(len(self.params)) if i not in done], a_t, clip)
        else:
            for i, p in enumerate(self.params):
                if i in done:
                    continue
                with p.device:
                    grad = self._grad(p, self.weight_decay)
                    self.m[i] *= self.beta1
                    self.m[i] += (1 - self.beta1) * grad
                    self.v[i] *= self.beta2
                    self.v[i] += (1 - self.beta2) * grad ** 2
                    p.data -= self.lr * a_t * self.m[i] / (self.v[i] ** 0.5 + self.eps)
        self.t += 1

    def _array_step(self, idx, a_t, clip):
        """optim/clip.py for the parameters `idx`: all of them when clipping (then nothing ran fused), else the ones the
        fused launch left out.  The norm comes to the host here (one read-back per device gradient)."""
        from . import clip as C
        if not idx:
            return
        scale = float(self.grad_scale)
        if clip:
            p0 = self.params[idx[0]]
            with p0.device:
                norm = C.total_norm([self.params[i].grad for i in idx], self.grad_scale)
                self.last_grad_norm = p0.xp.full((), norm, dtype=np.float32)
            coef, finite = C.coefficient(norm, self.max_grad_norm)
            if not finite:
                self._skipped_host += 1
                return
            scale *= coef
        for i in idx:
            p = self.params[i]
            with p.device:
                C.adam_update(p.data, p.grad, self.m[i], self.v[i], self.lr * a_t, self.lr * self.weight_decay, self.beta1,
                              self.beta2, self.eps, self.weight_decay, scale, self.decoupled_weight_decay)


class AdamW(Adam):
    """`Adam` with decoupled weight decay (see there) and the customary default of 1e-2."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None) -> None:
        super().__init__(params, lr, betas, eps, weight_decay, max_grad_norm, decoupled_weight_decay=True)
