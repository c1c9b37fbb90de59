"""Sampled next tokens for `Llama.generate`: temperature, top-k and top-p (nucleus), seeded and reproducible.

The reference's `generate` (llm/llama/model.py:258-269) only takes the argmax.  This module states the sampled pick and
runs it: on a HIP device through `pdn_sample_rows_f32` (csrc/sample.hip), elsewhere through the NumPy statement below,
which IS the contract (the kernel computes the same in fp32 / integer mass units).

For one row of logits z (length V) and temperature T > 0:
  1. top-k (k = 0 or k >= V: off): keep every token with z_i >= z_(k), the k-th largest value counting repeats;
  2. p_i = exp((z_i - max z) / T) over the kept tokens, normalised;
  3. top-p (top_p = 1: off): theta = the largest kept value such that the mass of {kept i : z_i >= theta} is at least
     top_p; keep exactly those (ties at theta are all kept);
  3b. min_p (min_p = 0: off; applied after top-k and top-p): a token kept so far stays kept iff
     exp((z_i - max z) / T) >= min_p -- its probability is at least min_p times the largest; the maximum always stays;
  4. renormalise; u = (w >> 40) * 2^-24 with w the first 64-bit word of Philox4x64-10 for counter (t, b, 0, 0) and key
     (seed, 0); the token is the smallest kept id whose inclusive cumulative probability (ascending ids) is > u.
`t` is the position of the generate-loop iteration that yields the token, `b` the batch row.

Per request (`generate_ragged`, `serve`, `serve_all`): each of temperature, top_k, top_p, seed and min_p is one value or a
sequence with one value per request (`check_request_args`, `Table`).  Request r then follows the statement above with its
own values, key (seed_r, 0) and counter (t, r); a request with temperature 0 in a run that samples takes the first maximum
of its logit row.  On a HIP device the per-row entries of include/pdn_persample.h (prefix pdnq_) run it; a library without
them, and every other device, applies `sample_rows_np` row by row.
"""
import numpy as np

_M0, _M1 = 0xD2E7470EE14C6C93, 0xCA5A826395121157
_W0, _W1 = 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B
_MASK32 = np.uint64(0xFFFFFFFF)


def check_args(temperature, top_k, top_p, seed):
    """Validate the sampling arguments of `generate`; returns them normalised (float, int, float, int)."""
    temperature, top_p = float(temperature), float(top_p)
    if not temperature >= 0.0:
        raise ValueError(f"temperature must be >= 0, got {temperature}")
    if int(top_k) != top_k or top_k < 0:
        raise ValueError(f"top_k must be a non-negative integer, got {top_k}")
    if not 0.0 < top_p <= 1.0:
        raise ValueError(f"top_p must lie in (0, 1], got {top_p}")
    if int(seed) != seed or not 0 <= int(seed) < 2 ** 64:
        raise ValueError(f"seed must be an integer in [0, 2^64), got {seed}")
    return temperature, int(top_k), top_p, int(seed)


def check_min_p(min_p):
    """Validate min_p: a float in [0, 1), 0 = off."""
    min_p = float(min_p)
    if not 0.0 <= min_p < 1.0:
        raise ValueError(f"min_p must lie in [0, 1), got {min_p}")
    return min_p


class Table:
    """Sampling parameters per request: (N,) arrays temperature, top_k, top_p, seed, min_p (checked values).  The three
    floats are held as the float32 values the device's parameter block stores (float32(0.1) > 0.1), so the statement on
    `cpu` draws with exactly the numbers the kernels read: a weight between the two roundings cannot split the devices."""

    def __init__(self, temperature, top_k, top_p, seed, min_p):
        f32 = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
        self.temperature, self.top_p, self.min_p = f32(temperature), f32(top_p), f32(min_p)
        self.top_k, self.seed = np.asarray(top_k, np.int64), np.asarray(seed, np.uint64)
        self.n = self.temperature.size
        self._blocks = np.stack([params_bytes(*self.row(r)) for r in range(self.n)])

    def row(self, r):
        """Request r's (temperature, top_k, top_p, seed, min_p)."""
        return (float(self.temperature[r]), int(self.top_k[r]), float(self.top_p[r]), int(self.seed[r]),
                float(self.min_p[r]))

    def blocks(self, reqs):
        """pdn_sample_params of requests `reqs`, (len(reqs), 3) int64 (a request < 0: request 0's, never read)."""
        return self._blocks[np.maximum(np.asarray(reqs, np.int64).reshape(-1), 0)]

    def draw_np(self, z, positions, reqs, rows):
        """The statement row by row: row b of z (B, V) with request reqs[b]'s values and counter (positions[b], rows[b])."""
        out = np.empty(len(z), np.int64)
        for b in range(len(z)):
            T, k, p, seed, m = self.row(int(reqs[b]))
            out[b] = sample_rows_np(z[b:b + 1], int(positions[b]), T, k, p, seed, rows=[int(rows[b])], min_p=m)[0]
        return out


def check_request_args(temperature, top_k, top_p, seed, min_p, n, what="request"):
    """Validate the sampling arguments of a call with `n` requests, each one value or a sequence of n values (every entry
    by the rules of `check_args` / `check_min_p`; ValueError names the request, or the argument of a wrong length).
    Returns `check_args`' tuple when every argument is one value and min_p is 0, else a `Table`."""
    args = {"temperature": temperature, "top_k": top_k, "top_p": top_p, "seed": seed, "min_p": min_p}
    seqs = {k for k, v in args.items() if np.ndim(v) > 0}
    if not seqs:
        out, m = check_args(temperature, top_k, top_p, seed), check_min_p(min_p)
        return out if m == 0.0 else Table(*([v] * n for v in out), [m] * n)
    for k in sorted(seqs):
        args[k] = list(args[k])
        if len(args[k]) != n:
            raise ValueError(f"{k}: {len(args[k])} values for {n} {what}s")
    cols = []
    for r in range(n):
        v = {k: a[r] if k in seqs else a for k, a in args.items()}
        try:
            cols.append(check_args(v["temperature"], v["top_k"], v["top_p"], v["seed"]) + (check_min_p(v["min_p"]),))
        except (ValueError, TypeError) as e:
            raise ValueError(f"{what} {r}: {e}") from None
    return Table(*zip(*cols))


def active(checked):
    """What a generation runs with: None (greedy: every temperature 0), the scalar tuple, or the Table."""
    if isinstance(checked, Table):
        return checked if (checked.temperature > 0).any() else None
    return checked if checked[0] > 0 else None


def _mulhilo(a, b):
    """(hi, lo) 64-bit halves of the 128-bit products a * b of uint64 arrays (b a scalar constant)."""
    b = np.uint64(b)
    a_lo, a_hi = a & _MASK32, a >> np.uint64(32)
    b_lo, b_hi = b & _MASK32, b >> np.uint64(32)
    ll, lh, hl, hh = a_lo * b_lo, a_lo * b_hi, a_hi * b_lo, a_hi * b_hi
    mid = (ll >> np.uint64(32)) + (lh & _MASK32) + (hl & _MASK32)
    hi = hh + (lh >> np.uint64(32)) + (hl >> np.uint64(32)) + (mid >> np.uint64(32))
    return hi, a * b


def philox4x64(counter, key):
    """Philox4x64-10 blocks: counter (..., 4) and key (..., 2) uint64 -> (..., 4) uint64 (Salmon et al., SC'11)."""
    c = np.array(np.broadcast_to(np.asarray(counter, np.uint64), np.broadcast_shapes(np.shape(counter)[:-1] + (4,),
                                                                                    np.shape(key)[:-1] + (4,))))
    k = np.array(np.broadcast_to(np.asarray(key, np.uint64), c.shape[:-1] + (2,)))
    with np.errstate(over="ignore"):
        for r in range(10):
            if r:
                k[..., 0] += np.uint64(_W0)
                k[..., 1] += np.uint64(_W1)
            hi0, lo0 = _mulhilo(c[..., 0], _M0)
            hi1, lo1 = _mulhilo(c[..., 2], _M1)
            c = np.stack([hi1 ^ c[..., 1] ^ k[..., 0], lo1, hi0 ^ c[..., 3] ^ k[..., 1], lo0], axis=-1)
    return c


def uniforms(t, rows, seed):
    """u in [0, 1) for counters (t, b, 0, 0), b in `rows`, key (seed, 0): (w >> 40) * 2^-24 of the block's first word."""
    rows = np.asarray(rows, np.uint64).reshape(-1)
    ctr = np.zeros((rows.size, 4), np.uint64)
    ctr[:, 0], ctr[:, 1] = np.uint64(t), rows
    w = philox4x64(ctr, np.array([seed, 0], np.uint64))[:, 0]
    return (w >> np.uint64(40)).astype(np.float64) * 2.0 ** -24


def kept_mask(z, top_k, top_p, temperature, min_p=0.0):
    """Steps 1-3b for one float64 row: the kept tokens and their renormalised probabilities (0 elsewhere)."""
    V = z.shape[0]
    kept = np.ones(V, bool)
    if 0 < top_k < V:
        kept = z >= np.partition(z, V - top_k)[V - top_k]
    w = np.where(kept, np.exp((z - z.max()) / temperature), 0.0)
    p = w / w.sum()
    if top_p < 1.0:
        vals, grp = np.unique(z[kept], return_inverse=True)
        cum = np.cumsum(np.bincount(grp.reshape(-1), weights=p[kept], minlength=vals.size)[::-1])   # largest value first
        theta = vals[::-1][min(int(np.searchsorted(cum, top_p, side="left")), vals.size - 1)]
        kept &= z >= theta
        p = np.where(kept, p, 0.0)
        p /= p.sum()
    if min_p > 0.0:
        kept &= np.exp((z - z.max()) / temperature) >= min_p
        p = np.where(kept, p, 0.0)
        p /= p.sum()
    return kept, p


def sample_rows_np(logits, t, temperature, top_k=0, top_p=1.0, seed=0, rows=None, min_p=0.0):
    """The NumPy statement of the contract: (B, V) logits -> (B,) int64 ids, row b drawn with counter (t, rows[b])."""
    z = np.asarray(logits, np.float64)
    B = z.shape[0]
    rows = np.arange(B) if rows is None else np.asarray(rows)
    if temperature == 0.0:
        return z.argmax(-1).astype(np.int64)
    u = uniforms(t, rows, seed)
    out = np.empty(B, np.int64)
    for b in range(B):
        _, p = kept_mask(z[b], top_k, top_p, temperature, min_p)
        cdf = np.cumsum(p)
        i = int(np.searchsorted(cdf, u[b], side="right"))     # first inclusive prefix > u
        out[b] = i if i < z.shape[1] and p[i] > 0 else int(np.flatnonzero(p)[-1])
    return out


def params_bytes(temperature, top_k, top_p, seed, min_p=0.0):
    """pdn_sample_params (include/pdn_hip.h) as three int64 words: {float T; int top_k; float top_p; float min_p;
    uint64_t seed}."""
    raw = np.zeros(24, np.uint8)
    raw[0:4] = np.frombuffer(np.float32(temperature).tobytes(), np.uint8)
    raw[4:8] = np.frombuffer(np.int32(top_k).tobytes(), np.uint8)
    raw[8:12] = np.frombuffer(np.float32(top_p).tobytes(), np.uint8)
    raw[12:16] = np.frombuffer(np.float32(min_p).tobytes(), np.uint8)
    raw[16:24] = np.frombuffer(np.uint64(seed).tobytes(), np.uint8)
    return raw.view(np.int64)


def params_buffer(temperature, top_k, top_p, seed):
    """A device copy of pdn_sample_params on the current HIP device (the allocator orders its reuse on the stream)."""
    from .. import hipnp as hp
    return hp.asarray(params_bytes(temperature, top_k, top_p, seed))


def sample_next(logits, t, temperature, top_k=0, top_p=1.0, seed=0):
    """Sampled next ids of a (B, V) logits Tensor: (B, 1) int64 on the logits' device.  temperature 0 = argmax."""
    from ..core import Tensor
    temperature, top_k, top_p, seed = check_args(temperature, top_k, top_p, seed)
    if temperature == 0.0:
        return logits.argmax(-1, True)
    B, V = logits.shape
    if logits.device.is_hip:
        from .. import hipnp as hp, _lib
        x = logits.data
        if x.dtype != np.float32:
            raise TypeError(f"sampling takes float32 logits on the GPU, got {x.dtype}")
        if x._strides[1] != 1 or x._strides[0] < V:
            x = x.copy()
        out = hp.empty((B, 1), np.int64)
        _lib.lib().call("pdn_sample_rows_f32", x._ptr, x._strides[0], B, V,
                        params_buffer(temperature, top_k, top_p, seed)._ptr, int(t), out._ptr, hp.stream())
        return Tensor(out, dtype=np.int64, device=logits.device, copy=False)
    ids = sample_rows_np(np.asarray(logits.numpy()), t, temperature, top_k, top_p, seed)
    return Tensor(ids.reshape(B, 1), dtype=np.int64, device=logits.device)


def sample_next_rows(logits, positions, temperature, top_k=0, top_p=1.0, seed=0, rows=None):
    """`sample_next` with a counter per row: row b of the (B, V) logits Tensor drawn with counter (positions[b], rows[b])
    (Llama.generate_ragged: every row at its own position; Llama.serve: `rows` = the request each row holds).  `rows`
    defaults to arange(B).  (B, 1) int64 on the logits' device."""
    from ..core import Tensor
    temperature, top_k, top_p, seed = check_args(temperature, top_k, top_p, seed)
    if temperature == 0.0:
        return logits.argmax(-1, True)
    B, V = logits.shape
    positions = np.asarray(positions, np.int64).reshape(B)
    if logits.device.is_hip:
        from .. import hipnp as hp, _lib
        x = logits.data
        if x.dtype != np.float32:
            raise TypeError(f"sampling takes float32 logits on the GPU, got {x.dtype}")
        if x._strides[1] != 1 or x._strides[0] < V:
            x = x.copy()
        out = hp.empty((B, 1), np.int64)
        pos, step = hp.asarray(positions.astype(np.int32)), hp.zeros((1,), np.int32)   # (the tick advances these copies)
        prm = params_buffer(temperature, top_k, top_p, seed)
        if rows is None:
            _lib.lib().call("pdn_decode_sample_tick_rows_f32", x._ptr, x._strides[0], B, V, prm._ptr, out._ptr, pos._ptr,
                            step._ptr, None, None, None, 0, 0, None, hp.stream())
        else:                                      # (the served tick: counter ids per row, a budget of one token)
            req, left = hp.asarray(np.asarray(rows, np.int32).reshape(B)), hp.asarray(np.ones(B, np.int32))
            _lib.lib().call("pdn_decode_sample_tick_slots_f32", x._ptr, x._strides[0], B, V, prm._ptr, out._ptr,
                            pos._ptr, step._ptr, req._ptr, left._ptr, 1, None, None, None, 0, 0, None, hp.stream())
        return Tensor(out, dtype=np.int64, device=logits.device, copy=False)
    z = np.asarray(logits.numpy())
    rows = np.arange(B) if rows is None else np.asarray(rows, np.int64).reshape(B)
    ids = np.array([sample_rows_np(z[b:b + 1], int(positions[b]), temperature, top_k, top_p, seed, rows=[rows[b]])[0]
                    for b in range(B)], np.int64)
    return Tensor(ids.reshape(B, 1), dtype=np.int64, device=logits.device)


def sample_next_table(logits, positions, table, reqs, rows=None):
    """`sample_next_rows` with parameters per row: row b of the (B, V) logits Tensor drawn with request reqs[b]'s values
    of `table` (a `Table`) and counter (positions[b], rows[b]); `rows` defaults to arange(B).  On a HIP device:
    pdnq_sample_rows_f32 (include/pdn_persample.h); a library without it, and every other device: the statement row by
    row.  (B, 1) int64 on the logits' device."""
    from ..core import Tensor
    B, V = logits.shape
    positions = np.asarray(positions, np.int64).reshape(B)
    reqs = np.asarray(reqs, np.int64).reshape(B)
    rows = np.arange(B) if rows is None else np.asarray(rows, np.int64).reshape(B)
    if logits.device.is_hip:
        from .. import hipnp as hp, _lib
        if _lib.provides("pdnq_sample_rows_f32"):
            x = logits.data
            if x.dtype != np.float32:
                raise TypeError(f"sampling takes float32 logits on the GPU, got {x.dtype}")
            if x._strides[1] != 1 or x._strides[0] < V:
                x = x.copy()
            out = hp.empty((B, 1), np.int64)
            prm, pos, rq = (hp.asarray(table.blocks(reqs)), hp.asarray(positions.astype(np.int32)),
                            hp.asarray(rows.astype(np.int32)))
            _lib.lib().call("pdnq_sample_rows_f32", x._ptr, x._strides[0], B, V, prm._ptr, pos._ptr, rq._ptr, out._ptr,
                            hp.stream())
            return Tensor(out, dtype=np.int64, device=logits.device, copy=False)
    ids = table.draw_np(np.asarray(logits.numpy()), positions, reqs, rows)
    return Tensor(ids.reshape(B, 1), dtype=np.int64, device=logits.device)


def draw_rows(logits, positions, sampling, reqs, rows=None):
    """The draw of a prompt pass or a step off the graph path: `sampling` is the call's scalar tuple (`sample_next_rows`)
    or its `Table` (`sample_next_table`, row b with request reqs[b]'s values)."""
    if isinstance(sampling, Table):
        return sample_next_table(logits, positions, sampling, reqs, rows)
    return sample_next_rows(logits, positions, *sampling, rows=rows)
