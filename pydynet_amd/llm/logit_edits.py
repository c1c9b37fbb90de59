"""Per-request logit edits for `Llama.generate`, `generate_ragged`, `serve` and `serve_all`: `allowed_token_ids`,
`logit_bias` and `min_new_tokens`.

This module states the contract in NumPy; on a HIP device the graph-replayed steps run it through csrc/logit_edit.hip
(include/pdn_logitedit.h), which computes the same bits.  For row b's fp32 logits z (length V) at the step that yields the
token at position t, with s_b the row's prompt length, in this order -- after the penalties of llm/penalties.py when
those are on:
  1. allowed_token_ids A_b (None: every token): for every v not in A_b, z[v] = -inf;
  2. logit_bias {v: beta}, beta a float32: beta finite: z[v] = fl32(z[v] + beta), one float32 rounding, no fused
     multiply-add; beta = -inf: z[v] = -inf -- an assignment, not an addition, so that a logit of +inf cannot turn into
     NaN; beta = +inf or NaN is rejected;
  3. min_new_tokens m: while t - s_b < m (the row has generated fewer than m tokens), z[v] = -inf for every v in the
     call's stop_ids.
  4. The contracts of llm/sampling.py (temperature 0: the first maximum) and llm/logprobs.py run unchanged on the edited
     row: the log-probability of a banned token is -inf.
The defaults (None, None, 0) are "off": `check_args` returns None for them and every caller keeps its plain path.
"""
import math
from collections.abc import Mapping

import numpy as np

MAX_BIAS = 1024          # bias entries per request: the kernel keeps a row's table in LDS (PDNE_MAX_BIAS)

_INT = (int, np.integer)
_REAL = (int, float, np.integer, np.floating)


def _ids(what, ids, V):
    """Token ids as a sorted int64 array without repeats; ValueError for a non-integer or one outside [0, V)."""
    if isinstance(ids, np.ndarray):
        if ids.dtype.kind not in "iu":
            raise ValueError(f"{what}: token ids must be integers, got dtype {ids.dtype}")
        out = ids.reshape(-1).astype(np.int64)
    else:
        ids = list(ids)
        for t in ids:
            if isinstance(t, (bool, np.bool_)) or not isinstance(t, _INT):
                raise ValueError(f"{what}: token ids must be integers, got {t!r}")
        out = np.array([int(t) for t in ids], np.int64).reshape(-1)
    if out.size and (out.min() < 0 or out.max() >= V):
        raise ValueError(f"{what}: token ids must lie in [0, {V})")
    return np.unique(out)


def _bias(what, bias, V):
    """One request's logit_bias {id: beta} as (ids int32 sorted, values float32), checked."""
    if not isinstance(bias, Mapping):
        raise ValueError(f"{what} must be a mapping of token id to bias, got {type(bias).__name__}")
    if len(bias) > MAX_BIAS:
        raise ValueError(f"{what}: {len(bias)} entries, at most MAX_BIAS = {MAX_BIAS} per request")
    keys = list(bias)
    for t in keys:
        if isinstance(t, (bool, np.bool_)) or not isinstance(t, _INT):
            raise ValueError(f"{what}: token ids must be integers, got {t!r}")
    ids = np.array([int(t) for t in keys], np.int64)
    if ids.size and (ids.min() < 0 or ids.max() >= V):
        raise ValueError(f"{what}: token ids must lie in [0, {V})")
    if np.unique(ids).size != ids.size:
        raise ValueError(f"{what}: a token id appears twice")
    vals = np.zeros(ids.size, np.float32)
    for j, t in enumerate(keys):
        v = bias[t]
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, _REAL):
            raise ValueError(f"{what}[{t}] must be a real number, got {v!r}")
        v = float(v)
        with np.errstate(over="ignore"):
            v32 = np.float32(v)
        if math.isnan(v) or v == math.inf or (v != -math.inf and not np.isfinite(v32)):
            raise ValueError(f"{what}[{t}] must be finite in float32, or -inf (a ban), got {v}")
        vals[j] = v32
    order = np.argsort(ids, kind="stable")
    return ids[order].astype(np.int32), vals[order]


def _per_request(name, value, n, single):
    """`value` as a list of n entries: one value for the whole call (`single(value)` is true) or one per request."""
    if value is None:
        return [None] * n
    if single(value):
        return [value] * n
    if isinstance(value, (str, bytes)) or not hasattr(value, "__len__"):
        raise ValueError(f"{name} must be one value or a sequence with one per request, got {value!r}")
    if len(value) != n:
        raise ValueError(f"{name}: {len(value)} entries for {n} requests")
    return list(value)


def _one_allowed(value):
    """An allowed set for the whole call: a flat collection of ids (empty included), not a sequence of sets / Nones."""
    if isinstance(value, np.ndarray):
        return value.ndim == 1 and value.dtype != object
    if isinstance(value, (set, frozenset, range)):
        return True
    if isinstance(value, (list, tuple)):
        return all(e is not None and np.ndim(e) == 0 and not isinstance(e, (set, frozenset)) for e in value)
    return False


class Edits:
    """The checked arguments of a call: `reqs[r]` = (allowed ids int64 sorted or None, bias ids int32 sorted, bias values
    float32) of request r, `m` = min_new_tokens, `stops` the call's stop ids (int64), `V` the vocabulary size."""

    def __init__(self, V, reqs, m, stops):
        self.V, self.reqs, self.m, self.stops = V, reqs, m, stops

    def allow_rows(self, reqs):
        return [self.reqs[int(r)][0] for r in reqs]

    def bias_rows(self, reqs):
        return [self.reqs[int(r)][1:] for r in reqs]

    def packed(self, reqs):
        """The device forms of requests `reqs`: (bits, on, ids, values, counts); bits / the table None when none has one."""
        allow, bias = self.allow_rows(reqs), self.bias_rows(reqs)
        bits, on = allow_bits(allow, self.V) if any(a is not None for a in allow) else (None, None)
        ids, vals, cnt = bias_tables(bias) if any(b[0].size for b in bias) else (None, None, None)
        return bits, on, ids, vals, cnt


def check_args(logit_bias=None, allowed_token_ids=None, min_new_tokens=0, V=0, n=1, stop_ids=(), speculate=0,
               stop_sequences=False):
    """Validate the edit arguments of a call with `n` prompts / requests over a vocabulary of `V` tokens; returns an `Edits`,
    or None when nothing is to be edited (all three at their defaults).  `stop_sequences`: the call has stop sequences
    (llm/stop_sequences.py) -- min_new_tokens then needs no stop id, and without one it edits nothing (the sequences are
    held back by their own matcher, no logit is touched for them).  ValueError: see the tests."""
    m = min_new_tokens
    if isinstance(m, (bool, np.bool_)) or not isinstance(m, _INT) or m < 0:
        raise ValueError(f"min_new_tokens must be a non-negative integer, got {m!r}")
    m = int(m)
    stops = np.unique(np.asarray(list(stop_ids), np.int64).reshape(-1))
    if m > 0 and not stops.size:
        if not stop_sequences:
            raise ValueError("min_new_tokens > 0 needs stop_ids (it keeps a request from stopping)")
        m = 0                                    # (no stop id to mask)
    biases = _per_request("logit_bias", logit_bias, n, lambda v: isinstance(v, Mapping))
    allows = _per_request("allowed_token_ids", allowed_token_ids, n, _one_allowed)
    reqs = []
    for r, (bias, allow) in enumerate(zip(biases, allows)):
        a = None
        if allow is not None:
            if isinstance(allow, (str, bytes, Mapping)) or not hasattr(allow, "__iter__"):
                raise ValueError(f"allowed_token_ids of request {r} must be a collection of token ids, got {allow!r}")
            a = _ids(f"allowed_token_ids of request {r}", allow, V)
            if not a.size:
                raise ValueError(f"allowed_token_ids of request {r} is empty")
        ids, vals = (np.zeros(0, np.int32), np.zeros(0, np.float32)) if bias is None else \
            _bias(f"logit_bias of request {r}", bias, V)
        gone = ids[np.isneginf(vals)].astype(np.int64)
        if m > 0:
            gone = np.union1d(gone, stops)
        left = (V if a is None else a.size) - (gone.size if a is None else np.intersect1d(a, gone).size)
        if left <= 0:
            raise ValueError(f"request {r}: its allowed tokens minus its banned tokens"
                             f"{' minus the stop ids (min_new_tokens > 0)' if m > 0 else ''} leave no token to pick")
        reqs.append((a, ids, vals))
    if m == 0 and all(a is None and not ids.size for a, ids, _ in reqs):
        return None
    if speculate:
        raise ValueError("logit_bias / allowed_token_ids / min_new_tokens cannot be combined with speculate > 0 "
                         "(draft positions would need their own edits)")
    return Edits(int(V), reqs, m, stops)


def apply(z, allow_rows=None, bias=None, generated=None, m=0, stop_ids=()):
    """The statement on arrays: z (B, V) float32 logits; allow_rows[b] = the ids row b may produce, or None; bias[b] =
    (ids, float32 values) or a mapping or None; generated[b] = t - s_b, the tokens row b has produced so far (None: 0);
    m = min_new_tokens with the call's stop_ids.  Returns the edited float32 rows (a new array)."""
    z = np.array(z, np.float32)
    B, V = z.shape
    stops = np.asarray(list(stop_ids), np.int64).reshape(-1)
    ninf = np.float32(-np.inf)
    for b in range(B):
        if allow_rows is not None and allow_rows[b] is not None:
            out = np.ones(V, bool)
            out[np.asarray(allow_rows[b], np.int64).reshape(-1)] = False
            z[b, out] = ninf
        if bias is not None and bias[b] is not None:
            e = bias[b]
            ids, vals = (list(e.keys()), list(e.values())) if isinstance(e, Mapping) else e
            ids, vals = np.asarray(ids, np.int64).reshape(-1), np.asarray(vals, np.float32).reshape(-1)
            with np.errstate(invalid="ignore", over="ignore"):
                z[b, ids] = np.where(np.isneginf(vals), ninf, z[b, ids] + vals)
        if m > 0 and stops.size and (0 if generated is None else int(generated[b])) < m:
            z[b, stops] = ninf
    return z


def allow_bits(allow_rows, V):
    """The allowed sets as the kernels keep them: ((R, ceil(V / 32)) int32 with bit v & 31 of word v >> 5 set for v in A_b,
    (R,) int32 on / off); a row without a set is off and its bits are zero."""
    bits = np.zeros((len(allow_rows), -(-V // 32)), np.uint32)
    on = np.zeros(len(allow_rows), np.int32)
    for b, a in enumerate(allow_rows):
        if a is None:
            continue
        a = np.unique(np.asarray(a, np.int64).reshape(-1))
        np.bitwise_or.at(bits[b], a >> 5, np.uint32(1) << (a & 31).astype(np.uint32))
        on[b] = 1
    return bits.view(np.int32), on


def bits_allow(bits, on, V):
    """`allow_bits` back: a list of sorted int64 id arrays, None for a row that is off."""
    w = np.asarray(bits).view(np.uint32)
    rows = ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(w.shape[0], -1)[:, :V].astype(bool)
    return [np.flatnonzero(r).astype(np.int64) if o else None for r, o in zip(rows, on)]


def bias_tables(bias):
    """The bias tables as the kernels keep them: ids (R, MAX_BIAS) int32 sorted by id, values (R, MAX_BIAS) float32, counts
    (R,) int32; bias[b] = (ids, values) or None."""
    ids = np.zeros((len(bias), MAX_BIAS), np.int32)
    vals = np.zeros((len(bias), MAX_BIAS), np.float32)
    cnt = np.zeros(len(bias), np.int32)
    for b, e in enumerate(bias):
        if e is None:
            continue
        i, v = np.asarray(e[0], np.int64).reshape(-1), np.asarray(e[1], np.float32).reshape(-1)
        if i.size > MAX_BIAS:
            raise ValueError(f"{i.size} bias entries, at most MAX_BIAS = {MAX_BIAS}")
        order = np.argsort(i, kind="stable")
        ids[b, :i.size], vals[b, :i.size], cnt[b] = i[order], v[order], i.size
    return ids, vals, cnt


def tables_bias(ids, vals, cnt):
    """`bias_tables` back: a list of (ids int32, values float32)."""
    return [(np.array(i[:c], np.int32), np.array(v[:c], np.float32)) for i, v, c in zip(ids, vals, cnt)]


def params_bytes(m):
    """pdne_logit_edit_params (include/pdn_logitedit.h) as two int64 words: {int min_new_tokens; int reserved[3]}."""
    return np.array([m, 0, 0, 0], np.int32).view(np.int64)


class Rows:
    """The per-row state of the statement on the host (every path without the device state of csrc/logit_edit.hip): the
    request each row holds (-1: none) and the position of its first generated token (its prompt length)."""

    def __init__(self, B, spec, reqs=None, start=None):
        self.spec = spec
        self.req = np.full(B, -1, np.int64)
        self.start = np.zeros(B, np.int64)
        if reqs is not None:                     # (generate / generate_ragged: row b holds request b from the start)
            self.reset(np.arange(B), reqs, start)

    def reset(self, rows, reqs, start):
        """Rows `rows` take requests `reqs` with prompt lengths `start`."""
        rows = np.asarray(rows, np.int64).reshape(-1)
        self.req[rows] = np.asarray(reqs, np.int64).reshape(-1)
        self.start[rows] = np.asarray(start, np.int64).reshape(-1)

    def apply(self, z, pos, rows=None):
        """The edited (len(rows), V) float32 logits of rows `rows` (default: all) at positions pos (one per listed row; a row
        at -1, or without a request, is left as it is)."""
        rows = np.arange(self.req.size) if rows is None else np.asarray(rows, np.int64).reshape(-1)
        pos = np.broadcast_to(np.asarray(pos, np.int64).reshape(-1), rows.shape)
        z = np.array(z, np.float32)
        live = np.flatnonzero((pos >= 0) & (self.req[rows] >= 0))
        if live.size:
            r = self.req[rows[live]]
            z[live] = apply(z[live], self.spec.allow_rows(r), self.spec.bias_rows(r), pos[live] - self.start[rows[live]],
                            self.spec.m, self.spec.stops)
        return z
