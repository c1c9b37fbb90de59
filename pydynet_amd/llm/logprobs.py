"""Token log-probabilities for `Llama.generate` / `generate_ragged` / `serve` / `serve_all` (`logprobs=n`) and
`Llama.score`.  This module states the contract in NumPy; the `cpu` device and the tests run it, and on a HIP device the
same values come from csrc/logprobs.hip (the standalone rows entry on prompt passes, generic steps and `score`, the tick
form inside the graph-replayed decode step).

Per step and row:
  * z is the logit row that the step's pick or draw reads: after the penalties of llm/penalties.py when they are on,
    before temperature, top-k and top-p.  With penalties off the values are the model's own distribution whatever the
    sampling settings.
  * logp = beam.log_softmax_rows(z): float32(z - lse), the log-sum-exp in float64.
  * `token`: logp of the token the step yielded.
  * `top_ids` / `top_logprobs`: the n best tokens by logp descending, ties to the lower id (-inf entries rank last).
  * a row that yields no token at that step (a stopped ragged row, an empty or still-prefilling `serve` slot, a row
    past its budget) has token = nan, top_ids = -1 and top_logprobs = nan.
n is an int in [0, MAX_N]; n = 0 returns `token` only (top arrays of width 0)."""
from collections import namedtuple

import numpy as np

from .beam import log_softmax_rows

MAX_N = 20                                      # OpenAI's cap on top_logprobs
UNSET = np.iinfo(np.int64).min                  # a record word the device has not written yet

Logprobs = namedtuple("Logprobs", ["token", "top_ids", "top_logprobs"])


def check_n(n, allow_none=True):
    """None (off, when allowed) or an int in [0, MAX_N]; anything else raises ValueError."""
    if n is None and allow_none:
        return None
    if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)):
        raise ValueError(f"logprobs must be None or an int in [0, {MAX_N}], got {n!r}")
    if not 0 <= int(n) <= MAX_N:
        raise ValueError(f"logprobs must lie in [0, {MAX_N}], got {n}")
    return int(n)


def rows(z, tokens, n):
    """The statement on logit rows z (R, V) and the tokens (R,) each row yielded (< 0: none).  Returns Logprobs with
    token (R,) float32, top_ids (R, n) int64, top_logprobs (R, n) float32."""
    z = np.asarray(z, np.float32)
    R, V = z.shape
    tokens = np.asarray(tokens, np.int64).reshape(R)
    tok = np.full(R, np.nan, np.float32)
    ids = np.full((R, n), -1, np.int64)
    top = np.full((R, n), np.nan, np.float32)
    live = np.flatnonzero(tokens >= 0)
    if live.size:
        lp = log_softmax_rows(z[live])
        tok[live] = lp[np.arange(live.size), tokens[live]]
        if n:
            for j, r in enumerate(live):
                order = np.lexsort((np.arange(V), -lp[j].astype(np.float64)))[:n]
                ids[r, :order.size] = order
                top[r, :order.size] = lp[j, order]
    return Logprobs(tok, ids, top)


def none(R, n):
    """Logprobs of R rows that yield nothing."""
    return Logprobs(np.full(R, np.nan, np.float32), np.full((R, n), -1, np.int64), np.full((R, n), np.nan, np.float32))


def merge(into, rows_, part):
    """Rows `rows_` of `into` (Logprobs, arrays written in place) take the values of `part` (Logprobs of len(rows_))."""
    rows_ = np.asarray(rows_, np.int64)
    into.token[rows_] = part.token
    into.top_ids[rows_] = part.top_ids
    into.top_logprobs[rows_] = part.top_logprobs
    return into


def record_words(n):
    """int64 words of one row's record of the tick form: the token's logp, n ids, n logps (float bits zero-extended)."""
    return 1 + 2 * n


def to_records(lp):
    """Logprobs (R rows) -> (R, 1 + 2n) int64 records, as the tick form writes them."""
    n = lp.top_ids.shape[1]
    rec = np.empty((lp.token.shape[0], record_words(n)), np.int64)
    rec[:, 0] = np.asarray(lp.token, np.float32).view(np.uint32)
    rec[:, 1:1 + n] = lp.top_ids
    rec[:, 1 + n:] = np.asarray(lp.top_logprobs, np.float32).view(np.uint32)
    return rec


def from_records(rec, n):
    """(R, 1 + 2n) int64 records -> Logprobs."""
    rec = np.asarray(rec, np.int64)
    bits = lambda a: np.ascontiguousarray(a).astype(np.uint32).view(np.float32)     # noqa: E731
    return Logprobs(bits(rec[:, 0]), rec[:, 1:1 + n].copy(), bits(rec[:, 1 + n:1 + 2 * n]).reshape(rec.shape[0], n))


def as_step(lp):
    """Logprobs of a decode step as `generate` yields them: token (B, 1), top arrays (B, n)."""
    return Logprobs(np.asarray(lp.token, np.float32).reshape(-1, 1), np.asarray(lp.top_ids, np.int64),
                    np.asarray(lp.top_logprobs, np.float32))
