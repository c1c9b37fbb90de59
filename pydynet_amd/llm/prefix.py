"""Prefix caching, `Llama.serve(..., prefill_chunk=C, prefix_cache=k)`, stated in NumPy: which prompt tokens of an admitted
request are not fed because a cache row already holds their keys / values.  It stands beside llm/chunked.py, whose
schedule it extends; every path of `serve` with the cache on follows this one statement.

The cache rows themselves are the store.  Row b's cache positions [0, len) hold the prompt keys / values of the row's
request and nothing rewrites them while the request decodes (decode steps write past len), so they survive until the row's
next admission.  The record of row b is `held[b]`, the prompt of the last request admitted to the row, and `valid[b]`, how
many of its leading tokens have their keys / values in the row: the prompt tokens fed or copied so far, len once the
prompt completed, 0 for a row never used.  Generated tokens are not part of the record: a decode step feeds the token of
position p - 1 at position p, so the keys past the prompt are not those a prompt pass over the same tokens would write.

A request with prompt p, admitted to row d, against the records AS THEY WERE BEFORE THIS STEP'S ADMISSIONS:
  m[b] = the length of the common prefix of p and held[b][:valid[b]];
  n    = min(max_b m[b], len(p) - 1): the last prompt token is always fed, its logits make the first token;
  n < k: no reuse (n = 0, the whole prompt is fed);
  donor: row d itself if m[d] >= n (no copy: the data is there), else the lowest row b with m[b] >= n;
  the row starts with fed = n; its record becomes held = p, valid = n, and valid follows fed as the prompt is fed.
A live row (prefilling or decoding) is a legal donor for its `valid` leading positions: it only ever writes at positions
>= valid.  Rows admitted in the same step see each other's OLD records only (two of them may take from each other: the copy
reads every source as it was before the launch), so a cold start with eight identical system prompts computes eight prompts
and the second wave hits.  Reused tokens do not count against the chunk budget C: nothing is fed for them."""
import numpy as np

from . import chunked

STATS = ("requests", "hits", "prompt_tokens", "reused_tokens", "copies", "launches")


def check_arg(prefix_cache, prefill_chunk):
    """The cache argument of `serve`: None (off: False / None), or the least number of tokens worth reusing, an integer
    k >= 1 (True = 1).  The cache needs a chunk.  Raises ValueError otherwise."""
    k = prefix_cache
    if k is None or (isinstance(k, (bool, np.bool_)) and not k):
        return None
    if isinstance(k, (bool, np.bool_)):
        k = 1
    elif not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError(f"prefix_cache must be a bool, None or an integer >= 1, got {prefix_cache!r}")
    if prefill_chunk is None:
        raise ValueError("prefix_cache needs prefill_chunk: without a chunk every prompt pass starts at position 0")
    return int(k)


def common(a, b):
    """The length of the common prefix of two token sequences."""
    a, b = np.asarray(a, np.int64).reshape(-1), np.asarray(b, np.int64).reshape(-1)
    n = min(a.size, b.size)
    diff = np.flatnonzero(a[:n] != b[:n])
    return int(diff[0]) if diff.size else n


def match(p, d, held, valid, k=1):
    """(donor, n) for prompt `p` admitted to row `d` against the records `held` (one token array per row, None: never
    used) and `valid` (S,): n tokens reused from row `donor` (donor == d: already in place); (d, 0) without reuse."""
    p0 = int(p[0])                                                    # (most rows differ in the first token already)
    m = np.array([0 if h is None or v <= 0 or int(h[0]) != p0 else common(p, np.asarray(h)[:int(v)])
                  for h, v in zip(held, valid)], np.int64)
    n = min(int(m.max()) if m.size else 0, len(p) - 1)
    if n < max(int(k), 1):
        return int(d), 0
    return (int(d) if m[d] >= n else int(np.flatnonzero(m >= n)[0])), n


class Schedule(chunked.Schedule):
    """chunked.Schedule with the rows' records: `admit()` gives, per admitted row, its donor and the tokens it reuses, and
    the row starts with fed = n.  `k` None: reuse forced to 0 (the paths that complete a prompt with one whole pass from
    position 0) -- the schedule is then chunked.Schedule's, step for step.  `stats`: the run's figures so far (STATS;
    `launches` is counted by whoever issues the copies, one per step that has one)."""

    def __init__(self, prompts, budgets, S, C, k=1):
        super().__init__([len(p) for p in prompts], budgets, S, C)
        self.prompts = [np.asarray(p, np.int64).reshape(-1) for p in prompts]
        self.k = None if k is None else int(k)
        self.held = [None] * self.S
        self._valid = np.zeros(self.S, np.int64)                      # (of the rows that are free; a live row's is `fed`)
        self.stats = dict.fromkeys(STATS, 0)

    @property
    def valid(self):
        return np.where(self.req >= 0, self.fed, self._valid)

    def admit(self):
        """Step 1: (rows, requests, donors, n), each (A,) int64."""
        valid = self.valid                                            # (the records before this step's admissions)
        rows, new = super().admit()
        if not rows.size:
            return rows, new, rows, rows
        donors, n = rows.copy(), np.zeros(rows.size, np.int64)
        if self.k is not None:
            for i, (d, r) in enumerate(zip(rows.tolist(), new.tolist())):
                donors[i], n[i] = match(self.prompts[r], d, self.held, valid, self.k)
        for d, r in zip(rows.tolist(), new.tolist()):
            self.held[d] = self.prompts[r]
        self.fed[rows] = n
        st = self.stats
        st["requests"] += int(rows.size)
        st["hits"] += int((n > 0).sum())
        st["prompt_tokens"] += int(sum(self.prompts[r].size for r in new.tolist()))
        st["reused_tokens"] += int(n.sum())
        st["copies"] += int(((n > 0) & (donors != rows)).sum())
        return rows, new, donors, n

    def finish(self, n, toks, stops=(), stopped=None):
        shown = super().finish(n, toks, stops, stopped)
        freed = shown != self.req                                     # (a row ends only after its whole prompt was fed)
        if freed.any():
            self._valid[freed] = self.lens[shown[freed]]
        return shown
