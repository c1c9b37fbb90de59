"""Prompt-lookup speculative decoding, `Llama.generate_ragged(..., speculate=k)`, stated in NumPy.  Every path of a
speculative generation follows this one statement; only how a pass's picks are computed differs between them.

Per target pass, for every row b still live:
  1. `draft`: the row's history h (prompt + every token yielded so far, T tokens) proposes up to k tokens by n-gram
     lookup.  For n = NGRAM down to 1 the key is h[T-n:T]; the largest j with j + n < T and h[j:j+n] == key gives the
     draft h[j+n : min(j+n+k, T)], and the search stops at the first n that matches (no match: an empty draft).  The
     draft is capped at left - 1 tokens, `left` being what the row may still yield, so a pass never feeds a position
     past the row's last decode step (which `generate_ragged` has checked against the KV cache and RoPE table).
  2. The pass feeds t_0 = h[T-1] and the draft t_1 .. t_d at consecutive cache positions from pos, the position at
     which the plain step would feed t_0 (the first decode step of a row of length len feeds at len + 1 and slot len is
     never written: the reference's quirk, kept).  Query j yields p_j: the greedy pick, or the draw with Philox counter
     (pos + j, b) -- exactly the token the plain step at position pos + j would produce from the same prefix.
  3. `accept`: a = the number of leading j < d with p_j == t_{j+1}.  The row yields p_0 .. p_a, cut after the first
     stop id, and moves a + 1 positions on (fewer if it stopped); `left` drops by the count yielded.
Every accepted draft token is the token the plain step would have yielded from the same logits, so where the picks are
computed by the plain step's own operators (the `cpu` statement path) the yielded streams are exactly those of
`speculate=0`; the graph-replayed HIP pass computes its logits with other kernels and agrees up to fp32 near-ties.
The cache slots past a row's new position may hold K/V of rejected drafts: within the run they are never read before
they are overwritten, because each pass appends its K/V before its attention reads the cache, and a pass reads only
slots up to the positions it has just written.  A row that stops (stop id or budget) leaves the K/V of the drafts
rejected in its last pass behind in slots the plain decode never writes; a later call that reads such a slot without
writing it first (the slot `len` of the first-decode-step quirk) sees them, where after `speculate=0` it would see
whatever the slot held before.  The cache contents left behind past a row's last position therefore differ from those
of `speculate=0` -- the same kind of dependence on earlier calls that slot `len` already has."""
import numpy as np

NGRAM = 3
MAX_SPECULATE = 16


def check_speculate(speculate, rows, max_rows=256):
    """The speculate argument of `generate_ragged`: an integer k in 0 .. MAX_SPECULATE with rows * (k + 1) <= max_rows
    (the query rows of one pass).  Raises ValueError otherwise."""
    k = speculate
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 0 <= k <= MAX_SPECULATE:
        raise ValueError(f"speculate must be an integer in 0..{MAX_SPECULATE}, got {k!r}")
    if int(rows) * (int(k) + 1) > max_rows:
        raise ValueError(f"prompts * (speculate + 1) = {int(rows) * (int(k) + 1)} exceeds {max_rows} query rows")
    return int(k)


def draft(h, k, left):
    """Step 1 for one row: the draft tokens, (d,) int64, from history h (T,), at most k tokens and at most left - 1."""
    h = np.asarray(h, np.int64).reshape(-1)
    T, cap = h.size, min(int(k), int(left) - 1)
    if cap <= 0:
        return np.zeros(0, np.int64)
    for n in range(NGRAM, 0, -1):
        key = h[T - n:T] if T >= n else None
        if key is None:
            continue
        for j in range(T - n - 1, -1, -1):                  # (the largest j with j + n < T first)
            if np.array_equal(h[j:j + n], key):
                return h[j + n:min(j + n + cap, T)].copy()
    return np.zeros(0, np.int64)


def accept(fed, picks, left, stops=()):
    """Steps 2-3 for one row: fed = [t_0, t_1 .. t_d], picks = [p_0 .. p_d].  Returns (yielded (c,) int64, a, stopped):
    the tokens the row yields, the number of drafts the picks agree with, and whether it yielded a stop id."""
    fed, picks = np.asarray(fed, np.int64).reshape(-1), np.asarray(picks, np.int64).reshape(-1)
    d = fed.size - 1
    a = 0
    while a < d and picks[a] == fed[a + 1]:
        a += 1
    out = picks[:min(a + 1, int(left))]
    hit = np.flatnonzero(np.isin(out, np.asarray(stops, np.int64)))
    if hit.size:
        return out[:hit[0] + 1].copy(), a, True
    return out.copy(), a, False


def counts():
    """The `Llama.last_speculation` dict of a run before its first pass."""
    return {"passes": 0, "drafted": 0, "accepted": 0, "tokens": 0}


class Rows:
    """The rows' state of a speculative run on the host: per row its history, the position its next pass feeds t_0 at
    (-1: stopped), and `left`; `out[b]` holds what the row has yielded (the prompt pass's token first)."""

    def __init__(self, rows, first, n, stops=()):
        self.stops = np.asarray(stops, np.int64)
        B = len(rows)
        self.hist = [np.concatenate([np.asarray(r, np.int64).reshape(-1), [int(t)]]) for r, t in zip(rows, first)]
        self.out = [[int(t)] for t in first]
        self.lens = np.array([np.asarray(r).size for r in rows], np.int64)
        self.left = np.full(B, int(n) - 1, np.int64)
        self.pos = self.lens + 1
        for b, t in enumerate(first):
            if self.left[b] <= 0 or np.isin(int(t), self.stops):
                self.pos[b], self.left[b] = -1, 0
        self.stats = counts()

    def live(self):
        return self.pos >= 0

    def plan(self, k):
        """The fed tokens of every row, [t_0, drafts...] (an empty list for a stopped row)."""
        return [[int(h[-1])] + draft(h, k, l).tolist() if p >= 0 else []
                for h, l, p in zip(self.hist, self.left, self.pos)]

    def finish(self, fed, picks):
        """Step 3 for every row, with each row's picks (a list per row, like `fed`)."""
        self.stats["passes"] += 1
        for b, (f, p) in enumerate(zip(fed, picks)):
            if not f:
                continue
            y, a, hit = accept(f, p, self.left[b], self.stops)
            self.take(b, y, len(f) - 1, min(a, y.size), hit)

    def take(self, b, y, d, acc, hit):
        """Row b yields y after a pass that fed it d drafts of which acc are yielded."""
        self.stats["drafted"] += int(d)
        self.stats["accepted"] += int(acc)
        self.stats["tokens"] += int(len(y))
        self.out[b] += [int(t) for t in y]
        self.hist[b] = np.concatenate([self.hist[b], np.asarray(y, np.int64)])
        self.left[b] -= len(y)
        self.pos[b] += len(y)
        if hit or self.left[b] <= 0:
            self.pos[b], self.left[b] = -1, 0

    def ready(self):
        """The number of steps every row can show: min over the live rows of their yielded count (a stopped row shows
        -1 from then on, so it never holds a step back)."""
        live = self.live()
        return min(len(o) for o, l in zip(self.out, live) if l) if live.any() else max(len(o) for o in self.out)

    def step(self, i):
        """Step i of the yield contract, (B, 1) int64: row b's token i, -1 once the row has stopped."""
        return np.array([o[i] if i < len(o) else -1 for o in self.out], np.int64).reshape(-1, 1)
