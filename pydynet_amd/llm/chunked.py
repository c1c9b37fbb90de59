"""The schedule of chunked prefill, `Llama.serve(..., prefill_chunk=C)`, stated in NumPy.  Every path of `serve` with a
chunk follows this one statement; only how a step's tokens are computed differs between them.

Per step:
  1. `admit`: the free rows take waiting requests exactly as in `serve` -- the lowest free row takes the lowest waiting
     request (a request with a budget of 0 never waits).  An admitted row starts prefilling from position 0.
  2. `feed`: at most C prompt tokens in total go to the rows still prefilling, in ascending request id (= admission
     order); each request's prompt is fed in order.  A row gets n[b] tokens at positions fed[b] .. fed[b] + n[b] - 1.
  3. The rows that decode (their prompt was complete before the step) yield one token each; a row whose last prompt
     token is fed in this step yields its first token (Philox counter (len, req) when sampled); a row still mid-prompt
     yields -1.
  4. `finish`: every row that yielded a token moves one position on and has one token less to go; a request ends at its
     budget, at a stop id or at the end of a stop sequence (llm/stop_sequences.py), and its row is free for the next
     step's admission.
With C at least the number of prompt tokens admitted at every step, every admitted prompt completes in its admission
step, and the steps are exactly those of `serve`."""
import numpy as np


def check_chunk(prefill_chunk, slots, max_rows=256):
    """The chunk argument of `serve`: None, or an integer C >= 1 with slots + C <= max_rows (the mixed step's query rows).
    Raises ValueError otherwise."""
    if prefill_chunk is None:
        return None
    C = prefill_chunk
    if isinstance(C, (bool, np.bool_)) or not isinstance(C, (int, np.integer)) or C < 1:
        raise ValueError(f"prefill_chunk must be an integer >= 1 or None, got {C!r}")
    if int(slots) + int(C) > max_rows:
        raise ValueError(f"slots + prefill_chunk = {int(slots) + int(C)} exceeds {max_rows} query rows")
    return int(C)


def feed(req, lens, fed, C):
    """Step 2 alone: n (S,) int64, the prompt tokens fed to each row.  req: (S,) request per row (-1: free); lens: (S,)
    prompt length of the row's request; fed: (S,) prompt tokens fed so far (== lens once the row decodes)."""
    req, lens, fed = (np.asarray(a, np.int64) for a in (req, lens, fed))
    n = np.zeros(req.shape, np.int64)
    left = int(C)
    for b in sorted(np.flatnonzero((req >= 0) & (fed < lens)).tolist(), key=lambda b: int(req[b])):
        if left <= 0:
            break
        n[b] = min(left, int(lens[b] - fed[b]))
        left -= int(n[b])
    return n


class Schedule:
    """The rows' state of a chunked `serve` run on the host.  Per row b: req[b] (-1: free), fed[b] (prompt tokens fed),
    pos[b] (the position of the row's next decode step; -1 while free or prefilling), left[b] (tokens it may still
    yield) and last[b] (its last token)."""

    def __init__(self, lens, budgets, S, C):
        self.lens = np.asarray(lens, np.int64)
        self.budgets = np.asarray(budgets, np.int64)
        self.S, self.C = int(S), int(C)
        self.queue = [r for r in range(len(self.lens)) if self.budgets[r] > 0]
        self.q = 0
        self.req = np.full(S, -1, np.int64)
        self.fed = np.zeros(S, np.int64)
        self.pos = np.full(S, -1, np.int64)
        self.left = np.zeros(S, np.int64)
        self.last = np.zeros(S, np.int64)

    def row_lens(self):
        return np.where(self.req >= 0, self.lens[np.maximum(self.req, 0)], 0)

    def admit(self):
        """Step 1: the rows admitted now and their requests, ((A,), (A,)) int64."""
        rows = np.flatnonzero(self.req < 0)[:len(self.queue) - self.q]
        new = np.array(self.queue[self.q:self.q + rows.size], np.int64)
        self.q += rows.size
        self.req[rows], self.fed[rows], self.pos[rows], self.left[rows] = new, 0, -1, self.budgets[new]
        return rows, new

    def busy(self):
        return bool((self.req >= 0).any())

    def plan(self):
        """Step 2 and who yields: (n, decode, complete) -- tokens fed per row, the rows that decode, the rows whose prompt
        completes in this step."""
        lens = self.row_lens()
        n = feed(self.req, lens, self.fed, self.C)
        decode = (self.req >= 0) & (self.fed >= lens)
        complete = (n > 0) & (self.fed + n == lens)
        return n, decode, complete

    def finish(self, n, toks, stops=(), stopped=None):
        """Step 4, after the step's tokens `toks` (S,) (-1 where a row yielded none): returns the requests shown for the
        step, (S,) int64 (the request in each row during the step).  `stopped` (S,) bool: the rows whose token ends a stop
        sequence; they end as at a stop id."""
        lens = self.row_lens()
        shown = self.req.copy()
        done_prompt = (n > 0) & (self.fed + n == lens)
        self.fed += n
        self.pos[done_prompt] = lens[done_prompt]
        has = (shown >= 0) & (toks >= 0)
        self.left[has] -= 1
        self.pos[has] += 1
        self.last[has] = toks[has]
        done = has & ((self.left <= 0) | np.isin(toks, np.asarray(stops, np.int64)))
        if stopped is not None:
            done |= has & np.asarray(stopped, bool)
        self.req[done], self.pos[done], self.left[done], self.fed[done] = -1, -1, 0, 0
        return shown
