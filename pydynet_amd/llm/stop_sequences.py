"""Multi-token stop sequences for `Llama.generate_ragged`, `serve` and `serve_all`: `stop_sequences`.

This module states the contract in NumPy; on a HIP device the graph-replayed steps run it through csrc/stop_seq.hip
(include/pdn_stopseq.h), which stops the same rows at the same steps.

The argument.  `stop_sequences` is
  * None or an empty sequence: off -- `check_args` returns None and every caller keeps its plain path;
  * a sequence of token-id sequences, e.g. [[13, 13], [2277, 29937]]: these sequences for every request;
  * a sequence with one entry per prompt / request, each None or a sequence of token-id sequences: per request.
The two forms are told apart by depth: elements that are sequences of integers give the shared form, elements that are
None or sequences of sequences the per-request form (its length must equal the number of prompts); a mixture raises.
Limits (ValueError before anything runs): ids are integers in [0, V), bools refused; a sequence holds 1 .. MAX_LEN tokens;
a request has at most MAX_SEQS distinct sequences (duplicates collapse); a call at most MAX_CALL_SEQS sequences over all
requests (requests with equal sets share one); not with speculate > 0.

The meaning.
  1. Let y_1, y_2, ... be the tokens a request generates; y_1 is the token that comes out of the prompt pass.
  2. A sequence q of length l matches at g when g >= l and y_{g-l+1} .. y_g == q.
  3. Prompt tokens never take part: a sequence that straddles the end of the prompt does not match.
  4. The request stops at the smallest g at which any of its sequences matches: y_g is yielded as a stop id is, from the
     next step on the row yields -1, its position stops advancing and its cache is no longer written; in `serve` its slot
     is free for the next admission.
  5. `stop_ids` and the budget act as before; whichever stops the row first wins.
  6. min_new_tokens = m > 0: a match ending at g counts only when g > m -- the g at which a stop id can first be yielded
     (llm/logit_edits.py masks a stop id while fewer than m tokens were generated before it), so a sequence of length 1
     and a stop id agree on the step.  Earlier matches are ignored, not banned: no logit is touched by this feature.
  7. `serve_all` cuts a request's tokens at the end of its first matching sequence, the matching tokens included.
No logit, no draw and no Philox counter changes: a request's output with `stop_sequences` is its output without them,
truncated at the match (`truncate`).
"""
import numpy as np

MAX_LEN = 16             # tokens of one sequence: a row's tail ring (PDNH_MAX_LEN of csrc/stop_seq.hip)
MAX_SEQS = 16            # distinct sequences of one request: one lane each
MAX_CALL_SEQS = 4096     # sequences of one call over all its requests

_INT = (int, np.integer)


def _is_seq(x):
    return not isinstance(x, (str, bytes, dict, set, frozenset)) and hasattr(x, "__len__") and hasattr(x, "__iter__")


def _is_id(x):
    return isinstance(x, (bool, np.bool_) + _INT) or (isinstance(x, np.ndarray) and x.ndim == 0)


def _one_set(what, seqs, V):
    """One request's sequences as a sorted tuple of distinct int tuples, checked."""
    out = set()
    for q in seqs:
        if not _is_seq(q):
            raise ValueError(f"{what}: a stop sequence must be a sequence of token ids, got {q!r}")
        q = list(q)
        for t in q:
            if isinstance(t, (bool, np.bool_)) or not isinstance(t, _INT):
                raise ValueError(f"{what}: token ids must be integers, got {t!r}")
            if not 0 <= int(t) < V:
                raise ValueError(f"{what}: token ids must lie in [0, {V}), got {int(t)}")
        if not 1 <= len(q) <= MAX_LEN:
            raise ValueError(f"{what}: a stop sequence holds 1 to MAX_LEN = {MAX_LEN} tokens, got {len(q)}")
        out.add(tuple(int(t) for t in q))
    if len(out) > MAX_SEQS:
        raise ValueError(f"{what}: {len(out)} distinct sequences, at most MAX_SEQS = {MAX_SEQS} per request")
    return tuple(sorted(out))


def truncate(tokens, seqs, m=0):
    """The g (1-based) at which the generated tokens `tokens` stop for the sequences `seqs` with min_new_tokens `m`, or
    None when no sequence matches at a g > m."""
    y = [int(t) for t in tokens]
    seqs = [[int(t) for t in q] for q in (seqs or ())]
    for g in range(max(int(m), 0) + 1, len(y) + 1):
        if any(len(q) <= g and y[g - len(q):g] == q for q in seqs):
            return g
    return None


def capacity(n, floor):
    """n rounded up to a power of two, at least `floor`."""
    c = floor
    while c < n:
        c *= 2
    return c


def packed(sets, set_of=None):
    """The sets `sets` (each a sequence of token-id sequences) as three int32 CSR arrays: set_off (n_sets + 1,) indexes into
    seq_off (n_seqs + 1,), which indexes into toks.  With `set_of` (one set id per request, -1: none) returns it as int32
    beside them."""
    set_off, seq_off, toks = [0], [0], []
    for s in sets:
        for q in s:
            toks += [int(t) for t in q]
            seq_off.append(len(toks))
        set_off.append(len(seq_off) - 1)
    out = (np.array(set_off, np.int32), np.array(seq_off, np.int32), np.array(toks, np.int32).reshape(-1))
    return out if set_of is None else out + (np.asarray(set_of, np.int32).reshape(-1),)


def padded(tables, caps):
    """The CSR arrays at a capacity `caps` = (sets, seqs, tokens): set_off (sets + 1,), seq_off (seqs + 1,), toks (tokens,);
    the sets and sequences past the call's are empty."""
    set_off, seq_off, toks = tables
    n_sets, n_seqs, n_toks = set_off.size - 1, seq_off.size - 1, toks.size
    if n_sets > caps[0] or n_seqs > caps[1] or n_toks > caps[2]:
        raise ValueError(f"{n_sets} sets / {n_seqs} sequences / {n_toks} tokens do not fit the capacity {tuple(caps)}")
    a, b, c = np.full(caps[0] + 1, n_seqs, np.int32), np.full(caps[1] + 1, n_toks, np.int32), np.zeros(caps[2], np.int32)
    a[:n_sets + 1], b[:n_seqs + 1], c[:n_toks] = set_off, seq_off, toks
    return a, b, c


def match(tables, s, tail, g, tok=None):
    """Whether a sequence of set `s` of the CSR `tables` ends at generated token g of a row whose tail ring `tail`
    (MAX_LEN,) holds y_j at slot j % MAX_LEN (`tok`: y_g itself, when the ring does not hold it yet)."""
    set_off, seq_off, toks = tables
    if s < 0 or s + 1 >= set_off.size:
        return False
    for q in range(int(set_off[s]), int(set_off[s + 1])):
        lo, hi = int(seq_off[q]), int(seq_off[q + 1])
        n = hi - lo
        if 1 <= n <= min(g, MAX_LEN) and all(
                int(toks[hi - 1 - j]) == (int(tok) if j == 0 and tok is not None else int(tail[(g - j) % MAX_LEN]))
                for j in range(n)):
            return True
    return False


class StopSeqs:
    """The checked `stop_sequences` of a call: `sets` the distinct sets (sorted tuples of int tuples), `set_of[r]` request
    r's set id (-1: none), `m` min_new_tokens, `tables` the CSR arrays of `packed`, `caps` their sizes rounded up to powers
    of two: the capacity of a plan that holds them."""

    def __init__(self, V, sets, set_of, m=0):
        self.V, self.sets, self.m = int(V), list(sets), int(m)
        self.set_of = np.asarray(set_of, np.int32).reshape(-1)
        self.tables = packed(self.sets)
        self.caps = (capacity(len(self.sets), 16), capacity(self.tables[1].size - 1, 64),
                     capacity(self.tables[2].size, 256))
        # the sets as `Rows.feed` compares them, all rows at once: every sequence backwards (its last token first), padded
        self.lens = np.zeros((len(self.sets), MAX_SEQS), np.int64)
        self.rev = np.full((len(self.sets), MAX_SEQS, MAX_LEN), -1, np.int64)
        for i, s in enumerate(self.sets):
            for j, q in enumerate(s):
                self.lens[i, j], self.rev[i, j, :len(q)] = len(q), q[::-1]

    def sets_of(self, reqs):
        reqs = np.asarray(reqs, np.int64).reshape(-1)
        return np.where(reqs >= 0, self.set_of[np.maximum(reqs, 0)], -1).astype(np.int32)

    def seqs(self, r):
        """Request r's sequences (a tuple of int tuples; empty: none)."""
        s = int(self.set_of[int(r)])
        return () if s < 0 else self.sets[s]


def check_args(stop_sequences=None, V=0, n=1, m=0, speculate=0):
    """Validate the `stop_sequences` of a call with `n` prompts / requests over a vocabulary of `V` tokens and
    min_new_tokens `m`; returns a `StopSeqs`, or None when the argument is off.  ValueError: see the module docstring."""
    ss = stop_sequences
    if ss is None:
        return None
    if not _is_seq(ss) or isinstance(ss, np.ndarray) and ss.ndim < 2:
        raise ValueError(f"stop_sequences must be a sequence of token-id sequences, or one such (or None) per request, "
                         f"got {ss!r}")
    ss = list(ss)
    if not ss:
        return None
    shared = [_is_seq(e) and all(_is_id(t) for t in e) for e in ss]
    per_req = [e is None or (_is_seq(e) and all(_is_seq(q) for q in e)) for e in ss]
    # (an empty element reads either way: [[]] is a shared sequence without tokens, refused below)
    if all(shared):
        sets = [_one_set("stop_sequences", ss, V)] * n
    elif all(per_req):
        if len(ss) != n:
            raise ValueError(f"stop_sequences: {len(ss)} entries for {n} requests")
        sets = [None if e is None or not len(e) else _one_set(f"stop_sequences of request {r}", e, V)
                for r, e in enumerate(ss)]
    else:
        raise ValueError("stop_sequences mixes token-id sequences with per-request entries (None or sequences of "
                         "sequences)")
    if all(s is None for s in sets):
        return None
    if isinstance(m, (bool, np.bool_)) or not isinstance(m, _INT) or m < 0:
        raise ValueError(f"min_new_tokens must be a non-negative integer, got {m!r}")
    if speculate:
        raise ValueError("stop_sequences cannot be combined with speculate > 0 (a match could end inside a draft)")
    distinct = sorted({s for s in sets if s is not None})
    if sum(len(s) for s in distinct) > MAX_CALL_SEQS:        # (equal sets are held once)
        raise ValueError(f"stop_sequences: more than {MAX_CALL_SEQS} sequences over all requests")
    index = {s: i for i, s in enumerate(distinct)}
    return StopSeqs(V, distinct, [-1 if s is None else index[s] for s in sets], m)


class Rows:
    """The host's per-row matcher: per row the set it matches against (-1: none), the count g of tokens its request has
    generated, its first token (-1: none yet) and the last MAX_LEN of them -- y_j at slot j % MAX_LEN of `tail`, as
    csrc/stop_seq.hip keeps them.  The eager and generic paths stop rows by it; the graph paths follow the device with it
    from the tokens they poll, as they follow the stop ids."""

    def __init__(self, B, spec, reqs=None):
        self.spec = spec
        self.set = np.full(B, -1, np.int32)
        self.count = np.zeros(B, np.int64)
        self.first = np.full(B, -1, np.int64)
        self.tail = np.full((B, MAX_LEN), -1, np.int32)
        if reqs is not None:                     # (generate_ragged: row b holds request b from the start)
            self.reset(np.arange(B), reqs)

    def reset(self, rows, reqs, first_tokens=None):
        """Rows `rows` take requests `reqs`: nothing generated, a cleared tail.  `first_tokens`: the requests' first tokens,
        fed right away; returns the listed rows this stopped, (len(rows),) bool."""
        rows = np.asarray(rows, np.int64).reshape(-1)
        self.set[rows] = self.spec.sets_of(reqs)
        self.count[rows], self.first[rows], self.tail[rows] = 0, -1, -1
        if first_tokens is None:
            return np.zeros(rows.size, bool)
        toks = np.full(self.set.size, -1, np.int64)
        toks[rows] = np.asarray(first_tokens, np.int64).reshape(-1)
        return self.feed(toks)[rows]

    def feed(self, tokens):
        """Every row's token of a step, (B,) (< 0: the row yielded none and is left as it is).  Returns the rows that stop
        at this token, (B,) bool."""
        tokens = np.asarray(tokens, np.int64).reshape(-1)
        stopped = np.zeros(tokens.size, bool)
        rows = np.flatnonzero((tokens >= 0) & (self.set >= 0))
        if not rows.size:
            return stopped
        g = self.count[rows] + 1
        self.count[rows] = g
        self.first[rows] = np.where(g == 1, tokens[rows], self.first[rows])
        self.tail[rows, g % MAX_LEN] = tokens[rows]
        # `match` for every row and sequence at once: the row's last MAX_LEN tokens, newest first, against the sequences
        # backwards; places past a sequence's length agree by definition
        j = np.arange(MAX_LEN)
        last = self.tail[rows[:, None], (g[:, None] - j) % MAX_LEN]                      # (R, MAX_LEN)
        lens, rev = self.spec.lens[self.set[rows]], self.spec.rev[self.set[rows]]        # (R, MAX_SEQS), (R, MAX_SEQS, MAX_LEN)
        same = ((last[:, None, :] == rev) | (j >= lens[:, :, None])).all(-1)
        stopped[rows] = (same & (lens >= 1) & (lens <= g[:, None])).any(-1) & (g > self.spec.m)
        return stopped
