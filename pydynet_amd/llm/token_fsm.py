"""Constrained decoding for `Llama.generate`, `generate_ragged`, `serve` and `serve_all`: `token_fsm`, a finite-state
machine over token ids that masks a row's logits by the row's current state and advances on the token the row is fed.

This module states the contract in NumPy; on a HIP device the graph-replayed steps run it through csrc/token_fsm.hip
(include/pdn_fsm.h), which computes the same bits.  A machine has states 0 .. S - 1; state s has explicit edges
{token: next state} and an optional default next state dflt[s] (-1: none): with a default every token is allowed in s, the
ones without an edge lead to dflt[s].  For row b's fp32 logits z (length V) at the step that yields the token at position
t, with s_b the row's prompt length and g = t - s_b the tokens it has generated so far:
  1. g == 0: the row's state is its request's start state.  g > 0: the state is advanced by the token fed at position
     t - 1 -- the explicit edge when there is one, else the default, else (neither: only when other edits banned every
     allowed token) the state is kept;
  2. z[v] = -inf for every v the state does not allow;
  3. order within a step: the penalties of llm/penalties.py, then this mask, then the edits of llm/logit_edits.py, then
     llm/sampling.py and llm/logprobs.py on the result: a token the machine bans has log-probability -inf;
  4. a row at a position < 0 is untouched and keeps its state; a request without a machine is off: state -1, no mask.
The device form is CSR: offsets (S + 1,), tokens (E,) sorted within each state, next (E,), dflt (S,), all int32; the
machines of one call are merged into one state space with a start state per request (`packed`).  A row's state is kept
as one 64-bit word, (position << 32) | state (`pair`): the state the row is in at that position.
The default (None) is off: `check_args` returns None for it and every caller keeps its plain path.
"""
from collections.abc import Mapping

import numpy as np

MAX_STATES = 65536       # states of one call's merged machines
MAX_EDGES = 1 << 22      # explicit edges of one call's merged machines (16 MiB of tokens, as much of next states)

_INT = (int, np.integer)


def _int(what, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, _INT):
        raise ValueError(f"{what} must be an integer, got {v!r}")
    return int(v)


class Tables:
    """A machine, or the merged machines of a call, in the device form (int32 arrays)."""

    def __init__(self, offsets, tokens, nxt, dflt):
        self.offsets, self.tokens, self.next, self.dflt = (np.ascontiguousarray(a, np.int32).reshape(-1)
                                                           for a in (offsets, tokens, nxt, dflt))

    @property
    def S(self):
        return self.dflt.size

    @property
    def E(self):
        return self.tokens.size

    def arrays(self):
        return self.offsets, self.tokens, self.next, self.dflt


class TokenFSM(Tables):
    """`transitions[s]`: a mapping {token id: next state} for states 0 .. S - 1; `start`: the state of a row that has
    generated nothing; `default[s]` (optional; -1: none): the next state of every token without an edge in s, which also
    allows every token there.  ValueError for a non-integer, a negative id (an id >= V: `check_args`), a next state
    outside [0, S), a state with neither an edge nor a default, or more than MAX_STATES states / MAX_EDGES edges."""

    def __init__(self, transitions, start=0, default=None):
        if isinstance(transitions, (Mapping, str, bytes)) or not hasattr(transitions, "__len__"):
            raise ValueError("transitions must be a sequence with one {token: next state} mapping per state")
        S = len(transitions)
        if S == 0:
            raise ValueError("a machine needs at least one state")
        if S > MAX_STATES:
            raise ValueError(f"{S} states, at most MAX_STATES = {MAX_STATES}")
        if default is None:
            dflt = np.full(S, -1, np.int64)
        else:
            if isinstance(default, (str, bytes, Mapping)) or not hasattr(default, "__len__") or len(default) != S:
                raise ValueError(f"default must hold one next state (or -1) per state, {S} of them")
            dflt = np.array([-1 if d is None else _int("a default state", d) for d in default], np.int64)
            if ((dflt < -1) | (dflt >= S)).any():
                raise ValueError(f"default states must lie in [0, {S}) or be -1")
        self.start = _int("the start state", start)
        if not 0 <= self.start < S:
            raise ValueError(f"the start state must lie in [0, {S}), got {self.start}")
        offsets, toks, nxts = np.zeros(S + 1, np.int64), [], []
        for s, edges in enumerate(transitions):
            if not isinstance(edges, Mapping):
                raise ValueError(f"transitions[{s}] must be a mapping of token id to next state, got {type(edges).__name__}")
            t = np.array([_int(f"a token id of state {s}", k) for k in edges], np.int64)
            n = np.array([_int(f"a next state of state {s}", edges[k]) for k in edges], np.int64)
            if t.size and t.min() < 0:
                raise ValueError(f"state {s}: token ids must not be negative")
            if n.size and (n.min() < 0 or n.max() >= S):
                raise ValueError(f"state {s}: next states must lie in [0, {S})")
            if np.unique(t).size != t.size:
                raise ValueError(f"state {s}: a token id appears twice")
            if not t.size and dflt[s] < 0:
                raise ValueError(f"state {s} has neither an edge nor a default: nothing could be picked there")
            order = np.argsort(t, kind="stable")
            toks.append(t[order])
            nxts.append(n[order])
            offsets[s + 1] = offsets[s] + t.size
            if offsets[s + 1] > MAX_EDGES:
                raise ValueError(f"more than MAX_EDGES = {MAX_EDGES} edges")
        tokens = np.concatenate(toks) if toks else np.zeros(0, np.int64)
        if tokens.size and tokens.max() > np.iinfo(np.int32).max:
            raise ValueError("token ids must fit 32 bits")
        super().__init__(offsets, tokens, np.concatenate(nxts) if nxts else np.zeros(0, np.int64), dflt)

    def check_vocab(self, V):
        if self.tokens.size and int(self.tokens.max()) >= V:
            raise ValueError(f"token_fsm: token ids must lie in [0, {V}), got {int(self.tokens.max())}")

    @classmethod
    def from_sequences(cls, seqs, end):
        """The trie of the token-id sequences `seqs`: exactly one of them, then `end`, which leads to a terminal state that
        loops on `end`.  A sequence that is a proper prefix of another allows both `end` and the continuation.  ValueError
        for no sequence, an empty or a repeated one, a non-integer, or `end` inside a sequence."""
        end = _int("end", end)
        seqs = [list(q) for q in seqs]
        if not seqs:
            raise ValueError("from_sequences needs at least one sequence")
        trans, done = [{}], set()
        for q in seqs:
            if not q:
                raise ValueError("from_sequences: an empty sequence")
            s = 0
            for t in q:
                t = _int("a token id", t)
                if t == end:
                    raise ValueError(f"from_sequences: the end token {end} appears inside a sequence")
                if t not in trans[s]:
                    trans.append({})
                    trans[s][t] = len(trans) - 1
                s = trans[s][t]
            if s in done:
                raise ValueError(f"from_sequences: the sequence {q} appears twice")
            done.add(s)
        trans.append({end: len(trans)})
        for s in done:
            trans[s][end] = len(trans) - 1
        return cls(trans, 0)

    @classmethod
    def free_until(cls, close, then):
        """Any tokens until `close`, then the machine `then`: state 0 has itself as its default and an edge `close` into
        the start of `then` (whose states follow, shifted by one)."""
        close = _int("close", close)
        if not isinstance(then, TokenFSM):
            raise ValueError(f"free_until: `then` must be a TokenFSM, got {type(then).__name__}")
        trans = [{close: then.start + 1}]
        for s in range(then.S):
            lo, hi = then.offsets[s], then.offsets[s + 1]
            trans.append({int(t): int(n) + 1 for t, n in zip(then.tokens[lo:hi], then.next[lo:hi])})
        return cls(trans, 0, [0] + [int(d) + 1 if d >= 0 else -1 for d in then.dflt])


def pair(state, pos):
    """A row's state word: (position << 32) | state (int64)."""
    return (np.asarray(pos, np.int64) << 32) | (np.asarray(state, np.int64) & 0xFFFFFFFF)


def unpair(word):
    """`pair` back: (state, position), int32 each."""
    w = np.atleast_1d(np.asarray(word, np.int64))
    return (w & 0xFFFFFFFF).astype(np.uint32).view(np.int32), (w >> 32).astype(np.int32)


def advance(fsm, states, tokens):
    """The states (B,) after each row is fed its token: the explicit edge, else the default, else the state itself; a
    state outside [0, S) (-1: off) stays."""
    states = np.array(states, np.int64).reshape(-1)
    tokens = np.asarray(tokens, np.int64).reshape(-1)
    for b, (s, t) in enumerate(zip(states.tolist(), tokens.tolist())):
        if not 0 <= s < fsm.S:
            continue
        lo, hi = int(fsm.offsets[s]), int(fsm.offsets[s + 1])
        j = lo + int(np.searchsorted(fsm.tokens[lo:hi], t))
        if j < hi and fsm.tokens[j] == t:
            states[b] = fsm.next[j]
        elif fsm.dflt[s] >= 0:
            states[b] = fsm.dflt[s]
    return states


def apply(z, fsm, states):
    """The mask on arrays: z (B, V) float32 logits, states (B,); a row in a state outside [0, S) (-1: off) or in a state
    with a default is left as it is.  Returns the masked float32 rows (a new array)."""
    z = np.array(z, np.float32)
    V = z.shape[1]
    for b, s in enumerate(np.asarray(states, np.int64).reshape(-1).tolist()):
        if not 0 <= s < fsm.S or fsm.dflt[s] >= 0:
            continue
        t = fsm.tokens[fsm.offsets[s]:fsm.offsets[s + 1]]
        out = np.ones(V, bool)
        out[t[t < V]] = False
        z[b, out] = np.float32(-np.inf)
    return z


def step_states(fsm, word, start_state, start, ids, pos):
    """The state every row is in at its position pos[b] (statement 1) from the rows' state words: the start state at
    g = pos - start <= 0; the word's state when the word is already at pos; else that state advanced by the fed token
    ids[b].  Rows at pos < 0 keep their word.  Returns (states (B,) int32 -- of rows at pos < 0: the word's --, the new
    words (B,) int64)."""
    word = np.array(word, np.int64).reshape(-1)
    pos = np.asarray(pos, np.int64).reshape(-1)
    s, tag = unpair(word)
    cur = np.where(tag == pos, s, advance(fsm, s, ids)).astype(np.int64)
    cur = np.where(pos - np.asarray(start, np.int64).reshape(-1) <= 0, np.asarray(start_state, np.int64).reshape(-1), cur)
    live = pos >= 0
    cur = np.where(live, cur, s)
    word[live] = pair(cur[live], pos[live])
    return cur.astype(np.int32), word


def packed(fsms):
    """The device form of a call's machines: `fsms[r]` = request r's TokenFSM or None.  Distinct machines (by identity) are
    merged into one state space in the order they first appear.  Returns (Tables, starts (n,) int32: request r's start
    state, -1 without a machine)."""
    seen, parts, base = {}, [], 0
    starts = np.full(len(fsms), -1, np.int32)
    for r, f in enumerate(fsms):
        if f is None:
            continue
        if id(f) not in seen:
            seen[id(f)] = base
            parts.append((f, base))
            base += f.S
        starts[r] = seen[id(f)] + f.start
    if base > MAX_STATES:
        raise ValueError(f"token_fsm: {base} states in one call, at most MAX_STATES = {MAX_STATES}")
    if sum(f.E for f, _ in parts) > MAX_EDGES:
        raise ValueError(f"token_fsm: more than MAX_EDGES = {MAX_EDGES} edges in one call")
    offsets, e0 = [np.zeros(1, np.int64)], 0
    for f, _ in parts:
        offsets.append(f.offsets[1:].astype(np.int64) + e0)
        e0 += f.E
    cat = lambda xs, shift: (np.concatenate([np.where(a >= 0, a + b, a) if shift else a for a, b in xs])
                             if xs else np.zeros(0, np.int32))
    return Tables(np.concatenate(offsets), cat([(f.tokens, 0) for f, _ in parts], False),
                  cat([(f.next, b) for f, b in parts], True), cat([(f.dflt, b) for f, b in parts], True)), starts


def unpacked(tables, start=0):
    """`packed` back: the TokenFSM over all states of `tables` that starts in `start`."""
    trans = [{int(t): int(n) for t, n in zip(tables.tokens[tables.offsets[s]:tables.offsets[s + 1]],
                                             tables.next[tables.offsets[s]:tables.offsets[s + 1]])}
             for s in range(tables.S)]
    return TokenFSM(trans, int(start), [int(d) for d in tables.dflt])


def padded(tables, S_cap, E_cap):
    """`tables` at a capacity: offsets (S_cap + 1,), tokens / next (E_cap,), dflt (S_cap,); the states past S have no edge
    and no default (nothing leads to them)."""
    S, E = tables.S, tables.E
    if S > S_cap or E > E_cap:
        raise ValueError(f"{S} states / {E} edges do not fit the capacity {S_cap} / {E_cap}")
    off = np.full(S_cap + 1, E, np.int32)
    off[:S + 1] = tables.offsets
    tok, nxt, dfl = np.zeros(E_cap, np.int32), np.zeros(E_cap, np.int32), np.full(S_cap, -1, np.int32)
    tok[:E], nxt[:E], dfl[:S] = tables.tokens, tables.next, tables.dflt
    return off, tok, nxt, dfl


def capacity(n, floor):
    """n rounded up to a power of two, at least `floor`."""
    c = floor
    while c < n:
        c *= 2
    return c


class Machines:
    """The checked `token_fsm` of a call: `fsms[r]` = request r's TokenFSM or None, `tables` their merged device form,
    `starts[r]` request r's start state in it (-1: off), `caps` = (S, E) rounded up to powers of two: the capacity of a
    plan that holds the tables."""

    def __init__(self, V, fsms):
        self.V, self.fsms = V, fsms
        self.tables, self.starts = packed(fsms)
        self.caps = (capacity(self.tables.S, 64), capacity(self.tables.E, 1024))

    def start_states(self, reqs):
        reqs = np.asarray(reqs, np.int64).reshape(-1)
        return np.where(reqs >= 0, self.starts[np.maximum(reqs, 0)], -1).astype(np.int32)


def check_args(token_fsm=None, V=0, n=1, speculate=0):
    """Validate the `token_fsm` of a call with `n` prompts / requests over a vocabulary of `V` tokens: one TokenFSM for
    every request, or a sequence with one TokenFSM (or None) per request.  Returns a `Machines`, or None when nothing is on.
    ValueError: another type, a wrong count, a token id >= V, too many states / edges in all, or speculate > 0."""
    if token_fsm is None:
        return None
    if isinstance(token_fsm, TokenFSM):
        fsms = [token_fsm] * n
    else:
        if isinstance(token_fsm, (str, bytes, Mapping)) or not hasattr(token_fsm, "__len__"):
            raise ValueError(f"token_fsm must be a TokenFSM or a sequence with one (or None) per request, got {token_fsm!r}")
        if len(token_fsm) != n:
            raise ValueError(f"token_fsm: {len(token_fsm)} entries for {n} requests")
        fsms = list(token_fsm)
        for r, f in enumerate(fsms):
            if f is not None and not isinstance(f, TokenFSM):
                raise ValueError(f"token_fsm of request {r} must be a TokenFSM or None, got {type(f).__name__}")
    if all(f is None for f in fsms):
        return None
    for f in fsms:
        if f is not None:
            f.check_vocab(V)
    if speculate:
        raise ValueError("token_fsm cannot be combined with speculate > 0 (draft positions would need their own states)")
    return Machines(int(V), fsms)


class Rows:
    """The per-row state of the statement on the host (every path without the device state of csrc/token_fsm.hip): the
    request each row holds (-1: none), its prompt length, its start state and its state word."""

    def __init__(self, B, spec, reqs=None, start=None):
        self.spec = spec
        self.req = np.full(B, -1, np.int64)
        self.start = np.zeros(B, np.int64)
        self.start_state = np.full(B, -1, np.int32)
        self.word = pair(np.full(B, -1), np.zeros(B))
        if reqs is not None:                     # (generate / generate_ragged: row b holds request b from the start)
            self.reset(np.arange(B), reqs, start)

    def reset(self, rows, reqs, start):
        """Rows `rows` take requests `reqs` with prompt lengths `start`."""
        rows = np.asarray(rows, np.int64).reshape(-1)
        self.req[rows] = np.asarray(reqs, np.int64).reshape(-1)
        self.start[rows] = np.asarray(start, np.int64).reshape(-1)
        self.start_state[rows] = self.spec.start_states(self.req[rows])
        self.word[rows] = pair(self.start_state[rows], self.start[rows])

    def step(self, z, ids, pos):
        """A step of every row: fed ids (B,) at positions pos (B,) (-1: a row that computes nothing, left as it is), the
        states advanced (statement 1) and the (B, V) float32 logits masked (a new array)."""
        pos = np.asarray(pos, np.int64).reshape(-1)
        ids = np.asarray(ids, np.int64).reshape(-1)
        cur, self.word = step_states(self.spec.tables, self.word, self.start_state, self.start, ids, pos)
        return apply(z, self.spec.tables, np.where(pos >= 0, cur, -1))
