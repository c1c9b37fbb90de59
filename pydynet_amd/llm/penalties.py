"""Repetition, presence and frequency penalties for `Llama.generate`, `generate_ragged`, `serve` and `serve_all`.

This module states the contract in NumPy; on a HIP device the graph-replayed steps run it through csrc/penalty.hip, which
computes the same bits.  For row b's fp32 logits z (length V) at the step that yields the token at position t:
  c[v] = how many times row b GENERATED token v at positions before t (prompt tokens are not counted),
  P    = the set of token ids in row b's prompt.
  1. repetition r (the Hugging Face / CTRL rule, once per token however often it appears): for every v with v in P or
     c[v] > 0, z[v] = z[v] / r if z[v] > 0, else z[v] * r;
  2. presence p and frequency f (the OpenAI rule, generated tokens only): for every v with c[v] > 0,
     z[v] = z[v] - (f * c[v] + p).
  3. The sampling contract of llm/sampling.py runs unchanged on the penalised row (temperature 0: the first maximum).
Every operation is one float32 rounding, in this order: z / r, z * r, f * c, + p, z - (...); no fused multiply-add.
The defaults (1, 0, 0) are "off": `check_args` returns None for them and every caller keeps its plain path.
"""
import math

import numpy as np


def check_args(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, speculate=0):
    """Validate the penalty arguments; returns (r, p, f) as Python floats, or None when all three are at their defaults."""
    vals = []
    for name, v in (("repetition_penalty", repetition_penalty), ("presence_penalty", presence_penalty),
                    ("frequency_penalty", frequency_penalty)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"{name} must be a real number, got {v!r}")
        v = float(v)
        if not math.isfinite(v) or not math.isfinite(float(np.float32(v))):
            raise ValueError(f"{name} must be finite (in float32), got {v}")
        vals.append(v)
    r, p, f = vals
    if not r > 0.0 or not np.float32(r) > 0:
        raise ValueError(f"repetition_penalty must be > 0, got {r}")
    if (r, p, f) == (1.0, 0.0, 0.0):
        return None
    if speculate:
        raise ValueError("penalties cannot be combined with speculate > 0 (draft positions would need their own counts)")
    return r, p, f


def penalize(z, counts, seen, r, p, f):
    """The statement on arrays: z (B, V) float32 logits, counts (B, V) generated-token counts, seen (B, V) bool prompt
    membership.  Returns the penalised float32 rows (a new array)."""
    z = np.array(z, np.float32)
    c = np.asarray(counts)
    seen = np.asarray(seen, bool)
    r32, p32, f32 = np.float32(r), np.float32(p), np.float32(f)
    with np.errstate(over="ignore", invalid="ignore"):
        rep = seen | (c > 0)
        z = np.where(rep, np.where(z > 0, z / r32, z * r32), z).astype(np.float32)
        sub = (f32 * c.astype(np.float32)).astype(np.float32) + p32
        z = np.where(c > 0, z - sub.astype(np.float32), z).astype(np.float32)
    return z


def seen_rows(prompts, V):
    """(B, V) bool: token v appears in prompt b."""
    out = np.zeros((len(prompts), V), bool)
    for b, q in enumerate(prompts):
        out[b, np.asarray(q, np.int64).reshape(-1)] = True
    return out


def seen_bits(prompts, V):
    """The prompt sets as the kernels keep them: (B, ceil(V / 32)) int32, bit v & 31 of word v >> 5 set for v in P."""
    bits = np.zeros((len(prompts), -(-V // 32)), np.uint32)
    for b, q in enumerate(prompts):
        q = np.unique(np.asarray(q, np.int64).reshape(-1))
        np.bitwise_or.at(bits[b], q >> 5, np.uint32(1) << (q & 31).astype(np.uint32))
    return bits.view(np.int32)


def packed(prompts):
    """The prompt lists of the reset entry: (ids (sum of lengths,) int64, offsets (A + 1,) int32)."""
    lens = [int(np.asarray(q).size) for q in prompts]
    ids = np.concatenate([np.asarray(q, np.int64).reshape(-1) for q in prompts]) if prompts else np.zeros(0, np.int64)
    return ids, np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def params_bytes(r, p, f):
    """pdn_penalty_params (include/pdn_hip.h) as two int64 words: {float repetition; float presence; float frequency;
    int reserved}."""
    return np.array([r, p, f, 0], np.float32).view(np.int64)


class Rows:
    """The per-row state of the statement on the host (every path without the device state of csrc/penalty.hip): row b's
    generated-token counts and prompt set, and the position of its first generated token (its prompt length).  A token
    fed at position t - 1 >= start[b] (the step at t > start[b]) is a generated one and is counted."""

    def __init__(self, B, V, values, prompts=None):
        self.values, self.V, self.prompts = values, V, prompts
        self.counts = np.zeros((B, V), np.int64)
        self.seen = np.zeros((B, V), bool)
        self.start = np.zeros(B, np.int64)
        if prompts is not None:                  # (generate / generate_ragged: row b holds prompt b from the start)
            self.reset(np.arange(B), prompts)

    def reset(self, rows, prompts):
        """Rows `rows` take new prompts: zero counts, their prompt sets, start = prompt length."""
        for b, q in zip(np.asarray(rows, np.int64).reshape(-1), prompts):
            q = np.asarray(q, np.int64).reshape(-1)
            self.counts[b] = 0
            self.seen[b] = False
            self.seen[b, q] = True
            self.start[b] = q.size

    def feed(self, ids, pos):
        """The step at positions pos (B,) (-1: a row that computes nothing) is fed ids (B,): count the generated ones."""
        ids, pos = np.asarray(ids, np.int64).reshape(-1), np.asarray(pos, np.int64).reshape(-1)
        for b in np.flatnonzero((pos >= 0) & (pos > self.start)):
            self.counts[b, ids[b]] += 1

    def apply(self, z, rows=None):
        """The penalised (len(rows), V) float32 logits of rows `rows` (default: all)."""
        rows = slice(None) if rows is None else np.asarray(rows, np.int64).reshape(-1)
        return penalize(z, self.counts[rows], self.seen[rows], *self.values)
