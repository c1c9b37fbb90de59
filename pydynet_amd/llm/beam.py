"""Beam search for `Llama.beam_search`: the W most probable continuations of each prompt, best finished sequences first.

This module states the contract in NumPy and runs it on the `cpu` device and in training mode; on a HIP device the same
steps run inside the graph-replayed decode step (csrc/beam.hip: top-k, select, KV-cache reorder).

Rows g * W .. g * W + W - 1 hold the beams of prompt g.  Step 0 is the prompt pass (its last real position's logits, only
beam 0's candidates: initial scores [0, -inf, ...]); step s >= 1 is one decode step of every live row.  Per step and live
group g:
  1. logp_r = z_r - logsumexp(z_r) for each beam row r, the log-sum-exp in float64, logp in float32;
  2. candidate (beam j, token v) has score float32(score_j + logp_j[v]); all candidates ordered by score descending,
     ties to the lower (beam index, token id);
  3. next beams: the first W candidates whose token is not a stop id (beam k = the k-th of them); a beam's tokens are its
     parent's tokens plus v, and its parent row's KV history comes with it;
  4. finished hypotheses: a stop-id candidate among the first W of the whole order, recorded as (step, parent beam, stop
     id, raw score), in that order;
  5. a group holding >= W finished hypotheses is done: its rows stop (position -1) and write no cache.
After `max_new_tokens` generated tokens the live beams of groups that are not done become hypotheses too.  A hypothesis'
normalised score is score / n_gen ** length_penalty (float64), n_gen = its generated tokens, a stop id included.  Per
group the W best by normalised score are returned, ties to the earlier step, then the earlier record (the finished
entries of a step in order, then the end-of-budget beams in beam order).
"""
import numpy as np

MAX_BEAMS = 16
MAX_STOPS = 16


def log_softmax_rows(z):
    """float32(z - logsumexp(z)) per row, the log-sum-exp in float64."""
    z = np.asarray(z, np.float64)
    m = z.max(-1, keepdims=True)
    lse = m + np.log(np.exp(z - m).sum(-1, keepdims=True))
    return (z - lse).astype(np.float32)


def topk_rows(z, W, stops):
    """Step 1 and the per-row part of step 2: for each row of z (R, V), the W best non-stop tokens by (logp desc, id asc)
    as (logp (R, W) float32, ids (R, W) int64) and the logp of every stop id (R, S) float32."""
    lp = log_softmax_rows(z)
    stops = np.asarray(stops, np.int64)
    masked = lp.copy()
    masked[:, stops] = -np.inf
    R, V = lp.shape
    ids = np.empty((R, W), np.int64)
    for r in range(R):
        order = np.lexsort((np.arange(V), -masked[r].astype(np.float64)))   # logp desc, then id asc
        ids[r] = order[:W]
    return np.take_along_axis(lp, ids, 1), ids, lp[:, stops]


def select_group(scores, cand_lp, cand_id, stop_lp, stops, W, first=False):
    """Steps 2-4 for one group: scores (W,) float32, cand_lp / cand_id (W, W), stop_lp (W, S) of its rows.  Returns
    (tokens (W,) int64, parent beams (W,) int64, new scores (W,) float32, finished [(parent beam, stop id, raw score)])."""
    nb = 1 if first else W
    sc = np.zeros(1, np.float32) if first else np.asarray(scores, np.float32)
    S = len(stops)
    beam = np.concatenate([np.repeat(np.arange(nb), W), np.repeat(np.arange(nb), S)])
    tok = np.concatenate([np.asarray(cand_id[:nb]).reshape(-1), np.tile(np.asarray(stops, np.int64), nb)])
    lp = np.concatenate([np.asarray(cand_lp[:nb], np.float32).reshape(-1), np.asarray(stop_lp[:nb], np.float32).reshape(-1)])
    score = (sc[beam] + lp).astype(np.float32)
    is_stop = np.arange(beam.size) >= nb * W
    order = np.lexsort((tok, beam, -score.astype(np.float64)))
    ns = order[~is_stop[order]][:W]
    fin = [(int(beam[c]), int(tok[c]), np.float32(score[c])) for c in order[:W] if is_stop[c]]
    return tok[ns].astype(np.int64), beam[ns].astype(np.int64), score[ns], fin


def backtrack(hist, s, j):
    """The tokens of beam j after step s: hist (steps, B_group, 2) of one group -> int64 array of length s + 1."""
    out = []
    for t in range(s, -1, -1):
        out.append(int(hist[t, j, 0]))
        j = int(hist[t, j, 1])
    return np.array(out[::-1], np.int64)


def results(hist, fins, live_scores, last_step, W, length_penalty):
    """Per group: the W best hypotheses, [(tokens, normalised score)], best first.
    hist (steps, G * W, 2) int: (token, parent beam) of every row at every step; fins[g] = [(step, parent beam, stop id,
    raw score)] in record order; live_scores[g]: None for a done group, else the (W,) scores of its beams after step
    `last_step` (their hypotheses end there)."""
    G = len(fins)
    out = []
    for g in range(G):
        h = np.asarray(hist)[:, g * W:(g + 1) * W]
        hyps = []
        for (s, par, stop, raw) in fins[g]:
            toks = np.concatenate([backtrack(h, s - 1, par), [stop]]) if s > 0 else np.array([stop], np.int64)
            hyps.append((toks.astype(np.int64), float(raw) / float(s + 1) ** length_penalty, s))
        if live_scores[g] is not None:
            for j in range(W):
                hyps.append((backtrack(h, last_step, j),
                             float(live_scores[g][j]) / float(last_step + 1) ** length_penalty, last_step))
        order = sorted(range(len(hyps)), key=lambda i: (-hyps[i][1], hyps[i][2], i))
        out.append([(hyps[i][0], hyps[i][1]) for i in order[:W]])
    return out
