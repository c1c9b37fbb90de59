"""Prefix caching (`Llama.serve(..., prefill_chunk=C, prefix_cache=k)`) on the CPU: the statement of llm/prefix.py against a
brute-force restatement, the argument checks, and end to end on the `cpu` device (where every prompt is computed in full) and
on the emulated C ABI with the copy entry of tests/abi_emulator/_extend.py (the graph path: the mixed step starts a row's
prefill behind the tokens it took), against the `cpu` reference of tests/test_serve.py under its first-difference margin
rule -- with at most one request of a case differing at all."""
import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm import chunked, penalties, prefix
from tests.abi_emulator import copy_prefix_np, counters, margin
from tests.test_serve import SAMPLED, V, _eval, _model, _reference, _want

PEN = dict(repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.2)
KINDS = {"own", "copy", "swap", "live", "short", "cap"}


# -- the statement against a brute-force restatement -----------------------------------------------------------------------
def _brute(p, d, held, valid, k):
    """(donor, n) by the words of the issue, with Python lists."""
    m = []
    for h, v in zip(held, valid):
        h = [] if h is None else list(h)[:int(v)]
        c = 0
        while c < len(p) and c < len(h) and int(p[c]) == int(h[c]):
            c += 1
        m.append(c)
    n = min(max(m), len(p) - 1)
    if n < k:
        return d, 0
    if m[d] >= n:
        return d, n
    return min(b for b in range(len(m)) if m[b] >= n), n


def test_match_against_brute_force():
    rng = np.random.default_rng(0)
    hits = own = other = 0
    for _ in range(3000):
        S = int(rng.integers(1, 6))
        held = [None if rng.random() < 0.2 else rng.integers(0, 4, int(rng.integers(1, 9))) for _ in range(S)]
        valid = [0 if h is None else int(rng.integers(0, len(h) + 1)) for h in held]
        p = rng.integers(0, 4, int(rng.integers(1, 9)))
        if rng.random() < 0.2 and held[0] is not None:
            p = held[0].copy()                                        # a prompt equal to a held prompt
        d, k = int(rng.integers(0, S)), int(rng.integers(1, 4))
        got = prefix.match(p, d, held, valid, k)
        assert got == _brute(p, d, held, valid, k), (p, d, held, valid, k)
        hits += got[1] > 0
        own += got[1] > 0 and got[0] == d
        other += got[1] > 0 and got[0] != d
        assert got[1] <= len(p) - 1 and (got[1] == 0 or got[1] >= k)
    assert hits > 500 and own > 100 and other > 100


def test_match_hand_cases():
    a = np.array([1, 2, 3, 0, 1])
    # the cap: a prompt equal to a held prompt reuses len - 1, the last token is fed
    assert prefix.match(a, 1, [a, None], [5, 0], 1) == (0, 4)
    assert prefix.match(a[:3], 1, [a, None], [5, 0], 1) == (0, 2)    # ... or a prefix of one
    assert prefix.match(a[:1], 0, [a], [5], 1) == (0, 0)              # one token: nothing to reuse
    # the threshold
    assert prefix.match([1, 2, 0, 0], 1, [a, None], [5, 0], 2) == (0, 2)
    assert prefix.match([1, 2, 0, 0], 1, [a, None], [5, 0], 3) == (1, 0)
    # the tie-break: the row's own contents first, then the lowest row
    assert prefix.match([1, 2, 3, 3], 2, [a, a, a], [5, 5, 5], 1) == (2, 3)
    assert prefix.match([1, 2, 3, 3], 2, [a, a, a[:2]], [5, 5, 2], 1) == (0, 3)
    assert prefix.match([1, 2, 3, 3], 2, [a[:1], a, a], [1, 5, 2], 1) == (1, 3)
    # own row counts when it reaches n even if another row matches as far
    assert prefix.match(a, 1, [a, a], [5, 4], 1) == (1, 4)
    # only the valid tokens of a record are offered
    assert prefix.match([1, 2, 3, 0, 0], 1, [a, None], [2, 0], 1) == (0, 2)
    assert prefix.match([1, 2, 3, 0, 0], 1, [a, None], [0, 0], 1) == (1, 0)


def test_schedule_same_step_admissions_see_old_records():
    p = np.array([1, 2, 3, 0])
    sch = prefix.Schedule([p, p, p, p], [1, 1, 1, 1], 2, 64)
    rows, new, don, n = sch.admit()                                   # a cold start: two equal prompts, both computed
    assert rows.tolist() == [0, 1] and don.tolist() == [0, 1] and n.tolist() == [0, 0]
    nf, dec, comp = sch.plan()
    assert nf.tolist() == [4, 4]
    sch.finish(nf, np.array([5, 5]))
    rows, new, don, n = sch.admit()                                   # the second wave hits, each row in its own contents
    assert don.tolist() == [0, 1] and n.tolist() == [3, 3] and sch.fed.tolist() == [3, 3]
    assert sch.plan()[0].tolist() == [1, 1]                           # reused tokens are not fed
    assert sch.stats == dict(requests=4, hits=2, prompt_tokens=16, reused_tokens=6, copies=0, launches=0)


def _step(sch):
    nf, dec, comp = sch.plan()
    sch.finish(nf, np.where(dec | comp, 7, -1))
    return nf.tolist()


def test_schedule_two_rows_take_from_each_other():
    a, b, c = np.array([1, 1, 2, 2, 3]), np.array([2, 2, 1, 1, 3]), np.array([3, 3, 3])
    sch = prefix.Schedule([a, b, c, b, a], [1, 1, 3, 1, 1], 3, 64)
    assert sch.admit()[3].tolist() == [0, 0, 0]
    assert _step(sch) == [5, 5, 3]                                    # rows 0 and 1 end after one token, row 2 goes on
    rows, new, don, n = sch.admit()
    assert rows.tolist() == [0, 1] and new.tolist() == [3, 4] and don.tolist() == [1, 0] and n.tolist() == [4, 4]
    assert _step(sch) == [1, 1, 0]
    assert sch.stats == dict(requests=5, hits=2, prompt_tokens=23, reused_tokens=8, copies=2, launches=0)


def test_schedule_live_donor_offers_only_its_valid_tokens():
    x, long = np.array([0]), np.array([3, 3, 3, 3, 0, 0, 0, 0, 1])
    sch = prefix.Schedule([x, long, long, long], [1, 1, 1, 1], 2, 4)
    sch.admit()
    assert _step(sch) == [1, 3] and sch.valid.tolist() == [1, 3]      # x completes and ends; `long` has 3 tokens fed
    rows, new, don, n = sch.admit()                                   # the same prompt: 9 tokens match, 3 are there
    assert rows.tolist() == [0] and new.tolist() == [2] and don.tolist() == [1] and n.tolist() == [3]
    assert sch.fed.tolist() == [3, 3] and sch.valid.tolist() == [3, 3]
    assert _step(sch) == [0, 4] and sch.valid.tolist() == [3, 7]      # request order: row 1 (request 1) is fed first
    assert _step(sch) == [2, 2] and sch.valid.tolist() == [5, 9]      # row 1 completes and ends
    rows, new, don, n = sch.admit()                                   # request 3: the whole prompt is in row 1; the cap
    assert rows.tolist() == [1] and don.tolist() == [1] and n.tolist() == [8]


def test_schedule_without_reuse_is_the_chunked_schedule():
    rng = np.random.default_rng(1)
    prompts = [rng.integers(0, 4, int(rng.integers(1, 9))) for _ in range(12)]
    budgets = rng.integers(0, 5, 12)
    a = chunked.Schedule([len(p) for p in prompts], budgets, 3, 5)
    b = prefix.Schedule(prompts, budgets, 3, 5, None)
    while True:
        ra, rb = a.admit(), b.admit()
        assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and not rb[3].any()
        if not a.busy():
            assert not b.busy()
            break
        pa, pb = a.plan(), b.plan()
        assert all(np.array_equal(x, y) for x, y in zip(pa, pb))
        toks = np.where(pa[1] | pa[2], 1, -1)
        assert np.array_equal(a.finish(pa[0], toks), b.finish(pb[0], toks))
    assert b.stats["reused_tokens"] == b.stats["hits"] == b.stats["copies"] == 0
    assert b.stats["requests"] == int((budgets > 0).sum())


# -- requests in which every kind of hit occurs --------------------------------------------------------------------------
def requests(vocab, seed, N=13):
    """N requests over three 10-token bases: a base's leading tokens, then a tail of its own; budgets 1 .. 6."""
    rng = np.random.default_rng(seed)
    base = [rng.integers(0, vocab, 10) for _ in range(3)]
    prompts, budgets = [], []
    for _ in range(N):
        b, a = base[int(rng.integers(0, 3))], int(rng.integers(0, 11))
        t = int(rng.integers(0 if a else 1, 4))
        prompts.append(np.concatenate([b[:a], rng.integers(0, vocab, t)]).astype(np.int64))
        budgets.append(int(rng.integers(1, 7)))
    return prompts, budgets


def simulate(prompts, lengths, S, C, k):
    """The statement's prediction for a run without stop ids in which request r yields lengths[r] tokens: (stats with
    `launches` = the steps that have a copy, the kinds of hit that occur)."""
    sch = prefix.Schedule(prompts, lengths, S, C, k)
    kinds, launches = set(), 0
    while True:
        live = (sch.req >= 0) & (sch.fed < sch.row_lens())
        held, valid = list(sch.held), sch.valid.copy()
        rows, new, don, n = sch.admit()
        if k is not None:
            for i, (d, r) in enumerate(zip(rows.tolist(), new.tolist())):
                assert (int(don[i]), int(n[i])) == _brute(prompts[r], d, held, valid, k)
                raw = _brute(prompts[r], d, held, valid, 1)[1]
                full = max(prefix.common(prompts[r], h[:v]) for h, v in zip(held, valid) if h is not None) if any(
                    h is not None for h in held) else 0
                if n[i] and don[i] == d:
                    kinds.add("own")
                if n[i] and don[i] != d:
                    kinds.add("copy")
                    if live[don[i]]:
                        kinds.add("live")
                    j = np.flatnonzero(rows == don[i])
                    if j.size and n[j[0]] and don[j[0]] == d:
                        kinds.add("swap")
                if 0 < raw < k:
                    kinds.add("short")
                if n[i] and full == len(prompts[r]):
                    kinds.add("cap")
            launches += bool(((n > 0) & (don != rows)).any())
        if not sch.busy():
            return dict(sch.stats, launches=launches), kinds
        nf, dec, comp = sch.plan()
        sch.finish(nf, np.where(dec | comp, 1, -1))


# (vocabulary 64: the model of tests/test_serve.py; the seed is chosen so that every kind of hit occurs and the reference
#  run shows no near-tie of its own: `test_reference_alone_shows_no_difference` and `test_every_kind_of_hit_occurs`)
SEED = 115
CASES = [(3, 4, True), (5, 64, True), (3, 64, 3), (5, 4, 3)]          # (slots, chunk, prefix_cache)


def _k(cache):
    return 1 if cache is True else int(cache)


def test_every_kind_of_hit_occurs():
    prompts, budgets = requests(V, SEED)
    seen = set()
    for S, C, cache in CASES:
        st, kinds = simulate(prompts, budgets, S, C, _k(cache))
        assert st["reused_tokens"] > 0 and st["copies"] > 0 and {"own", "copy"} <= kinds, (S, C, cache, st, kinds)
        seen |= kinds
    assert seen == KINDS, KINDS - seen


def _serve_all(m, prompts, budgets, **kw):
    return _eval(m, lambda: m.serve_all(prompts, budgets, **kw))


@pytest.mark.parametrize("kw", [{}, SAMPLED[0], SAMPLED[1], PEN])
def test_reference_alone_shows_no_difference(kw):
    """The `cpu` device without the cache through 3 and 5 slots, against generate_ragged over all requests: equal tokens,
    so a difference in the tests below is the cache's."""
    prompts, budgets = requests(V, SEED)
    ref, _ = _reference(prompts, budgets, **kw)
    want = _want(ref, budgets)
    for S, C in ((3, 4), (5, 64)):
        got = _serve_all(_model("cpu"), prompts, budgets, slots=S, prefill_chunk=C, **kw)
        assert all(np.array_equal(g, w) for g, w in zip(got, want)), (S, C)


# (the requests of tests/test_prefix_gpu.py: vocabulary 256 and the model of tests/test_serve_gpu.py; checked here, without
#  a GPU, in the same two ways)
GPU_SEED = 115


def test_every_kind_of_hit_occurs_in_the_gpu_requests():
    prompts, budgets = requests(256, GPU_SEED)
    seen = set()
    for S, C, cache in CASES:
        st, kinds = simulate(prompts, budgets, S, C, _k(cache))
        assert st["reused_tokens"] > 0 and st["copies"] > 0 and {"own", "copy"} <= kinds, (S, C, cache, st, kinds)
        seen |= kinds
    assert seen == KINDS, KINDS - seen


@pytest.mark.parametrize("kw", [{}, dict(temperature=0.9, top_p=0.92, seed=31), PEN])
def test_gpu_reference_alone_shows_no_difference(kw):
    from tests import test_serve_gpu as tg
    assert kw.get("seed") is None or kw == tg.SAMPLED
    prompts, budgets = requests(256, GPU_SEED)
    ref, _ = tg._ragged_reference(prompts, budgets, **kw)
    for S, C in ((3, 4), (5, 64)):
        got = tg._serve_all(tg._model("cpu", 8), prompts, budgets, slots=S, prefill_chunk=C, **kw)
        assert all(np.array_equal(g, ref[r, :n]) for r, (g, n) in enumerate(zip(got, budgets))), (S, C)


def compare(got, want, ref_logits, prompts, kw):
    """The rule of tests/test_serve.py's `_check`: tokens equal up to a request's first differing token, which must sit at
    a float64 margin below 1e-5 in the reference's logits (penalised as the request's were, when penalties are on) -- and
    at most one request may differ at all.  Returns, per request, the number of leading tokens that agree."""
    assert len(got) == len(want)
    same, differ = [], 0
    for r, (g, w) in enumerate(zip(got, want)):
        if np.array_equal(g, w):
            same.append(len(w))
            continue
        differ += 1
        n = min(len(g), len(w))
        bad = np.flatnonzero(g[:n] != w[:n])
        assert bad.size, (r, g, w)                                    # (same prefix, another length: a budget bug)
        s = int(bad[0])
        same.append(s)
        z = ref_logits[s][r]
        if "repetition_penalty" in kw:
            vocab = z.shape[-1]
            z = penalties.penalize(z[None], np.bincount(w[:s], minlength=vocab)[None],
                                   penalties.seen_rows([prompts[r]], vocab), kw["repetition_penalty"],
                                   kw["presence_penalty"], kw["frequency_penalty"])[0]
        if kw.get("temperature", 0) > 0:
            mg = margin(z, len(prompts[r]) + s, r, kw["temperature"], kw.get("top_k", 0), kw.get("top_p", 1.0), kw["seed"])
        else:
            srt = np.sort(z.astype(np.float64))
            mg = srt[-1] - srt[-2]
        assert mg < 1e-5, (r, s, mg)
    assert differ <= 1, differ
    return same


# -- arguments ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [0, -1, 1.5, "1", [1], np.float32(2.0), 2.0])
def test_bad_prefix_cache_raises_before_anything_runs(emulated_hip, bad):
    from pydynet_amd import _lib
    m = _model("hip:0")
    counters()
    n0 = len(_lib._LIB.calls)
    for call in (m.serve, m.serve_all):
        with pytest.raises(ValueError):
            call([[1, 2], [3]], 4, prefill_chunk=4, prefix_cache=bad)
    assert len(_lib._LIB.calls) == n0
    assert not any(counters())
    assert not hasattr(m, "prefix_stats")


@pytest.mark.parametrize("cache", [True, 1, 3, np.int64(2)])
def test_prefix_cache_needs_a_chunk(cache):
    m = _model("cpu")
    with pytest.raises(ValueError, match="prefill_chunk"):
        m.serve([[1, 2], [3]], 4, prefix_cache=cache)
    with pytest.raises(ValueError, match="prefill_chunk"):
        m.serve_all([[1, 2], [3]], 4, prefix_cache=cache)
    m.serve([[1, 2], [3]], 4, prefill_chunk=2, prefix_cache=cache)    # (checked when called, nothing runs yet)
    for off in (False, None):
        m.serve([[1, 2], [3]], 4, prefix_cache=off)                   # off needs none


# -- end to end --------------------------------------------------------------------------------------------------------------
E2E = [(S, C, cache, kw) for S, C, cache in CASES for kw in ({}, SAMPLED[1])] + [(3, 4, True, PEN), (5, 64, 2, PEN)]


@pytest.mark.parametrize("S,C,cache,kw", E2E)
def test_cpu_device_computes_every_prompt(S, C, cache, kw):
    prompts, budgets = requests(V, SEED)
    want = _serve_all(_model("cpu"), prompts, budgets, slots=S, prefill_chunk=C, **kw)
    m = _model("cpu")
    got = _serve_all(m, prompts, budgets, slots=S, prefill_chunk=C, prefix_cache=cache, **kw)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))       # the same passes: the same tokens
    st, _ = simulate(prompts, budgets, S, C, None)
    assert m.prefix_stats == st
    assert st["hits"] == st["reused_tokens"] == st["copies"] == st["launches"] == 0
    assert st["requests"] == len(prompts) and st["prompt_tokens"] == sum(len(p) for p in prompts)


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("S,C,cache,kw", E2E)
def test_emulated_matches_cpu_without_the_cache(emulated_hip, S, C, cache, kw, graphs, monkeypatch):
    from pydynet_amd.llm.llama import Llama
    monkeypatch.setattr(Llama, "graph_decode", graphs)
    Graph.clear()
    prompts, budgets = requests(V, SEED)
    _, logits = _reference(prompts, budgets, **kw)
    want = _serve_all(_model("cpu"), prompts, budgets, slots=S, prefill_chunk=C, **kw)
    m = _model("hip:0")
    counters()
    got = _serve_all(m, prompts, budgets, slots=S, prefill_chunk=C, prefix_cache=cache, **kw)
    c = counters()
    compare(got, want, logits, prompts, kw)
    assert [len(g) for g in got] == budgets
    st, _ = simulate(prompts, budgets, S, C, _k(cache))
    assert m.prefix_stats == st
    assert st["reused_tokens"] > 0 and st["copies"] > 0 and st["hits"] > 0
    assert c[38] == st["launches"] > 0 and c[33] > 0
    assert m._decode_st["mixed"]["C"] == C


@pytest.mark.parametrize("S,C,cache", CASES[:2])
def test_emulated_logprobs(emulated_hip, S, C, cache):
    Graph.clear()
    prompts, budgets = requests(V, SEED)
    _, logits = _reference(prompts, budgets)
    want = _serve_all(_model("cpu"), prompts, budgets, slots=S, prefill_chunk=C, logprobs=2)
    m = _model("hip:0")
    got = _serve_all(m, prompts, budgets, slots=S, prefill_chunk=C, logprobs=2, prefix_cache=cache)
    same = compare([g[0] for g in got], [w[0] for w in want], logits, prompts, {})
    for (_, g), (_, w), n in zip(got, want, same):
        # (the tolerance of tests/test_logprobs.py between two fp32 paths: ranks exact, values within 1e-4)
        assert np.allclose(g.token[:n], w.token[:n], rtol=0, atol=1e-4)
        assert np.array_equal(g.top_ids[:n], w.top_ids[:n])
        assert np.allclose(g.top_logprobs[:n], w.top_logprobs[:n], rtol=0, atol=1e-4)
    assert m.prefix_stats == simulate(prompts, budgets, S, C, _k(cache))[0] and m.prefix_stats["copies"] > 0


def test_emulated_refusing_library_computes_every_prompt(emulated_hip, monkeypatch):
    """Without the mixed step a prompt completes with one whole pass from position 0: nothing is reused."""
    from pydynet_amd.llm.llama import Llama
    Graph.clear()
    monkeypatch.setattr(Llama, "wide_decode", False)
    prompts, budgets = requests(V, SEED)
    want = _serve_all(_model("hip:0"), prompts, budgets, slots=3, prefill_chunk=4)
    m = _model("hip:0")
    counters()
    got = _serve_all(m, prompts, budgets, slots=3, prefill_chunk=4, prefix_cache=True)
    assert counters()[38] == 0
    assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert m.prefix_stats == simulate(prompts, budgets, 3, 4, None)[0] and m.prefix_stats["reused_tokens"] == 0


def test_stats_during_a_run_and_left_alone_when_off(emulated_hip):
    Graph.clear()
    prompts, budgets = requests(V, SEED)
    m = _model("hip:0")
    m.eval()
    try:
        with pdn.no_grad():
            seen = []
            for _ in m.serve(prompts, budgets, slots=3, prefill_chunk=4, prefix_cache=True):
                seen.append(dict(m.prefix_stats))
            final = dict(m.prefix_stats)
            assert seen[0]["requests"] == 3 and seen[-1] == final and final["reused_tokens"] > 0
            assert all(a[k] <= b[k] for a, b in zip(seen, seen[1:]) for k in prefix.STATS)
            for _ in m.serve(prompts, budgets, slots=3, prefill_chunk=4):
                pass
            assert m.prefix_stats == final                            # the cache off: the attribute is left alone
    finally:
        m.train(True)
        pdn.autograd.set_grad_enabled(True)


# -- off means off -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [{}, SAMPLED[1]])
def test_off_means_off(emulated_hip, kw):
    from pydynet_amd import _lib
    prompts, budgets = requests(V, SEED)

    def run(**extra):
        Graph.clear()
        m = _model("hip:0")
        _lib._LIB.calls.clear()
        counters()
        steps = _eval(m, lambda: [(r.copy(), t.copy()) for r, t in m.serve(prompts, budgets, slots=3, prefill_chunk=4,
                                                                            **kw, **extra)])
        return steps, counters(), [c for c in _lib._LIB.calls if "prefix" in c], m
    base, c0, _, _ = run()
    for off in (False, None):
        steps, c1, calls, m = run(prefix_cache=off)
        assert c1[38] == 0 and c1 == c0 and not calls and not hasattr(m, "prefix_stats")
        assert len(steps) == len(base)
        for (gr, gt), (wr, wt) in zip(steps, base):
            assert np.array_equal(gr, wr) and np.array_equal(gt, wt)
        assert m._decode_st["key"] is not None and "prefix" not in m._decode_st
