"""Sampling parameters per request and min_p (llm/sampling.py, include/pdn_persample.h) without a GPU: the NumPy contract,
the argument checks, and generate_ragged / serve_all with one parameter set per request on the `cpu` device and on the
emulated library (tests/abi_emulator/_persample.py) -- each request's tokens are those of the uniform run with its values."""
import numpy as np
import pytest

from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm import sampling as S
from pydynet_amd.llm.llama import Llama
from tests.abi_emulator import counters, remove
from tests.abi_emulator import _persample
from tests.test_logit_edits import _serve_all
from tests.test_ragged import V, _model, _prompts, _ragged


# ---- the contract --------------------------------------------------------------------------------------------------
def _kept_mask_before(z, top_k, top_p, temperature):
    """`kept_mask` as it stood before min_p (steps 1-3)."""
    Vz = z.shape[0]
    kept = np.ones(Vz, bool)
    if 0 < top_k < Vz:
        kept = z >= np.partition(z, Vz - top_k)[Vz - top_k]
    w = np.where(kept, np.exp((z - z.max()) / temperature), 0.0)
    p = w / w.sum()
    if top_p < 1.0:
        vals, grp = np.unique(z[kept], return_inverse=True)
        cum = np.cumsum(np.bincount(grp.reshape(-1), weights=p[kept], minlength=vals.size)[::-1])
        theta = vals[::-1][min(int(np.searchsorted(cum, top_p, side="left")), vals.size - 1)]
        kept &= z >= theta
        p = np.where(kept, p, 0.0)
        p /= p.sum()
    return kept, p


def _brute(z, top_k, top_p, T, min_p):
    """Steps 1-3b restated with sorts and plain loops in float64."""
    n = len(z)
    kept = np.ones(n, bool)
    if 0 < top_k < n:
        kept = z >= sorted(z.tolist(), reverse=True)[top_k - 1]
    w = np.exp((z - z.max()) / T)
    pr = np.where(kept, w, 0.0) / w[kept].sum()
    if top_p < 1.0:
        for theta in sorted(set(z[kept].tolist()), reverse=True):
            if pr[kept & (z >= theta)].sum() >= top_p:
                break
        kept = kept & (z >= theta)
    if min_p > 0.0:
        kept = kept & np.array([wi >= min_p for wi in w])
    pr = np.where(kept, w, 0.0)
    return kept, pr / pr.sum()


def test_min_p_against_a_brute_force_restatement():
    rng = np.random.default_rng(0)
    hit = 0
    for i in range(200):
        z = np.round(rng.standard_normal(int(rng.integers(2, 90))) * 3, 1)            # (rounded: repeated values)
        T, k = float(rng.uniform(0.3, 2.0)), int(rng.integers(0, 12))
        p, m = (1.0, float(rng.uniform(0.3, 1.0)))[i % 2], (0.0, float(rng.uniform(0.01, 0.9)))[i % 3 > 0]
        kept, pr = S.kept_mask(z, k, p, T, m)
        bk, bp = _brute(z, k, p, T, m)
        assert np.array_equal(kept, bk) and np.allclose(pr, bp, rtol=1e-12, atol=0) and kept[z.argmax()], i
        assert abs(pr.sum() - 1) < 1e-12 and (pr[~kept] == 0).all()
        hit += int(m > 0 and not np.array_equal(kept, S.kept_mask(z, k, p, T)[0]))
    assert hit > 40                                                                   # min_p removed something


def test_min_p_zero_is_the_function_of_before():
    rng = np.random.default_rng(1)
    for i in range(100):
        z = rng.standard_normal((3, int(rng.integers(2, 70)))) * 2
        T, k, p = float(rng.uniform(0.3, 2.0)), int(rng.integers(0, 9)), (1.0, float(rng.uniform(0.2, 1.0)))[i % 2]
        for row in z:
            for got in (S.kept_mask(row, k, p, T), S.kept_mask(row, k, p, T, 0.0), S.kept_mask(row, k, p, T, min_p=0.0)):
                want = _kept_mask_before(row, k, p, T)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        a = S.sample_rows_np(z, i, T, k, p, seed=i)
        assert np.array_equal(a, S.sample_rows_np(z, i, T, k, p, seed=i, min_p=0.0))
    assert np.array_equal(S.params_bytes(0.7, 3, 0.9, 5), S.params_bytes(0.7, 3, 0.9, 5, 0.0))
    assert S.params_bytes(0.7, 3, 0.9, 5).view(np.uint8)[12:16].tolist() == [0, 0, 0, 0]
    assert S.params_bytes(0.7, 3, 0.9, 5, 0.25).view(np.float32)[3] == 0.25


def test_order_top_k_then_top_p_then_min_p():
    """weights 1, 0.5, 0.3, 0.2 (T = 1), top_k = 3, top_p = 0.6, min_p = 0.4: top-k keeps {0, 1, 2}; over those the masses
    are 0.556 / 0.278 / 0.167, so top-p keeps {0, 1}; min_p then removes nothing.  min_p applied before top-p would leave
    {0, 1} with masses 0.667 / 0.333, and top-p would keep {0} alone."""
    z = np.log(np.array([1.0, 0.5, 0.3, 0.2]))
    kept, p = S.kept_mask(z, 3, 0.6, 1.0, 0.4)
    assert kept.tolist() == [True, True, False, False] and np.allclose(p, [2 / 3, 1 / 3, 0, 0])
    assert S.kept_mask(z, 0, 1.0, 1.0, 0.4)[0].tolist() == [True, True, False, False]
    assert S.kept_mask(z[[0, 1]], 0, 0.6, 1.0)[0].tolist() == [True, False]            # the other order's answer
    # after top-k: without it the fourth token (0.2) joins the top-p mass and the nucleus is the same, but min_p = 0.25
    # alone keeps three tokens where top_k = 2 before it keeps two
    assert S.kept_mask(z, 0, 1.0, 1.0, 0.25)[0].sum() == 3 and S.kept_mask(z, 2, 1.0, 1.0, 0.25)[0].sum() == 2
    # the boundary is inclusive and the maximum always stays
    assert S.kept_mask(z, 0, 1.0, 1.0, 0.5)[0].tolist() == [True, True, False, False]
    assert S.kept_mask(z, 0, 1.0, 1.0, 0.999)[0].tolist() == [True, False, False, False]


# ---- the checker ---------------------------------------------------------------------------------------------------
def test_checker_returns_the_scalar_tuple_or_a_table():
    assert S.check_request_args(0.5, 3, 0.9, 7, 0.0, 4) == S.check_args(0.5, 3, 0.9, 7) == (0.5, 3, 0.9, 7)
    assert S.active(S.check_request_args(0.0, 3, 0.9, 7, 0.0, 4)) is None
    t = S.check_request_args(0.5, 3, 0.9, 7, 0.25, 4)                  # min_p alone makes it a table
    assert isinstance(t, S.Table) and t.n == 4 and t.row(3) == (0.5, 3, float(np.float32(0.9)), 7, 0.25) and S.active(t) is t
    t = S.check_request_args([0.0, 1.5, 0.0], 2, (1.0, 0.5, 1.0), np.array([1, 2 ** 64 - 1, 3], np.uint64), 0.0, 3)
    assert t.row(1) == (1.5, 2, 0.5, 2 ** 64 - 1, 0.0) and t.row(2) == (0.0, 2, 1.0, 3, 0.0) and S.active(t) is t
    assert t.blocks([1, -1]).shape == (2, 3) and np.array_equal(t.blocks([1])[0], S.params_bytes(1.5, 2, 0.5, 2 ** 64 - 1))
    assert np.array_equal(t.blocks([-1])[0], t.blocks([0])[0])
    assert S.active(S.check_request_args([0.0, 0.0], 0, 1.0, [1, 2], 0.5, 2)) is None   # every temperature 0: greedy


BAD = [(dict(temperature=[1.0, 2.0]), "temperature: 2 values for 3 requests"),
       (dict(seed=[1, 2, 3, 4]), "seed: 4 values for 3 requests"),
       (dict(temperature=[1.0, -0.5, 1.0]), "request 1: temperature"),
       (dict(top_k=[0, 1, 2.5]), "request 2: top_k"),
       (dict(top_p=[0.0, 1.0, 1.0]), "request 0: top_p"),
       (dict(seed=[0, 1, -1]), "request 2: seed"),
       (dict(min_p=[0.0, 1.0, 0.0]), "request 1: min_p"),
       (dict(min_p=-0.1), "min_p"), (dict(min_p=1.0), "min_p"), (dict(min_p=float("nan")), "min_p")]


@pytest.mark.parametrize("bad,msg", BAD)
def test_bad_arguments_raise(bad, msg):
    with pytest.raises(ValueError, match=msg):
        S.check_request_args(**dict(dict(temperature=1.0, top_k=0, top_p=1.0, seed=0, min_p=0.0, n=3), **bad))
    m = _model("cpu")
    prompts = _prompts([2, 3, 1], seed=2)
    with pytest.raises(ValueError, match=msg):
        m.serve(prompts, 4, **bad)
    with pytest.raises(ValueError, match=msg.replace("request", "row")):
        m.generate_ragged(prompts, 4, **bad)


# ---- the mixed batch -----------------------------------------------------------------------------------------------
# request: 0 greedy, 1 T = 0.8, 2 top_k = 5, 3 top_p = 0.9, 4 min_p = 0.1, 5 another seed
MIX = dict(temperature=[0.0, 0.8, 1.0, 1.0, 1.0, 1.0], top_k=[0, 0, 5, 0, 0, 0], top_p=[1.0, 1.0, 1.0, 0.9, 1.0, 1.0],
           min_p=[0.0, 0.0, 0.0, 0.0, 0.1, 0.0], seed=[3, 3, 3, 3, 3, 11])
LENS, BUDGETS = [3, 1, 6, 2, 4, 5], [6, 9, 4, 8, 7, 9]


def _mix(N):
    """The mix for N requests (request r takes the values of r % 6) and its value set per request."""
    kw = {k: [v[r % 6] for r in range(N)] for k, v in MIX.items()}
    return kw, [{k: v[r] for k, v in kw.items()} for r in range(N)]


_uniform = {}


def _want(N, dev="cpu"):
    """Row r of the uniform generate_ragged run with request r's values for every row, cut to its budget."""
    if (N, dev) not in _uniform:
        prompts = _prompts([LENS[r % 6] + r // 6 for r in range(N)], seed=21)
        budgets = [BUDGETS[r % 6] for r in range(N)]
        rows = []
        for r, one in enumerate(_mix(N)[1]):
            full = _ragged(_model(dev, B=N), prompts, max(budgets), **one)
            rows.append(full[r, :budgets[r]].tolist())
        _uniform[(N, dev)] = (prompts, budgets, rows)
    return _uniform[(N, dev)]


def test_cpu_mixed_batch_is_the_uniform_runs():
    prompts, budgets, want = _want(6)
    kw = _mix(6)[0]
    assert len({tuple(w[:4]) for w in want}) > 3                        # the value sets do differ in what they yield
    got = _ragged(_model("cpu", B=6), prompts, max(budgets), **kw)
    assert [g[:b].tolist() for g, b in zip(got, budgets)] == want
    for chunk in (None, 4):
        got = _serve_all(_model("cpu", B=6), prompts, budgets, slots=2, prefill_chunk=chunk, **kw)
        assert [g.tolist() for g in got] == want
    got = _ragged(_model("cpu", B=6), prompts, max(budgets), speculate=2, **kw)
    assert [g[:b].tolist() for g, b in zip(got, budgets)] == want
    # scalars and sequences mixed; one value = that value for every request
    one = dict(temperature=[0.0, 0.8, 1.0, 1.0, 1.0, 1.0], seed=3, min_p=0.1, top_k=5)
    full = dict(one, seed=[3] * 6, min_p=[0.1] * 6, top_k=[5] * 6)
    assert np.array_equal(_ragged(_model("cpu", B=6), prompts, 5, **one), _ragged(_model("cpu", B=6), prompts, 5, **full))


@pytest.mark.parametrize("graphs", [True, False])
@pytest.mark.parametrize("S_,chunk", [(2, None), (2, 4), (10, None)])
def test_emulated_serve_all_mixed_batch(emulated_hip, graphs, S_, chunk, monkeypatch):
    _persample.extend()
    monkeypatch.setattr(Llama, "graph_decode", graphs)
    Graph.clear()
    N = 6 if S_ == 2 else 13
    prompts, budgets, want = _want(N)
    counters(50)
    m = _model("hip:0", B=N)
    got = _serve_all(m, prompts, budgets, slots=S_, prefill_chunk=chunk, **_mix(N)[0])
    c = counters(50)
    assert [g.tolist() for g in got] == want
    st = m._decode_st
    assert st["ok"] and st["per_row"] and st["key"][-1] == "per_row" and st["params"].shape == (S_, 3) and c[49] > 0
    assert c[28] == c[49] and (c[31] > 0) == (S_ > 8 or chunk is not None)


@pytest.mark.parametrize("how", ["graph", "nograph", "speculate", "wide", "generic", "module"])
def test_emulated_generate_ragged_mixed_batch(emulated_hip, how, monkeypatch):
    if how != "generic":
        _persample.extend()
    monkeypatch.setattr(Llama, "graph_decode", how != "nograph")
    if how == "module":
        monkeypatch.setattr(Llama, "fast_decode", False)
    Graph.clear()
    N = 13 if how == "wide" else 6
    prompts, budgets, want = _want(N)
    counters(50)
    m = _model("hip:0", B=N)
    got = _ragged(m, prompts, max(budgets), speculate=2 if how == "speculate" else 0, **_mix(N)[0])
    c = counters(50)
    assert [g[:b].tolist() for g, b in zip(got, budgets)] == want
    if how in ("graph", "nograph", "wide"):
        st = m._decode_st
        assert st["per_row"] and st["params"].shape == (N, 3) and c[49] == max(budgets) and (c[31] > 0) == (how == "wide")
        assert np.array_equal(st["params"].get(), S.Table(**_mix(N)[0]).blocks(np.arange(N)))
    elif how == "speculate":
        assert m._spec_st["per_row"] and m._spec_st["key"][-1] == "per_row" and c[49] > 1 and c[34] > 0
    elif how == "module":
        assert c[49] == max(budgets) and c[29] == 0        # every draw through the standalone entry
    else:
        assert c[49] == 0 and c[29] > 0                    # the statement row by row: no entry to call


def test_emulated_uniform_runs_on_the_device_too(emulated_hip):
    """The reference side of the promise through the emulated library as well: the uniform runs with request r's values."""
    _persample.extend()
    Graph.clear()
    assert _want(6, "hip:0")[2] == _want(6)[2]


def test_emulator_and_cpu_agree_without_the_entries(emulated_hip, monkeypatch):
    """A library without the pdnq_ entries (the emulator not extended), or with one removed: the plans refuse, every draw
    is the statement row by row, tokens as on `cpu`."""
    from pydynet_amd import _lib
    prompts, budgets, want = _want(6)
    kw = _mix(6)[0]
    for extended in (False, True):
        Graph.clear()
        if extended:
            _persample.extend()
            remove(monkeypatch, _lib._LIB, "pdnq_decode_sample_tick_slots_f32")
        assert not _lib.provides("pdnq_decode_sample_tick_slots_f32")
        counters(50)
        m = _model("hip:0", B=6)
        got = _ragged(m, prompts, max(budgets), **kw)
        assert [g[:b].tolist() for g, b in zip(got, budgets)] == want and m._decode_st["ok"] is False
        for chunk in (None, 4):
            got = _serve_all(_model("hip:0", B=6), prompts, budgets, slots=2, prefill_chunk=chunk, **kw)
            assert [g.tolist() for g in got] == want
        got = _ragged(_model("hip:0", B=6), prompts, max(budgets), speculate=2, **kw)
        assert [g[:b].tolist() for g, b in zip(got, budgets)] == want
        c = counters(50)
        assert c[29] > 0 and (c[49] > 0) == extended      # (extended: the standalone entry still draws the rows)


def test_with_penalties_logprobs_and_edits(emulated_hip):
    """The table beside one penalty set, logprobs = 2 and a logit bias: tokens and records as on `cpu`."""
    from tests.abi_emulator import _logitedit
    from tests.test_logit_edits import _with_lp
    _logitedit.extend()
    _persample.extend()
    Graph.clear()
    prompts, budgets, _ = _want(6)
    kw = dict(_mix(6)[0], repetition_penalty=1.3, presence_penalty=0.4, logprobs=2, logit_bias={7: 2.0, 9: -np.inf})
    mc, mh = _model("cpu", B=6), _model("hip:0", B=6)
    want = _with_lp(mc, mc.generate_ragged(prompts, 7, **kw))
    got = _with_lp(mh, mh.generate_ragged(prompts, 7, **kw))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]) and 9 not in got[0]
    assert np.allclose(got[1], want[1], rtol=1e-5, atol=1e-4) and mh._decode_st["per_row"] and mh._decode_st["pen"]
    want = _serve_all(_model("cpu", B=6), prompts, budgets, slots=2, **kw)
    got = _serve_all(_model("hip:0", B=6), prompts, budgets, slots=2, **kw)
    for (gt, gl), (wt, wl) in zip(got, want):
        assert np.array_equal(gt, wt) and np.array_equal(gl.top_ids, wl.top_ids)


# ---- the defaults --------------------------------------------------------------------------------------------------
def test_scalar_calls_keep_plan_key_launches_and_counters(emulated_hip):
    """With one value per argument and min_p = 0 a run is the one of before: the plan key has no new term, no pdnq_ entry
    is called, and every launch counter equals that of the call without the new keyword."""
    from pydynet_amd import _lib
    _persample.extend()
    Graph.clear()
    runtime = ("pdn_malloc", "pdn_free", "pdn_set_device", "pdn_compute_stream", "pdn_fill", "pdn_kernel_counters",
               "pdn_memcpy")                                   # (allocator / setup traffic differs between first uses)

    def run(fn):
        _lib._LIB.calls.clear()
        counters(50)
        out = fn()
        return out, counters(50), [c for c in _lib._LIB.calls if not c.startswith(runtime)]
    prompts = _prompts([3, 5, 2], seed=11)
    for kw in ({}, dict(temperature=0.8, top_k=5, top_p=0.9, seed=4)):
        m0, m1 = _model("hip:0"), _model("hip:0")
        base, c0, calls0 = run(lambda: _ragged(m0, prompts, 6, stop_ids=[5], **kw))
        again, c1, calls1 = run(lambda: _ragged(m1, prompts, 6, stop_ids=[5], min_p=0.0, **kw))
        assert np.array_equal(base, again) and c0 == c1 and calls0 == calls1 and c0[49] == 0
        assert not any(c.startswith("pdnq_") for c in calls0 + calls1)
        k0, k1 = m0._decode_st["key"], m1._decode_st["key"]
        assert len(k0) == len(k1) and "per_row" not in k1 and m1._decode_st["per_row"] is False
        assert m1._decode_st["params"] is None or m1._decode_st["params"].shape == (3,)
        for chunk in (None, 2):
            base, c0, calls0 = run(lambda: [o.tolist() for o in _serve_all(m0, prompts, 5, slots=2, prefill_chunk=chunk, **kw)])
            again, c1, calls1 = run(lambda: [o.tolist() for o in _serve_all(m1, prompts, 5, slots=2, prefill_chunk=chunk,
                                                                             min_p=0.0, **kw)])
            assert base == again and c0 == c1 and calls0 == calls1 and c0[49] == 0
            assert "per_row" not in m1._decode_st["key"]
        base, c0, calls0 = run(lambda: _ragged(m0, prompts, 6, speculate=2, **kw))
        again, c1, calls1 = run(lambda: _ragged(m1, prompts, 6, speculate=2, min_p=0.0, **kw))
        assert np.array_equal(base, again) and c0 == c1 and calls0 == calls1 and "per_row" not in m1._spec_st["key"]
    # with a table the key grows by one term, the last
    _ragged(m1, prompts, 6, temperature=[0.5, 0.0, 1.0])
    assert m1._decode_st["key"][-1] == "per_row" and len(m1._decode_st["key"]) == len(k0) + 1
    # a scalar call computes what the one-value-per-request call computes
    a = _ragged(_model("hip:0"), prompts, 6, temperature=0.8, top_k=5, top_p=0.9, seed=4)
    b = _ragged(_model("hip:0"), prompts, 6, temperature=[0.8] * 3, top_k=[5] * 3, top_p=[0.9] * 3, seed=[4] * 3)
    assert np.array_equal(a, b)
