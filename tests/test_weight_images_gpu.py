"""All weight plane images of a pass in one launch (include/pdn_wimages.h, csrc/weight_images.hip): a product that takes its
image from a bound set gives the BITS it gives when it builds the image itself, at the routes' smallest shapes -- 16384 rows
for the three projection forms (q | k | v with 3 x 288 columns and head dim 48, gate | up with F = 96 and dh + SwiGLU backward with F = 192,
the narrowest the entries take at that row count), 65536 rows for the output-resident forms (K = 288 NN and NT, K = 768 NN, 3 x 288 NT
blocks).  Every comparison is np.array_equal on the uint32 view; pdnw_stats counts set launches, images taken from a set and
per-call passes.  The graph-level cases run two layers at 65536 tokens with PDN_WIMAGES on and off."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 288
M_RTS, M_ORS = 16384, 65536
F, D, HD, LQ = 96, 288, 48, 256
FD = 192                                  # dh + SwiGLU backward: three tiles would leave the 8-wave kernel short of a full chip
EPS = 1e-6
FORMS = ["qkv", "gateup", "down_t", "nn288", "nt288", "nn768", "ntblocks"]
_CACHE = {}


def _lib_hp():
    from pydynet_amd import _lib, hipnp
    return _lib.lib(), hipnp


def _stats(L, reset=True):
    b, h, p = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    L.call("pdnw_stats", ctypes.byref(b), ctypes.byref(h), ctypes.byref(p), 1 if reset else 0)
    return b.value, h.value, p.value


class _env:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.get(self.name)
        os.environ[self.name] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ[self.name]
        else:
            os.environ[self.name] = self.old


def _shared():
    """the row operands, made once: 2048 random rows tiled (their values do not matter to the comparison, their size does)"""
    if "shared" not in _CACHE:
        L, hp = _lib_hp()
        rng = np.random.default_rng(18)
        x = np.tile(rng.standard_normal((2048, K), dtype=np.float32), (M_RTS // 2048, 1))
        a = np.tile(rng.standard_normal((2048, 864), dtype=np.float32), (M_ORS // 2048, 1))
        gu = np.tile(rng.standard_normal((2048, 2 * FD), dtype=np.float32), (M_RTS // 2048, 1))
        cos = np.cos(np.outer(np.arange(LQ), 1.0 / 10000 ** (np.arange(0, HD, 2) / HD))).astype(np.float32)
        sin = np.sin(np.outer(np.arange(LQ), 1.0 / 10000 ** (np.arange(0, HD, 2) / HD))).astype(np.float32)
        tab = hp.empty((LQ, HD, 2), np.float32)
        L.call("pdn_rope_table_f32", hp.from_numpy(cos)._ptr, hp.from_numpy(sin)._ptr, tab._ptr, LQ, HD, hp.stream())
        _CACHE["shared"] = dict(x=hp.from_numpy(x), a=hp.from_numpy(a), gu=hp.from_numpy(gu), tab=tab,
                                nw=hp.from_numpy((1 + 0.1 * rng.standard_normal(K)).astype(np.float32)),
                                res=hp.from_numpy(np.tile(rng.standard_normal((2048, D), dtype=np.float32), (M_ORS // 2048, 1))))
    return _CACHE["shared"]


def _special(w, axis):
    """a zero column, a 1e-30 column, a column holding Inf and one holding NaN (column = what gets one exponent)"""
    w = np.moveaxis(w, axis, -1)
    w[..., 3] = 0.0
    w[..., 40] *= np.float32(1e-30)
    w[..., 5, 70] = np.inf
    w[..., 9, 77] = np.nan
    return np.moveaxis(w, -1, axis)


class _Product:
    """one product: its weight on the device, the constructor call of its descriptor, and a run that returns its outputs"""

    def __init__(self, form, seed=0, special=False, layout=False):
        L, hp = _lib_hp()
        self.L, self.hp, self.form = L, hp, form
        s = _shared()
        rng = np.random.default_rng(1000 + seed + 17 * FORMS.index(form))
        pad = 64 if layout else 0                        # blocks further apart than they are large
        ldx = 320 if layout else K                       # rows further apart than they are wide
        if form == "qkv":
            w = (rng.standard_normal((3, K, D), dtype=np.float32) * 0.06).astype(np.float32)
            if special:
                w = _special(w, 2)
            buf = np.zeros((3, K * D + pad), np.float32)
            buf[:, :K * D] = w.reshape(3, -1)
            self.wd = hp.from_numpy(buf)
            stride = K * D + pad
            self.ctor = ("pdnw_desc_qkv", (self.wd._ptr, stride, D, K))

            def run():
                qkv, rms = hp.empty((M_RTS, 3 * D), np.float32), hp.empty((M_RTS,), np.float32)
                L.call("pdnp_qkv_rope_norm_fwd_f32", s["x"]._ptr, s["nw"]._ptr, EPS, rms._ptr, self.wd._ptr, stride, qkv._ptr,
                       s["tab"]._ptr, M_RTS, D, K, LQ, HD, K, hp.stream())
                return qkv, rms
        elif form == "gateup":
            w = (rng.standard_normal((2, K, F), dtype=np.float32) * 0.06).astype(np.float32)
            if special:
                w = _special(w, 2)
            buf = np.zeros((2, K * F + pad), np.float32)
            # layout: the up matrix BELOW the gate matrix (a negative stride)
            buf[:, :K * F] = w.reshape(2, -1)[::-1] if layout else w.reshape(2, -1)
            self.wd = hp.from_numpy(buf)
            stride = -(K * F + pad) if layout else K * F + pad
            gate_ptr = self.wd._ptr + (4 * (K * F + pad) if layout else 0)
            self.ctor = ("pdnw_desc_gateup", (gate_ptr, stride, F, K))

            def run():
                gu, h, rms = hp.empty((M_RTS, 2 * F), np.float32), hp.empty((M_RTS, F), np.float32), hp.empty((M_RTS,), np.float32)
                L.call("pdnp_gateup_swiglu_norm_fwd_f32", s["x"]._ptr, s["nw"]._ptr, EPS, rms._ptr, gate_ptr, stride, gu._ptr,
                       h._ptr, M_RTS, F, K, K, hp.stream())
                return gu, h, rms
        elif form == "down_t":
            w = (rng.standard_normal((FD, K), dtype=np.float32) * 0.06).astype(np.float32)
            if special:
                w = _special(w, 0)
            self.wd = hp.from_numpy(w)
            self.ctor = ("pdnw_desc_down_t", (self.wd._ptr, FD, K))

            def run():
                dgu = hp.empty((M_RTS, 2 * FD), np.float32)
                L.call("pdn_swiglu_bwd_gemm_f32", s["x"]._ptr, self.wd._ptr, s["gu"]._ptr, dgu._ptr, M_RTS, FD, K, K, hp.stream())
                return (dgu,)
        elif form in ("nn288", "nn768"):
            kk = 288 if form == "nn288" else 768
            ldb = ldx if form == "nn288" else D
            w = np.zeros((kk, ldb), np.float32)
            w[:, :D] = _special(rng.standard_normal((kk, D), dtype=np.float32), 1) if special else rng.standard_normal((kk, D), dtype=np.float32)
            self.wd, self.ldb, self.kk = hp.from_numpy(w), ldb, kk
            self.ctor = ("pdnw_desc_outres", (self.wd._ptr, kk, ldb, 0, 0, 0))

            def run(ldb_call=None, w_call=None):
                c = hp.empty((M_ORS, D), np.float32)
                L.call("pdn_gemm_outres_f32", s["a"]._ptr, (self.wd if w_call is None else w_call)._ptr, c._ptr, None, s["res"]._ptr, M_ORS, D, kk, 864,
                       ldb_call or ldb, D, 0, hp.stream())
                return (c,)
        elif form == "nt288":
            w = np.zeros((D, ldx), np.float32)
            w[:, :K] = _special(rng.standard_normal((D, K), dtype=np.float32), 0) if special else rng.standard_normal((D, K), dtype=np.float32)
            self.wd = hp.from_numpy(w)
            self.ctor = ("pdnw_desc_outres", (self.wd._ptr, K, ldx, 1, 0, 0))

            def run():
                c = hp.empty((M_ORS, D), np.float32)
                L.call("pdn_gemm_outres_f32", s["a"]._ptr, self.wd._ptr, c._ptr, None, None, M_ORS, D, K, 864, ldx, D, 1, hp.stream())
                return (c,)
        else:
            assert form == "ntblocks"
            w = rng.standard_normal((3, D, 288), dtype=np.float32)
            if special:
                w = _special(w, 1)
            buf = np.zeros((3, D * 288 + pad), np.float32)
            buf[:, :D * 288] = w.reshape(3, -1)
            self.wd = hp.from_numpy(buf)
            stride = D * 288 + pad
            self.ctor = ("pdnw_desc_outres", (self.wd._ptr, 864, 288, 1, 288, stride))

            def run():
                c = hp.empty((M_ORS, D), np.float32)
                L.call("pdn_gemm_outres_blocks_nt_f32", s["a"]._ptr, self.wd._ptr, stride, 288, 3, c._ptr, None, M_ORS, 864, D, hp.stream())
                return (c,)
        self.run = run

    def bits(self, *args, **kw):
        return [o.get().view(np.uint32) for o in self.run(*args, **kw)]


class _Set:
    """descriptor records filled by the constructors, the arena, one build; `with` binds it on a stream"""

    def __init__(self, ctors, stream=None):
        L, hp = _lib_hp()
        self.L, self.n = L, len(ctors)
        nb = L.query("pdnw_desc_bytes")
        self.recs = ctypes.create_string_buffer(nb * self.n)
        for i, (name, args) in enumerate(ctors):
            L.call(name, ctypes.addressof(self.recs) + i * nb, *args)
        self.nbytes = L.query("pdnw_set_bytes", self.recs, self.n)
        assert self.nbytes > 0 and self.nbytes % 256 == 0
        self.arena = hp.empty((self.nbytes // 4 + 64,), np.float32)
        self.arena[self.nbytes // 4:] = 7.5                   # canary behind the set
        self.stream = hp.stream() if stream is None else stream
        L.call("pdnw_set_build", self.recs, self.n, self.arena._ptr, hp.stream())

    def canary_ok(self):
        return bool((self.arena[self.nbytes // 4:].get() == 7.5).all())

    def __enter__(self):
        self.L.call("pdnw_bind", self.recs, self.n, self.arena._ptr, self.stream)
        return self

    def __exit__(self, *exc):
        self.L.call("pdnw_unbind")


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _bound_equals_unbound(p):
    L = p.L
    _stats(L)
    ref = p.bits()
    assert _stats(L) == (0, 0, 1)                              # a pass of its own
    st = _Set([p.ctor])
    with st:
        got = p.bits()
    assert _stats(L) == (1, 1, 0) and st.canary_ok()           # one launch built it, the product took it, no pass
    assert _same(ref, got)
    return ref


@pytest.mark.parametrize("form", FORMS)
def test_bound_set_gives_the_bits_of_the_per_call_pass(form):
    _bound_equals_unbound(_Product(form))


@pytest.mark.parametrize("form", FORMS)
def test_special_columns(form):
    """a zero column, a 1e-30 column, a column holding Inf and one holding NaN"""
    ref = _bound_equals_unbound(_Product(form, special=True))
    assert not np.isfinite(ref[0].view(np.float32)).all()      # (the Inf / NaN columns reached the product)


@pytest.mark.parametrize("form", ["qkv", "gateup", "nn288", "nt288", "ntblocks"])
def test_weight_layouts(form):
    """blocks as separate, equally spaced allocations (64 floats further apart than they are large; gate | up with the up
    matrix below the gate matrix), weights with ldb larger than their width"""
    _bound_equals_unbound(_Product(form, layout=True))


def test_one_launch_builds_all_forms_of_several_weights():
    L, hp = _lib_hp()
    prods = [_Product(f, seed=r) for r in range(2) for f in FORMS]
    _stats(L)
    refs = [p.bits() for p in prods]
    assert _stats(L) == (0, 0, len(prods))
    st = _Set([p.ctor for p in prods])
    with st:
        got = [p.bits() for p in prods]
    assert _stats(L) == (1, len(prods), 0) and st.canary_ok()
    assert all(_same(r, g) for r, g in zip(refs, got))


def test_misses_run_the_per_call_pass():
    L, hp = _lib_hp()
    p, other = _Product("nn288", layout=True), _Product("nn288", seed=5, layout=True)      # (ldb 320: room for another ldb)
    st = _Set([p.ctor])
    _stats(L)
    ref_other, ref_ldb = other.bits(), p.bits(ldb_call=304)
    ref = p.bits()
    assert _stats(L) == (0, 0, 3)
    with st:
        assert _same(ref_other, p.bits(w_call=other.wd)) and _stats(L) == (0, 0, 1)         # a weight not in the set
        assert _same(ref_ldb, p.bits(ldb_call=304)) and _stats(L) == (0, 0, 1)             # a different ldb
        assert _same(ref, p.bits()) and _stats(L) == (0, 1, 0)                             # (the set does serve its own)
    side = ctypes.c_void_p()
    L.call("pdn_stream_create", ctypes.byref(side), 0)
    try:
        st.stream = side.value
        with st:                                                                            # bound on another stream
            assert _same(ref, p.bits()) and _stats(L) == (0, 0, 1)
    finally:
        st.stream = hp.stream()
        hp.synchronize()
        L.call("pdn_stream_destroy", side.value)
    with _env("PDN_WIMAGES", "0"):                                                          # switched off in process
        with st:
            assert _same(ref, p.bits()) and _stats(L) == (0, 0, 1)
    with st:
        assert _same(ref, p.bits()) and _stats(L) == (0, 1, 0)
    assert _same(ref, p.bits()) and _stats(L) == (0, 0, 1)                                  # unbound again


# ---- graph level --------------------------------------------------------------------------------------------------------
def _graph_run(on):
    """two layers at 65536 tokens: a step; then a weight scaled in place, a forward, ANOTHER weight scaled in place between
    that forward and its backward, the backward.  -> bits of both losses and of every gradient, and the counts per pass"""
    from pydynet_amd.llm.llama import Llama
    from pydynet_amd.optim import Adam
    L, hp = _lib_hp()
    B, Lq = 256, 256
    rng = np.random.default_rng(3)
    ids, tgt = rng.integers(0, 512, (B, Lq)), rng.integers(0, 512, (B, Lq))
    with _env("PDN_WIMAGES", "1" if on else "0"):
        np.random.seed(0)
        model = Llama(512, 288, 6, 768, Lq, B, 2, np.float32)
        model.tok_embedding.weight.data[...] = (0.02 * rng.standard_normal((512, 288))).astype(np.float32)
        model.to("hip:0")
        opt = Adam(model.parameters(), lr=0.0)
        opt.flatten_grads()                                   # equally spaced gradients: the stacked products
        out, counts = [], []

        def grads():
            return {n: q.grad.get().view(np.uint32) for n, q in model.named_parameters() if q.requires_grad}

        _stats(L)
        loss = model.loss(ids, tgt)
        counts.append(_stats(L))
        loss.backward()
        counts.append(_stats(L))
        out.append((loss.numpy().view(np.uint32), grads()))
        opt.zero_grad()
        wq, wd = model.layers[0].attention.Q.weight, model.layers[1].ffn.down.weight
        wq.data[...] = wq.data * np.float32(1.5)              # between two loss() calls
        loss = model.loss(ids, tgt)
        counts.append(_stats(L))
        wd.data[...] = wd.data * np.float32(0.5)              # between the forward and its backward
        loss.backward()
        counts.append(_stats(L))
        out.append((loss.numpy().view(np.uint32), grads()))
    return out, counts


def test_graph_level_on_and_off(hip):
    on, con = _graph_run(True)
    off, coff = _graph_run(False)
    # one build per pass, eight images taken per layer and step (four per pass), no per-call pass
    assert con == [(1, 8, 0)] * 4, con
    assert all(c[0] == 0 and c[1] == 0 and c[2] == 8 for c in coff), coff
    for step in range(2):
        assert np.array_equal(on[step][0], off[step][0]), ("loss", step)
        assert on[step][1].keys() == off[step][1].keys() and len(on[step][1]) > 10
        for name in off[step][1]:
            assert np.array_equal(on[step][1][name], off[step][1][name]), (name, step)
    assert not np.array_equal(on[0][0], on[1][0])             # (the scaled weight was seen)
