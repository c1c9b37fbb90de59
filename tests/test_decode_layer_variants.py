"""The other half of the graph-replayed decode step, at every route: decode_attention_kernel<KPRE, VPRE, OPROJ, ROWS> behind the
four pdn_decode_attention*_f32 entries (csrc/decode.hip), decode_block_kernel<F4, VPRE, QP, PW, EXACT, ROWS> behind
pdn_decode_block_f32 / pdn_decode_block_rows_f32 (csrc/decode_block.hip), decode_mlp_kernel<NB, PD, EXACT> behind
pdn_decode_mlp_f32 (csrc/decode_layer.hip) and the chunked-prefill pair pdn_kv_append_rows_f32 /
pdn_decode_extend_attention_f32 (csrc/extend.hip) -- each against the plain float64 NumPy statement of the operation in
tests/decode_layer_ref.py (nothing there calls this package or the emulator).  The conventions are those of
tests/test_decode_step_variants.py:

  * every check is a `check_*(dev)` registered through `device_variants`: on the MI355X under `-m gpu`, on the NumPy emulation
    of the C ABI otherwise;
  * every output buffer starts as NaN and is larger than what may be written, every stride is wider than its row
    (qkv_row_stride > 3 D, cache_batch_stride > max_len D, wo_row_stride > D, ...): the padding and the rows past B must come
    back NaN, the inputs bit-identical; the cache rows at and above a row's position start as NaN: only the appended row may
    change, and no NaN may reach a result.

EXACT cases hold under `np.array_equal` -- operands for which every fp32 stage is exact in any order:
  count     cached K and the new k are zero, V integers in [-3, 3]: every score 0, every probability 1, l the number of keys
            of the range, the sums integers.  A dropped, doubled or out-of-range key row, a wrong range boundary, a stale
            LDS slot added to a sum.
  select    RoPE tables of quarter turns ((1, 0), (0, 1), (-1, 0), (0, -1), varied by position and pair), q = 32 e_j in one
            pair j per head; ONE key t* is 0 along the rotated q, every other key has a scaled score <= -1024 (expf and the
            float64 exp both return exactly 0): in t*'s range m = 0, l = 1, sums = V[t*]; in every other range all scores
            are equal: probabilities 1 (m there is one fp32 product and is held to 1e-6, everything else to equality).  Every
            key also carries +-LARGE across the rotated q: a q turned by the wrong table row or pair meets a positive
            score.  A key paired with another key's value, a wrong per-wave rescale, a wrong table row / pair index; the
            appended cache row (integers turned by quarter turns) is bit-exact.
FLOAT cases: standard-normal operands, the criterion of tests/test_decode_layer_gpu.py, max |got - ref| / max |ref| < 1e-5,
separately for m, l, the sums and the merged normalised row.  That constant is established up to ~400 keys per range; a case
with more first measures the error against float64 of a plain fp32 NumPy evaluation of the same sums and is held to
max(1e-5, 4 x that) (the factor: another summation order).  Every figure is printed (an MI355X run with the plain-fp32 figures:
profiles/decode_layer_variants_gpu_tests.txt).

Found by this file (HISTORY.md 4.10): decode_attention_kernel's 8-way combine of the PV partial sums filled only the first
256 of its 8 f4 slots; above head_dim 128 the final pass added slots nobody wrote (check_attention_head_dims_above_128).
decode_mlp_kernel's k-slices without a row re-read row `slice` of Wg / Wu, which lies behind the matrix when D < 16
(check_mlp_d4, check_mlp_d12)."""
import functools
from types import SimpleNamespace as NS_

import numpy as np
import pytest

from tests import decode_layer_ref as ref
from tests.conftest import device_variants

F32, F64 = np.float32, np.float64
EINVAL, EUNSUPPORTED = -1, -2
FLOAT_KEYS = 400                 # keys per range up to which max-norm 1e-5 is established (tests/test_decode_layer_gpu.py)


def _env(dev):
    from pydynet_amd import hipnp as hp, _lib
    from pydynet_amd.cuda import Device
    return hp, _lib.lib(), Device(dev)


def _ints(rng, shape, lo=-3, hi=3):
    return rng.integers(lo, hi + 1, shape).astype(F32)


def _err(got, want):
    return float(np.abs(np.asarray(got, F64) - want).max() / max(np.abs(want).max(), 1e-30))


def _rel(got, want, what, bound=1e-5):
    """The criterion of tests/test_decode_layer_gpu.py; the figure is printed before it is held to the bound."""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.isfinite(got).all(), (what, "not finite", int((~np.isfinite(got)).sum()), "of", got.size)
    err = _err(got, want)
    _FIGURES.append(f"{' '.join(str(w) for w in what[-2:]) if isinstance(what[-1], int) else what[-1]} {err:.2e}" +
                    ("" if bound == 1e-5 else f" (bound {bound:.2e})"))
    assert err < bound, (what, err, bound, "measured so far: " + ", ".join(_FIGURES))


_FIGURES = []


def _report(what, show=True):
    """One line per case with every figure `_rel` measured for it (all held to 1e-5 unless a bound is named)."""
    if show and _FIGURES:
        print(f"[decode_layer_variants] {' '.join(str(w) for w in what)}: " + ", ".join(_FIGURES))
    del _FIGURES[:]


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(~(np.asarray(got, F64) == np.asarray(want, F64)))
        i = tuple(bad[0])
        raise AssertionError((what, "elements off", len(bad), "of", got.size, "first at", tuple(int(j) for j in i),
                              float(got[i]), float(want[i])))


def _bits(a, b, what):
    """Bit-identical, NaN included."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and a.itemsize == 4, (what, a.shape, b.shape, a.dtype, b.dtype)
    bad = np.flatnonzero(a.reshape(-1).view(np.uint32) != b.reshape(-1).view(np.uint32))
    if len(bad):
        i = int(bad[0])
        raise AssertionError((what, "changed", len(bad), "of", a.size, "first at", i, a.reshape(-1)[i], b.reshape(-1)[i]))


def _padded(hp, rows, stride, extra=4):
    """rows (B, w) in a NaN-filled buffer with `stride` floats between rows and `extra` more NaN behind it: the device
    buffer and the host image it was made from."""
    B, w = rows.shape
    host = np.full(B * stride + extra, np.nan, F32)
    host[:B * stride].reshape(B, stride)[:, :w] = rows
    return hp.from_numpy(host), host


def _quarter_tables(rng, max_len, half):
    turn = rng.integers(0, 4, (max_len, half))
    return np.array([1, 0, -1, 0], F32)[turn], np.array([0, 1, 0, -1], F32)[turn]


def _angle_tables(rng, max_len, half):
    ang = rng.uniform(0, 6.28, (max_len, half))
    return np.cos(ang).astype(F32), np.sin(ang).astype(F32)


# =====================================================================================================================
# 1. the four pdn_decode_attention*_f32 entries
# =====================================================================================================================
Q_SCALE = 32.0


def _far(hd):
    """|k| along the rotated q of every key but t*: the scaled score -32 * far / sqrt(hd) is <= -1024."""
    return 32.0 * float(np.ceil(np.sqrt(hd)))


def _selector_rows(rng, cos_p, sin_p, H, hd, n, star):
    """(n, H, hd) ROTATED key rows for a query at a position with table rows cos_p / sin_p, and the raw q (H, hd): head h
    has q = 32 e_(2 j) in pair j = (3 h + 1) % half; key `star` (None: no such key among these) is 0 along the rotated q,
    every other key -far along it; every key +-far across it; integers elsewhere."""
    half = hd // 2
    q = np.zeros((H, hd), F32)
    k = _ints(rng, (n, H, hd))
    for h in range(H):
        j = (3 * h + 1) % half
        q[h, 2 * j] = Q_SCALE
        u = np.array([cos_p[j], sin_p[j]], F32)                     # the rotated e_0 of pair j: one of +-e_0, +-e_1
        v = np.array([-sin_p[j], cos_p[j]], F32)                    # ... and the direction across it
        along = np.full(n, -_far(hd), F32)
        if star is not None:
            along[star] = 0.0
        across = _far(hd) * rng.choice([-1.0, 1.0], n).astype(F32)
        k[:, h, 2 * j:2 * j + 2] = along[:, None] * u + across[:, None] * v
    return k, q


@functools.lru_cache(maxsize=None)
def _att_case(kind, B, H, hd, pos, ns, seed, star=None, oproj=False):
    """Operands and float64 reference of one launch.  pos: a tuple of B positions (< 0: a stopped row); `star`: the selected
    key of the select form (>= 0 from the first key, < 0 from the last: -1 is the new key itself, -2 the last cached one;
    clamped to the row's keys).  Cache rows at and above a row's position are NaN."""
    rng = np.random.default_rng(seed)
    D, half = H * hd, hd // 2
    T = [max(p, 0) + 1 for p in pos]
    max_len = max(T) + 3
    exact = kind != "float"
    cos, sin = _angle_tables(rng, max_len, half) if kind != "select" else _quarter_tables(rng, max_len, half)
    if kind == "float":
        qkv = rng.standard_normal((B, 3 * D)).astype(F32)
        kc = rng.standard_normal((B, max_len, D)).astype(F32)
        vc = rng.standard_normal((B, max_len, D)).astype(F32)
    else:
        qkv = _ints(rng, (B, 3 * D))
        kc = np.zeros((B, max_len, D), F32)
        vc = _ints(rng, (B, max_len, D))
        if kind == "count":
            qkv[:, D:2 * D] = 0.0
        else:
            for b in range(B):
                p, t = max(pos[b], 0), T[b]
                st = min(star, t - 1) if star >= 0 else max(t + star, 0)
                k, q = _selector_rows(rng, cos[p], sin[p], H, hd, t, st)
                kc[b, :t] = k.reshape(t, D)
                qkv[b, :D] = q.reshape(D)
                # the new key arrives UNROTATED: turn row t - 1 back (quarter turns: exact)
                qkv[b, D:2 * D] = ref.rotate(k[t - 1], cos[p], -sin[p]).reshape(D).astype(F32)
    for b in range(B):
        kc[b, max(pos[b], 0):] = np.nan
        vc[b, max(pos[b], 0):] = np.nan
    wo = None
    if oproj:
        wo = _ints(rng, (D, D), -2, 2) if exact else (rng.standard_normal((D, D)) / np.sqrt(D)).astype(F32)
    c = NS_(kind=kind, B=B, H=H, hd=hd, D=D, pos=pos, ns=ns, max_len=max_len, exact=exact, oproj=oproj, qkv=qkv, kc=kc, vc=vc,
            cos=cos, sin=sin, wo=wo, w=D if oproj else hd, star=star, seed=seed)
    c.rec, c.new, c.merged = [], [], []
    for b in range(B):
        rec, new = ref.decode_attention(qkv[b], kc[b], vc[b], cos.astype(F64), sin.astype(F64), pos[b], H, ns)
        rec = ref.project(rec, wo) if oproj else rec
        c.rec.append(rec)
        c.new.append(new)
        c.merged.append(ref.merge(rec))
    c.rec = np.stack(c.rec)
    c.keys = max(t1 - t0 for t in T for t0, t1 in ref.key_ranges(t, ns))
    c.bounds = dict(m=1e-5, l=1e-5, sums=1e-5, merged=1e-5)
    c.plain = None
    if kind == "float" and c.keys > FLOAT_KEYS:
        c.plain = _plain_fp32_errors(c)
        c.bounds = {k: max(1e-5, 4 * e) for k, e in c.plain.items()}
    for a in (qkv, kc, vc, cos, sin) + ((wo,) if oproj else ()):
        a.setflags(write=False)
    return c


def _plain_fp32_errors(c):
    """The same records evaluated plainly in fp32 NumPy (rotation, scores, exp, sums: every operand and result float32),
    against the float64 reference: the yardstick for ranges longer than FLOAT_KEYS keys."""
    H, hd, D = c.H, c.hd, c.D
    inv = F32(1) / np.sqrt(F32(hd))
    got = np.array(c.rec, F64)
    merged = []
    for b in range(c.B):
        p = max(c.pos[b], 0)

        def rot(x):
            a, bb = x[..., 0::2], x[..., 1::2]
            out = np.empty_like(x)
            out[..., 0::2], out[..., 1::2] = a * c.cos[p] - bb * c.sin[p], a * c.sin[p] + bb * c.cos[p]
            return out
        q, k = rot(c.qkv[b, :D].reshape(H, hd)), rot(c.qkv[b, D:2 * D].reshape(H, hd))
        K = np.concatenate([c.kc[b, :p].reshape(p, H, hd), k[None]])
        V = np.concatenate([c.vc[b, :p].reshape(p, H, hd), c.qkv[b, 2 * D:].reshape(1, H, hd)])
        for sp, (t0, t1) in enumerate(ref.key_ranges(p + 1, c.ns)):
            for h in range(H):
                if t1 > t0:
                    s = (K[t0:t1, h] @ q[h]) * inv
                    m = s.max()
                    e = np.exp(s - m)
                    assert s.dtype == e.dtype == F32
                    got[b, sp, h, 0], got[b, sp, h, 1], got[b, sp, h, 4:] = m, e.sum(dtype=F32), e @ V[t0:t1, h]
        merged.append(ref.merge(got[b]))
    live = c.rec[..., 1] > 0
    return dict(m=_err(got[..., 0][live], c.rec[..., 0][live]), l=_err(got[..., 1][live], c.rec[..., 1][live]),
                sums=_err(got[..., 4:][live], c.rec[..., 4:][live]), merged=_err(np.stack(merged), np.stack(c.merged)))


def _att_name(c, rows):
    return "pdn_decode_attention" + ("_oproj" if c.oproj else "") + ("_rows" if rows else "") + "_f32"


def _att_launch(hp, L, c, rows, what):
    """One call.  Checks everything but the records' values: what may not be written is NaN, what may not change has not,
    the one appended cache row per live sequence is the reference's.  Returns the records (B, ns, H, 4 + w)."""
    B, H, hd, D, ns, max_len = c.B, c.H, c.hd, c.D, c.ns, c.max_len
    assert rows or len(set(c.pos)) == 1
    qkv_rs, cbs, wo_rs, rr = 3 * D + 4, max_len * D + 8, D + 4, ns * H * (4 + c.w)
    Q, q_host = _padded(hp, c.qkv, qkv_rs)
    KC, kc_host = _padded(hp, c.kc.reshape(B, -1), cbs)
    VC, vc_host = _padded(hp, c.vc.reshape(B, -1), cbs)
    CS, SN = hp.from_numpy(np.ascontiguousarray(c.cos)), hp.from_numpy(np.ascontiguousarray(c.sin))
    pos_host = np.array(c.pos if rows else c.pos[:1], np.int32)
    POS = hp.from_numpy(pos_host)
    REC = hp.full(((B + 1) * rr + 4,), np.nan, F32)
    WO, wo_host = _padded(hp, c.wo, wo_rs) if c.oproj else (None, None)
    head = (Q._ptr, qkv_rs, CS._ptr, SN._ptr, KC._ptr, VC._ptr)
    tail = (B, H, hd, ns, cbs, POS._ptr, max_len, hp.stream())
    L.call(_att_name(c, rows), *head, *((WO._ptr, wo_rs, REC._ptr) if c.oproj else (REC._ptr,)), *tail)
    out = REC.get()
    assert np.isnan(out[B * rr:]).all(), (what, "records: wrote past row B")
    rec = out[:B * rr].reshape(B, ns, H, 4 + c.w)
    assert np.isnan(rec[..., 2:4]).all(), (what, "records: the two pad slots were written")
    _bits(Q.get(), q_host, what + ("qkv",))
    _bits(CS.get(), c.cos, what + ("cos",))
    _bits(SN.get(), c.sin, what + ("sin",))
    _bits(POS.get(), pos_host, what + ("pos",))
    if c.oproj:
        _bits(WO.get(), wo_host, what + ("Wo",))
    for name, buf, host, j in (("k", KC, kc_host, 0), ("v", VC, vc_host, 1)):
        got = buf.get()
        want, rows_got, rows_want = host.copy(), [], []
        for b in range(B):
            if c.pos[b] < 0:
                continue                                            # (a stopped row appends nothing)
            at = b * cbs + c.pos[b] * D
            rows_got.append(got[at:at + D]), rows_want.append(c.new[b][j])
            want[at:at + D] = got[at:at + D]                        # (judged below; -0 and 0 are the same row)
        if rows_got:
            (_same if c.exact else _rel)(np.stack(rows_got), np.stack(rows_want), what + ("appended " + name,))
        _bits(got, want, what + (name + " cache outside the appended rows",))
    return rec


def _att_verify(rec, c, what):
    want = c.rec
    dead = want[..., 1] == 0
    assert np.all(rec[..., 0][dead] == -np.inf) and np.all(rec[..., 1][dead] == 0) and np.all(rec[..., 4:][dead] == 0), \
        (what, "a range without keys is not [-inf, 0 | zeros]")
    live = ~dead
    assert np.isfinite(rec[..., :2][live]).all() and np.isfinite(rec[..., 4:][live]).all(), (what, "not finite")
    if c.exact:
        _same(rec[..., 1], want[..., 1], what + ("l",))
        _same(rec[..., 4:], want[..., 4:], what + ("sums",))
        zero = live & (want[..., 0] == 0)
        _same(rec[..., 0][zero], want[..., 0][zero], what + ("m",))
        rest = live & ~zero
        if rest.any():                                              # (all keys of the range at one score: one fp32 product)
            assert np.all(np.abs(rec[..., 0][rest] - want[..., 0][rest]) <= 1e-6 * np.abs(want[..., 0][rest])), (what, "m")
    else:
        _rel(rec[..., 0][live], want[..., 0][live], what + ("m",), c.bounds["m"])
        _rel(rec[..., 1][live], want[..., 1][live], what + ("l",), c.bounds["l"])
        _rel(rec[..., 4:][live], want[..., 4:][live], what + ("sums",), c.bounds["sums"])
    merged = np.stack([ref.merge(rec[b]) for b in range(c.B)])
    _rel(merged, np.stack(c.merged), what + ("merged",), c.bounds["merged"])


def _att_run(hp, L, kind, B, H, hd, pos, ns, seed, star=None, oproj=False, rows=False):
    if isinstance(pos, int):
        pos = (pos,) * B
    c = _att_case(kind, B, H, hd, tuple(pos), ns, seed, star, oproj)
    what = (_att_name(c, rows), kind, "B", B, "H", H, "hd", hd, "pos", pos if rows else pos[0], "ns", ns) + \
        (("star", star) if star is not None else ())
    _report((), False)
    if c.plain is not None:
        print(f"[decode_layer_variants] {' '.join(str(w) for w in what)}: {c.keys} keys per range, plain fp32 NumPy against "
              "float64: " + ", ".join(f"{k} {e:.2e}" for k, e in c.plain.items()))
    rec = _att_launch(hp, L, c, rows, what)
    _att_verify(rec, c, what)
    _report(what, not c.exact)
    return c, rec


def check_attention_every_head_dim(dev):
    """csrc/decode.hip decode_attention_kernel: `groups = dec_div(256, f4)`, `tg = dec_div(tid, f4)` (decode_stage.h: a
    float-reciprocal division) and the `tg < groups` mask for EVERY f4 = 1 .. 64 -- the count form at T = 5 keys in 3 ranges
    (2, 2 and 1 keys), two heads: one misplaced column quad or one thread past the last group changes an integer."""
    hp, L, device = _env(dev)
    with device:
        for hd in range(4, 257, 4):
            _att_run(hp, L, "count", 1, 2, hd, 4, 3, 1000 + hd)


HEAD_DIMS = (4, 44, 48, 64, 68, 128, 132, 192, 256)


def check_attention_head_dims(dev):
    """The three instantiations by head_dim -- 48 (KPRE 12, VPRE 13), 64 (16, 16), any (0, 0) -- and the head dims beside
    them: 4 (one column quad, 256 row groups), 44 / 68 (no power of two: 23 / 15 groups, idle threads), 128, 132 (7 groups of
    33 quads, 25 idle threads), 192, 256 (4 groups).  Each as count, select (t* = the first key, the last cached key, the new
    key) and float; T = 37 keys in 3 ranges, T = 1 (only the new key: nothing cached is read) with 1 and 4 ranges, and
    T = 3 with 64 ranges (61 of them without keys)."""
    hp, L, device = _env(dev)
    with device:
        for hd in HEAD_DIMS:
            for pos, ns in ((36, 3), (0, 1), (0, 4), (2, 64)):
                B = 2 if pos == 36 else 1
                _att_run(hp, L, "count", B, 2, hd, pos, ns, 1100 + hd)
                _att_run(hp, L, "float", B, 2, hd, pos, ns, 1200 + hd)
                for star in (0, -2, -1):
                    _att_run(hp, L, "select", B, 2, hd, pos, ns, 1300 + hd, star)


def check_attention_head_dims_above_128(dev):
    """csrc/decode.hip decode_attention_kernel, the combine of the PV partial sums: 8 threads per column quad add every 8th
    row group into 8 f4 slots, one thread per quad adds those 8.  Above head_dim 128, 8 f4 > 256 threads: a thread has to fill
    a second slot (left unwritten, the last pass added what the score buffer held there: floats 2048 .. 3071 at head_dim 256 --
    every column --, floats 1948 .. 1979 at head_dim 132 -- columns 100 .. 131).  The deciding cases are the count form with
    ONE range long enough that those floats provably hold probabilities (1.0 each): head_dim 256 at T = 3072, head_dim 132 at
    T = 2048 (H = 1, B = 1); then head_dim 192 (f4 = 48: slots 256 .. 383 of 384) as float with 1 and 3 ranges, and 132 / 256
    with short ranges, where the slots hold what the LDS held before."""
    hp, L, device = _env(dev)
    with device:
        _att_run(hp, L, "count", 1, 1, 256, 3071, 1, 1401)
        _att_run(hp, L, "count", 1, 1, 132, 2047, 1, 1402)
        for ns in (1, 3):
            _att_run(hp, L, "float", 2, 2, 192, 299, ns, 1403)
            _att_run(hp, L, "count", 1, 2, 192, 299, ns, 1404)
        for hd in (132, 256):
            _att_run(hp, L, "float", 1, 2, hd, 99, 1, 1405)
            _att_run(hp, L, "select", 1, 2, hd, 99, 1, 1406, 57)
            _att_run(hp, L, "count", 1, 1, hd, 99, 1, 1407, oproj=True)


def check_attention_register_preloads(dev):
    """csrc/decode.hip decode_attention_kernel<12, 13, ..> / <16, 16, ..>: a thread holds its first K row and VPRE V rows
    of its column quad in registers; keys beyond them are loaded in place.  head_dim 48: 21 row groups, VPRE x groups = 273
    -- T = 255 / 256 / 257 (the second pass of the score loop starts at key 256) and 273 / 274 (the first V row of the tail
    loop); head_dim 64: 16 groups, 256 V rows -- T = 256 / 257; T = 513 in one range (three passes of the score loop) for 48,
    64 and the generic 128.  One range, so that these are keys PER RANGE.  Count, float (T = 513: more than 400 keys per
    range, held to 4 x the plain fp32 NumPy error where that is above 1e-5) and select with t* at keys 63 / 64 (a wave
    edge), 255 / 256 (the pass edge), the last cached key and the new key."""
    hp, L, device = _env(dev)
    with device:
        for hd, Ts in ((48, (255, 256, 257, 273, 274, 513)), (64, (256, 257, 513)), (128, (513,))):
            for T in Ts:
                _att_run(hp, L, "count", 1, 2, hd, T - 1, 1, 1500 + T)
                _att_run(hp, L, "float", 1, 2, hd, T - 1, 1, 1600 + T)
            for star in (63, 64, 255, 256, -2, -1):
                _att_run(hp, L, "select", 1, 2, hd, 299, 1, 1700 + hd, star)


def check_attention_key_ranges(dev):
    """csrc/decode.hip decode_attention_kernel `chunk = (T + NS - 1) / NS, t0 = sp * chunk, t1 = min(T, t0 + chunk)` and
    `if (t0 >= t1)`: n_splits 1 / 3 / 4 / 64 at T = 1, 2, 5 (T < n_splits: ranges without keys, which must be [-inf, 0 |
    zeros]), 70 (64 ranges of 2 keys: 35 live) and 300 (ranges of 100 / 75 / 5 keys); head_dim 48 and 68.  Select with t* at the
    first and the last key of a middle range (T = 300, 3 ranges: keys 100 and 199) and beside the ranges' edge (99, 200)."""
    hp, L, device = _env(dev)
    with device:
        for hd in (48, 68):
            for ns in (1, 3, 4, 64):
                for T in (1, 2, 5, 70, 300):
                    _att_run(hp, L, "count", 2, 2, hd, T - 1, ns, 1800 + T)
                    _att_run(hp, L, "float", 2, 2, hd, T - 1, ns, 1900 + T)
            for star in (99, 100, 199, 200):
                _att_run(hp, L, "select", 1, 2, hd, 299, 3, 2000 + hd, star)


OPROJ_SHAPES = ((1, 48), (2, 12), (2, 20), (1, 28), (23, 44), (8, 128), (16, 64))


def check_attention_oproj(dev):
    """csrc/decode.hip decode_attention_kernel<.., OPROJ = true>: C workgroups share a (range, head), each with D / C
    columns of the head's rows of Wo; thread = (row slice, column quad), PW = 16 rows in registers, a tail loop behind them.
    D = 48 / 24 / 40 / 28: C = 4 / 3 / 2 / 1; D = 1012 (H = 23, head_dim 44): C = 1, nqd = 253 column quads, ONE row slice (3
    idle threads, 16 rows preloaded and 28 from the tail loop); D = 1024 with head_dim 128 (G = 4 slices: rows beyond PW x G =
    64 from the tail loop) and with head_dim 64 (exactly PW x G).  wo_row_stride = D + 4.  Count (integer Wo: exact), float,
    select; T = 37 in 3 ranges and T = 2 in 4 (two ranges without keys: all zeros)."""
    hp, L, device = _env(dev)
    with device:
        for H, hd in OPROJ_SHAPES:
            for pos, ns in ((36, 3), (1, 4)):
                _att_run(hp, L, "count", 1, H, hd, pos, ns, 2100 + hd, oproj=True)
                _att_run(hp, L, "float", 2 if H < 8 else 1, H, hd, pos, ns, 2200 + hd, oproj=True)
            _att_run(hp, L, "select", 1, H, hd, 36, 3, 2300 + hd, 17, oproj=True)


ROW_POS = (0, 255, -1, 256, 17)


def _row_alone(c, b):
    """Row b of a case as a case of its own at ONE position (a stopped row: position 0, where it appends its key)."""
    new = c.new[b] or ref.decode_attention(c.qkv[b], c.kc[b], c.vc[b], c.cos.astype(F64), c.sin.astype(F64), 0, c.H, c.ns)[1]
    return NS_(**{**vars(c), "B": 1, "pos": (max(c.pos[b], 0),), "qkv": c.qkv[b:b + 1], "kc": c.kc[b:b + 1], "vc": c.vc[b:b + 1],
                  "rec": c.rec[b:b + 1], "new": [new], "merged": c.merged[b:b + 1]})


def check_attention_rows(dev):
    """csrc/decode.hip decode_attention_kernel<.., ROWS = true>: B = 5 rows at positions 0, 255, stopped, 256 and 17, four
    ranges.  A stopped row (pos < 0) yields the records of position 0 from its own key alone, appends nothing and reads
    nothing cached (its whole cache row is NaN); every other cache row but the appended ones is untouched.  The entry with
    ONE position must give bit-equal records for each row alone.  head_dim 48, 64 and 68, with and without the Wo fold."""
    hp, L, device = _env(dev)
    with device:
        for hd, oproj in ((48, False), (48, True), (64, False), (64, True), (68, False), (68, True)):
            for kind, star in (("count", None), ("select", -2), ("select", -1), ("float", None)):
                seed = 2400 + hd
                c, rec = _att_run(hp, L, kind, len(ROW_POS), 2, hd, ROW_POS, 4, seed, star, oproj, rows=True)
                for b, p in enumerate(ROW_POS):
                    what = ("one position against rows", kind, hd, oproj, "row", b, "pos", p)
                    alone = _att_launch(hp, L, _row_alone(c, b), False, what)
                    _bits(alone[0], rec[b], what)
                    _report(what, False)


def check_attention_refusals(dev):
    """csrc/decode.hip decode_attention_impl's PDN_CHECK_ARGs, each EINVAL without a launch (the records stay NaN, the cache
    untouched): head_dim 6 and 260, n_splits 0 and 65, a qkv / records pointer 4 bytes off, a max_len whose scores exceed
    60 KiB (15361 with one range); with the Wo fold D = 1028 and n_splits x H = 257 (both: H = 257 at head_dim 4), D = 1032
    alone (H = 6 at head_dim 172) and a misaligned Wo.  Their neighbours are taken: max_len 15360, n_splits 64."""
    from pydynet_amd._lib import HipLibraryError
    hp, L, device = _env(dev)
    with device:
        # (each buffer as large as the refused shape would need, were it taken)
        sizes = (("qkv", 4096), ("kc", 15364 * 48), ("vc", 15364 * 48), ("rec", 272 * 1024))
        buf = {k: hp.full((n,), np.nan, F32) for k, n in sizes}
        tabs = hp.from_numpy(np.ones(16 * 1024 * 130, F32))
        wo = hp.from_numpy(np.ones(1040 * 1040, F32))
        pos = hp.from_numpy(np.zeros(8, np.int32))
        base = dict(H=1, hd=48, ns=1, max_len=8, q_off=0, r_off=0, wo_off=0, oproj=False)
        cases = {"head_dim 6": dict(hd=6), "head_dim 260": dict(hd=260), "n_splits 0": dict(ns=0), "n_splits 65": dict(ns=65),
                 "misaligned qkv": dict(q_off=4), "misaligned records": dict(r_off=4), "scores > 60 KiB": dict(max_len=15361),
                 "D 1028, n_splits * H 257": dict(H=257, hd=4, oproj=True), "D 1032": dict(H=6, hd=172, oproj=True),
                 "misaligned Wo": dict(wo_off=4, oproj=True)}
        for name, change in cases.items():
            a = {**base, **change}
            for rows in (False, True):
                D = a["H"] * a["hd"]
                head = (buf["qkv"]._ptr + a["q_off"], 3 * D + 4 - (3 * D) % 4, tabs._ptr, tabs._ptr, buf["kc"]._ptr, buf["vc"]._ptr)
                tail = (1, a["H"], a["hd"], a["ns"], 4 * ((a["max_len"] * D + 3) // 4), pos._ptr, a["max_len"], hp.stream())
                mid = (buf["rec"]._ptr + a["r_off"],)
                if a["oproj"]:
                    mid = (wo._ptr + a["wo_off"], D + 4 - D % 4) + mid
                entry = "pdn_decode_attention" + ("_oproj" if a["oproj"] else "") + ("_rows" if rows else "") + "_f32"
                with pytest.raises(HipLibraryError) as e:
                    L.call(entry, *head, *mid, *tail)
                assert e.value.code == EINVAL, (name, entry, e.value.code)
            for k in ("rec", "kc", "vc"):
                assert np.isnan(buf[k].get()).all(), (name, k, "was written")
        # the neighbours: 15360 scores (exactly 60 KiB) and 64 ranges at T = 1
        q = hp.from_numpy(np.zeros(3 * 48, F32))
        for ns, max_len in ((1, 15360), (64, 8)):
            kc, vc = hp.full((max_len * 48,), np.nan, F32), hp.full((max_len * 48,), np.nan, F32)
            rec = hp.full((ns * 52,), np.nan, F32)
            L.call("pdn_decode_attention_f32", q._ptr, 3 * 48, tabs._ptr, tabs._ptr, kc._ptr, vc._ptr, rec._ptr, 1, 1, 48, ns,
                   max_len * 48, pos._ptr, max_len, hp.stream())
            r = rec.get().reshape(ns, 52)
            assert r[0, 0] == 0 and r[0, 1] == 1 and np.all(r[0, 4:] == 0) and np.all(r[1:, 0] == -np.inf) and np.all(r[1:, 1] == 0)
            assert np.all(kc.get()[:48] == 0) and np.isnan(kc.get()[48:]).all()


for _fn in (check_attention_every_head_dim, check_attention_head_dims, check_attention_head_dims_above_128,
            check_attention_register_preloads, check_attention_key_ranges, check_attention_oproj, check_attention_rows,
            check_attention_refusals):
    device_variants(globals(), _fn)


# =====================================================================================================================
# 2. pdn_decode_block_f32 / pdn_decode_block_rows_f32
# =====================================================================================================================
BLOCK_ROUTES = {"hd 48 EXACT": (6, 48), "hd 48 PW 4": (2, 48), "hd 48 PW 16": (16, 48), "hd 48 PW 16, nsteps 48": (21, 48),
                "hd 64 EXACT": (4, 64), "hd 64 PW 4": (2, 64), "hd 64 PW 16": (16, 64)}


def _block_shape(D, hd):
    C = 4 if D % 16 == 0 else (3 if D % 12 == 0 else (2 if D % 8 == 0 else 1))
    SL, G, nqd = 256 // (hd // 4), 256 // (D // 4), D // C // 4
    return C, SL, G, nqd, 256 // nqd


def _block_route(H, hd):
    """(instantiation, pw_need, nsteps) as csrc/decode_block.hip decode_block_impl picks them."""
    D = H * hd
    C, SL, G, nqd, Go = _block_shape(D, hd)
    pw_need, nsteps, QP = (hd + Go - 1) // Go, (D + SL - 1) // SL, 14 if hd == 48 else 16
    return f"hd {hd} " + ("EXACT" if pw_need == 4 and nsteps == QP else ("PW 4" if pw_need <= 4 else "PW 16")), pw_need, nsteps


def _block_lds(D, H, hd, ns, max_len):
    """pdn_decode_block_lds_bytes, stated again: the row, the staging region, the scores of one range."""
    if not (hd in (48, 64) and H > 0 and D == H * hd and D <= 1024 and 1 <= ns <= 7 and (ns + 1) * H <= 256 and max_len >= 1):
        return 0
    C, SL, G, nqd, Go = _block_shape(D, hd)
    return 4 * (D + max(G * D, 3 * SL * hd) + max(-(-max_len // ns), (SL + 8) * hd, Go * nqd * 4))


@functools.lru_cache(maxsize=None)
def _blk_weights(exact, H, hd):
    """Exact: norm weight 1; Wq has one entry, 32, per head -- row i_h = h hd + 5, column h hd + 2 j_h, j_h = (3 h + 1) % (hd /
    2) --, so q = 32 e_(2 j_h) for every x with RMSNorm(x)[i_h] = 1; Wk and Wv signed-permutation-like (one entry of +-1 .. 3
    per column, any row); Wo integers in [-2, 2].  Float: standard normal / sqrt(D), norm weight about 1."""
    rng = np.random.default_rng(4000 + 100 * H + hd + exact)
    D, half = H * hd, hd // 2
    if exact:
        wq = np.zeros((D, D), F32)
        for h in range(H):
            wq[h * hd + 5, h * hd + 2 * ((3 * h + 1) % half)] = Q_SCALE
        wk, wv = np.zeros((D, D), F32), np.zeros((D, D), F32)
        for w in (wk, wv):
            w[rng.integers(0, D, D), np.arange(D)] = rng.choice([-3, -2, -1, 1, 2, 3], D)
        wo, nw, eps = _ints(rng, (D, D), -2, 2), np.ones(D, F32), 0.0
    else:
        wq, wk, wv, wo = ((rng.standard_normal((D, D)) / np.sqrt(D)).astype(F32) for _ in range(4))
        nw, eps = (1 + 0.1 * rng.standard_normal(D)).astype(F32), 1e-6
    return NS_(wq=wq, wk=wk, wv=wv, wo=wo, nw=nw, eps=eps, w64=[a.astype(F64) for a in (wq, wk, wv, wo)])


def _blk_case(kind, H, hd, B, pos, ns, n_parts, seed, star=None):
    """Operands and float64 reference of one launch.  Exact kinds: x = base + the parts is +-2 (+2 at the rows i_h) with
    eps = 0, so RMSNorm(x) is exactly +-1, q exactly 32 e_(2 j_h) and k, v small integers; `count`: the cached K are zero;
    `select`: quarter-turn tables and the cached keys of `_selector_rows` with t* = `star` (>= 0 from the first cached key, < 0
    from the last) -- the new key is a record of its own (m = one fp32 product, l = 1, sums = v Wo)."""
    rng = np.random.default_rng(seed)
    D, half, exact = H * hd, hd // 2, kind != "float"
    W = _blk_weights(exact, H, hd)
    P = [max(p, 0) for p in pos]
    max_len = max(P) + 4
    cos, sin = _quarter_tables(rng, max_len, half) if exact else _angle_tables(rng, max_len, half)
    if exact:
        x = 2.0 * rng.choice([-1.0, 1.0], (B, D))
        x[:, [h * hd + 5 for h in range(H)]] = 2.0
        parts = _ints(rng, (B, n_parts, D))
        base = (x - parts.astype(F64).sum(1)).astype(F32)
        kc, vc = np.zeros((B, max_len, D), F32), _ints(rng, (B, max_len, D))
        if kind == "select":
            for b in range(B):
                if P[b]:
                    st = min(star, P[b] - 1) if star >= 0 else max(P[b] + star, 0)
                    kc[b, :P[b]] = _selector_rows(rng, cos[P[b]], sin[P[b]], H, hd, P[b], st)[0].reshape(P[b], D)
    else:
        base = rng.standard_normal((B, D)).astype(F32)
        parts = (rng.standard_normal((B, n_parts, D)) / np.sqrt(max(n_parts, 1))).astype(F32)
        kc, vc = rng.standard_normal((B, max_len, D)).astype(F32), rng.standard_normal((B, max_len, D)).astype(F32)
    for b in range(B):
        kc[b, P[b]:], vc[b, P[b]:] = np.nan, np.nan
    c = NS_(kind=kind, B=B, H=H, hd=hd, D=D, pos=pos, ns=ns, n_parts=n_parts, max_len=max_len, exact=exact, base=base,
            parts=parts, kc=kc, vc=vc, cos=cos, sin=sin, W=W, w=D, bounds=dict(m=1e-5, l=1e-5, sums=1e-5, merged=1e-5))
    c.x, c.rec, c.new, c.merged = [], [], [], []
    for b in range(B):
        x, rec, new = ref.decode_block(base[b], parts[b], W.nw, W.eps, W.w64[0], W.w64[1], W.w64[2], cos.astype(F64),
                                       sin.astype(F64), kc[b], vc[b], pos[b], W.w64[3], H, ns)
        c.x.append(x), c.rec.append(rec), c.new.append(new), c.merged.append(ref.merge(rec))
    c.x, c.rec = np.stack(c.x), np.stack(c.rec)
    assert max(t1 - t0 for p in P for t0, t1 in ref.key_ranges(p, ns)) <= FLOAT_KEYS
    return c


def _blk_device_weights(hp, W, D):
    """Wqkv as three (D, D) blocks with w_row_stride = D + 4 and a row of NaN between the blocks; Wo with wo_row_stride =
    D + 4; uploaded once per shape, compared after every launch."""
    host = np.full((3, D + 1, D + 4), np.nan, F32)
    for j, w in enumerate((W.wq, W.wk, W.wv)):
        host[j, :D, :D] = w
    WO, wo_host = _padded(hp, W.wo, D + 4, extra=D + 8)
    return NS_(WQKV=hp.from_numpy(host), wqkv_host=host, WO=WO, wo_host=wo_host, NW=hp.from_numpy(W.nw))


def _blk_weights_unchanged(dv, W, what):
    for buf, host, name in ((dv.WQKV, dv.wqkv_host, "Wqkv"), (dv.WO, dv.wo_host, "Wo"), (dv.NW, W.nw, "norm_w")):
        _bits(buf.get(), host, what + (name,))


def _blk_run(hp, L, dv, route, kind, H, hd, B, pos, ns, n_parts, seed, star=None, rows=False):
    if isinstance(pos, int):
        pos = (pos,) * B
    c = _blk_case(kind, H, hd, B, tuple(pos), ns, n_parts, seed, star)
    D, max_len, W = c.D, c.max_len, c.W
    entry = "pdn_decode_block_rows_f32" if rows else "pdn_decode_block_f32"
    what = (entry, route, kind, "B", B, "H", H, "pos", pos if rows else pos[0], "ns", ns, "n_parts", n_parts) + \
        (("star", star) if star is not None else ())
    cbs, rr, parts_rs = max_len * D + 8, (ns + 1) * H * (4 + D), n_parts * D + 4
    _report((), False)
    BASE, base_host = _padded(hp, c.base, D + 4)
    PARTS, parts_host = _padded(hp, c.parts.reshape(B, -1), parts_rs) if n_parts else (None, None)
    XO = hp.full((B + 1, D + 4), np.nan, F32)
    KC, kc_host = _padded(hp, c.kc.reshape(B, -1), cbs)
    VC, vc_host = _padded(hp, c.vc.reshape(B, -1), cbs)
    CS, SN = hp.from_numpy(np.ascontiguousarray(c.cos)), hp.from_numpy(np.ascontiguousarray(c.sin))
    pos_host = np.array(pos if rows else pos[:1], np.int32)
    POS = hp.from_numpy(pos_host)
    REC = hp.full(((B + 1) * rr + 4,), np.nan, F32)
    L.call(entry, BASE._ptr, D + 4, PARTS._ptr if n_parts else None, n_parts, parts_rs if n_parts else 0, XO._ptr, D + 4,
           dv.NW._ptr, W.eps, dv.WQKV._ptr, D + 4, (D + 1) * (D + 4), CS._ptr, SN._ptr, KC._ptr, VC._ptr, cbs, POS._ptr, max_len,
           dv.WO._ptr, D + 4, REC._ptr, B, H, hd, ns, hp.stream())
    xo, out = XO.get(), REC.get()
    assert np.isnan(xo[B]).all() and np.isnan(xo[:B, D:]).all(), (what, "x_out: wrote outside its B x D block")
    (_same if c.exact else _rel)(xo[:B, :D], c.x, what + ("x_out",))
    assert np.isnan(out[B * rr:]).all(), (what, "records: wrote past row B")
    rec = out[:B * rr].reshape(B, ns + 1, H, 4 + D)
    assert np.isnan(rec[..., 2:4]).all(), (what, "records: the two pad slots were written")
    for buf, host, name in ((BASE, base_host, "base"), (CS, c.cos, "cos"), (SN, c.sin, "sin"), (POS, pos_host, "pos")) + \
            (((PARTS, parts_host, "parts"),) if n_parts else ()):       # (the weights: once per shape, _blk_weights_unchanged)
        _bits(buf.get(), host, what + (name,))
    for name, buf, host, j in (("k", KC, kc_host, 0), ("v", VC, vc_host, 1)):
        got = buf.get()
        want, rows_got, rows_want = host.copy(), [], []
        for b in range(B):
            if pos[b] >= 0:                                         # (a stopped row appends nothing)
                at = b * cbs + pos[b] * D
                rows_got.append(got[at:at + D]), rows_want.append(c.new[b][j])
                want[at:at + D] = got[at:at + D]                    # (judged below; -0 and 0 are the same row)
        if rows_got:
            (_same if c.exact else _rel)(np.stack(rows_got), np.stack(rows_want), what + ("appended " + name,))
        _bits(got, want, what + (name + " cache outside the appended rows",))
    _att_verify(rec, c, what)
    _report(what, not c.exact)


def _check_block(dev, route):
    """One instantiation of decode_block_kernel<F4, VPRE, QP, PW, EXACT, ROWS> through both entries.  n_ranges 1 / 4 / 7;
    positions 0 (no cached key: every range role leaves [-inf, 0 | zeros]), 1, NS - 1 (fewer cached keys than ranges), 256 NS
    and 256 NS + 1 (256 / 257 keys per range: the second pass of the score loop; head_dim 64: the first V row of the tail
    loop), head_dim 48 also 273 NS + 1 (274 per range: past VPRE x groups = 273).  The small positions with B = 1 and 8 and
    n_parts 0 and 5 (the plain-record hand-off of decode_stage.h), the large ones with B = 1 and 5 parts, and B = 8 at pos =
    256 with one range.  Each as float, count and select -- t* at the last cached key; at pos = 256 NS + 1 also at the first
    key, with one range at keys 63 / 64 (a wave's edge: the per-wave rescale factors fw[w]) and 255 / 256 (the pass edge),
    with more at the last key of the first range and the first of the second.  One ROWS launch of 5 rows at positions 0, 37,
    stopped, 300 and 17 (a stopped row: the records of position 0, nothing appended, nothing cached read)."""
    H, hd = BLOCK_ROUTES[route]
    D = H * hd
    name, pw_need, nsteps = _block_route(H, hd)
    assert route.startswith(name) and (("nsteps %d" % nsteps) in route or "nsteps" not in route), (route, name, pw_need, nsteps)
    hp, L, device = _env(dev)
    seed = 4100 + D
    with device:
        dvs = {e: _blk_device_weights(hp, _blk_weights(e, H, hd), D) for e in (True, False)}

        def run(kind, *a, **kw):
            _blk_run(hp, L, dvs[kind != "float"], route, kind, H, hd, *a, **kw)
        for ns in (1, 4, 7):
            assert L.query("pdn_decode_block_supported", D, H, hd, ns) == 1
            for pos in sorted({0, 1, ns - 1}):
                for B, n_parts in ((1, 0), (1, 5), (8, 0), (8, 5)):
                    for kind, star in (("float", None), ("count", None), ("select", 0)):
                        run(kind, B, pos, ns, n_parts, seed + pos, star)
            big = [256 * ns, 256 * ns + 1] + ([273 * ns + 1] if hd == 48 else [])
            for pos in big:
                chunk = -(-pos // ns)
                stars = ((0, 63, 64, 255, 256, -1) if ns == 1 else (0, chunk - 1, chunk, -1)) if pos == big[1] else (-1,)
                for kind, star in (("float", None), ("count", None)) + tuple(("select", s) for s in stars):
                    run(kind, 1, pos, ns, 5, seed + pos, star)
        run("float", 8, 256, 1, 0, seed + 7)
        run("select", 8, 256, 1, 0, seed + 7, 200)
        for kind, star in (("float", None), ("count", None), ("select", -1), ("select", 0)):
            run(kind, 5, (0, 37, -1, 300, 17), 4, 5, seed + 9, star, rows=True)
        for e in (True, False):
            _blk_weights_unchanged(dvs[e], _blk_weights(e, H, hd), (route, "after every launch of the shape"))


def _block_check(route):
    def check(dev):
        _check_block(dev, route)
    check.__name__ = "check_block_" + route.replace(",", "").replace(" ", "_").lower()
    check.__doc__ = "csrc/decode_block.hip, the instantiation '%s' (H = %d): see _check_block." % (route, BLOCK_ROUTES[route][0])
    return check


for _route in BLOCK_ROUTES:
    device_variants(globals(), _block_check(_route))


def check_block_refusals(dev):
    """csrc/decode_block.hip decode_block_impl: B = 9 is EINVAL; n_ranges = 8 is EUNSUPPORTED, so is (n_ranges + 1) x H = 257
    (257 is prime: only H = 257 with no range reaches it, a shape that is not taken on other grounds too), so is a max_len
    whose pdn_decode_block_lds_bytes exceed 64 KiB (the last max_len that fits is taken).  Nothing is written.
    pdn_decode_block_lds_bytes agrees with the emulator's statement and this file's over a grid of shapes."""
    from pydynet_amd._lib import HipLibraryError
    from tests.abi_emulator._decode import DecodeMixin
    hp, L, device = _env(dev)
    emu = DecodeMixin()
    for H, hd in list(BLOCK_ROUTES.values()) + [(1, 48), (22, 48), (3, 64), (17, 64), (4, 32), (257, 48)]:
        for ns in (0, 1, 3, 7, 8):
            for max_len in (0, 1, 255, 2048, 9000, 40000, 120000):
                got = L.query("pdn_decode_block_lds_bytes", H * hd, H, hd, ns, max_len)
                want = _block_lds(H * hd, H, hd, ns, max_len)
                assert got == emu.pdn_decode_block_lds_bytes(H * hd, H, hd, ns, max_len) == want, (H, hd, ns, max_len, got, want)
    H, hd, D = 2, 48, 96
    fits = max(m for m in range(1, 20000) if _block_lds(D, H, hd, 1, m) <= 65536)
    assert _block_lds(D, H, hd, 1, fits + 1) > 65536
    with device:
        W = _blk_weights(False, H, hd)
        dv = _blk_device_weights(hp, W, D)
        n = 9 * (fits + 2) * D
        KC, VC = hp.full((n,), np.nan, F32), hp.full((n,), np.nan, F32)
        tabs = hp.from_numpy(np.ones((fits + 2) * hd // 2, F32))
        BASE = hp.from_numpy(np.ones(9 * D, F32))
        POS = hp.from_numpy(np.zeros(9, np.int32))
        XO, REC = hp.full((9 * D,), np.nan, F32), hp.full((9 * 9 * 257 * (4 + D),), np.nan, F32)

        def call(entry, B, H_, ns, max_len):
            L.call(entry, BASE._ptr, D, None, 0, 0, XO._ptr, D, dv.NW._ptr, 1e-6, dv.WQKV._ptr, D + 4, (D + 1) * (D + 4), tabs._ptr,
                   tabs._ptr, KC._ptr, VC._ptr, max_len * D, POS._ptr, max_len, dv.WO._ptr, D + 4, REC._ptr, B, H_, hd, ns,
                   hp.stream())
        for entry in ("pdn_decode_block_f32", "pdn_decode_block_rows_f32"):
            for name, args, code in (("B = 9", (9, H, 1, 8), EINVAL), ("n_ranges = 8", (1, H, 8, 8), EUNSUPPORTED),
                                     ("(n_ranges + 1) H = 257", (1, 257, 0, 8), EUNSUPPORTED),
                                     ("LDS > 64 KiB", (1, H, 1, fits + 1), EUNSUPPORTED)):
                with pytest.raises(HipLibraryError) as e:
                    call(entry, *args)
                assert e.value.code == code, (entry, name, e.value.code)
                for buf in (XO, REC, KC, VC):
                    assert np.isnan(buf.get()).all(), (entry, name, "something was written")
        call("pdn_decode_block_f32", 1, H, 1, fits)
        assert np.isfinite(XO.get()[:D]).all() and np.isfinite(KC.get()[:D]).all() and np.isnan(KC.get()[D:]).all()


device_variants(globals(), check_block_refusals)


# =====================================================================================================================
# 3. pdn_decode_mlp_f32
# =====================================================================================================================
MLP_SHAPES = {4: (1, 4), 12: (1, 12), 36: (3, 12), 288: (6, 48), 292: (73, 4), 300: (3, 100), 1024: (16, 64)}    # D: (H, hd)


def _mlp_route(B, D):
    """(NB, PD, EXACT) as csrc/decode_layer.hip pdn_decode_mlp_f32 picks them."""
    G = 256 // (D // 4)
    exact = (D + 15) // 16 == 18 and (32 + G - 1) // G == 11
    return (1 if B == 1 else (2 if B == 2 else 4)), (11 if exact else 16), exact


def _mlp_records(hp, L, rng, D, B):
    """Records for the hand-off as family 1 leaves them: pdn_decode_attention_oproj_f32 at position 1 with the most ranges
    n_splits x H <= 256 allows up to 4 (T = 2: every range past the second has no keys: l = 0, zeros), verified there.
    -> (B, ns, H, 4 + D) float32 with NaN in the pad slots, ns, H."""
    H, hd = MLP_SHAPES[D]
    ns = min(4, 256 // H)
    c = _att_case("float", B, H, hd, (1,) * B, ns, 3000 + D, None, True)
    what = ("records for the feed-forward", D)
    rec = _att_launch(hp, L, c, False, what)
    _att_verify(rec, c, what)
    _report(what)
    assert (rec[..., 1] == 0).any()
    return rec, ns, H


def _mlp_weights(hp, rng, D, F, gate=None):
    """Wg / Wu (D, F) with w_row_stride = F + 4 and Wd (F, D) with wd_row_stride = D + 4, NaN in the padding and in a row
    behind each; `gate`: a Wg given by the case."""
    wg = (rng.standard_normal((D, F)) / np.sqrt(D)).astype(F32) if gate is None else gate
    wu = (rng.standard_normal((D, F)) / np.sqrt(D)).astype(F32)
    wd = (rng.standard_normal((F, D)) / np.sqrt(F)).astype(F32)
    nw = (1 + 0.1 * rng.standard_normal(D)).astype(F32)
    dev = [_padded(hp, a, a.shape[1] + 4, extra=16 * (a.shape[1] + 4)) for a in (wg, wu, wd)]     # (16 rows of NaN behind)
    return NS_(wg=wg, wu=wu, wd=wd, nw=nw, dev=dev, NW=hp.from_numpy(nw), D=D, F=F)


def _mlp_case(hp, L, W, base, rec, ns, H, with_out, what):
    B, D, F, J = base.shape[0], W.D, W.F, W.F // 32
    eps = 1e-6
    _report((), False)
    BASE, base_host = _padded(hp, base, D + 4)
    recs_rs = 0 if rec is None else ns * H * (4 + D) + 8
    REC, rec_host = _padded(hp, rec.reshape(B, -1), recs_rs) if rec is not None else (None, None)
    XO = hp.full((B + 1, D + 4), np.nan, F32)
    PARTS = hp.full((B + 1, J * D + 4), np.nan, F32)
    (WG, wg_host), (WU, wu_host), (WD, wd_host) = W.dev
    L.call("pdn_decode_mlp_f32", BASE._ptr, D + 4, REC._ptr if rec is not None else None, recs_rs, ns, H,
           XO._ptr if with_out else None, D + 4 if with_out else 0, W.NW._ptr, eps, WG._ptr, WU._ptr, F + 4, WD._ptr, D + 4,
           PARTS._ptr, J * D + 4, B, D, F, hp.stream())
    parts, xo = PARTS.get(), XO.get()
    assert np.isnan(parts[B]).all() and np.isnan(parts[:B, J * D:]).all(), (what, "parts: wrote outside its B x J x D block")
    _bits(BASE.get(), base_host, what + ("base",))
    for buf, host, name in ((WG, wg_host, "Wg"), (WU, wu_host, "Wu"), (WD, wd_host, "Wd")):
        _bits(buf.get(), host, what + (name,))
    _bits(W.NW.get(), W.nw, what + ("norm_w",))
    if rec is not None:
        _bits(REC.get(), rec_host, what + ("records",))
    want = [ref.decode_mlp(base[b], None if rec is None else rec[b], W.nw, eps, W.wg, W.wu, W.wd) for b in range(B)]
    if with_out:
        assert np.isnan(xo[B]).all() and np.isnan(xo[:B, D:]).all(), (what, "x_out: wrote outside its B x D block")
        if rec is None:
            _bits(xo[:B, :D], base, what + ("x_out is the base row",))
        else:
            _rel(xo[:B, :D], np.stack([h for h, _ in want]), what + ("x_out",))
    else:
        assert np.isnan(xo).all(), (what, "x_out")
    _rel(parts[:B, :J * D].reshape(B, J, D), np.stack([p for _, p in want]), what + ("parts",))
    _report(what)


def _check_mlp(dev, D):
    """csrc/decode_layer.hip decode_mlp_kernel<NB, PD, EXACT> at one D, B = 1 .. 8: NB = 1 / 2 / 4 rows per pass -- B = 3,
    5, 6, 7 leave a ragged last pass (`min(b0 + r, B - 1)`, `b0 + r < B`), B = 5 .. 8 two passes; F = 32 (one workgroup) and
    96; with the records of family 1 (the merge of decode_stage.h with ranges of l = 0; records_row_stride > the records)
    and without; x_out given and null (without records it receives the base row)."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(3100 + D)
    with device:
        rec8, ns, H = _mlp_records(hp, L, rng, D, 8)
        for F in (32, 96):
            W = _mlp_weights(hp, rng, D, F)
            for B in range(1, 9):
                assert _mlp_route(B, D) == ((1, 2, 4, 4, 4, 4, 4, 4)[B - 1], 11 if D == 288 else 16, D == 288)
                base = rng.standard_normal((B, D)).astype(F32)
                for with_rec in (True, False):
                    for with_out in (True, False):
                        what = ("pdn_decode_mlp_f32", "NB %d PD %d EXACT %d" % _mlp_route(B, D), "D", D, "F", F, "B", B,
                                "records", with_rec, "x_out", with_out)
                        _mlp_case(hp, L, W, base, rec8[:B] if with_rec else None, ns, H, with_out, what)


def check_mlp_d4(dev):
    """D = 4: one k-step, a quarter of it live.  Slices without a row must re-read a row that EXISTS (`k < D ? k : kslice`,
    kslice = min(slice, D - 1)): they went to row `slice` = 4 .. 15 of a 4-row Wg / Wu -- past the matrix, and 0 x what lay
    there was added (here 16 rows of NaN lie behind each matrix; found by this test).  G = 256 slices of the down projection
    for its 32 rows."""
    _check_mlp(dev, 4)


def check_mlp_d12(dev):
    """D = 12: one partial k-step (slices 12 .. 15 without a row, as at D = 4); nq = 3 column quads, G = 85 (one idle thread)."""
    _check_mlp(dev, 12)


def check_mlp_d36(dev):
    """D = 36: three k-steps, the last partial (4 of 16 slices); G = 28, 4 idle threads."""
    _check_mlp(dev, 36)


def check_mlp_d288(dev):
    """D = 288: the EXACT instantiations (18 k-steps, 11 rows of Wd: every weight load unconditional)."""
    _check_mlp(dev, 288)


def check_mlp_d292(dev):
    """D = 292: the first D past the 18 preloaded k-steps: the tail loop runs for 4 of the 16 slices; H = 73 heads merged."""
    _check_mlp(dev, 292)


def check_mlp_d300(dev):
    """D = 300: the tail loop for 12 slices; G = 3 with 31 idle threads, 11 rows of Wd and 5 masked ones."""
    _check_mlp(dev, 300)


def check_mlp_d1024(dev):
    """D = 1024: 64 k-steps (46 from the tail loop); G = 1: a thread holds 16 rows of Wd and takes 16 from the tail loop; the
    largest staged rows (8 x 1024 floats + scratch in LDS)."""
    _check_mlp(dev, 1024)


def check_mlp_saturated_gate(dev):
    """csrc/decode_layer.hip `hb = g / (1.f + expf(-g)) * u` with gate pre-activations of +-90 (85 .. 95): expf(90) is inf
    in fp32, so silu(-90) must come out as -0 (float64: -7e-38), silu(90) as 90 -- finite, and the float64 result."""
    hp, L, device = _env(dev)
    rng = np.random.default_rng(3200)
    with device:
        for D in (36, 288):
            base = rng.standard_normal((1, D)).astype(F32)
            nw = np.ones(D, F32)
            n = ref.rmsnorm(base[0], nw, 1e-6)
            g = rng.uniform(85, 95, 32) * rng.choice([-1, 1], 32)
            W = _mlp_weights(hp, rng, D, 32, gate=(np.outer(n, g) / (n @ n)).astype(F32))
            W.nw, W.NW = nw, hp.from_numpy(nw)
            got_g = ref.rmsnorm(base[0], nw, 1e-6) @ W.wg.astype(F64)
            assert np.all(np.abs(got_g) > 84) and (got_g > 0).any() and (got_g < 0).any()
            _mlp_case(hp, L, W, base, None, 0, 0, True, ("pdn_decode_mlp_f32", "gate +-90", "D", D))


for _fn in (check_mlp_d4, check_mlp_d12, check_mlp_d36, check_mlp_d288, check_mlp_d292, check_mlp_d300, check_mlp_d1024,
            check_mlp_saturated_gate):
    device_variants(globals(), _fn)


# =====================================================================================================================
# 4. pdn_kv_append_rows_f32 and pdn_decode_extend_attention_f32
# =====================================================================================================================
EX_MAX_RUN, EX_MAX_LEN = 33, 140


def _ex_layout(full):
    """runs [q0, n, start, ends] (one per cache row), n_q, and the runs that must be skipped.  Full: n = 1, 7, 8, 9, 15, 16,
    17, 33 (the 8-query append blocks and the 16-query attention blocks, one short, exact, one over; 33: three blocks) at
    start 0 and 100; T = start + n = 31 / 32 / 33, 63 / 64 / 65 and 127 / 128 / 129 (every key tile kt = 64 / 32 / 16 one
    short, exact, one over); `ends` on every second run, once with start + n = max_len (nothing to zero).  A row of the query
    buffer lies between two runs (never written).  Skipped: n = 0, n > max_run, q0 + n > n_q, start + n > max_len."""
    spec = [(n, s) for s in (0, 100) for n in (1, 7, 8, 9, 15, 16, 17, 33)] if full else [(1, 0), (9, 0), (17, 100), (33, 31)]
    if full:
        spec += [(15, 16), (16, 16), (17, 16), (16, 47), (16, 48), (16, 49), (17, 110), (17, 111), (17, 112),
                 (7, EX_MAX_LEN - 7)]
    runs, q0 = [], 1
    for i, (n, s) in enumerate(spec):
        runs.append([q0, n, s, int(i % 2 == 0 or s + n == EX_MAX_LEN)])
        q0 += n + 1
    skipped = [[q0, 0, 5, 1], [q0 + 1, EX_MAX_RUN + 1, 3, 1], [0, 3, EX_MAX_LEN - 2, 1]]
    n_q = q0 + 1 + EX_MAX_RUN + 1 + 2
    skipped.append([n_q - 2, 3, 9, 1])
    return runs + skipped, n_q, len(skipped)


@functools.lru_cache(maxsize=None)
def _ex_case(kind, hd, ns, full, seed):
    """Operands and float64 references of an append + extend pair, H = 2.  Cache row r holds context at positions [0,
    start_r) and NaN from there on.  `count`: every k zero, v integers.  `climb` (the select form of a layout whose queries
    share their keys): quarter-turn tables, but the identity in the selector pair j_h of head h; q = 32 e_(2 j_h); the key at
    position t has (t + 1) x far along it -- the scaled score climbs by >= 1024 per position, so a query selects the LAST key
    it may see in each range: its own position in its own range (l = 1, sums = that v), and the key one past it would win,
    were it not masked."""
    rng = np.random.default_rng(seed)
    H = 2
    D, half = H * hd, hd // 2
    runs, n_q, n_skipped = _ex_layout(full)
    R = len(runs)
    exact = kind != "float"
    cos, sin = _angle_tables(rng, EX_MAX_LEN, half) if kind == "float" else _quarter_tables(rng, EX_MAX_LEN, half)
    if kind == "float":
        qkv = rng.standard_normal((n_q, 3 * D)).astype(F32)
        kc = rng.standard_normal((R + 1, EX_MAX_LEN, D)).astype(F32)
        vc = rng.standard_normal((R + 1, EX_MAX_LEN, D)).astype(F32)
    else:
        qkv = _ints(rng, (n_q, 3 * D))
        kc = np.zeros((R + 1, EX_MAX_LEN, D), F32)
        vc = _ints(rng, (R + 1, EX_MAX_LEN, D))
        qkv[:, D:2 * D] = 0.0
        if kind == "climb":
            sel = [h * hd + 2 * ((3 * h + 1) % half) for h in range(H)]
            for h in range(H):
                cos[:, (3 * h + 1) % half], sin[:, (3 * h + 1) % half] = 1.0, 0.0
            kc[...] = _ints(rng, kc.shape)
            kc[:, :, sel] = (_far(hd) * (np.arange(EX_MAX_LEN) + 1))[None, :, None]
            kc[:, :, [s + 1 for s in sel]] = _far(hd) * rng.choice([-1.0, 1.0], (R + 1, EX_MAX_LEN, H))
            qkv[:, :D] = 0.0
            qkv[:, sel] = Q_SCALE
            for q0, n, s, _ in runs:                                # the new keys arrive unrotated: turn them back
                for j in range(n):
                    if 0 <= q0 + j < n_q and 0 <= s + j < EX_MAX_LEN:
                        qkv[q0 + j, D:2 * D] = ref.rotate(kc[0, s + j].reshape(H, hd), cos[s + j], -sin[s + j]).reshape(D)
    for r, (q0, n, s, _) in enumerate(runs):
        kc[r, max(s, 0):], vc[r, max(s, 0):] = np.nan, np.nan
    kc[R], vc[R] = np.nan, np.nan
    c = NS_(kind=kind, H=H, hd=hd, D=D, ns=ns, runs=np.array(runs, np.int32), n_q=n_q, R=R, exact=exact, qkv=qkv, kc=kc, vc=vc,
            cos=cos, sin=sin, n_skipped=n_skipped, bounds=dict(m=1e-5, l=1e-5, sums=1e-5, merged=1e-5))
    c.kc64, c.vc64 = kc.astype(F64), vc.astype(F64)
    ref.kv_append(qkv, cos.astype(F64), sin.astype(F64), c.kc64, c.vc64, runs, EX_MAX_RUN, H, EX_MAX_LEN)
    c.part = np.full((n_q, ns, H, 4 + hd), np.nan, F64)
    ref.extend_attention(qkv, cos.astype(F64), sin.astype(F64), c.kc64, c.vc64, runs, EX_MAX_RUN, H, ns, EX_MAX_LEN, c.part)
    c.taken = np.flatnonzero(~np.isnan(c.part[:, 0, 0, 1]))
    assert len(c.taken) == sum(n for _, n, _, _ in runs[:R - n_skipped])
    return c


def _ex_run(hp, L, kind, hd, ns, full, seed):
    c = _ex_case(kind, hd, ns, full, seed)
    H, D, R, n_q = c.H, c.D, c.R, c.n_q
    what = ("extend", kind, "hd", hd, "ns", ns, "runs", R)
    qkv_rs, cbs = 3 * D + 4, EX_MAX_LEN * D + 8
    _report((), False)
    Q, q_host = _padded(hp, c.qkv, qkv_rs)
    KC, kc_host = _padded(hp, c.kc.reshape(R + 1, -1), cbs)
    VC, vc_host = _padded(hp, c.vc.reshape(R + 1, -1), cbs)
    CS, SN, RUNS = (hp.from_numpy(np.ascontiguousarray(a)) for a in (c.cos, c.sin, c.runs))
    L.call("pdn_kv_append_rows_f32", Q._ptr, qkv_rs, CS._ptr, SN._ptr, KC._ptr, VC._ptr, cbs, RUNS._ptr, R, EX_MAX_RUN, n_q, H, hd,
           EX_MAX_LEN, hp.stream())
    after = []
    for name, buf, host, want64 in (("k", KC, kc_host, c.kc64), ("v", VC, vc_host, c.vc64)):
        got = buf.get()
        want = host.copy()
        inner = want[:(R + 1) * cbs].reshape(R + 1, cbs)[:, :EX_MAX_LEN * D]
        written = ~np.isnan(want64.reshape(R + 1, -1)) & np.isnan(inner)           # appended rows and zeroed slots
        got_in = got[:(R + 1) * cbs].reshape(R + 1, cbs)[:, :EX_MAX_LEN * D]
        assert written.any() and not written[R - c.n_skipped:].any()
        (_same if c.exact else _rel)(got_in[written], want64.reshape(R + 1, -1)[written], what + ("appended " + name,))
        inner[written] = got_in[written]
        _bits(got, want, what + (name + " cache outside the appended rows",))
        after.append(got)
    PART = hp.full(((n_q + 1) * c.ns * H * (4 + hd) + 4,), np.nan, F32)
    L.call("pdn_decode_extend_attention_f32", Q._ptr, qkv_rs, CS._ptr, SN._ptr, KC._ptr, VC._ptr, cbs, RUNS._ptr, R, EX_MAX_RUN,
           n_q, H, hd, c.ns, EX_MAX_LEN, PART._ptr, hp.stream())
    for buf, host, name in ((Q, q_host, "qkv"), (CS, c.cos, "cos"), (SN, c.sin, "sin"), (RUNS, c.runs, "runs"),
                            (KC, after[0], "k cache"), (VC, after[1], "v cache")):
        _bits(buf.get(), host, what + (name,))
    out = PART.get()
    part = out[:n_q * c.ns * H * (4 + hd)].reshape(n_q, c.ns, H, 4 + hd)
    idle = np.setdiff1d(np.arange(n_q), c.taken)
    assert np.isnan(out[part.size:]).all() and np.isnan(part[idle]).all(), (what, "records of a query row outside every run")
    rec = part[c.taken].copy()
    assert np.all(rec[..., 2:4] == 0), (what, "the pad slots of a record are zeros here")
    rec[..., 2:4] = np.nan
    want = c.part[c.taken]
    _att_verify(rec, NS_(rec=want, exact=c.exact, bounds=c.bounds, B=len(c.taken), merged=[ref.merge(r) for r in want]), what)
    _report(what, not c.exact)


def _check_extend(dev, hd):
    hp, L, device = _env(dev)
    with device:
        for kind in ("count", "climb", "float"):
            for ns in (1, 4):
                _ex_run(hp, L, kind, hd, ns, True, 5000 + hd)
            _ex_run(hp, L, kind, hd, 64, False, 5100 + hd)


def _extend_check(hd):
    def check(dev):
        _check_extend(dev, hd)
    check.__name__ = "check_extend_hd%d" % hd
    check.__doc__ = ("csrc/extend.hip kv_append_rows_kernel and extend_attention_kernel at head_dim %d (key tile kt = %d): the "
                     "layouts of _ex_layout with 1 and 4 key ranges, a small one with 64 (most ranges without keys), as count, "
                     "climb and float (_ex_case)." % (hd, 64 if hd <= 64 else (32 if hd <= 128 else 16)))
    return check


for _hd in (48, 64, 68, 128, 132, 256):
    device_variants(globals(), _extend_check(_hd))


def check_extend_runs_of_one_against_decode_rows(dev):
    """A layout of runs of length 1 is a ragged decode step: pdn_kv_append_rows_f32 + pdn_decode_extend_attention_f32 must
    give the records of pdn_decode_attention_rows_f32 at the same positions (0, 255, 256, 17, 3; 4 ranges), under the FLOAT
    criterion -- both are held to float64 elsewhere; here to each other."""
    hp, L, device = _env(dev)
    pos = (0, 255, 256, 17, 3)
    B, H, ns = len(pos), 2, 4
    with device:
        for hd in (48, 64, 132):
            c = _att_case("float", B, H, hd, pos, ns, 5200 + hd)
            D = c.D
            rows = _att_launch(hp, L, c, True, ("rows for the cross-check", hd))
            qkv_rs, cbs = 3 * D + 4, c.max_len * D + 8
            Q, _ = _padded(hp, c.qkv, qkv_rs)
            KC, _ = _padded(hp, c.kc.reshape(B, -1), cbs)
            VC, _ = _padded(hp, c.vc.reshape(B, -1), cbs)
            CS, SN = hp.from_numpy(np.ascontiguousarray(c.cos)), hp.from_numpy(np.ascontiguousarray(c.sin))
            RUNS = hp.from_numpy(np.array([[b, 1, pos[b], 0] for b in range(B)], np.int32))
            PART = hp.full((B * ns * H * (4 + hd),), np.nan, F32)
            L.call("pdn_kv_append_rows_f32", Q._ptr, qkv_rs, CS._ptr, SN._ptr, KC._ptr, VC._ptr, cbs, RUNS._ptr, B, 1, B, H, hd,
                   c.max_len, hp.stream())
            L.call("pdn_decode_extend_attention_f32", Q._ptr, qkv_rs, CS._ptr, SN._ptr, KC._ptr, VC._ptr, cbs, RUNS._ptr, B, 1, B,
                   H, hd, ns, c.max_len, PART._ptr, hp.stream())
            part = PART.get().reshape(B, ns, H, 4 + hd)
            what = ("runs of one against pdn_decode_attention_rows_f32", hd)
            dead = rows[..., 1] == 0
            assert np.array_equal(part[..., 1] == 0, dead) and np.all(part[..., 0][dead] == -np.inf)
            for name, sl in (("m", (..., 0)), ("l", (..., 1)), ("sums", (..., slice(4, None)))):
                _rel(part[sl][~dead], np.asarray(rows[sl][~dead], F64), what + (name,))
            merged = [np.stack([ref.merge(r[b]) for b in range(B)]) for r in (part, rows)]
            _rel(merged[0], merged[1], what + ("merged",))
            _report(what)


device_variants(globals(), check_extend_runs_of_one_against_decode_rows)


# =====================================================================================================================
# the harness notices what it is meant to notice (on the emulator, one injected defect each)
# =====================================================================================================================
def _attention_with_defect(emu, defect):
    """pdn_decode_attention_f32 of the emulator, its records replaced by the float64 statement with ONE defect: `boundary`
    -- the first range takes one key of the second (one range: the last key is dropped); `neighbour` -- key t is paired with
    the value of key t - 1."""
    from tests.abi_emulator import flat, view
    good = emu.pdn_decode_attention_f32

    def bad(qkv, rs, cos, sin, kc, vc, parts, B, H, hd, NS, cbs, pos, max_len, stream):
        rc = good(qkv, rs, cos, sin, kc, vc, parts, B, H, hd, NS, cbs, pos, max_len, stream)
        if rc:
            return rc
        D, half, p = H * hd, hd // 2, int(flat(pos, 1, np.int32)[0])
        T = p + 1
        c, s = (np.array(flat(t, max_len * half), F64).reshape(max_len, half)[p] for t in (cos, sin))
        out = flat(parts, B * NS * H * (4 + hd)).reshape(B, NS, H, 4 + hd)
        ranges = ref.key_ranges(T, NS)
        if defect == "boundary":
            if len([r for r in ranges if r[1] > r[0]]) > 1:
                ranges[0], ranges[1] = (0, ranges[0][1] + 1), (ranges[1][0] + 1, max(ranges[1][1], ranges[1][0] + 1))
            else:
                ranges[0] = (0, T - 1)
        for b in range(B):
            q = ref.rotate(np.array(view(qkv + 4 * b * rs, (H, hd), (hd, 1), F32)), c, s)
            K = np.array(view(kc + 4 * b * cbs, (T, H, hd), (D, hd, 1), F32), F64)         # (the new row is in the cache by now)
            V = np.array(view(vc + 4 * b * cbs, (T, H, hd), (D, hd, 1), F32), F64)
            rec = ref.records_of(q, K, np.roll(V, 1, axis=0) if defect == "neighbour" else V, ranges)
            out[b, ..., :2], out[b, ..., 4:] = rec[..., :2], rec[..., 4:]
        return 0
    return bad


def _harness_cases(hp, L, kinds):
    for kind, star in kinds:
        _att_run(hp, L, kind, 2, 2, 48, 36, 3, 9000, star)
        _att_run(hp, L, kind, 1, 2, 68, 36, 3, 9001, star, oproj=True)


def test_harness_notices_a_shifted_range_boundary(emulated_hip, monkeypatch):
    """The count and the float form each fail when the first key range takes one key of the second (and pass without)."""
    hp, L, device = _env("hip:0")
    for kind in (("count", None), ("float", None)):
        _harness_cases(hp, L, [kind])
    monkeypatch.setattr(L, "pdn_decode_attention_f32", _attention_with_defect(L, "boundary"))
    for kind in (("count", None), ("float", None)):
        with pytest.raises(AssertionError):
            _att_run(hp, L, kind[0], 2, 2, 48, 36, 3, 9000)
        with pytest.raises(AssertionError):
            _att_run(hp, L, kind[0], 1, 2, 68, 36, 3, 9001, oproj=True)


def test_harness_notices_a_key_paired_with_its_neighbours_value(emulated_hip, monkeypatch):
    """The select form (t* in the middle of a range, at its first key, the new key) and the float form each fail when key t
    is weighed against the value of key t - 1."""
    hp, L, device = _env("hip:0")
    kinds = (("select", 17), ("select", 13), ("select", -1), ("float", None))
    _harness_cases(hp, L, kinds)
    monkeypatch.setattr(L, "pdn_decode_attention_f32", _attention_with_defect(L, "neighbour"))
    for kind, star in kinds:
        with pytest.raises(AssertionError):
            _att_run(hp, L, kind, 2, 2, 48, 36, 3, 9000, star)
        with pytest.raises(AssertionError):
            _att_run(hp, L, kind, 1, 2, 68, 36, 3, 9001, star, oproj=True)


def test_harness_notices_a_write_by_a_stopped_row(emulated_hip, monkeypatch):
    """Every form fails when a stopped row leaves its key in cache slot 0 -- records and all else being right."""
    hp, L, device = _env("hip:0")
    from tests.abi_emulator import flat
    good = L.pdn_decode_attention_rows_f32

    def bad(qkv, rs, cos, sin, kc, vc, parts, B, H, hd, NS, cbs, pos, max_len, stream):
        rc = good(qkv, rs, cos, sin, kc, vc, parts, B, H, hd, NS, cbs, pos, max_len, stream)
        for b in np.flatnonzero(np.array(flat(pos, B, np.int32)) < 0):
            flat(kc + 4 * int(b) * cbs, H * hd)[...] = flat(qkv + 4 * (int(b) * rs + H * hd), H * hd)
        return rc
    for kind, star in (("count", None), ("select", -1), ("float", None)):
        _att_run(hp, L, kind, len(ROW_POS), 2, 48, ROW_POS, 4, 9002, star, rows=True)
    monkeypatch.setattr(L, "pdn_decode_attention_rows_f32", bad)
    for kind, star in (("count", None), ("select", -1), ("float", None)):
        with pytest.raises(AssertionError, match="cache outside the appended rows"):
            _att_run(hp, L, kind, len(ROW_POS), 2, 48, ROW_POS, 4, 9002, star, rows=True)
