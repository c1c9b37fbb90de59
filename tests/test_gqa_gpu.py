"""The grouped-query attention kernels (csrc/attention_gqa.hip, include/pdn_gqattn.h) through the C ABI against a float64
NumPy statement written here: K / V repeated along the head axis, multi-head attention, dK / dV summed over each group.
Outputs are NaN-prefilled, so an element no workgroup writes fails.  Tolerance: the criterion of
tests/test_attention_stream_gpu.py for these fp32-MFMA kernels, max abs error <= 2e-5 x the reference's largest entry + 1e-7,
for o, lse, dq, dk and dv alike."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = [  # B, H, Hkv, Lq, Lk, hd, causal, start, mask
    (2, 4, 2, 64, 64, 48, 1, 0, None),        # G = 2, two tiles: the units fill the workgroups exactly
    (1, 6, 2, 100, 100, 48, 1, 0, None),      # G = 3: a workgroup straddles two query tiles; ragged tail
    (2, 8, 2, 40, 40, 64, 0, 0, "head"),      # a mask per QUERY head, (1, H, Lq, Lk)
    (2, 8, 1, 33, 33, 32, 1, 0, None),        # MQA, G = 8: two workgroups per tile, a one-row tail tile
    (2, 4, 2, 7, 39, 32, 1, 32, None),        # cache prefill: k / v are views into a (B, 64, Hkv, hd) buffer
    (3, 4, 1, 1, 17, 24, 0, 0, "pad"),        # the decode row of Attention.step_rows: padding mask (B, 1, 1, Lk)
    (1, 4, 2, 130, 130, 128, 1, 0, None),     # largest head dim, five tiles
    (1, 2, 1, 300, 300, 16, 1, 0, None),      # dK/dV workgroups beyond the first; smallest head dim
]
CACHE_ROWS = 64


def _ref(q, k, v, do, causal, start, mask):
    B, Lq, H, hd = q.shape
    Lk, G = k.shape[1], H // k.shape[2]
    Q, DO = (a.astype(np.float64).transpose(0, 2, 1, 3) for a in (q, do))
    K, V = (np.repeat(a.astype(np.float64), G, axis=2).transpose(0, 2, 1, 3) for a in (k, v))
    s = Q @ K.swapaxes(-1, -2) / math.sqrt(hd)
    if causal:
        s = s + np.where(np.arange(Lk)[None, :] > np.arange(Lq)[:, None] + start, -np.inf, 0.0)
    if mask is not None:
        s = s + mask.astype(np.float64)
    m = s.max(-1, keepdims=True)
    e = np.exp(s - m)
    l = e.sum(-1, keepdims=True)
    p = e / l
    dp = DO @ V.swapaxes(-1, -2)
    ds = p * (dp - (dp * p).sum(-1, keepdims=True)) / math.sqrt(hd)
    tr = lambda a: a.transpose(0, 2, 1, 3)                                            # noqa: E731
    group = lambda a: tr(a).reshape(B, Lk, H // G, G, hd).sum(3)                      # noqa: E731
    return tr(p @ V), (m + np.log(l))[..., 0], tr(ds @ K), group(ds.swapaxes(-1, -2) @ Q), group(p.swapaxes(-1, -2) @ DO)


def _run(hip, case, twice=False):
    from pydynet_amd import _lib
    L = _lib.lib()
    B, H, Hkv, Lq, Lk, hd, causal, start, mkind = case
    rng = np.random.default_rng(sum(case[:8]))
    mk = lambda n, h: rng.standard_normal((B, n, h, hd), dtype=np.float32)            # noqa: E731
    q, k, v, do = mk(Lq, H), mk(Lk, Hkv), mk(Lk, Hkv), mk(Lq, H)
    mask = None
    if mkind == "head":
        mask = rng.standard_normal((1, H, Lq, Lk), dtype=np.float32)
    elif mkind == "pad":
        mask = np.where(np.arange(Lk)[None, :] > (Lk - 1 - 5 * np.arange(B))[:, None], -np.inf, 0.0)
        mask = mask.astype(np.float32).reshape(B, 1, 1, Lk)
    nan = lambda shape: hip.from_numpy(np.full(shape, np.nan, np.float32))            # noqa: E731
    Q, DO = hip.from_numpy(q), hip.from_numpy(do)
    Dq, Dk = H * hd, Hkv * hd
    if start:                                 # the keys live in the first Lk rows of a larger cache
        Kc, Vc = nan((B, CACHE_ROWS, Hkv, hd)), nan((B, CACHE_ROWS, Hkv, hd))
        Kc[:, :Lk], Vc[:, :Lk] = hip.from_numpy(k), hip.from_numpy(v)
        K, V, kv_bs = Kc[:, :Lk], Vc[:, :Lk], CACHE_ROWS * Dk
    else:
        K, V, kv_bs = hip.from_numpy(k), hip.from_numpy(v), Lk * Dk
    margs = [None, 0, 0, 0, 0]
    if mask is not None:
        Mdev = hip.from_numpy(mask)
        margs = [Mdev._ptr] + [0 if s == 1 else t for s, t in zip(mask.shape, Mdev._strides)]
    O, LSE = nan(q.shape), nan((B, H, Lq))
    assert L.query("pdnk_attention_supported", hd, H, Hkv) == 1
    L.call("pdnk_attention_fwd_f32", Q._ptr, K._ptr, V._ptr, O._ptr, LSE._ptr, B, H, Hkv, Lq, Lk, hd, Dq, Lq * Dq, Dk, kv_bs,
           causal, start, *margs, hip.stream())
    ws, wsb = hip.workspace(L.query("pdnk_attention_bwd_workspace_bytes", B, H, Lq))
    grads = []
    for _ in range(2 if twice else 1):
        # (gradients are written with the operand strides: contiguous k / v for the backward, as fused.attention gives it)
        Kb, Vb = hip.from_numpy(k), hip.from_numpy(v)
        DQ, DK, DV = nan(q.shape), nan(k.shape), nan(v.shape)
        L.call("pdnk_attention_bwd_f32", Q._ptr, Kb._ptr, Vb._ptr, O._ptr, DO._ptr, LSE._ptr, DQ._ptr, DK._ptr, DV._ptr,
               B, H, Hkv, Lq, Lk, hd, Dq, Lq * Dq, Dk, Lk * Dk, causal, start, *margs, ws, wsb, hip.stream())
        grads.append((DQ.get(), DK.get(), DV.get()))
    return (O.get(), LSE.get()) + grads[0], grads, _ref(q, k, v, do, causal, start, mask)


@pytest.mark.parametrize("case", CASES)
def test_gqa_kernels_match_float64(hip, case):
    got, _, ref = _run(hip, case)
    for what, a, b in zip(("o", "lse", "dq", "dk", "dv"), got, ref):
        scale = float(np.abs(b).max())
        err = float(np.abs(a.astype(np.float64) - b).max())       # (NaN where nothing was written: fails)
        print(f"{case} {what}: err {err:.3e} scale {scale:.3e} ratio {err / scale:.3e}")
        assert a.shape == b.shape and err <= 2e-5 * scale + 1e-7, (what, err, scale)


def test_gqa_backward_is_deterministic(hip):
    _, (first, second), _ = _run(hip, CASES[1], twice=True)
    assert all(np.array_equal(a, b) and np.isfinite(a).all() for a, b in zip(first, second))


def test_gqa_supported_declines_other_groups_and_head_dims(hip):
    from pydynet_amd import _lib
    L = _lib.lib()
    assert [L.query("pdnk_attention_supported", hd, H, Hkv) for hd, H, Hkv in ((48, 4, 4), (48, 16, 1), (40, 4, 2), (48, 6, 2))] \
        == [0, 0, 0, 1]
