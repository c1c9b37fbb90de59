"""core/fused/gqa.py (the statement of grouped-query attention) against a float64 repeat-and-sum written here, the `cpu`
device of `fused.attention` against the statement, the ValueErrors of the operator and the model, the checkpoint round trip
of a grouped model, and include/pdn_gqattn.h (prefix pdnk_) held to header = exports = emulation."""
import subprocess

import numpy as np
import pytest

from pydynet_amd import _lib
from pydynet_amd.core import Tensor, fused
from pydynet_amd.core.fused import gqa
from pydynet_amd.llm import io
from pydynet_amd.llm.llama import Llama


@pytest.mark.parametrize("Hkv,start", [(2, 0), (2, 5), (1, 0), (1, 5)])           # 4 heads: G = 2 and G = 4
def test_statement_is_repeat_attend_and_group_sum(Hkv, start):
    rng = np.random.default_rng(Hkv + start)
    B, H, Lq, hd = 2, 4, 6, 8
    Lk, G = Lq + start, H // Hkv
    q, do = rng.standard_normal((2, B, Lq, H, hd))
    k, v = rng.standard_normal((2, B, Lk, Hkv, hd))
    mask = rng.standard_normal((1, H, Lq, Lk))
    o, lse, p = gqa.forward(q, k, v, True, start, mask)
    dq, dk, dv = gqa.backward(q, k, v, p, do)
    Q, DO = q.transpose(0, 2, 1, 3), do.transpose(0, 2, 1, 3)
    K, Vx = (np.stack([a[:, :, h // G] for h in range(H)], 1) for a in (k, v))       # (B, H, Lk, hd): head h reads h // G
    s = Q @ K.swapaxes(-1, -2) / np.sqrt(hd) + mask
    s = s + np.where(np.arange(Lk)[None, :] > np.arange(Lq)[:, None] + start, -np.inf, 0.0)
    e = np.exp(s - s.max(-1, keepdims=True))
    pr = e / e.sum(-1, keepdims=True)
    dp = DO @ Vx.swapaxes(-1, -2)
    ds = pr * (dp - (dp * pr).sum(-1, keepdims=True)) / np.sqrt(hd)
    group = lambda a: a.reshape(B, Hkv, G, Lk, hd).sum(2).transpose(0, 2, 1, 3)     # noqa: E731
    for got, ref in ((o, (pr @ Vx).transpose(0, 2, 1, 3)), (lse, np.log(e.sum(-1)) + s.max(-1)),
                     (dq, (ds @ K).transpose(0, 2, 1, 3)), (dk, group(ds.swapaxes(-1, -2) @ Q)),
                     (dv, group(pr.swapaxes(-1, -2) @ DO))):
        assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    # the operator on `cpu` is the statement
    tq, tk, tv = (Tensor(a, requires_grad=True) for a in (q, k, v))
    out = fused.attention(tq, tk, tv, causal=True, start_pos=start, mask=mask)
    (out * Tensor(do)).sum().backward()
    for got, ref in ((out.data, o), (tq.grad, dq), (tk.grad, dk), (tv.grad, dv)):
        assert got.shape == ref.shape and np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


def test_value_errors_and_checkpoint_round_trip(tmp_path):
    t = lambda h: Tensor(np.zeros((1, 4, h, 8)))                                     # noqa: E731
    with pytest.raises(ValueError):
        fused.attention(t(4), t(3), t(3))
    with pytest.raises(ValueError):
        fused.attention(t(4), t(2), t(2), segment_ids=np.zeros((1, 4), np.int64))
    for bad in (3, 0, 8):
        with pytest.raises(ValueError):
            Llama(16, 32, 4, 64, 8, 1, 1, np.float32, n_kv_heads=bad)
    np.random.seed(0)
    a, b = (Llama(16, 32, 4, 64, 8, 1, 1, np.float32, n_kv_heads=2) for _ in range(2))
    assert a.layers[0].attention.K.weight.shape == (32, 16) and a.layers[0].attention.cache_v.shape == (1, 8, 2, 8)
    with pytest.raises(ValueError):
        a.loss(np.zeros((1, 8), np.int64), np.zeros(8, np.int64), segment_ids=np.zeros((1, 8), np.int64))
    for m in (a, b):
        m.tok_embedding.weight.data[...] = 0.5                                      # (the table starts unset)
    path = str(tmp_path / "gqa.npz")
    io.save_finetuned_parameters(a, path)
    io.load_finetuned_parameters(b, path)
    assert all(np.array_equal(p.numpy(), q.numpy()) for (_, p), (_, q) in zip(a.named_parameters(), b.named_parameters()))
    with pytest.raises(ValueError):                                                  # a multi-head model refuses the file
        io.load_finetuned_parameters(Llama(16, 32, 4, 64, 8, 1, 1, np.float32), path)


def test_header_exports_and_emulator_agree(emulated_hip):
    from tests.abi_emulator import _gqa
    protos = _lib.parse_header(_lib.GQA_HEADER_PATHS[0])
    assert len(protos) == 4 and all(n.startswith("pdnk_") for n in protos) and not set(protos) & set(_lib.parse_header())
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("pdnk_")}
    assert exported == set(protos), exported ^ set(protos)
    emulated = {n for n in dir(_gqa.GqaMixin) if n.startswith("pdnk_")}
    assert emulated == set(protos) and not _gqa.NOT_EMULATED and not any(_lib.provides(n) for n in protos)
    emu = _gqa.extend()
    assert isinstance(emu, _gqa.GqaMixin) and _gqa.extend() is emu and all(_lib.provides(n) for n in protos)
