"""label_smoothing and z_loss through the model: Llama.loss / token_losses / finetune_step on the 1-layer Llama of
tests/test_token_losses_llama.py (V 96, dim 288, 6 heads, ffn 768, L 32, B 2), emulated C ABI and (``-m gpu``) a real MI355X.

(a) loss(label_smoothing=0.1, z_loss=1e-2) and token_losses(...): values and every parameter gradient against the package's
    NumPy device; the criterion form equals the keyword form; keyword beside a criterion raises.
(b) A default-argument loss step issues the parent's entry points: counters, entry names and loss equal a run in which every
    pdnz_ entry and every function of core/fused/smooth_loss.py raises.
(c) 5 finetune_steps with z_loss at lr 1e-3 lower the batch's mean logsumexp^2."""
import ctypes

import numpy as np
import pytest

from pydynet_amd import _lib, nn
from pydynet_amd.core.fused import smooth_loss
from pydynet_amd.optim import Adam
from tests.conftest import device_variants
from tests.test_linear_ce import close, host
from tests.test_token_losses_llama import B, IGNORE, L, LR, V, _backward, _fused_nodes, _model

EPS, LAM = 0.1, 1e-2
_RUNTIME = ("malloc", "free", "memcpy", "memset", "event", "stream", "synchronize", "pool")


def _extend():
    from tests.abi_emulator import _loss, _rowloss, _segattn, _smoothloss
    _loss.extend()
    _segattn.extend()
    _rowloss.extend()
    _smoothloss.extend()                                  # (under the emulator: the pdnz_ entries of include/pdn_smoothloss.h)


def _batch(seed):
    rng = np.random.default_rng(seed)
    ids, tgt = rng.integers(0, V, (B, L)), rng.integers(0, V, (B, L))
    masked = tgt.copy()
    masked[0, :10], masked[1, :17] = IGNORE, IGNORE
    return ids, tgt, masked


def check_smoothed_losses_agree_with_the_numpy_device(dev):
    _extend()
    ids, tgt, masked = _batch(2)
    w = np.random.default_rng(3).standard_normal((B, L)).astype(np.float32)
    import pydynet_amd as pdn
    forms = {
        "loss": lambda m: m.loss(ids, tgt.reshape(-1), label_smoothing=EPS, z_loss=LAM),
        "masked loss": lambda m: m.loss(ids, masked.reshape(-1), ignore_index=IGNORE, label_smoothing=EPS, z_loss=LAM),
        "criterion": lambda m: m.loss(ids, masked.reshape(-1), nn.CrossEntropyLoss(ignore_index=IGNORE, label_smoothing=EPS, z_loss=LAM)),
        "sum criterion": lambda m: m.loss(ids, tgt.reshape(-1), nn.CrossEntropyLoss("sum", label_smoothing=EPS)),
        "rows": lambda m: (m.token_losses(ids, masked, ignore_index=IGNORE, label_smoothing=EPS, z_loss=LAM)
                           * pdn.Tensor(w, dtype=np.float32, device=m.lm_head.weight.device)).sum(),
    }

    def run(device):
        return {k: _backward(_model(device), f) for k, f in forms.items()}
    got, seen = _fused_nodes(lambda: run(dev))
    assert seen == [("mean", None), ("mean", IGNORE), ("mean", IGNORE), ("sum", None), ("none", IGNORE)], seen
    ref = run("cpu")
    for k in forms:
        print(k, got[k][0], "NumPy device", ref[k][0])
        close(np.array(got[k][0]), np.array(ref[k][0]), f"{k}: value against the NumPy device")
        assert set(got[k][1]) == set(ref[k][1]) and len(ref[k][1]) > 5
        for n in ref[k][1]:
            close(got[k][1][n], ref[k][1][n], f"{k}: grad {n} against the NumPy device")
    # the criterion form IS the keyword form
    assert got["criterion"][0] == got["masked loss"][0]
    for n in got["criterion"][1]:
        assert np.array_equal(got["criterion"][1][n], got["masked loss"][1][n]), n
    # the smoothed value differs from the plain one (the arguments reached the node)
    plain = _backward(_model(dev), lambda m: m.loss(ids, masked.reshape(-1), ignore_index=IGNORE))[0]
    assert abs(plain - got["masked loss"][0]) > 1e-2
    rows = host(_model(dev).token_losses(ids, masked, ignore_index=IGNORE, label_smoothing=EPS, z_loss=LAM))
    assert rows.shape == (B, L) and not rows[masked == IGNORE].any()
    close(np.array(rows.astype(np.float64).sum() / (masked != IGNORE).sum()), np.array(got["masked loss"][0]), "rows against the mean")
    m = _model(dev)
    for kw in ({"label_smoothing": EPS}, {"z_loss": LAM}):
        with pytest.raises(ValueError, match="criterion"):
            m.loss(ids, tgt.reshape(-1), nn.CrossEntropyLoss(), **kw)
        with pytest.raises(ValueError, match="criterion"):
            m.finetune_step(ids, tgt.reshape(-1), Adam(m.parameters(), lr=LR), nn.CrossEntropyLoss(), **kw)
    with pytest.raises(ValueError):
        m.loss(ids, tgt.reshape(-1), label_smoothing=1.5)
    with pytest.raises(TypeError):
        m.sequence_logprobs(ids, tgt, label_smoothing=EPS)      # a smoothed log-probability is not one


def _counters():
    buf = (ctypes.c_int64 * 46)()
    _lib.lib().call("pdn_kernel_counters", buf, 46, 1)
    return list(buf)


def check_default_loss_step_is_the_step_of_before(dev):
    _extend()
    ids, tgt, _ = _batch(4)
    tgt = tgt.reshape(-1)
    emu = _lib.lib()
    seen_calls, call = [], emu.call

    def one():
        m = _model(dev)
        opt = Adam(m.parameters(), lr=LR)
        m.finetune_step(ids, tgt, opt)                    # (first step: allocations, tables)
        _counters()
        del seen_calls[:]
        loss = m.finetune_step(ids, tgt, opt)
        calls = [n for n in seen_calls if not any(k in n for k in _RUNTIME) and n != "pdn_kernel_counters"]
        return loss, _counters(), calls
    emu.call = lambda name, *a: (seen_calls.append(name), call(name, *a))[1]
    try:
        base, seen = _fused_nodes(one)
    finally:
        del emu.call
    assert seen == [("mean", None)] * 2 and base[1][45] == 0 and base[1][44] == 0 and base[1][12] == 1 and base[1][13] == 1
    assert base[2] and not any(n.startswith("pdnz_") for n in base[2])

    def refuse(*a, **k):
        raise AssertionError("the smoothed loss ran in a step that never asked for it")
    names = [n for n in dir(smooth_loss) if callable(getattr(smooth_loss, n)) and getattr(getattr(smooth_loss, n), "__module__", "") == smooth_loss.__name__]
    assert {"rows", "dlogits", "cross_entropy", "linear_cross_entropy", "coefficients", "check_arguments", "value"} <= set(names)
    saved = {n: getattr(smooth_loss, n) for n in names}
    emu.call = lambda name, *a: refuse() if name.startswith("pdnz_") else (seen_calls.append(name), call(name, *a))[1]
    for n in saved:
        setattr(smooth_loss, n, refuse)
    try:
        again, seen = _fused_nodes(one)
    finally:
        del emu.call
        for n, f in saved.items():
            setattr(smooth_loss, n, f)
    assert again[0] == base[0] and again[1] == base[1] and again[2] == base[2]

    # ... and a smoothed step runs the same products, the pdnr_ backward and the pdnz_ entries around them
    def smoothed_step():
        m = _model(dev)
        opt = Adam(m.parameters(), lr=LR)
        _counters()
        m.finetune_step(ids, tgt, opt, label_smoothing=EPS, z_loss=LAM)
        return _counters()
    cnt, seen = _fused_nodes(smoothed_step)
    assert seen == [("mean", None)] and cnt[45] == 4 and cnt[44] == 1 and cnt[12] == 1 and cnt[13] == 1, (seen, cnt[45], cnt[44])


def check_z_loss_lowers_the_normaliser(dev):
    _extend()
    ids, tgt, _ = _batch(6)

    def five():
        m = _model(dev)
        opt = Adam(m.parameters(), lr=LR)

        def lse2():
            z = host(m.lm_head(m._forward_hidden(ids, 0))).astype(np.float64).reshape(B * L, V)
            return float((smooth_loss._lse(z) ** 2).mean())
        before = lse2()
        losses = [m.finetune_step(ids, tgt.reshape(-1), opt, z_loss=1.0) for _ in range(5)]
        return before, lse2(), losses
    (before, after, losses), seen = _fused_nodes(five)
    print("mean lse^2 before", before, "after 5 steps", after, "losses", losses)
    assert len(seen) == 5 and after < before and losses[-1] < losses[0]


for _f in (check_smoothed_losses_agree_with_the_numpy_device, check_default_loss_step_is_the_step_of_before,
           check_z_loss_lowers_the_normaliser):
    device_variants(globals(), _f)
