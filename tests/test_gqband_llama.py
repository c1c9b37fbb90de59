"""`Llama(..., n_kv_heads=, sliding_window=)`, the Mistral layer: the 2-layer Llama of tests/test_band_llama.py (vocabulary 64,
dim 128, 4 heads of 32, ffn 256, sequence 40, batch 2, window 12) over 2 key/value heads, on the emulated C ABI and
(``-m gpu``) an MI355X: (a) loss and every parameter gradient of one backward against the same model on the `cpu` device,
within the project's fp32 bound of 1e-4 relative; on the device both attention nodes run the windowed shared-K/V kernels of
include/pdn_gqbandattn.h (`_kind == "gqband"`, launch counter slot 59), under the emulator, which has no such entry, the
window runs as a mask; (b) the same model without a window, and a windowed model without n_kv_heads, keep the kernels they
had ("gqa" / "band") and leave slot 59 at 0."""
import ctypes

from pydynet_amd import _lib
from tests.abi_emulator import _gqa
from tests.conftest import device_variants
from tests.test_band_llama import W, _loss_and_grads, _model
from tests.test_gqa_llama import KV, _close


def _slot59():
    buf = (ctypes.c_int64 * 60)()
    _lib.lib().call("pdn_kernel_counters", buf, 60, 1)
    return buf[59]


def check_gqband_llama(dev):
    _gqa.extend()                                         # (under the emulator: the pdnk_ entries, which run the window as a mask)
    on_device = _lib.provides("pdnm_attention_fwd_f32")
    _slot59()
    loss, grads, nodes = _loss_and_grads(_model(dev, n_kv_heads=KV, sliding_window=W))
    assert len(nodes) == 2 and all(n.window == W for n in nodes)
    if on_device:
        assert all(n._kind == "gqband" for n in nodes) and _slot59() > 0
    else:
        assert all(n._kind == "gqa" for n in nodes) and _slot59() == 0
    ref_loss, ref_grads, _ = _loss_and_grads(_model("cpu", n_kv_heads=KV, sliding_window=W))
    assert abs(loss - ref_loss) <= 1e-4 * abs(ref_loss)
    for name, g in grads.items():
        _close(g, ref_grads[name], name)


def check_unchanged_models_keep_their_kernels(dev):
    _gqa.extend()
    _slot59()
    for kw, kind in ((dict(n_kv_heads=KV), "gqa"), (dict(sliding_window=W), "band")):
        nodes = _loss_and_grads(_model(dev, **kw))[2]
        if kind == "gqa" or _lib.provides("pdnb_attention_fwd_f32"):          # (the emulator runs a band as a mask)
            assert len(nodes) == 2 and all(n._kind == kind for n in nodes), kw
        assert _slot59() == 0, kw


for _f in (check_gqband_llama, check_unchanged_models_keep_their_kernels):
    device_variants(globals(), _f)
