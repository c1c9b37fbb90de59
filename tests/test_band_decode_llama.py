"""Graph-replayed decode of a sliding-window Llama (llm/decode_plan.py, csrc/decode_band.hip): the 2-layer model, prompts
and reference of tests/test_gqa_decode_llama.py with sliding_window=8, multi-head and over 2 key/value heads, on the emulated
C ABI and (``-m gpu``) an MI355X.  Greedy `generate` (7-token prompts: the window fills at the first step and slides for the
rest) and `generate_ragged` (prompts of 3 .. 9 tokens: rows under and over the window), 12 steps, at B = 2 and B = 9 (wide),
against the same model with fast_decode = False: equal tokens at every step, the plan's last logit rows within 1e-4 of the
reference's largest logit.  `_reference` asserts the tape-node path's top-2 margin above 1e-3 of its largest logit at every
step -- a condition on the inputs: SEED was chosen for it on the emulator, with the tape-node path alone."""
import subprocess

import numpy as np

from pydynet_amd import _lib
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm.llama import Llama
from tests.abi_emulator import _banddecode, _gqa, _gqdecode, counters
from tests.conftest import device_variants
from tests.test_gqa_decode_llama import DIM, FFN, HEADS, L, STEPS, V, _generate, _reference, _restoring

WINDOW, SEED = 8, 1


def _model(dev, B, kv, window=WINDOW):
    _gqa.extend()
    _gqdecode.extend()
    _banddecode.extend()                                  # (under the emulator: the pdnk_, pdnj_ and pdnv_ entries)
    Graph.clear()
    np.random.seed(SEED)
    m = Llama(V, DIM, HEADS, FFN, L, B, 2, np.float32, n_kv_heads=kv, sliding_window=window)
    m.tok_embedding.weight.data[...] = (0.5 * np.random.randn(V, DIM)).astype(np.float32)
    m.to(dev)
    m.eval()
    return m


def _run(m, B, ragged):
    """The tokens of a generation, the launch counters it moved and the emulator's call log (empty on the GPU)."""
    lib = _lib.lib()
    counters(59)
    mark = len(getattr(lib, "calls", ()))
    toks = _generate(m, B, ragged, ())
    return toks, counters(59), list(getattr(lib, "calls", ()))[mark:]


def _check(dev, B, ragged, kv):
    Llama.fast_decode = False                             # (the tape-node path; put back below and by `_restoring`)
    ref = _model(dev, B, kv)
    want = _generate(ref, B, ragged, ())
    ref_logits = _reference(ref, B, ragged, want)
    Llama.fast_decode = True
    m = _model(dev, B, kv)
    got, cnt, calls = _run(m, B, ragged)
    assert got.shape == (STEPS, B) and np.array_equal(got, want), (got.T, want.T)
    assert cnt[58] > 0 and cnt[31 if B > 8 else 58] > 0 and cnt[56] == 0
    assert (not calls or "pdnv_decode_attention_f32" in calls) and not any(n.startswith("pdnj_") for n in calls)
    st = m._decode_st
    z, zr = st["logits"].get(), ref_logits[-1]            # (no step is queued behind the last: its logit rows are the plan's)
    err = float(np.abs(z - zr).max() / np.abs(zr).max())
    assert st["window"] == WINDOW and st["gqa"] == (kv is not None) and st["wide"] == (B > 8) and err <= 1e-4, err


def check_model_without_a_window_keeps_the_parents_decode(dev):
    m = _model(dev, 2, None, window=None)
    _, cnt, calls = _run(m, 2, False)
    assert sum(cnt) > 0 and cnt[58] == 0 and not any(n.startswith("pdnv_") for n in calls)
    assert m._decode_st["window"] is None and "window" not in m._decode_st["key"]


def _case(B, ragged, kv):
    fn = lambda dev: _check(dev, B, ragged, kv)
    fn.__name__ = "check_band_%s_b%d_%s" % ("generate_ragged" if ragged else "generate", B, "gqa" if kv else "mha")
    return fn


for _f in [_case(B, ragged, kv) for B in (2, 9) for ragged in (False, True) for kv in (None, 2)] + [
        check_model_without_a_window_keeps_the_parents_decode]:
    device_variants(globals(), _restoring(_f))


def test_header_exports_and_emulator_agree(emulated_hip):
    protos = _lib.parse_header(_lib.BANDDECODE_HEADER_PATHS[0])
    assert len(protos) == 2 and all(n.startswith("pdnv_") for n in protos) and not set(protos) & set(_lib.parse_header())
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("pdnv_")}
    assert exported == set(protos), exported ^ set(protos)
    assert {n for n in dir(_banddecode.BandDecodeMixin) if n.startswith("pdnv_")} == set(protos) and not _banddecode.NOT_EMULATED
    assert not any(_lib.provides(n) for n in protos)
    emu = _banddecode.extend()
    assert isinstance(emu, _banddecode.BandDecodeMixin) and _banddecode.extend() is emu and all(_lib.provides(n) for n in protos)
