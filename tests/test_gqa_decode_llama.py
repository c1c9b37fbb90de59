"""Graph-replayed decode of a grouped-query Llama (llm/decode_plan.py, csrc/decode_gqa.hip): the 2-layer model of
tests/test_gqa_llama.py (vocabulary 64, dim 128, 4 heads over 2 key/value heads of 32) on the emulated C ABI and (``-m gpu``)
an MI355X.  Greedy `generate` and `generate_ragged`, 12 steps, at B = 2 (the five-launch form, six launches for a grouped
model) and B = 9 (the wide form), against the same model with the class switch fast_decode = False, the tape-node path:
the tokens of every step are equal, and the plan's logit rows of the last step -- behind twelve steps of its own cache
rows -- lie within 1e-4 of the reference's largest logit.  The reference's logits come from the operators that path runs
(`forward`, `_step_logits_rows`), and its top-2 margin is asserted to stay above 1e-3 of its largest logit at every step
(the seeds were chosen for that on the emulator), so a rounding difference cannot flip a token.  The new path must have run
(launch counter 56, the emulator's call log), a model with the default n_kv_heads must not touch it, and
include/pdn_gqdecode.h is held to header = exports = emulation."""
import subprocess

import numpy as np

from pydynet_amd import _lib
from pydynet_amd.autograd import set_grad_enabled
from pydynet_amd.core import Tensor
from pydynet_amd.core.tensor import Graph
from pydynet_amd.llm.llama import Llama
from tests.abi_emulator import _gqa, _gqdecode, counters
from tests.conftest import device_variants
from tests.test_llama_golden import host

V, DIM, HEADS, KV, FFN, L, STEPS = 64, 128, 4, 2, 256, 40, 12
_rng = np.random.default_rng(3)
IDS = _rng.integers(0, V, (9, 9))
LENS = [5, 9, 3, 7, 4, 8, 6, 9, 5]


def _model(dev, B, seed, kv=KV):
    _gqa.extend()
    _gqdecode.extend()                                    # (under the emulator: the pdnk_ and pdnj_ entries)
    Graph.clear()
    np.random.seed(seed)
    m = Llama(V, DIM, HEADS, FFN, L, B, 2, np.float32, n_kv_heads=kv)
    m.tok_embedding.weight.data[...] = (0.5 * np.random.randn(V, DIM)).astype(np.float32)
    m.to(dev)
    m.eval()
    return m


def _tokens(gen):
    return np.stack([host(t).reshape(-1) for t in gen])


def _generate(m, B, ragged, stop):
    if ragged:
        return _tokens(m.generate_ragged([IDS[b, :LENS[b]] for b in range(B)], STEPS, stop_ids=stop))
    return _tokens(m.generate(Tensor(IDS[:B, :7], dtype=np.int64, device=m.lm_head.weight.device), 7 + STEPS))


def _reference(ref, B, ragged, toks):
    """The logits of every decode step of the tape-node path, fed the tokens `toks` it yielded (-1: a stopped row)."""
    dev, lens, out = ref.lm_head.weight.device, np.array(LENS[:B]) if ragged else np.full(B, 7), []
    for i in range(1, STEPS):
        fed = Tensor(toks[i - 1].reshape(B, 1), dtype=np.int64, device=dev)
        if ragged:
            z = host(ref._step_logits_rows(fed, np.where(toks[i] >= 0, lens + i, -1)))
        else:
            z = host(ref.forward(fed, 7 + i))[:, -1]
        live = toks[i] >= 0
        top = np.sort(z[live], -1)
        assert np.all(top[:, -1] - top[:, -2] > 1e-3 * np.abs(z[live]).max()), (i, "the reference's margin")
        assert np.array_equal(z[live].argmax(-1), toks[i][live])
        out.append(z)
    return out


def _check(dev, B, ragged, seed, stop=()):
    Llama.fast_decode = False                             # (the tape-node path; put back below and by `_restoring`)
    ref = _model(dev, B, seed)
    want = _generate(ref, B, ragged, stop)
    ref_logits = _reference(ref, B, ragged, want)
    Llama.fast_decode = True
    m = _model(dev, B, seed)
    lib = _lib.lib()
    counters(57)
    mark = len(getattr(lib, "calls", ()))
    got = _generate(m, B, ragged, stop)
    assert got.shape == (STEPS, B) and np.array_equal(got, want), (got.T, want.T)
    cnt, calls = counters(57), list(getattr(lib, "calls", ()))[mark:]
    assert cnt[56] > 0 and cnt[31 if B > 8 else 56] > 0 and (not calls or "pdnj_decode_attention_f32" in calls)
    live = want[-1] >= 0                                  # (no step is queued behind the last: its logit rows are the plan's)
    z, zr = m._decode_st["logits"].get()[live], ref_logits[-1][live]
    err = float(np.abs(z - zr).max() / np.abs(zr).max())
    assert m._decode_st["gqa"] and m._decode_st["wide"] == (B > 8) and err <= 1e-4, err
    return want


def check_gqa_generate_b2(dev): _check(dev, 2, False, 11)
def check_gqa_generate_b9_wide(dev): _check(dev, 9, False, 11)
def check_gqa_generate_ragged_b2(dev): _check(dev, 2, True, 11)
def check_gqa_generate_ragged_b9_wide(dev): _check(dev, 9, True, 11)


def check_gqa_generate_ragged_stops_a_row(dev):
    Llama.fast_decode = False
    stop = [int(_generate(_model(dev, 2, 11), 2, True, ())[3, 0])]           # what row 0 yields at step 3
    want = _check(dev, 2, True, 11, stop)
    assert (want[4:, 0] == -1).all() and (want[:, 1] >= 0).any()


def check_default_kv_heads_keep_the_parents_decode(dev):
    m, lib = _model(dev, 2, 11, kv=None), _lib.lib()
    counters(57)
    mark = len(getattr(lib, "calls", ()))
    _generate(m, 2, False, ())
    cnt = counters(57)
    assert sum(cnt) > 0 and cnt[56] == 0 and not any(n.startswith("pdnj_") for n in list(getattr(lib, "calls", ()))[mark:])
    assert not m._decode_st["gqa"] and m._decode_st["qkv"].shape == (2, 3 * DIM)


def _restoring(fn):
    """`fn` with the class switch and the global grad mode (which Module.eval() turns off) put back behind it."""
    def run(dev):
        try:
            fn(dev)
        finally:
            Llama.fast_decode = True
            set_grad_enabled(True)
    run.__name__ = fn.__name__
    return run


for _f in (check_gqa_generate_b2, check_gqa_generate_b9_wide, check_gqa_generate_ragged_b2,
           check_gqa_generate_ragged_b9_wide, check_gqa_generate_ragged_stops_a_row,
           check_default_kv_heads_keep_the_parents_decode):
    device_variants(globals(), _restoring(_f))


def test_header_exports_and_emulator_agree(emulated_hip):
    protos = _lib.parse_header(_lib.GQDECODE_HEADER_PATHS[0])
    assert len(protos) == 2 and all(n.startswith("pdnj_") for n in protos) and not set(protos) & set(_lib.parse_header())
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if " T " in ln and ln.split()[-1].startswith("pdnj_")}
    assert exported == set(protos), exported ^ set(protos)
    assert {n for n in dir(_gqdecode.GqDecodeMixin) if n.startswith("pdnj_")} == set(protos) and not _gqdecode.NOT_EMULATED
    assert not any(_lib.provides(n) for n in protos)
    emu = _gqdecode.extend()
    assert isinstance(emu, _gqdecode.GqDecodeMixin) and _gqdecode.extend() is emu and all(_lib.provides(n) for n in protos)
