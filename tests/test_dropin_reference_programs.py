"""Drop-in check: the reference's model file (llm/llama/model.py), as a user of the reference writes it -- RoPE and
attention with plain Tensor operators, 62 generic nodes per block -- executed on this backend.

The reference's source does not travel with this repository; its plain-operator formulation is restated, operator for
operator and with the same parameter names, in tests/models_plain_llama.py, and that file is what runs here: it must
reproduce the golden trajectory the real reference produced (tests/golden/tiny_llama.npz) and, at the benchmark width,
take every fused chain."""
import os

import numpy as np

G = os.path.join(os.path.dirname(__file__), "golden")


def _load_model_file():
    import pydynet                                   # the alias package of this repo
    assert pydynet.Tensor.__module__.startswith("pydynet_amd")
    from tests import models_plain_llama
    return models_plain_llama


def _run(dev):
    from pydynet_amd.optim import Adam
    from pydynet_amd.core.tensor import Graph
    Graph.clear()
    mod = _load_model_file()
    d = np.load(os.path.join(G, "tiny_llama.npz"))
    np.random.seed(1234)
    m = mod.PlainLlama(64, 48, 2, 96, 64, 2, np.float32)
    names = [k[5:] for k in d.files if k.startswith("init/")]
    for n in names:
        m._parameters[n].data[...] = d["init/" + n]
    m.to(dev)
    opt = Adam(m.parameters(), lr=1e-3)
    losses = [m.finetune_step(d["ids"], d["tgt"], opt) for _ in range(5)]
    assert np.allclose(losses, d["losses"], rtol=1e-4), (losses, d["losses"])
    for n in names:
        # five Adam steps: an entry whose gradient sits at round-off level may step differently (u = lr * m / (sqrt(v) +
        # eps)); all but a handful agree to the north-star tolerance (same criterion as tests/test_frontend_parity.py).
        # On the HIP device the reference's attention chain runs as one fused node (core/fused/chain.py): another
        # summation order than the plain operators.
        w, b = m._parameters[n].numpy(), d["final/" + n]
        err = np.abs(w.astype(np.float64) - b)
        bad = err > 1e-6 + 1e-4 * float(np.abs(b).max())
        assert bad.sum() <= max(1, w.size // 500) and float(err.max()) <= 2 * 1e-3 * 5, (n, int(bad.sum()), float(err.max()))


def test_reference_llama_file_runs_on_cpu_device():
    _run("cpu")


def test_reference_llama_file_runs_on_emulated_hip(emulated_hip):
    _run("hip:0")


def test_reference_llama_file_at_the_benchmark_width_takes_every_chain(emulated_hip):
    """The model file at width 288 (the width the fused loss node serves) with the row thresholds lowered: its
    `finetune_step` (model.py:226-252) must run the attention chain, `silu(gate) * up`, the rotary embedding and
    the `Linear -> reshape -> CrossEntropyLoss` loss as ONE node each (core/fused/chain.py) and reproduce the trajectory of
    the same file on the NumPy device."""
    from pydynet_amd.optim import Adam
    from pydynet_amd.core import fused
    from pydynet_amd.core.fused import chain
    from pydynet_amd.core.tensor import Graph
    mod = _load_model_file()
    rng = np.random.default_rng(0)
    V, D, H, FF, L, B = 64, 288, 6, 96, 16, 2
    ids, tgt = rng.integers(0, V, (B, L)), rng.integers(0, V, (B, L))
    saved = (fused.linear_relu.min_rows, fused.linear_cross_entropy.min_rows)
    fused.linear_relu.min_rows, fused.linear_cross_entropy.min_rows = 1, 32
    counts0 = (chain.attn_link.fused_built, chain.swiglu_chain.taken, chain.rope_link.fused_built, chain.loss_chain.fused_built)
    out = {}
    try:
        for dev in ("cpu", "hip:0"):
            Graph.clear()
            np.random.seed(99)
            m = mod.PlainLlama(V, D, H, FF, 64, 2, np.float32)
            m.tok_embedding.weight.data[...] = (0.02 * np.random.randn(V, D)).astype(np.float32)
            m.to(dev)
            opt = Adam(m.parameters(), lr=1e-3)
            out[dev] = [m.finetune_step(ids, tgt, opt) for _ in range(3)]
    finally:
        fused.linear_relu.min_rows, fused.linear_cross_entropy.min_rows = saved
    taken = [b - a for a, b in zip(counts0, (chain.attn_link.fused_built, chain.swiglu_chain.taken, chain.rope_link.fused_built,
                                              chain.loss_chain.fused_built))]
    assert taken == [2 * 3, 2 * 3, 2 * 2 * 3, 3], taken          # per step: 2 layers x (attention, swiglu, q and k rotations), 1 loss
    assert np.allclose(out["hip:0"], out["cpu"], rtol=1e-4), out
    assert out["cpu"][-1] < out["cpu"][0]
