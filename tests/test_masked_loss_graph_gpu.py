"""A masked `finetune_step` inside a replayed hipnp.Graph: the count of valid tokens and its reciprocal live on the device, so the
replays follow a targets buffer whose mask -- and hence whose count -- changes between them, one of them down to a single valid
token.  Modelled on tests/test_grad_clip_graph_gpu.py; the model is tests/test_masked_llama.py's (the fused lm_head + loss
node with the masked finish and backward of include/pdn_loss.h)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

IGNORE = -100


def _targets():
    from tests.test_masked_llama import V, L, B
    rng = np.random.default_rng(9)
    base = rng.integers(0, V, (6, B * L))
    base[0, :10] = IGNORE                                 # the capture's own (warm-up + first replay): 54 valid tokens
    base[1, rng.random(B * L) < 0.5] = IGNORE             # about half
    base[2, :] = IGNORE
    base[2, 37] = 5                                       # a single valid token
    base[3, L:] = IGNORE                                  # the whole second sequence
    base[4, :] = base[4, :]                               # nothing ignored
    counts = [(row != IGNORE).sum() for row in base[:5]]
    assert counts[2] == 1 and len(set(counts)) == 5, counts
    return base[:5]


def trajectory(hip, use_graph):
    import pydynet_amd as pdn
    from pydynet_amd import hipnp
    from pydynet_amd.core import fused
    from pydynet_amd.optim import Adam
    from tests.test_masked_llama import _model, _fused_nodes, V, L, B, LR
    rng = np.random.default_rng(8)
    ids = rng.integers(0, V, (B, L))
    tgts = _targets()
    m = _model("hip:0")
    opt = Adam(m.parameters(), lr=LR)
    opt.flatten_grads()
    idd = pdn.Tensor(ids, dtype=np.int64, device="hip:0")
    tgd = pdn.Tensor(tgts[0], dtype=np.int64, device="hip:0")
    m.train(True)

    def step():
        opt.zero_grad()
        loss = m.loss(idd, tgd, ignore_index=IGNORE)
        loss.backward()
        opt.step()
        return loss

    def run():
        losses, reads = [], 0
        if use_graph:
            g = hip.Graph()
            get, count = hipnp.ndarray.get, [0]

            def counted(self, *a, **k):
                count[0] += 1
                return get(self, *a, **k)
            hipnp.ndarray.get = counted
            try:
                loss = g.capture(step)                    # steps 1 and 2 on the first targets
            finally:
                hipnp.ndarray.get = get
            reads = count[0]
            losses.append(loss.item())
            for row in tgts[1:]:
                tgd.data[...] = hip.from_numpy(row)
                g.replay()
                losses.append(loss.item())
            assert opt.t == 1 + 6
            g.destroy()
        else:
            step()
            losses.append(step().item())
            for row in tgts[1:]:
                tgd.data[...] = hip.from_numpy(row)
                losses.append(step().item())
        return losses, reads
    (losses, reads), seen = _fused_nodes(run)
    assert seen and all(i == IGNORE for i in seen), seen
    return losses, {n: p.numpy() for n, p in m.named_parameters()}, reads


def test_replayed_masked_steps_follow_the_targets_buffer(hip):
    eager, replayed = trajectory(hip, False), trajectory(hip, True)
    print("eager", eager[0], "replayed", replayed[0])
    assert replayed[2] == 0                               # the capture read nothing back to the host
    assert np.allclose(eager[0], replayed[0], rtol=1e-6), (eager[0], replayed[0])
    assert len(set(np.round(eager[0], 3))) == 5           # five different masks, five different losses
    for n in eager[1]:
        assert np.allclose(eager[1][n], replayed[1][n], rtol=1e-4, atol=2e-6), (n, float(np.abs(eager[1][n] - replayed[1][n]).max()))
