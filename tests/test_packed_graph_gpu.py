"""A packed `finetune_step` inside a replayed hipnp.Graph: the documents' bounds are made on the device from the `segment_ids`
buffer at every replay, so the replays follow a packing that changes between them -- ids, targets and segment ids rewritten in
place.  Modelled on tests/test_masked_loss_graph_gpu.py; the model is tests/test_packed_llama.py's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

IGNORE = -100


def _batches():
    from pydynet_amd.llm.packing import pack_sequences
    from tests.test_packed_llama import V, L
    rng = np.random.default_rng(41)
    out = []
    for lens in ((20, 33, 7, 40, 9, 11), (3, 58, 61, 2), (64, 30, 30), (17,) * 7):
        docs = [rng.integers(1, V, n) for n in lens]
        ids, tgt, seg = pack_sequences(docs, L, pad_id=0, ignore_index=IGNORE)
        assert ids.shape[0] >= 2
        out.append((ids[:2], tgt[:2].reshape(-1), seg[:2]))
    assert len({b[2].tobytes() for b in out}) == len(out)            # four different packings
    return out


def trajectory(hip, use_graph):
    import pydynet_amd as pdn
    from pydynet_amd import hipnp
    from pydynet_amd.optim import Adam
    from tests.test_packed_llama import _model, _counters, LR
    batches = _batches()
    m = _model("hip:0", 2)
    opt = Adam(m.parameters(), lr=LR)
    opt.flatten_grads()
    ids0, tgt0, seg0 = batches[0]
    idd = pdn.Tensor(ids0, dtype=np.int64, device="hip:0")
    tgd = pdn.Tensor(tgt0, dtype=np.int64, device="hip:0")
    sgd = hip.asarray(seg0.astype(np.int32))                         # the form a captured step re-reads
    m.train(True)

    def step():
        opt.zero_grad()
        loss = m.loss(idd, tgd, ignore_index=IGNORE, segment_ids=sgd)
        loss.backward()
        opt.step()
        return loss

    def load(batch):
        idd.data[...] = hip.from_numpy(batch[0])
        tgd.data[...] = hip.from_numpy(batch[1])
        sgd[...] = hip.from_numpy(batch[2].astype(np.int32))

    losses, reads = [], 0
    _counters()
    if use_graph:
        g = hip.Graph()
        get, count = hipnp.ndarray.get, [0]

        def counted(self, *a, **k):
            count[0] += 1
            return get(self, *a, **k)
        hipnp.ndarray.get = counted
        try:
            loss = g.capture(step)                                   # steps 1 and 2 on the first packing
        finally:
            hipnp.ndarray.get = get
        reads = count[0]
        losses.append(loss.item())
        for batch in batches[1:]:
            load(batch)
            g.replay()
            losses.append(loss.item())
        g.destroy()
    else:
        step()
        losses.append(step().item())
        for batch in batches[1:]:
            load(batch)
            losses.append(step().item())
    cnt = _counters()
    assert cnt[43] > 0 and cnt[7] == 0 and cnt[8] == 0, cnt          # the segmented kernels, never the persistent ones
    hip.check_index_errors()                                         # no row decreased
    return losses, {n: p.numpy() for n, p in m.named_parameters()}, reads


def test_replayed_packed_steps_follow_the_segment_buffer(hip):
    eager, replayed = trajectory(hip, False), trajectory(hip, True)
    print("eager", eager[0], "replayed", replayed[0])
    assert replayed[2] == 0                                          # the capture read nothing back to the host
    assert np.allclose(eager[0], replayed[0], rtol=1e-6), (eager[0], replayed[0])
    assert len(set(np.round(eager[0], 3))) == 4                      # four packings, four losses
    for n in eager[1]:
        assert np.allclose(eager[1][n], replayed[1][n], rtol=1e-4, atol=2e-6), (n, float(np.abs(eager[1][n] - replayed[1][n]).max()))
