"""Clipped Adam, AdamW and a scheduled learning rate inside a replayed hipnp.Graph: a replayed step is the same step as the
eager one.  The model and inputs are tests/test_grad_clip.py's; a StepLR(step_size=2, gamma=0.5) is stepped after every
optimizer step, so from the third step on every step runs at a rate the capture never saw."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 6            # the capture runs steps 1 and 2 (warm-up + first replay), then four replays; losses 2..6 are compared


def trajectory(hip, make_opt, use_graph):
    import pydynet_amd.nn.functional as F
    from pydynet_amd.optim import StepLR
    from tests.test_grad_clip import build
    net, x, y = build("hip:0")
    opt = make_opt(list(net.parameters()))
    sched = StepLR(opt, step_size=2, gamma=0.5)

    def step():
        loss = F.cross_entropy_loss(net(x), y)
        opt.zero_grad(); loss.backward(); opt.step()
        return loss
    losses, norms, nodes = [], [], 0

    def record(loss):
        losses.append(loss.item())
        if opt.last_grad_norm is not None:
            norms.append(hip.read_later(opt.last_grad_norm).item())
    if use_graph:
        g = hip.Graph()
        loss = g.capture(step)                      # steps 1 and 2, both at the initial rate (as in the eager run: step_size 2)
        sched.step(); sched.step()
        record(loss)
        for _ in range(N - 2):
            g.replay()
            sched.step()
            record(loss)
        nodes = g.nodes
        assert opt.t == 1 + N
        g.destroy()
    else:
        for i in range(N):
            loss = step()
            sched.step()
            if i:                                   # (the graph run cannot read the warm-up step's loss)
                record(loss)
    assert opt.lr < 0.2 * 1e-2                      # the rate really moved
    return losses, {n: p.numpy() for n, p in net.named_parameters()}, norms, nodes, opt


def same(a, b):
    (l0, p0), (l1, p1) = a[:2], b[:2]
    assert np.allclose(l0, l1, rtol=1e-6), (l0, l1)
    for n in p0:
        assert np.allclose(p0[n], p1[n], rtol=1e-4, atol=2e-6), (n, float(np.abs(p0[n] - p1[n]).max()))


def test_replayed_clipped_steps_equal_eager_steps(hip):
    from pydynet_amd.optim import Adam
    from tests.test_grad_clip import MAX_NORM

    def clipped(ps):
        return Adam(ps, lr=1e-2, max_grad_norm=MAX_NORM)
    eager, replayed = trajectory(hip, clipped, False), trajectory(hip, clipped, True)
    same(eager, replayed)
    assert len(replayed[2]) == N - 1 and all(n > MAX_NORM for n in replayed[2]), replayed[2]      # every step clipped
    assert np.allclose(eager[2], replayed[2], rtol=1e-5)
    assert replayed[4].skipped_steps() == 0
    # the unclipped capture ends in 2 launches (tick, update); the clipped one in 3 (partials, finalize + tick, update):
    # ONE node more (counted on the MI355X: 22 against 21) -- the finalize launch replaces the tick one for one.  (The
    # requirement is at most 2.)
    plain = trajectory(hip, lambda ps: Adam(ps, lr=1e-2), True)
    print("graph nodes: clipped", replayed[3], "plain", plain[3])
    assert replayed[3] - plain[3] == 1


def test_replayed_steps_follow_the_scheduled_rate(hip):
    """Plain Adam, no new argument: before the replay hook pushed a changed rate to the device, the replays kept the rate of
    the capture and the parameters ended far from the eager run's."""
    from pydynet_amd.optim import Adam

    def plain(ps):
        return Adam(ps, lr=1e-2)
    same(trajectory(hip, plain, False), trajectory(hip, plain, True))


def test_replayed_adamw_steps_equal_eager_steps(hip):
    from pydynet_amd.optim import AdamW

    def adamw(ps):
        return AdamW(ps, lr=1e-2, weight_decay=0.1)
    same(trajectory(hip, adamw, False), trajectory(hip, adamw, True))


def test_clip_grad_norm_refuses_capture(hip):
    import pydynet_amd.nn.functional as F
    from pydynet_amd.nn.utils import clip_grad_norm_
    from pydynet_amd.optim import Adam
    from tests.test_grad_clip import build
    net, x, y = build("hip:0")
    params = list(net.parameters())
    opt = Adam(params, lr=1e-3)

    def step():
        loss = F.cross_entropy_loss(net(x), y)
        opt.zero_grad(); loss.backward()
        clip_grad_norm_(params, 1.0)
        opt.step()
        return loss
    g = hip.Graph()
    with pytest.raises(RuntimeError, match="clip_grad_norm_"):
        g.capture(step)
    g.destroy()
