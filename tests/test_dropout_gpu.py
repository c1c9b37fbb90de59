"""The kernels of csrc/dropout.hip on an MI355X, bit for bit against the statement (pydynet_amd/core/fused/dropout.py)."""
import functools

import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd.core import fused
from pydynet_amd.core.fused.dropout import blocks, dropout_np

pytestmark = pytest.mark.gpu

TWO_TRIPS = 4 * 256 * 4 * 2048 + 7        # 4 floats * DR_THREADS * DR_UNROLL * DR_GRID_CAP of csrc/dropout.hip: a second trip, ragged
SEED, START = 2 ** 40 + 11, 2 ** 32 - 2                       # (the counter carries into its high word inside a call)


@functools.lru_cache(maxsize=None)
def _inputs(n):
    rng = np.random.default_rng(n)
    return tuple(rng.standard_normal(n).astype(np.float32) for _ in range(3))


def _dev(a, grad=False):
    return pdn.Tensor(a, dtype=np.float32, device="hip:0", requires_grad=grad)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1025, TWO_TRIPS])
@pytest.mark.parametrize("p", [0, 0.1, 0.5, 0.9])
def test_forward_and_gradients_equal_the_statement(hip, p, n):
    xh, rh, wh = _inputs(n)
    gen = pdn.Generator(SEED, "hip:0")
    gen.set_state((SEED, START))
    x, r, w = _dev(xh, True), _dev(rh, True), _dev(wh)
    y = fused.dropout(x, p, gen)                              # two consecutive calls on one generator
    out = fused.dropout_add(x, r, p, gen)
    (y * w).sum().backward()
    dx_first = x.grad.get().copy()
    (out * w).sum().backward()
    o1 = START + blocks(n)
    if p == 0:
        assert y is x and gen.get_state() == (SEED, START)
        want = (xh, xh + rh, wh, wh)
    else:
        assert gen.get_state() == (SEED, START + 2 * blocks(n))
        want = (dropout_np(xh, p, SEED, START), dropout_np(xh, p, SEED, o1, residual=rh), dropout_np(wh, p, SEED, START),
                dropout_np(wh, p, SEED, o1))
    assert np.array_equal(y.data.get(), want[0]) and np.array_equal(out.data.get(), want[1])
    assert np.array_equal(dx_first, want[2]) and np.array_equal(x.grad.get(), want[2] + want[3]) and np.array_equal(r.grad.get(), wh)


def test_strided_and_misaligned_inputs(hip):
    xh = np.random.default_rng(1).standard_normal((37, 53)).astype(np.float32)
    gen = pdn.Generator(3, "hip:0")
    x = _dev(xh)
    y = fused.dropout(x.T, 0.5, gen)                          # non-contiguous: the node works on a contiguous copy
    assert np.array_equal(y.data.get(), dropout_np(xh.T, 0.5, 3, 0))
    flat, fh = x.reshape(-1), xh.reshape(-1)
    z = fused.dropout_add(flat[1:1030], flat[3:1032], 0.5, gen)     # contiguous views inside an array: 4-byte aligned only
    assert np.array_equal(z.data.get(), dropout_np(fh[1:1030], 0.5, 3, blocks(xh.size), residual=fh[3:1032]))


def test_replays_draw_fresh_masks_and_regenerate_them_backward(hip):
    n, p = 1025, 0.5
    xh, _, wh = _inputs(n)
    gen = pdn.Generator(9, "hip:0")
    x, w = _dev(xh, True), _dev(wh)

    def step():
        x.zero_grad()
        y = fused.dropout(x, p, gen)
        (y * w).sum().backward()
        return y, x.grad

    g = hip.Graph()
    y, dx = g.capture(step)                                   # (the warm-up and the capture's own replay: two claims)
    assert gen.get_state() == (9, 2 * blocks(n))
    seen = []
    for _ in range(2):
        o = gen.get_state()[1]
        g.replay()
        seen.append(y.data.get())
        assert np.array_equal(seen[-1], dropout_np(xh, p, 9, o)) and np.array_equal(dx.get(), dropout_np(wh, p, 9, o))
    assert not np.array_equal(seen[0], seen[1])
    g.destroy()
