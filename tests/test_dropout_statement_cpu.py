"""The statement of the device-drawn dropout (pydynet_amd/core/fused/dropout.py) on the NumPy device."""
import numpy as np
import pytest

import pydynet_amd as pdn
from pydynet_amd import nn, special
from pydynet_amd.core import fused
from pydynet_amd.core.fused.dropout import blocks, dropout_np, kept, philox4x32_10, scale


def test_philox_known_answer():
    # Random123 kat_vectors: philox4x32 10 rounds, counter 0, key 0
    assert [int(w) for w in philox4x32_10((0, 0, 0, 0), (0, 0))] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]


@pytest.mark.parametrize("n", [1, 5, 1025])
def test_node_equals_statement_and_claims_continue(n):
    seed, start, p = 2 ** 40 + 11, 2 ** 32 - 1, 0.3           # (the counter carries into its high word inside the call)
    gen = pdn.Generator(seed)
    gen.set_state((seed, start))
    x = pdn.Tensor(np.random.default_rng(n).standard_normal(n).astype(np.float32), requires_grad=True)
    r = pdn.Tensor(np.ones(n, np.float32), requires_grad=True)
    y = fused.dropout(x, p, gen)
    assert gen.get_state() == (seed, start + blocks(n))
    z = fused.dropout_add(x, r, p, gen)
    assert gen.get_state() == (seed, start + 2 * blocks(n))
    (y + z).sum().backward()                                  # (gradients of 1: s and 2 s are exact in any dtype the engine carries)
    k0, k1 = kept(n, p, seed, start), kept(n, p, seed, start + blocks(n))
    assert np.array_equal(y.data, np.where(k0, x.data * scale(p), np.float32(0))) and y.data.dtype == np.float32
    assert np.array_equal(z.data, dropout_np(x.data, p, seed, start + blocks(n), residual=r.data))
    assert np.array_equal(x.grad, scale(p) * (k0.astype(np.float32) + k1.astype(np.float32)))
    assert np.array_equal(r.grad, np.ones(n))
    gen.set_state((seed, start))                              # the state replays the mask
    assert np.array_equal(fused.dropout(x, p, gen).data, y.data)
    assert fused.dropout(x, 0, gen) is x and gen.get_state() == (seed, start + blocks(n))     # p = 0 claims nothing
    assert gen.manual_seed(5).get_state() == (5, 0)


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_kept_fraction(p):
    n = 2 ** 20
    assert abs(kept(n, p, 0, 0).mean() - (1 - p)) <= 5 * np.sqrt(p * (1 - p) / n)


def test_dropout_without_generator_draws_what_rand_draws():
    x = pdn.Tensor(np.random.default_rng(0).standard_normal((7, 9)))
    layer = nn.Dropout(0.4)
    np.random.seed(12)
    y = layer(x)
    np.random.seed(12)
    want = x.data * (special.rand(7, 9).data < 1 - 0.4).astype(x.dtype) / (1 - 0.4)
    assert np.array_equal(y.data, want)
    drawn = nn.Dropout(0.4, generator=pdn.Generator(1))(x)     # ... and with one, the statement (any floating dtype on "cpu")
    assert np.array_equal(drawn.data, dropout_np(x.data, 0.4, 1, 0))
