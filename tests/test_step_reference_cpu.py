"""CPU: the one walker of tests/step_reference.py knows every layer kind the package's nn can build, and refuses what it does not know -- a chain with a kind that has no law,
and a leg that overrides a kind the network does not hold -- by name, instead of walking past it."""
import inspect
import types

import numpy as np
import pytest

import step_reference as S

nn = S.nn


def _buildable_kinds():
    """the kinds of nn's layer classes that hold parameters' shapes (the refusal-only names -- BatchNorm, InstanceNorm, Parallel -- and the flatten marker have none)"""
    return {c.kind for c in vars(nn).values() if inspect.isclass(c) and isinstance(getattr(c, "kind", None), str) and hasattr(c, "shapes")}


def test_every_kind_nn_can_build_has_a_law_and_block_names():
    kinds = _buildable_kinds()
    assert {"dense", "conv", "maxpool", "meanpool", "adaptivemaxpool", "adaptivemeanpool", "layernorm", "groupnorm", "dropout", "activation", "skip", "lstm", "gru", "rnn"} <= kinds
    assert kinds <= set(S.default_laws()), kinds - set(S.default_laws())
    assert kinds <= set(S.BLOCK_NAMES), kinds - set(S.BLOCK_NAMES)
    assert "act" in S.default_laws()      # the fused activation is an entry of its own


def test_a_chain_of_every_kind_is_walked_and_its_blocks_tile_the_parameters():
    net = nn.Chain(nn.Conv(3, 1, 4, nn.relu, pad=1), nn.MaxPool(2), nn.GroupNorm(4, 2), nn.SkipConnection(nn.Chain(nn.Conv(3, 4, 4, pad=1)), "+"), nn.MeanPool(1), nn.AdaptiveMaxPool(2),
                   nn.Activation(nn.gelu), nn.GlobalMeanPool(), nn.flattenbatch, nn.Dense(4, 6, nn.tanh), nn.LayerNorm(6), nn.Dropout(0.5), nn.LSTM(6, 5), nn.GRU(5, 4), nn.RNN(4, 3),
                   nn.Dense(3, 2))
    p = nn.glorot_params(net, seed=1).astype(np.float64) + 0.1
    q = S.q_values(net, p, np.random.default_rng(0).standard_normal((2, 3, 1, 8, 8)))
    assert len(q) == 2 and q[0].shape == (3, 2) and np.isfinite(q).all()
    blks = S.blocks(net)
    assert blks[0][1].start == 0 and blks[-1][1].stop == p.size and all(a[1].stop == b[1].start for a, b in zip(blks, blks[1:]))
    assert {nm.split(".")[0].rstrip("0123456789") for nm, _ in blks} == {"conv", "gn", "dense", "ln", "lstm", "gru", "rnn"}


def test_an_unknown_kind_is_refused_by_name():
    net = nn.Chain(nn.Dense(4, 4), nn.Dense(4, 2))
    net.layers.insert(1, types.SimpleNamespace(kind="batchnorm", act=nn.identity, shapes=lambda: []))
    with pytest.raises(ValueError, match="batchnorm"):
        S.q_step(net, [[], [], []], S._t64(np.zeros((1, 4))), {})
    inner = nn.Chain(nn.Dense(4, 4), nn.SkipConnection(nn.Chain(nn.Dense(4, 4)), "+"), nn.Dense(4, 2))
    inner.layers[1].layers.layers.append(types.SimpleNamespace(kind="parallel"))      # inside a block too
    with pytest.raises(ValueError, match="parallel"):
        S.laws_for(inner)


def test_a_leg_that_overrides_an_absent_kind_is_refused():
    net = nn.Chain(nn.Dense(4, 4, nn.relu), nn.Dense(4, 2)); p = nn.glorot_params(net, seed=1); x = np.ones((3, 4))
    law = S.default_laws()["layernorm"]
    with pytest.raises(ValueError, match="layernorm"):      # a real kind the network does not hold
        S.q_values(net, p, x, leg={"layernorm": law})
    with pytest.raises(ValueError, match="layer_norm"):      # a misspelt one
        S.q_values(net, p, x, leg={"layer_norm": law})
    with pytest.raises(ValueError, match="skip"):
        S.ff_step(net, p, p, (x, np.zeros(3, int), np.zeros(3), x, np.zeros(3), np.ones(3)), 0.9, True, leg={"skip": law})
    np.testing.assert_array_equal(S.q_values(net, p, x, leg={"act": S.default_laws()["act"], "dense": S.default_laws()["dense"]}), S.q_values(net, p, x))      # present kinds: accepted
