"""CPU: the fp64 reference for any recurrent chain (tests/recurrent_reference.py), which tests/test_recurrent_edges_gpu.py checks the engine
against, pinned to torch's cells, to the single-kind references (gru_reference.py, rnn_reference.py), to the NumPy oracle's LSTM, to central finite
differences on a mixed chain and to the oracle's Adam; and the C twin against the oracle on stacked LSTMs."""
import importlib
import types

import numpy as np
import pytest
import torch

import __graft_entry__ as ge
import dqn_oracle as O
import gru_reference as GR
import recurrent_reference as R
import ref
import rnn_reference as RR
from drqn_common import check_against_oracle, draws, feed, make_episodes, make_handle, oracle_recur_state

F64 = torch.float64


@pytest.fixture(scope="module")
def nn():
    return importlib.import_module(ge.load_package().__name__ + ".nn")


def _cell_case(torch_cell, n_gates, seed=0):
    rng = np.random.default_rng(seed)
    n_in, H, B = 7, 5, 4
    Wi, Wh, b = rng.standard_normal((n_gates * H, n_in)), rng.standard_normal((n_gates * H, H)), rng.standard_normal(n_gates * H)
    cell = torch_cell.double()
    with torch.no_grad():
        cell.weight_ih.copy_(torch.tensor(Wi)); cell.weight_hh.copy_(torch.tensor(Wh)); cell.bias_ih.copy_(torch.tensor(b)); cell.bias_hh.zero_()
    xs = [torch.tensor(rng.standard_normal((B, n_in))) for _ in range(6)]
    return cell, (torch.tensor(Wi.T.copy()), torch.tensor(Wh.T.copy()), torch.tensor(b)), xs, rng, B, H


def test_lstm_cell_equals_torch_lstmcell():
    """the reference's LSTM cell (gates i, f, g, o) is torch.nn.LSTMCell with weight_ih = Wi, weight_hh = Wh, bias_ih = b, bias_hh = 0"""
    cell, (Wi, Wh, b), xs, rng, B, H = _cell_case(torch.nn.LSTMCell(7, 5), 4)
    h = h_ref = torch.tensor(rng.standard_normal((B, H))); c = c_ref = torch.tensor(rng.standard_normal((B, H)))
    with torch.no_grad():
        for x in xs:
            h_ref, c_ref = cell(x, (h_ref, c_ref))
            h, c = R.lstm_cell(x, h, c, Wi, Wh, b)
            np.testing.assert_allclose(h.numpy(), h_ref.numpy(), rtol=1e-13, atol=1e-13)
            np.testing.assert_allclose(c.numpy(), c_ref.numpy(), rtol=1e-13, atol=1e-13)


def test_gru_and_rnn_cells_equal_torch_cells():
    """the chain steps of the reference reach torch.nn.GRUCell and torch.nn.RNNCell (tanh, relu) through the cells they share with gru_reference / rnn_reference"""
    cases = [(torch.nn.GRUCell(7, 5), 3, types.SimpleNamespace(kind="gru", act=0)),
             (torch.nn.RNNCell(7, 5, nonlinearity="tanh"), 1, types.SimpleNamespace(kind="rnn", act=2)),
             (torch.nn.RNNCell(7, 5, nonlinearity="relu"), 1, types.SimpleNamespace(kind="rnn", act=1))]
    for tc, ng, layer in cases:
        cell, (Wi, Wh, b), xs, rng, B, H = _cell_case(tc, ng)
        hs = {0: torch.tensor(rng.standard_normal((B, H)))}; h_ref = hs[0]
        with torch.no_grad():
            for x in xs:
                h_ref = cell(x, h_ref)
                y = R._chain_step([layer], [[Wi, Wh, b]], x, hs, 0)
                np.testing.assert_allclose(y.numpy(), h_ref.numpy(), rtol=1e-13, atol=1e-13)
                np.testing.assert_allclose(hs[0].numpy(), h_ref.numpy(), rtol=1e-13, atol=1e-13)


def _ring_and_batch(net, nn, E, nA, B, T, seed):
    rng = np.random.default_rng(seed)
    spec = types.SimpleNamespace(obs_shape=(E,), n_actions=nA)
    ring = make_episodes(spec, max(12, B + 4), T, rng)
    idx, start = draws(ring, B, rng)
    n = nn.glorot_params(net, seed=3).size
    p_on = (nn.glorot_params(net, seed=3) + 0.05 * rng.standard_normal(n)).astype(np.float32)
    p_tg = (nn.glorot_params(net, seed=4) + 0.05 * rng.standard_normal(n)).astype(np.float32)
    return R.sample_batch(ring, idx, start, T, (E,)), p_on, p_tg


SINGLE_KIND = {      # name -> (builder, E, nA, B, T, gamma, double_q, single-kind reference)
    "gru_plain": (lambda nn: nn.Chain(nn.GRU(6, 16), nn.Dense(16, 4)), 6, 4, 5, 6, 0.95, 1, GR),
    "dense_gru_dueling": (lambda nn: nn.create_dueling_network(nn.Chain(nn.Dense(6, 12, nn.relu), nn.GRU(12, 16), nn.Dense(16, 5))), 6, 5, 6, 5, 0.9, 1, GR),
    "gru_gru": (lambda nn: nn.Chain(nn.GRU(6, 10), nn.GRU(10, 8), nn.Dense(8, 3)), 6, 3, 4, 7, 0.9, 0, GR),
    "rnn_sigmoid": (lambda nn: nn.Chain(nn.RNN(6, 8, nn.sigmoid), nn.Dense(8, 3)), 6, 3, 5, 3, 0.9, 0, RR),
    "rnn_relu_dueling": (lambda nn: nn.create_dueling_network(nn.Chain(nn.Dense(6, 12, nn.relu), nn.RNN(12, 16, nn.relu), nn.Dense(16, 5))), 6, 5, 6, 5, 0.95, 1, RR),
    "rnn_stack_identity_tanh": (lambda nn: nn.Chain(nn.RNN(6, 9, nn.identity), nn.RNN(9, 7), nn.Dense(7, 4)), 6, 4, 3, 9, 0.99, 1, RR),
}


@pytest.mark.parametrize("name", list(SINGLE_KIND))
def test_single_kind_chains_equal_their_references(nn, name):
    mk, E, nA, B, T, gamma, dq, S = SINGLE_KIND[name]
    net = mk(nn)
    batch, p_on, p_tg = _ring_and_batch(net, nn, E, nA, B, T, 7)
    got = R.train_grads(net, nn, p_on, p_tg, batch, gamma, dq)
    want = S.drqn_train_step(net, nn, p_on, p_tg, batch, gamma, dq)
    np.testing.assert_allclose(got["loss"], want["loss"], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(got["grads"], want["grads"], rtol=1e-12, atol=1e-12 * np.abs(want["grads"]).max())
    assert got["grad_norm"] == pytest.approx(want["grad_norm"], rel=1e-12)
    # the policy step and its state
    rng = np.random.default_rng(1)
    xs = [torch.tensor(rng.random((3, E))) for _ in range(4)]
    with torch.no_grad():
        arrs = GR.param_arrays(net, nn, p_on)
        qa, ha = R.seq_q(net, nn, arrs, xs); qb, hb = S.seq_q(net, nn, arrs, xs)
    for a, b in zip(qa, qb):
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=1e-12, atol=1e-14)
    assert sorted(ha) == sorted(hb)
    for i in ha:
        np.testing.assert_allclose(ha[i].numpy(), hb[i].numpy(), rtol=1e-12, atol=1e-14)


def _oracle_net(nn, net, E):
    """nn descriptors -> the NumPy oracle's RecurrentNetwork (LSTM / Dense), same Flux.params order"""
    conv = lambda ls: [O.LSTM(l.n_in, l.n_out) if l.kind == "lstm" else O.Dense(l.n_in, l.n_out, l.act) for l in ls]
    if isinstance(net, nn.DuelingNetwork):
        return O.RecurrentNetwork((E,), conv(net.base), conv(net.val), conv(net.adv))
    return O.RecurrentNetwork((E,), conv(net.layers))


LSTM_CHAINS = {
    "lstm_plain": (lambda nn: nn.Chain(nn.LSTM(6, 8), nn.Dense(8, 3)), 6, 3, 4, 5, 0.9, 0),
    "lstm_lstm": (lambda nn: nn.Chain(nn.LSTM(6, 12), nn.LSTM(12, 8), nn.Dense(8, 4)), 6, 4, 5, 6, 0.95, 1),
    "lstm_dense_lstm_dueling": (lambda nn: nn.create_dueling_network(nn.Chain(nn.LSTM(6, 10), nn.Dense(10, 12, nn.tanh), nn.LSTM(12, 8), nn.Dense(8, 5))), 6, 5, 6, 4, 0.99, 1),
}


@pytest.mark.parametrize("name", list(LSTM_CHAINS))
def test_lstm_chains_equal_the_numpy_oracle(nn, name):
    mk, E, nA, B, T, gamma, dq = LSTM_CHAINS[name]
    net = mk(nn)
    batch, p_on, p_tg = _ring_and_batch(net, nn, E, nA, B, T, 8)
    got = R.train_grads(net, nn, p_on, p_tg, batch, gamma, dq)
    onet = _oracle_net(nn, net, E)
    s, a, r, sp, d, m = batch
    o = O.drqn_train_step(onet, onet.unflatten(p_on), onet.unflatten(p_tg), (list(s), list(a), list(r), list(sp), list(d), list(m)), gamma=gamma, double_q=bool(dq))
    go = O.Network.flatten(o["grads"])
    np.testing.assert_allclose(got["loss"], o["loss"], rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(got["grads"], go, rtol=1e-10, atol=1e-10 * np.abs(go).max())
    # the policy's state after a few steps: the oracle's Recur state, layer by layer (h, c)
    rng = np.random.default_rng(2)
    xs = [rng.random((3, E)) for _ in range(4)]
    _, want = oracle_recur_state(onet, p_on, xs)
    with torch.no_grad():
        _, hs = R.seq_q(net, nn, GR.param_arrays(net, nn, p_on), [torch.tensor(x) for x in xs])
    got_l = R.hidden_layout(net, nn, hs)
    assert len(got_l) == len(want)
    for (h, c), (ho, co) in zip(got_l, want):
        np.testing.assert_allclose(h, ho, rtol=1e-12, atol=1e-14); np.testing.assert_allclose(c, co, rtol=1e-12, atol=1e-14)


def test_mixed_chain_gradient_equals_central_finite_differences(nn):
    """Dense -> LSTM -> GRU -> RNN(relu) -> Dense, dueling: autograd against fp64 central differences on 3 coordinates of every block (h0, c0
    included), the Bellman targets held fixed (they are constants of the loss).  Independent of how the cells are composed."""
    net = nn.create_dueling_network(nn.Chain(nn.Dense(5, 9, nn.tanh), nn.LSTM(9, 7), nn.GRU(7, 6), nn.RNN(6, 5, nn.relu), nn.Dense(5, 4)))
    batch, p_on, p_tg = _ring_and_batch(net, nn, 5, 4, 4, 5, 9)
    p_on = p_on + np.float32(0.3) * np.random.default_rng(4).standard_normal(p_on.size).astype(np.float32)      # state0 and biases well away from 0
    got = R.train_grads(net, nn, p_on, p_tg, batch, 0.9, 1)
    assert not R.dead_blocks(net, nn, got["grads"])
    ys = got["ys"]
    p64 = np.asarray(p_on, np.float64)

    def loss_at(p):
        with torch.no_grad():
            return float(R.batch_loss(net, nn, GR.param_arrays(net, nn, p), batch, ys))
    rng = np.random.default_rng(0)
    eps = 1e-6
    for nm, sl in R.blocks(net, nn):
        idx = np.arange(sl.start, sl.stop)
        gb = np.abs(got["grads"][idx])
        pick = [int(idx[np.argmax(gb)])] + list(rng.choice(idx, size=min(2, idx.size - 1), replace=False))      # the block's largest coordinate + 2 at random
        for k in pick:
            pp, pm = p64.copy(), p64.copy(); pp[k] += eps; pm[k] -= eps
            fd = (loss_at(pp) - loss_at(pm)) / (2 * eps)
            assert abs(fd - got["grads"][k]) <= 1e-7 * np.abs(got["grads"]).max() + 1e-6 * abs(fd), (nm, k, fd, got["grads"][k])


def test_block_check_rejects_a_dead_block(nn):
    """a config whose block gradient is negligible is rejected, not passed vacuously"""
    net = nn.Chain(nn.RNN(6, 8, nn.sigmoid), nn.Dense(8, 3))
    batch, p_on, p_tg = _ring_and_batch(net, nn, 6, 3, 4, 3, 10)
    g = R.train_grads(net, nn, p_on, p_tg, batch, 0.9, 0)["grads"]
    assert not R.dead_blocks(net, nn, g)
    R.check_grads(net, nn, g.copy(), g)
    sl = dict(R.blocks(net, nn))["rnn0.h0"]
    g2 = g.copy(); g2[sl] *= 1e-6
    assert R.dead_blocks(net, nn, g2) == ["rnn0.h0"]
    with pytest.raises(AssertionError, match="negligible"):
        R.check_grads(net, nn, g2, g2)
    g3 = g.copy(); g3[sl] *= 1.01      # a 1 % error in one small block fails
    with pytest.raises(AssertionError, match="rnn0.h0"):
        R.check_grads(net, nn, g3, g)


def test_fp64_adam_equals_the_oracle_adam_over_steps():
    """R.Adam (fp64 m, v, t) is dqn_oracle's Adam on fp64 arrays: bias correction at t = 1, 2, 3"""
    rng = np.random.default_rng(3)
    p = rng.standard_normal(50); a = R.Adam(50); st = O.AdamState([p.copy()], 1e-3)
    q = p.copy()
    for _ in range(3):
        g = rng.standard_normal(50) * 1e-2
        p = a.step(p, g); q = O.adam_update([q], [g], st)[0]
        np.testing.assert_allclose(p, q, rtol=1e-14, atol=1e-16)


STACKED_LSTM = {
    "lstm_lstm": (O.RecurrentNetwork((6,), [O.LSTM(6, 12), O.LSTM(12, 8), O.Dense(8, 4, O.ACT_IDENTITY)]), 5, 6, dict(gamma=0.95, double_q=1)),
    "lstm_dense_lstm_dueling": (O.RecurrentNetwork((6,), [O.LSTM(6, 10), O.Dense(10, 12, O.ACT_TANH), O.LSTM(12, 8)], [O.Dense(8, 1, O.ACT_IDENTITY)], [O.Dense(8, 5, O.ACT_IDENTITY)]), 6, 4, dict(gamma=0.99, double_q=1)),
}


@pytest.mark.parametrize("name", list(STACKED_LSTM))
def test_twin_equals_the_oracle_on_stacked_lstms(name):
    ge.build()
    net, B, T, kw = STACKED_LSTM[name]
    rng = np.random.default_rng(5)
    cap = max(12, B + 4)
    h, hp, layers = make_handle(ref.Twin, net, B, T, kw, cap=cap)
    eps = make_episodes(net, cap + 3, T, rng)
    feed(h, eps)
    ring = [None] * cap
    for i, ep in enumerate(eps):
        ring[i % cap] = ep
    p_on = (O.Network.flatten(O.init_params_recurrent(net, 3)) + 0.05 * rng.standard_normal(net.n_params())).astype(np.float32)
    p_tg = (O.Network.flatten(O.init_params_recurrent(net, 4)) + 0.05 * rng.standard_normal(net.n_params())).astype(np.float32)
    h.set_params(p_on, 0); h.set_params(p_tg, 1)
    check_against_oracle(h, net, ring, B, T, kw, np.random.default_rng(11), (p_on, p_tg))
    h.close()
