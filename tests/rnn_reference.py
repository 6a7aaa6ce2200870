"""fp64 torch reference for recurrent Q-networks with Flux RNN layers (TEST INFRASTRUCTURE): the plain RNN cell (Flux 0.14 RNNCell,
h' = σ.(Wi*x .+ Wh*h .+ b)).  The recurrent batch_train! of src/solver.jl:239-287 on a given sampled batch and the policy's Recur state are
recurrent_reference's, which runs any mix of cells; its names are reachable from here as they always were."""
from gru_reference import _act, param_arrays      # noqa: F401


def rnn_cell(x, h, Wi, Wh, b, act):
    """x: (B, in), h: (B, H); Wi: (in, H), Wh: (H, H), b: (H,) -- the C-order views of Flux's Wi (H, in), Wh (H, H); act: DQN_ACT_* code"""
    return _act(x @ Wi + h @ Wh + b, act)


def __getattr__(name):
    """the chain step, the Recur state, the recurrent train step and its check are recurrent_reference's, one for every cell (it imports the cell from here: hence by name, late)"""
    if name in ("_chain_step", "init_state", "q_step", "seq_q", "drqn_train_step", "check_step"):
        import recurrent_reference
        return getattr(recurrent_reference, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
