"""fp64 torch reference for recurrent Q-networks with Flux GRU layers (TEST INFRASTRUCTURE): the GRU cell (gates r, z, n; Flux 0.14 GRUCell) and the flat-vector
split every reference shares.  The recurrent batch_train! of src/solver.jl:239-287 on a given sampled batch and the policy's Recur state are recurrent_reference's,
which runs any mix of cells; its names are reachable from here as they always were.  Networks are the package's own nn descriptors."""
import numpy as np
import torch

F64 = torch.float64


def gru_cell(x, h, Wi, Wh, b):
    """x: (B, in), h: (B, H); Wi: (in, 3H), Wh: (H, 3H), b: (3H,) -- the C-order views of Flux's Wi (3H, in), Wh (3H, H)"""
    H = h.shape[1]
    gx, gh = x @ Wi, h @ Wh
    r = torch.sigmoid(gx[:, :H] + gh[:, :H] + b[:H])
    z = torch.sigmoid(gx[:, H:2 * H] + gh[:, H:2 * H] + b[H:2 * H])
    n = torch.tanh(gx[:, 2 * H:] + r * gh[:, 2 * H:] + b[2 * H:])
    return (1 - z) * n + z * h


def param_arrays(net, nn, flat):
    """flat Flux.params vector -> list of fp64 tensors (C-order shapes of nn's descriptors), one list per layer"""
    out, off = [], 0
    for l in nn.all_layers(net):
        shapes = l.shapes()
        arrs = []
        for s in shapes:
            k = int(np.prod(s))
            arrs.append(torch.tensor(np.asarray(flat[off:off + k], np.float64).reshape(s), dtype=F64))
            off += k
        out.append(arrs)
    assert off == len(flat)
    return out


def _act(y, act):
    return {0: y, 1: torch.relu(y), 2: torch.tanh(y), 3: torch.sigmoid(y)}[act] if act in (0, 1, 2, 3) else y


def __getattr__(name):
    """the chain step, the Recur state, the recurrent train step and its check are recurrent_reference's, one for every cell (it imports the cell from here: hence by name, late)"""
    if name in ("_chain_step", "init_state", "q_step", "seq_q", "drqn_train_step", "check_step"):
        import recurrent_reference
        return getattr(recurrent_reference, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
