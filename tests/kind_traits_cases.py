"""The networks behind tests/golden/kind_traits_cpu.json and kind_traits_gpu.json: what the engine decided for each of them BEFORE the per-kind clauses of csrc/ were folded into
one traits table (docs/history/kind_traits.md).  The fixtures hold, per case, what `observe_cpu` / `observe_gpu` returned on that commit; the tests call the same two functions on
the library under test and compare for equality.  Nothing here computes an expected value.

CPU (dqn_plan_default runs build_layers + default_plan on the host): the refusal text, or the full default plan at B = 8 and B = 128.
GPU: the launch names of one train step (dqn_profile_step) and of a middle step (dqn_profile_steady_step), the acting program's fused_tail (dqn_envs_info), and the refusal
texts of dqn_comm_init / DQN_SIM_WORLD."""
import importlib
import os

import numpy as np

import __graft_entry__ as ge

pkg = ge.load_package()
nn = importlib.import_module(pkg.__name__ + ".nn")
abi = nn._abi
D, CV, LSTM, MAXP, MEANP, LN, DO, SK = abi.LAYER_DENSE, abi.LAYER_CONV, abi.LAYER_LSTM, abi.LAYER_MAXPOOL, abi.LAYER_MEANPOOL, abi.LAYER_LAYERNORM, abi.LAYER_DROPOUT, abi.LAYER_SKIPADD
P_HALF = 0x3FE00000      # the high word of the Float64 0.5


def desc(kind, stream=0, act=0, n_in=0, n_out=0, cin=0, cout=0, k=0, s=0):
    d = abi.LayerDesc(); d.kind, d.act, d.stream, d.n_in, d.n_out, d.cin, d.cout, d.kh, d.kw, d.sh, d.sw = kind, act, stream, n_in, n_out, cin, cout, k, k, s, s
    return d


dn = lambda a, b, **kw: desc(D, n_in=a, n_out=b, **kw)
cv = lambda ci, co, k=3, s=1, pad=0, **kw: desc(CV, cin=ci, cout=co, k=k, s=s, n_in=pad, n_out=pad, **kw)
pool = lambda kind=MAXP, k=2, s=2, **kw: desc(kind, k=k, s=s, **kw)
ln = lambda n=16, **kw: desc(LN, n_in=n, n_out=n, **kw)
do = lambda **kw: desc(DO, cout=P_HALF, **kw)
sk = lambda m, n=0, **kw: desc(SK, cin=m, n_in=n, n_out=n, **kw)
lower = lambda *ls: nn.lower(nn.Chain(*ls))[0]
relu, tanh = nn.relu, nn.tanh


# ------------------------------------------------------------------ CPU: refusals and default plans
def _cpu_cases():
    first, head = dn(6, 16, act=1), dn(16, 4)
    vec = dict(obs=(6, 1, 1)); img = dict(obs=(2, 8, 8))
    c = {}
    # the four output-layer refusals
    c["out_pool"] = ([cv(2, 1), pool(k=3, s=3)], img)                                  # 1 x 6 x 6 -> 1 x 2 x 2 = 4 = n_actions
    c["out_ln"] = ([dn(6, 4), ln(4)], vec)
    c["out_do"] = ([dn(6, 4), do()], vec)
    c["out_skip"] = ([dn(6, 4), dn(4, 4), sk(1)], vec)
    # two refusals of each own-level kind's block
    c["pool_after_dense"] = ([dn(128, 16), pool(), head], img)
    c["pool_window"] = ([pool(k=9, s=1), dn(128, 4)], img)
    c["pool_act"] = ([pool(MEANP, act=1), dn(32, 4)], img)
    c["cpad_too_large"] = ([cv(2, 4, pad=3), dn(4, 4)], img)
    c["cpad_stream"] = ([cv(2, 4), desc(CV, stream=1, cin=4, cout=4, k=3, s=1, n_in=1, n_out=1), dn(4, 4)], img | dict(dueling=1))
    c["ln_first"] = ([ln(6), dn(6, 4)], vec)
    c["ln_after_ln"] = ([first, ln(), ln(), head], vec)
    c["ln_size"] = ([first, ln(12), head], vec)
    c["do_first"] = ([do(), dn(6, 4)], vec)
    c["do_after_do"] = ([first, do(), do(), head], vec)
    c["do_p_one"] = ([first, desc(DO, cout=0x3FF00000), head], vec)
    c["skip_m0"] = ([first, dn(16, 16), sk(0), head], vec)
    c["skip_nested"] = ([first, dn(16, 16), sk(1), dn(16, 16), sk(3), head], vec)
    c["skip_n_to_m"] = ([first, dn(16, 32, act=1), dn(32, 12), sk(2), dn(12, 4)], vec)
    # accepted networks holding each kind: the full default plan
    c["plan_dense_wide"] = (lower(nn.Dense(6, 2048, relu), nn.Dense(2048, 600, relu), nn.Dense(600, 256, relu), nn.Dense(256, 4)), vec)
    c["plan_pool_first"] = (lower(nn.MaxPool(2), nn.Conv(3, 2, 16, relu), nn.Dense(64, 4)), img)
    c["plan_pool_mid"] = (lower(nn.Conv(3, 2, 16, relu), nn.MeanPool(2), nn.Conv(2, 16, 16, relu), nn.Dense(64, 4)), img)
    c["plan_pool_wide"] = (lower(nn.Conv(3, 2, 64, relu), nn.MaxPool((2, 2), stride=1), nn.Dense(1600, 4)), img)      # a pool whose out_feat exceeds every threshold of default_plan
    c["plan_cpad"] = (lower(nn.Conv(3, 2, 16, relu, pad=1), nn.Conv(3, 16, 16, relu, stride=2, pad=1), nn.Dense(256, 4)), img)
    c["plan_ln"] = (lower(nn.Dense(6, 1040, relu), nn.LayerNorm(1040), nn.Dense(1040, 256, relu), nn.Dense(256, 4)), vec)
    c["plan_do"] = (lower(nn.Dense(6, 1040, relu), nn.Dropout(0.5), nn.Dense(1040, 256, relu), nn.Dense(256, 4)), vec)
    c["plan_skip"] = (lower(nn.Dense(6, 1040, relu), nn.SkipConnection(nn.Chain(nn.LayerNorm(1040), nn.Dense(1040, 1040, relu), nn.Dropout(0.1)), "+"), nn.Dense(1040, 4)), vec)
    c["plan_all_dueling"] = (nn.lower(nn.create_dueling_network(nn.Chain(nn.Conv(3, 2, 16, relu, pad=1), nn.MaxPool(2), nn.Conv(3, 16, 16, relu), nn.Dense(64, 256, relu), nn.LayerNorm(256),
                                                                        nn.SkipConnection(nn.Chain(nn.Dense(256, 256, relu), nn.Dropout(0.5)), "+"), nn.Dense(256, 128, relu), nn.Dense(128, 4))))[0], img | dict(dueling=1))
    # a feature vector is a (n, 1, 1) map to build_layers: a 1x1 Conv may follow a LayerNorm and a 1x1 pool that Conv
    c["plan_ln_conv_pool"] = (lower(nn.Dense(6, 16, relu), nn.LayerNorm(16), nn.Conv(1, 16, 8, relu), nn.MaxPool(1), nn.Dense(8, 4)), vec)
    c["plan_lstm_fused"] = (lower(nn.LSTM(6, 8), nn.Dense(8, 4)), vec | dict(recurrence=1, trace_length=3))
    c["plan_lstm_ln"] = (lower(nn.LSTM(6, 8), nn.LayerNorm(8), nn.Dense(8, 4)), vec | dict(recurrence=1, trace_length=3))
    c["plan_lstm_do"] = (lower(nn.LSTM(6, 8), nn.Dropout(0.5), nn.Dense(8, 4)), vec | dict(recurrence=1, trace_length=3))
    c["plan_lstm_skip"] = (lower(nn.LSTM(6, 8), nn.SkipConnection(nn.Dense(8, 8), "+"), nn.Dense(8, 4)), vec | dict(recurrence=1, trace_length=3))
    return c


CPU_CASES = _cpu_cases()


def observe_cpu(name):
    layers, kw = CPU_CASES[name]
    kw = dict(kw); obs = kw.pop("obs"); out = {}
    for B in (8, 128):
        hp = pkg.default_hparams(batch_size=B, n_actions=4, obs_c=obs[0], obs_h=obs[1], obs_w=obs[2], buffer_size=256, **({"dueling": 0} | kw))
        try:
            out[f"B{B}"] = {"plan": [list(p) for p in pkg.default_plan(layers, hp)]}
        except pkg.DQNError as e:
            out[f"B{B}"] = {"error": str(e)}
    return out


# ------------------------------------------------------------------ GPU: launch programs, fused_tail, replica refusals
def _trunk(x=None, wide=1056, mid=128):
    """Dense(32, 32) -> [x] -> Dense(32, wide) -> Dense(wide, mid) -> Dense(mid, 4): wide = 1056 > 1024 makes the heads' producer a split-K layer at B < 128 (k_red_head),
    wide = 64 leaves it unsplit (k_head_cols4)"""
    return [nn.Dense(32, 32, relu)] + ([x()] if x else []) + [nn.Dense(32, wide, relu), nn.Dense(wide, mid, relu), nn.Dense(mid, 4)]


INSERTS = {"": None, "_ln": lambda: nn.LayerNorm(32), "_do": lambda: nn.Dropout(0.5), "_skip": lambda: nn.SkipConnection(nn.Dense(32, 32, tanh), "+")}
LN1_POOL3 = lambda: (nn.Dense(32, 16, relu), nn.LayerNorm(16), nn.Conv(1, 16, 8, relu), nn.MaxPool(1), nn.Dense(8, 4))      # a feature vector is a (n, 1, 1) map: LayerNorm at layer 1, pool at layer 3
VEC, IMG, ENVOBS = (32, 1, 1), (2, 8, 8), (4, 5, 5)


def _gpu_cases():
    """name -> dict(net, obs, B, hp, env (switches set while the engine is created), envs (bool: record fused_tail instead of a train step), refuse (bool: record the refusals))"""
    c = {}
    case = lambda name, net, obs=VEC, B=8, env=None, envs=False, refuse=False, **hp: c.__setitem__(name, dict(net=net, obs=obs, B=B, hp=hp, env=env or {}, envs=envs, refuse=refuse))
    for sfx, x in INSERTS.items():
        tiny = [nn.Dense(32, 32, relu)] + ([x()] if x else []) + [nn.Dense(32, 16, relu), nn.Dense(16, 4)]
        case("tiny" + sfx, nn.Chain(*tiny))                                                   # the single-workgroup step where nothing declines it
        case("red_head" + sfx, nn.Chain(*_trunk(x)), prioritized_replay=0)
        case("head_cols4" + sfx, nn.Chain(*_trunk(x, wide=64)), prioritized_replay=0)
        rec = [nn.LSTM(6, 8)] + ([{"_ln": lambda: nn.LayerNorm(8), "_do": lambda: nn.Dropout(0.5), "_skip": lambda: nn.SkipConnection(nn.Dense(8, 8, tanh), "+")}[sfx]()] if x else []) + [nn.Dense(8, 4)]
        case("lstm" + sfx, nn.Chain(*rec), obs=(6, 1, 1), B=4, recurrence=1, trace_length=3, prioritized_replay=0)
    case("tiny_off", nn.Chain(nn.Dense(32, 32, relu), nn.Dense(32, 16, relu), nn.Dense(16, 4)), env={"DQN_NO_TINY": "1"})
    case("dueling_b8", nn.create_dueling_network(nn.Chain(nn.Dense(32, 64, relu), nn.Dense(64, 32, relu), nn.Dense(32, 4))), env={"DQN_NO_TINY": "1"}, dueling=1)
    case("red_head_dueling", nn.create_dueling_network(nn.Chain(nn.Dense(32, 1056, relu), nn.Dense(1056, 128, relu), nn.Dense(128, 4))), dueling=1, prioritized_replay=0)
    # one network per own-level kind
    case("pool_first", nn.Chain(nn.MaxPool(2), nn.Conv(3, 2, 16, relu), nn.Dense(64, 4)), obs=IMG)
    case("pool_first_u8", nn.Chain(nn.MaxPool(2), nn.Conv(3, 2, 16, relu), nn.Dense(64, 4)), obs=IMG, B=32, obs_dtype=abi.OBS_U8)
    case("pool_mid", nn.Chain(nn.Conv(3, 2, 8, relu), nn.MeanPool(2), nn.Dense(72, 16, relu), nn.Dense(16, 4)), obs=IMG)
    case("cpad", nn.Chain(nn.Conv(3, 2, 8, relu, pad=1), nn.Conv(3, 8, 8, relu, stride=2, pad=1), nn.Dense(128, 16, relu), nn.Dense(16, 4)), obs=IMG)
    case("cpad_u8", nn.Chain(nn.Conv(3, 2, 8, relu, pad=1), nn.Dense(512, 16, relu), nn.Dense(16, 4)), obs=IMG, B=32, obs_dtype=abi.OBS_U8)
    case("cpad_head_cols4", nn.Chain(nn.Conv(3, 2, 8, relu, pad=1), nn.MaxPool(2), nn.Dense(128, 128, relu), nn.Dense(128, 4)), obs=IMG, prioritized_replay=0)      # a padded conv and a pool do NOT decline the fused head launch
    case("ln", nn.Chain(nn.Dense(32, 16, relu), nn.LayerNorm(16, relu), nn.Dense(16, 4)), prioritized_replay=0)
    case("do", nn.Chain(nn.Dense(32, 16, relu), nn.Dropout(0.5), nn.Dense(16, 16, relu), nn.Dense(16, 4)), prioritized_replay=0)
    case("skip_alias", nn.Chain(nn.Dense(32, 16, relu), nn.SkipConnection(nn.Dense(16, 16), "+"), nn.Dense(16, 4)), prioritized_replay=0)
    case("skip_join", nn.Chain(nn.Dense(32, 16, relu), nn.SkipConnection(nn.Dense(16, 16, tanh), "+"), nn.Dense(16, 4)), prioritized_replay=0)
    case("droq", nn.Chain(nn.Dense(32, 16, relu), nn.SkipConnection(nn.Chain(nn.Dense(16, 16), nn.Dropout(0.1), nn.LayerNorm(16, relu)), "+"), nn.Dense(16, 4)), prioritized_replay=0)
    case("droq_dueling", nn.create_dueling_network(nn.Chain(nn.Dense(32, 16, relu), nn.SkipConnection(nn.Chain(nn.Dense(16, 16), nn.Dropout(0.1), nn.LayerNorm(16, relu)), "+"), nn.Dense(16, 4))), dueling=1)
    case("ln_conv_pool", nn.Chain(*LN1_POOL3()), prioritized_replay=0)      # every own-level forward and backward piece but Dropout's and the join's behind a LayerNorm
    # the carrier scans of the priority block (B = 128, prioritized): two LDS-tiled dW launches split the block; a pool and a padded conv between them are no carriers
    case("carriers", nn.Chain(nn.Conv(3, 2, 16, relu), nn.Conv(3, 16, 16, relu), nn.Dense(256, 32, relu), nn.Dense(32, 4)), obs=IMG, B=128)
    case("carriers_own_level", nn.Chain(nn.Conv(3, 2, 16, relu), nn.MaxPool(2), nn.Conv(3, 16, 16, relu, pad=1), nn.Dense(144, 32, relu), nn.Dense(32, 4)), obs=IMG, B=128)
    case("carriers_ln_skip", nn.Chain(nn.Conv(3, 2, 16, relu), nn.Dense(576, 32, relu), nn.LayerNorm(32), nn.SkipConnection(nn.Chain(nn.Dense(32, 32, relu), nn.Dropout(0.5)), "+"), nn.Dense(32, 4)), obs=IMG, B=128)
    # the acting program's tail (TestMDP observations, 8 copies)
    envc = lambda name, *ls: case("act_" + name, nn.Chain(*ls), obs=ENVOBS, envs=True)
    envc("dense", nn.Dense(100, 32, relu), nn.Dense(32, 128, relu), nn.Dense(128, 4))
    envc("ln", nn.Dense(100, 32, relu), nn.LayerNorm(32), nn.Dense(32, 128, relu), nn.Dense(128, 4))
    envc("do", nn.Dense(100, 32, relu), nn.Dropout(0.5), nn.Dense(32, 128, relu), nn.Dense(128, 4))
    envc("skip", nn.Dense(100, 32, relu), nn.SkipConnection(nn.Dense(32, 32), "+"), nn.Dense(32, 128, relu), nn.Dense(128, 4))
    envc("conv", nn.Conv(3, 4, 8, relu), nn.Dense(72, 128, relu), nn.Dense(128, 4))
    envc("cpad", nn.Conv(3, 4, 8, relu, pad=1), nn.Dense(200, 128, relu), nn.Dense(128, 4))
    envc("pool", nn.Conv(2, 4, 8, relu), nn.MaxPool(2), nn.Dense(32, 128, relu), nn.Dense(128, 4))      # a pool does NOT decline the fused tail
    # replicas: the refusal names the kind of highest priority (padded conv, pool, LayerNorm, Dropout, skip block), not the first own-level layer: a network with a
    # LayerNorm at layer 1 and a pool at layer 3 names the pool (ln1_pool3); with a padded conv at layer 2 as well, that one (ln1_cpad2_pool3)
    ref = lambda name, *ls, obs=VEC: case("refuse_" + name, nn.Chain(*ls), obs=obs, refuse=True, prioritized_replay=0)
    ref("ln1_pool3", *LN1_POOL3())
    ref("ln1_cpad2_pool3", nn.Dense(32, 16, relu), nn.LayerNorm(16), nn.Conv(3, 16, 8, relu, pad=1), nn.MaxPool(1), nn.Dense(8, 4))
    ref("pool0_cpad1", nn.MaxPool(2), nn.Conv(3, 2, 8, relu, pad=1), nn.Dense(128, 4), obs=IMG)
    ref("do1_ln3", nn.Dense(32, 16, relu), nn.Dropout(0.5), nn.Dense(16, 16, relu), nn.LayerNorm(16), nn.Dense(16, 4))
    ref("skip2_do3", nn.Dense(32, 16, relu), nn.SkipConnection(nn.Dense(16, 16), "+"), nn.Dropout(0.5), nn.Dense(16, 4))
    ref("pool1_ln3", nn.Conv(3, 2, 8, relu), nn.MeanPool(2), nn.Dense(72, 16, relu), nn.LayerNorm(16), nn.Dense(16, 4), obs=IMG)
    for k, net in (("cpad", (nn.Conv(3, 2, 8, relu, pad=(1, 2)), nn.Dense(640, 4))), ("pool", (nn.MaxPool(2), nn.Dense(32, 4)))):
        ref(k, *net, obs=IMG)
    ref("ln", nn.Dense(32, 16, relu), nn.LayerNorm(16), nn.Dense(16, 4))
    ref("do", nn.Dense(32, 16, relu), nn.Dropout(0.5), nn.Dense(16, 4))
    ref("skip", nn.Dense(32, 16, relu), nn.SkipConnection(nn.Dense(16, 16), "+"), nn.Dense(16, 4))
    return c


GPU_CASES = _gpu_cases()


class _environ:
    """the engine reads its switches once, at creation"""
    def __init__(self, kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _engine(c, env):
    layers, dueling = nn.lower(c["net"])
    hp = pkg.default_hparams(**({"batch_size": c["B"], "n_actions": 4, "obs_c": c["obs"][0], "obs_h": c["obs"][1], "obs_w": c["obs"][2], "dueling": 0, "buffer_size": 2 * c["B"],
                                "learning_rate": 1e-3, "gamma": 0.95, "seed": 5} | c["hp"]))
    with _environ(env):
        h = pkg.Engine(layers, hp)
    p = nn.glorot_params(c["net"], seed=3)
    h.set_params(p, 0); h.sync_target()
    return h, hp


def _fill(h, hp, c):
    rng = np.random.default_rng(11); n = 2 * c["B"]; shape = tuple(c["obs"])
    obs = (lambda m: rng.integers(0, 256, (m,) + shape).astype(np.uint8)) if hp.obs_dtype == abi.OBS_U8 else (lambda m: rng.random((m,) + shape, dtype=np.float32))
    if hp.recurrence:
        for _ in range(n):
            T = hp.trace_length; d = np.zeros(T, np.uint8); d[-1] = 1
            h.episode_add(obs(T), rng.integers(0, 4, T).astype(np.int32), rng.standard_normal(T).astype(np.float32), obs(T), d)
            h.episode_commit()
    else:
        h.replay_add(obs(n), rng.integers(0, 4, n).astype(np.int32), rng.standard_normal(n).astype(np.float32), obs(n), (rng.random(n) < 0.2).astype(np.uint8))


def _refusal(fn):
    try:
        fn()
    except pkg.DQNError as e:
        return str(e)
    return None


def observe_gpu(name):
    c = GPU_CASES[name]
    if c["refuse"]:
        h, _ = _engine(c, c["env"])
        out = {"comm_init": _refusal(lambda: h.comm_init(bytes(128), 0, 1))}
        h.close()
        out["sim_world"] = _refusal(lambda: _engine(c, c["env"] | {"DQN_SIM_WORLD": "2"})[0].close())
        return out
    h, hp = _engine(c, c["env"])
    if c["envs"]:
        envs = importlib.import_module(pkg.__name__ + ".envs")
        h.envs_create(envs.TestMDP((5, 5), 4, 6, n=8, seed=3), max_episode_length=100, seed=17)
        out = {"fused_tail": h.envs_info()[1]}
    else:
        _fill(h, hp, c)
        out = {"step": [n for n, _ in h.profile_step(max_entries=512)]}
        if not hp.recurrence:
            out["steady"] = [n for n, _ in h.profile_step(max_entries=512, steady=True)]
    h.close()
    return out
