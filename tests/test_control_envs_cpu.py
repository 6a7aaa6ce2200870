"""CPU: the twins of the control device environments (envs.MountainCar / envs.InvertedPendulum) -- known answers of the laws worked by hand, the twins' Philox
against the tests' own, the ABI struct against the header and the shim, the mirror's refusals, the case table's branch margins, and two control known answers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as ge
import control_envs_common as CC
from test_shim_static_cpu import SHIM, julia_struct_layout

pkg = ge.load_package()
nn, envs, S = CC.load(pkg)


def test_twin_draws_are_the_device_layout():
    for seed, t, i, p in ((1, 0, 0, 13), (2 ** 40 + 5, 7, 3, 12), (99, 2 ** 33, 1023, 14), (7, 5, 31, 1)):
        assert int(envs.philox_u32(seed, t, [i], p)[0]) == CC.philox(seed, t, i, p)
        assert envs.u01(envs.philox_u32(seed, t, [i], p))[0] == CC.u01(CC.philox(seed, t, i, p))
    ip = envs.InvertedPendulum(n=4, seed=9, init_half=0.25)
    want = np.stack([(CC.draws(9, 0, 4, 13) - 0.5) * 2.0 * 0.25, (CC.draws(9, 0, 4, 14) - 0.5) * 2.0 * 0.25], 1)
    np.testing.assert_array_equal(ip.s, want)
    assert np.all(np.abs(ip.s) <= 0.25) and ip.obs_shape == (2,) and ip.n_actions == 3 and ip.discount == 0.99 and ip.observe().dtype == np.float32


def test_mountaincar_known_answers():
    """the first step from (-0.5, 0) under each action, the clamp and the wall, by hand"""
    mc = envs.MountainCar(n=3)
    np.testing.assert_array_equal(mc.s, [[-0.5, 0.0]] * 3)
    r = mc.act([0, 1, 2])
    grav = np.cos(3.0 * -0.5) * (-0.0025)
    for i, push in enumerate((-1.0, 0.0, 1.0)):
        v = 0.0 + push * 0.001 + grav
        assert mc.s[i, 1] == v and mc.s[i, 0] == -0.5 + v
    np.testing.assert_array_equal(r, np.float32([-1, -1, -1])); assert not mc.terminated().any()
    s, r, d, _ = mc.step_law(np.array([[0.0, -0.07], [0.0, 0.0699]]), np.array([0, 2]))      # cos(0) = 1: gravity takes 0.0025
    np.testing.assert_array_equal(s, [[-0.07, -0.07], [0.0 + (0.0699 + 0.001 - 0.0025), 0.0699 + 0.001 - 0.0025]])      # clamped to exactly -v_max; the other copy is not
    s, r, d, _ = mc.step_law(np.array([[-1.19, -0.07]]), np.array([1]))
    np.testing.assert_array_equal(s, [[-1.2, 0.0]]); assert r[0] == -1.0 and not d[0]      # walled: exactly (x_min, 0)
    s, r, d, _ = mc.step_law(np.array([[0.45, 0.06]]), np.array([2]))
    assert d[0] and r[0] == 99.0 and s[0, 0] >= 0.5
    mc.reset(np.array([True, False, True]))
    np.testing.assert_array_equal(mc.s[[0, 2]], [[-0.5, 0.0]] * 2); assert mc.s[1, 1] == grav


def test_pendulum_known_answers():
    """acc at theta = 0 is -alpha * u / ((4/3 - alpha * m) * l); explicit Euler from the pre-step state; falling from init_half = 1.5"""
    ip = envs.InvertedPendulum(n=1, noise=0.0)
    c = ip.c
    for a, u in ((0, -50.0), (1, 0.0), (2, 50.0)):
        s, r, d, _ = ip.step_law(np.array([[0.0, 0.3]]), np.array([a]), np.array([0.75]))
        acc = -c["alpha"] * u / ((4.0 / 3.0 - c["alpha"] * c["m"]) * c["l"])
        assert s[0, 0] == 0.0 + 0.3 * 0.1 and abs(s[0, 1] - (0.3 + acc * 0.1)) <= 1e-15 and r[0] == 0.0 and not d[0]
    assert c["alpha"] == 1.0 / (2.0 + 8.0) and float(c["theta_max"]) == np.pi / 2
    noisy = envs.InvertedPendulum(n=1)      # u = a + noise * (U - 0.5): U = 0.75 adds 5
    s1, _, _, _ = noisy.step_law(np.array([[0.0, 0.0]]), np.array([1]), np.array([0.75]))
    assert abs(s1[0, 1] - (-c["alpha"] * 5.0 / ((4.0 / 3.0 - c["alpha"] * c["m"]) * c["l"])) * 0.1) <= 1e-16
    s, r, d, _ = ip.step_law(np.array([[1.55, 0.5]]), np.array([1]), np.array([0.5]))
    assert d[0] and r[0] == -1.0 and s[0, 0] == 1.55 + 0.5 * 0.1
    wide = envs.InvertedPendulum(n=64, seed=3, init_half=1.5)
    fell = np.zeros(64, bool)
    for _ in range(100):
        wide.act(np.ones(64, np.int64)); fell |= wide.terminated()
    assert fell.all()


def test_struct_layout_agrees_between_ctypes_header_and_shim(tmp_path):
    abi = pkg._abi
    fields = [f[0] for f in abi.ControlEnv._fields_]
    offs = ", ".join(f"offsetof(dqn_control_env, {f})" for f in fields)
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "dqn_mi355x.h"\nint main(){size_t v[] = {sizeof(dqn_control_env), ' + offs + ', DQN_ENV_MOUNTAINCAR, DQN_ENV_PENDULUM, '
           'DQN_ENV_RAND_PEND_NOISE, DQN_ENV_RAND_PEND_THETA0, DQN_ENV_RAND_PEND_OMEGA0, sizeof(dqn_env_spec), sizeof(dqn_tabular_env)};'
           'for (unsigned i = 0; i < sizeof v / sizeof *v; i++) printf("%zu ", v[i]);}')
    (tmp_path / "t.c").write_text(src)
    subprocess.run(["gcc", "-I", os.path.join(ge.ROOT, "include"), str(tmp_path / "t.c"), "-o", str(tmp_path / "t")], check=True)
    got = list(map(int, subprocess.run([str(tmp_path / "t")], capture_output=True, text=True, check=True).stdout.split()))
    want = [ctypes.sizeof(abi.ControlEnv)] + [getattr(abi.ControlEnv, f).offset for f in fields] + [abi.ENV_MOUNTAINCAR, abi.ENV_PENDULUM, 12, 13, 14,
                                                                                                      ctypes.sizeof(abi.EnvSpec), ctypes.sizeof(abi.TabularEnv)]
    assert got == want and fields[4:] == list(envs._ControlEnv.FIELDS) and (abi.ENV_MOUNTAINCAR, abi.ENV_PENDULUM) == (3, 4) == (envs.MountainCar.KIND, envs.InvertedPendulum.KIND)
    size, offsets = julia_struct_layout(open(SHIM).read(), "ControlEnv")
    assert size == ctypes.sizeof(abi.ControlEnv) and list(offsets) == fields
    for f, off in offsets.items():
        assert off == getattr(abi.ControlEnv, f).offset, f


def test_shim_source():
    src = open(SHIM).read()
    assert "(:dqn_envs_create_control, LIB)" in src and "(:dqn_envs_peek_state, LIB)" in src
    assert "function envs_create_control!(e::Engine, mdp::Union{POMDPModels.MountainCar,POMDPModels.InvertedPendulum}; n_envs, max_episode_length = 100, seed = 0)" in src
    for field in ("mdp.cost", "mdp.jackpot", "mdp.g", "mdp.m", "mdp.l", "mdp.M", "mdp.alpha", "mdp.dt"):
        assert field in src, field
    # the defaults written into the two constructors are the twin's
    d = envs._ControlEnv.ALL_DEFAULTS
    mc = src[src.index("control_spec(mdp::POMDPModels.MountainCar"):src.index("control_spec(mdp::POMDPModels.InvertedPendulum")]
    assert "0.001, 3.0, 0.0025, 0.07, -1.2, 0.5, mdp.cost, mdp.jackpot, -0.5, 0.0" in mc and "50.0, 20.0, pi / 2, 0.1)" in mc
    assert (d["force"], d["freq"], d["gravity"], d["v_max"], d["x_min"], d["goal"], d["x0"], d["v0"], d["u_max"], d["noise"], d["init_half"]) == (0.001, 3.0, 0.0025, 0.07, -1.2, 0.5, -0.5, 0.0, 50.0, 20.0, 0.1)


def test_python_side_refusals():
    def bad(cls, match, **c):
        with pytest.raises(ValueError, match=match):
            cls(**c)
    bad(envs.MountainCar, r"unknown constant 'mass'", mass=1.0)
    bad(envs.MountainCar, r"gravity = nan is not finite", gravity=np.nan)
    bad(envs.MountainCar, r"v_max = 0 must be > 0", v_max=0.0)
    bad(envs.MountainCar, r"x_min = 0\.5 must lie below goal = 0\.5", x_min=0.5)
    bad(envs.InvertedPendulum, r"dt = -0\.1 must be > 0", dt=-0.1)
    bad(envs.InvertedPendulum, r"l = 0 must be > 0", l=0.0)
    bad(envs.InvertedPendulum, r"alpha \* m = 1\.5 must lie below 4/3", alpha=0.75)
    bad(envs.InvertedPendulum, r"theta_max = inf is not finite", theta_max=np.inf)
    assert envs.is_control(envs.MountainCar()) and envs.is_control(envs.InvertedPendulum()) and not envs.is_control(envs.SimpleGridWorld()) and not envs.is_tabular(envs.MountainCar())
    h = envs.InvertedPendulum(n=2, seed=1, init_half=0.3).host_copy(5, seed=4)
    assert h.n == 5 and h.seed == 4 and float(h.c["init_half"]) == 0.3


@pytest.mark.parametrize("name", ["mc_goal", "mc_wall", "mc_clamp", "pend"])
def test_case_table_branch_margins(name):
    """the GPU cases on the twin under random actions: every branch quantity stays further than 1e-9 from its switch point, and the case meets its branches"""
    spec, max_len = CC.cases(envs)[name]
    env = spec.host_copy(32, seed=7)
    rng = np.random.default_rng(0)
    steps, seen, worst = np.zeros(32, np.int64), dict(done=False, wall=False, clamp=False, trunc=False), np.inf
    for _ in range(40):
        env.act(rng.integers(0, 3, 32))
        worst = min(worst, float(env.margin.min()))
        steps += 1
        ended = env.terminated() | (steps >= max_len)
        seen["done"] |= bool(env.terminated().any()); seen["trunc"] |= bool((ended & ~env.terminated()).any())
        if name.startswith("mc"):
            seen["wall"] |= bool(((env.s[:, 0] == -1.2) & (env.s[:, 1] == 0.0)).any()); seen["clamp"] |= bool((np.abs(env.s[:, 1]) == 0.07).any())
        env.reset(ended); steps[ended] = 0
    assert worst > CC.MARGIN, worst
    for k in {"mc_goal": ("done",), "mc_wall": ("wall", "trunc"), "mc_clamp": ("clamp", "trunc"), "pend": ("done",)}[name]:
        assert seen[k], (k, seen)


def test_control_known_answers():
    """a linear network Dense(2, 3) without hidden layer.  MountainCar, Q = [-v, 0, +v] (push with the velocity): the default car reaches the goal.  Pendulum,
    Q = [-(theta + omega), 0, theta + omega]: up for 300 steps from every one of 200 reset draws; always left (Q = [1, 0, 0]) falls.  Recomputed from the twin"""
    r, steps, margin = CC.twin_evaluation(envs.MountainCar(), "mc", 1, 200, 0)
    assert margin > CC.MARGIN and steps < 200 and r == 100.0 - steps
    mc = envs.MountainCar(n=1)
    for k in range(int(steps)):
        mc.act(np.argmax(CC.linear_q("mc", mc.observe()), axis=1))
    assert mc.terminated()[0] and 0.5 <= mc.s[0, 0] < 0.5 + 0.07
    print(f"MountainCar: goal on step {int(steps)} with x = {mc.s[0, 0]:.5f}")
    ip = envs.InvertedPendulum(n=200, seed=5)
    for _ in range(300):
        ip.act(np.argmax(CC.linear_q("pend", ip.observe()), axis=1))
        assert not ip.terminated().any() and ip.margin.min() > CC.MARGIN
    left, fell = envs.InvertedPendulum(n=200, seed=5), np.zeros(200, np.int64)
    for k in range(1, 301):
        left.act(np.zeros(200, np.int64))
        fell[(fell == 0) & left.terminated()] = k
    assert fell.min() > 0 and fell.max() < 300
    print(f"pendulum pushed always left: falls within {fell.min()}-{fell.max()} steps")
