"""CPU: the rollout cadence (csrc/rollout_sched.h) as a stand-alone program.

tests/host/rollout_sched_main.cpp includes the header (pure C++ over dqn_rollout_cfg, no HIP include) and holds rollout_due to the reference's loop walked one env
step at a time (both cadences, t in 1..40, n in {1, 3, 4, 8, 1024}, train_freq in {0, 1, 2, 3, 4, 7, 16, 17}, target_update_freq in {0, 1, 5, 6, 25}) and
rollout_unit to soundness against that per-step law.  It is built with AddressSanitizer and UBSan and run directly (its own main, nothing preloaded, nothing
loaded into Python); the sanitizers' exit status is part of the assertion."""
import os
import re
import subprocess

import __graft_entry__ as ge


def test_rollout_sched_standalone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "rollout_sched_main")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wall", "-Werror",
                    "-I", ge.CSRC, os.path.join(ge.ROOT, "tests", "host", "rollout_sched_main.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "rollout_sched OK" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_the_cadence_is_written_nowhere_else_in_the_env_loop():
    """the two host files of the env loop read every train / sync decision from rollout_sched.h: no modulus by a frequency, no env-step quotient of their own"""
    for name in ("engine_envs.hip", "engine_group.hip"):
        src = open(os.path.join(ge.CSRC, name)).read()
        for pat in (r"%\s*[\w.>-]*train_freq", r"%\s*[\w.>-]*target_update_freq", r"\(t \* n\) /"):
            assert not re.search(pat, src), (name, pat)
        assert "rollout_due(" in src
