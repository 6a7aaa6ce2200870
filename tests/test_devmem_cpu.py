"""CPU: the owner of the host side's device memory (csrc/devmem.h) as a stand-alone program, and the library's live counters where no device exists.

tests/host/devmem_main.cpp defines the header's four allocator macros to a counting malloc / free that can refuse the k-th request, so the header compiles
with no HIP include.  It is built with AddressSanitizer and UBSan and run directly (its own main, nothing preloaded, nothing loaded into Python); the
sanitizers' exit status is part of the assertion: a leak, a double free or a use after free fails the run even where every CHECK holds."""
import ctypes
import os
import subprocess

import pytest

import __graft_entry__ as ge
import ref
from nets import nature_dueling


def test_devscope_standalone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "devmem_main")
    # (the sanitizer runtimes are linked into the executable: its verdict does not depend on the order in which shared libraries load)
    subprocess.run(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wall", "-Werror",
                    "-I", ge.CSRC, os.path.join(ge.ROOT, "tests", "host", "devmem_main.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    assert r.returncode == 0 and "devmem OK" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_debug_devmem_is_unmoved_by_a_refused_create():
    """dqn_debug_devmem takes no handle; a dqn_engine_create that is refused leaves both counters where they were -- (0, 0) where no device exists"""
    import torch
    pkg = ge.build()
    before = pkg._abi.debug_devmem(pkg.fns())
    net = nature_dueling()
    with pytest.raises(pkg.DQNError):
        pkg.Engine(ref.layers_from_network(net), ref.hparams_for(net, batch_size=4096))      # batch_size > 1024: refused with or without a device
    assert pkg._abi.debug_devmem(pkg.fns()) == before
    if not torch.cuda.is_available():
        assert before == (0, 0)
    assert pkg._abi.PROTOS["debug_devmem"] == [ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)]
    assert pkg.fns()["debug_devmem"](None, None) == 0      # either pointer may be NULL
