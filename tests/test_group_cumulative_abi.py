"""CPU: the boundary of stomp_group_create_flags (include/stomp_engine.h) -- the entry point that
lets a group accept engines with use_cumulative_costs.  The symbol is exported, its argument checks
fail before any engine or device is touched (so they run on a machine without a GPU), the accept
bits compile from C with their values, and the ABI version did not move (a function was added, no
layout changed).  tests/GROUP_CUMULATIVE.md lists the cases."""
import ctypes as C
import os
import subprocess

import pytest

from stomp_motion_planner_icra2011_amd import engine as eng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_entry_point():
    lib = eng.load_library()
    assert hasattr(lib, "stomp_group_create_flags")
    assert "stomp_group_create_flags" in eng.EXPORTED


def create_flags(engines, n, accept, compact, out=True):
    lib = eng.load_library()
    h = C.c_void_p()
    rc = lib.stomp_group_create_flags(engines, n, accept, compact, C.byref(h) if out else None)
    assert not h.value
    return rc, lib.stomp_last_error().decode()


def test_invalid_arguments_are_refused_before_any_engine_is_touched():
    # the engine handles below are never dereferenced: every call must return at its argument checks
    fake = (C.c_void_p * 2)(None, None)
    rc, msg = create_flags(None, 2, eng.STOMP_GROUP_ACCEPT_CUMULATIVE, -1)
    assert rc == -1 and "invalid group arguments" in msg, (rc, msg)
    rc, msg = create_flags(fake, 0, eng.STOMP_GROUP_ACCEPT_CUMULATIVE, -1)
    assert rc == -1 and "invalid group arguments" in msg, (rc, msg)
    rc, msg = create_flags(fake, 2, 3, 0, out=False)
    assert rc == -1 and "invalid group arguments" in msg, (rc, msg)
    rc, msg = create_flags(fake, 2, 4, -1)
    assert rc == -1 and "accept" in msg, (rc, msg)
    rc, msg = create_flags(fake, 2, 3, 2)
    assert rc == -1 and "compact" in msg, (rc, msg)
    rc, msg = create_flags(fake, 2, 3, -2)
    assert rc == -1 and "compact" in msg, (rc, msg)
    # valid flags, null engine handles: still refused without a device
    rc, msg = create_flags(fake, 2, 3, 1)
    assert rc == -1 and "null engine" in msg, (rc, msg)


@pytest.mark.parametrize("compiler,flag,lang", [("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "c++")])
def test_accept_bits_and_abi_version_compile(tmp_path, compiler, flag, lang):
    src = tmp_path / "flags.c"
    src.write_text('#include <stdio.h>\n#include "stomp_engine.h"\n'
                   "int main(void){\n"
                   "  int (*f)(stomp_engine* const*, int32_t, uint32_t, int32_t, stomp_group**) = 0;\n"
                   "  if (sizeof(f) == 0) f = stomp_group_create_flags;   /* the declared type, never linked */\n"
                   '  printf("%u %u %d %d\\n", STOMP_GROUP_ACCEPT_STATE_TERMS, STOMP_GROUP_ACCEPT_CUMULATIVE,\n'
                   "         STOMP_ENGINE_ABI_VERSION, (int)sizeof(stomp_group_options));\n"
                   "  return f != 0;}\n")
    exe = tmp_path / "flags"
    subprocess.check_call([compiler, flag, "-x", lang, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           str(src), "-O1", "-o", str(exe)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["1", "2", "4", "12"]
