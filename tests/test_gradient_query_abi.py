"""CPU: the boundary of stomp_engine_query_gradients (include/stomp_engine.h).  The header still
compiles as C99 and C++11 with a call compiled in and the ABI version unchanged, the library exports
the symbol, the ctypes mirror of stomp_gradient_query has the compiler's layout, the NULL and
struct_size refusals are made before any engine or device is touched (so they run on a machine
without a GPU) and write nothing, and the call's host-only validation and table construction
(csrc/query_grad_host.h) run clean in a stand-alone program under the address and undefined-behaviour
sanitizers.  tests/GRADIENT_QUERY.md lists the cases.

Without the feature the symbol and the struct do not exist: every case fails."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from stomp_motion_planner_icra2011_amd import engine as eng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "stomp_engine_query_gradients"


def test_header_compiles_as_c_and_cpp_with_a_call_and_keeps_its_version(tmp_path):
    src = tmp_path / "h.c"
    src.write_text('#include "stomp_engine.h"\n'
                   'int ask(stomp_engine* e, const double* states, double* grad){\n'
                   'stomp_gradient_query q = {0}; q.struct_size = (int32_t)sizeof q; q.num_states = 1;\n'
                   'q.states = states; q.field_bias[2] = 0.5; q.state_gradient = grad; q.in_collision = 0;\n'
                   'return stomp_engine_query_gradients(e, &q);}\n'
                   'int main(void){return STOMP_ENGINE_ABI_VERSION - 4;}\n')
    lib = eng.load_library()._name
    for compiler, flag in (("gcc", "-std=c99"), ("g++", "-std=c++11")):
        exe = tmp_path / ("h_" + compiler)
        subprocess.check_call([compiler, flag, "-x", "c" if compiler == "gcc" else "c++", "-Wall", "-Werror",
                               "-Wno-missing-field-initializers", "-I", os.path.join(ROOT, "include"), str(src),
                               "-o", str(exe), "-x", "none", lib, "-Wl,-rpath," + os.path.dirname(lib)])
        assert subprocess.call([str(exe)]) == 0          # STOMP_ENGINE_ABI_VERSION stays 4
    assert eng.ABI_VERSION == 4


def test_header_declares_and_library_exports_the_symbol():
    with open(os.path.join(ROOT, "include", "stomp_engine.h")) as f:
        text = f.read()
    lib = eng.load_library()
    assert re.search(r"^int " + NAME + r"\(stomp_engine\* e, const stomp_gradient_query\* q\);", text, re.M)
    assert hasattr(lib, NAME) and NAME in eng.EXPORTED
    # the state query's comment keeps its sentence and points here; the descent's rules are named as not applying
    assert "no gradient" in text and "distance_field" in text
    assert "1e-10" in text and "not of this service" in text


def test_struct_layout_matches_c(tmp_path):
    cls = eng.stomp_gradient_query
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "stomp_engine.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(stomp_gradient_query));']
    for field, _ in cls._fields_:
        lines.append(f'printf("{field} %zu\\n", offsetof(stomp_gradient_query, {field}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    out = dict(l.rsplit(" ", 1) for l in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(out["size"]) == C.sizeof(cls)
    for field, _ in cls._fields_:
        assert int(out[field]) == getattr(cls, field).offset, field
    assert [f for f, _ in cls._fields_][0] == "struct_size"


def test_null_and_struct_size_are_refused_before_any_engine_is_touched():
    lib = eng.load_library()
    dp = C.POINTER(C.c_double)
    states = np.array([0.1, 0.2, 0.3, 0.4])
    sentinel = -7.25
    grad = np.full(4, sentinel)
    flag = np.full(1, 201, np.uint8)
    # a handle that is not null and never dereferenced: every call must return at its argument checks
    fake = C.cast(C.create_string_buffer(4096), C.c_void_p)

    def query(size=C.sizeof(eng.stomp_gradient_query), st=states):
        q = eng.stomp_gradient_query()
        q.struct_size = size
        q.num_states = 1
        q.states = st.ctypes.data_as(dp) if st is not None else None
        q.state_gradient = grad.ctypes.data_as(dp)
        q.in_collision = flag.ctypes.data_as(C.POINTER(C.c_uint8))
        return q

    def call(*args):
        rc = lib.stomp_engine_query_gradients(*args)
        return rc, lib.stomp_last_error().decode()

    good = query()
    rc, msg = call(None, C.byref(good))
    assert rc == -1 and "null engine" in msg, (rc, msg)
    rc, msg = call(fake, None)
    assert rc == -1 and "null query" in msg, (rc, msg)
    for size in (0, C.sizeof(eng.stomp_gradient_query) - 8, C.sizeof(eng.stomp_gradient_query) + 8):
        bad = query(size=size)
        rc, msg = call(fake, C.byref(bad))
        assert rc == -1 and "struct_size" in msg, (size, rc, msg)
    bad = query(st=None)
    rc, msg = call(fake, C.byref(bad))
    assert rc == -1 and "null states" in msg, (rc, msg)
    assert (grad == sentinel).all() and flag[0] == 201           # nothing was written


def test_host_validation_and_tables_run_clean_under_the_sanitizers(tmp_path):
    # a stand-alone program with its own main (nothing that loads into Python is run under a sanitizer)
    exe = tmp_path / "host_check"
    subprocess.check_call(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "stomp_motion_planner_icra2011_amd", "csrc"),
                           os.path.join(ROOT, "tests", "gradient_query_host_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "host check passed" in r.stdout, r.stdout
