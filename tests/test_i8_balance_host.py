"""The share planner of the int8 scan's long passes (csrc/ehx_balance.h) on the CPU: tests/host/balance_check.cpp includes
nothing but that header and is built by the plain host compiler.  It feeds random factors, tile counts from 0 to 40 000 and
chunk counts of 8, 64 and 256 and checks that the cover is exact and the bounds monotone, that an XCD's share follows its
factor (zero-tile XCDs included), that the clamp holds, that the first measurement is applied in full and later ones with
gain 1/4, and that a corrupted table or inconsistent factors fall back to the uniform split — the kernel's own arithmetic."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "embeddinghub_amd", "csrc")


def test_planner_header_includes_the_standard_library_only():
    src = open(os.path.join(CSRC, "ehx_balance.h")).read()
    includes = [line.split()[1] for line in src.splitlines() if line.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes
    prog = open(os.path.join(ROOT, "tests", "host", "balance_check.cpp")).read()
    assert [line.split()[1] for line in prog.splitlines() if line.startswith('#include "')] == ['"ehx_balance.h"']


def test_balance_check(tmp_path):
    exe = tmp_path / "balance_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "host", "balance_check.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "balance_check ok" in p.stdout


def test_the_switch_is_a_documented_knob_and_the_hooks_stay_out_of_the_abi():
    env_h = open(os.path.join(CSRC, "ehx_env.h")).read()
    assert 'flag("EHX_I8_BALANCE"' in env_h
    assert "`EHX_I8_BALANCE`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    hooks = open(os.path.join(CSRC, "ehx_testhooks.cpp")).read()
    for name in ("ehx_test_i8_balance_force", "ehx_test_i8_balance_read"):
        assert name in hooks and name not in header
