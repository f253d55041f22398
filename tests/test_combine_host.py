"""The request combiner behind ehx_knn and ehx_set (csrc/ehx_combine.h) on the CPU: tests/host/combine_hammer.cpp includes
nothing but that header, is built by the plain host compiler and runs 64 threads x 200 requests through it with no device.
It checks that every request is served exactly once, that no group mixes k or exceeds its cap, that every request of a failed
group — and no other — sees that group's rc and error text, and that it terminates (its own alarm() guards that)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "embeddinghub_amd", "csrc")


def test_combiner_header_includes_the_standard_library_only():
    src = open(os.path.join(CSRC, "ehx_combine.h")).read()
    includes = [line.split()[1] for line in src.splitlines() if line.startswith("#include")]
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes
    prog = open(os.path.join(ROOT, "tests", "host", "combine_hammer.cpp")).read()
    assert [line.split()[1] for line in prog.splitlines() if line.startswith('#include "')] == ['"ehx_combine.h"']


def test_combine_hammer(tmp_path):
    exe = tmp_path / "combine_hammer"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-Wall", "-Werror", "-I", CSRC,
                           os.path.join(ROOT, "tests", "host", "combine_hammer.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "combine_hammer ok: 12800 requests" in p.stdout
