"""CPU-side checks of the large-k scan route: the pass planner (largek_passes through its test hook, against the Python
mirror of tests/largek_cases.py), the hooks that stay outside the ABI, the knobs, and the resource usage of k_radius.hip
built for gfx950."""
import ctypes as C
import os
import re
import subprocess

import pytest

import largek_cases as lc
from embeddinghub_amd import _lib
from embeddinghub_amd import build as ehx_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ("ehx_test_largek_counters", "ehx_test_largek_plan")


def _plan(n, growth, cap=64):
    raw = C.CDLL(_lib.LIB_PATH)
    raw.ehx_test_largek_plan.restype = C.c_uint32
    raw.ehx_test_largek_plan.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint32)]
    pairs, consts = (C.c_uint32 * (2 * cap))(), (C.c_uint32 * 4)()
    m = raw.ehx_test_largek_plan(n, growth, pairs, cap, consts)
    assert m <= cap
    return [(pairs[2 * i], pairs[2 * i + 1]) for i in range(m)], list(consts)


def test_the_hooks_are_exported_and_not_part_of_the_abi():
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for h in HOOKS:
        assert h not in header and h not in _lib.SYMBOLS and hasattr(raw, h)
    assert "k_radius.hip" in ehx_build.SOURCES and "ehx_largek.cpp" in ehx_build.SOURCES
    assert re.search(r"#define EHX_ABI_VERSION 5\b", header)   # no symbol or struct of the ABI changed
    assert re.search(r"#define EHX_MAX_K 48u\b", header) and re.search(r"#define EHX_MAX_K_PAGED 1024u\b", header)


def test_constants_match_the_model_s():
    _, consts = _plan(20000, 4)
    assert consts == [lc.SAMPLE, lc.K_MIN, lc.K_MAX, lc.MIN_QUERIES]


@pytest.mark.parametrize("growth", [2, 4, 8, 16])
def test_pass_plan(growth):
    S = lc.SAMPLE
    sizes = [1, 255, 256, 257, 16384, 17000, 20000, 40000, S * growth - 1, S * growth, S * growth + 1, S * growth + 257,
             S * growth ** 2, S * growth ** 2 + 1, 10 ** 6, 6250000, 2 ** 32 - 1]
    for n in sizes:
        plan, _ = _plan(n, growth)
        assert plan == lc.passes(n, growth), (n, growth)
        n_tiles = -(-n // lc.TILE)
        # a disjoint cover of all tiles, in order, no empty pass
        t = 0
        for t0, nt in plan:
            assert t0 == t and nt > 0
            t += nt
        assert t == n_tiles
        # every cut but the last lies at the first tile boundary at or beyond S g^j rows (a whole number of tiles: S and the
        # tile are powers of two); the last pass takes the rest
        for j, (t0, nt) in enumerate(plan[:-1], start=1):
            assert (t0 + nt) * lc.TILE == S * growth ** j
        assert (len(plan) == 1) == (n <= S * growth)
        assert n > S * growth ** (len(plan) - 1) or len(plan) == 1


def test_the_default_plan_of_the_gpu_cases():
    assert _plan(20000, 4)[0] == [(0, 16), (16, 48), (64, 15)]
    assert _plan(17000, 4)[0] == [(0, 16), (16, 48), (64, 3)]
    assert _plan(4096, 4)[0] == [(0, 16)]
    assert len(_plan(10 ** 6, 4)[0]) == 5 and len(_plan(6250000, 4)[0]) == 7
    assert _plan(20000, 1)[0] == _plan(20000, 2)[0] and _plan(20000, 99)[0] == _plan(20000, 16)[0]   # clamped to [2, 16]


def test_the_knobs_are_read_in_one_place_and_documented():
    env_h = open(os.path.join(ehx_build.CSRC, "ehx_env.h")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for knob in ("EHX_LARGEK", "EHX_LARGEK_GROWTH", "EHX_LARGEK_MIN_QUERIES"):
        assert '"%s"' % knob in env_h and knob in doc


def test_largek_kernels_use_no_scratch_and_spill_no_vector_registers(tmp_path):
    src = os.path.join(ehx_build.CSRC, "k_radius.hip")
    flags = [f for f in ehx_build.FLAGS if f != "-shared"]
    r = subprocess.run([ehx_build.HIPCC] + flags + ["-Rpass-analysis=kernel-resource-usage", "-x", "hip", "-c", src, "-o",
                                                    str(tmp_path / "k_radius.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = re.findall(r"Function Name: (\S+)", r.stderr)
    for kern, count in (("radius_rerank_kernel", 6), ("radius_seed_kernel", 1)):
        assert sum(kern in n for n in names) == count, names
    assert len(names) == 7
    for what in ("ScratchSize \\[bytes/lane\\]", "VGPRs Spill"):
        vals = re.findall(what + r": (\d+)", r.stderr)
        assert len(vals) == len(names) and all(v == "0" for v in vals), (what, vals)
