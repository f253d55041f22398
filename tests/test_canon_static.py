"""CPU-side check that the oracle's distance arithmetic is stated once: the split of a row into body and tail, the residual
join of the inner product and the register ring's schedule each occur in exactly one place of the kernel sources
(csrc/k_canon.h), so a correction to the order is one edit."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "embeddinghub_amd", "csrc")
CANON = "k_canon.h"


def _code(path):
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def _sources():
    paths = sorted(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(CSRC, "*.hip")) +
                   glob.glob(os.path.join(CSRC, "*.cpp")))
    assert os.path.join(CSRC, CANON) in paths, paths
    return {os.path.basename(p): _code(p) for p in paths}


def _counts(pattern, flags=0):
    return {name: len(re.findall(pattern, code, flags)) for name, code in _sources().items()
            if re.search(pattern, code, flags)}


def test_the_body_split_is_stated_once():
    assert _counts(r"dims\s*&\s*~15u") == {CANON: 1}
    assert _counts(r"dims\s*&\s*~3u") == {CANON: 1}
    code = _sources()[CANON]
    split = re.search(r"canon_body\(uint32_t dims\)\s*\{(.*?)\n\}", code, re.S)
    assert split and "dims & ~15u" in split.group(1) and "dims & ~3u" in split.group(1)


def test_the_residual_join_is_stated_once():
    # res + res_tail - 1: both halves turned into distances (1 - sum) inside one add
    join = r"ex_add\(\s*ex_sub\(1\.0f,\s*\w+\),\s*ex_sub\(1\.0f,\s*tail\)\)"
    assert _counts(join) == {CANON: 1}
    # ... and nothing else turns a tail into a distance
    assert _counts(r"ex_sub\(1\.0f,\s*\w*tail\w*\)") == {CANON: 1}
    # the horizontal sum ((p0 + p1) + p2) + p3
    assert _counts(r"ex_add\(ex_add\(ex_add\(\w+(\[\d\])?, \w+(\[\d\])?\), \w+(\[\d\])?\), \w+(\[\d\])?\)") == {CANON: 1}


def test_one_sort_and_one_ring_schedule():
    src = _sources()
    assert not any("wave_sort64_8" in code for code in src.values())
    assert sum(len(re.findall(r"\buint64_t wave_sort64\(", code)) for code in src.values()) == 1
    # the hand-unrolled ring: one steady state and one drain in all of the sources, not one per walker under any name
    everything = "\n".join(src.values())
    assert not ("EHX_GRP_LOAD" in everything and "EHX_LANE_LOAD" in everything)
    assert _counts(r"\+ 5 <= \w+") == {CANON: 1}
    assert _counts(r"\brem\w* >= 3\b") == {CANON: 2}   # the drain: its load and its accumulate of the third block


def test_the_rerank_kernels_use_the_shared_key_rule():
    # the NaN rule of a (distance, id) key lives in dist_key (k_exact_common.h): the re-rank does not restate it
    src = _sources()
    assert "d == d" in src["k_exact_common.h"]
    assert "d == d" not in src["k_select.hip"] and "f32_to_ordered(d)" not in src["k_select.hip"]
    assert len(re.findall(r"\bdist_key\(", src["k_select.hip"])) == 2


def test_row_row_dist_is_a_member_of_the_family():
    src = _sources()
    assert "float row_row_dist(" in src[CANON] and "float row_row_dist(" not in src["k_insert.hip"]
    assert '#include "%s"' % CANON in src["ehx_kernels.h"]
