"""CPU-side checks of the ownership rule of the host sources: every raw allocation / creation / destruction call of the
HIP runtime lives in the one file that defines the owners (csrc/ehx_own.h), so nothing a space holds on the device can be
created without a destructor behind it; and the live-resource count the owners keep is a test hook, not part of the ABI."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "embeddinghub_amd", "csrc")
OWNERS = "ehx_own.h"
RAW = ["hipMalloc(", "hipFree(", "hipHostMalloc(", "hipHostFree(", "hipEventCreate", "hipEventDestroy(", "hipStreamCreate",
       "hipStreamDestroy("]


def _code(path):
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return re.sub(r"//[^\n]*", "", src)


def test_raw_resource_calls_live_in_the_owners_file_only():
    host = sorted(glob.glob(os.path.join(CSRC, "*.cpp"))) + [os.path.join(CSRC, "ehx_internal.h")]
    assert len(host) >= 8, host
    for path in host:
        code = _code(path)
        for tok in RAW:
            assert tok not in code, "%s calls %s...: use an owner of %s" % (os.path.basename(path), tok, OWNERS)
    owners = _code(os.path.join(CSRC, OWNERS))
    for tok in RAW:
        assert tok in owners, "%s does not wrap %s" % (OWNERS, tok)
    assert '#include "%s"' % OWNERS in _code(os.path.join(CSRC, "ehx_internal.h"))


def test_live_resource_hook_is_not_part_of_the_abi():
    from embeddinghub_amd import _lib
    header = open(os.path.join(ROOT, "include", "ehx.h")).read()
    assert "ehx_test_live_resources" not in header
    assert "ehx_test_live_resources" not in _lib.SYMBOLS
    assert "ehx_test_live_resources" in _code(os.path.join(CSRC, "ehx_space.cpp"))
