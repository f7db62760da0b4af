"""The cross-tile stream of the 256-row gemm4 tile (csrc/gemm4.hip ``PIPE``) keeps asm-read fragments in registers
across more code than the plain K loop: a tile's first period, the loop, the two tail periods that stage the next
tile, and (bf16 / lens / GeGLU) the epilogue.  Simulate the LDS counter over every instantiation -- plain, two-source
and streamed -- and over what follows each loop up to the drain of its last reads (isa_check.violations, the check the
extension build runs)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from taboo_brittleness_amd import isa_check  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(isa_check.HIPCC) and shutil.which("hipcc") is None, reason="no hipcc")


@pytest.fixture(scope="module")
def asm():
    return isa_check.compile_asm()


def test_every_variant_keeps_its_outstanding_reads(asm):
    bad = {k: v[:3] for k, v in isa_check.violations(asm).items() if v}
    assert bad == {}


def test_streamed_kernels_exist_with_loop_and_tail(asm):
    ls = isa_check.loops(asm, variants=True)
    for epi in (0, 3, 4, 6):
        key = f"gemm4_kernel<256, {epi}, 0, 1>"
        assert key in ls, sorted(ls)
        pre, body = ls[key]
        tail = isa_check._TAILS[key]
        # a first period in front of the loop, one period in it, two behind it
        assert sum("mfma" in x for x in pre) == 128 and sum("mfma" in x for x in body) == 128, key
        assert sum("mfma" in x for x in tail) == 256, key
        # the first period starts every accumulate chain from the literal 0; no other MFMA does
        assert sum(x.startswith("v_mfma") and x.rstrip().endswith(", 0") for x in pre) == 64, key
        assert not any(x.startswith("v_mfma") and x.rstrip().endswith(", 0") for x in body + tail), key
        # no period spills, the loop's selects no staging source, and neither waits for a whole tile's loads
        for x in body + tail:
            assert not x.startswith("scratch_"), (key, x)
        for x in body:
            assert not x.startswith(("s_cselect", "v_readfirstlane", "v_cndmask")), (key, x)
        assert not any(x.startswith("s_waitcnt") and "vmcnt(0)" in x for x in body), key
    for epi in (1, 2, 5):                     # split-K / JumpReLU / fused head keep the plain loop only
        assert f"gemm4_kernel<256, {epi}, 0, 1>" not in ls
