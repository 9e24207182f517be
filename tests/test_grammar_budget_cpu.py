"""The compiler's resource report for the four grammar kernels (no GPU needed: hipcc cross-compiles), obtained as
tests/test_kernel_budget_cpu.py obtains it.  The design's own condition is that the call stack lives in registers -- four 64-bit
words shifted as one 256-bit register, no dynamically indexed local array -- so scratch is 0 for all four.  The VGPR counts are
reported in DESIGN.md ("Grammar-guided decoding"), not bounded here."""
import os
import shutil

import pytest

from test_kernel_budget_cpu import HIPCC, _report

KERNELS = ("grammar_build_kernel", "grammar_apply_kernel", "grammar_advance_kernel", "grammar_reset_kernel")


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")
def test_the_grammar_kernels_use_no_scratch():
    kernels = _report("grammar.hip")
    for sub in KERNELS:
        hits = {n: r for n, r in kernels.items() if sub in n}
        assert len(hits) == 1, f"grammar.hip: no single kernel matching {sub}"
        for name, r in hits.items():
            print(name, r)
            assert r["scratch"] == 0, (name, r)
