"""The challenge stream's kernel in the built gfx950 code objects (CPU test:
reads the disassembly only): k_challenge exists once in both libraries and
none of its conditional branches depends on loaded data (tests/isa_taint.py),
so the instruction stream is the same whatever the seeds and draw indices.
Its scratch use is covered with every other kernel's by
tests/test_code_object.py::test_no_scratch_outside_the_allowlist."""
import os

import pytest

import isa_taint
from test_code_object import LIBS, LLVM, ROOT, code_object, demangle


@pytest.mark.parametrize("lib", LIBS)
def test_challenge_kernel_has_no_data_dependent_branch(lib):
    path = os.path.join(ROOT, lib)
    if not os.path.exists(path) or not os.path.exists(f"{LLVM}/llvm-objdump"):
        pytest.skip("library or ROCm LLVM tools not present")
    ks = isa_taint.parse(code_object(path, [f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn"]))
    mine = {sym: ins for sym, ins in ks.items() if demangle(sym) == "k_challenge"}
    assert len(mine) == 1, sorted(demangle(s) for s in ks)[:80]
    (ins,) = mine.values()
    assert isa_taint.data_dependent_branches(ins) == []
