"""ISA check of the built stored-distance 16-lane row kernels (CPU test, no GPU): the same check as
test_isa_rows16_loads.py, on `vecchia_rows16d_kernel`'s four instantiations (one per covariance; the
distances do not depend on d). The loop body is shared source, force-inlined into both kernels, so each
must show the row load's 15 two-read blocks, and no instruction may name one of their in-flight
destination registers before the wait.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import tempfile

import pytest

from test_isa_hazards import LIB, OBJDUMP, _parse
from test_isa_rows16_loads import check_function


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(OBJDUMP)), reason="library or llvm-objdump absent")
def test_stored_form_row_load_registers_untouched_until_the_wait():
    tmp = tempfile.mkdtemp(prefix="gpb_isa_")
    try:
        lib = os.path.join(tmp, "lib.so")
        shutil.copy(LIB, lib)
        subprocess.run([OBJDUMP, "--offloading", lib], cwd=tmp, check=True, capture_output=True)
        kernels, bad = 0, []
        for f in sorted(os.listdir(tmp)):
            if not f.endswith("gfx950"):
                continue
            dis = subprocess.run([OBJDUMP, "-d", "--mcpu=gfx950", os.path.join(tmp, f)], check=True,
                                 capture_output=True, text=True).stdout
            name, instrs = None, []
            for line in dis.splitlines() + ["<end>:"]:
                if line.endswith(">:"):
                    if name and "vecchia_rows16d_kernel" in name:
                        n, b = check_function(instrs)
                        assert n == 15, f"{name}: {n} two-read blocks, expected 15 (columns 1..15)"
                        kernels += 1
                        bad += [f"{name}: {x}" for x in b]
                    name, instrs = line, []
                    continue
                p = _parse(line)
                if p is not None:
                    instrs.append(p)
        assert kernels == 4, f"expected 4 instantiations of the stored-distance row kernel, found {kernels}"
        assert not bad, "in-flight row-load registers touched before the wait:\n" + "\n".join(bad[:10])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
