"""ISA check of the built 16-lane row kernels (CPU test, no GPU): the row load's two-read form
(vecchia_rows16.hip `lds_read_split2`) issues its LDS reads from inline asm, so the compiler does not
know that their destination registers are still in flight when the statement ends. The source routes
every use through statements that follow an `s_waitcnt lgkmcnt(0)`; this scans the shipped library's
disassembly and checks that, in every instantiation, no instruction names one of those registers
between the read that targets it and that wait (a copy or a spill of the register there would move
stale data).
"""
from __future__ import annotations

import os
import shutil
import subprocess
import tempfile

import pytest

from test_isa_hazards import LIB, OBJDUMP, _parse, _vregs


def check_function(instrs: list[tuple[str, list[str]]]) -> tuple[int, list[str]]:
    """Number of two-read blocks and the instructions that touch an in-flight register before the wait."""
    masks = [i for i, (mn, ops) in enumerate(instrs) if mn == "s_and_b32" and ops[:2] == ["exec_lo", "exec_lo"]]
    if not masks:
        return 0, []
    own = set()   # the blocks' own reads: two in front of the saved mask, two under the narrowed one
    for i in masks:
        block = [i - 3, i - 2, i + 2, i + 3]
        assert all(instrs[k][0] == "ds_read_b64" for k in block), [instrs[k] for k in block]
        assert instrs[i - 3][1][0] == instrs[i + 2][1][0] and instrs[i - 2][1][0] == instrs[i + 3][1][0]
        own.update(block)
    wait = next(k for k in range(masks[-1], len(instrs))
                if instrs[k][0] == "s_waitcnt" and "lgkmcnt(0)" in " ".join(instrs[k][1]))
    pending, bad = set(), []
    for k in range(masks[0] - 3, wait):
        mn, ops = instrs[k]
        regs = set().union(*[_vregs(o.split()[0]) for o in ops]) if ops else set()
        if k in own:
            if _vregs(ops[1].split()[0]) & pending:   # an address register must not be in flight either
                bad.append(f"{mn} {', '.join(ops)}")
            pending |= _vregs(ops[0])
        elif regs & pending:
            bad.append(f"{mn} {', '.join(ops)}")
    return len(masks), bad


def test_checker_flags_a_use_before_the_wait():
    block = [("ds_read_b64", ["v[4:5]", "v1"]), ("ds_read_b64", ["v[6:7]", "v2"]), ("s_mov_b64", ["s[8:9]", "exec"]),
             ("s_and_b32", ["exec_lo", "exec_lo", "0xfffefffe"]), ("s_and_b32", ["exec_hi", "exec_hi", "0xfffefffe"]),
             ("ds_read_b64", ["v[4:5]", "v3"]), ("ds_read_b64", ["v[6:7]", "v0"]), ("s_mov_b64", ["exec", "s[8:9]"])]
    wait = [("s_waitcnt", ["lgkmcnt(0)"])]
    use = [("v_mov_b32_e32", ["v9", "v4"])]
    assert check_function(block + wait + use) == (1, [])
    assert check_function(block + [("v_mul_f64", ["v[10:11]", "v[12:13]", "v[14:15]"])] + wait) == (1, [])
    assert check_function(block + use + wait)[1]


@pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(OBJDUMP)), reason="library or llvm-objdump absent")
def test_row_load_registers_untouched_until_the_wait():
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
                    if name and "vecchia_rows16_kernel" in name:
                        n, b = check_function(instrs)
                        assert n == 15, f"{name}: {n} two-read blocks, expected 15 (columns 1..15)"
                        kernels += 1
                        bad += [f"{name}: {x}" for x in b]
                    name, instrs = line, []
                    continue
                p = _parse(line)
                if p is not None:
                    instrs.append(p)
        assert kernels == 8, f"expected 8 instantiations of the 16-lane row kernel, found {kernels}"
        assert not bad, "in-flight row-load registers touched before the wait:\n" + "\n".join(bad[:10])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
