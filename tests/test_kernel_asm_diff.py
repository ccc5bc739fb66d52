"""scripts/kernel_asm_diff.py on hand-written assembly: what it ignores (comments, the function
number of block labels, the symbol's own name, the kernarg size) and what it reports."""
import os
import subprocess
import sys

TOOL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "kernel_asm_diff.py")

FUNC = """\t.globl\t{name}
\t.type\t{name},@function
{name}: ; @{name}
; %bb.0:
\ts_load_dword s2, s[0:1], 0x0 ; a comment
\ts_cbranch_scc1 .LBB{n}_2

\tv_mov_b32_e32 v0, {imm}
.LBB{n}_2:
\ts_endpgm
\t.amdhsa_kernel {name}
\t\t.amdhsa_kernarg_size {kernarg}
\t\t.amdhsa_next_free_vgpr {vgpr}
\t.end_amdhsa_kernel
.Lfunc_end{n}:
\t.size\t{name}, .Lfunc_end{n}-{name}
"""


def _asm(path, *funcs):
    path.write_text("\t.text\n" + "".join(
        FUNC.format(name=name, n=n, imm=kw.get("imm", 1), kernarg=kw.get("kernarg", 72), vgpr=kw.get("vgpr", 8))
        for n, (name, kw) in enumerate(funcs)))
    return str(path)


def _run(old, new, *maps):
    cmd = [sys.executable, TOOL, "--old", *old, "--new", *new]
    for m in maps:
        cmd += ["--map", m]
    out = subprocess.run(cmd, capture_output=True, text=True)
    return out.returncode, out.stdout


def test_identical_across_files_names_and_label_numbers(tmp_path):
    a = _asm(tmp_path / "a.s", ("plain_k", {}))
    b = _asm(tmp_path / "b.s", ("other_k", {}), ("drop_k", {"imm": 2}))  # drop_k is function 1 here
    c = _asm(tmp_path / "c.s", ("merged_k", {"imm": 2, "kernarg": 76}), ("plain_k", {}), ("other_k", {}))
    rc, out = _run([a, b], [c], "^drop_k$=merged_k")
    assert rc == 0, out
    lines = {ln.split()[0]: ln for ln in out.splitlines() if ln and not ln.startswith(" ")}
    assert "IDENTICAL (" in lines["plain_k"] and "IDENTICAL (" in lines["other_k"]
    assert "IDENTICAL but .amdhsa_kernarg_size" in lines["merged_k"]
    assert "-.amdhsa_kernarg_size 72" in out and "+.amdhsa_kernarg_size 76" in out


def test_an_instruction_or_a_register_count_is_a_difference(tmp_path):
    a = _asm(tmp_path / "a.s", ("k", {}))
    for kw, shown in (({"imm": 3}, "+v_mov_b32_e32 v0, 3"), ({"vgpr": 9}, "+.amdhsa_next_free_vgpr 9")):
        rc, out = _run([a], [_asm(tmp_path / "b.s", ("k", kw))])
        assert rc == 1 and "DIFFERENT" in out and shown in out, out


def test_a_function_on_one_side_only_is_a_difference(tmp_path):
    a = _asm(tmp_path / "a.s", ("k", {}), ("gone_k", {}))
    rc, out = _run([a], [_asm(tmp_path / "b.s", ("k", {}))])
    assert rc == 1 and "ONLY IN OLD" in out, out
