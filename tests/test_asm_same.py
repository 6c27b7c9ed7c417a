"""tools/asm_same.py on synthetic device-assembly snippets (CPU, milliseconds): what differs between two dumps of one program only because the functions sit in
another translation unit -- the .Lpost_getpc<n> numbering, the function index in local labels, the column of trailing comments -- must compare identical;
one changed operand must not."""
import importlib.util
import os

import pytest

TOOL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "asm_same.py")
spec = importlib.util.spec_from_file_location("asm_same", TOOL)
asm_same = importlib.util.module_from_spec(spec)
spec.loader.exec_module(asm_same)


def function(name, k, getpc, pad, operand="v3"):
    """one function as llc prints it: function index k in its labels, getpc label number, `pad` more spaces in front of trailing comments"""
    sp = " " * (26 + pad)
    return "\n".join([
        "\t.protected\t%s" % name,
        "\t.globl\t%s" % name,
        "\t.p2align\t8",
        "\t.type\t%s,@function" % name,
        "%s:%s; @%s" % (name, sp, name),
        "; %bb.0:",
        "\ts_load_dwordx2 s[0:1], s[4:5], 0x0",
        "\tv_add_f64 v[0:1], v[0:1], v[2:3]",
        "\ts_cbranch_scc0 .LBB%d_2" % k,
        "; %%bb.1:%s; %%if.then" % sp,
        "\ts_getpc_b64 s[2:3]",
        ".Lpost_getpc%d:" % getpc,
        "\ts_add_u32 s2, s2, (.LBB%d_3-.Lpost_getpc%d)&4294967295" % (k, getpc),
        "\ts_addc_u32 s3, s3, (.LBB%d_3-.Lpost_getpc%d)>>32" % (k, getpc),
        "\ts_setpc_b64 s[2:3]",
        ".LBB%d_2:%s; %%for.body" % (k, sp),
        "%s; =>This Inner Loop Header: Depth=1" % sp,
        "\tv_mov_b32_e32 v1, %s" % operand,
        "\ts_branch .LBB%d_2" % k,
        ".LBB%d_3:%s; Loop exit from BB%d_2" % (k, sp, k),
        "\ts_endpgm",
        ".Lfunc_end%d:" % k,
        "\t.size\t%s, .Lfunc_end%d-%s" % (name, k, name),
        "%s; -- End function" % sp,
    ]) + "\n"


HEAD = "\t.text\n\t.amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"\n"
FRAME, CALLEE, AUX = "_ZN4dtrl17dtrl_frame_kernelEv", "_ZN4dtrl13kin_dyn_termsINS_5WSRefEEEvRT_", "_ZN4dtrl15dtrl_gather_f32EPf"
ONLY = "frame_kernel,kin_dyn_terms"


def run(tmp_path, old, new, *opts):
    a, b = tmp_path / "old.s", tmp_path / "new.s"
    a.write_text(old); b.write_text(new)
    return asm_same.main([str(a), str(b)] + list(opts))


def big_unit():
    """the kernels behind an auxiliary kernel, with a data label in front: what a unit with auxiliary kernels and a host class dumps"""
    return HEAD + "\t.type\tlut,@object\nlut:\n\t.long\t1\n" + function(AUX, 0, 0, 0) + function(CALLEE, 1, 3, 0) + function(FRAME, 2, 4, 0) + "\t.type\t__hip_cuid_aaaa,@object\n__hip_cuid_aaaa:\n"


def small_unit(operand="v3"):
    """the same two functions alone: other function indices, other getpc numbers, wider comment column"""
    return HEAD + function(CALLEE, 0, 0, 3) + function(FRAME, 1, 1, 3, operand) + "\t.type\t__hip_cuid_bbbb,@object\n__hip_cuid_bbbb:\n"


def test_moved_functions_compare_identical(tmp_path, capsys):
    assert run(tmp_path, big_unit(), small_unit(), "--only", ONLY) == 0
    out = capsys.readouterr().out
    assert "identical" in out
    # what was left out is named, per file
    assert "not compared in %s: %s" % (tmp_path / "old.s", AUX) in out
    assert "not compared in %s: (none)" % (tmp_path / "new.s") in out


@pytest.mark.parametrize("what", ["getpc", "label", "column"])
def test_each_unit_artefact_alone_is_masked(tmp_path, what):
    base = HEAD + function(FRAME, 1, 1, 0)
    other = HEAD + function(FRAME, 2 if what == "label" else 1, 7 if what == "getpc" else 1, 5 if what == "column" else 0)
    assert base != other
    assert run(tmp_path, base, other, "--only", "frame_kernel") == 0
    if what != "label":   # (a whole-file comparison keeps the function index: the functions sit where they sat)
        assert run(tmp_path, base, other) == 0


def test_changed_operand_is_different(tmp_path, capsys):
    assert run(tmp_path, big_unit(), small_unit("v4"), "--only", ONLY) == 1
    out = capsys.readouterr().out
    assert "DIFFERENT: 1 of" in out and "v_mov_b32_e32 v1, v4" in out
    assert run(tmp_path, small_unit(), small_unit("v4")) == 1


def test_comment_only_lines_and_quoted_semicolons_are_kept(tmp_path):
    base = HEAD + function(FRAME, 0, 0, 0)
    assert run(tmp_path, base, base.replace("; %bb.0:", "; %bb.9:")) == 1
    a = base + "\t.asciz\t\"a;b\"\n"
    assert run(tmp_path, a, a.replace("a;b", "a;c")) == 1


def test_missing_function_is_different(tmp_path, capsys):
    assert run(tmp_path, big_unit(), HEAD + function(FRAME, 0, 0, 0), "--only", ONLY) == 1
    assert "DIFFERENT: functions matching" in capsys.readouterr().out
    assert run(tmp_path, big_unit(), small_unit(), "--only", "no_such_function") == 1


def test_command_line_exit_status(tmp_path):
    import subprocess, sys
    a, b = tmp_path / "a.s", tmp_path / "b.s"
    a.write_text(big_unit()); b.write_text(small_unit("v4"))
    assert subprocess.run([sys.executable, TOOL, str(a), str(b), "--only", ONLY], capture_output=True).returncode == 1
