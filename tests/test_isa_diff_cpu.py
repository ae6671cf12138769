"""scripts/isa_diff.py on canned assembly: what counts as the same kernel,
what as a different one, and a kernel that only one side has."""
import importlib.util
import io
import os

SPEC = importlib.util.spec_from_file_location(
    "isa_diff", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "scripts", "isa_diff.py"))
isa_diff = importlib.util.module_from_spec(SPEC)
SPEC.loader.exec_module(isa_diff)


def _kernel(name, index, body, vgprs=8, comment="first"):
    """One kernel as the compiler lays it out: label, code, .amdhsa_kernel
    block, .Lfunc_end; `index` is the function's number in its unit."""
    code = "\n".join(f"\t{line}" for line in body)
    return f"""\t.globl\t{name}
{name}: ; @{name}
; %bb.0: ; {comment}
{code}
\ts_cbranch_scc1 .LBB{index}_2 ; {comment}
.LBB{index}_2:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {name}
\t\t.amdhsa_next_free_vgpr {vgprs}
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{index}:
\t.size\t{name}, .Lfunc_end{index}-{name}
; NumVgprs: {vgprs} ; {comment}
"""


def _unit(kernels, lds=0):
    """kernels: (name, body) in the unit's order -> the listing with metadata."""
    text = "".join(_kernel(n, i, b) for i, (n, b) in enumerate(kernels))
    meta = "".join(f"""  - .agpr_count:     0
    .args:
      - .offset:         0
        .size:           8
    .group_segment_fixed_size: {lds}
    .name:           {n}
    .symbol:         {n}.kd
    .vgpr_count:     8
""" for n, _ in kernels)
    return f"\t.text\n{text}\t.amdgpu_metadata\n---\namdhsa.kernels:\n{meta}amdhsa.target:   amdgcn-amd-amdhsa--gfx950\n...\n"


A = ("_Z1aPf", ["v_mov_b32_e32 v0, 0", "global_store_dword v1, v0, s[0:1]"])
B = ("_Z1bPf", ["v_add_f32_e32 v0, v0, v0"])


def _compare(old, new):
    out = io.StringIO()
    bad = isa_diff.compare(old, new, out=out)
    return bad, {line.split()[-1]: line for line in out.getvalue().splitlines()[:-1]}


def test_same_up_to_comments_and_block_numbering():
    old = _unit([A, B])
    new = _unit([B, A]).replace("first", "second")  # other order: other .LBB<n>_ numbers
    assert old != new
    bad, lines = _compare(old, new)
    assert bad == 0
    assert all(line.startswith("same") for line in lines.values()) and sorted(lines) == [A[0], B[0]]


def test_one_changed_line_names_the_kernel():
    old = _unit([A, B])
    new = _unit([A, (B[0], ["v_add_f32_e32 v0, v0, v1"])])
    bad, lines = _compare(old, new)
    assert bad == 1
    assert lines[A[0]].startswith("same")
    assert lines[B[0]].startswith("different (code)")


def test_descriptor_and_metadata_count():
    old = _unit([A])
    bad, lines = _compare(old, old.replace(".amdhsa_next_free_vgpr 8", ".amdhsa_next_free_vgpr 9"))
    assert bad == 1 and lines[A[0]].startswith("different (code)")
    bad, lines = _compare(old, _unit([A], lds=64))
    assert bad == 1 and lines[A[0]].startswith("different (metadata)")


def test_kernel_on_one_side_only():
    bad, lines = _compare(_unit([A, B]), _unit([A]))
    assert bad == 1 and lines[B[0]].startswith("only in old") and lines[A[0]].startswith("same")
    bad, lines = _compare(_unit([A]), _unit([A, B]))
    assert bad == 1 and lines[B[0]].startswith("only in new")


def test_exit_status(tmp_path):
    old, new = tmp_path / "old.s", tmp_path / "new.s"
    old.write_text(_unit([A, B]))
    new.write_text(_unit([A, B]))
    assert isa_diff.main([str(old), str(new)]) == 0
    new.write_text(_unit([A]))
    assert isa_diff.main([str(old), str(new)]) == 1
