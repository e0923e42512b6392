"""CPU-only: the kernel a 256 x 256 GEMM launch takes (`md::gemm256_form`, csrc/kernels/gemm.hip) against the recorded choice of the
launcher from before the choice had a function of its own (tests/golden/gemm256_form_table.txt; tests/native/gemm_form_table.cpp
describes the sweep and the line format). Nothing is launched; the program is plain host C++."""
import os
import shutil
import subprocess

import pytest


def test_gemm256_form_table_equals_the_recorded_selection(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "burn_depth_amd", "csrc")
    exe = str(tmp_path / "gemm_form_table")
    build = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + csrc,
                            os.path.join(root, "tests", "native", "gemm_form_table.cpp"), "-x", "c++", os.path.join(csrc, "kernels", "gemm.hip"),
                            os.path.join(csrc, "md_common.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    got = run.stdout.splitlines()
    want = open(os.path.join(root, "tests", "golden", "gemm256_form_table.txt")).read().splitlines()
    assert len(got) == len(want), (len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"line {i + 1}: selected\n  {g}\nrecorded\n  {w}"
    # the sweep reaches every form: each kernel family, each epilogue kind a default build launches, the diagnostic build, a refusal
    forms = [w.split(" : ")[1].split() for w in want]
    launched = [f for f in forms if f[0] != "refused"]
    assert {f[0] for f in launched} == {"one_tile", "loop_p", "loop_r"}
    assert {int(f[1]) for f in launched if f[0] == "one_tile"} >= {0, 1, 2, 3, 4, 5, 6, 7, 9, 11}
    loops = {(f[0], f[2], f[3], f[4]) for f in launched if f[0] != "one_tile"}  # (family, fold, qkv, conv): all eight instantiations
    assert loops == {("loop_p", "0", "0", "0"), ("loop_p", "1", "0", "0"), ("loop_p", "0", "1", "0"), ("loop_p", "1", "1", "0"), ("loop_p", "0", "1", "1"),
                     ("loop_r", "0", "0", "0"), ("loop_r", "1", "0", "0"), ("loop_r", "0", "0", "1")}
    assert any(f[0] == "one_tile" and f[5] == "1" for f in launched) and len(launched) < len(forms)
