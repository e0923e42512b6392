"""CPU-only: the union-find of the connected components (`kernels/components_math.h`) in a host program with a
std::atomic policy (tests/native/components_host.cpp describes the shapes): hook and flatten as the device launches them, on one
thread and on up to 16, against a sequential union-find, under the address and undefined-behaviour sanitizers. The loop structure
has to end and to keep parent[v] <= v here, before it meets a GPU."""
import os
import shutil
import subprocess

import pytest


def test_union_find_on_host_threads_equals_the_sequential_labels(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "burn_depth_amd", "csrc")
    exe = str(tmp_path / "components_host")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++20", "-Wall", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I" + csrc, os.path.join(root, "tests", "native", "components_host.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    lines = run.stdout.splitlines()
    assert len(lines) == 2 * 14 and all(line.endswith(": ok") for line in lines), run.stdout
    assert {line.split(" rows")[0].strip() for line in lines} >= {"F = 4097", "strip descending", "fan", "islands", "invalid corners"}
    assert any("threads  1" in line for line in lines) and any("threads  1" not in line for line in lines)
