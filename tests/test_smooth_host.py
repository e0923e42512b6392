"""CPU-only: the arithmetic of the mesh smoothing (`kernels/smooth_math.h`) in a host program
(tests/native/smooth_host.cpp) that runs the device's lines sequentially on seeded meshes written here, under the address and
undefined-behaviour sanitizers. Its checksums of the smoothed rows and the normals, and its counters, are those of
`pipeline.smooth_mesh`: the header and the numpy restatement state one contract before either meets a GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from burn_depth_amd import pipeline as P
from test_smooth_mesh import STEP, _fan, _grid, _octahedron, _small_fans, _strip

f32 = np.float32


def _fnv1a(a):
    h = 0xcbf29ce484222325
    for b in np.ascontiguousarray(a).view(np.uint8).ravel().tolist():
        h = ((h ^ b) * 0x100000001b3) & ((1 << 64) - 1)
    return h


def _cases():
    xyz, faces = _grid(17, noise=0.01)
    N = len(xyz)
    bad_rows = np.concatenate([xyz, [[np.nan, 0, 0], [0, np.inf, 0], [0, 0, 5000.0]]]).astype(f32)
    bad_faces = np.concatenate([[[0, 1, -1], [0, 1, N + 3], [3, 3, 4], [N, 1, 2], [N + 2, 1, 2]], faces]).astype(np.int32)
    fans = _small_fans(200, seed=5)
    return [("octahedron", *_octahedron(), STEP, 3, 0.5, -0.53, 1),
            ("grid pinned", xyz, faces, STEP, 10, 0.5, -0.53, 1),
            ("grid free", xyz, faces, STEP, 4, 1.0, 0.0, 0),
            ("grid shuffled", xyz, faces[np.random.default_rng(3).permutation(len(faces))], STEP, 10, 0.5, -0.53, 1),
            ("bad corners", bad_rows, bad_faces, STEP, 2, 0.5, -1.0, 0),
            ("strip", *_strip(257), STEP, 2, 0.33, 0.0, 0),
            ("fan", *_fan(1000), STEP, 3, 0.5, -0.53, 0),
            ("small fans", *fans, STEP, 1, 0.77, 0.0, 0),
            ("no faces", xyz, np.zeros((0, 3), np.int32), STEP, 1, 0.5, 0.0, 1),
            ("no rows", np.zeros((0, 3), f32), np.array([[0, 1, 2]], np.int32), STEP, 1, 0.5, 0.0, 1)]


def test_the_header_run_sequentially_on_the_host_equals_the_numpy_reference(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "burn_depth_amd", "csrc")
    exe = str(tmp_path / "smooth_host")
    build = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-I" + csrc, os.path.join(root, "tests", "native", "smooth_host.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-3000:]
    cases, paths = _cases(), []
    for i, (_, xyz, faces, step, iterations, lam, mu, pin) in enumerate(cases):
        paths.append(str(tmp_path / f"mesh{i}.bin"))
        with open(paths[-1], "wb") as f:
            f.write(np.array([len(xyz), len(faces), iterations, pin], np.int32).tobytes())
            f.write(np.array([step, lam, mu], f32).tobytes())
            f.write(np.ascontiguousarray(xyz, f32).tobytes())
            f.write(np.ascontiguousarray(faces, np.int32).tobytes())
    run = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    lines = run.stdout.splitlines()
    assert len(lines) == len(cases)
    for line, (name, xyz, faces, step, iterations, lam, mu, pin) in zip(lines, cases):
        ref = P.smooth_mesh(xyz, faces, step, iterations, lam, mu=mu, pin_boundary=bool(pin), normals=True)
        want = f"xyz {_fnv1a(ref.xyz):016x} normals {_fnv1a(ref.normals):016x} stats " + " ".join(str(v) for v in ref.stats.tolist())
        assert line == want, (name, line, want)
