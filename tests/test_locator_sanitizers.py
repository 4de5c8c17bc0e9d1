"""The candidate grid that host and device location share (build_locator_grid; plain C++, no HIP) compiled with
AddressSanitizer + UndefinedBehaviorSanitizer into a stand-alone program and driven over the meshes of
tests/test_points_host.py (tests/sanitize/locator_grid_driver.cpp): every cell in every bin its box meets, sorted bin
lists without duplicates, and mfgpu_locate_points through the grid equal to a search over all cells.
Sanitizers run on the CPU build only; the locate kernel's indexing is covered by the parity and red-zone tests on the GPU.
The sanitizer runtimes are linked statically, so the program needs nothing of the environment it is started in and the
test leaves that alone."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dealii-cuda_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_locator_grid_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "locator_grid_driver")
    src = [os.path.join(ROOT, "tests", "sanitize", "locator_grid_driver.cpp")] + [
        os.path.join(CSRC, f) for f in ("mfgpu_points_locate.cpp", "mfgpu_transfer_build.cpp", "mfgpu_plan.cpp", "mfgpu_mesh.cpp",
                                        "mfgpu_mesh_adaptive.cpp", "mfgpu_mesh_ball.cpp", "mfgpu_mg_hierarchy.cpp")]
    cc = subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                         "-fno-sanitize-recover=undefined",
                         "-fno-omit-frame-pointer", "-std=c++17", "-I", CSRC, "-I", os.path.join(ROOT, "include"), *src, "-o", exe],
                        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert cc.returncode == 0, cc.stdout[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900, env=env)
    assert run.returncode == 0 and "done bad=0" in run.stdout, run.stdout[-4000:]
    assert "ERROR: AddressSanitizer" not in run.stdout and "runtime error" not in run.stdout, run.stdout[-4000:]
