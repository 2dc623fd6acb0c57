"""No GPU: persistent_grid (csrc/pk_kernels.hpp), the one function that sizes the grids of the persistent observe kernels
(k_step_regs, k_step_pub, k_step_pub_big, k_step_pub_duo) from the CU count, the workgroups a CU holds, the particle range and the
CUs a split step leaves to the all-to-all.  tests/persistent_grid_host_main.cpp is a program of its own, built as host C++ with the
address and undefined-behaviour sanitizers and run directly; it holds the function to the arithmetic the launchers wrote out one by
one before, over

  * n_cu in {1, 8, 256}, per_cu in {1, 2, 3},
  * reserve_cus in {-1, 0, 1, n_cu - 1, n_cu, n_cu + 1} (a reserve outside (0, n_cu) is ignored),
  * P in {0, 1, 7, 100 000} with the ranges (0, -1) (p1 < 0: all of them), (0, P), (3, 3), (5, 3), (P - 1, P)
    (an empty range: no workgroup; never more workgroups than particles).

A report from either sanitizer fails the run."""
import os
import subprocess

from parakeet_slam_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))


def test_persistent_grid_under_sanitizers(tmp_path):
    exe = str(tmp_path / "persistent_grid_host")
    hipcc = build._hipcc()
    # (host code only: the sanitizers are named for the host compilation alone.  pk_kernels.hpp declares the launchers, so it wants
    # HIP's types: as plain C++ the runtime's headers come from beside the compiler, and no HIP call is made)
    roots = [os.path.dirname(os.path.dirname(p)) for p in (hipcc, os.path.realpath(hipcc))] + ["/opt/rocm"]
    hip_include = next(os.path.join(r, "include") for r in roots if os.path.exists(os.path.join(r, "include", "hip", "hip_runtime.h")))
    cmd = [hipcc, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", hip_include, "-D__HIP_PLATFORM_AMD__=1", "-Xarch_host", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(HERE, "persistent_grid_host_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=0"  # (the leak checker needs ptrace, which a sandbox may refuse)
    env["UBSAN_OPTIONS"] = "print_stacktrace=1"
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "persistent_grid ok", r.stdout
    assert r.stderr.strip() == "", r.stderr  # neither sanitizer had anything to say
