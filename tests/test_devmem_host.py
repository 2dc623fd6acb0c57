"""No GPU: the bookkeeping of the filter's memory registry (csrc/pk_devmem.hpp) over malloc / free stand-ins that can be told to
fail the k-th allocation.  tests/devmem_host_main.cpp is a program of its own, built as host C++ with the address and
undefined-behaviour sanitizers and run directly; it checks that

  * the byte totals equal the sums over the live blocks after any sequence of alloc / alloc_host / release / reserve,
  * a reserve with need <= cap allocates nothing (and does not wait for the stream),
  * an allocation that fails inside a grouped reserve leaves every member null or registered, and cap == 0,
  * release_all (and the registry's end) leaves no live block,
  * a second release of a block, a release of null and of a pointer that never was a block do nothing.

A report from either sanitizer fails the run."""
import os
import subprocess

from parakeet_slam_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))


def test_registry_bookkeeping_under_sanitizers(tmp_path):
    exe = str(tmp_path / "devmem_host")
    # (host code only: the sanitizers are named for the host compilation alone)
    cmd = [build._hipcc(), "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Xarch_host", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(HERE, "devmem_host_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ)
    # (leaks: the stand-ins keep their own list of what is out, and the program checks it is empty at the end -- the leak checker
    # needs ptrace, which a sandbox may refuse)
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=0"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1"
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "devmem ok", r.stdout
    assert r.stderr.strip() == "", r.stderr  # neither sanitizer had anything to say
