"""No GPU: the per-scan blocks (csrc/pk_scan_block.hpp) -- where everything lies in the block a scan travels in, and the host code
that fills the maximum-likelihood one (blob_directions, build_blob_grid, ml_scan_fill, ml_scan_ranges).
tests/scan_block_host_main.cpp is a program of its own, built as host C++ with the address and undefined-behaviour sanitizers and
run directly.  Every scan is filled into a heap buffer of exactly ml_scan_worst_bytes -- what stage_ml_scan reserves -- so a write
past the reservation is a report.  It checks

  * the offsets, the upload size and the worst case against the arithmetic stage_ml_scan, enqueue_association, staged_range_offset /
    staged_upload_bytes, upload_known_scan and dense_observe wrote out by hand before, spelled out longhand in the program;
  * that sections do not overlap, that tables, rec32 and the upload size are multiples of 16 and the range rows lie at a multiple
    of 8, that the upload never exceeds the worst case;
  * start non-decreasing and ending at the list length, order a permutation of 0..B-1 ascending inside a cell, every idx9 entry
    < B, rec32 and the exact records the blobs in order, rng_cell[t] == rng[order[t]] with a grid and a plain copy without, a scan
    without range rows the size it has always had; and that a block filled from its own blobs (the staged copy) comes out the same;

over B = 1; B = 7 in one colour cell; B = 64 over 20 cells an axis (the clamp to kGridMax); B = 300 random colours with and without
the duplicated lists, and with the grid given up behind the build; want_grid = false; and B = 7 400 whose duplicated lists pass
65 535 entries, so that n9 falls back to 0 -- two adjacent cells in the interior of a 4 x 3 grid, which nine columns list each (two
cells that ARE the grid are listed by two columns: 2 B entries, far below the limit; the program checks the total it built) -- each
with and without range rows, a third of which are NaN.

A report from either sanitizer fails the run."""
import os
import subprocess

from parakeet_slam_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))


def test_scan_block_under_sanitizers(tmp_path):
    exe = str(tmp_path / "scan_block_host")
    hipcc = build._hipcc()
    # (host code only, as tests/test_persistent_grid_host.py builds its program: pk_kernels.hpp wants HIP's types, no HIP call is made)
    roots = [os.path.dirname(os.path.dirname(p)) for p in (hipcc, os.path.realpath(hipcc))] + ["/opt/rocm"]
    hip_include = next(os.path.join(r, "include") for r in roots if os.path.exists(os.path.join(r, "include", "hip", "hip_runtime.h")))
    cmd = [hipcc, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", hip_include, "-D__HIP_PLATFORM_AMD__=1", "-Xarch_host", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(HERE, "scan_block_host_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=0:abort_on_error=0"  # (the leak checker needs ptrace, which a sandbox may refuse)
    env["UBSAN_OPTIONS"] = "print_stacktrace=1"
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "scan_block ok", r.stdout
    assert r.stderr.strip() == "", r.stderr  # neither sanitizer had anything to say
