"""The lean groups of k_step_pub's two-pair instance over bench.py's trajectory ("lean groups"): per step, the
groups k_cand_entries marked lean, the groups in use, the pairs that fell back to the usual body (pk_observe_lean_stats) and the
particles flagged.  python scripts/gpu_diag_lean.py [particles [landmarks [steps]]]"""
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from parakeet_slam_amd import _lib  # noqa: E402

P = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
L = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
N = int(sys.argv[3]) if len(sys.argv) > 3 else 55
means, covs, scans = bench.synthetic_inputs(L, N)
ws = bench.synthetic_controls(N)
rnd = random.Random(7)
us = [rnd.random() for _ in range(N)]
f = _lib.DeviceFilter(P, L)
f.upload_map(means, covs.reshape(L, 25))
for s in range(N):
    f.step(0.2, ws[s], 0.1, scans[s], us[s], seed=7, draw=s, domain=_lib.PK_WEIGHTS_LOG)
    st = f.observe_lean_stats()
    print("step %2d  marked %2d of %2d groups  fallbacks %6d  flagged %d  pub %r" % (
        s, st["marked"], st["in_use"], st["fallbacks"], f.observe_flagged()[0], f.observe_pub_stats()), flush=True)
f.close()
