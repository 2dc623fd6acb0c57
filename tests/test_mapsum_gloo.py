"""CPU, worlds of 2 and 3 over gloo: ShardedFilter.map_summary (parakeet_slam_amd/sharded.py) -- the all-reduce of the maximum
log-weight, the all-gather of the ranks' moments blocks and Chan's combination in rank order are the product's own; the per-shard
moments come from a test-only OracleShard that answers map_moments from its NumPy state.  Checked in the middle of a multi-step
run -- between the observe and the resample by the weights, behind the balanced exchange uniformly -- against ONE OracleShard
holding all particles (mapsum_reference.py: the two-pass computation and the tolerances)."""
import numpy as np
import pytest
import torch.multiprocessing as mp

from mapsum_reference import check, moments_of, two_pass
from sharded_common import OracleShard, init_gloo, noise, scenario, store_file

L, STEPS, SKEW = 6, 3, 4.0


class MomentsShard(OracleShard):
    def map_moments(self, weighting=0, gmax=None):
        o = self.o
        w = None
        if weighting == 1:
            w = np.exp(o.logw - (o.logw.max() if gmax is None else gmax))
        return moments_of(o.mean, o.cov, o.count, w)


def worker(rank, world, store, P_local, q):
    try:
        init_gloo(rank, world, store)
        from parakeet_slam_amd.sharded import ShardedFilter, TorchComm

        means, covs, scans = scenario(L, STEPS)
        P = P_local * world
        z, us = noise(P, STEPS, 11)
        sf = ShardedFilter(P_local, L, comm=TorchComm(), shard=MomentsShard(P_local, means, covs), placement="balanced")
        res = []
        for s in range(STEPS):
            sf.reset_weights()
            sf.motion(0.2, 0.1, 0.1, z=z[s])
            sf.observe(scans[s], ids=np.arange(1, L + 1))
            sf.f.o.logw += np.linspace(0.0, SKEW, P)[sf.logical_index()]
            a = sf.map_summary("weights")
            sf.resample(float(us[s]), domain=1)
            b = sf.map_summary("uniform")  # behind the exchange
            res.append((a, b, sf.last_migrated))
        q.put((rank, res))
    except Exception:  # pragma: no cover
        import traceback

        q.put((rank, "ERR " + traceback.format_exc()))


def reference_run(P):
    means, covs, scans = scenario(L, STEPS)
    z, us = noise(P, STEPS, 11)
    sh = OracleShard(P, means, covs)
    o, out = sh.o, []
    for s in range(STEPS):
        o.reset_weights()
        o.motion(0.2, 0.1, 0.1, z[s])
        o.observe(scans[s], ids=np.arange(1, L + 1))
        o.logw += np.linspace(0.0, SKEW, P)
        a = two_pass(o.mean, o.cov, o.count, np.exp(o.logw - o.logw.max()))
        tot = sh.shard_block_totals(float(o.logw.max()), 1)
        hi = sh.shard_offspring(tot, 0, P, float(us[s]), True)
        o.gather(np.minimum(np.searchsorted(np.maximum.accumulate(hi[1:]), np.arange(P), side="right"), P - 1))
        out.append((a, two_pass(o.mean, o.cov, o.count)))
    return out


@pytest.mark.parametrize("world,P_local", [(2, 1024), (3, 300)])
def test_sharded_map_summary_is_the_single_filters(world, P_local):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    store = store_file()
    procs = [ctx.Process(target=worker, args=(r, world, store, P_local, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = {}
    for _ in range(world):
        r, res = q.get(timeout=300)
        assert not isinstance(res, str), res
        got[r] = res
    for p in procs:
        p.join(timeout=60)
    ref = reference_run(world * P_local)
    assert sum(got[r][s][2] for r in range(world) for s in range(STEPS)) > 0, "particles must have moved between the ranks"
    for s in range(STEPS):
        for r in range(world):
            check(got[r][s][0], ref[s][0], what="world %d rank %d step %d, by the weights" % (world, r, s))
            check(got[r][s][1], ref[s][1], what="world %d rank %d step %d, behind the exchange" % (world, r, s))
        for r in range(1, world):  # every rank combines the same blocks in the same order
            for k in (0, 1):
                assert np.array_equal(got[r][s][k].mean, got[0][s][k].mean) and np.array_equal(got[r][s][k].cov, got[0][s][k].cov)
                assert got[r][s][k].n_eff == got[0][s][k].n_eff


def make_moments_shard(P, means, covs, immutable=None):
    """Shard factory of the facade's CPU rehearsal (module level: picklable for the spawned ranks)."""
    return MomentsShard(P, means, covs, immutable)


def test_facade_over_two_ranks_answers_with_rank_zeros_estimate():
    """FastSLAM(devices=[0, 1]).map_summary(): the "map_summary" command of the child loop (parakeet_slam_amd/multi.py), against the
    particles' own feature sets as the facade's views hand them out."""
    import random

    import parakeet_slam_amd as pk
    from conftest import load_golden
    from test_multi_facade_gloo import View

    g = load_golden("step_small")
    P, Lg = int(g["P"]), int(g["L"])
    np.random.seed(int(g["seed"]))
    random.seed(int(g["seed"]))
    pk.msgs.Time.set_now(0.0)
    feats = [pk.Feature(mean=g["means0"][l], covar=g["covs0"][l]) for l in range(Lg)]
    fs = pk.FastSLAM(feats, num_particles=P, devices=[0, 1], backend="gloo", _shard_factory=make_moments_shard)
    try:
        tw = pk.msgs.Twist()
        tw.linear.x, tw.angular.z = float(g["v"]), float(g["w"])
        fs.last_control = tw
        t = 0.0
        for s in range(2):
            t += float(g["dts"][s])
            pk.msgs.Time.set_now(t)
            fs.cam_cb(View(pk, g["blobs"][s]))
        got = fs.map_summary()
        sets = [fs.particles[i].feature_set for i in range(P)]
        means = np.array([[fsi[l + 1].mean for l in range(Lg)] for fsi in sets], dtype=np.float64)
        covs = np.array([[fsi[l + 1].covar for l in range(Lg)] for fsi in sets], dtype=np.float64)
        counts = np.array([[fsi[l + 1].update_count for l in range(Lg)] for fsi in sets])
        check(got, two_pass(means, covs, counts), what="facade over two ranks")
        assert sorted(got.as_features()) == list(range(1, Lg + 1))
        with pytest.raises(ValueError):
            fs.map_summary("linear")
    finally:
        fs.close()
