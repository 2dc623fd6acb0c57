"""The measurement-informed proposal on growing maps (pk_proposal_grow; DESIGN.md section 4, "The proposal on growing maps") in plain
Python -- the yardstick of tests/test_proposal_grow_host.py and tests/test_gpu_proposal_grow.py.  TEST INFRASTRUCTURE ONLY.  Needs
no GPU.

Composed of grow_ranges_reference / grow_init_reference and range_proposal_reference BY IMPORT, and no algebra is restated: the
growing oracle's inner filter becomes a RangedProposalOracle, and ``propose`` IS SingleSighting.observe -- its bookkeeping loop and
its retirement pass, line for line -- with the inner filter's ``propose`` standing where that method calls the inner ``observe``.  So
the association runs at the predicted pose against the untouched state, spare slots included; the settled matches to confirmed
landmarks condition the draw (ProposalOracle.matches drops potential features); the update runs at the sampled pose; and the loop
then walks the ids the step returned (0 = unmatched) at the pose the inner filter stands at: the sampled one.  A scan without a
finite range is ProposalOracle.propose and Triangulating.add_hypothesis, call for call.
"""
import numpy as np

from oracle.fastslam_oracle import low_variance_ancestors, truth_step

import grow_init_reference as gi
import grow_ranges_reference as gr
import odom_reference as odo
import proposal_reference as pr
from bearing_model_reference import wrapped_scan
from grow_ranges_reference import SingleSighting, SingleSightingOracle, SingleSightingRetiringOracle
from range_bearing_reference import RangeBearingOracle
from range_proposal_reference import RangedProposalOracle


class ProposedGrowth(object):
    """The mix-in, in front of SingleSighting.  ``under_proposal`` (behind ``under_ranges``) re-classes the inner filter;
    ``propose(control, z, blobs, ranges, variances)`` is one step and returns the settled ids."""

    def under_proposal(self):
        assert type(self.f) is RangeBearingOracle
        self.f.__class__ = RangedProposalOracle
        return self

    def propose(self, control, z, blobs, ranges=None, variances=None, fresh=True):
        f = self.f

        def step(scan, ranges=None, variances=None):
            del f.observe  # (the inner propose updates through the class's own observe)
            return f.propose(control, z, scan, ranges, variances, fresh=fresh)

        f.observe = step  # where SingleSighting.observe calls the inner observe, the inner propose runs
        try:
            return SingleSighting.observe(self, blobs, ranges, variances)
        finally:
            f.__dict__.pop("observe", None)


class ProposalGrowOracle(ProposedGrowth, SingleSightingOracle):
    pass


class ProposalGrowRetiringOracle(ProposedGrowth, SingleSightingRetiringOracle):
    pass


# ---------------------------------------------------------------------------------------------------------------- shared scenes
# grow_ranges_reference's four ranged scenes and grow_init_reference's unranged bearing_0.1 / bearing_0.1_retiring, each under the
# twist (the oracle's hard-wired motion noise) and under odometry with ALPHAS: 64 particles, 10 preset + 3 unknown landmarks, 14
# steps, noise seed 6, noise-free wrapped scans.
C = gi.SMALL
L0 = C["L0"]
ALPHAS = (2.0, 0.2, 0.2, 0.2)
MOTIONS = ("twist", "odometry")
RANGED = tuple(gr.SCENES)
UNRANGED = ("bearing_0.1", "bearing_0.1_retiring")
SEED = gr.SEED


def scene_shape(name):
    """(spare slots, reading capacity, retirement (A, M) or None, min_parallax)."""
    if name in gr.SCENES:
        _every, spare, retire, _phantom = gr.SCENES[name]
        return spare, gr.R, retire, gr.MIN_PARALLAX
    _model, mp, R, retire, seed = gi.GPU_SCENES[name]
    assert _model == "bearing" and seed == SEED
    return C["spare"], R, retire, mp


def scene_map(name):
    return gr.scene_map(name) if name in gr.SCENES else gi.small_map()


def scene_oracle(name, P=None, cls=None):
    """The scene's oracle (cls: another pair (plain, retiring) of classes with the same constructors, e.g. the plain growing one)."""
    spare, _R, retire, mp = scene_shape(name)
    world, covs = gi.small_world()
    plain, retiring = cls or (ProposalGrowOracle, ProposalGrowRetiringOracle)
    P = C["P"] if P is None else P
    if retire:
        o = retiring(P, world[:L0], covs[:L0], spare, C["thr"], retire[0], retire[1], min_parallax=mp)
    else:
        o = plain(P, world[:L0], covs[:L0], spare, C["thr"], min_parallax=mp)
    o = o.under_ranges()
    return o.under_proposal() if isinstance(o, ProposedGrowth) else o


def scene_scan(name, world, pose, step):
    """(blobs, ranges or None, variances or None) of the scene's scan."""
    if name in gr.SCENES:
        return gr.scene_scan(name, world, pose, step)
    return wrapped_scan(world, pose), None, None


class Step(object):
    """One step of ``drive``: the oracle has proposed; ``finish()`` resamples it by its own ancestors."""

    def __init__(self, o, s, pose, prev, blobs, rng, var, z, u, control, ids):
        self.o, self.s, self.pose, self.prev, self.blobs, self.rng, self.var = o, s, pose, prev, blobs, rng, var
        self.z, self.u, self.control, self.ids = z, u, control, ids
        self.logw = o.f.logw.copy()
        self.anc = low_variance_ancestors(np.exp(self.logw - np.max(self.logw)), u)
        self.done = False

    def finish(self):
        if not self.done:
            self.o.gather(self.anc)
            self.done = True


def control_of(motion, prev, pose, alphas=ALPHAS):
    if motion == "twist":
        return pr.twist(C["v"], C["w"], C["dt"])
    return pr.odom(odo.delta(prev, pose), alphas)


def drive(name, o, motion, steps=None, seed=SEED):
    """grow_init_reference.drive's drive and random stream with ``propose`` in place of the move and the observe: yields a Step
    behind every step, resampled in the log domain when the caller comes back."""
    world, _ = gi.small_world()
    P = o.f.P
    rs = np.random.RandomState(seed)
    pose = (0.0, 0.0, 0.0)
    for s in range(C["steps"] if steps is None else steps):
        prev, pose = pose, truth_step(pose, C["v"], C["w"], C["dt"])
        blobs, rng, var = scene_scan(name, world, pose, s)
        z, u = rs.standard_normal((P, 3)), float(rs.uniform())
        control = control_of(motion, prev, pose)
        ids = o.propose(control, z, blobs, rng, var)
        st = Step(o, s, pose, prev, blobs, rng, var, z, u, control, ids)
        yield st
        st.finish()
