"""The inputs of the contact-state tests, shared by tests/test_contact_state_host.py (which holds them to their conditions in float64)
and tests/test_gpu_contact_state.py (which never runs on inputs that the reference alone does not pass).  Nothing here runs product code.

Conditions, from the fp32 rows in float64 (contact_state_ref.input_conditions):
  * no candidate within 1e-6 m of the ground: an fp32 height may fall on the other side there, and the count k is compared exactly;
  * no element whose two lowest heights are closer than 1e-5 m: fp32 may then pick the other candidate, whose (x, z) and velocity are
    other numbers.  Shipped Laikago (bodies of 96 .. 588 mesh candidates) has such elements: there, and only there, point_xz, velocity
    and the VJP leave out the elements under 1e-5 m -- at most 5 % of a case's elements; height, depth and count are compared on all."""
import functools

import numpy as np

from contact_state_ref import input_conditions
from generated_robots import GROUND_WRENCH_ROBOTS
from joint_coords_ref import fk_states, load_tpl, random_coords
from test_gpu_state_ops_generated import frozen, gw_states, gw_template, lowered, stride_case

GROUND, GAP, NEAR_TIED_CAP = 1e-6, 1e-5, 0.05
SHIPPED_SETS = 6
SHIPPED_SEED = {"laikago": 7, "human": 8}   # (human 7: two corners of a box 3.9e-8 m apart in height)
STRIDE_COUNTS = [63, 64, 65, 129]
# (free1 scaled: its one candidate and its centre of mass sit at the body's origin -- the quaternion does not enter)
GENERATED_CASES = [(n, k) for n in GROUND_WRENCH_ROBOTS for k in ("tumbled", "shallow", "scaled") if (n, k) != ("free1", "scaled")]
SHIPPED_CASES = [("laikago", "shipped"), ("human", "shipped")]
CASES = GENERATED_CASES + SHIPPED_CASES


@functools.lru_cache(maxsize=None)
def shipped_states(name):
    """eval_fk (float64, rounded to fp32) of random coordinates of a shipped robot, 6 sets, every set moved in y so that its lowest
    candidate is 1 .. 5 mm in the ground."""
    tpl = load_tpl(name)
    seed = SHIPPED_SEED[name]
    q, qd = random_coords(tpl, SHIPPED_SETS, seed=seed)
    bq, bqd = fk_states(tpl, q, qd)
    bq = lowered(tpl, bq, bqd, np.random.RandomState(seed).uniform(0.001, 0.005, SHIPPED_SETS))
    frozen(bq, bqd)
    return bq, bqd


TIED = (3, 67, 70)   # the candidates of the tie template's body 0 that share the lowest y


@functools.lru_cache(maxsize=None)
def tie_case():
    """helpers.chain2 with its contact arrays replaced: body 0 carries 130 candidates of which TIED share the lowest y (-0.05) and
    differ in x and z, all others at least 1 cm higher; body 1 three points.  4 sets, IDENTITY quaternions -- the heights of the tied
    three are then the same number in every dtype (p.y + y exactly: the rotation's other terms are exact zeros) --, the tied three 3 mm
    in the ground, random positions in x and z and random twists."""
    from diffphys_amd import sim
    from helpers import build_template, chain2

    tpl = dict(build_template(chain2(sim.JOINT_REVOLUTE)))
    rng = np.random.RandomState(77)
    pts = rng.uniform(-0.05, 0.05, (133, 3))
    pts[:130, 1] = rng.uniform(-0.04, 0.05, 130)
    pts[list(TIED), 1] = -0.05
    tpl["contact_body"] = np.r_[np.zeros(130, np.int32), np.ones(3, np.int32)]
    tpl["contact_point"] = pts.astype(np.float32)
    tpl["contact_dist"] = np.zeros(133, np.float32)
    tpl["contact_material"] = np.zeros(133, np.int32)
    tpl["shape_materials"] = np.asarray([[1.0e4, 30.0, 1.0e2, 1.0]], np.float32)
    S = 4
    bq = np.zeros((S, 2, 7), np.float32)
    bq[..., 6] = 1.0
    bq[..., 0], bq[..., 2] = rng.uniform(-1, 1, (S, 2)), rng.uniform(-1, 1, (S, 2))
    bq[..., 1] = np.float32(0.05) - np.float32(0.003)
    bqd = (rng.randn(S, 2, 6) * 0.5).astype(np.float32)
    frozen(bq, bqd)
    return tpl, bq, bqd


def case(name, kind):
    """-> (template, body_q [S, nb, 7], body_qd [S, nb, 6]) fp32, read-only"""
    if kind == "shipped":
        return (load_tpl(name),) + shipped_states(name)
    if kind == "stride":
        return stride_case(int(name))
    return (gw_template(name),) + gw_states(name, kind)


@functools.lru_cache(maxsize=None)
def conditions(name, kind):
    """Asserts the conditions above for a case -> (input_conditions' dict, compared [S, nb]: the elements whose point_xz, velocity and VJP
    rows are compared -- all of them, but for Laikago's near-tied ones)."""
    tpl, bq, bqd = case(name, kind)
    C = input_conditions(tpl, bq, bqd)
    tag = "%s %s" % (name, kind)
    assert C["ground"] >= GROUND, "%s: a candidate %.2e m from the ground: pick another seed" % (tag, C["ground"])
    near = C["gap"] < GAP
    print("%s: nearest candidate to the ground %.2e m, smallest gap of the two lowest heights %.2e m, %d of %d elements under %.0e m" % (
        tag, C["ground"], C["gap"].min(), near.sum(), near.size, GAP))
    if (name, kind) == ("laikago", "shipped"):
        assert near.mean() <= NEAR_TIED_CAP, "%s: %d of %d elements near-tied: pick another seed" % (tag, near.sum(), near.size)
    else:
        assert not near.any(), "%s: two lowest heights %.2e m apart: pick another seed" % (tag, C["gap"].min())
    return C, ~near
