"""The two state ops -- joint coordinates (PD_POSE_JOINT_COORDS) and the ground-contact wrench (PD_POSE_GROUND_WRENCH), forward and VJP
kernels of ppr-diffphys_amd/csrc/pd_pose.hip -- on GENERATED robots (tests/generated_robots.py) and adversarial states, on a real MI355X
(run with -m gpu).  The shipped templates leave most of these kernels' arithmetic unexercised: turned child frames (q_off), revolute
joints on rotated joint_X_p with general axes, mixed joint types, 8 children, a non-FREE root, nb up to 256 and every sets-per-workgroup
case of the VJP; tumbled, far-away, grazing and un-normalised bodies, contact_dist > 0, one candidate, lane-stride candidate counts.

References: tests/joint_coords_ref.py (held to oracle/ref_torch.py on these robots by tests/test_state_ops_generated_host.py) and
tests/ground_wrench_common.py over oracle/ref_torch.py eval_body_contacts, in float64, given the SAME fp32 states as the GPU.
Bar (the project's: test_gpu_joint_coords.bar, test_gpu_ground_wrench.check), per tensor: relmax(GPU, f64) <= max(4 x relmax(fp32 torch,
f64), 1e-5), every output finite; and an input-quality condition, in every comparison: the fp32 torch evaluation is itself within 1e-4
of float64 (a seed that breaks it has put the reference on a branch edge: change the seed).  Every comparison prints GPU / fp32 / bar;
no element is ever excluded.  Measured on one MI355X: DESIGN.md section 8."""
import functools

import numpy as np
import pytest
import torch

from gpu_harness import FWD, dev, dev_inputs  # noqa: F401
from generated_robots import GROUND_WRENCH_ROBOTS, ROBOTS, robot, rollout_inputs
from ground_wrench_common import candidate_probe, wrench_and_state_grads
from helpers import build_template, chain2, relmax
from joint_coords_ref import coords_of, fk_states, joint_coords, oracle_template, random_coords, tangent

pytestmark = pytest.mark.gpu

RATES = ["generalized", "measured"]
# state sets per robot for the joint coordinates: S * nb crosses 256-element boundaries (inside a set wherever nb does not divide 256),
# the VJP's last workgroup (256 // nb whole sets) is partly filled and there are at least two where nb <= 128; S * nb <= 600
SETS = {"mixed25": 23, "rev64": 9, "cmp31": 17, "mixed129": 3, "rev256": 2, "world5": 103, "free1": 300}
# state sets per robot for the tumbled / shallow ground-wrench states
GW_SETS = {"mixed25": 12, "rev64": 5, "cmp31": 10, "mixed129": 3, "free1": 200}
GW_SEED = {"mixed25": 0, "rev64": 1, "cmp31": 0, "mixed129": 0, "free1": 0}   # (rev64: 0 puts the fp32 yardstick 1.2e-4 from float64)
STRIDE_SEED = 1000   # (900: a candidate 9e-7 m from the ground at k = 64)


def bar(what, gpu, f32, ref, floor=1e-5):
    e_gpu, e_32 = relmax(gpu, ref), relmax(f32, ref)
    lim = max(4 * e_32, floor)
    print("%s: GPU %.2e / fp32 torch %.2e / bar %.2e" % (what, e_gpu, e_32, lim))
    assert np.isfinite(np.asarray(gpu)).all(), what
    assert e_32 <= 1e-4, "%s: the fp32 torch evaluation is %.2e from float64 -- a branch edge in the inputs: change the seed" % (what, e_32)
    assert np.isfinite(e_gpu) and e_gpu <= lim, "%s: GPU error %.2e vs fp32 torch %.2e" % (what, e_gpu, e_32)
    return lim


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)


# ------------------------------------------------------------------------------------------------------------------ joint coordinates
@functools.lru_cache(maxsize=None)
def fk_case(name):
    """eval_fk (float64, rounded to fp32) of random coordinates with 0.05 <= |angle| <= 1 and random unit root quaternions."""
    tpl = robot(name)
    S = SETS[name]
    q, qd = random_coords(tpl, S, seed=300 + S, lo=0.05, hi=1.0)
    bq, bqd = fk_states(tpl, q, qd)
    frozen(q, qd, bq, bqd)
    return dict(tpl=tpl, S=S, nb=int(tpl["nb"]), nq=int(tpl["nq"]), nqd=int(tpl["nqd"]), q=q, qd=qd, bq=bq, bqd=bqd)


@functools.lru_cache(maxsize=None)
def vjp_seeds(name):
    C = fk_case(name)
    rng = np.random.RandomState(17)
    g_q, g_qd = rng.randn(C["S"], C["nq"]).astype(np.float32), rng.randn(C["S"], C["nqd"]).astype(np.float32)
    frozen(g_q, g_qd)
    return g_q, g_qd


@functools.lru_cache(maxsize=None)
def restated(name, rates, dtype):
    """(joint_q, joint_qd, g_body_q, g_body_qd) of the restatement and its autograd in ``dtype``: computed once, shared by the tests."""
    C = fk_case(name)
    out = coords_of(C["tpl"], dtype, C["bq"], C["bqd"], rates, *(g.copy() for g in vjp_seeds(name)))
    frozen(*out)
    return out


def rows13(bq, bqd, dev):
    return torch.from_numpy(np.concatenate([bq, bqd], -1).reshape(-1, 13)).to(dev)


@functools.lru_cache(maxsize=None)
def gpu_joint_table(name, rates):
    from diffphys_amd import hip_backend

    return hip_backend.joint_table(robot(name), rates, torch.device("cuda:0"))


def test_the_launch_shapes_are_the_ones_meant():
    """What SETS promises, checked against the kernels' mapping: forward 256 elements per workgroup, VJP 256 // nb sets per workgroup."""
    seen = set()
    for name, S in SETS.items():
        nb = int(robot(name)["nb"])
        per_wg = 256 // nb
        assert S * nb > 256 and S * nb <= 600
        assert S % per_wg != 0 or per_wg == 1             # the last VJP workgroup is partly filled
        assert nb > 128 or -(-S // per_wg) >= 2           # at least two workgroups
        if 256 % nb:
            assert any((k * 256) % nb for k in range(1, S * nb // 256 + 1))   # a forward workgroup boundary inside a set
        seen.add((per_wg, 256 - per_wg * nb))
    assert seen == {(10, 6), (4, 0), (8, 8), (1, 127), (1, 0), (51, 1), (256, 0)}   # (sets per workgroup, idle lanes)


@pytest.mark.parametrize("rates", RATES)
@pytest.mark.parametrize("name", list(ROBOTS))
def test_joint_coords_values(name, rates, dev):
    from diffphys_amd import hip_backend

    C = fk_case(name)
    jq, jqd = hip_backend.joint_coords(gpu_joint_table(name, rates), C["nb"], rows13(C["bq"], C["bqd"], dev))
    assert jq.shape == (C["S"], C["nq"]) and jqd.shape == (C["S"], C["nqd"])
    r64, r32 = restated(name, rates, torch.float64), restated(name, rates, torch.float32)
    tag = "%s x %d %s " % (name, C["S"], rates)
    bar(tag + "joint_q", jq.cpu().numpy(), r32[0], r64[0])
    bar(tag + "joint_qd", jqd.cpu().numpy(), r32[1], r64[1])


@pytest.mark.parametrize("rates", RATES)
@pytest.mark.parametrize("name", list(ROBOTS))
def test_joint_coords_vjp(name, rates, dev):
    """g_state of random g_q, g_qd -- the parent-side gather included -- against float64 autograd of the restatement; the quaternion part
    of both projected onto the tangent space of the unit sphere (tests/test_gpu_joint_coords.py says why); two calls, the same bits."""
    from diffphys_amd import hip_backend

    C = fk_case(name)
    nb, S = C["nb"], C["S"]
    g_q, g_qd = vjp_seeds(name)
    args = (gpu_joint_table(name, rates), nb, rows13(C["bq"], C["bqd"], dev), torch.tensor(g_q, device=dev), torch.tensor(g_qd, device=dev))
    g_s = hip_backend.joint_coords_vjp(*args)
    assert g_s.shape == (S * nb, 13)
    assert torch.equal(g_s, hip_backend.joint_coords_vjp(*args))   # fixed summation order: the same bits
    g_s = g_s.cpu().numpy().reshape(S, nb, 13)
    r64, r32 = restated(name, rates, torch.float64), restated(name, rates, torch.float32)
    tag = "%s x %d %s " % (name, S, rates)
    bar(tag + "g_body_q", tangent(g_s[..., :7], C["bq"]), tangent(r32[2], C["bq"]), tangent(r64[2], C["bq"]))
    bar(tag + "g_body_qd", g_s[..., 7:], r32[3], r64[3])
    par = np.asarray(C["tpl"]["joint_parent"]).reshape(nb)
    ty = np.asarray(C["tpl"]["joint_type"]).reshape(nb)
    kids = np.bincount(par[par >= 0], minlength=nb)
    if name == "mixed25":   # a body that gathers 8 children is in the comparison, and every one of the 8 contributes
        assert kids[0] == 8 and np.abs(r64[3][:, 0]).max() > 0
        assert all(np.abs(r64[3][:, c]).max() > 0 or ty[c] == 3 for c in np.flatnonzero(par == 0))
    if name == "world5":    # a non-FREE root (a joint to the world, X_p alone) with children is in the comparison
        assert par[0] == -1 and ty[0] != 4 and kids[0] >= 1 and np.abs(r64[3][:, 0]).max() > 0
    if nb > 1:
        inner = np.flatnonzero(kids >= 1)
        assert np.abs(r64[3][:, inner]).max() > 0


@pytest.mark.parametrize("name", ["mixed25", "cmp31", "world5"])
def test_joint_coords_round_trip_through_the_products_own_kernels(name, dev):
    """ForwardKinematics(InverseKinematics(state)) against the state under the bar of tests/test_gpu_joint_coords.py
    test_round_trip_through_the_products_own_kernels (4 x the round trip of the fp32 torch restatement and eval_fk), and against the same
    round trip in float64 under this file's bar (robots with revolute joints: the 4-decimal axes make either round trip miss the state by
    1e-4, so only the second comparison is sharp there)."""
    from diffphys_amd import dp_model, sim
    from oracle import ref_torch as rt

    C = fk_case(name)
    S, nb = C["S"], C["nb"]
    env = sim.Model.from_template(C["tpl"], S, dev)
    bq = torch.tensor(C["bq"]).to(dev).view(S, 1, nb, 7)
    bqd = torch.tensor(C["bqd"]).to(dev).view(S, 1, nb, 6)
    back_q, back_qd = dp_model.ForwardKinematics.apply(*dp_model.InverseKinematics.apply(bq, bqd, env), env)[:2]
    assert back_q.shape == bq.shape and back_qd.shape == bqd.shape
    back_q, back_qd = back_q.view(S, nb, 7).cpu().numpy(), back_qd.view(S, nb, 6).cpu().numpy()
    trip = {}
    for dtype in (torch.float32, torch.float64):
        T_ = oracle_template(C["tpl"], dtype)
        j = joint_coords(T_, torch.tensor(C["bq"], dtype=dtype), torch.tensor(C["bqd"], dtype=dtype), "generalized")
        trip[dtype] = [a.numpy() for a in rt.eval_fk(T_, *j)]
    for k, (got, what) in enumerate(((back_q, "body_q"), (back_qd, "body_qd"))):
        tag = "%s x %d round trip %s" % (name, S, what)
        e_gpu, e_32 = relmax(got, (C["bq"], C["bqd"])[k]), relmax(trip[torch.float32][k], (C["bq"], C["bqd"])[k])
        print("%s against the state: GPU %.2e / fp32 torch %.2e / bar %.2e" % (tag, e_gpu, e_32, max(4 * e_32, 1e-5)))
        assert np.isfinite(got).all() and e_gpu <= max(4 * e_32, 1e-5)
        bar(tag + " against the float64 round trip", got, trip[torch.float32][k], trip[torch.float64][k])




@functools.lru_cache(maxsize=None)
def sim_case(name):
    """One GPU rollout of a generated robot (generic-joint kernels): bs 3, 8 steps, 3 mm in the ground, frames at states 0, 4, 8 -- run
    only for its joint-violating frame states and its own grf."""
    from diffphys_amd import hip_backend, sim

    dev = torch.device("cuda:0")
    tpl = robot(name)
    inp = rollout_inputs(tpl, bs=3, T=8, seed=1)
    env = sim.Model.from_template(tpl, 3, dev)
    dm = hip_backend.device_model(env)
    t = dev_inputs(inp, dev)
    pos, vel, grf, jaf, ws = dm.rollout_forward(3, 8, inp["dt"], *[t[k] for k in FWD], frame2step=inp["frame2step"])
    return dict(tpl=tpl, inp=inp, env=env, nb=dm.nb, t=t, pos=pos, vel=vel, grf=grf)


@pytest.mark.parametrize("name", ["mixed25", "cmp31"])
def test_joint_coords_of_simulated_states(name, dev):
    """Frames of a rollout: the joints are slightly violated there (x_err != 0, swing != 0, FIXED joints off), which eval_fk-made states
    never are."""
    from diffphys_amd import hip_backend

    C = sim_case(name)
    nb, F = C["nb"], len(C["inp"]["frame2step"])
    assert F == 3
    state = torch.cat([C["pos"], C["vel"]], -1).reshape(-1, 13).contiguous()
    q_np, qd_np = C["pos"].view(F * 3, nb, 7).cpu().numpy(), C["vel"].view(F * 3, nb, 6).cpu().numpy()
    assert np.abs(q_np.reshape(F, 3, nb, 7)[1:] - q_np.reshape(F, 3, nb, 7)[:1]).max() > 1e-4   # it moved
    for rates in RATES:
        jq, jqd = hip_backend.joint_coords(gpu_joint_table(name, rates), nb, state)
        r64, r32 = coords_of(C["tpl"], torch.float64, q_np, qd_np, rates), coords_of(C["tpl"], torch.float32, q_np, qd_np, rates)
        bar("%s simulated %s joint_q" % (name, rates), jq.cpu().numpy(), r32[0], r64[0])
        bar("%s simulated %s joint_qd" % (name, rates), jqd.cpu().numpy(), r32[1], r64[1])
        assert np.abs(r64[1]).max() > 1e-2   # the robot is moving


# ---------------------------------------------------------------------------------------------------------------------- ground wrench
@functools.lru_cache(maxsize=None)
def gw_template(name):
    """The generated robot with DISTINCT material rows (every shape brings its own row, all equal as generated): row m scaled by random
    factors in 0.6 .. 1.4, so that a wrong material index shows."""
    tpl = dict(robot(name))
    M = np.asarray(tpl["shape_materials"], np.float32).reshape(-1, 4).copy()
    M[:, 1] = np.maximum(M[:, 1], 5.0)   # kd > 0: the damping term is in the comparison
    tpl["shape_materials"] = (M * np.random.RandomState(5).uniform(0.6, 1.4, M.shape)).astype(np.float32)
    return tpl


def lowest(tpl, bq, bqd, per_body):
    """float64: the height of the lowest candidate of every state set [S] or, per_body, of every body [S, nb] (inf without candidates)."""
    c = candidate_probe(tpl, np.array(bq), np.array(bqd))[0]
    if not per_body:
        return c.min(1)
    cb = np.asarray(tpl["contact_body"]).reshape(-1)
    out = np.full((c.shape[0], int(tpl["nb"])), np.inf)
    for b in np.unique(cb):
        out[:, b] = c[:, cb == b].min(1)
    return out


def lowered(tpl, bq, bqd, depth, per_body=False):
    """A copy of fp32 states [S, nb, 7] moved in y so that the lowest candidate of every set (every body: per_body, depth [S, nb]) sits
    ``depth`` in the ground -- computed in float64 from the fp32 rows, then rounded: the depth holds to an fp32 ulp of the height."""
    out = np.array(bq, np.float32)
    low = lowest(tpl, out, bqd, per_body)
    shift = np.where(np.isfinite(low), low + depth, 0.0)
    out[..., 1] = (out[..., 1].astype(np.float64) - (shift if per_body else shift[:, None])).astype(np.float32)
    return out


@functools.lru_cache(maxsize=None)
def gw_states(name, kind):
    """fp32 states [S, nb, 7], [S, nb, 6] of a generated robot.
    tumbled: eval_fk of random coordinates, random unit root quaternion, root x and z uniform in +-50 m, every set moved in y so that its
             median body centre is at 0 (about half the bodies under the ground; free1, one body: y uniform in -0.1 .. 0.2)
    shallow: the same sets with the lowest candidate of each 1 .. 5 mm in the ground (unclamped forces, few bodies touch)
    scaled:  the shallow sets with every state quaternion scaled by a random factor in 0.7 .. 1.4 (rows taken as they are), then moved
             again so that the lowest candidate is 1 .. 5 mm in the ground"""
    tpl = gw_template(name)
    S, nb = GW_SETS[name], int(tpl["nb"])
    rng = np.random.RandomState(700 + nb + GW_SEED[name])
    q, qd = random_coords(tpl, S, seed=500 + nb + GW_SEED[name], lo=0.0, hi=1.0)
    q[:, 0], q[:, 2] = rng.uniform(-50, 50, S), rng.uniform(-50, 50, S)
    bq, bqd = fk_states(tpl, q, qd)
    if nb > 1:
        bq[..., 1] = (bq[..., 1].astype(np.float64) - np.median(bq[..., 1].astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    else:
        bq[..., 1] = rng.uniform(-0.1, 0.2, (S, 1)).astype(np.float32)
    depth = rng.uniform(0.001, 0.005, S)
    if kind == "shallow":
        bq = lowered(tpl, bq, bqd, depth)
    elif kind == "scaled":
        bq[..., 3:] *= rng.uniform(0.7, 1.4, (S, nb, 1)).astype(np.float32)
        bq = lowered(tpl, bq, bqd, depth)
    else:
        assert kind == "tumbled"
    frozen(bq, bqd)
    return bq, bqd


@functools.lru_cache(maxsize=None)
def mixed25_table():
    from diffphys_amd import hip_backend

    tpl = gw_template("mixed25")
    nb, nc, nmat = int(tpl["nb"]), len(tpl["contact_body"]), len(tpl["shape_materials"])
    L = hip_backend.contact_table_layout(nb, nc, nmat)
    t = hip_backend.contact_table_host(tpl)
    return tpl, t[L["bodies"]: L["points"]].reshape(nb, 12).astype(np.float64)   # the host table's body rows, as the kernel reads them


def quat_to(d, e, twist):
    """unit quaternion (float64 xyzw) that turns unit vector d onto unit vector e, after a turn by ``twist`` about d"""
    c = np.cross(d, e)
    w = 1.0 + float(d @ e)
    if w < 1e-9:   # opposite: any axis normal to d
        c, w = np.cross(d, [1.0, 0, 0] if abs(d[0]) < 0.9 else [0, 1.0, 0]), 0.0
    a = np.r_[c, w] / np.linalg.norm(np.r_[c, w])
    b = np.r_[d * np.sin(twist / 2), np.cos(twist / 2)]
    av, bv = a[:3], b[:3]
    return np.r_[a[3] * bv + b[3] * av + np.cross(av, bv), a[3] * b[3] - av @ bv]


@functools.lru_cache(maxsize=None)
def grazing_states():
    """mixed25, 6 sets in which EVERY body grazes the early-out of gw_stage: its bounding sphere (centre, radius, largest dist of the host
    table, float64) dips 0.1 .. 1 mm below y = max dist.  Sets 0 .. 2: random orientations -- the lowest candidate is above or below the
    ground as the orientation falls (a body with one candidate, radius 0: always below).  Sets 3 .. 5: a random candidate of the body
    turned straight down, to the very bottom of the sphere -- it touches, by the dip, at the one place where the early-out has no room.
    x, z uniform in +-1 m, random twists.  The bodies of a set need not hang together: the op takes every row on its own."""
    tpl, B = mixed25_table()
    nb, S = int(tpl["nb"]), 6
    rng = np.random.RandomState(41)
    cb = np.asarray(tpl["contact_body"]).reshape(-1)
    cp = np.asarray(tpl["contact_point"], np.float64).reshape(-1, 3)
    bq = np.zeros((S, nb, 7), np.float32)
    quat = rng.randn(S, nb, 4)
    quat /= np.linalg.norm(quat, axis=-1, keepdims=True)
    for s in range(3, S):
        for b in range(nb):
            mine = np.flatnonzero(cb == b)
            d = cp[mine[rng.randint(len(mine))]] - B[b, 5:8]
            if np.linalg.norm(d) > 1e-6:
                quat[s, b] = quat_to(d / np.linalg.norm(d), np.asarray([0.0, -1.0, 0.0]), rng.uniform(-3, 3))
    bq[..., 3:] = quat
    bq[..., 0], bq[..., 2] = rng.uniform(-1, 1, (S, nb)), rng.uniform(-1, 1, (S, nb))
    q = bq[..., 3:].astype(np.float64)   # the fp32 rows, as the kernel gets them
    u, w = q[..., :3], q[..., 3]
    ey = np.asarray([0.0, 1.0, 0.0])
    row1 = ey * (2 * w * w - 1)[..., None] - 2 * w[..., None] * np.cross(u, ey) + 2 * u * u[..., 1:2]   # R^T e_y: height = p_y + row1 . x
    dip = rng.uniform(1e-4, 1e-3, (S, nb))
    assert (B[:, 4] > 0).all()
    bq[..., 1] = (B[:, 9] - dip - (row1 * B[:, 5:8]).sum(-1) + np.linalg.norm(row1, axis=-1) * B[:, 8]).astype(np.float32)
    bqd = (rng.randn(S, nb, 6) * 0.5).astype(np.float32)
    frozen(bq, bqd)
    return bq, bqd


def gw_case(name, kind):
    if kind == "grazing":
        return (gw_template("mixed25"),) + grazing_states()
    return (gw_template(name),) + gw_states(name, kind)


@functools.lru_cache(maxsize=None)
def gw_reference(name, kind, dtype):
    """(wrench, g_body_q, g_body_qd, g_materials) of the torch oracle in ``dtype`` with the g_out of gw_seed: once, shared."""
    tpl, bq, bqd = gw_case(name, kind)
    out = wrench_and_state_grads(tpl, dtype, bq.astype(np.float64), bqd.astype(np.float64), gw_seed(name, kind).copy())
    frozen(*out)
    return out


@functools.lru_cache(maxsize=None)
def gw_seed(name, kind):
    bq = gw_case(name, kind)[1]
    g = np.random.RandomState(3).randn(bq.shape[0], bq.shape[1], 6).astype(np.float32)
    frozen(g)
    return g


@functools.lru_cache(maxsize=None)
def gw_probe(name, kind):
    """float64 per (set, candidate): height, largest |force component| (NaN above the ground); no candidate within 1e-6 m of the ground,
    where an fp32 height may fall on the other side (test_gpu_ground_wrench.assert_off_the_ground)."""
    tpl, bq, bqd = gw_case(name, kind)
    c, fmax = candidate_probe(tpl, bq.astype(np.float64), bqd.astype(np.float64))
    assert np.abs(c).min() >= 1e-6, "%s %s: a candidate %.2e m from the ground: pick another seed" % (name, kind, np.abs(c).min())
    return c, fmax


# (free1 scaled: its one candidate and its centre of mass sit at the body's origin -- the quaternion does not enter)
GW_CASES = [(n, k) for n in GROUND_WRENCH_ROBOTS for k in ("tumbled", "shallow", "scaled") if (n, k) != ("free1", "scaled")] + [("mixed25", "grazing")]


@functools.lru_cache(maxsize=None)
def gpu_contact_table(name):
    from diffphys_amd import hip_backend

    return hip_backend.contact_table(gw_template(name), device=torch.device("cuda:0"))


def test_the_ground_wrench_states_are_the_ones_meant():
    """In float64: per robot at least 20 candidates on the +-500 N clamp and 20 touching below it, bodies with a sphere (dist > 0, one
    candidate) among the touching ones, about half of the tumbled candidates under the ground at up to 50 m from the origin; the
    grazing bodies: both outcomes."""
    for name in GROUND_WRENCH_ROBOTS:
        tpl = gw_template(name)
        dist = np.asarray(tpl["contact_dist"]).reshape(-1)
        n_clamp = n_free = n_sphere = 0
        for kind in ("tumbled", "shallow", "scaled"):
            c, fmax = gw_probe(name, kind)
            n_clamp += int(np.nansum(fmax >= 500.0))
            n_free += int(np.nansum(fmax < 500.0))
            n_sphere += int(((c < 0) & (dist > 0)[None]).sum())
        print("%s: %d candidates on the clamp, %d touching below it, %d of them spheres" % (name, n_clamp, n_free, n_sphere))
        assert n_clamp >= 20 and n_free >= 20 and n_sphere >= 1
        c = gw_probe(name, "tumbled")[0]
        bq = gw_states(name, "tumbled")[0]
        assert np.abs(bq[..., [0, 2]]).max() > 25.0
        if name != "free1":
            assert 0.3 < (c < 0).mean() < 0.7, (c < 0).mean()
        for kind in ("shallow", "scaled"):
            low = gw_probe(name, kind)[0].min(1)
            assert (low <= -0.001 + 1e-6).all() and (low >= -0.005 - 1e-6).all()
        qn = np.linalg.norm(gw_states(name, "scaled")[0][..., 3:].astype(np.float64), axis=-1)
        assert qn.min() < 0.8 and qn.max() > 1.25
    tpl, B = mixed25_table()
    low = lowest(tpl, *grazing_states(), per_body=True)
    gw_probe("mixed25", "grazing")
    assert (low[:3] < 0).any() and (low[:3] > 0).any(), "random orientations: both outcomes"
    assert (low[3:] < 0).all() and (low[3:] > -1.1e-3).all(), "a candidate at the bottom of the sphere touches, by the dip"
    assert (low[:3, B[:, 4] == 1] < 0).all() and (B[:, 4] == 1).any() and (B[B[:, 4] == 1, 9] > 0).all()


@pytest.mark.parametrize("name,kind", GW_CASES)
def test_ground_wrench_values(name, kind, dev, oracle_libs):
    from diffphys_amd import hip_backend

    tpl, bq, bqd = gw_case(name, kind)
    gw_probe(name, kind)
    S, nb = bq.shape[:2]
    out = hip_backend.ground_wrench(gpu_contact_table(name), nb, rows13(bq, bqd, dev)).cpu().numpy().reshape(S, nb, 6)
    w64, w32 = gw_reference(name, kind, torch.float64)[0], gw_reference(name, kind, torch.float32)[0]
    bar("%s %s wrench" % (name, kind), out, w32, w64)
    idle = np.abs(w64).max(-1) == 0   # bodies that touch nothing: exact zeros, from the early-out or from the sweep
    assert (~idle).any() and (out[idle] == 0).all() and (np.abs(out[~idle]).max(-1) > 0).all()
    assert idle.any() or (nb == 1 and kind != "tumbled")   # (one body whose only candidate was put in the ground)


@pytest.mark.parametrize("name,kind", GW_CASES)
def test_ground_wrench_vjps(name, kind, dev, oracle_libs):
    """The state VJP (raw partials: both sides extend off the unit sphere by the same polynomial) and the material VJP, per-element rows
    summed by hip_backend.colsum; two calls, the same bits."""
    from diffphys_amd import hip_backend

    tpl, bq, bqd = gw_case(name, kind)
    gw_probe(name, kind)
    S, nb = bq.shape[:2]
    nmat = len(tpl["shape_materials"])
    args = (gpu_contact_table(name), nb, nmat, rows13(bq, bqd, dev), torch.tensor(gw_seed(name, kind), device=dev).reshape(-1, 6))
    g_s, g_m = hip_backend.ground_wrench_vjp(*args)
    again = hip_backend.ground_wrench_vjp(*args)
    assert g_s.shape == (S * nb, 13) and g_m.shape == (S * nb, nmat, 4)
    assert torch.equal(g_s, again[0]) and torch.equal(g_m, again[1])
    r64, r32 = gw_reference(name, kind, torch.float64), gw_reference(name, kind, torch.float32)
    g_s = g_s.cpu().numpy().reshape(S, nb, 13)
    tag = "%s %s " % (name, kind)
    bar(tag + "g_body_q", g_s[..., :7], r32[1], r64[1])
    bar(tag + "g_body_qd", g_s[..., 7:], r32[2], r64[2])
    bar(tag + "g_materials", hip_backend.colsum(g_m.view(-1, nmat * 4)).cpu().numpy().reshape(nmat, 4), r32[3], r64[3])
    idle = np.abs(r64[0]).max(-1) == 0
    assert (g_s[idle] == 0).all() and (g_m.cpu().numpy().reshape(S, nb, -1)[idle] == 0).all()
    assert np.abs(r64[3]).max() > 0 and np.abs(r64[1]).max() > 0


STRIDE_COUNTS = [1, 63, 64, 65, 128, 129]


@functools.lru_cache(maxsize=None)
def stride_case(k):
    """helpers.chain2 with its contact arrays replaced: body 0 carries k random points on a 5 cm shell, body 1 three points with
    contact_dist 0.02; materials alternate by candidate (the masked per-material sweep); 5 sets, every body in a random orientation with
    its lowest candidate 2 .. 8 mm in the ground."""
    from diffphys_amd import sim

    tpl = dict(build_template(chain2(sim.JOINT_REVOLUTE)))
    rng = np.random.RandomState(STRIDE_SEED + k)
    pts = rng.randn(k + 3, 3)
    pts *= 0.05 / np.linalg.norm(pts, axis=1, keepdims=True)
    pts[k:] += np.asarray([0.0, -0.1, 0.02])
    tpl["contact_body"] = np.r_[np.zeros(k, np.int32), np.ones(3, np.int32)]
    tpl["contact_point"] = pts.astype(np.float32)
    tpl["contact_dist"] = np.r_[np.zeros(k), np.full(3, 0.02)].astype(np.float32)
    tpl["contact_material"] = (np.arange(k + 3) % 2).astype(np.int32)
    tpl["shape_materials"] = np.asarray([[1.0e4, 30.0, 1.0e2, 1.0], [6.0e3, 10.0, 40.0, 0.4]], np.float32)
    S = 5
    bq = np.zeros((S, 2, 7), np.float32)
    bq[..., 0], bq[..., 2] = rng.uniform(-1, 1, (S, 2)), rng.uniform(-1, 1, (S, 2))
    quat = rng.randn(S, 2, 4)
    bq[..., 3:] = quat / np.linalg.norm(quat, axis=-1, keepdims=True)
    bqd = (rng.randn(S, 2, 6) * 0.5).astype(np.float32)
    bq = lowered(tpl, bq, bqd, rng.uniform(0.002, 0.008, (S, 2)), per_body=True)
    frozen(bq, bqd)
    return tpl, bq, bqd


@pytest.mark.parametrize("k", STRIDE_COUNTS)
def test_ground_wrench_lane_stride_edges(k, dev, oracle_libs):
    from diffphys_amd import hip_backend

    tpl, bq, bqd = stride_case(k)
    S = bq.shape[0]
    q64, qd64 = bq.astype(np.float64), bqd.astype(np.float64)
    c, _ = candidate_probe(tpl, q64, qd64)
    assert np.abs(c).min() >= 1e-6, "a candidate %.2e m from the ground: pick another seed" % np.abs(c).min()
    assert ((c[:, :k] < 0).sum(1) >= 1).all() and ((c[:, k:] < 0).sum(1) >= 1).all()
    table = hip_backend.contact_table(tpl, device=dev)
    assert table[4 + 8 + 11].item() == (-1 if k > 1 else 0) and table[4 + 8 + 12 + 11].item() == -1   # mixed materials: the masked sweep
    state = rows13(bq, bqd, dev)
    g_out = np.random.RandomState(4).randn(S, 2, 6).astype(np.float32)
    out = hip_backend.ground_wrench(table, 2, state).cpu().numpy().reshape(S, 2, 6)
    g_s, g_m = hip_backend.ground_wrench_vjp(table, 2, 2, state, torch.from_numpy(g_out).to(dev).reshape(-1, 6))
    r64 = wrench_and_state_grads(tpl, torch.float64, q64, qd64, g_out)
    r32 = wrench_and_state_grads(tpl, torch.float32, q64, qd64, g_out)
    tag = "k = %d " % k
    bar(tag + "wrench", out, r32[0], r64[0])
    g_s = g_s.cpu().numpy().reshape(S, 2, 13)
    bar(tag + "g_body_q", g_s[..., :7], r32[1], r64[1])
    bar(tag + "g_body_qd", g_s[..., 7:], r32[2], r64[2])
    bar(tag + "g_materials", hip_backend.colsum(g_m.view(-1, 8)).cpu().numpy().reshape(2, 4), r32[3], r64[3])
    assert (np.abs(r64[3]).max(1) > 0).all() or k == 1   # both material rows are in the comparison


@pytest.mark.parametrize("name", ["mixed25", "cmp31"])
def test_res_f_plus_op_is_the_generic_rollouts_grf(name, dev):
    """res_f[step] + op(frame state) against the grf the rollout launch itself wrote, on the generic-joint kernels: the candidate terms
    are the same bits, only the order of a few fp32 additions differs (tests/test_gpu_ground_wrench.py
    test_res_f_plus_op_is_the_rollouts_grf: 31 * 2^-24 = 2e-6 < 1e-5)."""
    from diffphys_amd import hip_backend

    C = sim_case(name)
    f2s, T = C["inp"]["frame2step"], C["inp"]["nsteps"]
    frames = [f for f, s in enumerate(f2s) if s < T]
    assert len(frames) == 2
    table = hip_backend.env_contact_table(C["env"], dev)
    for f in frames:
        st = torch.cat([C["pos"][f], C["vel"][f]], -1).contiguous()
        got = C["t"]["res_f"][f2s[f]] + hip_backend.ground_wrench(table, C["nb"], st)
        e = relmax(got.cpu().numpy(), C["grf"][f].cpu().numpy())
        print("%s frame %d: relmax %.2e" % (name, f, e))
        assert e <= 1e-5, (f, e)
    assert C["grf"][frames].abs().max().item() > 10.0
