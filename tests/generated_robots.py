"""Generated robots, shared by scripts/gpu_stress_robots.py (random robots through the rollouts), the state-op tests
(tests/test_state_ops_generated_host.py, tests/test_gpu_state_ops_generated.py) and the rollout tests on fixed generated robots
(ROLLOUT_ROBOTS: tests/test_rollout_generated_host.py, tests/test_gpu_rollout_generated.py): random trees with revolute / compound (the *_R / *_P /
*_Y triples) / fixed joints, random axes and joint frames, box and sphere collisions, as URDF text for the model compiler
(diffphys_amd.import_urdf.parse_urdf).  Nothing here runs product code beyond the model compiler.

A box gives its body 8 contact candidates, a sphere one candidate with contact_dist = its radius (a body with ONE candidate: a bounding
sphere of radius 0); every shape brings its own material row."""
import functools
import os
import tempfile

import numpy as np

from helpers import build_template, free_body


def make_urdf(rng, kinds, n_joints, rotated, branchy, star=0):
    """URDF text of a random tree: a base link and ``n_joints`` joints whose kinds are drawn from ``kinds`` ("rev", "cmp", "fix"); every
    joint adds one body.  rotated: joint origins rotated by up to 0.6 rad per angle and general (4-decimal, so not exactly unit) revolute
    axes, otherwise signed coordinate axes; branchy: a random earlier body as parent, otherwise a chain.  star = k: the first k joints
    hang on the base and no later one does, so that the base has exactly k children.  Every draw comes from ``rng``, in a fixed order
    (star = 0 draws what scripts/gpu_stress_robots.py has always drawn)."""
    def coll():
        o = "%.3f %.3f %.3f" % tuple(rng.uniform(-0.03, 0.03, 3))
        if rng.rand() < 0.6:
            return '<collision><origin xyz="%s"/><geometry><box size="%.3f %.3f %.3f"/></geometry></collision>' % ((o,) + tuple(rng.uniform(0.04, 0.1, 3)))
        return '<collision><origin xyz="%s"/><geometry><sphere radius="%.3f"/></geometry></collision>' % (o, rng.uniform(0.02, 0.05))
    links = ['<link name="base">%s</link>' % coll()]
    joints, bodies = [], ["base"]
    for i in range(n_joints):
        if i < star:
            par = "base"
        elif star:
            par = bodies[1 + rng.randint(len(bodies) - 1)] if branchy else bodies[-1]
        else:
            par = bodies[rng.randint(len(bodies))] if branchy else bodies[-1]
        kind = kinds[rng.randint(len(kinds))]
        xyz = "%.3f %.3f %.3f" % tuple(rng.uniform(-0.12, 0.12, 3))
        rpy = "%.3f %.3f %.3f" % tuple(rng.uniform(-0.6, 0.6, 3)) if rotated else "0 0 0"
        ax = rng.randn(3); ax /= np.linalg.norm(ax)
        if not rotated:
            ax = np.eye(3)[rng.randint(3)] * (1 if rng.rand() < 0.5 else -1)
        axs = "%.4f %.4f %.4f" % tuple(ax)
        if kind == "rev":
            links.append('<link name="L%d">%s</link>' % (i, coll()))
            joints.append('<joint name="j%d" type="continuous"><parent link="%s"/><child link="L%d"/><axis xyz="%s"/><origin xyz="%s" rpy="%s"/><limit effort="1" velocity="1"/></joint>' % (i, par, i, axs, xyz, rpy))
            bodies.append("L%d" % i)
        elif kind == "fix":
            links.append('<link name="F%d">%s</link>' % (i, coll()))
            joints.append('<joint name="j%d" type="fixed"><parent link="%s"/><child link="F%d"/><origin xyz="%s" rpy="%s"/></joint>' % (i, par, i, xyz, rpy))
            bodies.append("F%d" % i)
        else:
            links.append('<link name="c%d_R"/><link name="c%d_P"/><link name="c%d_Y">%s</link>' % (i, i, i, coll()))
            joints.append('<joint name="c%d_R" type="revolute"><parent link="%s"/><child link="c%d_R"/><axis xyz="1 0 0"/><origin xyz="%s" rpy="%s"/><limit lower="-1.5" upper="1.5" effort="1" velocity="1"/></joint>'
                          '<joint name="c%d_P" type="revolute"><parent link="c%d_R"/><child link="c%d_P"/><axis xyz="0 1 0"/></joint>'
                          '<joint name="c%d_Y" type="revolute"><parent link="c%d_P"/><child link="c%d_Y"/><axis xyz="0 0 1"/></joint>' % (i, par, i, xyz, rpy, i, i, i, i, i, i))
            bodies.append("c%d_Y" % i)
    return '<?xml version="1.0"?>\n<robot name="r">\n' + "\n".join(links) + "\n" + "\n".join(joints) + "\n</robot>\n"


def turn_child_frames(tpl, rng):
    """A copy of the template in which every COMPOUND joint's child frame joint_X_c carries a random unit quaternion, angle uniform in
    +-0.8 rad about a random axis (tests/test_gpu_parity.py test_rotated_child_joint_frame_takes_the_generic_kernel turns two)."""
    out = dict(tpl)
    X_c = np.array(tpl["joint_X_c"], np.float32).reshape(int(tpl["nb"]), 7).copy()
    for b in np.flatnonzero(np.asarray(tpl["joint_type"]).reshape(-1) == 5):
        ax = rng.randn(3); ax /= np.linalg.norm(ax)
        ang = rng.uniform(-0.8, 0.8)
        X_c[b, 3:6] = ax * np.sin(ang / 2)
        X_c[b, 6] = np.cos(ang / 2)
    out["joint_X_c"] = X_c
    return out


# name -> (seed, kinds, n_joints, rotated, branchy, star, floating, child frames turned); nb = 1 + n_joints
ROBOTS = {
    "mixed25": (25, ("rev", "cmp", "fix"), 24, True, True, 8, True, True),    # everything at once; a body with 8 children
    "rev64": (64, ("rev",), 63, True, False, 0, True, False),                 # a deep chain, general axes
    "cmp31": (31, ("cmp",), 30, True, True, 0, True, True),                   # q_off everywhere
    "mixed129": (129, ("rev", "cmp", "fix"), 128, True, True, 0, True, False),
    "rev256": (258, ("rev",), 255, True, True, 0, True, False),               # the op's advertised limit (seed: <= 8 children everywhere)
    "world5": (5, ("rev",), 4, True, True, 0, False, False),                  # a root jointed to the world (no FREE joint)
    "free1": None,                                                            # helpers.free_body(): one FREE body
}
GROUND_WRENCH_ROBOTS = ("mixed25", "rev64", "cmp31", "mixed129", "free1")   # rev256: 256 materials, the contact table takes 255


# The robots the ROLLOUTS take (nb <= 64, at most 8 children per body): tests/test_rollout_generated_host.py, tests/test_gpu_rollout_generated.py.
# Same tuple as ROBOTS, with an optional ninth entry: keyword overrides of the import (joint limits).
ROLLOUT_ROBOTS = {
    "mixed25": ROBOTS["mixed25"],                                             # generic, width 32, a body with 8 children, turned frames
    "cmp31": ROBOTS["cmp31"],                                                 # generic through turned child frames only
    "rev64": ROBOTS["rev64"],                                                 # revolute kernels, width 64, depth 64, general axes
    "free1": None,                                                            # one body, one candidate
    "rev12": (12, ("rev",), 11, True, True, 0, True, False),                  # quad-lane eligible: both families, general axes
    "mixed48": (48, ("rev", "cmp", "fix"), 47, True, True, 0, True, True),    # generic at width 64 with tables in LDS
    "cmp20": (20, ("cmp",), 19, True, True, 0, True, False),                  # the compound-only instantiation off the human / quad templates
    "worldmix9": (7, ("rev", "cmp", "fix"), 8, True, True, 0, False, False),   # a world joint with a joint mix (seed: of 1 .. 9 the one whose envs all touch the ground with bodies other than the base)
    "cmp20-limits": (20, ("cmp",), 19, True, True, 0, True, False, dict(limit_ke=40.0, limit_kd=1.0)),   # compound limit forces
}
ROLLOUT_LIMITS = {"cmp20-limits": ((1, 3, 1.62),)}   # rollout_inputs(limits=): env 1 starts with the _R angle of body 3 beyond the limit of 1.5
WORLD_DEPTH = 0.003   # a world-jointed robot of ROLLOUT_ROBOTS: the lowest candidate of its rest pose is this far in the ground


def _import(name, recipe, height):
    from diffphys_amd import sim
    from diffphys_amd.import_urdf import parse_urdf

    seed, kinds, n_joints, rotated, branchy, star, floating, turned = recipe[:8]
    kw = dict(limit_ke=0.0, limit_kd=0.0)
    kw.update(recipe[8] if len(recipe) > 8 else {})
    rng = np.random.RandomState(seed)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, name + ".urdf")
        with open(path, "w") as f:
            f.write(make_urdf(rng, list(kinds), n_joints, rotated, branchy, star))
        b = sim.ModelBuilder()
        parse_urdf(path, b, xform=sim.transform((0, height, 0), sim.quat_identity()), floating=floating, density=1000.0, armature=0.002,
                   stiffness=30.0, damping=0.3, shape_ke=1e4, shape_kd=5.0, shape_kf=1e2, shape_mu=0.5, **kw)
    tpl = build_template(b, attach_ke=3000.0, attach_kd=30.0)
    if turned:
        tpl = turn_child_frames(tpl, rng)
    assert int(tpl["nb"]) == 1 + n_joints
    return tpl


def rest_low(tpl):
    """float64: the height of the lowest contact candidate of the template's rest pose (joint_q, no motion)."""
    import torch

    from ground_wrench_common import candidate_probe
    from oracle import ref_torch as rt

    T64 = rt.Template(tpl, torch.float64)
    q = torch.as_tensor(np.asarray(tpl["joint_q"], np.float64)[None])
    bq, bqd = rt.eval_fk(T64, q, torch.zeros(1, int(tpl["nqd"]), dtype=torch.float64))
    return float(candidate_probe(tpl, bq.numpy(), bqd.numpy())[0].min())


@functools.lru_cache(maxsize=None)
def robot(name):
    """The template dict of a named robot of ROBOTS or ROLLOUT_ROBOTS: built once per process, shared, never written.  A robot of
    ROLLOUT_ROBOTS whose root is jointed to the world cannot be dropped by its inputs (it has no root coordinates): it is imported once
    at the usual height, its lowest rest-pose candidate measured, and imported again with the base WORLD_DEPTH deep in the ground."""
    if name == "free1":
        return build_template(free_body())
    if name in ROBOTS:
        return _import(name, ROBOTS[name], 0.3)
    recipe = ROLLOUT_ROBOTS[name]
    tpl = _import(name, recipe, 0.3)
    if not recipe[6]:
        tpl = _import(name, recipe, 0.3 - (rest_low(tpl) + WORLD_DEPTH))
    return tpl


def rollout_inputs(tpl, bs=3, T=8, seed=0, depth=0.003, limits=()):
    """float32 rollout inputs for a generated robot, the recipe of scripts/gpu_stress_robots.py: joint angles uniform in +-0.3, a random
    yaw, every env dropped so that its lowest contact candidate is ``depth`` in the ground (float64 eval_fk of the torch oracle), small
    twists, torques, residual wrenches and PD targets; frames at states 0, T // 2 and T; dt = 0.5 ms.
    A root jointed to the world has no pose coordinates: no yaw is drawn, every coordinate is a joint angle, every dof has a PD gain and
    no env is shifted (robot() has put the rest pose WORLD_DEPTH into the ground); the draws of a FREE root are what they have always been.
    limits: (env, body, angle) triples -- the first coordinate (the _R angle) of that COMPOUND body's joint starts at ``angle``."""
    import torch

    from ground_wrench_common import candidate_probe
    from oracle import ref_torch as rt

    nb, nq, nqd = int(tpl["nb"]), int(tpl["nq"]), int(tpl["nqd"])
    free = int(np.asarray(tpl["joint_type"]).reshape(-1)[0]) == 4
    rq, rqd = (7, 6) if free else (0, 0)   # the root's pose coordinates and dofs
    rng = np.random.RandomState(seed)
    q = np.tile(np.asarray(tpl["joint_q"], np.float64), (bs, 1))
    q[:, rq:] = rng.uniform(-0.3, 0.3, (bs, nq - rq))
    if free:
        yaw = rng.uniform(-0.5, 0.5, bs)
        q[:, 3:7] = np.stack([0 * yaw, np.sin(yaw / 2), 0 * yaw, np.cos(yaw / 2)], -1)
    qs, ty = np.asarray(tpl["joint_q_start"]).reshape(-1), np.asarray(tpl["joint_type"]).reshape(-1)
    for env, body, angle in limits:
        assert int(ty[body]) == 5, "limits= names COMPOUND bodies"
        q[env, int(qs[body])] = angle
    m1, I1 = np.asarray(tpl["body_mass"], np.float64).copy(), np.asarray(tpl["body_inertia"], np.float64).reshape(nb, 3, 3).copy()
    if not free:   # the importer gives a base that is jointed to the world no mass: it gets the mean of the other bodies', so that it moves
        m1[0], I1[0] = m1[1:].mean(), I1[1:].mean(0)   # on its attachment springs and the world joint carries a load
    mass = np.tile(m1, bs)
    inertia = np.tile(I1, (bs, 1, 1))
    ke = np.tile(np.r_[np.zeros(rqd), np.full(nqd - rqd, 30.0)], bs)
    f2s = sorted(set([0, T // 2, T]))
    F = len(f2s)
    inp = dict(q_init=q.reshape(-1), qd_init=rng.randn(bs * nqd) * 0.1, torques=rng.randn(T, bs * nqd) * 0.05, res_f=rng.randn(T, bs * nb, 6) * 0.05,
               refs=rng.uniform(-0.2, 0.2, (T, bs * nqd)), target_ke=ke, target_kd=ke * 0.01, body_mass=mass, body_inv_mass=1 / mass, body_inertia=inertia,
               body_inv_inertia=np.linalg.inv(inertia), adj_pos=rng.randn(F, bs * nb, 7) * 1e-3, adj_vel=rng.randn(F, bs * nb, 6) * 1e-3)
    inp = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in inp.items()}
    if free:
        T64 = rt.Template(tpl, torch.float64)
        qi = inp["q_init"].reshape(bs, nq).copy()
        bq, bqd = rt.eval_fk(T64, torch.as_tensor(qi, dtype=torch.float64), torch.as_tensor(inp["qd_init"].reshape(bs, nqd), dtype=torch.float64))
        low = candidate_probe(tpl, bq.numpy(), bqd.numpy())[0].min(1)   # the lowest candidate of every env
        qi[:, 1] -= (low + depth).astype(np.float32)
        inp["q_init"] = np.ascontiguousarray(qi.reshape(-1))
    inp.update(frame2step=f2s, nsteps=T, dt=5e-4)
    return inp


def rollout_case(name, T, seed=0, bs=3, every_state=False):
    """(template, rollout_inputs) of a robot of ROLLOUT_ROBOTS, with its ROLLOUT_LIMITS; every_state: every state 0 .. T is a frame (no
    adjoint seeds then: forward only)."""
    tpl = robot(name)
    inp = rollout_inputs(tpl, bs=bs, T=T, seed=seed, limits=ROLLOUT_LIMITS.get(name, ()))
    if every_state:
        inp["frame2step"] = list(range(T + 1))
        del inp["adj_pos"], inp["adj_vel"]
    return tpl, inp


def joint_class(tpl):
    """"revolute", "compound" or "generic": the kernel instantiation the library picks (csrc/pd_host.hip chain_topology) -- a mix of joint
    types, a joint to the world or a child joint frame whose quaternion is not the identity takes the generic one."""
    nb = int(tpl["nb"])
    ty, par = np.asarray(tpl["joint_type"]).reshape(-1), np.asarray(tpl["joint_parent"]).reshape(-1)
    kinds = set(int(t) for t in ty) - {4}
    world = bool(((ty != 4) & (par < 0)).any())
    turned = bool((np.asarray(tpl["joint_X_c"], np.float32).reshape(nb, 7)[:, 3:] != np.asarray([0, 0, 0, 1], np.float32)).any())
    if world or turned or kinds not in ({1}, {5}):
        return "generic"
    return "revolute" if kinds == {1} else "compound"


TENSORS = ("wp_pos", "wp_vel", "grf", "jaf")


def oracle_pair(tpl, inp):
    """(fp32, float64) forward rollouts of the C oracle on the same inputs, the twist evaluation switched as helpers.own_trajectory_check
    switches it: scale-invariant where the robot has FIXED joints (what the kernels evaluate), literal otherwise."""
    from oracle.ref_c import RefC

    has_fixed = 3 in set(int(t) for t in np.asarray(tpl["joint_type"]).reshape(-1))
    out = []
    for dtype in (np.float32, np.float64):
        rc = RefC(tpl, dtype)
        rc.set_twist_eval(has_fixed)
        try:
            out.append(rc.rollout_forward(inp, inp["nsteps"], inp["frame2step"], inp["dt"]))
        finally:
            rc.set_twist_eval(False)
    return out[0], out[1]


def yardstick(st32, st64):
    """per output tensor: the fp32 oracle's relmax error against the float64 one"""
    from helpers import relmax

    return {k: relmax(st32[k], st64[k]) for k in TENSORS}
