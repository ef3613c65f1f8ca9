"""Generated robots, shared by scripts/gpu_stress_robots.py (random robots through the rollouts) and the state-op tests
(tests/test_state_ops_generated_host.py, tests/test_gpu_state_ops_generated.py): random trees with revolute / compound (the *_R / *_P /
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


@functools.lru_cache(maxsize=None)
def robot(name):
    """The template dict of a named robot of ROBOTS: built once per process, shared, never written."""
    from diffphys_amd import sim
    from diffphys_amd.import_urdf import parse_urdf

    if name == "free1":
        return build_template(free_body())
    seed, kinds, n_joints, rotated, branchy, star, floating, turned = ROBOTS[name]
    rng = np.random.RandomState(seed)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, name + ".urdf")
        with open(path, "w") as f:
            f.write(make_urdf(rng, list(kinds), n_joints, rotated, branchy, star))
        b = sim.ModelBuilder()
        parse_urdf(path, b, xform=sim.transform((0, 0.3, 0), sim.quat_identity()), floating=floating, density=1000.0, armature=0.002,
                   stiffness=30.0, damping=0.3, shape_ke=1e4, shape_kd=5.0, shape_kf=1e2, shape_mu=0.5, limit_ke=0.0, limit_kd=0.0)
    tpl = build_template(b, attach_ke=3000.0, attach_kd=30.0)
    if turned:
        tpl = turn_child_frames(tpl, rng)
    assert int(tpl["nb"]) == 1 + n_joints
    return tpl


def rollout_inputs(tpl, bs=3, T=8, seed=0, depth=0.003):
    """float32 rollout inputs for a generated FREE-root robot, the recipe of scripts/gpu_stress_robots.py: joint angles uniform in +-0.3,
    a random yaw, every env dropped so that its lowest contact candidate is ``depth`` in the ground (float64 eval_fk of the torch
    oracle), small twists, torques, residual wrenches and PD targets; frames at states 0, T // 2 and T; dt = 0.5 ms."""
    import torch

    from ground_wrench_common import candidate_probe
    from oracle import ref_torch as rt

    nb, nq, nqd = int(tpl["nb"]), int(tpl["nq"]), int(tpl["nqd"])
    rng = np.random.RandomState(seed)
    q = np.tile(np.asarray(tpl["joint_q"], np.float64), (bs, 1))
    q[:, 7:] = rng.uniform(-0.3, 0.3, (bs, nq - 7))
    yaw = rng.uniform(-0.5, 0.5, bs)
    q[:, 3:7] = np.stack([0 * yaw, np.sin(yaw / 2), 0 * yaw, np.cos(yaw / 2)], -1)
    mass = np.tile(np.asarray(tpl["body_mass"], np.float64), bs)
    inertia = np.tile(np.asarray(tpl["body_inertia"], np.float64), (bs, 1, 1))
    ke = np.tile(np.r_[np.zeros(6), np.full(nqd - 6, 30.0)], bs)
    f2s = sorted(set([0, T // 2, T]))
    F = len(f2s)
    inp = dict(q_init=q.reshape(-1), qd_init=rng.randn(bs * nqd) * 0.1, torques=rng.randn(T, bs * nqd) * 0.05, res_f=rng.randn(T, bs * nb, 6) * 0.05,
               refs=rng.uniform(-0.2, 0.2, (T, bs * nqd)), target_ke=ke, target_kd=ke * 0.01, body_mass=mass, body_inv_mass=1 / mass, body_inertia=inertia,
               body_inv_inertia=np.linalg.inv(inertia), adj_pos=rng.randn(F, bs * nb, 7) * 1e-3, adj_vel=rng.randn(F, bs * nb, 6) * 1e-3)
    inp = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in inp.items()}
    T64 = rt.Template(tpl, torch.float64)
    qi = inp["q_init"].reshape(bs, nq).copy()
    bq, bqd = rt.eval_fk(T64, torch.as_tensor(qi, dtype=torch.float64), torch.as_tensor(inp["qd_init"].reshape(bs, nqd), dtype=torch.float64))
    low = candidate_probe(tpl, bq.numpy(), bqd.numpy())[0].min(1)   # the lowest candidate of every env
    qi[:, 1] -= (low + depth).astype(np.float32)
    inp["q_init"] = np.ascontiguousarray(qi.reshape(-1))
    inp.update(frame2step=f2s, nsteps=T, dt=5e-4)
    return inp
