"""Host side of the body-acceleration op, PD_POSE_BODY_ACCEL = 19: the argument checks of the two pose entries for the new op code, what
the float64 restatement (tests/body_accel_ref.py) rests on -- the central difference of analytic rigid twists along a joint path, the
autograd JVP of the twists for the bias term, the mass-matrix identity of the RNEA chain --, the continuous limit of inertial_wrench,
the slot gather and the wrappers' refusals.  All without a GPU.

The identities run on a float64 copy of the template with its quaternions and axes normalised in float64
(generalized_force_ref.unit_template).  FREE joints below another body: none of the generated robots has one (worldmix9 and world5
have no FREE joint at all), so body_accel_ref.free_leaf_template ("freeleaf5": world5 with its last body on a FREE joint) is added
to the finite-difference robots.

Measured here: finite difference at h = 1e-4 at most 2.6e-7 of max |out| (human, measured rates; values up to 35) on every robot and
mode (bar 1e-6), the error at h / 2 a quarter of it (ratio 3.99 .. 4.01; bar >= 3); bias term against the autograd JVP 2.0e-15 of max
(bar 1e-10); mass-matrix identity 1.4e-15 of max (bar 1e-10); newton_euler_wrench against inertial_wrench: rounding, see
test_newton_euler_wrench_is_the_limit_of_inertial_wrench."""
import ctypes

import numpy as np
import pytest
import torch

from body_accel_ref import (DOFS, RATES, body_accelerations, body_twists, mass_matrix, rnea, robot_template, slot_index, slots_of)
from generalized_force_ref import unit_template
from joint_coords_ref import compound_axes, oracle_template, random_coords
from joint_wrench_ref import template

F64 = torch.float64
FD_ROBOTS = ("laikago", "human", "cmp31", "mixed25", "worldmix9", "world5", "freeleaf5")


# ------------------------------------------------------------------------------------------------------------- (a) the C ABI
def test_pose_entries_check_the_new_op_without_a_gpu():
    from diffphys_amd import hip_backend

    lib = hip_backend.lib()
    err = lambda: lib.pd_last_error()
    assert hip_backend.POSE_BODY_ACCEL == 19
    assert lib.pd_abi_version() == 9
    assert lib.pd_pose_op(19, 0, None, 13, None, None, None) == 0    # (on the parent commit 19 is an unknown op: this fails there)
    assert lib.pd_pose_op_vjp(19, 0, None, 13, None, None, None, None, None) == 0
    assert lib.pd_pose_op(19, 0, None, 256, None, None, None) == 0
    buf = (ctypes.c_float * 64)()   # host memory: the call must be refused before anything is launched or read
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.pd_pose_op(19, 26, None, 13, None, p, None) != 0 and b"NULL operand" in err()
    assert lib.pd_pose_op_vjp(19, 26, None, 13, p, p, None, p, None) != 0 and b"NULL operand" in err()
    # a bad group size, at every n
    assert lib.pd_pose_op(19, 14, p, 13, p, p, None) != 0 and b"n % g" in err()
    assert lib.pd_pose_op_vjp(19, 14, p, 13, p, p, None, p, None) != 0 and b"n % g" in err()
    assert lib.pd_pose_op(19, 0, None, 0, None, None, None) != 0 and b"n % g" in err()
    # the cap on the bodies per state set, at every n
    assert lib.pd_pose_op(19, 0, None, 257, None, None, None) != 0 and b"at most 256" in err() and b"PD_POSE_BODY_ACCEL" in err()
    assert lib.pd_pose_op_vjp(19, 257, p, 257, p, p, None, p, None) != 0 and b"at most 256" in err()
    # the table has no gradient: a non-NULL g_a is refused, at n = 0 too
    assert lib.pd_pose_op_vjp(19, 13, p, 13, p, p, p, p, None) != 0 and b"g_a" in err() and b"PD_POSE_BODY_ACCEL" in err()
    assert lib.pd_pose_op_vjp(19, 0, None, 13, None, None, p, None, None) != 0 and b"g_a" in err()
    # the refusal order is the shared one: n % g, the cap, g_a
    assert lib.pd_pose_op_vjp(19, 14, p, 13, p, p, p, p, None) != 0 and b"n % g" in err()
    assert lib.pd_pose_op_vjp(19, 257, p, 257, p, p, p, p, None) != 0 and b"at most 256" in err()
    off = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16 + 4)
    assert lib.pd_pose_op(19, 13, off, 13, p, p, None) != 0 and b"aligned" in err() and b"joint table" in err()
    for op in (18, 20):   # the gap before the code and the code after it: unknown ops
        assert lib.pd_pose_op(op, 0, None, 13, None, None, None) != 0 and b"unknown op" in err()
        assert lib.pd_pose_op_vjp(op, 13, p, 13, p, p, None, p, None) != 0 and b"unknown op" in err()


# ------------------------------------------------------------------------------------------------------------ (b) the identities
def _unit(name):
    tpl = unit_template(robot_template(name))
    return tpl, oracle_template(tpl)


def _coords(tpl, S, seed):
    q, _ = random_coords(tpl, S, seed=seed, lo=0.05, hi=1.0)
    return torch.tensor(q, dtype=F64)


def _path(tpl, T, q0, r0, s, t, rates):
    """The joint path at time t: slot rates r0 + t s in the joint_qd layout, coordinates moved from q0 for the time t at the rates r0
    mean (REVOLUTE: q' = r; COMPOUND: q' = rho, the generalised rates of the slot rates; FREE: the joint's rotation turns at r_0..2 and
    the child's centre of mass moves at r_3..5, both in the joint frame).  First order in t: the second-order term of a twice
    differentiable path through (q0, r0, s) is even in t and drops out of the central difference.
    -> (body_q with unit quaternions, the rigid twists body_twists_ref of it)"""
    from oracle import ref_torch as rt

    S = q0.shape[0]
    q = q0.clone()
    for b in range(T.nb):
        ty, qs, qds = T.joint_type[b], T.q_start[b], T.qd_start[b]
        if ty == rt.JOINT_REVOLUTE:
            q[:, qs] = q0[:, qs] + t * r0[:, qds]
        elif ty == rt.JOINT_COMPOUND:
            rho = [r0[:, qds], r0[:, qds + 1], r0[:, qds + 2]]
            if rates == "measured":
                ax = compound_axes(q0[:, qs: qs + 3])
                g = rt.dot(ax[0], ax[2])
                rho = [(rho[0] - g * rho[2]) / (1 - g * g), rho[1], (rho[2] - g * rho[0]) / (1 - g * g)]
            q[:, qs: qs + 3] = q0[:, qs: qs + 3] + t * torch.stack(rho, -1)
        elif ty == rt.JOINT_FREE:
            com = T.com[b].expand(S, 3)
            p0, quat0 = q0[:, qs: qs + 3], q0[:, qs + 3: qs + 7]
            ang = r0[:, qds: qds + 3]
            n = ang.norm(dim=-1)
            quat = rt.q_mul(rt.q_axis_angle(ang / n[:, None], n * t), quat0)
            c = p0 + rt.q_rot(quat0, com) + t * r0[:, qds + 3: qds + 6]
            q[:, qs: qs + 3], q[:, qs + 3: qs + 7] = c - rt.q_rot(quat, com), quat
    bq, _ = rt.eval_fk(T, q, torch.zeros(S, T.nqd, dtype=F64))
    bq = torch.cat([bq[..., :3], bq[..., 3:] / bq[..., 3:].norm(dim=-1, keepdim=True)], -1)
    return bq, body_twists(T, bq, slots_of(tpl, r0 + t * s), rates)


@pytest.mark.parametrize("rates", RATES)
@pytest.mark.parametrize("name", FD_ROBOTS)
def test_out_is_the_central_difference_of_rigid_twists(name, rates):
    """On exact rigid states, out = d/dt body_twists_ref along the joint path whose slot rates change at s: central difference at
    h = 1e-4, bar 1e-6 of max |out|; and the error at h / 2 is at most a third of it -- what remains is the difference's own
    truncation error (h^2), not a missing term."""
    tpl, T = _unit(name)
    S = 3
    q0 = _coords(tpl, S, 1700 + len(name))
    rng = np.random.RandomState(31 + len(name))
    r0, s = torch.tensor(rng.randn(S, T.nqd), dtype=F64), torch.tensor(rng.randn(S, T.nqd), dtype=F64)
    bq, tw = _path(tpl, T, q0, r0, s, 0.0, rates)
    out = body_accelerations(T, bq, tw, slots_of(tpl, s), rates)
    scale = float(out.abs().max())

    def err(h):
        fd = (_path(tpl, T, q0, r0, s, h, rates)[1] - _path(tpl, T, q0, r0, s, -h, rates)[1]) / (2 * h)
        return float((out - fd).abs().max())

    e1, e2 = err(1e-4), err(5e-5)
    print("%s %s finite difference: %.2e at h = 1e-4, %.2e at h / 2 (ratio %.2f), values up to %.3g" % (name, rates, e1, e2, e1 / e2, scale))
    assert scale > 0.1 and e1 <= 1e-6 * scale
    assert e1 >= 3 * e2


@pytest.mark.parametrize("name", ["world5", "rev64", "laikago"])
def test_bias_term_is_the_jvp_of_the_twists(name):
    """s = 0, generalized mode, hinge-only robots (q' = qd; world5 is one as it stands, rev64 and laikago with their FREE root held
    still at zero rates): out = sum_j d(J qd) / dq_j qd_j, the autograd JVP of body_twists_ref o eval_fk in q along qd with the slot
    rates held.  Bar 1e-10 of max |out|."""
    from oracle import ref_torch as rt

    tpl, T = _unit(name)
    assert set(T.joint_type) <= {rt.JOINT_REVOLUTE, rt.JOINT_FIXED, rt.JOINT_FREE}
    S = 2
    q0 = _coords(tpl, S, 1800)
    qd = torch.tensor(np.random.RandomState(5).randn(S, T.nqd), dtype=F64)
    dq = torch.zeros_like(q0)   # d joint_q / dt in the coordinates' layout
    for b in range(T.nb):
        if T.joint_type[b] == rt.JOINT_FREE:
            assert T.joint_parent[b] < 0
            qd[:, T.qd_start[b]: T.qd_start[b] + 6] = 0.0
        elif T.joint_type[b] == rt.JOINT_REVOLUTE:
            dq[:, T.q_start[b]] = qd[:, T.qd_start[b]]
    r6 = slots_of(tpl, qd)

    def twists(q):
        bq, _ = rt.eval_fk(T, q, torch.zeros_like(qd))
        return body_twists(T, bq, r6, "generalized")

    tw, jvp = torch.autograd.functional.jvp(twists, q0, dq)
    bq, _ = rt.eval_fk(T, q0, torch.zeros_like(qd))
    out = body_accelerations(T, bq, tw, torch.zeros(S, T.nb, 6, dtype=F64), "generalized")
    scale = float(out.abs().max())
    e = float((out - jvp).abs().max())
    print("%s bias term against the JVP: %.2e of max %.3g" % (name, e / scale, scale))
    assert scale > 0.1 and e <= 1e-10 * scale


@pytest.mark.parametrize("name", ["laikago", "human", "mixed25"])
def test_rnea_difference_is_the_mass_matrix(name):
    """rnea_ref(qdd) - rnea_ref(0) = H qdd, H from the restatement's Jacobian as dp_utils.mass_matrix builds it.  Bar 1e-10 of max."""
    tpl, T = _unit(name)
    S = 2
    q0 = _coords(tpl, S, 1900)
    rng = np.random.RandomState(9)
    qd, qdd = torch.tensor(rng.randn(S, T.nqd), dtype=F64), torch.tensor(rng.randn(S, T.nqd), dtype=F64)
    bq, _ = _path(tpl, T, q0, qd, qdd, 0.0, "generalized")
    lhs = rnea(T, tpl, bq, qd, qdd) - rnea(T, tpl, bq, qd, None)
    rhs = (mass_matrix(T, tpl, bq) @ qdd[..., None])[..., 0]
    scale = float(rhs.abs().max())
    e = float((lhs - rhs).abs().max())
    print("%s rnea(qdd) - rnea(0) against H qdd: %.2e of max %.3g" % (name, e / scale, scale))
    assert scale > 0 and e <= 1e-10 * scale


# ------------------------------------------------------------------------------------------------------------ (c) the binding
class _Env:
    def __init__(self, tpl):
        self.nb, self._tpl, self._contact_table = int(tpl["nb"]), tpl, None

    def template(self):
        return self._tpl


def test_newton_euler_wrench_is_the_limit_of_inertial_wrench():
    """dp_utils.newton_euler_wrench against dp_utils.inertial_wrench on (w, v) -> ((w + alpha dt) (1 - 0.1 dt), v + a dt), float64.
    inertial_wrench divides the next angular velocity by (1 - 0.1 dt) before it differences, so on that pair of twists it returns
    R (I R^T alpha + R^T w x I R^T w) and m (a - gravity) themselves: the two functions agree to ROUNDING at every dt, torque and force
    alike -- not merely to first order in dt.  A difference that is rounding noise does not halve with dt (it grows like eps / dt), so
    the convergence is asserted as what it is: both differences below 1e-10 of max at dt and at dt / 2 (measured 9e-14 and 2e-13 of max
    for the torque, 5e-15 and 2e-14 for the force), which bounds the dt / 2 difference far below 0.6 x any first-order term.  WITHOUT the
    factor on the next angular velocity the torques differ by 0.1 I w at every dt: that is asserted too, so the damping is seen."""
    from diffphys_amd import dp_utils

    tpl = template("laikago")
    env = _Env(tpl)
    nb = env.nb
    rng = np.random.RandomState(13)
    quat = rng.randn(2, nb, 4)
    bq = torch.tensor(np.concatenate([rng.randn(2, nb, 3), quat / np.linalg.norm(quat, axis=-1, keepdims=True)], -1), dtype=F64)
    bqd, acc = torch.tensor(rng.randn(2, nb, 6), dtype=F64), torch.tensor(rng.randn(2, nb, 6), dtype=F64)
    m = torch.tensor(np.asarray(tpl["body_mass"], np.float64).reshape(nb))
    I = torch.tensor(np.asarray(tpl["body_inertia"], np.float64).reshape(nb, 3, 3))
    ne = dp_utils.newton_euler_wrench(bq, bqd, acc, m, I, env)
    assert ne.shape == (2, nb, 6)

    def diff(dt, damped=True):
        w1 = (bqd[..., :3] + acc[..., :3] * dt) * ((1.0 - 0.1 * dt) if damped else 1.0)
        iw = dp_utils.inertial_wrench(bq, bqd, torch.cat([w1, bqd[..., 3:] + acc[..., 3:] * dt], -1), dt, m, I, env)
        return float((iw - ne)[..., :3].abs().max() / ne[..., :3].abs().max()), float((iw - ne)[..., 3:].abs().max() / ne[..., 3:].abs().max())

    dt = 1e-3
    (t1, f1), (t2, f2) = diff(dt), diff(dt / 2)
    print("newton_euler_wrench against inertial_wrench: torque %.1e / %.1e of max at dt / dt/2, force %.1e / %.1e" % (t1, t2, f1, f2))
    assert max(t1, t2, f1, f2) <= 1e-10
    t_raw, f_raw = diff(dt, damped=False)
    assert t_raw > 1e-3 and f_raw <= 1e-10   # the undamped pair: a zeroth-order torque difference, 0.1 I w


def test_slot_gather_and_wrapper_refusals_without_a_gpu():
    from diffphys_amd import dp_model, dp_utils, hip_backend

    tpl = template("laikago")
    nb, nqd = int(tpl["nb"]), int(tpl["nqd"])
    env = _Env(tpl)
    # the gather: slot k of body b <- dof qd_start[b] + k, zero elsewhere, broadcast over the leading shape
    qdd = torch.arange(1.0, nqd + 1.0)
    got = dp_utils._rate_slots(qdd, (2, 3), _Env(tpl), "cpu")
    idx = slot_index(tpl)
    want = np.concatenate([qdd.numpy(), [0.0]])[idx]
    assert got.shape == (2, 3, nb, 6) and np.array_equal(got[1, 2].numpy(), want) and (got[0, 0] == got[1, 2]).all()
    assert all((idx[b] < nqd).sum() == DOFS[int(np.asarray(tpl["joint_type"]).reshape(-1)[b])] for b in range(nb))
    table = hip_backend.joint_table(tpl, "measured", device="cpu")
    rows = torch.zeros(2 * nb, 19)
    with pytest.raises(ValueError, match="joint_table"):   # a bare tensor carries no dimensions
        hip_backend.body_accelerations(torch.zeros(table.numel()), nb, rows)
    with pytest.raises(ValueError, match="a jointforce table"):
        hip_backend.body_accelerations(hip_backend.joint_force_table(tpl, device="cpu"), nb, rows)
    with pytest.raises(ValueError, match=r"\(p, q xyzw, w, v, s\[6\]\)"):
        hip_backend.body_accelerations(table, nb, torch.zeros(2 * nb, 13))
    with pytest.raises(ValueError, match="multiple"):
        hip_backend.body_accelerations(table, nb, rows[:5])
    with pytest.raises(ValueError, match="nb"):
        hip_backend.body_accelerations_vjp(table, nb + 1, torch.zeros(2 * (nb + 1), 19), torch.zeros(2 * (nb + 1), 6))
    with pytest.raises(ValueError, match="GPU"):    # no CPU fallback: refused before any launch
        hip_backend.body_accelerations(table, nb, rows)
    with pytest.raises(ValueError, match="GPU"):
        hip_backend.body_accelerations_vjp(table, nb, rows, torch.zeros(2 * nb, 6))
    bq, bqd, qd = torch.zeros(2, 3, nb, 7), torch.zeros(2, 3, nb, 6), torch.zeros(2, 3, nqd)
    m, I = torch.ones(nb), torch.eye(3).expand(nb, 3, 3)
    with pytest.raises(TypeError, match="GPU"):
        dp_model.BodyAccelerations.apply(bq, bqd, torch.zeros(2, 3, nb, 6), env, "generalized")
    with pytest.raises(TypeError, match="GPU"):
        dp_utils.body_accelerations(bq, bqd, qd, env)
    with pytest.raises(TypeError, match="GPU"):
        dp_utils.body_accelerations(bq, bqd, None, env)
    with pytest.raises(TypeError, match="GPU"):   # the chains end in the ops: HIP only
        dp_utils.rnea(bq, qd, qd, m, I, env)
    with pytest.raises(TypeError, match="GPU"):
        dp_utils.bias_forces(bq, qd, m, I, env)
    with pytest.raises(TypeError, match="GPU"):
        dp_utils.forward_dynamics(bq, qd, qd, m, I, env)
    with pytest.raises(ValueError, match="rates"):   # a rate convention that is none, before anything else
        dp_utils.rnea(bq, qd, qd, m, I, env, rates="actuator")
    with pytest.raises(ValueError, match="body_q"):   # newton_euler_wrench is plain torch: it runs here, and checks its shapes
        dp_utils.newton_euler_wrench(bq[..., :6], bqd, bqd, m, I, env)
    assert env._contact_table is None   # nothing was built for a refused call
    if torch.cuda.is_available():   # the shape and mode checks sit behind the device check
        with pytest.raises(ValueError, match="body_q"):
            dp_utils.body_accelerations(bq.cuda()[..., :6], bqd.cuda(), qd.cuda(), env)
        with pytest.raises(ValueError, match="joint_qdd"):
            dp_utils.body_accelerations(bq.cuda(), bqd.cuda(), qd.cuda()[..., :5], env)
        with pytest.raises(ValueError, match="rates"):
            dp_utils.body_accelerations(bq.cuda(), bqd.cuda(), qd.cuda(), env, rates="actuator")
