"""Shared by tests/test_body_accel_host.py and tests/test_gpu_body_accel.py: the torch restatement (float64, or float32 as the yardstick)
of the body-acceleration op PD_POSE_BODY_ACCEL -- J qdd + Jdot qd of the articulation on a state, every velocity-dependent term taken
from the state's own twists -- on the state sets of generalized_force_ref (its ``tree`` / ``case`` / ``CASES``), and the joint-space
chains built on it (Newton-Euler wrench, RNEA, mass matrix).  Nothing here runs product code beyond the model compiler.

Per joint i with parent pi (w_pi = v_pi = 0 and a constant frame without one), on joint_coords_ref's frames and axes, with
x_b = p_b + R(q_b) com_b, o0 = the origin of the set's body 0, d_b = x_b - o0, s = the six slots of the row:
  every joint  om_i = w_i - w_pi
  REVOLUTE  omd_i = (R_wj axis) s_0 + w_pi x om_i     ud_i = 0    o_i = p_wj    od_i = v_pi + w_pi x (p_wj - x_pi)   (0 without parent)
  COMPOUND  ah_k = R_wj R_off a_k, m_k = ah_k . om_i, rho = G^-1 m (always the Gram solve, G_02 = a_0 . a_2)
            "generalized": rhod = s_0..2     "measured": rhod = G^-1 (s_0 - sd rho_2, s_1, s_2 - sd rho_0), sd = rho_1 a_0 . (a_1 x a_2)
            omd_i = sum_k ah_k rhod_k + w_pi x om_i + rho_0 rho_1 ah_0 x ah_1 + rho_0 rho_2 ah_0 x ah_2 + rho_1 rho_2 ah_1 x ah_2
            ud_i = 0, o_i and od_i as REVOLUTE
  FREE      u_i = v_i - v_pi - w_pi x (x_i - x_pi)
            omd_i = R_wj s_0..2 + w_pi x om_i     ud_i = R_wj s_3..5 + w_pi x u_i     o_i = x_i    od_i = v_i
  FIXED     omd_i = w_pi x om_i, ud_i = 0, anchor as REVOLUTE
  e_i = ud_i - omd_i x (o_i - o0) - om_i x od_i
  alpha_b = sum omd_i,  a_b = sum e_i + alpha_b x d_b + w_b x v_b   over the joints of b and of its ancestors
Every lever is a difference about o0; nothing is accumulated about the world origin."""
import functools

import numpy as np
import torch

from body_twists_ref import DOFS, EFFORTS_OF, RATES, body_twists, slot_index, slots_of  # noqa: F401  (re-exported for the two test files)
from generalized_force_ref import CASES, case, generalized_force, tree  # noqa: F401
from joint_coords_ref import compound_axes, joint_frame, oracle_template, random_coords
from joint_wrench_ref import _jitter, template

TENSORS = ("out", "g_body_q", "g_body_qd", "g_acc")


def free_leaf_template():
    """world5 (a root FIXED to the world, four REVOLUTE bodies) with its last body, a child of body 0, hung on a FREE joint instead: the
    one robot here whose FREE joint has a parent (none of the generated robots has one; worldmix9 and world5 have no FREE joint at all)."""
    tpl = dict(template("world5"))
    assert int(tpl["nb"]) == 5 and int(np.asarray(tpl["joint_parent"]).reshape(-1)[4]) == 0
    assert int(np.asarray(tpl["joint_q_start"]).reshape(-1)[4]) == 3 and int(np.asarray(tpl["joint_qd_start"]).reshape(-1)[4]) == 3
    ty = np.array(tpl["joint_type"]).reshape(-1).copy()
    ty[4] = 4
    tpl["joint_type"], tpl["nq"], tpl["nqd"] = ty, 10, 9
    return tpl


def robot_template(name):
    return free_leaf_template() if name == "freeleaf5" else template(name)


@functools.lru_cache(maxsize=None)
def accel_case(name, S, shift=None):
    """generalized_force_ref.case (float64 FK of random coordinates jittered off the joint manifold, rounded to fp32), also for
    "freeleaf5" -> dict(tpl, nb, nqd, bq [S, nb, 7]), shared and never written"""
    if name != "freeleaf5":
        return case(name, S, shift)
    from oracle import ref_torch as rt

    tpl = free_leaf_template()
    q, qd = random_coords(tpl, S, seed=500 + S, lo=0.05, hi=1.0)
    bq, bqd = rt.eval_fk(oracle_template(tpl), torch.as_tensor(q), torch.as_tensor(qd))
    bq, _ = _jitter(np.random.RandomState(2000 + 11 * S), bq.numpy(), bqd.numpy())
    if shift is not None:
        bq[..., :3] += np.asarray(shift, np.float64)
    bq = bq.astype(np.float32)
    bq.setflags(write=False)
    return dict(tpl=tpl, nb=int(tpl["nb"]), nqd=int(tpl["nqd"]), bq=bq)


def body_accelerations(T, body_q, body_qd, acc6, rates="generalized"):
    """body_q [S, nb, 7], body_qd [S, nb, 6] (w, v of the centre of mass), acc6 [S, nb, 6] slot derivatives of the template's dtype ->
    [S, nb, 6] = (alpha, a) per body, world axes, a of the body's centre of mass."""
    from oracle import ref_torch as rt

    assert rates in RATES
    S = body_q.shape[0]
    o0 = body_q[:, 0, :3]
    _, depth = tree(T)
    zero3 = torch.zeros(S, 3, dtype=T.dtype)
    d = [(body_q[:, b, :3] - o0) + rt.q_rot(body_q[:, b, 3:], T.com[b].expand(S, 3)) for b in range(T.nb)]
    A, E = [None] * T.nb, [None] * T.nb
    for i in range(T.nb):
        ty, par = T.joint_type[i], T.joint_parent[i]
        s6 = acc6[:, i]
        _, q_wj, w_p, v_p = joint_frame(T, body_q, body_qd, i)
        w_i, v_i = body_qd[:, i, :3], body_qd[:, i, 3:]
        om = w_i - w_p
        p_pj = T.X_p[i, :3].expand(S, 3)
        if ty == rt.JOINT_FREE:
            ro, od = d[i], v_i
        elif par >= 0:
            ro = (body_q[:, par, :3] - o0) + rt.q_rot(body_q[:, par, 3:], p_pj)
            od = v_p + rt.cross(w_p, rt.q_rot(body_q[:, par, 3:], p_pj - T.com[par].expand(S, 3)))   # p_wj - x_pi
        else:
            ro, od = p_pj - o0, zero3
        omd, ud = rt.cross(w_p, om), zero3
        if ty == rt.JOINT_FREE:
            u = v_i - v_p - (rt.cross(w_p, d[i] - d[par]) if par >= 0 else zero3)
            omd = rt.q_rot(q_wj, s6[:, :3]) + omd
            ud = rt.q_rot(q_wj, s6[:, 3:]) + rt.cross(w_p, u)
        elif ty == rt.JOINT_REVOLUTE:
            omd = rt.q_rot(q_wj, T.axis[i].expand(S, 3)) * s6[:, :1] + omd
        elif ty == rt.JOINT_COMPOUND:
            q_off = T.X_c[i, 3:].expand(S, 4)
            q_pc = rt.q_mul(rt.q_mul(rt.q_mul(rt.q_conj(q_off), rt.q_conj(q_wj)), body_q[:, i, 3:]), q_off)
            axes = compound_axes(rt.quat_decompose(q_pc))
            q_w = rt.q_mul(q_wj, q_off)
            ah = [rt.q_rot(q_w, ax) for ax in axes]
            m = [rt.dot(a, om) for a in ah]
            s = rt.dot(axes[0], axes[2])
            den = 1.0 - s * s
            rho = [(m[0] - s * m[2]) / den, m[1], (m[2] - s * m[0]) / den]
            rhod = [s6[:, 0], s6[:, 1], s6[:, 2]]
            if rates == "measured":
                sd = rho[1] * rt.dot(axes[0], rt.cross(axes[1], axes[2]))
                t0, t2 = s6[:, 0] - sd * rho[2], s6[:, 2] - sd * rho[0]
                rhod = [(t0 - s * t2) / den, s6[:, 1], (t2 - s * t0) / den]
            omd = (ah[0] * rhod[0][:, None] + ah[1] * rhod[1][:, None] + ah[2] * rhod[2][:, None] + omd
                   + rt.cross(ah[0], ah[1]) * (rho[0] * rho[1])[:, None] + rt.cross(ah[0], ah[2]) * (rho[0] * rho[2])[:, None]
                   + rt.cross(ah[1], ah[2]) * (rho[1] * rho[2])[:, None])
        elif ty != rt.JOINT_FIXED:
            raise NotImplementedError("joint type %d" % ty)
        A[i], E[i] = omd, ud - rt.cross(omd, ro) - rt.cross(om, od)
    for i in sorted(range(T.nb), key=lambda b: depth[b]):   # the op's order: roots first, the body's own share plus its parent's sum
        par = T.joint_parent[i]
        if par >= 0:
            A[i], E[i] = A[i] + A[par], E[i] + E[par]
    return torch.stack([torch.cat([A[b], E[b] + rt.cross(A[b], d[b]) + rt.cross(body_qd[:, b, :3], body_qd[:, b, 3:])], -1)
                        for b in range(T.nb)], 1)


def newton_euler(body_q, body_qd, body_acc, mass, inertia, gravity):
    """(t, f) [S, nb, 6]: t = R (I R^T alpha + R^T w x I R^T w), f = m (a - gravity [m != 0]); mass [nb], inertia [nb, 3, 3], gravity [3]"""
    from oracle import ref_torch as rt

    S, nb = body_q.shape[:2]
    q = body_q[..., 3:].reshape(-1, 4)
    wb = rt.q_rot_inv(q, body_qd[..., :3].reshape(-1, 3)).reshape(S, nb, 3)
    ab = rt.q_rot_inv(q, body_acc[..., :3].reshape(-1, 3)).reshape(S, nb, 3)
    Iw, Ia = (inertia @ wb[..., None])[..., 0], (inertia @ ab[..., None])[..., 0]
    t = rt.q_rot(q, (Ia + torch.cross(wb, Iw, dim=-1)).reshape(-1, 3)).reshape(S, nb, 3)
    f = mass[:, None] * (body_acc[..., 3:] - gravity * (mass != 0).to(body_q.dtype)[:, None])
    return torch.cat([t, f], -1)


def inertia_of(tpl, dtype):
    """-> mass [nb], inertia [nb, 3, 3], gravity [3] of a template in ``dtype``"""
    nb = int(tpl["nb"])
    return (torch.tensor(np.asarray(tpl["body_mass"], np.float64).reshape(nb), dtype=dtype),
            torch.tensor(np.asarray(tpl["body_inertia"], np.float64).reshape(nb, 3, 3), dtype=dtype),
            torch.tensor(np.asarray(tpl["gravity"], np.float64).reshape(3), dtype=dtype))


def rnea(T, tpl, body_q, joint_qd, joint_qdd, rates="generalized", external=None):
    """The chain of dp_utils.rnea on the restatements: body_twists, body_accelerations, newton_euler - external, generalized_force with
    the conjugate efforts -> [S, nqd].  joint_qdd None: zeros."""
    mass, inertia, gravity = inertia_of(tpl, T.dtype)
    tw = body_twists(T, body_q, slots_of(tpl, joint_qd), rates)
    acc6 = torch.zeros_like(tw) if joint_qdd is None else slots_of(tpl, joint_qdd)
    acc = body_accelerations(T, body_q, tw, acc6, rates)
    need = newton_euler(body_q, tw, acc, mass, inertia, gravity)
    if external is not None:
        need = need - external
    return generalized_force(T, body_q, need, EFFORTS_OF[rates])


def mass_matrix(T, tpl, body_q):
    """H [S, nqd, nqd] = sum_b J_b^T diag(R I R^T, m) J_b of the generalised rates, as dp_utils.mass_matrix builds it: the columns of J
    are body_twists of the unit rates."""
    from oracle import ref_torch as rt

    mass, inertia, _ = inertia_of(tpl, T.dtype)
    S, nb, nqd = body_q.shape[0], T.nb, T.nqd
    cols = [body_twists(T, body_q, slots_of(tpl, torch.eye(nqd, dtype=T.dtype)[j].expand(S, nqd)), "generalized") for j in range(nqd)]
    J = torch.stack(cols, -1)   # [S, nb, 6, nqd]
    q = body_q[..., None, 3:].expand(S, nb, nqd, 4).reshape(-1, 4)
    Aw = rt.q_rot_inv(q, J[..., :3, :].transpose(-1, -2).reshape(-1, 3)).reshape(S, nb, nqd, 3)
    IA = Aw @ inertia.transpose(-1, -2)
    Jv = J[..., 3:, :]
    return (Aw @ IA.transpose(-1, -2)).sum(1) + (mass[None, :, None, None] * (Jv.transpose(-1, -2) @ Jv)).sum(1)


def twists_of(C, seed=67):
    """standard-normal twists [S, nb, 6] of a case, float32 (any state: the op is held to its formula, not to rigid states)"""
    return np.random.RandomState(seed).randn(C["bq"].shape[0], C["nb"], 6).astype(np.float32)


def acc_of(C, seed=71):
    """standard-normal slot derivatives [S, nb, 6] of a case, float32, every slot filled (the op must ignore the unused ones)"""
    return np.random.RandomState(seed).randn(C["bq"].shape[0], C["nb"], 6).astype(np.float32)


def g_out_of(C, seed=73):
    return np.random.RandomState(seed).randn(C["bq"].shape[0], C["nb"], 6).astype(np.float32)


def accel_of(C, dtype, rates, g_out=None):
    """The restatement on a case in ``dtype`` -> dict(out); with g_out [S, nb, 6] also autograd of <g_out, out>: g_body_q, g_body_qd,
    g_acc."""
    T = oracle_template(C["tpl"], dtype)
    need = g_out is not None
    bq = torch.tensor(np.array(C["bq"]), dtype=dtype).requires_grad_(need)
    bqd = torch.tensor(twists_of(C), dtype=dtype).requires_grad_(need)
    a6 = torch.tensor(acc_of(C), dtype=dtype).requires_grad_(need)
    out = body_accelerations(T, bq, bqd, a6, rates)
    if not need:
        return dict(out=out.numpy())
    (out * torch.as_tensor(np.asarray(g_out), dtype=dtype)).sum().backward()
    return dict(out=out.detach().numpy(), g_body_q=bq.grad.numpy(), g_body_qd=bqd.grad.numpy(), g_acc=a6.grad.numpy())


def rows19(C):
    """The op's operand rows [S * nb, 19] = (p, q xyzw, w, v, s[6]), numpy float32."""
    return np.ascontiguousarray(np.concatenate([C["bq"], twists_of(C), acc_of(C)], -1).reshape(-1, 19), dtype=np.float32)
