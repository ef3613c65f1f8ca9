"""Shared by tests/test_joint_coords_host.py and tests/test_gpu_joint_coords.py: the torch restatement (float64, or float32 as the
yardstick) of the joint-coordinates op PD_POSE_JOINT_COORDS -- the inverse of oracle/ref_torch.py eval_fk, built from that module's own
quaternion functions -- and the state sets the op is held to.  Nothing here runs product code.

For body i with parent par the joint frame is X_wj = X_parent X_p[i] (X_p[i] alone, w_p = v_p = 0 without a parent);
r_err = conj(q_wj) q_c, w_err = w_c - w_p (eval_body_joints, ref_torch.py:263-281).
  FREE      q = (R_wj^-1 (p_c - p_wj), r_err), qd = (R_wj^-1 w_err, R_wj^-1 (v_c - v_p - w_err x com))   -- eval_fk solved for its inputs
  REVOLUTE  q = the twist angle of ref_torch.py:291-298, 2 acos(twist.w) sign(axis . twist.xyz), evaluated as 2 sgn atan2(|axis| |da|, w)
            with da = r_err.xyz . axis (the same function: acos(x / sqrt(x^2 + y^2)) = atan2(y, x) for y >= 0); qd = w_err . R_wj axis
  COMPOUND  q = quat_decompose(conj(q_off) conj(q_wj) q_c q_off); measured rates m_k = (R_wj R_off a_k) . w_err on the axes of
            ref_torch.py:311-316; rates "measured": qd = m; "generalized": qd = G^-1 m, G_kj = a_k . a_j, of which only s = a_0 . a_2 is
            off the diagonal: qd_1 = m_1, qd_0 = (m_0 - s m_2) / (1 - s^2), qd_2 = (m_2 - s m_0) / (1 - s^2)
  FIXED     no coordinates"""
import os

import numpy as np
import torch

from helpers import GOLDEN

WIDTH = {1: (1, 1), 3: (0, 0), 4: (7, 6), 5: (3, 3)}   # joint type -> (coordinates, rates)


def load_tpl(name):
    """A shipped template by name, or the 17-body Laikago with four FIXED toes of tests/golden."""
    if name == "laikago_toes":
        with np.load(os.path.join(GOLDEN, "template_laikago_toes.npz")) as z:
            return {k: z[k] for k in z.files}
    from diffphys_amd import robots

    return dict(robots.load_template(name))


def oracle_template(tpl, dtype=torch.float64):
    from oracle import ref_torch

    return ref_torch.Template(tpl, dtype)


def joint_frame(T, body_q, body_qd, i):
    """-> p_wj, q_wj, w_p, v_p of body i for states [S, nb, 7], [S, nb, 6]   (ref_torch.py:263-273)"""
    from oracle import ref_torch as rt

    S = body_q.shape[0]
    p_wj, q_wj = T.X_p[i, :3].expand(S, 3), T.X_p[i, 3:].expand(S, 4)
    w_p = torch.zeros(S, 3, dtype=T.dtype)
    v_p = torch.zeros(S, 3, dtype=T.dtype)
    par = T.joint_parent[i]
    if par >= 0:
        pp, qp = body_q[:, par, :3], body_q[:, par, 3:]
        p_wj = pp + rt.q_rot(qp, p_wj)
        q_wj = rt.q_mul(qp, q_wj)
        w_p, v_p = body_qd[:, par, :3], body_qd[:, par, 3:]
    return p_wj, q_wj, w_p, v_p


def compound_axes(angles):
    """the axis chain of ref_torch.py:311-316 for angles [S, 3] -> a_0, a_1, a_2 in the joint's own frame"""
    from oracle import ref_torch as rt

    S = angles.shape[0]
    e = torch.eye(3, dtype=angles.dtype)
    axis_0 = e[0].expand(S, 3)
    q_0 = rt.q_axis_angle(axis_0, angles[:, 0])
    axis_1 = rt.q_rot(q_0, e[1].expand(S, 3))
    q_1 = rt.q_axis_angle(axis_1, angles[:, 1])
    axis_2 = rt.q_rot(rt.q_mul(q_1, q_0), e[2].expand(S, 3))
    return axis_0, axis_1, axis_2


def joint_coords(T, body_q, body_qd, rates="generalized"):
    """body_q [S, nb, 7], body_qd [S, nb, 6] (Warp order w, v) of the template's dtype -> (joint_q [S, nq], joint_qd [S, nqd])."""
    from oracle import ref_torch as rt

    assert rates in ("generalized", "measured")
    S = body_q.shape[0]
    jq, jqd = [None] * T.nq, [None] * T.nqd

    def put(dst, start, cols):
        for k in range(cols.shape[1]):
            dst[start + k] = cols[:, k]

    for i in range(T.nb):
        ty, qs, qds = T.joint_type[i], T.q_start[i], T.qd_start[i]
        if ty == rt.JOINT_FIXED:
            continue
        p_wj, q_wj, w_p, v_p = joint_frame(T, body_q, body_qd, i)
        p_c, q_c = body_q[:, i, :3], body_q[:, i, 3:]
        w_c, v_c = body_qd[:, i, :3], body_qd[:, i, 3:]
        r_err = rt.q_mul(rt.q_conj(q_wj), q_c)
        w_err = w_c - w_p
        if ty == rt.JOINT_FREE:
            put(jq, qs, torch.cat([rt.q_rot_inv(q_wj, p_c - p_wj), r_err], -1))
            lin = v_c - v_p - rt.cross(w_err, T.com[i].expand(S, 3))
            put(jqd, qds, torch.cat([rt.q_rot_inv(q_wj, w_err), rt.q_rot_inv(q_wj, lin)], -1))
        elif ty == rt.JOINT_REVOLUTE:
            axis = T.axis[i].expand(S, 3)
            da = rt.dot(r_err[:, :3], axis)
            sgn = torch.where(da < 0, -1.0, 1.0).to(T.dtype)
            alen = torch.sqrt(rt.dot(T.axis[i], T.axis[i]))
            put(jq, qs, (2.0 * sgn * torch.atan2(da.abs() * alen, r_err[:, 3]))[:, None])
            put(jqd, qds, rt.dot(w_err, rt.q_rot(q_wj, axis))[:, None])
        elif ty == rt.JOINT_COMPOUND:
            q_off = T.X_c[i, 3:].expand(S, 4)
            q_pc = rt.q_mul(rt.q_mul(rt.q_mul(rt.q_conj(q_off), rt.q_conj(q_wj)), q_c), q_off)
            angles = rt.quat_decompose(q_pc)
            axes = compound_axes(angles)
            q_w = rt.q_mul(q_wj, q_off)
            m = [rt.dot(rt.q_rot(q_w, ax), w_err) for ax in axes]
            if rates == "generalized":
                s = rt.dot(axes[0], axes[2])
                den = 1.0 - s * s
                m = [(m[0] - s * m[2]) / den, m[1], (m[2] - s * m[0]) / den]
            put(jq, qs, angles)
            put(jqd, qds, torch.stack(m, -1))
        else:
            raise NotImplementedError("joint type %d" % ty)
    assert all(c is not None for c in jq) and all(c is not None for c in jqd), "a coordinate no joint owns"
    return torch.stack(jq, -1), torch.stack(jqd, -1)


def random_coords(tpl, S, seed, lo=0.0, hi=1.0, zero_sets=0):
    """Random joint coordinates [S, nq], [S, nqd] (float64 numpy): angles uniform with lo <= |q| <= hi, FREE joints with a random
    position, a random UNIT quaternion and random rates; the first ``zero_sets`` sets sit at the reference pose (all angles exactly 0)."""
    rng = np.random.RandomState(seed)
    nb, nq, nqd = int(tpl["nb"]), int(tpl["nq"]), int(tpl["nqd"])
    q = rng.uniform(lo, hi, (S, nq)) * np.where(rng.rand(S, nq) < 0.5, -1.0, 1.0)
    qd = rng.randn(S, nqd)
    q[:zero_sets] = 0.0
    for i in range(nb):
        if int(tpl["joint_type"][i]) == 4:
            s = int(tpl["joint_q_start"][i])
            q[:, s: s + 3] = rng.uniform(-1.0, 1.0, (S, 3))
            quat = rng.randn(S, 4)
            q[:, s + 3: s + 7] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
    return q, qd


def fk_states(tpl, q, qd):
    """ref_torch.eval_fk in float64, rounded to fp32 -- the numbers every evaluation (GPU, float64, float32) is then given."""
    from oracle import ref_torch as rt

    T = oracle_template(tpl)
    bq, bqd = rt.eval_fk(T, torch.as_tensor(q, dtype=torch.float64), torch.as_tensor(qd, dtype=torch.float64))
    return bq.numpy().astype(np.float32), bqd.numpy().astype(np.float32)


def coords_of(tpl, dtype, body_q, body_qd, rates, g_q=None, g_qd=None):
    """The restatement on numpy states [S, nb, 7], [S, nb, 6] in ``dtype`` -> (joint_q, joint_qd) numpy; with g_q / g_qd also autograd of
    <g_q, joint_q> + <g_qd, joint_qd> -> (joint_q, joint_qd, g_body_q, g_body_qd)."""
    T = oracle_template(tpl, dtype)
    need = g_q is not None
    bq = torch.tensor(np.array(body_q), dtype=dtype).requires_grad_(need)
    bqd = torch.tensor(np.array(body_qd), dtype=dtype).requires_grad_(need)
    jq, jqd = joint_coords(T, bq, bqd, rates)
    if not need:
        return jq.numpy(), jqd.numpy()
    ((jq * torch.as_tensor(np.asarray(g_q), dtype=dtype)).sum() + (jqd * torch.as_tensor(np.asarray(g_qd), dtype=dtype)).sum()).backward()
    return jq.detach().numpy(), jqd.detach().numpy(), bq.grad.numpy(), bqd.grad.numpy()


def tangent(g_q, body_q):
    """The quaternion part of a pose gradient [.., 7] projected onto the tangent space of the unit sphere at body_q: g - (g . q) q."""
    g = np.array(g_q, dtype=np.float64)
    q = np.asarray(body_q, np.float64)[..., 3:]
    q = q / np.linalg.norm(q, axis=-1, keepdims=True)
    g[..., 3:] -= (g[..., 3:] * q).sum(-1, keepdims=True) * q
    return g
