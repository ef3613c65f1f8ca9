"""Shared by tests/test_body_twists_host.py and tests/test_gpu_body_twists.py: the torch restatement (float64, or float32 as the
yardstick) of the body-twist op PD_POSE_BODY_TWIST -- the articulation's Jacobian applied to joint rates, the exact transpose of
generalized_force_ref.generalized_force in each mode -- on the state sets of generalized_force_ref (its ``tree`` / ``case`` / ``CASES``).
Nothing here runs product code beyond the model compiler.

Per joint i, on joint_coords_ref's frames and axes, with x_b = p_b + R(q_b) com_b:
  REVOLUTE  w_i = (R_wj axis) r_0                  u_i = 0             o_i = p_wj
  COMPOUND  w_i = sum_k (R_wj R_off a_k) rho_k     u_i = 0             o_i = p_wj;  "generalized": rho = r; "measured": rho = G^-1 r,
            G_kj = a_k . a_j (only s = a_0 . a_2 off the diagonal)
  FREE      w_i = R_wj r_0..2                      u_i = R_wj r_3..5   o_i = x_i
  FIXED     nothing
  w_b = sum w_i,  v_b = sum (u_i + w_i x (x_b - o_i)) over the joints of b and of its ancestors
Every lever is formed from differences about o0 = the origin of the set's body 0: c_i = u_i - w_i x (o_i - o0) is summed down the
tree with w_i (roots first, the parent's sum plus the body's own share) and v_b = C_b + W_b x (x_b - o0) -- in float64 the definition
to rounding, in float32 free of the set's distance from the world origin."""
import numpy as np
import torch

from generalized_force_ref import CASES, case, tree  # noqa: F401  (CASES / case: re-exported for the two test files)
from joint_coords_ref import compound_axes, joint_frame, oracle_template

RATES = ("measured", "generalized")
EFFORTS_OF = {"measured": "actuator", "generalized": "generalized"}   # the conjugate effort convention of generalized_force
TENSORS = ("out", "g_body_q", "g_rates")
DOFS = {1: 1, 3: 0, 4: 6, 5: 3}   # joint type -> rate slots in use: REVOLUTE, FIXED, FREE, COMPOUND


def slot_index(tpl):
    """[nb, 6] int64: dof qd_start[b] + k behind slot k of body b, nqd (an appended zero column) for a slot no dof uses -- written out
    here, independently of hip_backend.joint_rate_slot_index."""
    nb, nqd = int(tpl["nb"]), int(tpl["nqd"])
    idx = np.full((nb, 6), nqd, np.int64)
    for b in range(nb):
        for k in range(DOFS[int(tpl["joint_type"][b])]):
            idx[b, k] = int(tpl["joint_qd_start"][b]) + k
    return idx


def slots_of(tpl, joint_qd):
    """joint_qd [S, nqd] (torch) -> rate slots [S, nb, 6], zero where no dof is"""
    idx = torch.as_tensor(slot_index(tpl).reshape(-1))
    padded = torch.cat([joint_qd, joint_qd.new_zeros(joint_qd.shape[0], 1)], -1)
    return padded.index_select(-1, idx).reshape(joint_qd.shape[0], int(tpl["nb"]), 6)


def body_twists(T, body_q, rates6, rates="generalized"):
    """body_q [S, nb, 7] poses, rates6 [S, nb, 6] rate slots of the template's dtype -> [S, nb, 6] = (w, v) per body, world axes, v of
    the body's centre of mass."""
    from oracle import ref_torch as rt

    assert rates in RATES
    S = body_q.shape[0]
    o0 = body_q[:, 0, :3]
    kids, depth = tree(T)
    zero_qd = torch.zeros(S, T.nb, 6, dtype=T.dtype)
    zero3 = torch.zeros(S, 3, dtype=T.dtype)
    d = [(body_q[:, b, :3] - o0) + rt.q_rot(body_q[:, b, 3:], T.com[b].expand(S, 3)) for b in range(T.nb)]
    W, C = [None] * T.nb, [None] * T.nb
    for i in range(T.nb):
        ty, par = T.joint_type[i], T.joint_parent[i]
        r6 = rates6[:, i]
        _, q_wj, _, _ = joint_frame(T, body_q, zero_qd, i)
        p_pj = T.X_p[i, :3].expand(S, 3)
        if ty == rt.JOINT_FREE:
            anchor = d[i]
        elif par >= 0:
            anchor = (body_q[:, par, :3] - o0) + rt.q_rot(body_q[:, par, 3:], p_pj)
        else:
            anchor = p_pj - o0
        w, u = zero3, zero3
        if ty == rt.JOINT_FREE:
            w, u = rt.q_rot(q_wj, r6[:, :3]), rt.q_rot(q_wj, r6[:, 3:])
        elif ty == rt.JOINT_REVOLUTE:
            w = rt.q_rot(q_wj, T.axis[i].expand(S, 3)) * r6[:, :1]
        elif ty == rt.JOINT_COMPOUND:
            q_off = T.X_c[i, 3:].expand(S, 4)
            q_pc = rt.q_mul(rt.q_mul(rt.q_mul(rt.q_conj(q_off), rt.q_conj(q_wj)), body_q[:, i, 3:]), q_off)
            axes = compound_axes(rt.quat_decompose(q_pc))
            rho = [r6[:, 0], r6[:, 1], r6[:, 2]]
            if rates == "measured":
                s = rt.dot(axes[0], axes[2])
                den = 1.0 - s * s
                rho = [(rho[0] - s * rho[2]) / den, rho[1], (rho[2] - s * rho[0]) / den]
            e = axes[0] * rho[0][:, None] + axes[1] * rho[1][:, None] + axes[2] * rho[2][:, None]
            w = rt.q_rot(rt.q_mul(q_wj, q_off), e)
        elif ty != rt.JOINT_FIXED:
            raise NotImplementedError("joint type %d" % ty)
        W[i], C[i] = w, u - rt.cross(w, anchor)
    for i in sorted(range(T.nb), key=lambda b: depth[b]):   # the op's order: roots first, the body's own share plus its parent's sum
        par = T.joint_parent[i]
        if par >= 0:
            W[i], C[i] = W[i] + W[par], C[i] + C[par]
    return torch.stack([torch.cat([W[b], C[b] + rt.cross(W[b], d[b])], -1) for b in range(T.nb)], 1)


def rates_of(C, seed=53):
    """standard-normal rate slots [S, nb, 6] of a case, float32, every slot filled (the op must ignore the unused ones)"""
    return np.random.RandomState(seed).randn(C["bq"].shape[0], C["nb"], 6).astype(np.float32)


def g_out_of(C, seed=59):
    return np.random.RandomState(seed).randn(C["bq"].shape[0], C["nb"], 6).astype(np.float32)


def twists_of(C, dtype, rates, g_out=None):
    """The restatement on a case in ``dtype`` -> dict(out); with g_out [S, nb, 6] also autograd of <g_out, out>: g_body_q, g_rates."""
    T = oracle_template(C["tpl"], dtype)
    need = g_out is not None
    bq = torch.tensor(np.array(C["bq"]), dtype=dtype).requires_grad_(need)
    r6 = torch.tensor(rates_of(C), dtype=dtype).requires_grad_(need)
    out = body_twists(T, bq, r6, rates)
    if not need:
        return dict(out=out.numpy())
    (out * torch.as_tensor(np.asarray(g_out), dtype=dtype)).sum().backward()
    return dict(out=out.detach().numpy(), g_body_q=bq.grad.numpy(), g_rates=r6.grad.numpy())


def rows13(C):
    """The op's operand rows [S * nb, 13] = (p, q xyzw, r[6]), numpy float32."""
    return np.ascontiguousarray(np.concatenate([C["bq"], rates_of(C)], -1).reshape(-1, 13), dtype=np.float32)
