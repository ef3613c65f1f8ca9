"""Shared by tests/test_generalized_force_host.py and tests/test_gpu_generalized_force.py: the torch restatement (float64, or float32 as
the yardstick) of the generalised-force op PD_POSE_GENERALIZED_FORCE -- the transpose of the articulation's Jacobian applied to per-body
wrenches, built from oracle/ref_torch.py's quaternion functions and joint_coords_ref's joint_frame / compound_axes -- and the state sets
the op is held to.  Nothing here runs product code beyond the model compiler (generated_robots).

With x_b = p_b + R(q_b) com_b, F_i = sum_{b in subtree(i)} f_b and N_i(o) = sum_{b in subtree(i)} (t_b + (x_b - o) x f_b):
  REVOLUTE  tau = (R_wj axis) . N_i(p_wj)
  COMPOUND  g_k = (R_wj R_off a_k) . N_i(p_wj) on the angles and axes of joint_coords_ref; efforts "generalized": tau = g;
            "actuator": tau = G^-1 g, G_kj = a_k . a_j (only s = a_0 . a_2 off the diagonal)
  FREE      (R_wj^-1 N_i(x_i), R_wj^-1 F_i)
  FIXED     nothing
The moments are accumulated about o0 = the origin of the set's body 0 and moved to each anchor afterwards, every lever arm formed from
differences of positions: in float64 the definition above to rounding, in float32 free of the set's distance from the world origin --
the form the fp32 yardstick needs (about the world origin it would carry 300 m x 1e-7 of lever error into every moment)."""
import functools

import numpy as np
import torch

from joint_coords_ref import compound_axes, joint_frame, oracle_template, random_coords
from joint_wrench_ref import _jitter, template

EFFORTS = ("actuator", "generalized")
TENSORS = ("out", "g_body_q", "g_body_f")
# (robot, state sets, shift) of every GPU case.  laikago 41: 19 sets per workgroup, the last workgroup partial; human: compound joints;
# laikago_toes: FIXED joints; mixed25 11: every joint type, a body with 8 children, turned frames, two workgroups; cmp31: q_off
# everywhere; rev64: a chain of depth 64 (the level sweep); worldmix9 / world5: no FREE joint; rev256: the cap; free1: one FREE body;
# the last: every position moved by (300, 0, -200) m -- the moment reference point.
FAR = (300.0, 0.0, -200.0)
CASES = [("laikago", 1, None), ("laikago", 41, None), ("human", 3, None), ("laikago_toes", 2, None), ("mixed25", 11, None),
         ("cmp31", 3, None), ("rev64", 5, None), ("worldmix9", 4, None), ("world5", 3, None), ("rev256", 1, None), ("rev256", 2, None),
         ("free1", 3, None), ("laikago", 3, FAR)]


def tree(T):
    """-> (children in index order per body, depth per body)"""
    kids = [[c for c in range(T.nb) if T.joint_parent[c] == i] for i in range(T.nb)]
    depth = [0] * T.nb
    for i in range(T.nb):   # parents come before their children in every template here; asserted
        par = T.joint_parent[i]
        assert par < i
        depth[i] = 0 if par < 0 else depth[par] + 1
    return kids, depth


def subtree_sums(T, body_q, body_f):
    """-> F [nb] x [S, 3], M [nb] x [S, 3] (the moment about o0), d [nb] x [S, 3] = x_b - o0, o0 [S, 3]; the op's summation order: levels
    deepest first, own share first, then the children in index order."""
    from oracle import ref_torch as rt

    S = body_q.shape[0]
    o0 = body_q[:, 0, :3]
    kids, depth = tree(T)
    d = [(body_q[:, b, :3] - o0) + rt.q_rot(body_q[:, b, 3:], T.com[b].expand(S, 3)) for b in range(T.nb)]
    F = [body_f[:, b, 3:] for b in range(T.nb)]
    M = [body_f[:, b, :3] + rt.cross(d[b], F[b]) for b in range(T.nb)]
    for i in sorted(range(T.nb), key=lambda b: -depth[b]):
        for c in kids[i]:
            F[i] = F[i] + F[c]
            M[i] = M[i] + M[c]
    return F, M, d, o0


def generalized_force(T, body_q, body_f, efforts="actuator"):
    """body_q [S, nb, 7] poses, body_f [S, nb, 6] wrenches (torque, force; world axes, the force at the body's centre of mass) of the
    template's dtype -> [S, nqd] in the joint_qd layout."""
    from oracle import ref_torch as rt

    assert efforts in EFFORTS
    S = body_q.shape[0]
    F, M, d, o0 = subtree_sums(T, body_q, body_f)
    zero_qd = torch.zeros(S, T.nb, 6, dtype=T.dtype)
    out = [None] * T.nqd
    for i in range(T.nb):
        ty, qds, par = T.joint_type[i], T.qd_start[i], T.joint_parent[i]
        if ty == rt.JOINT_FIXED:
            continue
        _, q_wj, _, _ = joint_frame(T, body_q, zero_qd, i)
        p_pj = T.X_p[i, :3].expand(S, 3)
        if ty == rt.JOINT_FREE:
            r = d[i]
        elif par >= 0:
            r = (body_q[:, par, :3] - o0) + rt.q_rot(body_q[:, par, 3:], p_pj)
        else:
            r = p_pj - o0
        N = M[i] - rt.cross(r, F[i])
        if ty == rt.JOINT_FREE:
            cols = torch.cat([rt.q_rot_inv(q_wj, N), rt.q_rot_inv(q_wj, F[i])], -1)
        elif ty == rt.JOINT_REVOLUTE:
            cols = rt.dot(rt.q_rot(q_wj, T.axis[i].expand(S, 3)), N)[:, None]
        elif ty == rt.JOINT_COMPOUND:
            q_off = T.X_c[i, 3:].expand(S, 4)
            q_pc = rt.q_mul(rt.q_mul(rt.q_mul(rt.q_conj(q_off), rt.q_conj(q_wj)), body_q[:, i, 3:]), q_off)
            axes = compound_axes(rt.quat_decompose(q_pc))
            q_w = rt.q_mul(q_wj, q_off)
            g = [rt.dot(rt.q_rot(q_w, ax), N) for ax in axes]
            if efforts == "actuator":
                s = rt.dot(axes[0], axes[2])
                den = 1.0 - s * s
                g = [(g[0] - s * g[2]) / den, g[1], (g[2] - s * g[0]) / den]
            cols = torch.stack(g, -1)
        else:
            raise NotImplementedError("joint type %d" % ty)
        for k in range(cols.shape[1]):
            out[qds + k] = cols[:, k]
    assert all(c is not None for c in out), "a dof no joint owns"
    return torch.stack(out, -1) if out else torch.zeros(S, 0, dtype=T.dtype)


def unit_template(tpl):
    """A float64 copy of the template with the quaternions of joint_X_p / joint_X_c and the joint axes normalised in float64 (the shipped
    constants are fp32-rounded: 1e-7 off the sphere, which the identities of the host tests would see as 1e-5)."""
    out = dict(tpl)
    nb = int(tpl["nb"])
    for k in ("joint_X_p", "joint_X_c"):
        X = np.asarray(tpl[k], np.float64).reshape(nb, 7).copy()
        X[:, 3:] /= np.linalg.norm(X[:, 3:], axis=-1, keepdims=True)
        out[k] = X
    ax = np.asarray(tpl["joint_axis"], np.float64).reshape(nb, 3).copy()
    n = np.linalg.norm(ax, axis=-1, keepdims=True)
    out["joint_axis"] = np.where(n > 0, ax / np.where(n > 0, n, 1.0), ax)
    out["body_com"] = np.asarray(tpl["body_com"], np.float64)
    return out


@functools.lru_cache(maxsize=None)
def case(name, S, shift=None, exact=False):
    """dict(tpl, nb, nqd, bq [S, nb, 7], bf [S, nb, 6]) float32, shared and never written: float64 FK of random coordinates (angles
    0.05 <= |q| <= 1, the root within +-1 m) jittered off the joint manifold as joint_wrench_ref._jitter does (exact: not jittered), every
    position moved by ``shift``, then rounded to fp32; standard-normal wrenches."""
    from oracle import ref_torch as rt

    tpl = template(name)
    nb, nqd = int(tpl["nb"]), int(tpl["nqd"])
    rng = np.random.RandomState(2000 + 11 * S + len(name))
    q, qd = random_coords(tpl, S, seed=500 + S, lo=0.05, hi=1.0)
    bq, bqd = rt.eval_fk(oracle_template(tpl), torch.as_tensor(q), torch.as_tensor(qd))
    bq, bqd = bq.numpy(), bqd.numpy()
    if not exact:
        bq, bqd = _jitter(rng, bq, bqd)
    if shift is not None:
        bq = bq.copy()
        bq[..., :3] += np.asarray(shift, np.float64)
    C = dict(tpl=tpl, nb=nb, nqd=nqd, bq=bq.astype(np.float32), bf=rng.randn(S, nb, 6).astype(np.float32))
    for v in C.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return C


def g_out_of(C, seed=37):
    return np.random.RandomState(seed).randn(C["bq"].shape[0], C["nqd"]).astype(np.float32)


def force_of(C, dtype, efforts, g_out=None):
    """The restatement on a case in ``dtype`` -> dict(out); with g_out [S, nqd] also autograd of <g_out, out>: g_body_q, g_body_f."""
    T = oracle_template(C["tpl"], dtype)
    need = g_out is not None
    bq = torch.tensor(np.array(C["bq"]), dtype=dtype).requires_grad_(need)
    bf = torch.tensor(np.array(C["bf"]), dtype=dtype).requires_grad_(need)
    out = generalized_force(T, bq, bf, efforts)
    if not need:
        return dict(out=out.numpy())
    (out * torch.as_tensor(np.asarray(g_out), dtype=dtype)).sum().backward()
    return dict(out=out.detach().numpy(), g_body_q=bq.grad.numpy(), g_body_f=bf.grad.numpy())


def rows13(C):
    """The op's operand rows [S * nb, 13] = (p, q xyzw, t, f), numpy float32."""
    return np.ascontiguousarray(np.concatenate([C["bq"], C["bf"]], -1).reshape(-1, 13), dtype=np.float32)
