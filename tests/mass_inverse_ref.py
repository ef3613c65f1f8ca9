"""Shared by tests/test_mass_inverse_host.py and tests/test_gpu_mass_inverse.py: the torch restatement (float64 as the reference, float32
as the yardstick) of the mass-matrix-inverse op PD_POSE_MASS_INVERSE -- H^-1 applied to a joint-space vector by the articulated-body
recursion, H = sum_b J_b^T diag(R_b I_b R_b^T, m_b) J_b with J the Jacobian of body_twists_ref in either rate mode -- on the state sets
of body_accel_ref (``accel_case`` / ``CASES`` / ``freeleaf5``), the dense H it is held to, and the composed gradient formula.  Nothing
here runs product code beyond the model compiler.

Everything in world axes about o0 = the origin of the set's body 0, spatial vectors (angular, linear at o0), so children's quantities
add without a transform.  Per body b with d = x_b - o0, Ibar = R sym(I) R^T:
  spatial inertia   [[Ibar - m [d]x[d]x, m [d]x], [-m [d]x, m 1]]
  motion subspace   REVOLUTE (ah, -ah x r_i);  COMPOUND three such columns from Ah ("generalized") or Ah G^-1 ("measured");
                    FREE (R_wj e_k, -R_wj e_k x d_b) and (0, R_wj e_k);  FIXED none   (r_i = the joint's anchor - o0)
Up, deepest level first:  IA = I_b + sum Ia_c, pA = sum pa_c (children in index order), U = IA S, D = S^T U = L diag(dd) L^T,
  W = L^-1 U^T, z = L^-1 (r_b - S^T pA);  Ia = IA - W^T dd^-1 W (exactly 0 behind a 6-dof joint), pa = pA + W^T dd^-1 z;
  a body without a dof hands IA, pA up unchanged.
Down, from the roots:  x_b = L^-T dd^-1 (z - W a_pi),  a_b = a_pi + S x_b.
D is never inverted: the LDL^T factor is applied by substitution."""
import numpy as np
import torch

from body_accel_ref import CASES, accel_case, inertia_of, robot_template  # noqa: F401  (re-exported for the two test files)
from body_twists_ref import DOFS, RATES, body_twists, slot_index, slots_of  # noqa: F401
from generalized_force_ref import tree
from joint_coords_ref import compound_axes, joint_frame, oracle_template

ALL_CASES = CASES + [("freeleaf5", 4, None)]   # + the one robot whose FREE joint has a parent
TENSORS = ("out", "g_body_q", "g_r", "g_mass", "g_inertia")


def _skew(v):
    z = torch.zeros_like(v[:, 0])
    return torch.stack([torch.stack([z, -v[:, 2], v[:, 1]], -1), torch.stack([v[:, 2], z, -v[:, 0]], -1),
                        torch.stack([-v[:, 1], v[:, 0], z], -1)], -2)


def _rotm(q):
    """[S, 4] -> [S, 3, 3], the linear map of ref_torch.q_rot for ANY quaternion (columns = the rotated unit vectors)"""
    from oracle import ref_torch as rt

    e = torch.eye(3, dtype=q.dtype)
    return torch.stack([rt.q_rot(q, e[k].expand(q.shape[0], 3)) for k in range(3)], -1)


def spatial_inertia(body_q, b, d, mass, inertia):
    """[S, 6, 6] of body b about o0; mass [S, nb], inertia [S, nb, 3, 3] (its symmetric part enters)"""
    S = body_q.shape[0]
    R = _rotm(body_q[:, b, 3:])
    Is = 0.5 * (inertia[:, b] + inertia[:, b].transpose(-1, -2))
    Ibar = R @ Is @ R.transpose(-1, -2)
    m = mass[:, b, None, None]
    dx = _skew(d)
    eye = torch.eye(3, dtype=body_q.dtype).expand(S, 3, 3)
    top = torch.cat([Ibar - m * (dx @ dx), m * dx], -1)
    bot = torch.cat([-m * dx, m * eye], -1)
    return torch.cat([top, bot], -2)


def motion_subspace(T, body_q, i, d, o0, rates):
    """-> the columns of S_i, each [S, 6] = (angular, linear at o0); FIXED: none"""
    from oracle import ref_torch as rt

    S = body_q.shape[0]
    ty, par = T.joint_type[i], T.joint_parent[i]
    zero_qd = torch.zeros(S, T.nb, 6, dtype=T.dtype)
    _, q_wj, _, _ = joint_frame(T, body_q, zero_qd, i)
    p_pj = T.X_p[i, :3].expand(S, 3)
    if ty == rt.JOINT_FREE:
        anchor = d[i]
    elif par >= 0:
        anchor = (body_q[:, par, :3] - o0) + rt.q_rot(body_q[:, par, 3:], p_pj)
    else:
        anchor = p_pj - o0
    ang = lambda a: torch.cat([a, -rt.cross(a, anchor)], -1)
    if ty == rt.JOINT_FIXED:
        return []
    if ty == rt.JOINT_REVOLUTE:
        return [ang(rt.q_rot(q_wj, T.axis[i].expand(S, 3)))]
    e = torch.eye(3, dtype=T.dtype)
    if ty == rt.JOINT_FREE:
        E = [rt.q_rot(q_wj, e[k].expand(S, 3)) for k in range(3)]
        return [ang(a) for a in E] + [torch.cat([torch.zeros_like(a), a], -1) for a in E]
    if ty == rt.JOINT_COMPOUND:
        q_off = T.X_c[i, 3:].expand(S, 4)
        q_pc = rt.q_mul(rt.q_mul(rt.q_mul(rt.q_conj(q_off), rt.q_conj(q_wj)), body_q[:, i, 3:]), q_off)
        axes = list(compound_axes(rt.quat_decompose(q_pc)))
        if rates == "measured":   # the columns of A G^-1
            s = rt.dot(axes[0], axes[2])[:, None]
            den = 1.0 - s * s
            axes = [(axes[0] - axes[2] * s) / den, axes[1], (axes[2] - axes[0] * s) / den]
        q_w = rt.q_mul(q_wj, q_off)
        return [ang(rt.q_rot(q_w, a)) for a in axes]
    raise NotImplementedError("joint type %d" % ty)


def _ldl(D, K):
    """D[a][b] ([S] tensors, b <= a used) -> L[a][b] (b < a), dd[a]:  D = L diag(dd) L^T"""
    L = [[None] * K for _ in range(K)]
    dd = [None] * K
    for j in range(K):
        t = D[j][j]
        for p in range(j):
            t = t - L[j][p] * L[j][p] * dd[p]
        dd[j] = t
        for i in range(j + 1, K):
            t = D[i][j]
            for p in range(j):
                t = t - L[i][p] * L[j][p] * dd[p]
            L[i][j] = t / dd[j]
    return L, dd


def mass_inverse(T, body_q, mass, inertia, r6, rates="generalized"):
    """body_q [S, nb, 7], mass [S, nb], inertia [S, nb, 3, 3], r6 [S, nb, 6] joint-space force slots of the template's dtype ->
    [S, nb, 6]: H^-1 r in the same slots, 0 in a slot no dof uses."""
    assert rates in RATES
    from oracle import ref_torch as rt

    S = body_q.shape[0]
    o0 = body_q[:, 0, :3]
    kids, depth = tree(T)
    d = [(body_q[:, b, :3] - o0) + rt.q_rot(body_q[:, b, 3:], T.com[b].expand(S, 3)) for b in range(T.nb)]
    Ia, pa, keep = [None] * T.nb, [None] * T.nb, [None] * T.nb
    for b in sorted(range(T.nb), key=lambda i: -depth[i]):
        IA = spatial_inertia(body_q, b, d[b], mass, inertia)
        pA = torch.zeros(S, 6, dtype=T.dtype)
        for c in kids[b]:
            IA, pA = IA + Ia[c], pA + pa[c]
        cols = motion_subspace(T, body_q, b, d, o0, rates)
        K = len(cols)
        assert K == DOFS[T.joint_type[b]]
        if K == 0:
            Ia[b], pa[b], keep[b] = IA, pA, None
            continue
        U = [(IA @ s[..., None])[..., 0] for s in cols]
        D = [[(cols[a] * U[c]).sum(-1) for c in range(K)] for a in range(K)]
        u = [r6[:, b, k] - (cols[k] * pA).sum(-1) for k in range(K)]
        L, dd = _ldl(D, K)
        W, z = [None] * K, [None] * K
        for k in range(K):
            W[k], z[k] = U[k], u[k]
            for p in range(k):
                W[k], z[k] = W[k] - L[k][p][:, None] * W[p], z[k] - L[k][p] * z[p]
        Ia[b], pa[b] = IA, pA
        for k in range(K):
            Ia[b] = Ia[b] - (W[k][:, :, None] * W[k][:, None, :]) / dd[k][:, None, None]
            pa[b] = pa[b] + W[k] * (z[k] / dd[k])[:, None]
        if K == 6:   # nothing passes a 6-dof joint: exactly zero, not the rounding residue
            Ia[b] = torch.zeros_like(IA)
        keep[b] = (cols, L, dd, W, z)
    acc, out = [None] * T.nb, [None] * T.nb
    zero = torch.zeros(S, dtype=T.dtype)
    for b in sorted(range(T.nb), key=lambda i: depth[i]):
        par = T.joint_parent[b]
        a = acc[par] if par >= 0 else torch.zeros(S, 6, dtype=T.dtype)
        x = [zero] * 6
        if keep[b] is not None:
            cols, L, dd, W, z = keep[b]
            K = len(cols)
            y = [(z[k] - (W[k] * a).sum(-1)) / dd[k] for k in range(K)]
            for k in range(K - 1, -1, -1):
                t = y[k]
                for i in range(k + 1, K):
                    t = t - L[i][k] * x[i]
                x[k] = t
            for k in range(K):
                a = a + cols[k] * x[k][:, None]
        acc[b], out[b] = a, torch.stack(x, -1)
    return torch.stack(out, 1)


def body_weights(tpl, S, dtype):
    """-> mass [S, nb], inertia [S, nb, 3, 3]: the template's, one copy per set"""
    m, I, _ = inertia_of(tpl, dtype)
    return m.expand(S, -1).clone(), I.expand(S, -1, -1, -1).clone()


def jacobian(T, tpl, body_q, rates):
    """[S, nb, 6, nqd]: body_twists of the unit rates, every column in one call"""
    S, nb, nqd = body_q.shape[0], T.nb, T.nqd
    eye = torch.eye(nqd, dtype=T.dtype)
    bq = body_q[:, None].expand(S, nqd, nb, 7).reshape(S * nqd, nb, 7)
    tw = body_twists(T, bq, slots_of(tpl, eye.repeat(S, 1)), rates)
    return tw.reshape(S, nqd, nb, 6).permute(0, 2, 3, 1)


def twist_form(body_q, mass, inertia, ta, tb):
    """sum_b ta_b . diag(R sym(I) R^T, m)_b . tb_b per set -> [S]; twists [S, nb, 6] = (w, v of the centre of mass)"""
    from oracle import ref_torch as rt

    S, nb = body_q.shape[:2]
    q = body_q[..., 3:].reshape(-1, 4)
    a = rt.q_rot_inv(q, ta[..., :3].reshape(-1, 3)).reshape(S, nb, 3)
    b = rt.q_rot_inv(q, tb[..., :3].reshape(-1, 3)).reshape(S, nb, 3)
    Is = 0.5 * (inertia + inertia.transpose(-1, -2))
    return ((a * (Is @ b[..., None])[..., 0]).sum(-1) + mass * (ta[..., 3:] * tb[..., 3:]).sum(-1)).sum(-1)


def dense_H(T, tpl, body_q, mass, inertia, rates="generalized"):
    """H [S, nqd, nqd] = sum_b J_b^T diag(R sym(I) R^T, m) J_b; in "generalized" mode dp_utils.mass_matrix"""
    from oracle import ref_torch as rt

    S, nb, nqd = body_q.shape[0], T.nb, T.nqd
    J = jacobian(T, tpl, body_q, rates)
    q = body_q[..., None, 3:].expand(S, nb, nqd, 4).reshape(-1, 4)
    Aw = rt.q_rot_inv(q, J[..., :3, :].transpose(-1, -2).reshape(-1, 3)).reshape(S, nb, nqd, 3)
    Is = 0.5 * (inertia + inertia.transpose(-1, -2))
    Jv = J[..., 3:, :]
    return (Aw @ Is @ Aw.transpose(-1, -2)).sum(1) + (mass[:, :, None, None] * (Jv.transpose(-1, -2) @ Jv)).sum(1)


def unslot(tpl, x6):
    """[S, nb, 6] slots -> [S, nqd] in the joint_qd layout"""
    idx = slot_index(tpl).reshape(-1)
    used = np.nonzero(idx < int(tpl["nqd"]))[0]
    out = x6.new_zeros(x6.shape[0], int(tpl["nqd"]))
    out[:, torch.as_tensor(idx[used])] = x6.reshape(x6.shape[0], -1)[:, torch.as_tensor(used)]
    return out


def r_of(C, seed=79):
    """standard-normal joint-space force slots [S, nb, 6] of a case, float32, every slot filled (the op must ignore the unused ones)"""
    return np.random.RandomState(seed).randn(C["bq"].shape[0], C["nb"], 6).astype(np.float32)


def g_out_of(C, seed=83):
    return np.random.RandomState(seed).randn(C["bq"].shape[0], C["nb"], 6).astype(np.float32)


def inverse_of(C, dtype, rates, g_out=None, r6=None):
    """The restatement on a case in ``dtype`` -> dict(out); with g_out [S, nb, 6] also autograd of <g_out, out>: g_body_q, g_r, g_mass,
    g_inertia (per set)."""
    T = oracle_template(C["tpl"], dtype)
    need = g_out is not None
    S = C["bq"].shape[0]
    bq = torch.tensor(np.array(C["bq"]), dtype=dtype).requires_grad_(need)
    r = torch.tensor(np.array(r_of(C) if r6 is None else r6), dtype=dtype).requires_grad_(need)
    m, I = (t.requires_grad_(need) for t in body_weights(C["tpl"], S, dtype))
    out = mass_inverse(T, bq, m, I, r, rates)
    if not need:
        return dict(out=out.numpy())
    (out * torch.as_tensor(np.asarray(g_out), dtype=dtype)).sum().backward()
    return dict(out=out.detach().numpy(), g_body_q=bq.grad.numpy(), g_r=r.grad.numpy(), g_mass=m.grad.numpy(), g_inertia=I.grad.numpy())


def rows23(C, r6=None):
    """The op's operand rows [S * nb, 23] = (p, q xyzw, m, I row-major, r[6]), numpy float32."""
    S, nb = C["bq"].shape[0], C["nb"]
    m, I = body_weights(C["tpl"], S, torch.float32)
    r = r_of(C) if r6 is None else np.asarray(r6, np.float32)
    return np.ascontiguousarray(np.concatenate([C["bq"], m.numpy()[..., None], I.numpy().reshape(S, nb, 9), r], -1).reshape(-1, 23),
                                dtype=np.float32)
