"""Shared by tests/test_mass_matrix_host.py and tests/test_gpu_mass_matrix.py: the torch restatement (float64 as the reference, float32
as the yardstick) of the joint-space mass-matrix op PD_POSE_MASS_MATRIX -- H = sum_b J_b^T diag(R_b sym(I_b) R_b^T, m_b) J_b by the
composite-rigid-body recursion -- and of its vector-Jacobian product, on mass_inverse_ref's state sets (``ALL_CASES``), spatial inertias
and motion subspaces, held to mass_inverse_ref.dense_H.  Nothing here runs product code beyond the model compiler.

Everything in world axes about o0 = the origin of the set's body 0, spatial vectors (angular, linear at o0), as mass_inverse_ref:
  up, deepest level first   Ic_i = I_i + sum_children Ic_c                 (the table's child order)
  per body i with dofs      F_i = Ic_i S_i                                 (6 x K_i)
  walk j = i, pi(i), ...    H[dofs_j, dofs_i] = S_j^T F_i,  H[dofs_i, dofs_j] = its transpose;  every other entry exactly 0
The VJP of <G, H>, G arbitrary, Gs = (G + G^T) / 2 in blocks Gs_ji (K_j x K_i):
  A_i = sum_{j in anc*(i)} S_j Gs_ji                                      (ancestor walk, i included)
  Q_i = A_i S_i^T + S_i A_i^T - S_i Gs_ii S_i^T,   dL/dI_b = P_b = sum_{i in anc*(b)} Q_i
  dL/dS_i = Z_i = 2 (Ic_i A_i + sum_{k in desc(i)} F_k Gs_ki)
and from (P_b, Z_i) into poses, masses and inertias through ``spatial_inertia`` and ``motion_subspace`` (here by autograd of
sum <P_b, I_b> + sum <Z_i, S_i> with P and Z held constant; the kernel chains them by hand)."""
import numpy as np
import torch

from mass_inverse_ref import (ALL_CASES, DOFS, RATES, accel_case, body_weights, dense_H, motion_subspace, robot_template,  # noqa: F401
                              spatial_inertia)
from generalized_force_ref import tree
from joint_coords_ref import oracle_template

TENSORS = ("out", "g_body_q", "g_mass", "g_inertia")


def dof_starts(tpl):
    return np.asarray(tpl["joint_qd_start"]).reshape(-1).astype(np.int64)


def related_mask(tpl):
    """[nqd, nqd] bool: True where the two dofs belong to bodies one of which is the other's ancestor (or the same body)"""
    nb, nqd = int(tpl["nb"]), int(tpl["nqd"])
    par = np.asarray(tpl["joint_parent"]).reshape(-1)
    ty = np.asarray(tpl["joint_type"]).reshape(-1)
    qds = dof_starts(tpl)
    mask = np.zeros((nqd, nqd), bool)
    for i in range(nb):
        Ki, j = DOFS[int(ty[i])], i
        while j >= 0:
            Kj = DOFS[int(ty[j])]
            mask[qds[j]: qds[j] + Kj, qds[i]: qds[i] + Ki] = True
            mask[qds[i]: qds[i] + Ki, qds[j]: qds[j] + Kj] = True
            j = int(par[j])
    return mask


def parts(T, tpl, body_q, mass, inertia, rates):
    """-> (Sm, Ib, Ic, F): per body the motion subspace [S, 6, K] (None without a dof), its own and its composite spatial inertia
    [S, 6, 6] about o0 and F = Ic S"""
    from oracle import ref_torch as rt

    S = body_q.shape[0]
    o0 = body_q[:, 0, :3]
    kids, depth = tree(T)
    d = [(body_q[:, b, :3] - o0) + rt.q_rot(body_q[:, b, 3:], T.com[b].expand(S, 3)) for b in range(T.nb)]
    Sm, Ib, Ic, F = [None] * T.nb, [None] * T.nb, [None] * T.nb, [None] * T.nb
    for b in sorted(range(T.nb), key=lambda i: -depth[i]):
        Ib[b] = spatial_inertia(body_q, b, d[b], mass, inertia)
        Ic[b] = Ib[b]
        for c in kids[b]:
            Ic[b] = Ic[b] + Ic[c]
        cols = motion_subspace(T, body_q, b, d, o0, rates)
        assert len(cols) == DOFS[T.joint_type[b]]
        if cols:
            Sm[b] = torch.stack(cols, -1)
            F[b] = Ic[b] @ Sm[b]
    return Sm, Ib, Ic, F


def crba(T, tpl, body_q, mass, inertia, rates="generalized"):
    """body_q [S, nb, 7], mass [S, nb], inertia [S, nb, 3, 3] -> H [S, nqd, nqd] in the joint_qd layout"""
    assert rates in RATES
    Sm, _, _, F = parts(T, tpl, body_q, mass, inertia, rates)
    qds = dof_starts(tpl)
    S, nqd = body_q.shape[0], T.nqd
    H = torch.zeros(S, nqd, nqd, dtype=body_q.dtype)
    blocks = []
    for i in range(T.nb):
        if Sm[i] is None:
            continue
        j = i
        while j >= 0:
            if Sm[j] is not None:
                blocks.append((j, i, Sm[j].transpose(-1, -2) @ F[i]))
            j = T.joint_parent[j]
    pieces = H
    for j, i, blk in blocks:   # (out of place: autograd flows through every block)
        Kj, Ki = blk.shape[-2:]
        pad = torch.zeros(S, nqd, nqd, dtype=body_q.dtype)
        pad[:, qds[j]: qds[j] + Kj, qds[i]: qds[i] + Ki] = blk
        if j != i:
            pad[:, qds[i]: qds[i] + Ki, qds[j]: qds[j] + Kj] = blk.transpose(-1, -2)
        else:   # the diagonal block from its upper triangle: the same value on both sides
            up = torch.triu(blk)
            pad[:, qds[i]: qds[i] + Ki, qds[i]: qds[i] + Ki] = up + torch.triu(blk, 1).transpose(-1, -2)
        pieces = pieces + pad
    return pieces


def vjp_parts(T, tpl, body_q, mass, inertia, rates, G):
    """G [S, nqd, nqd] arbitrary -> (P, Z): dL/dI_b [S, 6, 6] per body and dL/dS_i [S, 6, K_i] (None without a dof), by the formulas"""
    Sm, _, Ic, F = parts(T, tpl, body_q, mass, inertia, rates)
    qds = dof_starts(tpl)
    kids, depth = tree(T)
    Gs = 0.5 * (G + G.transpose(-1, -2))
    K = [0 if s is None else s.shape[-1] for s in Sm]
    blk = lambda j, i: Gs[:, qds[j]: qds[j] + K[j], qds[i]: qds[i] + K[i]]
    zero66 = torch.zeros(body_q.shape[0], 6, 6, dtype=body_q.dtype)
    A, Q = [None] * T.nb, [zero66] * T.nb
    for i in range(T.nb):
        if not K[i]:
            continue
        A[i], j = 0, i
        while j >= 0:
            if K[j]:
                A[i] = A[i] + Sm[j] @ blk(j, i)
            j = T.joint_parent[j]
        Si = Sm[i]
        Q[i] = A[i] @ Si.transpose(-1, -2) + Si @ A[i].transpose(-1, -2) - Si @ blk(i, i) @ Si.transpose(-1, -2)
    P = [None] * T.nb
    for b in sorted(range(T.nb), key=lambda i: depth[i]):
        par = T.joint_parent[b]
        P[b] = Q[b] + (P[par] if par >= 0 else 0)
    Z = [None] * T.nb
    for i in range(T.nb):
        if not K[i]:
            continue
        acc = Ic[i] @ A[i]
        for k in range(T.nb):
            if k == i or not K[k]:
                continue
            j = T.joint_parent[k]
            while j >= 0 and j != i:
                j = T.joint_parent[j]
            if j == i:
                acc = acc + F[k] @ blk(k, i)
        Z[i] = 2.0 * acc
    return P, Z


def crba_vjp(T, tpl, body_q, mass, inertia, rates, G):
    """-> (g_body_q, g_mass, g_inertia) of <G, H>: the formulas' (P, Z) chained through the spatial inertias and motion subspaces"""
    with torch.no_grad():
        P, Z = vjp_parts(T, tpl, body_q, mass, inertia, rates, G)
    leaves = [t.detach().clone().requires_grad_(True) for t in (body_q, mass, inertia)]
    Sm, Ib, _, _ = parts(T, tpl, leaves[0], leaves[1], leaves[2], rates)
    form = 0
    for b in range(T.nb):
        form = form + (P[b] * Ib[b]).sum()
        if Sm[b] is not None:
            form = form + (Z[b] * Sm[b]).sum()
    return torch.autograd.grad(form, leaves)


def g_out_of(C, seed=89):
    """a standard-normal, NOT symmetric upstream gradient [S, nqd, nqd], float32"""
    return np.random.RandomState(seed).randn(C["bq"].shape[0], C["nqd"], C["nqd"]).astype(np.float32)


def scaled_error(H, H64):
    """E(H) = max_ab |H - H64|_ab / sqrt(H64_aa H64_bb): the per-entry scale (a FREE block is about 20, distal hinges about 2e-3)"""
    H, H64 = np.asarray(H, np.float64), np.asarray(H64, np.float64)
    dg = np.sqrt(np.diagonal(H64, axis1=-2, axis2=-1))
    return float((np.abs(H - H64) / (dg[..., :, None] * dg[..., None, :])).max())


def matrix_of(C, dtype, rates, g_out=None, shared=False, dense=True):
    """dense_H (dense=False: the recursion) on a case in ``dtype`` -> dict(out); with g_out [S, nqd, nqd] also autograd of <g_out, H>:
    g_body_q, g_mass, g_inertia (per set; shared: masses and inertias are one copy for all sets, so theirs are the sums)"""
    T = oracle_template(C["tpl"], dtype)
    need = g_out is not None
    S = C["bq"].shape[0]
    bq = torch.tensor(np.array(C["bq"]), dtype=dtype).requires_grad_(need)
    m, I = (t.requires_grad_(need) for t in body_weights(C["tpl"], S, dtype))
    out = dense_H(T, C["tpl"], bq, m, I, rates) if dense else crba(T, C["tpl"], bq, m, I, rates)
    if not need:
        return dict(out=out.detach().numpy())
    (out * torch.as_tensor(np.asarray(g_out), dtype=dtype)).sum().backward()
    gm, gI = m.grad.numpy(), I.grad.numpy()
    if shared:
        gm, gI = gm.sum(0), gI.sum(0)
    return dict(out=out.detach().numpy(), g_body_q=bq.grad.numpy(), g_mass=gm, g_inertia=gI)


def rows17(C):
    """The op's operand rows [S * nb, 17] = (p, q xyzw, m, I row-major), numpy float32."""
    S, nb = C["bq"].shape[0], C["nb"]
    m, I = body_weights(C["tpl"], S, torch.float32)
    return np.ascontiguousarray(np.concatenate([C["bq"], m.numpy()[..., None], I.numpy().reshape(S, nb, 9)], -1).reshape(-1, 17),
                                dtype=np.float32)
