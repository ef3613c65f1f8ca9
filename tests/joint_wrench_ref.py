"""Shared by tests/test_joint_wrench_host.py and tests/test_gpu_joint_wrench.py: the torch restatement (float64, or float32 as the
yardstick) of the joint-wrench op PD_POSE_JOINT_WRENCH -- oracle/ref_torch.py eval_body_joints as a function of ONE state set and the
controls, built from that module's own quaternion functions -- and the state sets the op is held to.  Nothing here runs product code
beyond the model compiler (generated_robots).

The restatement is eval_body_joints (ref_torch.py:254-334) with three evaluations written in their stable forms, the SAME functions:
  twist angle   2 sgn atan2(|axis| |da|, w), da = r_err.xyz . axis           for 2 acos(normalize((axis da, w)).w) sgn (:294-297)
  FIXED error   v h, h = 2 atan2(|v|, w) / |v| (series of atan(x) / x below |v| / w = 1e-2)   for normalize(v) 2 acos(w), |r_err| = 1 (:287)
  lever arms    r_c = -R(q_c) com_c, r_p = R(q_p) (p_pj - com_p), x_err = (p_c - p_p) - R(q_p) p_pj      for the differences of :272-278
A literal fp32 acos is 1e-4 .. 1e-3 off float64 on robots with FIXED joints: as the fp32 yardstick it would make the 4 x bar
meaningless.  In float64 the restatement and eval_body_joints agree to 1e-9 (tests/test_joint_wrench_host.py)."""
import functools

import numpy as np
import torch

from generated_robots import robot
from joint_coords_ref import compound_axes, joint_frame, load_tpl, oracle_template, random_coords

SHIPPED = ("laikago", "human", "laikago_toes")
TENSORS = ("out", "g_body_q", "g_body_qd", "g_act", "g_target", "g_ke", "g_kd")
# (robot, state sets, kind) of every GPU case.  Laikago 41: 19 sets per workgroup, the last workgroup partial; mixed25 11: two workgroups,
# every joint type, turned child frames, a body with 8 children; rev256: the cap, one set per workgroup; worldmix9 / world5: roots
# jointed to the world; cmp20-limits "limits": angles beyond both limits with both rate signs; free1: zeros.
CASES = [("laikago", 1, "fk"), ("laikago", 5, "fk"), ("laikago", 41, "fk"), ("human", 3, "fk"), ("laikago_toes", 2, "fk"),
         ("mixed25", 11, "fk"), ("cmp31", 3, "fk"), ("worldmix9", 4, "fk"), ("world5", 3, "fk"), ("cmp20-limits", 4, "limits"),
         ("rev256", 1, "fk"), ("rev256", 2, "fk"), ("free1", 3, "fk")]


def template(name):
    return load_tpl(name) if name in SHIPPED else robot(name)


def fixed_ang(v, w):
    """normalize(v) 2 acos(w) of a unit quaternion (v, w) in its scale-invariant form v h (csrc/pd_math.h fixed_ang_h)."""
    s2 = (v * v).sum(-1)
    small = (w > 0) & (s2 < 1e-4 * w * w)
    ws = torch.where(small, w, torch.ones_like(w))
    x2 = torch.where(small, s2, torch.zeros_like(s2)) / (ws * ws)
    series = 2.0 * (1.0 - x2 * (1.0 / 3.0 - x2 * (1.0 / 5.0 - x2 * (1.0 / 7.0)))) / ws
    sl = torch.sqrt(torch.where(small, torch.ones_like(s2), s2))
    return v * torch.where(small, series, 2.0 * torch.atan2(sl, w) / sl)[:, None]


def joint_pairs(T, body_q, body_qd, target, act, ke, kd, drop_fixed_angle=False):
    """-> per body None (FREE) or (t, f, r_p or None, r_c), each [S, 3].  drop_fixed_angle: FIXED joints without their angular spring."""
    from oracle import ref_torch as rt

    S = body_q.shape[0]
    ake, akd, ads = T.attach_ke, T.attach_kd, 0.01
    pairs = []
    for i in range(T.nb):
        ty, par, qds = T.joint_type[i], T.joint_parent[i], T.qd_start[i]
        if ty == rt.JOINT_FREE:
            pairs.append(None)
            continue
        _, q_wj, w_p, v_p = joint_frame(T, body_q, body_qd, i)
        p_c, q_c = body_q[:, i, :3], body_q[:, i, 3:]
        w_c, v_c = body_qd[:, i, :3], body_qd[:, i, 3:]
        p_pj = T.X_p[i, :3].expand(S, 3)
        r_c = -rt.q_rot(q_c, T.com[i].expand(S, 3))
        if par >= 0:
            pp, qp = body_q[:, par, :3], body_q[:, par, 3:]
            r_p = rt.q_rot(qp, (T.X_p[i, :3] - T.com[par]).expand(S, 3))
            x_err = (p_c - pp) - rt.q_rot(qp, p_pj)
        else:
            r_p, x_err = None, p_c - p_pj
        r_err = rt.q_mul(rt.q_conj(q_wj), q_c)
        v_err, w_err = v_c - v_p, w_c - w_p
        f = x_err * ake + v_err * akd
        lim = lambda j: (T.limit_lower[j], T.limit_upper[j], T.limit_ke[j], T.limit_kd[j])
        if ty == rt.JOINT_FIXED:
            t = w_err * akd * ads
            if not drop_fixed_angle:
                t = t + rt.q_rot(q_wj, fixed_ang(r_err[:, :3], r_err[:, 3])) * ake
        elif ty == rt.JOINT_REVOLUTE:
            axis = T.axis[i].expand(S, 3)
            axis_p, axis_c = rt.q_rot(q_wj, axis), rt.q_rot(q_c, axis)
            da = rt.dot(r_err[:, :3], axis)
            sgn = torch.where(da < 0, -1.0, 1.0).to(T.dtype)
            q = 2.0 * sgn * torch.atan2(da.abs() * torch.sqrt(rt.dot(T.axis[i], T.axis[i])), r_err[:, 3])
            qd = rt.dot(w_err, axis_p)
            t = rt.eval_joint_force(q, qd, target[:, qds], ke[:, qds], kd[:, qds], act[:, qds], *lim(qds), axis_p)
            t = t + rt.cross(axis_p, axis_c) * ake + (w_err - qd[:, None] * axis_p) * akd * ads
        elif ty == rt.JOINT_COMPOUND:
            q_off = T.X_c[i, 3:].expand(S, 4)
            q_pc = rt.q_mul(rt.q_mul(rt.q_mul(rt.q_conj(q_off), rt.q_conj(q_wj)), q_c), q_off)
            angles = rt.quat_decompose(q_pc)
            q_w = rt.q_mul(q_wj, q_off)
            t = torch.zeros(S, 3, dtype=T.dtype)
            for k, ax in enumerate(compound_axes(angles)):
                axw, j = rt.q_rot(q_w, ax), qds + k
                t = t + rt.eval_joint_force(angles[:, k], rt.dot(axw, w_err), target[:, j], ke[:, j], kd[:, j], act[:, j], *lim(j), axw)
            t, f = torch.clamp(t, -1.0e4, 1.0e4), torch.clamp(f, -1.0e4, 1.0e4)
        else:
            raise NotImplementedError("joint type %d" % ty)
        pairs.append((t, f, r_p, r_c))
    return pairs


def joint_wrench(T, body_q, body_qd, target, act, ke, kd, drop_fixed_angle=False):
    """body_q [S, nb, 7], body_qd [S, nb, 6] (Warp order w, v), target / act / ke / kd [S, nqd] of the template's dtype -> [S, nb, 6]:
    out_i = -(t_i + r_c x f_i, f_i) + sum over the children c of i, in index order, of (t_c + r_p x f_c, f_c)."""
    from oracle import ref_torch as rt

    S = body_q.shape[0]
    pairs = joint_pairs(T, body_q, body_qd, target, act, ke, kd, drop_fixed_angle)
    out = []
    for i in range(T.nb):
        acc = torch.zeros(S, 6, dtype=T.dtype)
        if pairs[i] is not None:
            t, f, _, r_c = pairs[i]
            acc = acc - torch.cat([t + rt.cross(r_c, f), f], -1)
        for c in range(T.nb):
            if T.joint_parent[c] == i and pairs[c] is not None:
                t, f, r_p, _ = pairs[c]
                acc = acc + torch.cat([t + rt.cross(r_p, f), f], -1)
        out.append(acc)
    return torch.stack(out, 1)


def _jitter(rng, bq, bqd, pos=2e-3, rot=1e-2, twist=0.3):
    """FK states pushed off the joint manifold (float64): positions by ~pos m, rotations by ~rot rad about random axes, twists random."""
    from oracle import ref_torch as rt

    bq, bqd = bq.copy(), bqd.copy()
    bq[..., :3] += pos * rng.randn(*bq.shape[:-1], 3)
    aa = rot * rng.randn(*bq.shape[:-1], 3)
    ang = np.linalg.norm(aa, axis=-1, keepdims=True)
    dq = np.concatenate([aa / ang * np.sin(ang / 2), np.cos(ang / 2)], -1)
    q = rt.q_mul(torch.as_tensor(dq), torch.as_tensor(bq[..., 3:])).numpy()
    bq[..., 3:] = q / np.linalg.norm(q, axis=-1, keepdims=True)
    bqd += twist * rng.randn(*bqd.shape)
    return bq, bqd


def controls(rng, S, nqd, gain=30.0):
    """targets +-0.5, gains 30 / 0.3 with per-dof variation, small torques -> dict of float32 [S, nqd]"""
    c = dict(target=rng.uniform(-0.5, 0.5, (S, nqd)), ke=gain * (1.0 + 0.3 * rng.uniform(-1, 1, (S, nqd))),
             kd=0.01 * gain * (1.0 + 0.3 * rng.uniform(-1, 1, (S, nqd))), act=0.05 * rng.randn(S, nqd))
    return {k: v.astype(np.float32) for k, v in c.items()}


@functools.lru_cache(maxsize=None)
def case(name, S, kind="fk"):
    """dict(tpl, nb, nqd, bq [S, nb, 7], bqd [S, nb, 6], target / act / ke / kd [S, nqd]), float32, shared and never written: float64 FK
    of random coordinates (angles 0.05 <= |q| <= 1, the root within +-1 m) jittered off the manifold, then rounded to fp32.
    kind "limits": the first angle of every COMPOUND joint of the sets 0 .. 3 starts at +1.62, -1.62, +1.7, -1.7 -- beyond the limits of
    +-1.5 -- and the twists are drawn so that both rate signs occur.  kind "exact": no jitter (the states FK made)."""
    from oracle import ref_torch as rt

    tpl = template(name)
    nb, nqd = int(tpl["nb"]), int(tpl["nqd"])
    rng = np.random.RandomState(1000 + 7 * S + len(name))
    q, qd = random_coords(tpl, S, seed=300 + S, lo=0.05, hi=1.0)
    if kind == "limits":
        ty, qs = np.asarray(tpl["joint_type"]).reshape(-1), np.asarray(tpl["joint_q_start"]).reshape(-1)
        for s, a in zip(range(S), (1.62, -1.62, 1.7, -1.7)):
            q[s, [int(qs[b]) for b in range(nb) if int(ty[b]) == 5]] = a
    T64 = oracle_template(tpl)
    bq, bqd = rt.eval_fk(T64, torch.as_tensor(q), torch.as_tensor(qd))
    bq, bqd = bq.numpy(), bqd.numpy()
    if kind != "exact":
        bq, bqd = _jitter(rng, bq, bqd)
    C = dict(tpl=tpl, nb=nb, nqd=nqd, bq=bq.astype(np.float32), bqd=bqd.astype(np.float32), **controls(rng, S, nqd))
    for v in C.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return C


def wrench_of(C, dtype, g_out=None, drop_fixed_angle=False, **override):
    """The restatement on a case in ``dtype`` -> dict(out); with g_out [S, nb, 6] also autograd of <g_out, out>: g_body_q, g_body_qd and
    g_act, g_target, g_ke, g_kd [S, nqd].  override: arrays that stand in for the case's."""
    C = dict(C, **override)
    T = oracle_template(C["tpl"], dtype)
    need = g_out is not None
    names = ("bq", "bqd", "target", "act", "ke", "kd")
    t = {k: torch.tensor(np.array(C[k]), dtype=dtype).requires_grad_(need) for k in names}
    out = joint_wrench(T, *[t[k] for k in names], drop_fixed_angle=drop_fixed_angle)
    if not need:
        return dict(out=out.numpy())
    if out.requires_grad:   # (a robot without a joint that pulls: nothing to differentiate)
        (out * torch.as_tensor(np.asarray(g_out), dtype=dtype)).sum().backward()
    grad = lambda k: t[k].grad.numpy() if t[k].grad is not None else np.zeros(t[k].shape)
    return dict(out=out.detach().numpy(), g_body_q=grad("bq"), g_body_qd=grad("bqd"), g_act=grad("act"), g_target=grad("target"),
                g_ke=grad("ke"), g_kd=grad("kd"))


def input_conditions(C):
    """float64, per case: dict(theta = the largest |second angle| of a COMPOUND joint, limit_gap = the smallest distance of a dof with a
    limit gain from its limits, limit_rate = the smallest |rate| of a dof beyond such a limit, clamp_gap = the smallest relative distance
    of a COMPOUND pair's component from +-1e4, engaged = the number of (set, dof) beyond a limit with a gain)."""
    from oracle import ref_torch as rt
    from joint_coords_ref import joint_coords

    T = oracle_template(C["tpl"])
    bq, bqd = torch.tensor(np.array(C["bq"]), dtype=torch.float64), torch.tensor(np.array(C["bqd"]), dtype=torch.float64)
    c = {k: torch.tensor(np.array(C[k]), dtype=torch.float64) for k in ("target", "act", "ke", "kd")}
    theta, gap, rate, engaged, clamp_gap = 0.0, np.inf, np.inf, 0, np.inf
    if T.nq:
        jq, jqd = joint_coords(T, bq, bqd, "measured")
        for i in range(T.nb):
            ty, qs, qds = T.joint_type[i], T.q_start[i], T.qd_start[i]
            n_dof = {rt.JOINT_REVOLUTE: 1, rt.JOINT_COMPOUND: 3}.get(ty, 0)
            if ty == rt.JOINT_COMPOUND:
                theta = max(theta, float(jq[:, qs + 1].abs().max()))
            for k in range(n_dof):
                if float(T.limit_ke[qds + k]) == 0.0 and float(T.limit_kd[qds + k]) == 0.0:
                    continue
                a, r = jq[:, qs + k], jqd[:, qds + k]
                lo, up = T.limit_lower[qds + k], T.limit_upper[qds + k]
                gap = min(gap, float(torch.minimum((a - lo).abs(), (a - up).abs()).min()))
                beyond = (a < lo) | (a > up)
                engaged += int(beyond.sum())
                if beyond.any():
                    rate = min(rate, float(r[beyond].abs().min()))
    unclamped = joint_pairs_raw(T, bq, bqd, c)
    if unclamped.size:
        clamp_gap = float(np.abs(np.abs(unclamped) / 1.0e4 - 1.0).min())
    return dict(theta=theta, limit_gap=gap, limit_rate=rate, engaged=engaged, clamp_gap=clamp_gap)


def joint_pairs_raw(T, bq, bqd, c):
    """The COMPOUND joints' pairs BEFORE the clamp, float64 numpy [number of compound joints, S, 6] (torque, force)."""
    from oracle import ref_torch as rt

    S = bq.shape[0]
    raw = []
    for i in range(T.nb):
        if T.joint_type[i] != rt.JOINT_COMPOUND:
            continue
        par, qds = T.joint_parent[i], T.qd_start[i]
        _, q_wj, w_p, v_p = joint_frame(T, bq, bqd, i)
        q_c = bq[:, i, 3:]
        x_err = bq[:, i, :3] - T.X_p[i, :3] if par < 0 else (bq[:, i, :3] - bq[:, par, :3]) - rt.q_rot(bq[:, par, 3:], T.X_p[i, :3].expand(S, 3))
        f = x_err * T.attach_ke + (bqd[:, i, 3:] - v_p) * T.attach_kd
        w_err = bqd[:, i, :3] - w_p
        q_off = T.X_c[i, 3:].expand(S, 4)
        angles = rt.quat_decompose(rt.q_mul(rt.q_mul(rt.q_mul(rt.q_conj(q_off), rt.q_conj(q_wj)), q_c), q_off))
        q_w = rt.q_mul(q_wj, q_off)
        t = torch.zeros(S, 3, dtype=T.dtype)
        for k, ax in enumerate(compound_axes(angles)):
            axw, j = rt.q_rot(q_w, ax), qds + k
            t = t + rt.eval_joint_force(angles[:, k], rt.dot(axw, w_err), c["target"][:, j], c["ke"][:, j], c["kd"][:, j], c["act"][:, j],
                                        T.limit_lower[j], T.limit_upper[j], T.limit_ke[j], T.limit_kd[j], axw)
        raw.append(torch.cat([t, f], -1).numpy())
    return np.asarray(raw)


def slot_index(tpl):
    """[nb, 3]: the dof behind slot k of each body's joint (qd_start + k), or nqd for a slot no dof uses -- restated, not imported."""
    nb, nqd = int(tpl["nb"]), int(tpl["nqd"])
    ty, qds = np.asarray(tpl["joint_type"]).reshape(-1), np.asarray(tpl["joint_qd_start"]).reshape(-1)
    idx = np.full((nb, 3), nqd, np.int64)
    for b in range(nb):
        for k in range({1: 1, 5: 3}.get(int(ty[b]), 0)):
            idx[b, k] = int(qds[b]) + k
    return idx


def rows25(C, fill=0.0, **override):
    """The op's operand rows [S * nb, 25] (numpy float32) of a case: state, then act, target, ke, kd in the body's dof slots; ``fill`` in
    the slots no dof uses."""
    C = dict(C, **override)
    idx = slot_index(C["tpl"])
    S = C["bq"].shape[0]
    cols = [C["bq"], C["bqd"]]
    for k in ("act", "target", "ke", "kd"):
        ext = np.concatenate([C[k], np.full((S, 1), fill, np.float32)], 1)
        cols.append(ext[:, idx])   # [S, nb, 3]
    return np.ascontiguousarray(np.concatenate(cols, -1).reshape(S * C["nb"], 25), dtype=np.float32)


def dof_grads(tpl, g_rows):
    """g_rows [S, nb, 25] -> dict(g_act, g_target, g_ke, g_kd) [S, nqd]: the used slots' entries scattered back to their dofs."""
    idx = slot_index(tpl)
    nqd = int(tpl["nqd"])
    S = g_rows.shape[0]
    out = {}
    for j, k in enumerate(("g_act", "g_target", "g_ke", "g_kd")):
        ext = np.zeros((S, nqd + 1))
        ext[:, idx.reshape(-1)] = g_rows[:, :, 13 + 3 * j: 16 + 3 * j].reshape(S, -1)
        out[k] = ext[:, :nqd]
    return out


def unused_slots(tpl):
    """[nb, 12] bool: the control columns (13 .. 24 of a row) no dof of the body's joint uses."""
    return np.tile(slot_index(tpl) == int(tpl["nqd"]), (1, 4))
