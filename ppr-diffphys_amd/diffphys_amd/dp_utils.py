"""Loss / frame utilities around the simulator boundary.
Same names and semantics as /root/reference/diffphys/dp_utils.py (cited per function)."""
from typing import NamedTuple

import torch

from .dataloader import bullet2gl  # noqa: F401  (re-exported like the reference's dp_utils)


class _PoseOpHip(torch.autograd.Function):
    """One of the pose compositions / projections below as ONE HIP launch, its vector-Jacobian product as one more (C ABI
    ``pd_pose_op`` / ``pd_pose_op_vjp``; the Jacobian is taken inside the kernel by forward-mode differentiation of the
    code that computed the value)."""

    @staticmethod
    def forward(ctx, op, a, b):
        from . import hip_backend

        a, b = a.detach().contiguous(), b.detach().contiguous()
        ctx.op = op
        ctx.save_for_backward(a, b)
        return hip_backend.pose_op(op, a, b)

    @staticmethod
    def backward(ctx, g):
        from . import hip_backend

        a, b = ctx.saved_tensors
        need_a, need_b = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        g_a, g_b = hip_backend.pose_op_vjp(ctx.op, a, b, g.contiguous(), need_a, need_b)
        return None, g_a, g_b


def _need_gpu(what, *ts):
    """The pose algebra and se3_loss run as HIP kernels and nowhere else: float32 GPU tensors, or an error (no CPU / torch fallback;
    their float64 torch restatement is test infrastructure: oracle/pose_torch.py)."""
    for t in ts:
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32):
            raise TypeError("%s needs float32 GPU tensors (the product path has no CPU fallback); got %s" % (
                what, "%s on %s" % (t.dtype, t.device) if torch.is_tensor(t) else type(t).__name__))


def compose_delta(target_q, delta_root):
    """delta (bs,T,6 axis-angle) applied on the left of target (bs,T,7)   dp_utils.py:22-31"""
    _need_gpu("compose_delta", target_q, delta_root)
    if not (target_q.shape[-1] == 7 and delta_root.shape[-1] == 6 and target_q.shape[:-1] == delta_root.shape[:-1]):
        raise ValueError("compose_delta: target (..., 7) and delta (..., 6) with equal leading shapes; got %s and %s" % (tuple(target_q.shape), tuple(delta_root.shape)))
    return _PoseOpHip.apply(0, target_q, delta_root)


def remove_nan(t, bs=None, clip=False):
    """in place NaN -> 0 (and optional +-0.01 clip)   dp_utils.py:43-57"""
    t.masked_fill_(t.isnan(), 0)  # (the reference's t[t.isnan()] = 0 without its host synchronisation)
    if clip:
        t.clamp_(-0.01, 0.01)


def rotate_frame(global_q, target_q):
    """T = T_global @ T_target   dp_utils.py:60-73"""
    _need_gpu("rotate_frame", global_q, target_q)
    if not (global_q.shape == (7,) and target_q.shape[-1] == 7):
        raise ValueError("rotate_frame: one global pose (7,) against targets (..., 7); got %s and %s" % (tuple(global_q.shape), tuple(target_q.shape)))
    return _PoseOpHip.apply(1, global_q, target_q)


def rotate_frame_vel(global_q, target_qd):
    """rotate (linear, angular) halves by the rotation of global_q   dp_utils.py:76-84"""
    _need_gpu("rotate_frame_vel", global_q, target_qd)
    if not (global_q.shape == (7,) and target_qd.shape[-1] == 6):
        raise ValueError("rotate_frame_vel: one global pose (7,) against twists (..., 6); got %s and %s" % (tuple(global_q.shape), tuple(target_qd.shape)))
    return _PoseOpHip.apply(2, global_q, target_qd)


def reduce_loss(loss_seq, clip=False, th=0):
    """(bs,T) -> scalar; with clip, a rollout's loss is zeroed (in place) from the first step that exceeds the threshold on -- the
    threshold being 10x the median of the positive entries of ENV 0: the reference computes it at i == 0 and reuses it for every env
    (dp_utils.py:93-110).  When env 0 has no positive entry the reference's median of an empty selection is NaN, ``th == 0`` is never
    true again and ``loss > NaN`` is false: nothing is clipped in the whole batch -- reproduced here (held to the reference's own outputs,
    tests/golden/ref_host_reduce_loss.npz).  Same values and in-place effect as the reference's per-env loop without its host
    synchronisations (~4 per env and iteration)."""
    if clip and loss_seq.shape[0] > 0:
        row = loss_seq.detach()[0]
        rp = row > 0
        srt = torch.where(rp, row, torch.full_like(row, float("inf"))).sort().values
        med = srt.gather(0, ((rp.sum() - 1).clamp(min=0) // 2).reshape(1))[0]  # torch.median: the lower one
        th0 = torch.where(rp.any(), med * 10, torch.full_like(med, float("nan")))
        if torch.is_tensor(th):
            th = torch.where(th.detach().to(th0) == 0, th0, th.detach().to(th0))
        elif th == 0:
            th = th0
        keep = (loss_seq.detach() > th).cumsum(1) == 0
        loss_seq.masked_fill_(~keep, 0)  # assignment like the reference's loss_seq[i, idx:] = 0: an inf / NaN past the clip is zeroed, not 0 * inf
    pos = loss_seq > 0
    mean_pos = torch.where(pos, loss_seq, torch.zeros_like(loss_seq)).sum() / pos.sum().clamp(min=1)
    return torch.where(loss_seq.sum() > 0, mean_pos, loss_seq.mean())


class _ReduceLossHip(torch.autograd.Function):
    """reduce_loss WITHOUT clipping on a float32 GPU table (bs, F), as the library's one-workgroup launch (``pd_reduce_loss``, the code the
    trajectory-loss entries run; held to the reference's own outputs in tests/test_ref_fixtures.py) and one multiply for the gradient
    (scale = d value / d entry, written by the same launch) -- the torch composition above is ~15 launches forward and ~8 backward."""

    @staticmethod
    def forward(ctx, table):
        from . import hip_backend

        reduced, scale = hip_backend.reduce_loss(table.detach().contiguous(), clip=False, want_scale=table.requires_grad)
        if table.requires_grad:
            ctx.save_for_backward(scale)
        return reduced[0]

    @staticmethod
    def backward(ctx, g):
        (scale,) = ctx.saved_tensors
        return g * scale


def reduce_loss_masked(loss_seq, mask):
    """reduce_loss(loss_seq with the entries under `mask` set to 0) -- the two state losses of phys_model.forward (dp_model.py:783-805 of the
    reference: `loss[outseq_idx] = 0` then reduce_loss).  float32 GPU tables take the HIP launch, anything else the torch composition."""
    x = loss_seq.masked_fill(mask, 0.0)
    if x.is_cuda and x.dtype == torch.float32 and x.dim() == 2:
        return _ReduceLossHip.apply(x)
    return reduce_loss(x)


class _Se3LossHip(torch.autograd.Function):
    """se3_loss and both gradients in one HIP launch (C ABI ``pd_se3_loss``)."""

    @staticmethod
    def forward(ctx, pred, gt, rot_ratio):
        from . import hip_backend

        need = pred.requires_grad or gt.requires_grad
        loss, gp, gg = hip_backend.se3_loss(pred.detach().contiguous(), gt.detach().contiguous(), rot_ratio, want_grads=need)
        if need:
            ctx.save_for_backward(gp, gg)
        return loss

    @staticmethod
    def backward(ctx, g):
        gp, gg = ctx.saved_tensors
        g = g.unsqueeze(-1)
        return (g * gp if ctx.needs_input_grad[0] else None), (g * gg if ctx.needs_input_grad[1] else None), None


def se3_loss(pred, gt, rot_ratio=0.1):
    """|dp|^2 + rot_ratio * angle(R_pred R_gt^T); quaternion (real-last) or axis-angle rotations   dp_utils.py:113-138.
    One HIP launch for the value and both gradients (``pd_se3_loss``); float32 GPU tensors only."""
    _need_gpu("se3_loss", pred, gt)
    if pred.shape != gt.shape:
        raise ValueError("se3_loss: pred and gt must have the same shape; got %s and %s" % (tuple(pred.shape), tuple(gt.shape)))
    return _Se3LossHip.apply(pred, gt, rot_ratio)


def parse_rtk(rtk):
    """rtk (..., 4, 4): rows 0-2 [R|t] world -> view, row 3 (fx, fy, cx, cy) -> (rtmat (..., 4, 4), kmat (..., 3, 3))   dp_utils.py:184-197.
    Plain slicing on any device, as the reference does it."""
    rtmat = torch.zeros_like(rtk)
    rtmat[..., :3, :] = rtk[..., :3, :]
    rtmat[..., -1, -1] = 1
    kmat = torch.zeros_like(rtk[..., :3, :3])
    kmat[..., 0, 0] = rtk[..., 3, 0]
    kmat[..., 1, 1] = rtk[..., 3, 1]
    kmat[..., 0, 2] = rtk[..., 3, 2]
    kmat[..., 1, 2] = rtk[..., 3, 3]
    kmat[..., -1, -1] = 1
    return rtmat, kmat


def _check_cameras(what, bodies, rtk):
    if not (torch.is_tensor(bodies) and torch.is_tensor(rtk) and bodies.dim() >= 2 and bodies.shape[-1] == 7 and rtk.dim() >= 2
            and tuple(rtk.shape[-2:]) == (4, 4) and tuple(bodies.shape[:-2]) == tuple(rtk.shape[:-2])):
        raise ValueError("%s: bodies (..., K, 7) and rtk (..., 4, 4) with equal leading shapes; got %s and %s" % (
            what, tuple(getattr(bodies, "shape", ())), tuple(getattr(rtk, "shape", ()))))


def project_bodies(bodies, rtk):
    """Body origins (..., K, 7) through the pinhole cameras rtk (..., 4, 4) -> pixels (..., K, 2)   dp_utils.py:200-214.
    One HIP launch (``pd_pose_op`` PD_POSE_PROJECT; the camera of a leading index serves its K bodies) and one for the gradients of
    BOTH operands; float32 GPU tensors only.  No clamp: a point in the camera plane gives inf / NaN, as in the reference."""
    _check_cameras("project_bodies", bodies, rtk)
    _need_gpu("project_bodies", bodies, rtk)
    return _PoseOpHip.apply(3, rtk, bodies)


def project_points(bodies, rtk, body_index, points):
    """Body-fixed keypoints: point m = points[m] (M, 3) in the frame of body body_index[m] (M,) of bodies (..., K, 7), through rtk
    (..., 4, 4) -> pixels (..., M, 2) (``pd_pose_op`` PD_POSE_PROJECT_POINT).  Differentiable in bodies, rtk and points."""
    _check_cameras("project_points", bodies, rtk)
    if not (torch.is_tensor(body_index) and torch.is_tensor(points) and body_index.dim() == 1 and tuple(points.shape) == (body_index.numel(), 3)):
        raise ValueError("project_points: body_index (M,) and points (M, 3); got %s and %s" % (
            tuple(getattr(body_index, "shape", ())), tuple(getattr(points, "shape", ()))))
    _need_gpu("project_points", bodies, rtk, points)
    sel = bodies.index_select(-2, body_index.to(device=bodies.device, dtype=torch.long))
    return _PoseOpHip.apply(4, rtk, torch.cat([sel, points.expand(sel.shape[:-1] + (3,))], -1))


def reproj_loss(sim_2d, target_2d, rtk):
    """Mean pixel distance of the keypoints of each (env, frame) in units of the focal length: (..., K, 2) x 2, rtk (..., 4, 4) -> (...)
    -- the 2D term the reference leaves commented out (dp_model.py:781-792)."""
    return (sim_2d - target_2d).norm(2, -1).mean(-1) / rtk[..., 3, 0]


def _check_states(what, body_q, body_qd, nb):
    """body_q (..., nb, 7) and body_qd (..., nb, 6) with equal leading shapes, or a ValueError -> that leading shape."""
    if not (body_q.dim() >= 2 and tuple(body_q.shape[-2:]) == (nb, 7) and tuple(body_qd.shape[-2:]) == (nb, 6)
            and body_q.shape[:-2] == body_qd.shape[:-2]):
        raise ValueError("%s: body_q (..., %d, 7) and body_qd (..., %d, 6) with equal leading shapes; got %s and %s" % (
            what, nb, nb, tuple(body_q.shape), tuple(body_qd.shape)))
    return tuple(body_q.shape[:-2])


def _state_rows(body_q, body_qd, *more):
    """The operand rows of a state op, detached: [n, 13] = (p, q xyzw, w, v) from body_q (..., 7) and body_qd (..., 6), in their order;
    ``more`` = (body_mass (...), body_inertia (..., 3, 3)) appends the ten columns of the centroidal op's [n, 23] rows."""
    return torch.cat([t.detach().reshape(-1, w) for t, w in zip((body_q, body_qd) + more, (7, 6, 1, 9))], dim=1)


class _GroundWrenchHip(torch.autograd.Function):
    """The ground-contact wrench of body states as ONE HIP launch, its vector-Jacobian product as one more (``pd_pose_op`` /
    ``pd_pose_op_vjp``, PD_POSE_GROUND_WRENCH), the material gradient summed by ``pd_colsum``."""

    @staticmethod
    def forward(ctx, body_q, body_qd, materials, env):
        from . import hip_backend

        nb = int(env.nb)
        table = hip_backend.env_contact_table(env, body_q.device)
        nmat = hip_backend._table_tag(table)[1][2]
        if materials is not None:
            table = hip_backend.with_materials(table, nmat, materials)
        state = _state_rows(body_q, body_qd)
        ctx.table, ctx.nb, ctx.nmat = table, nb, nmat
        ctx.save_for_backward(state)
        return hip_backend.ground_wrench(table, nb, state).view(body_q.shape[:-1] + (6,))

    @staticmethod
    def backward(ctx, g):
        from . import hip_backend

        (state,) = ctx.saved_tensors
        need_state = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        g_s, g_m = hip_backend.ground_wrench_vjp(ctx.table, ctx.nb, ctx.nmat, state, g.to(torch.float32).contiguous().view(-1, 6),
                                                 need_state=need_state, need_materials=ctx.needs_input_grad[2])
        lead = g.shape[:-1]
        g_q = g_s[:, :7].reshape(lead + (7,)) if ctx.needs_input_grad[0] else None
        g_qd = g_s[:, 7:].reshape(lead + (6,)) if ctx.needs_input_grad[1] else None
        if g_m is not None:
            g_m = hip_backend.colsum(g_m.view(-1, ctx.nmat * 4)).view(ctx.nmat, 4)
        return g_q, g_qd, g_m, None


def ground_wrench(body_q, body_qd, env, materials=None):
    """Each body's ground-contact contribution to body_f (eval_body_contacts, integrator_euler.py:93-179 of the reference, as a function of
    the state): body_q (..., nb, 7) poses (p, q xyzw) and body_qd (..., nb, 6) twists in Warp order (w, v) -- wp_pos / wp_vel rows
    reshaped to (..., nb, .) -- -> (..., nb, 6) wrenches (torque, force), zeros for a body that touches nothing.  One HIP launch with the
    rollout kernels' own per-candidate arithmetic; differentiable in body_q, body_qd (raw partials; the quaternion entries are not
    projected) and in ``materials`` [nmat, 4] = (ke, kd, kf, mu) rows, a float32 GPU tensor that stands in for the env's rows.
    materials=None: the env's materials, no material gradient.  The differentiable ground-reaction force of a rollout frame is
    ``res_f[frame2step[f]] + ground_wrench(wp_pos[f], wp_vel[f], env)``.  float32 GPU tensors only."""
    _need_gpu("ground_wrench", body_q, body_qd, *(() if materials is None else (materials,)))
    _check_states("ground_wrench", body_q, body_qd, int(env.nb))
    return _GroundWrenchHip.apply(body_q, body_qd, materials, env)


def joint_coords(body_q, body_qd, env, rates="generalized"):
    """The joint coordinates of body states -- the inverse of forward kinematics (Warp's eval_ik): body_q (..., nb, 7) poses (p, q xyzw)
    and body_qd (..., nb, 6) twists in Warp order (w, v) -- wp_pos / wp_vel rows reshaped to (..., nb, .) -- -> (joint_q (..., nq),
    joint_qd (..., nqd)) in the layouts ``ForwardKinematics`` takes.  rates="generalized": the generalised velocities (FK of the result
    gives the state back); rates="measured": the rates a step's PD controller sees; they differ for COMPOUND joints only, and the
    generalised ones are singular at |second angle| = pi / 2.  One HIP launch (``dp_model.InverseKinematics``), differentiable in
    body_q and body_qd (raw partials; the quaternion entries are not projected).  float32 GPU tensors only."""
    from .dp_model import InverseKinematics

    _need_gpu("joint_coords", body_q, body_qd)
    nb = int(env.nb)
    lead = _check_states("joint_coords", body_q, body_qd, nb)
    q, qd = InverseKinematics.apply(body_q.reshape(-1, 1, nb, 7), body_qd.reshape(-1, 1, nb, 6), env, rates)
    return q.reshape(lead + (q.shape[-1],)), qd.reshape(lead + (qd.shape[-1],))


class CentroidalState(NamedTuple):
    """What :func:`centroidal` returns: views of one (..., 16) tensor."""
    mass: torch.Tensor              # (...)     M = sum m_i
    com: torch.Tensor               # (..., 3)  c = sum m_i x_i / M
    com_vel: torch.Tensor           # (..., 3)  c_dot = P / M
    momentum: torch.Tensor          # (..., 3)  P = sum m_i v_i
    angular_momentum: torch.Tensor  # (..., 3)  L about c
    kinetic: torch.Tensor           # (...)     T
    potential: torch.Tensor         # (...)     V = -sum m_i gravity . x_i


def centroidal(body_q, body_qd, body_mass, body_inertia, env):
    """The whole-body quantities of body states, per state set: body_q (..., nb, 7) poses (p, q xyzw) and body_qd (..., nb, 6) twists in
    Warp order (w, v; v the velocity of the body's centre of mass) -- wp_pos / wp_vel rows reshaped to (..., nb, .) --, body_mass
    broadcastable to (..., nb) and body_inertia (body frame, about the body's centre of mass: the rollouts' ``body_inertia``)
    broadcastable to (..., nb, 3, 3) -> :class:`CentroidalState` (mass, com, com_vel, momentum, angular_momentum about the centre of
    mass, kinetic, potential), views of one (..., 16) tensor.  The bodies' centres of mass and gravity are the env's.  One HIP launch
    (``dp_model.Centroidal``), differentiable in the first four arguments (raw partials; quaternions are taken as they are); shared
    masses are broadcast HERE, outside the Function, so autograd sums their gradient over the state sets.  float32 GPU tensors only."""
    from .dp_model import Centroidal

    _need_gpu("centroidal", body_q, body_qd, body_mass, body_inertia)
    nb = int(env.nb)
    lead = _check_states("centroidal", body_q, body_qd, nb)

    def fits(t, shape):
        try:
            return tuple(torch.broadcast_shapes(tuple(t.shape), shape)) == shape
        except RuntimeError:
            return False

    if not (fits(body_mass, lead + (nb,)) and fits(body_inertia, lead + (nb, 3, 3)) and tuple(body_inertia.shape[-2:]) == (3, 3)):
        raise ValueError("centroidal: body_mass must broadcast to %s and body_inertia to %s; got %s and %s" % (
            lead + (nb,), lead + (nb, 3, 3), tuple(body_mass.shape), tuple(body_inertia.shape)))
    out = Centroidal.apply(body_q, body_qd, body_mass.expand(lead + (nb,)), body_inertia.expand(lead + (nb, 3, 3)), env)
    return CentroidalState(out[..., 0], out[..., 1:4], out[..., 4:7], out[..., 7:10], out[..., 10:13], out[..., 13], out[..., 14])


class ContactState(NamedTuple):
    """What :func:`contact_state` returns, per body: views of one (..., nb, 8) tensor."""
    height: torch.Tensor     # (..., nb)     h of the lowest contact candidate c* (lowest index on ties); +inf for a body without candidates
    point_xz: torch.Tensor   # (..., nb, 2)  world (x, z) of c*
    velocity: torch.Tensor   # (..., nb, 3)  u = v + w x rr of c*, the velocity the contact model sees
    depth: torch.Tensor      # (..., nb)     s = sum of -h_c over the touching candidates (!(h_c > 0): the rollouts' touch decision)
    count: torch.Tensor      # (..., nb)     their number, as a float; carries no gradient


def contact_state(body_q, body_qd, env):
    """The ground-contact geometry of body states, per body: body_q (..., nb, 7) poses (p, q xyzw) and body_qd (..., nb, 6) twists in the
    rollouts' order (w, v) -- wp_pos / wp_vel rows reshaped to (..., nb, .), or ``ForwardKinematics``' outputs -- ->
    :class:`ContactState` (height, point_xz, velocity, depth, count).  Heights and the touch decision are the rollout kernels' own
    arithmetic on the env's contact candidates; every candidate of every body is swept.  One HIP launch
    (``dp_model.ContactState``), differentiable in body_q and body_qd (raw partials; quaternions are taken as they are): through the
    lowest candidate, and through the depth sum.  A body without candidates has height +inf and zeros elsewhere, and a zero gradient:
    :func:`penetration_loss` and :func:`skate_loss` mask such bodies out.  float32 GPU tensors only."""
    from .dp_model import ContactState as _ContactState

    _need_gpu("contact_state", body_q, body_qd)
    _check_states("contact_state", body_q, body_qd, int(env.nb))
    out = _ContactState.apply(body_q, body_qd, env)
    return ContactState(out[..., 0], out[..., 1:3], out[..., 3:6], out[..., 6], out[..., 7].detach())


def _contact_bodies(cs, bodies, *fields):
    """The chosen bodies' columns of ``fields`` with the bodies WITHOUT candidates (height +inf) replaced by zeros BEFORE any arithmetic
    (a select, not a product: inf * 0 never forms, in the value or in the gradient) -> (mask, fields..., number of bodies kept)."""
    pick = (lambda t: t) if bodies is None else (lambda t: t.index_select(cs.height.dim() - 1, torch.as_tensor(
        bodies, dtype=torch.long, device=cs.height.device).reshape(-1)))
    mask = pick(cs.height) != float("inf")
    out = []
    for f in fields:
        f = pick(f)
        out.append(torch.where(mask if f.dim() == mask.dim() else mask.unsqueeze(-1), f, torch.zeros((), dtype=f.dtype, device=f.device)))
    m = mask.to(cs.height.dtype).reshape(-1)
    return (mask,) + tuple(out) + (torch.dot(m, m).clamp(min=1.0),)


# (the sums below are dot products, like phys_model._mean_sq: torch's multi-block full reductions replay stale inside a captured HIP graph)
def penetration_loss(cs, bodies=None):
    """Ground-penetration term of a :class:`ContactState`: mean of depth^2 over the chosen bodies (``bodies``: indices along the body
    axis; None = all) that have contact candidates, over all leading dimensions.  depth = sum of -h_c over a body's touching
    candidates, so the term is zero -- with a zero gradient -- for states that touch nothing.  0 when no chosen body has candidates."""
    _, depth, kept = _contact_bodies(cs, bodies, cs.depth)
    d = depth.reshape(-1)
    return torch.dot(d, d) / kept


def skate_loss(cs, h0=0.02, bodies=None):
    """Foot-skate term of a :class:`ContactState`: mean over the chosen bodies that have contact candidates (and all leading dimensions) of
    clamp(1 - height / h0, 0, 1) * (velocity.x^2 + velocity.z^2) -- the horizontal speed of a body's lowest candidate, weighted 1 at and
    below the ground and falling linearly to 0 at height h0 (metres) above it."""
    _, height, vel, kept = _contact_bodies(cs, bodies, cs.height, cs.velocity)
    near = (1.0 - height / float(h0)).clamp(0.0, 1.0)
    return torch.dot(near.reshape(-1), (vel[..., 0] ** 2 + vel[..., 2] ** 2).reshape(-1)) / kept


def joint_wrench(body_q, body_qd, env, refs, target_ke, target_kd, torques=None):
    """What the joint pass of a step adds to each body's body_f (eval_body_joints, integrator_euler.py:289-451 of the reference, as a
    function of the state and the controls): the PD force, the limit force and the attachment springs of the body's own joint and of
    its children's.  body_q (..., nb, 7) poses (p, q xyzw) and body_qd (..., nb, 6) twists in Warp order (w, v) -- wp_pos / wp_vel rows
    reshaped to (..., nb, .) --; refs (the PD targets), target_ke, target_kd and torques broadcastable to (..., nqd) in the rollouts'
    dof layout (torques=None: zeros, no gradient) -> (..., nb, 6) wrenches (torque, force).  One HIP launch
    (``dp_model.JointWrench``), differentiable in every tensor argument (raw partials; quaternions are taken as they are); joint
    limits and attachment gains are the env's and carry no gradient.  The controls are gathered into the op's per-body dof slots and
    broadcast HERE, outside the Function, so autograd sums the gradient of a shared gain over the state sets.  The differentiable
    jaf of a rollout frame is ``joint_wrench(wp_pos[f], wp_vel[f], env, refs[s], target_ke, target_kd, torques[s])`` with
    ``s = frame2step[f]``.  float32 GPU tensors only."""
    from . import hip_backend
    from .dp_model import JointWrench

    controls = (refs, target_ke, target_kd) + (() if torques is None else (torques,))
    _need_gpu("joint_wrench", body_q, body_qd, *controls)
    nb = int(env.nb)
    lead = _check_states("joint_wrench", body_q, body_qd, nb)
    idx = hip_backend.env_joint_slot_index(env, body_q.device)
    nqd = int(env.template()["nqd"])

    def slots(t, name):
        try:
            ok = t.dim() >= 1 and tuple(torch.broadcast_shapes(tuple(t.shape), lead + (nqd,))) == lead + (nqd,)
        except RuntimeError:
            ok = False
        if not ok:
            raise ValueError("joint_wrench: %s must broadcast to %s; got %s" % (name, lead + (nqd,), tuple(t.shape)))
        # slot k of body b <- dof qd_start[b] + k, or the appended zero column
        t = t.expand(t.shape[:-1] + (nqd,))
        t = torch.cat([t, t.new_zeros(t.shape[:-1] + (1,))], dim=-1)
        return t.index_select(-1, idx).reshape(t.shape[:-1] + (nb, 3)).expand(lead + (nb, 3))

    tgt3, ke3, kd3 = slots(refs, "refs"), slots(target_ke, "target_ke"), slots(target_kd, "target_kd")
    act3 = body_q.new_zeros(lead + (nb, 3)) if torques is None else slots(torques, "torques")
    return JointWrench.apply(body_q, body_qd, act3, tgt3, ke3, kd3, env)


def generalized_force(body_q, body_f, env, efforts="actuator"):
    """The generalised joint forces of per-body wrenches -- the transpose of the articulation's Jacobian: body_q (..., nb, 7) poses
    (p, q xyzw; wp_pos rows reshaped to (..., nb, 7)) and body_f (..., nb, 6) wrenches (torque, force) in world axes, the force acting
    at the body's centre of mass -- a ``grf``, ``jaf`` or body_f row -- -> (..., nqd) in the joint_qd layout: for every REVOLUTE and
    COMPOUND dof the torque the wrenches on the joint's subtree exert about its axis, for a FREE joint (R_wj^-1 moment about the child
    body's centre of mass, R_wj^-1 force) of the net wrench on its subtree; FIXED joints have no entry.
    efforts="actuator": a COMPOUND joint's entries are the efforts jf_k with sum_k axis_k jf_k of the same projections -- the units of
    ``torques`` and of the PD force, conjugate to the measured rates of ``joint_coords``; singular at |second angle| = pi / 2.
    efforts="generalized": the bare projections, conjugate to the generalised rates.  The two differ for COMPOUND joints only.  The
    FREE entries are conjugate to the child body's twist (w, v), NOT to ``joint_coords``' FREE linear rate (which carries Warp's
    unrotated-com lever).  One HIP launch (``dp_model.GeneralizedForce``), differentiable in both tensors (raw partials; quaternions
    are taken as they are).  float32 GPU tensors only."""
    from .dp_model import GeneralizedForce

    _need_gpu("generalized_force", body_q, body_f)
    _check_states("generalized_force", body_q, body_f, int(env.nb))
    return GeneralizedForce.apply(body_q, body_f, env, efforts)


def _q_rot(q, v, inverse=False):
    """R(q) v, or R(q)^T v: the rollouts' form, x (2 w^2 - 1) +- 2 w (u x x) + 2 u (u . x) with q = (u, w)"""
    u, w = q[..., :3], q[..., 3:]
    c = 2.0 * w * torch.cross(u, v, dim=-1)
    return v * (2.0 * w * w - 1.0) + (-c if inverse else c) + 2.0 * u * (u * v).sum(-1, keepdim=True)


def inertial_wrench(body_q, body_qd, body_qd_next, dt, body_mass, body_inertia, env):
    """The total body_f (..., nb, 6) = (torque, force) for which one step of the rollouts' integrator (integrate_bodies,
    integrator_euler.py:21-91 of the reference) takes the twists body_qd (..., nb, 6) of the poses body_q (..., nb, 7) to body_qd_next,
    both in Warp order (w, v): the integrator solved for its force input --
        f = m ((v' - v) / dt - gravity [m != 0])
        t = R (I (R^T w' / (1 - 0.1 dt) - R^T w) / dt + R^T w x I R^T w),   R = R(q)
    with gravity on the bodies with mass, the gyroscopic term and the (1 - 0.1 dt) angular damping undone.  body_mass broadcastable to
    (..., nb), body_inertia (body frame, about the centre of mass: the rollouts' ``body_inertia``) to (..., nb, 3, 3); gravity is the
    env's.  EXACT (to rounding) where the step clamped neither w' nor v' at +-10, for unit quaternions and a body_inv_inertia that is
    the inverse of body_inertia; a clamped component has lost its force and comes back too small.  A body without mass gets force 0.
    Plain torch on the tensors' device and dtype, differentiable by autograd in every tensor argument."""
    nb = int(env.nb)
    _check_states("inertial_wrench", body_q, body_qd, nb)
    _check_states("inertial_wrench", body_q, body_qd_next, nb)
    gravity = torch.as_tensor([float(g) for g in env.template()["gravity"]], dtype=body_q.dtype, device=body_q.device)
    r0 = body_q[..., 3:]
    w0, v0, w1, v1 = body_qd[..., :3], body_qd[..., 3:], body_qd_next[..., :3], body_qd_next[..., 3:]
    mass = torch.as_tensor(body_mass, dtype=body_q.dtype, device=body_q.device)[..., None]
    inertia = torch.as_tensor(body_inertia, dtype=body_q.dtype, device=body_q.device)
    f = mass * ((v1 - v0) / dt - gravity * (mass != 0).to(body_q.dtype))
    wb = _q_rot(r0, w0, inverse=True)
    Iwb = (inertia @ wb[..., None])[..., 0]
    dwb = (_q_rot(r0, w1 / (1.0 - 0.1 * dt), inverse=True) - wb) / dt
    tb = (inertia @ dwb[..., None])[..., 0]
    t = _q_rot(r0, tb + torch.cross(wb, Iwb, dim=-1))
    return torch.cat([t, f.expand(t.shape)], -1)


def inverse_dynamics(body_q, body_qd, body_qd_next, dt, body_mass, body_inertia, env, external=None, efforts="actuator"):
    """The joint-space forces a motion needs: ``generalized_force(body_q, inertial_wrench(...) - external, env, efforts)`` -> (..., nqd).
    ``external`` (..., nb, 6): the wrenches something other than the joints supplies (a rollout's grf = res_f + ground_wrench(state));
    None: nothing, every body's whole inertial wrench is asked of the joints.
    SIGN: the entries are what the bodies RECEIVE, read in joint space.  A rollout's joint pass puts -axis * jf on the child body, so on
    a rollout's own states the REVOLUTE / COMPOUND entries are -jf (jf = PD force + ``torques`` - limit force: with zero gains, minus the
    applied torques), and the FREE entries are the residual wrench on the root that no joint and no ``external`` explains -- zero for
    a physical motion.  HIP (``generalized_force``): float32 GPU tensors only; differentiable in every tensor argument."""
    need = inertial_wrench(body_q, body_qd, body_qd_next, dt, body_mass, body_inertia, env)
    if external is not None:
        need = need - external
    return generalized_force(body_q, need.contiguous(), env, efforts)


def body_twists(body_q, joint_qd, env, rates="generalized"):
    """The rigid-body twists of joint rates -- the articulation's Jacobian applied to them, the conjugate of ``generalized_force``:
    body_q (..., nb, 7) poses (p, q xyzw) and joint_qd broadcastable to (..., nqd) in the joint_qd layout -> (..., nb, 6) twists in the
    rollouts' order (w, v), world axes, v the velocity of the body's centre of mass: what every body does when the joints move at
    those rates and the links are rigid.  ``ForwardKinematics``' velocities are NOT that (Warp's eval_fk leaves out the levers of the
    ancestors' angular velocities); these are what ``contact_state``, ``centroidal``, ``inertial_wrench`` and ``inverse_dynamics`` assume.
    rates="generalized" pairs with ``joint_coords(rates="generalized")`` and ``generalized_force(efforts="generalized")``,
    rates="measured" with ``joint_coords(rates="measured")`` and ``efforts="actuator"``; they differ for COMPOUND joints only.  In each
    pairing sum(generalized_force * joint_qd) = sum(body_f * body_twists).  A FREE joint's six entries are conjugate to
    ``generalized_force``'s FREE entries: (R_wj^-1 w, R_wj^-1 v) of what the joint adds to the child body's twist, v of its centre of
    mass -- NOT ``joint_coords``' FREE linear rate, which carries Warp's unrotated-com lever (``rigid_twists`` converts).  One HIP
    launch (``dp_model.BodyTwists``), differentiable in both tensors (raw partials; quaternions are taken as they are).  The rates are
    gathered into the op's per-body slots HERE, outside the Function, so autograd sums the gradient of a shared rate over the state
    sets.  float32 GPU tensors only."""
    from . import hip_backend
    from .dp_model import BodyTwists

    _need_gpu("body_twists", body_q, joint_qd)
    nb, nqd = int(env.nb), int(env.template()["nqd"])
    if not (body_q.dim() >= 2 and tuple(body_q.shape[-2:]) == (nb, 7)):
        raise ValueError("body_twists: body_q must be (..., %d, 7); got %s" % (nb, tuple(body_q.shape)))
    lead = tuple(body_q.shape[:-2])
    try:
        ok = joint_qd.dim() >= 1 and tuple(torch.broadcast_shapes(tuple(joint_qd.shape), lead + (nqd,))) == lead + (nqd,)
    except RuntimeError:
        ok = False
    if not ok:
        raise ValueError("body_twists: joint_qd must broadcast to %s; got %s" % (lead + (nqd,), tuple(joint_qd.shape)))
    hip_backend._jc_rate_mode(rates)
    return BodyTwists.apply(body_q, _rate_slots(joint_qd, lead, env, body_q.device), env, rates)


def _rate_slots(t, lead, env, device):
    """(..., nqd) in the joint_qd layout, broadcastable to lead + (nqd,) -> lead + (nb, 6): slot k of body b <- dof qd_start[b] + k, or
    the appended zero column.  Plain torch indexing, so autograd sums the gradient of a shared entry."""
    from . import hip_backend

    nb, nqd = int(env.nb), int(env.template()["nqd"])
    t = t.expand(t.shape[:-1] + (nqd,))
    t = torch.cat([t, t.new_zeros(t.shape[:-1] + (1,))], dim=-1)
    idx = hip_backend.env_joint_rate_slot_index(env, device)
    return t.index_select(-1, idx).reshape(t.shape[:-1] + (nb, 6)).expand(lead + (nb, 6))


def jacobian(body_q, env, rates="generalized"):
    """The articulation's Jacobian: body_q (..., nb, 7) -> (..., nb, 6, nqd), column j the twists (w, v of the centre of mass, world
    axes) of unit rate on dof j -- ``body_twists`` on the poses repeated nqd times against the identity, ONE launch of
    S * nqd * nb rows for S state sets (Laikago: 18 * 13 rows per set), so it is meant for a few sets, not for a batch of thousands.
    ``jacobian @ joint_qd`` is ``body_twists``; its transpose applied to wrenches is ``generalized_force`` of the paired convention.
    Differentiable in body_q.  float32 GPU tensors only."""
    _need_gpu("jacobian", body_q)
    nb, nqd = int(env.nb), int(env.template()["nqd"])
    if not (body_q.dim() >= 2 and tuple(body_q.shape[-2:]) == (nb, 7)):
        raise ValueError("jacobian: body_q must be (..., %d, 7); got %s" % (nb, tuple(body_q.shape)))
    lead = tuple(body_q.shape[:-2])
    eye = torch.eye(nqd, dtype=body_q.dtype, device=body_q.device)
    tw = body_twists(body_q.unsqueeze(-3).expand(lead + (nqd, nb, 7)), eye.expand(lead + (nqd, nqd)), env, rates)   # (..., nqd, nb, 6)
    return tw.permute(tuple(range(len(lead))) + (len(lead) + 1, len(lead) + 2, len(lead)))


def mass_matrix(body_q, body_mass, body_inertia, env, method="jacobian", rates="generalized"):
    """The joint-space mass matrix H = sum_b J_b^T diag(R_b I_b R_b^T, m_b 1) J_b: body_q (..., nb, 7), body_mass broadcastable to
    (..., nb), body_inertia (body frame, about the centre of mass) to (..., nb, 3, 3) -> (..., nqd, nqd), with qd^T H qd / 2 the
    kinetic energy of ``body_twists(body_q, qd, env, rates)``.
    method="jacobian" (the default): plain torch on ``jacobian(body_q, env, "generalized")`` -- its S * nqd * nb rows, so for a few
    state sets, not a batch of thousands --, the generalised rates only (rates="measured" raises ValueError); differentiable in every
    tensor argument.
    method="crba": the composite-rigid-body recursion as ONE HIP launch (``dp_model.MassMatrix``, ``pd_pose_op`` code 23), any batch
    size, either rate convention ("measured": the matrix whose inverse ``mass_inverse`` applies in that mode); exactly symmetric, exactly
    0 between dofs of unrelated bodies; the inertia is taken as symmetric.  Differentiable ONCE in all three tensors by a kernel of its
    own.  Masses and inertias are broadcast HERE, outside the Function, so autograd sums the gradient of a shared entry.  float32 GPU
    tensors only."""
    if method not in ("jacobian", "crba"):
        raise ValueError("mass_matrix: method must be \"jacobian\" or \"crba\"; got %r" % (method,))
    if rates not in ("generalized", "measured"):
        raise ValueError("mass_matrix: rates must be \"generalized\" or \"measured\"; got %r" % (rates,))
    if method == "crba":
        from .dp_model import MassMatrix

        _need_gpu("mass_matrix", body_q, body_mass, body_inertia)
        nb = int(env.nb)
        if not (body_q.dim() >= 2 and tuple(body_q.shape[-2:]) == (nb, 7)):
            raise ValueError("mass_matrix: body_q must be (..., %d, 7); got %s" % (nb, tuple(body_q.shape)))
        lead = tuple(body_q.shape[:-2])
        for name, t, tail in (("body_mass", body_mass, (nb,)), ("body_inertia", body_inertia, (nb, 3, 3))):
            try:
                ok = t.dim() >= len(tail) and tuple(torch.broadcast_shapes(tuple(t.shape), lead + tail)) == lead + tail
            except RuntimeError:
                ok = False
            if not ok:
                raise ValueError("mass_matrix: %s must broadcast to %s; got %s" % (name, lead + tail, tuple(t.shape)))
        return MassMatrix.apply(body_q, body_mass.expand(lead + (nb,)), body_inertia.expand(lead + (nb, 3, 3)), env, rates)
    if rates != "generalized":
        raise ValueError("mass_matrix: rates=\"measured\" is served by method=\"crba\" only; method=\"jacobian\" is the generalised rates'")
    J = jacobian(body_q, env, "generalized")
    mass = torch.as_tensor(body_mass, dtype=J.dtype, device=J.device)
    inertia = torch.as_tensor(body_inertia, dtype=J.dtype, device=J.device)
    Jw, Jv = J[..., :3, :], J[..., 3:, :]
    cols = Jw.transpose(-1, -2)
    A = _q_rot(body_q[..., None, 3:].expand(cols.shape[:-1] + (4,)), cols, inverse=True)   # (..., nb, nqd, 3): the angular columns in the body frame
    IA = A @ inertia.transpose(-1, -2)                                        # rows (I a)^T
    return (A @ IA.transpose(-1, -2)).sum(-3) + (mass[..., None, None] * (Jv.transpose(-1, -2) @ Jv)).sum(-3)


def _free_roots(tpl):
    """-> [(body, qd_start, the quaternion of joint_X_p)] of the template's FREE joints; ValueError if one of them has a parent."""
    import numpy as np

    nb = int(tpl["nb"])
    ty = np.asarray(tpl["joint_type"]).reshape(nb)
    par = np.asarray(tpl["joint_parent"]).reshape(nb)
    qds = np.asarray(tpl["joint_qd_start"]).reshape(-1)
    X_p = np.asarray(tpl["joint_X_p"], dtype=np.float32).reshape(nb, 7)
    free = [b for b in range(nb) if int(ty[b]) == 4]   # JOINT_FREE
    bad = [b for b in free if par[b] >= 0]
    if bad:
        raise ValueError("rigid_twists: the FREE joint of body %d has a parent (body %d); only FREE joints of the world are served" % (
            bad[0], par[bad[0]]))
    return [(b, int(qds[b]), X_p[b, 3:]) for b in free]


def rigid_twists(body_q, body_qd, env):
    """Body states whose twists may not be rigid -- ``ForwardKinematics``' outputs -- -> (..., nb, 6) rigid twists of the same joint
    rates: the hinge rates and the FREE angular rates of ``joint_coords(body_q, body_qd, env, "generalized")``, the FREE linear
    entries R_wj^-1 v of the FREE body's own twist, then ``body_twists``.  A rigid state (a rollout's) comes back unchanged to
    rounding; on FK states every angular part and the rows of the FREE roots are kept and the other linear parts are replaced by the
    rigid ones.  Robots whose FREE joints have no parent; ValueError otherwise.  Two HIP launches, differentiable in both tensors.
    float32 GPU tensors only."""
    from . import hip_backend

    free = _free_roots(env.template())
    _need_gpu("rigid_twists", body_q, body_qd)
    _check_states("rigid_twists", body_q, body_qd, int(env.nb))
    _, jqd = joint_coords(body_q, body_qd, env, "generalized")
    if free:
        # (the index and the joint frames live on the model: nothing is uploaded per call, so a captured iteration can hold the call)
        idx, quats = hip_backend._env_table(env, ("freeroots", str(body_q.device)), lambda tpl: (
            torch.as_tensor([s + 3 + k for _, s, _ in _free_roots(tpl) for k in range(3)], dtype=torch.long, device=body_q.device),
            torch.as_tensor([[float(x) for x in q] for _, _, q in _free_roots(tpl)], dtype=torch.float32, device=body_q.device)))
        lin = [_q_rot(quats[k].expand(body_qd.shape[:-2] + (4,)), body_qd[..., b, 3:], inverse=True) for k, (b, _, _) in enumerate(free)]
        jqd = jqd.index_copy(-1, idx, torch.cat(lin, dim=-1))
    return body_twists(body_q, jqd, env, "generalized")


EFFORTS_OF = {"generalized": "generalized", "measured": "actuator"}   # rate convention -> the conjugate efforts of generalized_force


def body_accelerations(body_q, body_qd, joint_qdd, env, rates="generalized"):
    """The accelerations of the bodies of a state -- J qdd + Jdot qd of the articulation, the second-order term next to ``body_twists``:
    body_q (..., nb, 7) poses, body_qd (..., nb, 6) twists (w, v of the centre of mass; a rollout's states as they are, or
    ``body_twists`` of joint rates) and joint_qdd broadcastable to (..., nqd), the time derivatives of the joint rates in the joint_qd
    layout -> (..., nb, 6) = (alpha, a) in world axes, a the acceleration of the body's centre of mass.  joint_qdd=None means zeros:
    the bias acceleration Jdot qd.  Every velocity-dependent term comes from the twists themselves (a body's and its parent's): no joint
    rates are passed, and on a state whose twists are not rigid the result is the op's formula (include/ppr_diffphys.h), not a time
    derivative of anything.  rates: the convention joint_qdd's COMPOUND entries are read in, as for ``body_twists``.  A FREE joint's six
    entries are the derivatives of ``body_twists``' FREE slots.  One HIP launch (``dp_model.BodyAccelerations``), differentiable in all
    three tensors (raw partials; quaternions are taken as they are).  joint_qdd is gathered into the op's per-body slots HERE, outside
    the Function, so autograd sums the gradient of a shared entry.  float32 GPU tensors only."""
    from . import hip_backend
    from .dp_model import BodyAccelerations

    _need_gpu("body_accelerations", body_q, body_qd, *(() if joint_qdd is None else (joint_qdd,)))
    nb, nqd = int(env.nb), int(env.template()["nqd"])
    lead = _check_states("body_accelerations", body_q, body_qd, nb)
    if joint_qdd is None:
        acc6 = body_q.new_zeros(lead + (nb, 6))
    else:
        try:
            ok = joint_qdd.dim() >= 1 and tuple(torch.broadcast_shapes(tuple(joint_qdd.shape), lead + (nqd,))) == lead + (nqd,)
        except RuntimeError:
            ok = False
        if not ok:
            raise ValueError("body_accelerations: joint_qdd must broadcast to %s; got %s" % (lead + (nqd,), tuple(joint_qdd.shape)))
    hip_backend._jc_rate_mode(rates)
    if joint_qdd is not None:
        acc6 = _rate_slots(joint_qdd, lead, env, body_q.device)
    return BodyAccelerations.apply(body_q, body_qd, acc6, env, rates)


def newton_euler_wrench(body_q, body_qd, body_acc, body_mass, body_inertia, env):
    """The total body_f (..., nb, 6) = (torque, force) that gives the bodies of a state the accelerations body_acc (..., nb, 6) =
    (alpha, a of the centre of mass) -- Newton and Euler per body:
        t = R (I R^T alpha + R^T w x I R^T w),   R = R(q)          f = m (a - gravity [m != 0])
    The continuous counterpart of ``inertial_wrench`` (which solves the rollouts' discrete step, with its (1 - 0.1 dt) angular damping,
    for the force): no time step and no damping here.  body_mass broadcastable to (..., nb), body_inertia (body frame, about the centre
    of mass) to (..., nb, 3, 3); gravity is the env's; a body without mass gets force 0.  Plain torch on the tensors' device and
    dtype, differentiable by autograd in every tensor argument."""
    nb = int(env.nb)
    _check_states("newton_euler_wrench", body_q, body_qd, nb)
    _check_states("newton_euler_wrench", body_q, body_acc, nb)
    gravity = torch.as_tensor([float(g) for g in env.template()["gravity"]], dtype=body_q.dtype, device=body_q.device)
    r0 = body_q[..., 3:]
    mass = torch.as_tensor(body_mass, dtype=body_q.dtype, device=body_q.device)[..., None]
    inertia = torch.as_tensor(body_inertia, dtype=body_q.dtype, device=body_q.device)
    f = mass * (body_acc[..., 3:] - gravity * (mass != 0).to(body_q.dtype))
    wb = _q_rot(r0, body_qd[..., :3], inverse=True)
    ab = _q_rot(r0, body_acc[..., :3], inverse=True)
    Iwb = (inertia @ wb[..., None])[..., 0]
    Iab = (inertia @ ab[..., None])[..., 0]
    t = _q_rot(r0, Iab + torch.cross(wb, Iwb, dim=-1))
    return torch.cat([t, f.expand(t.shape)], -1)


def rnea(body_q, joint_qd, joint_qdd, body_mass, body_inertia, env, external=None, rates="generalized"):
    """Inverse dynamics of a joint-space trajectory point (q as poses, qd, qdd) -- the recursive Newton-Euler algorithm on the state ops:
    ``body_twists(body_q, joint_qd)``, ``body_accelerations`` of those twists and joint_qdd, ``newton_euler_wrench`` - ``external``, and
    ``generalized_force`` with the efforts conjugate to ``rates`` (generalized <-> generalized, measured <-> actuator) -> (..., nqd) =
    H qdd + C(q, qd) qd + g - J^T external.  joint_qd and joint_qdd broadcastable to (..., nqd); joint_qdd=None means zeros.
    ``external`` (..., nb, 6): the wrenches something other than the joints supplies, as for ``inverse_dynamics``, whose SIGN convention
    this keeps: the entries are what the bodies RECEIVE, read in joint space.  Three HIP launches forward and three for the gradient;
    differentiable in every tensor argument.  float32 GPU tensors only."""
    from . import hip_backend

    hip_backend._jc_rate_mode(rates)
    tw = body_twists(body_q, joint_qd, env, rates)
    acc = body_accelerations(body_q, tw, joint_qdd, env, rates)
    need = newton_euler_wrench(body_q, tw, acc, body_mass, body_inertia, env)
    if external is not None:
        need = need - external
    return generalized_force(body_q, need.contiguous(), env, EFFORTS_OF[rates])


def bias_forces(body_q, joint_qd, body_mass, body_inertia, env, external=None, rates="generalized"):
    """C(q, qd) qd + g - J^T external: ``rnea`` with joint_qdd=None -> (..., nqd)."""
    return rnea(body_q, joint_qd, None, body_mass, body_inertia, env, external, rates)


def forward_dynamics(body_q, joint_qd, tau, body_mass, body_inertia, env, external=None, method="dense"):
    """The joint accelerations the joint-space forces tau (..., nqd) produce, in ``rnea``'s sign convention and the generalized rates:
    H^-1 (tau - ``bias_forces``) -> (..., nqd), so ``forward_dynamics(rnea(qdd)) = qdd``.
    method="dense" (the default): solve(``mass_matrix``, .), plain torch (a dense solve) on ``mass_matrix(method="jacobian")`` --
    S * nqd * nb rows through ``body_twists`` --: it is meant for a few state sets, not for a batch of thousands.
    method="crba": the same dense solve on ``mass_matrix(method="crba")``, H from one HIP launch at any batch size.
    method="articulated": ``mass_inverse`` of the same right-hand side, the articulated-body recursion in one HIP launch behind the
    three of ``bias_forces``: O(nb) per set, any batch size, once differentiable.  Differentiable in every tensor argument.  float32
    GPU tensors only (method="crba" on anything else: ValueError)."""
    if method not in ("dense", "articulated", "crba"):
        raise ValueError("forward_dynamics: method must be \"dense\", \"crba\" or \"articulated\"; got %r" % (method,))
    if method == "articulated":
        rhs = tau - bias_forces(body_q, joint_qd, body_mass, body_inertia, env, external, "generalized")
        return mass_inverse(body_q, rhs, body_mass, body_inertia, env, "generalized")
    if method == "crba":
        try:
            _need_gpu("forward_dynamics", body_q, joint_qd, tau, body_mass, body_inertia)
        except TypeError as e:   # the method is a HIP kernel and nothing else
            raise ValueError("forward_dynamics: method=\"crba\" is not available for these tensors -- %s" % (e,)) from None
        H = mass_matrix(body_q, body_mass, body_inertia, env, method="crba")
    else:
        H = mass_matrix(body_q, body_mass, body_inertia, env)
    rhs = tau - bias_forces(body_q, joint_qd, body_mass, body_inertia, env, external, "generalized")
    return torch.linalg.solve(H, rhs[..., None])[..., 0]


def mass_inverse(body_q, tau, body_mass, body_inertia, env, rates="generalized"):
    """H^-1 applied to a joint-space vector: body_q (..., nb, 7) poses, tau broadcastable to (..., nqd) in the joint_qd layout (the
    efforts conjugate to ``rates``), body_mass broadcastable to (..., nb), body_inertia (body frame, about the centre of mass; taken as
    symmetric) to (..., nb, 3, 3) -> (..., nqd) = the joint accelerations tau produces on the articulation at rest without gravity,
    H = sum_b J_b^T diag(R_b I_b R_b^T, m_b 1) J_b with J the Jacobian of ``body_twists`` in the same convention (rates="generalized":
    H is ``mass_matrix``).  The articulated-body recursion as ONE HIP launch (``dp_model.MassInverse``, ``pd_pose_op`` code 21), O(nb)
    per state set: the primitive of forward dynamics, impulse response and J H^-1 J^T at rollout batch sizes.  Differentiable ONCE in
    all four tensors; the gradient is composed from the same kernel and ``body_twists`` (three launches).  tau is gathered into the op's
    per-body slots and masses and inertias are broadcast HERE, outside the Function, so autograd sums the gradient of a shared entry.
    A singular H (a massless body on a joint with dofs) gives inf / NaN.  float32 GPU tensors only."""
    from . import hip_backend
    from .dp_model import MassInverse

    _need_gpu("mass_inverse", body_q, tau, body_mass, body_inertia)
    nb, nqd = int(env.nb), int(env.template()["nqd"])
    if not (body_q.dim() >= 2 and tuple(body_q.shape[-2:]) == (nb, 7)):
        raise ValueError("mass_inverse: body_q must be (..., %d, 7); got %s" % (nb, tuple(body_q.shape)))
    lead = tuple(body_q.shape[:-2])
    for name, t, tail in (("tau", tau, (nqd,)), ("body_mass", body_mass, (nb,)), ("body_inertia", body_inertia, (nb, 3, 3))):
        try:
            ok = t.dim() >= len(tail) and tuple(torch.broadcast_shapes(tuple(t.shape), lead + tail)) == lead + tail
        except RuntimeError:
            ok = False
        if not ok:
            raise ValueError("mass_inverse: %s must broadcast to %s; got %s" % (name, lead + tail, tuple(t.shape)))
    hip_backend._jc_rate_mode(rates)
    x6 = MassInverse.apply(body_q, body_mass.expand(lead + (nb,)), body_inertia.expand(lead + (nb, 3, 3)),
                           _rate_slots(tau, lead, env, body_q.device), env, rates)
    return x6.reshape(lead + (6 * nb,)).index_select(-1, hip_backend.env_joint_dof_slot_index(env, body_q.device))


def mass_matrix_inverse(body_q, body_mass, body_inertia, env):
    """H^-1 of the generalised rates, (..., nqd, nqd): ``mass_inverse`` on the identity -- nqd right-hand sides per state set, ONE
    launch of S * nqd * nb rows.  ``mass_matrix_inverse @ mass_matrix`` is the identity to rounding.  Differentiable once.  float32 GPU
    tensors only."""
    _need_gpu("mass_matrix_inverse", body_q, body_mass, body_inertia)
    nb, nqd = int(env.nb), int(env.template()["nqd"])
    if not (body_q.dim() >= 2 and tuple(body_q.shape[-2:]) == (nb, 7)):
        raise ValueError("mass_matrix_inverse: body_q must be (..., %d, 7); got %s" % (nb, tuple(body_q.shape)))
    lead = tuple(body_q.shape[:-2])
    eye = torch.eye(nqd, dtype=body_q.dtype, device=body_q.device)
    cols = mass_inverse(body_q.unsqueeze(-3).expand(lead + (nqd, nb, 7)), eye, body_mass.unsqueeze(-2) if body_mass.dim() > 1 else body_mass,
                        body_inertia.unsqueeze(-4) if body_inertia.dim() > 3 else body_inertia, env, "generalized")   # [..., j, :] = H^-1 e_j
    return cols.transpose(-1, -2)


def compute_com(body_q, part_com, part_mass):
    """mass-weighted COM of one articulation (numpy)   dp_utils.py:86-90"""
    from scipy.spatial.transform import Rotation as R

    c = (R.from_quat(body_q[:, 3:]).as_matrix() @ part_com)[..., 0] + body_q[:, :3]
    return (c * part_mass[:, None]).sum(0) / part_mass.sum()
