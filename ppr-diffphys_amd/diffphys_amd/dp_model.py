"""The two autograd boundaries of the reference, backed by the HIP library.

``ForwardWarp`` and ``ForwardKinematics`` keep the reference's names, argument
order, tensor layouts, side effects and gradient post-processing
(/root/reference/diffphys/dp_model.py:1022-1130 and :1145-1400) so that
``phys_model.forward`` can call them unchanged; see INTEGRATION.md.

Differences that are deliberate:
  * one kernel launch per rollout instead of a Python loop of Warp launches;
  * ``self.state_steps`` is not needed (the trajectory lives in a workspace
    tensor owned by the autograd ctx);
  * ``self.sim_trajs`` / ``body_q_numpy`` are lazy host views (:class:`HostFrames`): the env-0 copy the reference makes
    eagerly for visualisation happens on first access, so neither ``forward`` synchronises the host;
  * ``body_mass`` gets a zero gradient: the reference kernel loads it and never
    uses it (/root/reference/diffphys/integrator_euler.py:43).
"""
import numpy as np
import torch

from . import hip_backend
from .dp_utils import _need_gpu, _q_rot, _state_rows


def convert_ppr_warp(tensor):
    """[linear, angular] <=> [angular, linear] on the last axis (dp_model.py:1014-1019)."""
    return torch.cat([tensor[..., 3:6], tensor[..., 0:3], tensor[..., 6:]], -1)


class HostFrames:
    """Env-0 poses of every frame as a list of numpy arrays -- what the reference builds eagerly for visualisation
    (``self.sim_trajs`` dp_model.py:1237-1244, ``body_q_numpy`` :1066-1072) and ``query()`` consumes (:855-860).  Here the
    device-to-host copy happens on first access, so ``forward()`` itself never synchronises the host (SURVEY section 8(b):
    "no host sync inside the op except the optional env-0 trajectory copy")."""

    def __init__(self, frames_dev):  # [F, nb, 7] device tensor (a detached view; nothing writes it afterwards)
        self._dev, self._host = frames_dev.detach(), None

    def _get(self):
        if self._host is None:
            self._host = list(self._dev.detach().cpu().numpy())
            self._dev = None
        return self._host

    def __len__(self):
        return len(self._host) if self._host is not None else int(self._dev.shape[0])

    def __getitem__(self, i):
        return self._get()[i]

    def __iter__(self):
        return iter(self._get())


def _f32c(t):
    """detached, float32, contiguous -- without touching a tensor that already is (the usual case; three tensor ops saved per input).
    None stays None: an absent ``torques`` / ``res_f`` (all zeros; the library gets a NULL pointer and reads nothing for it)."""
    if t is None:
        return None
    t = t.detach()
    return t if (t.dtype is torch.float32 and t.is_contiguous()) else t.to(torch.float32).contiguous()


def _save_kw(ctx):
    """Nothing to differentiate (torch.no_grad(), or no input needs a gradient): the rollout runs forward-only -- no trajectory, no
    loss seeds are saved, the outputs are the same bits.  Otherwise the saving call, unchanged (no extra keyword: a backend object that
    predates the forward-only mode keeps working on the differentiable path)."""
    return {} if any(ctx.needs_input_grad) else {"save_trajectory": False}


class ForwardKinematics(torch.autograd.Function):
    """rj_q [T,bs,nq], rj_qd [T,bs,nqd], env -> body_q [bs,T,nb,7], body_qd [bs,T,nb,6], body_q_numpy."""

    @staticmethod
    def forward(ctx, rj_q, rj_qd, env):
        is_cuda = rj_q.is_cuda
        if not is_cuda:  # the reference moves CPU inputs to the GPU (dp_model.py:1030-1035)
            rj_q, rj_qd = rj_q.cuda(), rj_qd.cuda()
        num_frames, bs, _ = rj_q.shape
        dm = hip_backend.device_model(env)
        jq = rj_q.detach().to(torch.float32).contiguous()
        jqd = rj_qd.detach().to(torch.float32).contiguous()
        body_q, body_qd = dm.fk_forward(jq.view(num_frames * bs, -1), jqd.view(num_frames * bs, -1))
        ctx.dm, ctx.shape, ctx.is_cuda = dm, (num_frames, bs), is_cuda
        ctx.save_for_backward(jq, jqd)
        body_q = body_q.view(num_frames, bs, dm.nb, 7).permute(1, 0, 2, 3).contiguous()
        body_qd = body_qd.view(num_frames, bs, dm.nb, 6).permute(1, 0, 2, 3).contiguous()
        body_q_numpy = HostFrames(body_q[0])  # env 0, one array per frame (visualisation); copied to the host on first use
        if not is_cuda:
            body_q, body_qd = body_q.cpu(), body_qd.cpu()
        return body_q, body_qd, body_q_numpy

    @staticmethod
    def backward(ctx, adj_body_qs, adj_body_qd, _):
        jq, jqd = ctx.saved_tensors
        num_frames, bs = ctx.shape
        dm = ctx.dm
        aq = adj_body_qs.to(jq.device, torch.float32).permute(1, 0, 2, 3).contiguous()
        aqd = adj_body_qd.to(jq.device, torch.float32).permute(1, 0, 2, 3).contiguous()
        gq, gqd = dm.fk_backward(jq.view(num_frames * bs, -1), jqd.view(num_frames * bs, -1), aq, aqd)

        def post(g, last):  # the reference's post-processing (dp_model.py:1109-1110,1122-1123: NaN -> 0, values > 1 -> 1, upper
            g = g.view(num_frames, bs, last)  # clamp only) is applied by the kernel where it stores the gradients (pd_fk_backward)
            return g if ctx.is_cuda else g.cpu()

        return post(gq, dm.nq), post(gqd, dm.nqd), None


class InverseKinematics(torch.autograd.Function):
    """body_q [bs,T,nb,7], body_qd [bs,T,nb,6], env, rates -> rj_q [T,bs,nq], rj_qd [T,bs,nqd]: the joint coordinates of body states, the
    inverse of :class:`ForwardKinematics` in its own shapes (Warp's eval_ik; ``pd_pose_op`` PD_POSE_JOINT_COORDS, one launch forward and
    one for the vector-Jacobian product).  body_qd is in Warp order (w, v), as ForwardKinematics returns it and wp_vel holds it.
    rates="generalized": joint_qd are the generalised velocities (``ForwardKinematics.apply(*InverseKinematics.apply(bq, bqd, env),
    env)[:2]`` gives (bq, bqd) back, up to the gimbal lock of a compound joint at |second angle| = pi / 2); rates="measured": the
    rates the PD controller of a step sees (they differ for COMPOUND joints only).  float32 GPU tensors, or an error: no CPU
    fallback.  The gradients are the raw partials (quaternion entries not projected), nothing is scrubbed."""

    @staticmethod
    def forward(ctx, body_q, body_qd, env, rates="generalized"):
        nb = int(env.nb)
        _need_gpu("InverseKinematics", body_q, body_qd)
        if not (body_q.dim() == 4 and tuple(body_q.shape[2:]) == (nb, 7) and body_qd.dim() == 4 and tuple(body_qd.shape[2:]) == (nb, 6)
                and body_q.shape[:2] == body_qd.shape[:2]):
            raise ValueError("InverseKinematics: body_q [bs, T, %d, 7] and body_qd [bs, T, %d, 6]; got %s and %s" % (
                nb, nb, tuple(body_q.shape), tuple(body_qd.shape)))
        table = hip_backend.env_joint_table(env, body_q.device, rates)
        bs, T = int(body_q.shape[0]), int(body_q.shape[1])
        state = _state_rows(body_q.permute(1, 0, 2, 3), body_qd.permute(1, 0, 2, 3))
        ctx.table, ctx.nb, ctx.shape = table, nb, (bs, T)
        ctx.save_for_backward(state)
        q, qd = hip_backend.joint_coords(table, nb, state)
        return q.reshape(T, bs, -1), qd.reshape(T, bs, -1)

    @staticmethod
    def backward(ctx, g_q, g_qd):
        (state,) = ctx.saved_tensors
        bs, T = ctx.shape
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return None, None, None, None
        flat = lambda g: g.to(torch.float32).reshape(T * bs, -1).contiguous()
        g_s = hip_backend.joint_coords_vjp(ctx.table, ctx.nb, state, flat(g_q), flat(g_qd)).view(T, bs, ctx.nb, 13).permute(1, 0, 2, 3)
        return (g_s[..., :7] if ctx.needs_input_grad[0] else None), (g_s[..., 7:] if ctx.needs_input_grad[1] else None), None, None


class Centroidal(torch.autograd.Function):
    """body_q (..., nb, 7), body_qd (..., nb, 6) in Warp order (w, v), body_mass (..., nb), body_inertia (..., nb, 3, 3), env ->
    (..., 16) = (M, c, c_dot, P, L about c, T, V, 0) per state set: the whole-body quantities of body states (``pd_pose_op``
    PD_POSE_CENTROIDAL, one launch forward and one for the vector-Jacobian product).  All four tensors carry the SAME leading shape:
    broadcasting shared masses is the caller's (``dp_utils.centroidal`` does it with expand, so that autograd sums their gradient).
    float32 GPU tensors, or an error: no CPU fallback.  The gradients are the raw partials (quaternion entries not projected, no
    symmetry assumed for the inertia), nothing is scrubbed."""

    @staticmethod
    def forward(ctx, body_q, body_qd, body_mass, body_inertia, env):
        nb = int(env.nb)
        _need_gpu("Centroidal", body_q, body_qd, body_mass, body_inertia)
        lead = tuple(body_q.shape[:-2])
        if not (body_q.dim() >= 2 and tuple(body_q.shape) == lead + (nb, 7) and tuple(body_qd.shape) == lead + (nb, 6)
                and tuple(body_mass.shape) == lead + (nb,) and tuple(body_inertia.shape) == lead + (nb, 3, 3)):
            raise ValueError("Centroidal: body_q (..., %d, 7), body_qd (..., %d, 6), body_mass (..., %d) and body_inertia (..., %d, 3, 3) "
                             "with equal leading shapes; got %s, %s, %s and %s" % (
                                 nb, nb, nb, nb, tuple(body_q.shape), tuple(body_qd.shape), tuple(body_mass.shape), tuple(body_inertia.shape)))
        table = hip_backend.env_mass_table(env, body_q.device)
        rows = _state_rows(body_q, body_qd, body_mass, body_inertia)
        ctx.table, ctx.nb, ctx.lead = table, nb, lead
        ctx.save_for_backward(rows)
        return hip_backend.centroidal(table, nb, rows).view(lead + (16,))

    @staticmethod
    def backward(ctx, g):
        (rows,) = ctx.saved_tensors
        if not any(ctx.needs_input_grad[:4]):
            return None, None, None, None, None
        lead, nb = ctx.lead, ctx.nb
        g_r = hip_backend.centroidal_vjp(ctx.table, nb, rows, g.to(torch.float32).reshape(-1, 16).contiguous())
        need = ctx.needs_input_grad
        return (g_r[:, :7].reshape(lead + (nb, 7)) if need[0] else None, g_r[:, 7:13].reshape(lead + (nb, 6)) if need[1] else None,
                g_r[:, 13].reshape(lead + (nb,)) if need[2] else None, g_r[:, 14:].reshape(lead + (nb, 3, 3)) if need[3] else None, None)


class ContactState(torch.autograd.Function):
    """body_q (..., nb, 7), body_qd (..., nb, 6) in Warp order (w, v), env -> (..., nb, 8) = (h, x, z, u.xyz, s, k) per body: height,
    world (x, z) and velocity of its lowest contact candidate, the summed depth and the number of its touching candidates
    (``pd_pose_op`` PD_POSE_CONTACT_STATE on the env's contact table, one launch forward and one for the vector-Jacobian product); a
    body without candidates gives (+inf, 0, 0, 0, 0, 0, 0, 0).  float32 GPU tensors, or an error: no CPU fallback.  The gradients are
    the raw partials (quaternion entries not projected), nothing is scrubbed; the count k has none."""

    @staticmethod
    def forward(ctx, body_q, body_qd, env):
        nb = int(env.nb)
        _need_gpu("ContactState", body_q, body_qd)
        lead = tuple(body_q.shape[:-2])
        if not (body_q.dim() >= 2 and tuple(body_q.shape) == lead + (nb, 7) and tuple(body_qd.shape) == lead + (nb, 6)):
            raise ValueError("ContactState: body_q (..., %d, 7) and body_qd (..., %d, 6) with equal leading shapes; got %s and %s" % (
                nb, nb, tuple(body_q.shape), tuple(body_qd.shape)))
        table = hip_backend.env_contact_table(env, body_q.device)
        state = _state_rows(body_q, body_qd)
        ctx.table, ctx.nb, ctx.lead = table, nb, lead
        ctx.save_for_backward(state)
        return hip_backend.contact_state(table, nb, state).view(lead + (nb, 8))

    @staticmethod
    def backward(ctx, g):
        (state,) = ctx.saved_tensors
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return None, None, None
        lead, nb = ctx.lead, ctx.nb
        g_s = hip_backend.contact_state_vjp(ctx.table, nb, state, g.to(torch.float32).reshape(-1, 8).contiguous())
        return (g_s[:, :7].reshape(lead + (nb, 7)) if ctx.needs_input_grad[0] else None,
                g_s[:, 7:].reshape(lead + (nb, 6)) if ctx.needs_input_grad[1] else None, None)


class JointWrench(torch.autograd.Function):
    """body_q (..., nb, 7), body_qd (..., nb, 6) in Warp order (w, v), act3, target3, ke3, kd3 (..., nb, 3), env -> (..., nb, 6) =
    (torque, force) per body: what the joint pass of a step adds to body_f for that state and those controls -- the PD force, the
    limit force and the attachment springs of the body's own joint and of its children's (``pd_pose_op`` PD_POSE_JOINT_WRENCH on the
    env's joint-force table, one launch forward and one for the vector-Jacobian product).  The four control tensors hold each body's
    joint controls in dof slots 0..2 (a REVOLUTE joint reads slot 0, a COMPOUND joint all three, FIXED and FREE joints none: an unused
    slot may hold anything and gets a zero gradient) and carry the SAME leading shape as the states: gathering them from the
    rollout's dof layout and broadcasting shared gains is the caller's (``dp_utils.joint_wrench`` does both, so that autograd sums the
    gradient of a shared gain).  float32 GPU tensors, or an error: no CPU fallback.  The gradients are the raw partials (quaternion
    entries not projected), nothing is scrubbed; limits and attachment gains have none."""

    @staticmethod
    def forward(ctx, body_q, body_qd, act3, target3, ke3, kd3, env):
        nb = int(env.nb)
        _need_gpu("JointWrench", body_q, body_qd, act3, target3, ke3, kd3)
        lead = tuple(body_q.shape[:-2])
        if not (body_q.dim() >= 2 and tuple(body_q.shape) == lead + (nb, 7) and tuple(body_qd.shape) == lead + (nb, 6)
                and all(tuple(c.shape) == lead + (nb, 3) for c in (act3, target3, ke3, kd3))):
            raise ValueError("JointWrench: body_q (..., %d, 7), body_qd (..., %d, 6) and act3, target3, ke3, kd3 (..., %d, 3) with equal "
                             "leading shapes; got %s, %s and %s" % (nb, nb, nb, tuple(body_q.shape), tuple(body_qd.shape),
                                                                    [tuple(c.shape) for c in (act3, target3, ke3, kd3)]))
        table = hip_backend.env_joint_force_table(env, body_q.device)
        rows = torch.cat([t.detach().reshape(-1, w) for t, w in zip((body_q, body_qd, act3, target3, ke3, kd3), (7, 6, 3, 3, 3, 3))], dim=1)
        ctx.table, ctx.nb, ctx.lead = table, nb, lead
        ctx.save_for_backward(rows)
        return hip_backend.joint_wrench(table, nb, rows).view(lead + (nb, 6))

    @staticmethod
    def backward(ctx, g):
        (rows,) = ctx.saved_tensors
        need = ctx.needs_input_grad
        if not any(need[:6]):
            return (None,) * 7
        lead, nb = ctx.lead, ctx.nb
        g_r = hip_backend.joint_wrench_vjp(ctx.table, nb, rows, g.to(torch.float32).reshape(-1, 6).contiguous())
        cols = ((0, 7), (7, 13), (13, 16), (16, 19), (19, 22), (22, 25))
        return tuple(g_r[:, a:b].reshape(lead + (nb, b - a)) if need[k] else None for k, (a, b) in enumerate(cols)) + (None,)


class GeneralizedForce(torch.autograd.Function):
    """body_q (..., nb, 7), body_f (..., nb, 6) = (torque, force) per body in world axes, the force at the body's centre of mass -- a
    grf, jaf or body_f row --, env, efforts -> (..., nqd): the generalised joint forces those wrenches amount to, the transpose of the
    articulation's Jacobian (``pd_pose_op`` PD_POSE_GENERALIZED_FORCE on the env's joint table, one launch forward and one for the
    vector-Jacobian product): the torque about every REVOLUTE / COMPOUND axis, the net wrench on the subtree of a FREE joint, in the
    joint_qd layout.  efforts="actuator": COMPOUND entries in the units of ``torques`` and the PD force; "generalized": conjugate to the
    generalised rates.  float32 GPU tensors, or an error: no CPU fallback.  The gradients are the raw partials (quaternion entries
    not projected), nothing is scrubbed."""

    @staticmethod
    def forward(ctx, body_q, body_f, env, efforts="actuator"):
        nb = int(env.nb)
        _need_gpu("GeneralizedForce", body_q, body_f)
        lead = tuple(body_q.shape[:-2])
        if not (body_q.dim() >= 2 and tuple(body_q.shape) == lead + (nb, 7) and tuple(body_f.shape) == lead + (nb, 6)):
            raise ValueError("GeneralizedForce: body_q (..., %d, 7) and body_f (..., %d, 6) with equal leading shapes; got %s and %s" % (
                nb, nb, tuple(body_q.shape), tuple(body_f.shape)))
        table = hip_backend.env_joint_table(env, body_q.device, hip_backend.efforts_mode(efforts))
        rows = _state_rows(body_q, body_f)
        ctx.table, ctx.nb, ctx.lead = table, nb, lead
        ctx.save_for_backward(rows)
        out = hip_backend.generalized_force(table, nb, rows)
        return out.view(lead + (out.shape[-1],))

    @staticmethod
    def backward(ctx, g):
        (rows,) = ctx.saved_tensors
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return None, None, None, None
        lead, nb = ctx.lead, ctx.nb
        g_r = hip_backend.generalized_force_vjp(ctx.table, nb, rows, g.to(torch.float32).reshape(-1, g.shape[-1]).contiguous())
        return (g_r[:, :7].reshape(lead + (nb, 7)) if ctx.needs_input_grad[0] else None,
                g_r[:, 7:].reshape(lead + (nb, 6)) if ctx.needs_input_grad[1] else None, None, None)


class BodyTwists(torch.autograd.Function):
    """body_q (..., nb, 7), rates6 (..., nb, 6) = the rates of each body's joint in six slots (``hip_backend.joint_rate_slot_index``;
    a slot no dof uses may hold anything and gets a zero gradient), env, rates -> (..., nb, 6) = (w, v) per body in world axes, v of
    the body's centre of mass: the rigid twists those joint rates give, the articulation's Jacobian applied to them (``pd_pose_op``
    PD_POSE_BODY_TWIST on the env's joint table, one launch forward and one for the vector-Jacobian product).  rates="generalized" or
    "measured": the COMPOUND convention, that of ``joint_coords``.  Gathering the slots from the joint_qd layout is the caller's
    (``dp_utils.body_twists`` does it, so that autograd sums a shared rate's gradient).  float32 GPU tensors, or an error: no CPU
    fallback.  The gradients are the raw partials (quaternion entries not projected), nothing is scrubbed."""

    @staticmethod
    def forward(ctx, body_q, rates6, env, rates="generalized"):
        nb = int(env.nb)
        _need_gpu("BodyTwists", body_q, rates6)
        lead = tuple(body_q.shape[:-2])
        if not (body_q.dim() >= 2 and tuple(body_q.shape) == lead + (nb, 7) and tuple(rates6.shape) == lead + (nb, 6)):
            raise ValueError("BodyTwists: body_q (..., %d, 7) and rates6 (..., %d, 6) with equal leading shapes; got %s and %s" % (
                nb, nb, tuple(body_q.shape), tuple(rates6.shape)))
        table = hip_backend.env_joint_table(env, body_q.device, rates)
        rows = _state_rows(body_q, rates6)
        ctx.table, ctx.nb, ctx.lead = table, nb, lead
        ctx.save_for_backward(rows)
        return hip_backend.body_twists(table, nb, rows).view(lead + (nb, 6))

    @staticmethod
    def backward(ctx, g):
        (rows,) = ctx.saved_tensors
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return None, None, None, None
        lead, nb = ctx.lead, ctx.nb
        g_r = hip_backend.body_twists_vjp(ctx.table, nb, rows, g.to(torch.float32).reshape(-1, 6).contiguous())
        return (g_r[:, :7].reshape(lead + (nb, 7)) if ctx.needs_input_grad[0] else None,
                g_r[:, 7:].reshape(lead + (nb, 6)) if ctx.needs_input_grad[1] else None, None, None)


class BodyAccelerations(torch.autograd.Function):
    """body_q (..., nb, 7), body_qd (..., nb, 6) twists (w, v of the centre of mass), acc6 (..., nb, 6) = the time derivatives of the
    rates of each body's joint in six slots (``hip_backend.joint_rate_slot_index``; a slot no dof uses may hold anything and gets a zero
    gradient), env, rates -> (..., nb, 6) = (alpha, a) per body in world axes, a of the body's centre of mass: J qdd + Jdot qd of the
    articulation on that state (``pd_pose_op`` PD_POSE_BODY_ACCEL on the env's joint table, one launch forward and one for the
    vector-Jacobian product).  rates="generalized" or "measured": the COMPOUND convention the slots are read in, that of
    ``joint_coords``.  Gathering the slots from the joint_qd layout is the caller's (``dp_utils.body_accelerations`` does it).  float32
    GPU tensors, or an error: no CPU fallback.  The gradients are the raw partials (quaternion entries not projected)."""

    @staticmethod
    def forward(ctx, body_q, body_qd, acc6, env, rates="generalized"):
        nb = int(env.nb)
        _need_gpu("BodyAccelerations", body_q, body_qd, acc6)
        lead = tuple(body_q.shape[:-2])
        if not (body_q.dim() >= 2 and tuple(body_q.shape) == lead + (nb, 7) and tuple(body_qd.shape) == lead + (nb, 6)
                and tuple(acc6.shape) == lead + (nb, 6)):
            raise ValueError("BodyAccelerations: body_q (..., %d, 7), body_qd and acc6 (..., %d, 6) with equal leading shapes; got %s, %s and %s" % (
                nb, nb, tuple(body_q.shape), tuple(body_qd.shape), tuple(acc6.shape)))
        table = hip_backend.env_joint_table(env, body_q.device, rates)
        rows = torch.cat([t.detach().reshape(-1, w) for t, w in ((body_q, 7), (body_qd, 6), (acc6, 6))], dim=1)
        ctx.table, ctx.nb, ctx.lead = table, nb, lead
        ctx.save_for_backward(rows)
        return hip_backend.body_accelerations(table, nb, rows).view(lead + (nb, 6))

    @staticmethod
    def backward(ctx, g):
        (rows,) = ctx.saved_tensors
        if not any(ctx.needs_input_grad[:3]):
            return None, None, None, None, None
        lead, nb = ctx.lead, ctx.nb
        g_r = hip_backend.body_accelerations_vjp(ctx.table, nb, rows, g.to(torch.float32).reshape(-1, 6).contiguous())
        return (g_r[:, :7].reshape(lead + (nb, 7)) if ctx.needs_input_grad[0] else None,
                g_r[:, 7:13].reshape(lead + (nb, 6)) if ctx.needs_input_grad[1] else None,
                g_r[:, 13:].reshape(lead + (nb, 6)) if ctx.needs_input_grad[2] else None, None, None)


def _twist_form_partials(q, m, inertia, tx, tl):
    """The partials of E = -sum_b tl_b . diag(R(q_b) sym(I_b) R(q_b)^T, m_b 1) . tx_b, the pairing of two twist fields [n, 6] = (w, v)
    through the bodies' inertias, in closed form: q [n, 4] xyzw (raw partials: R is ``_q_rot``'s polynomial), m [n, 1], inertia
    [n, 3, 3] -> (g_tx [n, 6], g_tl [n, 6], g_q [n, 4], g_m [n, 1], g_inertia [n, 3, 3]).  Plain torch on any device and dtype."""
    sym = 0.5 * (inertia + inertia.transpose(-1, -2))
    a, b = _q_rot(q, tl[:, :3], inverse=True), _q_rot(q, tx[:, :3], inverse=True)
    Ia, Ib = (sym * a[:, None, :]).sum(-1), (sym * b[:, None, :]).sum(-1)   # (elementwise: a batched 3 x 3 matmul costs milliseconds here)
    g_m = -(tl[:, 3:] * tx[:, 3:]).sum(-1, keepdim=True)
    g_i = -0.5 * (a[:, :, None] * b[:, None, :] + b[:, :, None] * a[:, None, :])
    g_tx = -torch.cat([_q_rot(q, Ia), m * tl[:, 3:]], dim=-1)
    g_tl = -torch.cat([_q_rot(q, Ib), m * tx[:, 3:]], dim=-1)
    u, w = q[:, :3], q[:, 3:]
    g_q = 0
    for v, g in ((tl[:, :3], -Ib), (tx[:, :3], -Ia)):   # the adjoint of R(q)^T v in q: v (2 w^2 - 1) - 2 w (u x v) + 2 u (u . v)
        uv, gu, gv = (u * v).sum(-1, keepdim=True), (g * u).sum(-1, keepdim=True), (g * v).sum(-1, keepdim=True)
        g_u = -2.0 * w * torch.cross(v, g, dim=-1) + 2.0 * (uv * g + gu * v)
        g_w = 4.0 * w * gv - 2.0 * (g * torch.cross(u, v, dim=-1)).sum(-1, keepdim=True)
        g_q = g_q + torch.cat([g_u, g_w], dim=-1)
    return g_tx, g_tl, g_q, g_m, g_i


class MassInverse(torch.autograd.Function):
    """body_q (..., nb, 7), body_mass (..., nb), body_inertia (..., nb, 3, 3) (body frame, about the centre of mass; its symmetric part
    enters), r6 (..., nb, 6) = the joint-space force entries of each body's joint in six slots (``hip_backend.joint_rate_slot_index``;
    a slot no dof uses may hold anything and gets a zero gradient), env, rates -> (..., nb, 6) = x = H^-1 r in the same slots, 0 where
    no dof is: H = J^T M J the articulation's mass matrix in the rate convention ``rates`` (``pd_pose_op`` PD_POSE_MASS_INVERSE on the
    env's joint table: the articulated-body recursion, one launch).  All four tensors carry the full leading shape; gathering the slots
    and broadcasting masses and inertias is the caller's (``dp_utils.mass_inverse`` does both, so that autograd sums shared ones).

    The gradient is COMPOSED, there is no adjoint kernel: H is symmetric, so with lam = H^-1 g (the same kernel once more) the slot
    gradient is lam, and the gradient in poses, masses and inertias is that of -sum_b tlam_b . M_b(q_b, m_b, I_b) . tx_b with
    tx = body_twists(body_q, x), tlam = body_twists(body_q, lam), x and lam held constant: one launch of op 17 on the 2 S stacked sets,
    one of its VJP, and M_b's partials in closed form in plain torch (``_twist_form_partials``).  When r6 alone needs a gradient only the first launch runs.  ONCE differentiable: backward
    works on detached tensors, a second derivative is not available.  float32 GPU tensors, or an error: no CPU fallback.  Raw partials
    (quaternion entries not projected)."""

    @staticmethod
    def forward(ctx, body_q, body_mass, body_inertia, r6, env, rates="generalized"):
        nb = int(env.nb)
        _need_gpu("MassInverse", body_q, body_mass, body_inertia, r6)
        lead = tuple(body_q.shape[:-2])
        if not (body_q.dim() >= 2 and tuple(body_q.shape) == lead + (nb, 7) and tuple(body_mass.shape) == lead + (nb,)
                and tuple(body_inertia.shape) == lead + (nb, 3, 3) and tuple(r6.shape) == lead + (nb, 6)):
            raise ValueError("MassInverse: body_q (..., %d, 7), body_mass (..., %d), body_inertia (..., %d, 3, 3) and r6 (..., %d, 6) with equal "
                             "leading shapes; got %s, %s, %s and %s" % (nb, nb, nb, nb, tuple(body_q.shape), tuple(body_mass.shape),
                                                                        tuple(body_inertia.shape), tuple(r6.shape)))
        table = hip_backend.env_joint_table(env, body_q.device, rates)
        rows = torch.cat([t.detach().reshape(-1, w) for t, w in ((body_q, 7), (body_mass, 1), (body_inertia, 9), (r6, 6))], dim=1)
        out = hip_backend.mass_inverse(table, nb, rows)
        ctx.table, ctx.nb, ctx.lead = table, nb, lead
        ctx.save_for_backward(rows, out)
        return out.view(lead + (nb, 6))

    @staticmethod
    def backward(ctx, g):
        rows, x = ctx.saved_tensors
        if not any(ctx.needs_input_grad[:4]):
            return None, None, None, None, None, None
        lead, nb, n = ctx.lead, ctx.nb, rows.shape[0]
        lam = hip_backend.mass_inverse(ctx.table, nb, torch.cat([rows[:, :17], g.to(torch.float32).reshape(-1, 6)], dim=1))
        g_r = lam.reshape(lead + (nb, 6)) if ctx.needs_input_grad[3] else None
        if not any(ctx.needs_input_grad[:3]):
            return None, None, None, g_r, None, None
        pose = rows[:, :7]
        rows13 = torch.cat([torch.cat([pose, x], dim=1), torch.cat([pose, lam], dim=1)], dim=0)
        tw = hip_backend.body_twists(ctx.table, nb, rows13)
        g_tx, g_tl, g_q, g_m, g_i = _twist_form_partials(rows[:, 3:7], rows[:, 7:8], rows[:, 8:17].reshape(n, 3, 3), tw[:n], tw[n:])
        g_tw = torch.cat([g_tx, g_tl], dim=0)
        g_body_q = None
        if ctx.needs_input_grad[0]:
            g13 = hip_backend.body_twists_vjp(ctx.table, nb, rows13, g_tw.contiguous())
            g_pose = g13[:n, :7] + g13[n:, :7]
            g_pose[:, 3:] += g_q
            g_body_q = g_pose.reshape(lead + (nb, 7))
        return (g_body_q, g_m.reshape(lead + (nb,)) if ctx.needs_input_grad[1] else None,
                g_i.reshape(lead + (nb, 3, 3)) if ctx.needs_input_grad[2] else None, g_r, None, None)


class MassMatrix(torch.autograd.Function):
    """body_q (..., nb, 7), body_mass (..., nb), body_inertia (..., nb, 3, 3) (body frame, about the centre of mass; its symmetric part
    enters), env, rates -> (..., nqd, nqd) = H = J^T M J, the joint-space mass matrix of the articulation in the rate convention
    ``rates``, in the joint_qd layout (``pd_pose_op`` PD_POSE_MASS_MATRIX on the env's joint table: the composite-rigid-body recursion,
    one launch forward and one for the vector-Jacobian product, a kernel of its own that takes any upstream gradient, symmetric or
    not).  All three tensors carry the full leading shape; broadcasting masses and inertias is the caller's (``dp_utils.mass_matrix``
    does it, so that autograd sums shared ones).  ONCE differentiable.  float32 GPU tensors, or an error: no CPU fallback.  Raw
    partials (quaternion entries not projected; the inertia's are those of its symmetric part)."""

    @staticmethod
    def forward(ctx, body_q, body_mass, body_inertia, env, rates="generalized"):
        nb = int(env.nb)
        _need_gpu("MassMatrix", body_q, body_mass, body_inertia)
        lead = tuple(body_q.shape[:-2])
        if not (body_q.dim() >= 2 and tuple(body_q.shape) == lead + (nb, 7) and tuple(body_mass.shape) == lead + (nb,)
                and tuple(body_inertia.shape) == lead + (nb, 3, 3)):
            raise ValueError("MassMatrix: body_q (..., %d, 7), body_mass (..., %d) and body_inertia (..., %d, 3, 3) with equal leading "
                             "shapes; got %s, %s and %s" % (nb, nb, nb, tuple(body_q.shape), tuple(body_mass.shape), tuple(body_inertia.shape)))
        table = hip_backend.env_joint_table(env, body_q.device, rates)
        rows = torch.cat([t.detach().reshape(-1, w) for t, w in ((body_q, 7), (body_mass, 1), (body_inertia, 9))], dim=1)
        out = hip_backend.mass_matrix(table, nb, rows)
        ctx.table, ctx.nb, ctx.lead = table, nb, lead
        ctx.save_for_backward(rows)
        return out.view(lead + tuple(out.shape[1:]))

    @staticmethod
    def backward(ctx, g):
        (rows,) = ctx.saved_tensors
        if not any(ctx.needs_input_grad[:3]):
            return None, None, None, None, None
        lead, nb = ctx.lead, ctx.nb
        nqd = int(g.shape[-1])
        g_r = hip_backend.mass_matrix_vjp(ctx.table, nb, rows, g.to(torch.float32).reshape(-1, nqd, nqd).contiguous())
        return (g_r[:, :7].reshape(lead + (nb, 7)) if ctx.needs_input_grad[0] else None,
                g_r[:, 7].reshape(lead + (nb,)) if ctx.needs_input_grad[1] else None,
                g_r[:, 8:].reshape(lead + (nb, 3, 3)) if ctx.needs_input_grad[2] else None, None, None)


def checkpoint_plan(nsteps, frame2step, K):
    """The launches of a checkpointed rollout adjoint: ``nsteps`` steps cut into segments of ``K`` (the last one shorter when K does not
    divide nsteps).  Pure; -> (launch_frames, segments).

    launch_frames: the frame list of the ONE forward-only launch -- the caller's ``frame2step`` in its order, then the boundary steps
    K, 2K, ... (< nsteps) that are not frames already: no step twice, so the library's validation passes.

    segments: one (start, end, local_frame2step, caller_indices, has_carry) per segment, first to last; the backward walks it in reverse.
    The segment is the rollout of steps [start, end) from state ``start``.  ``caller_indices`` are the positions in ``frame2step`` of the
    frames it seeds -- those with start <= step < end, and step == nsteps in the last segment -- and ``local_frame2step`` their steps
    relative to ``start``, in the caller's order; with ``has_carry`` (every segment but the last) one more local frame follows, at
    state end - start, whose seed is the state adjoint handed back by the segment after.  A caller frame ON a boundary step belongs to
    the later segment, as its state 0: it is seeded once.  K >= nsteps gives one segment, the caller's own call."""
    nsteps, K = int(nsteps), int(K)
    frames = [int(s) for s in frame2step]
    if K < 1:
        raise ValueError("checkpoint_plan: K = %d, a segment has at least one step" % K)
    if nsteps < 0 or any(s < 0 or s > nsteps for s in frames) or len(set(frames)) != len(frames):
        raise ValueError("checkpoint_plan: frame2step must hold distinct steps in 0..%d" % nsteps)
    have = set(frames)
    launch_frames = frames + [b for b in range(K, nsteps, K) if b not in have]
    segments = []
    for start in range(0, max(nsteps, 1), K):
        end = min(start + K, nsteps)
        has_carry = end < nsteps
        idx = [i for i, s in enumerate(frames) if start <= s < end or (not has_carry and s == end)]
        local = [frames[i] - start for i in idx] + ([end - start] if has_carry else [])
        segments.append((start, end, local, idx, has_carry))
    return launch_frames, segments


def checkpoint_steps_for(nsteps, bytes_per_step, bytes_per_boundary, budget_bytes):
    """The largest segment length K in 1..nsteps whose checkpointed adjoint fits ``budget_bytes``: a K-step workspace
    (K x bytes_per_step; ``4 * dm.workspace_floats(bs, 1)``) plus ceil(nsteps / K) boundary states (bytes_per_boundary each;
    ``4 * 13 * bs * nb``).  Pure.  ValueError, naming the shortfall, when no K fits -- K = 1 included."""
    nsteps = int(nsteps)
    if nsteps < 1:
        raise ValueError("checkpoint_steps_for: nsteps = %d, nothing to segment" % nsteps)
    need = lambda K: K * int(bytes_per_step) + -(-nsteps // K) * int(bytes_per_boundary)
    for K in range(nsteps, 0, -1):
        if need(K) <= budget_bytes:
            return K
    best = min(range(1, nsteps + 1), key=need)
    raise ValueError("checkpoint_steps_for: %d bytes short -- K = 1 needs %d bytes, the cheapest segment length (K = %d) needs %d, the budget is %d"
                     % (need(best) - budget_bytes, need(1), best, need(best), budget_bytes))


def _remove_nan(g):
    """remove_nan of the boundary (NaN -> 0, +-inf kept) as a torch op: for the one gradient the adjoint kernel hands back raw."""
    return torch.where(g != g, torch.zeros_like(g), g)


def grads_wanted(needs_input_grad):
    """The ``want=`` of the adjoint launch from an autograd ctx's ``needs_input_grad``: of the per-step gradients (torques, res_f, refs --
    inputs 2, 3, 4 of ForwardWarp, ForwardWarpState, ForwardWarpTrajLoss and ForwardWarpTrajLossFK alike) those whose input needs one.
    The rest are neither allocated nor computed, and the Function returns None for them."""
    return tuple(n for n, i in (("torques", 2), ("res_f", 3), ("refs", 4)) if needs_input_grad[i])


def _want_kw(ctx):
    """The ``want=`` keyword of the adjoint call -- absent when all three per-step gradients are needed: the call is then the one it
    always was (as _save_kw: a backend object that predates the selective adjoint keeps working where every input needs a gradient)."""
    want = grads_wanted(ctx.needs_input_grad)
    return {} if len(want) == len(hip_backend.GRAD_NAMES) else {"want": want}


def _view(g, name, like):
    """a per-step gradient shaped as its input, or None when it was not asked for"""
    return g[name].view_as(like) if name in g else None


def _publish(self, dm, frame2step, nsteps, wp_pos, grf, jaf, wp_vel=None):
    """The side outputs on ``self`` that phys_model.query() consumes (dp_model.py:855-860).  A frame at state `nsteps` has no force
    snapshot in the reference (:1225-1228 append for step in steps_idx only): keep its list lengths.  ``sim_vels``: env 0's frame twists
    beside ``sim_trajs`` (query(joint_coords=True) needs both halves of the state)."""
    has_f = [f for f, s in enumerate(frame2step) if s < nsteps]
    self.grfs = [grf[f] for f in has_f]
    self.jafs = [jaf[f] for f in has_f]
    self.sim_trajs = HostFrames(wp_pos[:, : dm.nb])
    self.sim_vels = None if wp_vel is None else HostFrames(wp_vel[:, : dm.nb])


def _grad_tuple(g, init, torques, res_f, refs, inertia, inv_inertia, mass_shape, device):
    """The gradients of the eleven rollout inputs in ForwardWarp's order.  init: those of the first two inputs; a per-step gradient that
    was not asked for is None; body_mass gets zeros (the module docstring)."""
    return init + (_view(g, "torques", torques), _view(g, "res_f", res_f), _view(g, "refs", refs), g["target_ke"], g["target_kd"],
                   torch.zeros(mass_shape, dtype=torch.float32, device=device), g["body_inv_mass"],
                   g["body_inertia"].view_as(inertia), g["body_inv_inertia"].view_as(inv_inertia))


_SUMMED = ("target_ke", "target_kd", "body_inv_mass", "body_inertia", "body_inv_inertia")  # gradients that are sums over the steps


def _checkpoint_forward(dm, bs, nsteps, dt, inp, frame2step, K):
    """Forward of the checkpointed ForwardWarp: ONE forward-only launch whose frames are the caller's plus the segment boundaries.
    -> the caller's (wp_pos, wp_vel, grf, jaf), and the boundary states [segments - 1, bs*nb, 13] kept for the backward."""
    launch_frames, segments = checkpoint_plan(nsteps, frame2step, K)
    F = len(frame2step)
    pos, vel, grf, jaf, _ = dm.rollout_forward(bs, nsteps, dt, *inp, frame2step=launch_frames, save_trajectory=False)
    row = {s: f for f, s in enumerate(launch_frames)}
    states = torch.empty(len(segments) - 1, bs * dm.nb, 13, dtype=torch.float32, device=pos.device)
    for j, seg in enumerate(segments[1:]):
        states[j, :, :7] = pos[row[seg[0]]]
        states[j, :, 7:] = vel[row[seg[0]]]
    if len(launch_frames) > F:  # the caller's frames as tensors of their own: the boundary rows are not kept alive behind them
        pos, vel, grf, jaf = pos[:F].clone(), vel[:F].clone(), grf[:F].clone(), jaf[:F].clone()
    return pos, vel, grf, jaf, states


def _checkpoint_backward(dm, bs, nsteps, dt, inp, frame2step, K, states, adj_pos, adj_vel, want=hip_backend.GRAD_NAMES):
    """Backward of the checkpointed ForwardWarp -> the gradient dict of DeviceModel.rollout_backward.  Segments last to first: a saving
    forward of the segment from its boundary state into the one K-step workspace, then its adjoint, seeded with the caller's seeds
    inside the segment and the state adjoint carried from the segment after (raw).  No host synchronisation.  want: the per-step
    gradients to compute -- only they get their full [T] tensor, whose step slices the segments' selective launches fill."""
    q_init, qd_init, torques, res_f, refs, ke, kd, inv_m, inertia, inv_inertia = inp
    _, segments = checkpoint_plan(nsteps, frame2step, K)
    dev, N = refs.device, bs * dm.nb
    want = hip_backend.grad_want(want)
    g = dm._alloc_grads(bs, nsteps, dev, want=want)
    tmp = {k: torch.empty_like(g[k]) for k in _SUMMED}
    ws = torch.empty(dm.workspace_floats(bs, min(K, nsteps)), dtype=torch.float32, device=dev)
    carry = torch.empty(N, 13, dtype=torch.float32, device=dev) if len(segments) > 1 else None
    none7, none6 = torch.empty(0, N, 7, dtype=torch.float32, device=dev), torch.empty(0, N, 6, dtype=torch.float32, device=dev)
    for i in range(len(segments) - 1, -1, -1):
        start, end, local, idx, has_carry = segments[i]
        n = end - start
        seg_ws = ws[: dm.workspace_floats(bs, n)]
        ctl = tuple(None if t is None else t[start:end] for t in (torques, res_f, refs))  # (an absent control: nothing to slice)
        init = dict(state0=states[i - 1]) if i > 0 else {}
        q0 = (None, None) if i > 0 else (q_init, qd_init)
        dm.rollout_forward(bs, n, dt, *q0, *ctl, ke, kd, inv_m, inertia, inv_inertia, frame2step=[], want_forces=False,
                           out=dict(ws=seg_ws, wp_pos=none7, wp_vel=none6), **init)
        contiguous = idx == list(range(idx[0], idx[0] + len(idx))) if idx else True
        if not has_carry and contiguous:
            sp, sv = (adj_pos[idx[0]: idx[0] + len(idx)], adj_vel[idx[0]: idx[0] + len(idx)]) if idx else (none7, none6)
        else:
            sp = torch.cat([adj_pos[j: j + 1] for j in idx] + ([carry[None, :, :7]] if has_carry else []))
            sv = torch.cat([adj_vel[j: j + 1] for j in idx] + ([carry[None, :, 7:]] if has_carry else []))
        first = i == len(segments) - 1  # the first segment processed writes the sums' accumulators themselves
        gs = {k: (g[k] if first else tmp[k]) for k in _SUMMED}
        gs.update({k: g[k][start:end] for k in want})
        if i > 0:
            gs["state0"] = carry
        else:
            gs.update(q_init=g["q_init"], qd_init=g["qd_init"])
        dm.rollout_backward(bs, n, dt, *q0, ctl[0], ctl[2], ke, kd, inv_m, inertia, inv_inertia, local, seg_ws, sp, sv,
                            out=dict(grads=gs), want=want, **init)
        if not first:
            for k in _SUMMED:
                g[k].add_(tmp[k])
    return g


class ForwardWarp(torch.autograd.Function):
    """ForwardWarp.apply(q_init, qd_init, torques, res_f, refs, target_ke, target_kd, body_mass,
    body_inv_mass, body_inertia, body_inv_inertia, self) -> (wp_pos [F,bs*nb,7], wp_vel [F,bs*nb,6]).

    ``torques`` and ``res_f`` may each be None -- "all zeros", here and in ForwardWarpState / ForwardWarpTrajLoss / ForwardWarpTrajLossFK:
    nothing is allocated or read for an absent one, outputs and gradients are those of the call with zero tensors bit for bit, and the
    gradient returned for its position is None.

    Read from ``self``: ``env``, ``steps_idx``, ``frame2step``, ``dt``, ``num_envs``; optionally ``checkpoint_steps``.
    Written to ``self``: ``grfs``, ``jafs`` (lists of F tensors [bs*nb,6]), ``sim_trajs`` (F numpy [nb,7], env 0).

    ``self.checkpoint_steps = K`` (absent, None, 0 or K >= nsteps: the single-launch path, unchanged) selects the CHECKPOINTED adjoint
    when a gradient is wanted: the forward is one forward-only launch that also emits the states at steps K, 2K, ...; the backward
    re-runs one K-step segment at a time, last to first, into one K-step workspace and carries the state adjoint from segment to segment
    (:func:`checkpoint_plan`).  Memory: K instead of nsteps steps of workspace, plus 52 bytes per body per boundary.  Outputs, per-step
    gradients (torques, res_f, refs) and the q_init / qd_init gradients are the single launch's bits; the five gradients that are sums
    over the steps (target_ke, target_kd, body_inv_mass, body_inertia, body_inv_inertia) are added up per segment, last segment first,
    in fp32 -- a re-associated sum.  NaN policy, a stated difference: each segment scrubs what it stores (NaN -> 0) and the carried
    adjoint is raw, so an env whose adjoint turns NaN gets zero per-step gradients in every earlier segment, as in the single launch;
    but what the segments processed BEFORE the NaN arose added to the five sums stays there, where the single launch returns 0."""

    @staticmethod
    def forward(ctx, q_init, qd_init, torques, res_f, refs, target_ke, target_kd, body_mass, body_inv_mass, body_inertia,
                body_inv_inertia, self):
        env = self.env
        dm = hip_backend.device_model(env)
        bs = int(self.num_envs)
        nsteps = len(self.steps_idx)
        frame2step = list(self.frame2step)
        dev = q_init.device
        c = _f32c
        inp = [c(t) for t in (q_init, qd_init, torques, res_f, refs, target_ke, target_kd, body_inv_mass, body_inertia,
                              body_inv_inertia)]
        frame2step = [int(s) for s in frame2step]
        K = int(getattr(self, "checkpoint_steps", None) or 0)
        ctx.checkpoint = K if (0 < K < nsteps and any(ctx.needs_input_grad)) else 0
        if ctx.checkpoint:
            wp_pos, wp_vel, grf, jaf, ws = _checkpoint_forward(dm, bs, nsteps, float(self.dt), inp, frame2step, K)  # (ws: the boundary states)
        else:
            wp_pos, wp_vel, grf, jaf, ws = dm.rollout_forward(bs, nsteps, self.dt, *inp, frame2step=frame2step, **_save_kw(ctx))
        ctx.dm, ctx.meta = dm, (bs, nsteps, float(self.dt), frame2step)
        ctx.save_for_backward(ws, *inp)
        ctx.mass_shape = body_mass.shape
        _publish(self, dm, frame2step, nsteps, wp_pos, grf, jaf, wp_vel)
        return wp_pos, wp_vel

    @staticmethod
    def backward(ctx, adj_body_qs, adj_body_qd):
        ws, q_init, qd_init, torques, res_f, refs, ke, kd, inv_m, inertia, inv_inertia = ctx.saved_tensors
        bs, nsteps, dt, frame2step = ctx.meta
        want = _want_kw(ctx)  # per-step gradients nobody asked for are not allocated, computed or stored
        if ctx.checkpoint:
            g = _checkpoint_backward(ctx.dm, bs, nsteps, dt, (q_init, qd_init, torques, res_f, refs, ke, kd, inv_m, inertia, inv_inertia),
                                     frame2step, ctx.checkpoint, ws, adj_body_qs.to(torch.float32).contiguous(),
                                     adj_body_qd.to(torch.float32).contiguous(), **want)
        else:
            g = ctx.dm.rollout_backward(bs, nsteps, dt, q_init, qd_init, torques, refs, ke, kd, inv_m, inertia, inv_inertia,
                                        frame2step, ws, adj_body_qs.to(torch.float32).contiguous(),
                                        adj_body_qd.to(torch.float32).contiguous(), **want)
        # remove_nan (dp_model.py:1294-1384: NaN -> 0 on every returned gradient, inf kept) is applied by the adjoint kernel where it
        # stores the gradients (pd_rollout_backward): no pass over the tensors here
        return _grad_tuple(g, (g["q_init"], g["qd_init"]), torques, res_f, refs, inertia, inv_inertia, ctx.mass_shape, refs.device) + (None,)


_MATERIAL_CHUNK_BYTES = 64 << 20  # per-element material gradients of one step chunk of ForwardWarpContact.backward


def material_gradient(dm, table, nmat, ws, bs, nsteps, g_res_f):
    """d loss / d shape_materials [nmat, 4] of a rollout from what its launches left: the saved states (workspace ``ws``) and the adjoint's
    g_res_f [T, bs*nb, 6], which is the adjoint of body_f.  The contact wrench of step t is a function G of state t and the materials
    alone and enters body_f additively, so the gradient is sum_t <g_res_f[t], dG(state_t, materials)/dmaterials>: the ground-wrench
    VJP on the saved states in chunks of steps (temporaries bounded whatever T), each chunk's elements summed by ``colsum`` into a row,
    the rows by one more ``colsum`` -- fixed order throughout.  Raw: the caller applies the boundary's remove_nan."""
    N = bs * dm.nb
    body_q, body_qd, _, _ = dm.saved_trajectory(ws, bs, nsteps)
    per = max(1, _MATERIAL_CHUNK_BYTES // max(1, N * nmat * 16))
    rows = []
    for t0 in range(0, nsteps, per):
        t1 = min(nsteps, t0 + per)
        state = torch.cat([body_q[t0:t1], body_qd[t0:t1]], dim=-1).view(-1, 13)
        _, g_m = hip_backend.ground_wrench_vjp(table, dm.nb, nmat, state, g_res_f[t0:t1].reshape(-1, 6), need_state=False)
        rows.append(hip_backend.colsum(g_m.view(-1, nmat * 4)))
    if not rows:
        return torch.zeros(nmat, 4, dtype=torch.float32, device=ws.device)
    return (rows[0] if len(rows) == 1 else hip_backend.colsum(torch.stack(rows))).view(nmat, 4)


class ForwardWarpContact(torch.autograd.Function):
    """ForwardWarp with the ground-contact materials as a twelfth, differentiable input (contact system identification):

        wp_pos, wp_vel = ForwardWarpContact.apply(<the 11 inputs of ForwardWarp>, shape_materials [nmat, 4], self)

    shape_materials holds the rows (ke, kd, kf, mu) of ``self.env``'s materials.  Outputs, side outputs on ``self`` and the eleven other
    gradients are ForwardWarp's.
    Forward: the rows are read to the host ONCE -- a synchronising copy of 4 nmat floats -- and, when they differ from the env's,
    ``env.set_shape_materials`` installs them: the device model is then rebuilt (a materials update costs a model build; the C ABI has
    no entry that re-binds them).  Because of both, the call raises under stream capture.  Then the saving rollout, unchanged.
    Backward: the adjoint launch with g_res_f asked for (dropped afterwards when res_f itself needs no gradient), then
    :func:`material_gradient` -- the ground-wrench op's VJP over the saved trajectory, fully parallel over steps -- and the boundary's
    remove_nan.  No rollout kernel knows about materials.
    ``self.checkpoint_steps`` set: raises -- the checkpointed adjoint keeps no full trajectory; accumulating per segment is not built."""

    @staticmethod
    def forward(ctx, q_init, qd_init, torques, res_f, refs, target_ke, target_kd, body_mass, body_inv_mass, body_inertia,
                body_inv_inertia, shape_materials, self):
        if int(getattr(self, "checkpoint_steps", None) or 0):
            raise NotImplementedError("ForwardWarpContact: checkpoint_steps is set -- the material gradient needs the whole saved trajectory; "
                                      "unset it (segment-wise accumulation is not implemented)")
        if not (torch.is_tensor(shape_materials) and shape_materials.is_cuda):
            raise TypeError("ForwardWarpContact: shape_materials must be a GPU tensor [nmat, 4]")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ForwardWarpContact cannot be captured: it reads shape_materials to the host and may rebuild the device model")
        env = self.env
        M = shape_materials.detach().to(torch.float32).cpu().numpy()  # the one synchronising copy: 4 nmat floats
        if M.shape != tuple(np.shape(env.t_shape_materials)) or not np.array_equal(M, env.t_shape_materials):
            env.set_shape_materials(M)
        dm = hip_backend.device_model(env)
        bs, nsteps = int(self.num_envs), len(self.steps_idx)
        frame2step = [int(s) for s in self.frame2step]
        c = _f32c
        inp = [c(t) for t in (q_init, qd_init, torques, res_f, refs, target_ke, target_kd, body_inv_mass, body_inertia,
                              body_inv_inertia)]
        wp_pos, wp_vel, grf, jaf, ws = dm.rollout_forward(bs, nsteps, self.dt, *inp, frame2step=frame2step, **_save_kw(ctx))
        ctx.dm, ctx.meta = dm, (bs, nsteps, float(self.dt), frame2step)
        # the table of THIS call's materials: a later set_shape_materials on the env does not reach a pending backward
        ctx.table = hip_backend.env_contact_table(env, wp_pos.device) if ctx.needs_input_grad[11] else None
        ctx.nmat = int(M.shape[0])
        ctx.save_for_backward(ws, *inp)
        ctx.mass_shape = body_mass.shape
        _publish(self, dm, frame2step, nsteps, wp_pos, grf, jaf, wp_vel)
        return wp_pos, wp_vel

    @staticmethod
    def backward(ctx, adj_body_qs, adj_body_qd):
        ws, q_init, qd_init, torques, res_f, refs, ke, kd, inv_m, inertia, inv_inertia = ctx.saved_tensors
        bs, nsteps, dt, frame2step = ctx.meta
        asked = grads_wanted(ctx.needs_input_grad)
        need_m = ctx.needs_input_grad[11]
        want = hip_backend.grad_want(asked + (("res_f",) if need_m else ()))
        g = ctx.dm.rollout_backward(bs, nsteps, dt, q_init, qd_init, torques, refs, ke, kd, inv_m, inertia, inv_inertia, frame2step, ws,
                                    adj_body_qs.to(torch.float32).contiguous(), adj_body_qd.to(torch.float32).contiguous(), want=want)
        g_m = None
        if need_m:
            g_m = _remove_nan(material_gradient(ctx.dm, ctx.table, ctx.nmat, ws, bs, nsteps, g["res_f"]))
            if "res_f" not in asked:
                g = {k: v for k, v in g.items() if k != "res_f"}
        return _grad_tuple(g, (g["q_init"], g["qd_init"]), torques, res_f, refs, inertia, inv_inertia, ctx.mass_shape, refs.device) + (g_m, None)


class ForwardWarpState(torch.autograd.Function):
    """ForwardWarp started from a BODY state instead of joint coordinates:

        wp_pos, wp_vel = ForwardWarpState.apply(body_q0 [bs*nb,7], body_qd0 [bs*nb,6], torques, res_f, refs, target_ke, target_kd,
                                                body_mass, body_inv_mass, body_inertia, body_inv_inertia, self)

    State 0 is (body_q0, body_qd0) as given -- the rows of a frame's wp_pos / wp_vel; no FK, no re-normalisation -- so a window whose
    inputs are the ``wp_pos[-1]`` / ``wp_vel[-1]`` of the window before (its frame at state nsteps) continues that rollout bit for
    bit, and ordinary autograd chains the windows' adjoints.  Reads and writes ``self`` as ForwardWarp (``checkpoint_steps`` is not
    read); forward-only when nothing needs a gradient.  The gradients of body_q0 / body_qd0 leave the kernel raw and get the
    boundary's remove_nan (NaN -> 0, +-inf kept) here, by a torch op on those two small tensors."""

    @staticmethod
    def forward(ctx, body_q0, body_qd0, torques, res_f, refs, target_ke, target_kd, body_mass, body_inv_mass, body_inertia,
                body_inv_inertia, self):
        dm = hip_backend.device_model(self.env)
        bs, nsteps = int(self.num_envs), len(self.steps_idx)
        frame2step = [int(s) for s in self.frame2step]
        c = _f32c
        state0 = torch.cat([c(body_q0).reshape(-1, 7), c(body_qd0).reshape(-1, 6)], dim=1)
        inp = [c(t) for t in (torques, res_f, refs, target_ke, target_kd, body_inv_mass, body_inertia, body_inv_inertia)]
        wp_pos, wp_vel, grf, jaf, ws = dm.rollout_forward(bs, nsteps, self.dt, None, None, *inp, frame2step=frame2step, state0=state0,
                                                          **_save_kw(ctx))
        ctx.dm, ctx.meta = dm, (bs, nsteps, float(self.dt), frame2step)
        ctx.save_for_backward(ws, state0, *inp)
        ctx.mass_shape, ctx.q0_shape, ctx.qd0_shape = body_mass.shape, body_q0.shape, body_qd0.shape
        _publish(self, dm, frame2step, nsteps, wp_pos, grf, jaf, wp_vel)
        return wp_pos, wp_vel

    @staticmethod
    def backward(ctx, adj_body_qs, adj_body_qd):
        ws, state0, torques, res_f, refs, ke, kd, inv_m, inertia, inv_inertia = ctx.saved_tensors
        bs, nsteps, dt, frame2step = ctx.meta
        g = ctx.dm.rollout_backward(bs, nsteps, dt, None, None, torques, refs, ke, kd, inv_m, inertia, inv_inertia, frame2step, ws,
                                    adj_body_qs.to(torch.float32).contiguous(), adj_body_qd.to(torch.float32).contiguous(), state0=state0,
                                    **_want_kw(ctx))
        g0 = _remove_nan(g["state0"])
        init = (g0[:, :7].reshape(ctx.q0_shape), g0[:, 7:].reshape(ctx.qd0_shape))
        return _grad_tuple(g, init, torques, res_f, refs, inertia, inv_inertia, ctx.mass_shape, refs.device) + (None,)


class ForwardWarpTrajLoss(torch.autograd.Function):
    """ForwardWarp with the one loss term that back-propagates through the rollout evaluated INSIDE it (SURVEY section 8 row f4;
    reference: dp_model.py:733-779 -- ForwardWarp.apply, then loss_traj = reduce_loss(se3_loss(sim_position, target_position).mean(-1)
    with outseq entries zeroed, clip=True); pos_state / vel_state / distill use sim_position.detach(), :795,802):

        loss_traj, wp_pos, wp_vel = ForwardWarpTrajLoss.apply(<the 11 inputs of ForwardWarp>, target_position [bs,F,nb,7],
                                                              outseq_idx [bs,F] bool, self)

    loss_traj is the reduced scalar; wp_pos / wp_vel come back DETACHED (non-differentiable outputs: what the other loss terms and
    query() consume) -- unless ``self.differentiable_states`` is True (opt-in, read like ``checkpoint_steps``): then they are differentiable
    outputs, and what a further term (dp_utils.reproj_loss on project_bodies(wp_pos), say) sends back to them is added to the adjoint's own
    seeds (adj_pos / adj_vel of ``pd_rollout_backward_traj_loss``): the gradients are those of that library call, bit for bit.
    Forward = ONE rollout launch that also evaluates se3_loss and its gradients at the frame states + one
    one-workgroup launch for reduce_loss; backward = a few-microsecond launch that builds the seeds from what the forward left, scaled
    by the upstream gradient of loss_traj read on the device, then the adjoint rollout launch -- no pose, seed or per-frame loss goes
    through a torch op in between.
    Side outputs on ``self`` as ForwardWarp, plus ``self.traj_loss_info`` = (loss, clip threshold, positives left, clipped envs)."""

    @staticmethod
    def forward(ctx, q_init, qd_init, torques, res_f, refs, target_ke, target_kd, body_mass, body_inv_mass, body_inertia,
                body_inv_inertia, target_position, outseq_idx, self):
        return _traj_loss_forward(ctx, (q_init, qd_init, torques, res_f, refs, target_ke, target_kd, body_mass, body_inv_mass, body_inertia,
                                        body_inv_inertia), target_position, outseq_idx, self, None)

    @staticmethod
    def backward(ctx, g_loss, _gp, _gv):
        return _traj_loss_backward(ctx, g_loss, None, (_gp, _gv)) + (None,)


class ForwardWarpTrajLossFK(torch.autograd.Function):
    """ForwardWarpTrajLoss plus the FK of the control reference (dp_model.py:758 of the reference:
    ``ForwardKinematics.apply(queried_q, queried_qd, self.env)``) in the SAME launches -- the second half of SURVEY section 8 row f4:

        loss_traj, wp_pos, wp_vel, queried_position [bs,F,nb,7], queried_velocity [bs,F,nb,6], pid_ref =
            ForwardWarpTrajLossFK.apply(<the 11 inputs of ForwardWarp>, target_position, outseq_idx, queried_q [F,bs,nq], queried_qd [F,bs,nqd], self)

    The FK chains are extra workgroups of the reduce_loss launch that follows the rollout launch, their adjoint (with
    ForwardKinematics.backward's NaN -> 0 / > 1 -> 1 post-processing) extra workgroups of the seeds launch in front of the adjoint
    rollout; the kernels write / read the [bs, F, ...] layout directly (the reference permutes and copies, :1093-1094).  Values and
    gradients are those of ForwardKinematics.apply bit for bit (same device code)."""

    @staticmethod
    def forward(ctx, q_init, qd_init, torques, res_f, refs, target_ke, target_kd, body_mass, body_inv_mass, body_inertia,
                body_inv_inertia, target_position, outseq_idx, queried_q, queried_qd, self):
        return _traj_loss_forward(ctx, (q_init, qd_init, torques, res_f, refs, target_ke, target_kd, body_mass, body_inv_mass, body_inertia,
                                        body_inv_inertia), target_position, outseq_idx, self, (queried_q, queried_qd))

    @staticmethod
    def backward(ctx, g_loss, _gp, _gv, g_qpos, g_qvel, _pid):
        g = _traj_loss_backward(ctx, g_loss, (g_qpos, g_qvel), (_gp, _gv))
        return g[:13] + g[13:] + (None,)


def _traj_loss_forward(ctx, rollout_inputs, target_position, outseq_idx, self, queried):
    (q_init, qd_init, torques, res_f, refs, target_ke, target_kd, body_mass, body_inv_mass, body_inertia, body_inv_inertia) = rollout_inputs
    dm = hip_backend.device_model(self.env)
    bs, nsteps = int(self.num_envs), len(self.steps_idx)
    frame2step = [int(s) for s in self.frame2step]
    c = _f32c
    inp = [c(t) for t in (q_init, qd_init, torques, res_f, refs, target_ke, target_kd, body_inv_mass, body_inertia,
                          body_inv_inertia)]
    tgt = c(target_position).view(bs, len(frame2step), dm.nb, 7)
    outseq = None if outseq_idx is None else outseq_idx.detach().to(torch.bool).contiguous()
    need_gt = target_position.requires_grad
    fk = None if queried is None else (c(queried[0]), c(queried[1]))
    wp_pos, wp_vel, grf, jaf, ws, tl = dm.rollout_forward_traj_loss(bs, nsteps, self.dt, *inp, frame2step=frame2step, target_pos=tgt,
                                                                    outseq=outseq, rot_ratio=0.1, want_seed_gt=need_gt, fk=fk, **_save_kw(ctx))
    # What the backward needs of tl -- WITHOUT the Function's outputs: an output kept on ctx closes the cycle ctx -> tensor -> grad_fn ->
    # ctx through C++ references that Python's collector cannot see, and every iteration would then pin its buffers for good (ADVICE r4:
    # ~30 MB per iteration at 4096 envs).  The FK outputs' shapes are all the backward wants of them.
    ctx.dm, ctx.meta = dm, (bs, nsteps, float(self.dt), frame2step)
    ctx.tl = {k: v for k, v in tl.items() if k not in ("fk_body_q", "fk_body_qd", "reduced")}
    ctx.fk_shapes = None if fk is None else (tuple(tl["fk_body_q"].shape), tuple(tl["fk_body_qd"].shape))
    ctx.save_for_backward(ws, *inp, *(fk or ()))
    ctx.mass_shape, ctx.tgt_shape = body_mass.shape, target_position.shape
    _publish(self, dm, frame2step, nsteps, wp_pos, grf, jaf, wp_vel)
    self.traj_loss_info = tl["reduced"]
    # self.differentiable_states (absent / False: the states come back detached, as they always did): wp_pos / wp_vel are differentiable
    # outputs and their incoming gradients join the adjoint's own seeds (_traj_loss_backward).  Gradients nobody sent stay None then.
    ctx.diff_states = bool(getattr(self, "differentiable_states", False))
    if ctx.diff_states:
        ctx.set_materialize_grads(False)
    else:
        ctx.mark_non_differentiable(wp_pos, wp_vel)
    out = (tl["reduced"][0].clone(), wp_pos, wp_vel)
    if fk is not None:
        body_q, body_qd = tl["fk_body_q"], tl["fk_body_qd"]
        out += (body_q, body_qd, HostFrames(body_q[0]))  # env 0, one array per frame (visualisation), as ForwardKinematics
    return out


def _traj_loss_backward(ctx, g_loss, g_queried, g_states):
    ws, q_init, qd_init, torques, res_f, refs, ke, kd, inv_m, inertia, inv_inertia = ctx.saved_tensors[:11]
    bs, nsteps, dt, frame2step = ctx.meta
    tl = ctx.tl
    adj = {}
    if ctx.diff_states:
        gp, gv = g_states
        if gp is not None or gv is not None:  # the entry wants both or neither: an absent one is zeros
            n = len(frame2step) * bs * ctx.dm.nb
            z = lambda k: torch.zeros(n * k, dtype=torch.float32, device=ws.device)
            adj = dict(adj_pos=z(7) if gp is None else gp.detach().to(torch.float32).contiguous(),
                       adj_vel=z(6) if gv is None else gv.detach().to(torch.float32).contiguous())
        if g_loss is None:  # only the states were used
            g_loss = torch.zeros(1, dtype=torch.float32, device=ws.device)
    gl = g_loss.detach().to(torch.float32).reshape(1).contiguous()
    fk = None
    if g_queried is not None and (g_queried[0] is not None or g_queried[1] is not None):
        jq, jqd = ctx.saved_tensors[11:13]
        z = lambda sh: torch.zeros(sh, dtype=torch.float32, device=ws.device)
        aq = z(ctx.fk_shapes[0]) if g_queried[0] is None else g_queried[0].to(torch.float32).contiguous()
        aqd = z(ctx.fk_shapes[1]) if g_queried[1] is None else g_queried[1].to(torch.float32).contiguous()
        fk = (jq, jqd, aq, aqd)
    g = ctx.dm.rollout_backward_traj_loss(bs, nsteps, dt, q_init, qd_init, torques, refs, ke, kd, inv_m, inertia, inv_inertia,
                                          frame2step, ws, tl, gl, fk=fk, **adj, **_want_kw(ctx))
    g_tgt = None
    if ctx.needs_input_grad[11] and tl["seed_gt"] is not None:  # d loss_traj / d target pose = g x share / nb x d se3 / d gt
        # a zero share is an ASSIGNMENT in the reference (loss_seq[i, idx:] = 0, loss_traj[outseq_idx] = 0): nothing flows there, not 0 * inf
        k = (tl["scale"] * (gl / ctx.dm.nb))[:, :, None, None]
        g_tgt = torch.where(k != 0, tl["seed_gt"] * k, torch.zeros_like(tl["seed_gt"])).view(ctx.tgt_shape)
    out = _grad_tuple(g, (g["q_init"], g["qd_init"]), torques, res_f, refs, inertia, inv_inertia, ctx.mass_shape, ws.device) + (g_tgt, None)
    if g_queried is not None:
        out += (g.get("fk_joint_q"), g.get("fk_joint_qd"))
    ctx.tl = None  # the sweep's buffers go with it (a second backward through the same graph is not supported, as with saved tensors)
    return out
