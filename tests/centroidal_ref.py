"""The whole-body (centroidal) quantities of body states -- what PD_POSE_CENTROIDAL computes -- restated over oracle/ref_torch.py's own
q_rot / q_rot_inv / cross in a chosen dtype, with autograd: the yardstick of tests/test_centroidal_host.py and
tests/test_gpu_centroidal.py.  Nothing here runs product code.

Per body i of a state set (quaternions as they are, not normalised):
    x_i = p_i + q_rot(q_i, com_i)        wb_i = q_rot_inv(q_i, w_i)
    M = sum m_i      c = sum m_i x_i / M      P = sum m_i v_i      c_dot = P / M
    L = sum [ q_rot(q_i, I_i wb_i) + m_i (x_i - c) x (v_i - c_dot) ]
    T = sum [ m_i |v_i|^2 / 2 + wb_i . I_i wb_i / 2 ]      V = -sum m_i gravity . x_i"""
import numpy as np
import torch

NAMES = ("mass", "com", "com_vel", "momentum", "angular_momentum", "kinetic", "potential")
SLICES = dict(mass=slice(0, 1), com=slice(1, 4), com_vel=slice(4, 7), momentum=slice(7, 10), angular_momentum=slice(10, 13),
              kinetic=slice(13, 14), potential=slice(14, 15))


def centroidal(body_q, body_qd, mass, inertia, com, gravity):
    """body_q [..., nb, 7], body_qd [..., nb, 6] (w, v), mass [..., nb], inertia [..., nb, 3, 3], com [nb, 3], gravity [3] (torch, one
    dtype) -> [..., 16] = (M, c, c_dot, P, L, T, V, 0)."""
    from oracle import ref_torch as rt

    p, q = body_q[..., :3], body_q[..., 3:]
    w, v = body_qd[..., :3], body_qd[..., 3:]
    m = mass[..., None]
    x = p + rt.q_rot(q, com.expand(p.shape))
    wb = rt.q_rot_inv(q, w)
    M = mass.sum(-1, keepdim=True)
    c = (m * x).sum(-2) / M
    P = (m * v).sum(-2)
    cd = P / M
    h = (inertia * wb[..., None, :]).sum(-1)
    L = (rt.q_rot(q, h) + m * rt.cross(x - c[..., None, :], v - cd[..., None, :])).sum(-2)
    T = (0.5 * mass * (v * v).sum(-1) + 0.5 * (wb * h).sum(-1)).sum(-1, keepdim=True)
    V = -(mass * (x * gravity).sum(-1)).sum(-1, keepdim=True)
    return torch.cat([M, c, cd, P, L, T, V, torch.zeros_like(M)], -1)


def template_constants(tpl, dtype):
    return (torch.as_tensor(np.asarray(tpl["body_com"], np.float64).reshape(-1, 3), dtype=dtype),
            torch.as_tensor(np.asarray(tpl["gravity"], np.float64).reshape(3), dtype=dtype))


def centroidal_of(tpl, dtype, body_q, body_qd, mass, inertia, g_out=None):
    """numpy in -> the [S, 16] output in ``dtype`` and, with g_out [S, 16], autograd of <g_out, out>:
    (out, g_body_q, g_body_qd, g_mass, g_inertia), numpy."""
    com, grav = template_constants(tpl, dtype)
    need = g_out is not None
    t = [torch.as_tensor(np.array(a), dtype=dtype).requires_grad_(need) for a in (body_q, body_qd, mass, inertia)]
    out = centroidal(*t, com, grav)
    if not need:
        return (out.numpy(),)
    (out * torch.as_tensor(np.array(g_out), dtype=dtype)).sum().backward()
    return (out.detach().numpy(),) + tuple(a.grad.numpy() for a in t)
