"""Shared by tests/test_ground_wrench_host.py and tests/test_gpu_ground_wrench.py: the two-material model the ground-wrench op is held
to, and its float64 / float32 torch yardsticks (oracle/ref_torch.py eval_body_contacts; nothing here runs product code)."""
import numpy as np
import torch

from helpers import tight_inputs

MATERIALS = np.asarray([[1.0e4, 30.0, 1.0e2, 1.0], [6.0e3, 10.0, 40.0, 0.4]], np.float32)   # (ke, kd, kf, mu)
MATERIALS_B = np.asarray([[8.0e3, 20.0, 70.0, 0.8], [1.2e4, 5.0, 1.5e2, 0.6]], np.float32)  # the rows of the "materials update" tests


def two_material_template(name, materials=MATERIALS):
    """The shipped template with two materials: candidates of even bodies take row 0, of odd bodies row 1."""
    from diffphys_amd import robots

    tpl = dict(robots.load_template(name))
    tpl["shape_materials"] = np.asarray(materials, np.float32).copy()
    tpl["contact_material"] = (np.asarray(tpl["contact_body"]) % 2).astype(np.int32)
    return tpl


def model_inputs(tpl, name, bs=3, T=6, seed=5, lowered_env=None):
    """tight_inputs of the common model; lowered_env: that env's root 6 cm further into the ground (contact forces on the +-500 N clamp)."""
    inp = tight_inputs(tpl, name, bs, T, seed=seed)
    if lowered_env is not None:
        q = inp["q_init"].reshape(bs, -1).copy()
        q[lowered_env, 1] -= 0.06
        inp["q_init"] = np.ascontiguousarray(q.reshape(-1))
    return inp


def oracle_template(tpl, dtype):
    from oracle import ref_torch

    return ref_torch.Template(tpl, dtype)


def oracle_wrench(T, body_q, body_qd):
    """eval_body_contacts(T, q, qd, 0): [S, nb, 7], [S, nb, 6] -> [S, nb, 6]"""
    from oracle import ref_torch

    return ref_torch.eval_body_contacts(T, body_q, body_qd, torch.zeros(body_q.shape[:-1] + (6,), dtype=T.dtype))


def candidate_probe(tpl, body_q, body_qd):
    """float64, per (state set, candidate): the height c and the largest |component| of the unclamped contact force (NaN where c > 0)."""
    from oracle import ref_torch as rt

    T = oracle_template(tpl, torch.float64)
    q, qd = torch.as_tensor(body_q, dtype=torch.float64), torch.as_tensor(body_qd, dtype=torch.float64)
    cb = T.c_body
    X = q[:, cb]
    p, r = X[..., :3], X[..., 3:]
    n = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)
    cp = p + rt.q_rot(r, T.c_point[None].expand(q.shape[0], -1, 3)) - n * T.c_dist[None, :, None]
    rr = cp - (p + rt.q_rot(r, T.com[cb][None].expand(q.shape[0], -1, 3)))
    dpdt = qd[:, cb, 3:] + rt.cross(qd[:, cb, :3], rr)
    c = cp[..., 1]
    mat = T.materials[T.c_mat]
    vn = dpdt[..., 1]
    vt = dpdt - n * vn[..., None]
    fnfd = c * mat[:, 0] + torch.minimum(vn, torch.zeros_like(vn)) * mat[:, 1] * (c < 0).to(torch.float64)
    a_, b_ = mat[:, 2] * rt.safe_length(vt), -mat[:, 3] * fnfd
    f = n * fnfd[..., None] + rt.safe_normalize(vt) * torch.where(a_ < b_, a_, b_)[..., None]
    fmax = torch.where(c > 0, torch.full_like(c, float("nan")), f.abs().amax(-1))
    return c.numpy(), fmax.numpy()


def wrench_and_state_grads(tpl, dtype, body_q, body_qd, g_out=None):
    """The oracle's wrench [S, nb, 6] and, with g_out, autograd of <g_out, wrench> -> (wrench, g_body_q, g_body_qd, g_materials), numpy."""
    T = oracle_template(tpl, dtype)
    q = torch.as_tensor(np.asarray(body_q), dtype=dtype).clone().requires_grad_(g_out is not None)
    qd = torch.as_tensor(np.asarray(body_qd), dtype=dtype).clone().requires_grad_(g_out is not None)
    if g_out is not None:
        T.materials.requires_grad_(True)
    w = oracle_wrench(T, q, qd)
    if g_out is None:
        return w.numpy()
    (w * torch.as_tensor(np.asarray(g_out), dtype=dtype)).sum().backward()
    return w.detach().numpy(), q.grad.numpy(), qd.grad.numpy(), T.materials.grad.numpy()


def oracle_rollout_grads(tpl, dtype, inp, loss_fn, wrt=("materials",), need_grf=False):
    """Autograd through the torch oracle's rollout.  loss_fn(pos [F, bs*nb, 7], vel [F, bs*nb, 6], grfs) -> scalar, the frames those of
    inp["frame2step"] (state nsteps included), grfs [frames with a step < nsteps, bs*nb, 6] or None; wrt: "materials" or rollout input
    names.  -> dict of numpy gradients."""
    from helpers import INPUT_NAMES
    from oracle import ref_torch

    T = oracle_template(tpl, dtype)
    t = {k: torch.as_tensor(np.asarray(inp[k]), dtype=dtype).clone() for k in INPUT_NAMES}
    leaves = {}
    for k in wrt:
        leaves[k] = T.materials.requires_grad_(True) if k == "materials" else t[k].requires_grad_(True)
    f2s = [int(s) for s in inp["frame2step"]]
    args = [t[k] for k in INPUT_NAMES] + [inp["nsteps"], f2s, inp["dt"]]
    allq, allqd = ref_torch.rollout(T, *args, return_all=True)
    pos, vel = allq[f2s].reshape(len(f2s), -1, 7), allqd[f2s].reshape(len(f2s), -1, 6)
    grfs = ref_torch.rollout(T, *args)[2] if need_grf else None
    loss_fn(pos, vel, grfs).backward()
    return {k: v.grad.numpy() for k, v in leaves.items()}
