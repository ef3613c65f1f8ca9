"""The per-body ground-contact state of body states -- what PD_POSE_CONTACT_STATE computes -- restated over oracle/ref_torch.py's own
q_rot / cross in a chosen dtype, with autograd: the yardstick of tests/test_contact_state_host.py and tests/test_gpu_contact_state.py.
Nothing here runs product code.

Per candidate c of body b (P_c = contact_point, dist_c; quaternions as they are, not normalised):
    rp = q_rot(q, P_c)      rc = q_rot(q, com_b)      h_c = p.y + rp.y - dist_c
    rr_c = (rp.x - rc.x, h_c - p.y - rc.y, rp.z - rc.z)      u_c = v + w x rr_c
Per body: c* = the candidate of lowest h_c (first one in template order on ties) -> (h_c*, p.x + rp*.x, p.z + rp*.z, u_c*, s, k) with k the
number of candidates with not (h_c > 0) and s the sum of -h_c over them; (+inf, 0, 0, 0, 0, 0, 0, 0) for a body without candidates.
The arg-min index and the touch mask are taken in the dtype that is evaluated."""
import numpy as np
import torch

NAMES = ("height", "point_xz", "velocity", "depth", "count")
SLICES = dict(height=slice(0, 1), point_xz=slice(1, 3), velocity=slice(3, 6), depth=slice(6, 7), count=slice(7, 8))


def candidates(T, body_q, body_qd):
    """T: ref_torch.Template; body_q [S, nb, 7], body_qd [S, nb, 6] (w, v) of its dtype -> per (set, candidate): h [S, nc],
    (x, z) [S, nc, 2], u [S, nc, 3]."""
    from oracle import ref_torch as rt

    S, cb = body_q.shape[0], T.c_body
    X = body_q[:, cb]
    p, q = X[..., :3], X[..., 3:]
    w, v = body_qd[:, cb, :3], body_qd[:, cb, 3:]
    rp = rt.q_rot(q, T.c_point[None].expand(S, -1, 3))
    rc = rt.q_rot(q, T.com[cb][None].expand(S, -1, 3))
    h = p[..., 1] + rp[..., 1] - T.c_dist[None]
    rr = torch.stack([rp[..., 0] - rc[..., 0], h - p[..., 1] - rc[..., 1], rp[..., 2] - rc[..., 2]], -1)
    u = v + rt.cross(w, rr)
    return h, torch.stack([p[..., 0] + rp[..., 0], p[..., 2] + rp[..., 2]], -1), u


def contact_state(T, body_q, body_qd):
    """body_q [S, nb, 7], body_qd [S, nb, 6] (w, v) of the template's dtype -> [S, nb, 8] = (h, x, z, u.xyz, s, k)."""
    S = body_q.shape[0]
    h, xz, u = candidates(T, body_q, body_qd)
    rows = []
    none = torch.cat([torch.full((S, 1), float("inf"), dtype=T.dtype), torch.zeros(S, 7, dtype=T.dtype)], -1)
    for b in range(T.nb):
        idx = torch.nonzero(T.c_body == b).reshape(-1)   # template order
        if idx.numel() == 0:
            rows.append(none)
            continue
        hb = h[:, idx]
        best = hb.detach().argmin(1, keepdim=True)   # the first minimum
        pick = lambda t: t[:, idx].gather(1, best[..., None].expand(S, 1, t.shape[-1]))[:, 0]
        touch = ~(hb.detach() > 0)
        depth = torch.where(touch, -hb, torch.zeros_like(hb)).sum(1, keepdim=True)
        rows.append(torch.cat([hb.gather(1, best), pick(xz), pick(u), depth, touch.sum(1, keepdim=True).to(T.dtype)], -1))
    return torch.stack(rows, 1)


def contact_state_of(tpl, dtype, body_q, body_qd, g_out=None):
    """numpy states [S, nb, 7], [S, nb, 6] -> the [S, nb, 8] output in ``dtype`` and, with g_out [S, nb, 8] (entry 7 has no gradient to
    carry), autograd of <g_out, out>: (out, g_body_q, g_body_qd), numpy."""
    from oracle import ref_torch

    T = ref_torch.Template(tpl, dtype)
    need = g_out is not None
    bq = torch.tensor(np.array(body_q), dtype=dtype).requires_grad_(need)
    bqd = torch.tensor(np.array(body_qd), dtype=dtype).requires_grad_(need)
    out = contact_state(T, bq, bqd)
    if not need:
        return (out.numpy(),)
    g = torch.as_tensor(np.array(g_out), dtype=dtype)
    # bodies without candidates: +inf times its seed is not a number to differentiate; their row carries no gradient either way
    (torch.where(torch.isinf(out), torch.zeros_like(out), out) * g).sum().backward()
    return out.detach().numpy(), bq.grad.numpy(), bqd.grad.numpy()


def field(out, name):
    v = out[..., SLICES[name]]
    return v[..., 0] if v.shape[-1] == 1 else v


def input_conditions(tpl, body_q, body_qd):
    """float64, from the fp32 rows as the kernel gets them -> dict: ground = the smallest |h_c| over all candidates; gap [S, nb] = the
    distance of every element's two lowest heights (inf for a body of fewer than two candidates); winner [S, nb] = the index of the
    lowest candidate INSIDE its body (-1 without candidates); count [nb] = candidates per body."""
    from oracle import ref_torch

    T = ref_torch.Template(tpl, torch.float64)
    h = candidates(T, torch.as_tensor(np.array(body_q), dtype=torch.float64), torch.as_tensor(np.array(body_qd), dtype=torch.float64))[0].numpy()
    cb = np.asarray(tpl["contact_body"]).reshape(-1)
    S, nb = h.shape[0], int(tpl["nb"])
    gap, winner, count = np.full((S, nb), np.inf), np.full((S, nb), -1, np.int64), np.zeros(nb, np.int64)
    for b in range(nb):
        hb = h[:, cb == b]
        count[b] = hb.shape[1]
        if hb.shape[1]:
            winner[:, b] = hb.argmin(1)
        if hb.shape[1] > 1:
            two = np.sort(hb, axis=1)[:, :2]
            gap[:, b] = two[:, 1] - two[:, 0]
    return dict(ground=float(np.abs(h).min()) if h.size else np.inf, gap=gap, winner=winner, count=count)
