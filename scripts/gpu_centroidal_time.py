#!/usr/bin/env python3
"""Device time of the whole-body (centroidal) op (pd_pose_op PD_POSE_CENTROIDAL): forward and vector-Jacobian product on 100 states per
env, Laikago 4096 envs by default (arguments: robot:bs ...), and beside it the same expression composed from torch ops in fp32 on the
GPU (forward, and forward + backward of <g_out, out> by autograd: what a user would write without the op).  The states are the FK
kernel's of random joint coordinates; masses and inertias are the template's, per state set.  Timed by the rule of
gpu_common.timed.  Also printed: the bytes each launch moves at the least -- 92 B read per body (forward: + 64 B written per state set; VJP: + 64 B read per set and 92 B written per body) -- the bandwidth that
amounts to and its fraction of the HBM peak (8 TB/s)."""
import sys
from gpu_common import timed
import numpy as np, torch
from diffphys_amd import hip_backend, robots, sim

cfgs = [(a.split(":")[0], int(a.split(":")[1])) for a in sys.argv[1:] if not a.startswith("--")] or [("laikago", 4096)]
dev = torch.device("cuda:0")
T = 100
HBM_PEAK = 8.0e12


def q_rot(q, v, sign=1.0):
    u, w = q[..., :3], q[..., 3:]
    return v * (2.0 * w * w - 1.0) + sign * 2.0 * w * torch.cross(u, v, dim=-1) + 2.0 * u * (u * v).sum(-1, keepdim=True)


def torch_centroidal(bq, bqd, mass, inertia, com, grav):
    """the definition of include/ppr_diffphys.h, op by op: [S, nb, .] -> [S, 16]"""
    p, q, w, v, m = bq[..., :3], bq[..., 3:], bqd[..., :3], bqd[..., 3:], mass[..., None]
    x = p + q_rot(q, com.expand_as(p))
    wb = q_rot(q, w, -1.0)
    M = mass.sum(-1, keepdim=True)
    c = (m * x).sum(-2) / M
    P = (m * v).sum(-2)
    cd = P / M
    h = (inertia * wb[..., None, :]).sum(-1)
    L = (q_rot(q, h) + m * torch.cross(x - c[..., None, :], v - cd[..., None, :], dim=-1)).sum(-2)
    Tk = (0.5 * mass * (v * v).sum(-1) + 0.5 * (wb * h).sum(-1)).sum(-1, keepdim=True)
    V = -(mass * (x * grav).sum(-1)).sum(-1, keepdim=True)
    return torch.cat([M, c, cd, P, L, Tk, V, torch.zeros_like(M)], -1)


for name, bs in cfgs:
    tpl = robots.load_template(name)
    env = sim.Model.from_template(tpl, bs, dev)
    dm = hip_backend.device_model(env)
    nb, nq, nqd = dm.nb, dm.nq, dm.nqd
    sets = bs * T
    gen = torch.Generator(device=dev).manual_seed(0)
    q = torch.rand(sets, nq, device=dev, generator=gen) * 2.0 - 1.0
    q[:, 3:7] = torch.nn.functional.normalize(torch.randn(sets, 4, device=dev, generator=gen), dim=1)
    qd = torch.randn(sets, nqd, device=dev, generator=gen)
    bq, bqd = dm.fk_forward(q.contiguous(), qd)
    bq, bqd = bq.reshape(sets, nb, 7), bqd.reshape(sets, nb, 6)
    mass = torch.tensor(np.asarray(tpl["body_mass"], np.float32), device=dev).expand(sets, nb).contiguous()
    inertia = torch.tensor(np.asarray(tpl["body_inertia"], np.float32), device=dev).expand(sets, nb, 3, 3).contiguous()
    rows = torch.cat([bq, bqd, mass[..., None], inertia.reshape(sets, nb, 9)], -1).reshape(-1, 23).contiguous()
    g_out = torch.randn(sets, 16, device=dev, generator=gen)
    n = sets * nb
    out = torch.empty(sets, 16, device=dev)
    g_b = torch.empty(n, 23, device=dev)
    table = hip_backend.mass_table(tpl, dev)
    L, st = hip_backend.lib(), hip_backend._stream
    fwd = lambda: hip_backend._check(L.pd_pose_op(hip_backend.POSE_CENTROIDAL, n, table.data_ptr(), nb, rows.data_ptr(), out.data_ptr(), st()))
    vjp = lambda: hip_backend._check(L.pd_pose_op_vjp(hip_backend.POSE_CENTROIDAL, n, table.data_ptr(), nb, rows.data_ptr(), g_out.data_ptr(),
                                                     None, g_b.data_ptr(), st()))
    t_f, t_v = timed(fwd), timed(vjp)
    b_f = n * 92 + sets * 64
    b_v = n * 92 * 2 + sets * 64
    print("CENTROIDAL %-8s bs=%-5d states/env=%d elements=%d  forward %.4f ms (%.1f MB, %.0f GB/s, %.0f %% of the HBM floor)  "
          "vjp %.4f ms (%.1f MB, %.0f GB/s, %.0f %% of the HBM floor)" % (
              name, bs, T, n, t_f, b_f / 1e6, b_f / t_f / 1e6, 100 * b_f / HBM_PEAK / (t_f * 1e-3), t_v, b_v / 1e6, b_v / t_v / 1e6,
              100 * b_v / HBM_PEAK / (t_v * 1e-3)), flush=True)

    com = torch.tensor(np.asarray(tpl["body_com"], np.float32).reshape(nb, 3), device=dev)
    grav = torch.tensor(np.asarray(tpl["gravity"], np.float32).reshape(3), device=dev)
    leaves = [a.clone().requires_grad_(True) for a in (bq, bqd, mass, inertia)]
    with torch.no_grad():
        ref = torch_centroidal(bq, bqd, mass, inertia, com, grav)
        t_tf = timed(lambda: torch_centroidal(bq, bqd, mass, inertia, com, grav))

    def torch_fwd_bwd():
        for a in leaves:
            a.grad = None
        (torch_centroidal(*leaves, com, grav) * g_out).sum().backward()

    t_tfb = timed(torch_fwd_bwd)
    fwd()
    torch.cuda.synchronize()
    dev_max = float(((out - ref).abs().amax(0) / (ref.abs().amax(0) + 1e-30)).max())
    print("CENTROIDAL %-8s torch composition (fp32, eager): forward %.4f ms, forward + backward %.4f ms -> the op is %.1f x faster forward, "
          "%.1f x faster forward + vjp (%.4f ms); largest column-relative difference of the two forwards %.1e" % (
              name, t_tf, t_tfb, t_tf / t_f, t_tfb / (t_f + t_v), t_f + t_v, dev_max), flush=True)
