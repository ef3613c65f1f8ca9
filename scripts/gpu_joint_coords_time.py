#!/usr/bin/env python3
"""Device time of the joint-coordinates op (pd_pose_op PD_POSE_JOINT_COORDS): forward and vector-Jacobian product on 100 states per env,
Laikago 4096 envs and human 1024 envs by default (arguments: robot:bs ...).  The states are the FK kernel's of random joint coordinates
(angles uniform in +-1, random unit root quaternions).  Timed by the rule of gpu_common.timed.  Also printed:
the bytes each launch moves at the least -- 52 B read per body plus the outputs (forward: 4 (nq + nqd) B per state set; VJP: that read again as g_out, 52 B written per body) -- and the bandwidth that amounts to."""
import sys
from gpu_common import timed
import torch
from diffphys_amd import hip_backend, robots, sim

cfgs = [(a.split(":")[0], int(a.split(":")[1])) for a in sys.argv[1:] if not a.startswith("--")] or [("laikago", 4096), ("human", 1024)]
dev = torch.device("cuda:0")
T = 100


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
    state = torch.cat([bq.reshape(-1, 7), bqd.reshape(-1, 6)], 1).contiguous()
    g_out = torch.randn(sets, nq + nqd, device=dev, generator=gen)
    n = sets * nb
    out = torch.empty(sets, nq + nqd, device=dev)
    g_b = torch.empty(n, 13, device=dev)
    L, st = hip_backend.lib(), hip_backend._stream
    for rates in ("generalized", "measured"):
        table = hip_backend.joint_table(tpl, rates, dev)
        fwd = lambda: hip_backend._check(L.pd_pose_op(hip_backend.POSE_JOINT_COORDS, n, table.data_ptr(), nb, state.data_ptr(), out.data_ptr(), st()))
        vjp = lambda: hip_backend._check(L.pd_pose_op_vjp(hip_backend.POSE_JOINT_COORDS, n, table.data_ptr(), nb, state.data_ptr(), g_out.data_ptr(),
                                                         None, g_b.data_ptr(), st()))
        t_f, t_v = timed(fwd), timed(vjp)
        b_f = n * 52 + sets * (nq + nqd) * 4
        b_v = n * 52 * 2 + sets * (nq + nqd) * 4
        print("JOINTCOORDS %-8s bs=%-5d states/env=%d rates=%-11s elements=%d  forward %.4f ms (%.1f MB, %.0f GB/s)  vjp %.4f ms (%.1f MB, %.0f GB/s)" % (
            name, bs, T, rates, n, t_f, b_f / 1e6, b_f / t_f / 1e6, t_v, b_v / 1e6, b_v / t_v / 1e6), flush=True)
