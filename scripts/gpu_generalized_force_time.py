#!/usr/bin/env python3
"""Device time of the generalised-force op (pd_pose_op PD_POSE_GENERALIZED_FORCE), forward and VJP, on the frame poses of a rollout and
its own jaf -- Laikago 4096 and human 1024 by default (arguments: robot:bs ...), 100 steps, the first four frames -- beside the
joint-coordinates op (pd_pose_op PD_POSE_JOINT_COORDS, rates measured: forward and VJP) on the same frames.  Each measured piece is timed
by the rule of gpu_common.timed.  Also printed: the element count (frames x bs x nb) and the bytes the two launches move."""
import sys
from gpu_common import FWD, timed
import torch
from diffphys_amd import hip_backend, robots, sim, synth

cfgs = [(a.split(":")[0], int(a.split(":")[1])) for a in sys.argv[1:] if not a.startswith("--")] or [("laikago", 4096), ("human", 1024)]
dev = torch.device("cuda:0")
FRAMES = 4


for name, bs in cfgs:
    tpl = robots.load_template(name)
    T = 100
    inp = synth.make_inputs(tpl, name, bs=bs, nsteps=T, seed=0, seqs=("mi-trot", "mi-spin"))
    env = sim.Model.from_template(tpl, bs, dev)
    dm = hip_backend.device_model(env)
    t = {k: torch.from_numpy(inp[k]).to(dev) for k in FWD}
    fos = list(inp["frame2step"])
    pos, vel, _, jaf, _ = dm.rollout_forward(bs, T, inp["dt"], *[t[k] for k in FWD], frame2step=fos, out=dm.alloc_rollout(bs, T, len(fos), dev))
    nb, nqd = dm.nb, dm.nqd
    F = min(FRAMES, len(fos))
    rows = torch.cat([pos, jaf], -1)[:F].reshape(-1, 13).contiguous()
    state = torch.cat([pos, vel], -1)[:F].reshape(-1, 13).contiguous()
    n = rows.shape[0]
    table = hip_backend.env_joint_table(env, dev, "measured")
    g_q, g_qd = torch.randn(n // nb, dm.nq, device=dev), torch.randn(n // nb, nqd, device=dev)
    res = dict(gf_fwd=timed(lambda: hip_backend.generalized_force(table, nb, rows)),
               gf_vjp=timed(lambda: hip_backend.generalized_force_vjp(table, nb, rows, g_qd)),
               jc_fwd=timed(lambda: hip_backend.joint_coords(table, nb, state)),
               jc_vjp=timed(lambda: hip_backend.joint_coords_vjp(table, nb, state, g_q, g_qd)))
    sets = n // nb
    print("GENFORCE %-8s bs=%-5d frames=%d elements=%d bytes fwd %d vjp %d  generalized force fwd %.4f ms  vjp %.4f ms  |  "
          "joint coords fwd %.4f ms  vjp %.4f ms" % (
              name, bs, F, n, (n * 13 + sets * nqd) * 4, (n * 13 + sets * nqd + n * 13) * 4, res["gf_fwd"], res["gf_vjp"], res["jc_fwd"], res["jc_vjp"]),
          flush=True)
