#!/usr/bin/env python3
"""Device time of the ground-wrench op (pd_pose_op PD_POSE_GROUND_WRENCH) beside the adjoint launch of the same run, Laikago 4096 x 100 by
default (arguments: robot:bs ...).  Each measured piece is timed by the rule of gpu_common.timed:
  material gradient   dp_model.material_gradient over the whole saved trajectory: the chunked VJP launches and their colsums
  frame wrench        the forward op on the states of the rollout's frames (the differentiable-grf recipe)
  adjoint             the rollout's adjoint launch (pd_last_kernel_ms), which produced the g_res_f the material gradient contracts
Also printed: the element count (T x bs x nb) and the share of elements -- one wavefront each -- that found a touching candidate."""
import sys
from gpu_common import BWD, FWD, timed
import numpy as np, torch
from diffphys_amd import dp_model, hip_backend, robots, sim, synth

cfgs = [(a.split(":")[0], int(a.split(":")[1])) for a in sys.argv[1:] if not a.startswith("--")] or [("laikago", 4096)]
dev = torch.device("cuda:0")


for name, bs in cfgs:
    tpl = robots.load_template(name)
    T = 100
    inp = synth.make_inputs(tpl, name, bs=bs, nsteps=T, seed=0, seqs=("mi-trot", "mi-spin"))
    env = sim.Model.from_template(tpl, bs, dev)
    dm = hip_backend.device_model(env)
    dm.set_timing(True)
    t = {k: torch.from_numpy(inp[k]).to(dev) for k in FWD + ("adj_pos", "adj_vel")}
    fos = list(inp["frame2step"])
    bufs = dm.alloc_rollout(bs, T, len(fos), dev)
    pos, vel, grf, jaf, ws = dm.rollout_forward(bs, T, inp["dt"], *[t[k] for k in FWD], frame2step=fos, out=bufs)
    adj = []
    for it in range(9):
        g = dm.rollout_backward(bs, T, inp["dt"], *[t[k] for k in BWD], fos, ws, t["adj_pos"], t["adj_vel"], out=bufs)
        torch.cuda.synchronize()
        if it >= 4:
            adj.append(dm.last_kernel_ms(1))
    table = hip_backend.env_contact_table(env, dev)
    nmat = len(tpl["shape_materials"])
    t_mat = timed(lambda: dp_model.material_gradient(dm, table, nmat, ws, bs, T, g["res_f"]))
    frames = torch.cat([pos, vel], -1).view(-1, 13)
    t_frm = timed(lambda: hip_backend.ground_wrench(table, dm.nb, frames))
    bq, bqd, _, _ = dm.saved_trajectory(ws, bs, T)
    touching = 0
    for s in range(0, T, 10):   # the forward op on the saved states, ten steps at a time: which elements touch
        w = hip_backend.ground_wrench(table, dm.nb, torch.cat([bq[s: s + 10], bqd[s: s + 10]], -1).view(-1, 13))
        touching += int((w != 0).any(1).sum().item())
    n = T * bs * dm.nb
    print("GROUNDWRENCH %-8s bs=%-5d T=%d nmat=%d elements=%d touching=%.2f %%  material gradient %.3f ms  frame wrench (%d frames, %d elements) "
          "%.4f ms  adjoint %.4f ms" % (name, bs, T, nmat, n, 100.0 * touching / n, t_mat, len(fos), frames.shape[0], t_frm,
                                         float(np.median(adj))), flush=True)
