#!/usr/bin/env python3
"""Device time of the contact-state op (pd_pose_op PD_POSE_CONTACT_STATE), forward and VJP, on the frame states of a rollout -- Laikago
4096 and human 1024 by default (arguments: robot:bs ...), 100 steps, the first four frames -- beside the ground-wrench op (forward and
state VJP) on the SAME rows.  Each measured piece is timed by the rule of gpu_common.timed.  Also printed:
the element count (frames x bs x nb), the candidates a state set sweeps, the share of elements with a touching candidate, and the two launches on the 10 x 24 state sets of phys_model's training window (what reg_pen /
reg_skate add to an iteration)."""
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
    pos, vel, _, _, _ = dm.rollout_forward(bs, T, inp["dt"], *[t[k] for k in FWD], frame2step=fos, out=dm.alloc_rollout(bs, T, len(fos), dev))
    nb, nmat = dm.nb, len(tpl["shape_materials"])
    rows = torch.cat([pos, vel], -1)[:FRAMES].reshape(-1, 13).contiguous()
    n = rows.shape[0]
    table = hip_backend.env_contact_table(env, dev)
    g8, g6 = torch.randn(n, 8, device=dev), torch.randn(n, 6, device=dev)
    out = hip_backend.contact_state(table, nb, rows)
    res = dict(cs_fwd=timed(lambda: hip_backend.contact_state(table, nb, rows)),
               cs_vjp=timed(lambda: hip_backend.contact_state_vjp(table, nb, rows, g8)),
               gw_fwd=timed(lambda: hip_backend.ground_wrench(table, nb, rows)),
               gw_vjp=timed(lambda: hip_backend.ground_wrench_vjp(table, nb, nmat, rows, g6, need_materials=False)))
    wdw = rows[: 240 * nb].contiguous()   # phys_model's training window: 10 envs x 24 frames
    gw8 = g8[: wdw.shape[0]].contiguous()
    res["wdw_fwd"] = timed(lambda: hip_backend.contact_state(table, nb, wdw))
    res["wdw_vjp"] = timed(lambda: hip_backend.contact_state_vjp(table, nb, wdw, gw8))
    print("CONTACTSTATE %-8s bs=%-5d frames=%d elements=%d candidates/set=%d touching=%.2f %%  contact state fwd %.4f ms  vjp %.4f ms  |  "
          "ground wrench fwd %.4f ms  state vjp %.4f ms  |  240 sets (%d elements): fwd %.4f ms  vjp %.4f ms" % (
              name, bs, min(FRAMES, len(fos)), n, len(tpl["contact_body"]), 100.0 * float((out[:, 7] > 0).float().mean()),
              res["cs_fwd"], res["cs_vjp"], res["gw_fwd"], res["gw_vjp"], wdw.shape[0], res["wdw_fwd"], res["wdw_vjp"]), flush=True)
