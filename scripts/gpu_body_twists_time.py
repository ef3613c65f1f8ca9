#!/usr/bin/env python3
"""Device time of the body-twist op (pd_pose_op PD_POSE_BODY_TWIST), forward and VJP, on the frame poses of a rollout and the measured
joint rates of the same frames gathered into the op's six slots -- Laikago 4096 and human 1024 by default (arguments: robot:bs ...),
100 steps, the first four frames -- beside the joint-coordinates op (pd_pose_op PD_POSE_JOINT_COORDS, rates measured: forward and VJP)
on the same frames.  Each measured piece is timed by the rule of gpu_common.timed.  Also printed: the element count (frames x bs x nb)
and the bytes the two launches move."""
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
    nb, nqd = dm.nb, dm.nqd
    F = min(FRAMES, len(fos))
    state = torch.cat([pos, vel], -1)[:F].reshape(-1, 13).contiguous()
    n = state.shape[0]
    table = hip_backend.env_joint_table(env, dev, "measured")
    _, jqd = hip_backend.joint_coords(table, nb, state)
    slots = torch.cat([jqd, jqd.new_zeros(n // nb, 1)], -1).index_select(-1, hip_backend.env_joint_rate_slot_index(env, dev))
    rows = torch.cat([state[:, :7], slots.reshape(n, 6)], -1).contiguous()
    g_out = torch.randn(n, 6, device=dev)
    g_q, g_qd = torch.randn(n // nb, dm.nq, device=dev), torch.randn(n // nb, nqd, device=dev)
    res = dict(bt_fwd=timed(lambda: hip_backend.body_twists(table, nb, rows)),
               bt_vjp=timed(lambda: hip_backend.body_twists_vjp(table, nb, rows, g_out)),
               jc_fwd=timed(lambda: hip_backend.joint_coords(table, nb, state)),
               jc_vjp=timed(lambda: hip_backend.joint_coords_vjp(table, nb, state, g_q, g_qd)))
    print("BODYTWIST %-8s bs=%-5d frames=%d elements=%d bytes fwd %d vjp %d  body twists fwd %.4f ms  vjp %.4f ms  |  "
          "joint coords fwd %.4f ms  vjp %.4f ms" % (
              name, bs, F, n, n * (13 + 6) * 4, n * (13 + 6 + 13) * 4, res["bt_fwd"], res["bt_vjp"], res["jc_fwd"], res["jc_vjp"]),
          flush=True)
