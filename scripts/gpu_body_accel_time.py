#!/usr/bin/env python3
"""Device time of the body-acceleration op (pd_pose_op PD_POSE_BODY_ACCEL), forward and VJP, on the frame states of a rollout as they
are, with the measured joint rates of the same frames standing in for the slot derivatives -- Laikago 4096 and human 1024 by default
(arguments: robot:bs ...), 100 steps, the first four frames -- beside the body-twist op (pd_pose_op PD_POSE_BODY_TWIST: forward and
VJP) on the same frames in the same run.  Each measured piece is timed by the rule of gpu_common.timed.  Also printed: the element count
(frames x bs x nb) and the bytes the two launches move."""
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
    nb = dm.nb
    F = min(FRAMES, len(fos))
    state = torch.cat([pos, vel], -1)[:F].reshape(-1, 13).contiguous()
    n = state.shape[0]
    table = hip_backend.env_joint_table(env, dev, "measured")
    _, jqd = hip_backend.joint_coords(table, nb, state)
    slots = torch.cat([jqd, jqd.new_zeros(n // nb, 1)], -1).index_select(-1, hip_backend.env_joint_rate_slot_index(env, dev)).reshape(n, 6)
    rows19 = torch.cat([state, slots], -1).contiguous()
    rows13 = torch.cat([state[:, :7], slots], -1).contiguous()
    g_out = torch.randn(n, 6, device=dev)
    res = dict(ba_fwd=timed(lambda: hip_backend.body_accelerations(table, nb, rows19)),
               ba_vjp=timed(lambda: hip_backend.body_accelerations_vjp(table, nb, rows19, g_out)),
               bt_fwd=timed(lambda: hip_backend.body_twists(table, nb, rows13)),
               bt_vjp=timed(lambda: hip_backend.body_twists_vjp(table, nb, rows13, g_out)))
    print("BODYACCEL %-8s bs=%-5d frames=%d elements=%d bytes fwd %d vjp %d  body accelerations fwd %.4f ms  vjp %.4f ms  |  "
          "body twists fwd %.4f ms  vjp %.4f ms" % (
              name, bs, F, n, n * (19 + 6) * 4, n * (19 + 6 + 19) * 4, res["ba_fwd"], res["ba_vjp"], res["bt_fwd"], res["bt_vjp"]),
          flush=True)
