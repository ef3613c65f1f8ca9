#!/usr/bin/env python3
"""Device time of the joint-wrench op (pd_pose_op PD_POSE_JOINT_WRENCH), forward and VJP, on the frame states of a rollout -- Laikago
4096 and human 1024 by default (arguments: robot:bs ...), 100 steps, the first four frames, each with the controls of its step -- beside
the joint-coordinates op (pd_pose_op PD_POSE_JOINT_COORDS, rates measured: forward and VJP) on the SAME states.  Each measured piece is
timed by the rule of gpu_common.timed.  Also printed: the element count (frames x bs x nb), the bytes the two launches move, and the
largest difference between the op and the rollout's own jaf on those frames, over max |jaf|."""
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
    steps = [min(int(s), T - 1) for s in fos[:F]]
    idx = hip_backend.env_joint_slot_index(env, dev)

    def slots(x):   # [F, bs, nqd] -> [F * bs * nb, 3]
        return torch.cat([x, x.new_zeros(x.shape[:-1] + (1,))], -1).index_select(-1, idx).reshape(-1, 3)

    per_step = lambda k: t[k].view(T, bs, nqd)[steps]
    gain = lambda k: t[k].view(1, bs, nqd).expand(F, bs, nqd)
    state = torch.cat([pos, vel], -1)[:F].reshape(-1, 13).contiguous()
    rows = torch.cat([state, slots(per_step("torques")), slots(per_step("refs")), slots(gain("target_ke")), slots(gain("target_kd"))], 1).contiguous()
    n = rows.shape[0]
    jf_table, jc_table = hip_backend.env_joint_force_table(env, dev), hip_backend.env_joint_table(env, dev, "measured")
    g6 = torch.randn(n, 6, device=dev)
    g_q, g_qd = torch.randn(n // nb, dm.nq, device=dev), torch.randn(n // nb, nqd, device=dev)
    out = hip_backend.joint_wrench(jf_table, nb, rows)
    ref = jaf[:F].reshape(-1, 6)
    diff = float((out - ref).abs().max() / ref.abs().max())
    res = dict(jw_fwd=timed(lambda: hip_backend.joint_wrench(jf_table, nb, rows)),
               jw_vjp=timed(lambda: hip_backend.joint_wrench_vjp(jf_table, nb, rows, g6)),
               jc_fwd=timed(lambda: hip_backend.joint_coords(jc_table, nb, state)),
               jc_vjp=timed(lambda: hip_backend.joint_coords_vjp(jc_table, nb, state, g_q, g_qd)))
    print("JOINTWRENCH %-8s bs=%-5d frames=%d elements=%d bytes fwd %d vjp %d  joint wrench fwd %.4f ms  vjp %.4f ms  |  "
          "joint coords fwd %.4f ms  vjp %.4f ms  |  op against the rollout's jaf: %.2e of max |jaf|" % (
              name, bs, F, n, n * (25 + 6) * 4, n * (25 + 6 + 25) * 4, res["jw_fwd"], res["jw_vjp"], res["jc_fwd"], res["jc_vjp"], diff), flush=True)
