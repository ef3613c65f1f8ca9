#!/usr/bin/env python3
"""Device time of the mass-matrix-inverse op (pd_pose_op PD_POSE_MASS_INVERSE) -- forward, and the composed backward of
dp_model.MassInverse (op 21 once more, op 17 forward on the stacked sets, op 17 VJP, M_b in torch) -- on the frame poses of a rollout,
the measured joint rates of the same frames standing in for the joint-space forces -- Laikago 4096 and human 1024 by default (arguments:
robot:bs ...), 100 steps, the first four frames -- beside the body-twist op (pd_pose_op PD_POSE_BODY_TWIST: forward and VJP) on the same
frames in the same run, and dp_utils.forward_dynamics dense against articulated on the same state sets (halved until the dense path fits
in memory).  Each measured piece is timed by the rule of gpu_common.timed.  Also printed: the element count (frames x bs x nb), the bytes
the forward launch moves and the largest difference between the two forward-dynamics paths."""
import sys
from gpu_common import FWD, timed
import numpy as np
import torch
from diffphys_amd import dp_model, dp_utils, hip_backend, robots, sim, synth

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
    S = n // nb
    table = hip_backend.env_joint_table(env, dev, "generalized")
    _, jqd = hip_backend.joint_coords(table, nb, state)
    slots = torch.cat([jqd, jqd.new_zeros(S, 1)], -1).index_select(-1, hip_backend.env_joint_rate_slot_index(env, dev)).reshape(n, 6)
    mass = torch.from_numpy(np.asarray(tpl["body_mass"], np.float32).reshape(nb)).to(dev)
    inertia = torch.from_numpy(np.asarray(tpl["body_inertia"], np.float32).reshape(nb, 3, 3)).to(dev)
    rows23 = torch.cat([state[:, :7], mass.repeat(S)[:, None], inertia.reshape(nb, 9).repeat(S, 1), slots], -1).contiguous()
    rows13 = torch.cat([state[:, :7], slots], -1).contiguous()
    g_out = torch.randn(n, 6, device=dev)
    bq = state[:, :7].reshape(S, nb, 7).clone().requires_grad_(True)
    m_s, i_s = mass.expand(S, nb).clone().requires_grad_(True), inertia.expand(S, nb, 3, 3).clone().requires_grad_(True)
    r6 = slots.reshape(S, nb, 6).clone().requires_grad_(True)
    out = dp_model.MassInverse.apply(bq, m_s, i_s, r6, env, "generalized")
    out_r = dp_model.MassInverse.apply(bq.detach(), m_s.detach(), i_s.detach(), r6, env, "generalized")   # the slots alone need a gradient
    res = dict(mi_fwd=timed(lambda: hip_backend.mass_inverse(table, nb, rows23)),
               mi_bwd=timed(lambda: torch.autograd.grad(out, (bq, m_s, i_s, r6), g_out.view(S, nb, 6), retain_graph=True)),
               mi_bwd_r=timed(lambda: torch.autograd.grad(out_r, (r6,), g_out.view(S, nb, 6), retain_graph=True)),
               bt_fwd=timed(lambda: hip_backend.body_twists(table, nb, rows13)),
               bt_vjp=timed(lambda: hip_backend.body_twists_vjp(table, nb, rows13, g_out)))
    print("MASSINV %-8s bs=%-5d frames=%d elements=%d bytes fwd %d  mass inverse fwd %.4f ms  composed backward %.4f ms (slots alone %.4f ms)"
          "  |  body twists fwd %.4f ms  vjp %.4f ms" % (
              name, bs, F, n, n * (23 + 6) * 4, res["mi_fwd"], res["mi_bwd"], res["mi_bwd_r"], res["bt_fwd"], res["bt_vjp"]), flush=True)
    del out, out_r, bq, m_s, i_s, r6
    sets = S
    while sets >= 1:   # forward dynamics on the same sets: the dense path builds S * nqd * nb Jacobian rows and an [S, nqd, nqd] solve
        q, v = state[: sets * nb, :7].reshape(sets, nb, 7), jqd[:sets].contiguous()
        tau = torch.randn(sets, jqd.shape[-1], device=dev, generator=torch.Generator(device=dev).manual_seed(3))
        try:
            dense = dp_utils.forward_dynamics(q, v, tau, mass, inertia, env)
            t_dense = timed(lambda: dp_utils.forward_dynamics(q, v, tau, mass, inertia, env))
        except torch.cuda.OutOfMemoryError:
            sets //= 2
            continue
        art = dp_utils.forward_dynamics(q, v, tau, mass, inertia, env, method="articulated")
        t_art = timed(lambda: dp_utils.forward_dynamics(q, v, tau, mass, inertia, env, method="articulated"))
        t_bias = timed(lambda: dp_utils.bias_forces(q, v, mass, inertia, env))
        print("MASSINV %-8s forward_dynamics on %d sets: dense %.4f ms  articulated %.4f ms (bias_forces alone %.4f ms)  largest difference "
              "%.2e of max |qdd| %.3g" % (name, sets, t_dense, t_art, t_bias, float((dense - art).abs().max() / art.abs().max()),
                                          float(art.abs().max())), flush=True)
        break
