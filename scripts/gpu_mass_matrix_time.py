#!/usr/bin/env python3
"""Device time of the joint-space mass matrix through dp_utils.mass_matrix: method="crba" (pd_pose_op PD_POSE_MASS_MATRIX, one launch;
backward its VJP kernel, one launch) against method="jacobian" (the comparison: op 17 on S * nqd * nb rows and plain torch, backward by
autograd through them) -- forward, and forward + backward under a random, not symmetric upstream gradient with poses, masses and
inertias all requiring one -- on the last frame's poses of a rollout, one state set per env: Laikago 4096 and human 1024 sets by
default (arguments: robot:sets ...), 100 steps.  Each measured piece is timed by the rule of gpu_common.timed, both methods in the same
run.  Also printed: the rows the jacobian path sends through op 17, the bytes of H, the kernels' own times (hip_backend.mass_matrix /
mass_matrix_vjp on prepared rows) and the largest difference between the two methods over sqrt(H_aa H_bb)."""
import sys
from gpu_common import FWD, timed
import numpy as np
import torch
from diffphys_amd import dp_utils, hip_backend, robots, sim, synth

cfgs = [(a.split(":")[0], int(a.split(":")[1])) for a in sys.argv[1:] if not a.startswith("--")] or [("laikago", 4096), ("human", 1024)]
dev = torch.device("cuda:0")


for name, bs in cfgs:
    tpl = robots.load_template(name)
    T = 100
    inp = synth.make_inputs(tpl, name, bs=bs, nsteps=T, seed=0, seqs=("mi-trot", "mi-spin"))
    env = sim.Model.from_template(tpl, bs, dev)
    dm = hip_backend.device_model(env)
    t = {k: torch.from_numpy(inp[k]).to(dev) for k in FWD}
    fos = list(inp["frame2step"])
    pos, _, _, _, _ = dm.rollout_forward(bs, T, inp["dt"], *[t[k] for k in FWD], frame2step=fos, out=dm.alloc_rollout(bs, T, len(fos), dev))
    nb, nqd = dm.nb, int(tpl["nqd"])
    poses = pos[-1].reshape(bs, nb, 7).contiguous()   # one state set per env
    mass = torch.from_numpy(np.asarray(tpl["body_mass"], np.float32).reshape(nb)).to(dev)
    inertia = torch.from_numpy(np.asarray(tpl["body_inertia"], np.float32).reshape(nb, 3, 3)).to(dev)
    g_out = torch.randn(bs, nqd, nqd, device=dev, generator=torch.Generator(device=dev).manual_seed(5))

    def both(method):
        leaves = [poses.clone().requires_grad_(True), mass.clone().requires_grad_(True), inertia.clone().requires_grad_(True)]

        def fwd_bwd():
            H = dp_utils.mass_matrix(leaves[0], leaves[1], leaves[2], env, method=method)
            return torch.autograd.grad(H, leaves, g_out)

        with torch.no_grad():
            t_f = timed(lambda: dp_utils.mass_matrix(poses, mass, inertia, env, method=method))
        return t_f, timed(fwd_bwd)

    crba_f, crba_fb = both("crba")
    jac_f, jac_fb = both("jacobian")
    table = hip_backend.env_joint_table(env, dev, "generalized")
    rows = torch.cat([poses.reshape(-1, 7), mass.repeat(bs)[:, None], inertia.reshape(nb, 9).repeat(bs, 1)], -1).contiguous()
    k_f = timed(lambda: hip_backend.mass_matrix(table, nb, rows))
    k_v = timed(lambda: hip_backend.mass_matrix_vjp(table, nb, rows, g_out))
    with torch.no_grad():
        a = dp_utils.mass_matrix(poses, mass, inertia, env, method="crba").double()
        b = dp_utils.mass_matrix(poses, mass, inertia, env, method="jacobian").double()
    dg = torch.diagonal(b, dim1=-2, dim2=-1).sqrt()
    diff = float(((a - b).abs() / (dg[:, :, None] * dg[:, None, :])).max())
    print("MASSMAT %-8s sets=%-5d nb=%d nqd=%d jacobian rows %d  H bytes %d  |  forward: crba %.4f ms  jacobian %.4f ms  |  forward + backward: "
          "crba %.4f ms  jacobian %.4f ms  |  kernels alone: fwd %.4f ms  vjp %.4f ms  |  crba - jacobian %.2e of sqrt(H_aa H_bb)" % (
              name, bs, nb, nqd, bs * nqd * nb, bs * nqd * nqd * 4, crba_f, jac_f, crba_fb, jac_fb, k_f, k_v, diff), flush=True)
