#!/usr/bin/env python3
"""Device time of the 2D keypoint projection and its vector-Jacobian product (dp_utils.project_bodies: pd_pose_op PD_POSE_PROJECT, one launch
each way) beside the torch composition of the same formula (the reference's project_bodies: parse_rtk, two batched matmuls, a division, and
autograd's backward of that), at the two shapes the rollout is run at: Laikago 4096 envs x 4 frames x 13 bodies and 10 x 24 x 13.
    python scripts/gpu_reproj_time.py [repeats]
The two are timed in turns, `repeats` blocks each (device events around 200 forward + backward pairs per block); medians and min .. max."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "ppr-diffphys_amd"))
import numpy as np
import torch

from diffphys_amd import dp_utils

assert torch.cuda.is_available(), "needs a GPU"
dev = torch.device("cuda:0")
REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
INNER = 200


def torch_project(bodies, rtk):  # the reference's lines (dp_utils.py:200-214)
    point = bodies[..., :3]
    rtmat, kmat = dp_utils.parse_rtk(rtk)
    rtmat, kmat = rtmat[..., None, :, :], kmat[..., None, :, :]
    point = torch.cat([point, torch.ones_like(point[..., :1])], -1)
    point = (rtmat @ point[..., None])[..., :3, :]
    point = kmat @ point
    return point[..., :2, 0] / point[..., 2:3, 0]


def block(fn, bodies, rtk, w):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(INNER):
        bodies.grad = None
        (fn(bodies, rtk) * w).sum().backward()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / INNER * 1e3   # us per forward + backward


for bs, F, nb in ((4096, 4, 13), (10, 24, 13)):
    g = torch.Generator().manual_seed(0)
    bodies = torch.randn(bs, F, nb, 7, generator=g).to(dev).requires_grad_(True)
    rtk = torch.randn(bs, F, 4, 4, generator=g)
    rtk[..., 2, :3] *= 0.1   # every point in front of its camera
    rtk[..., 2, 3] = rtk[..., 2, 3].abs() + 3.0
    rtk = rtk.to(dev)
    w = torch.randn(bs, F, nb, 2, generator=g).to(dev)
    a, b = dp_utils.project_bodies(bodies, rtk), torch_project(bodies, rtk)
    print("%d x %d x %d: HIP vs torch composition, values max |d| / max(1, |x|) = %.1e" % (
        bs, F, nb, float(((a - b).abs() / b.abs().clamp(min=1)).max())))
    fns = {"hip": dp_utils.project_bodies, "torch": torch_project}
    t = {k: [] for k in fns}
    for k, fn in fns.items():
        block(fn, bodies, rtk, w)   # warm-up of this shape
    for _ in range(REPEATS):
        for k, fn in fns.items():
            t[k].append(block(fn, bodies, rtk, w))
    for k in fns:
        v = np.asarray(t[k])
        print("REPROJ %-5s %5d x %2d x %2d: forward + backward (incl. the weighted sum and its backward) %.1f us, median of %d (%.1f .. %.1f)" % (
            k, bs, F, nb, np.median(v), len(v), v.min(), v.max()), flush=True)
    # the two launches alone, without autograd around them
    from diffphys_amd import hip_backend as hb

    bd, go = bodies.detach(), w
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    v = []
    for _ in range(REPEATS + 1):
        e[0].record()
        for _ in range(INNER):
            hb.pose_op(3, rtk, bd)
            hb.pose_op_vjp(3, rtk, bd, go, need_a=False)
        e[1].record()
        torch.cuda.synchronize()
        v.append(e[0].elapsed_time(e[1]) / INNER * 1e3)
    v = np.asarray(v[1:])
    print("REPROJ launches %5d x %2d x %2d: pd_pose_op + pd_pose_op_vjp (g_b only) %.1f us, median of %d (%.1f .. %.1f)" % (
        bs, F, nb, np.median(v), len(v), v.min(), v.max()), flush=True)
