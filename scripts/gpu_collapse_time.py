#!/usr/bin/env python3
"""Forward + adjoint kernel times of laikago_toes (tests/golden/template_laikago_toes.npz) as compiled against the same robot with its
fixed toe joints collapsed (sim.collapse_fixed_joints), on one library build, the two models alternating.  Warm-up and median rule of
scripts/gpu_time.py: batches of ten forward + adjoint pairs enqueued back to back, the last launches of each batch timed by HIP events,
the first batches discarded.  Prints the chosen kernels' geometry (DeviceModel.last_launch_info) and default widths.

    python scripts/gpu_collapse_time.py [bs ...]          # default 4096 512, 100 steps
"""
import os
import sys

from gpu_common import BWD, FWD, ROOT
import numpy as np, torch
from diffphys_amd import hip_backend, sim, synth

dev = torch.device("cuda:0")
with np.load(os.path.join(ROOT, "tests", "golden", "template_laikago_toes.npz")) as z:
    orig = {k: z[k] for k in z.files}
models = {"original": orig, "collapsed": sim.collapse_fixed_joints(orig)[0]}
T = 100
for bs in [int(a) for a in sys.argv[1:]] or [4096, 512]:
    runs = {}
    for key, tpl in models.items():
        inp = synth.make_inputs(tpl, "laikago", bs=bs, nsteps=T, seed=0, seqs=("mi-trot", "mi-spin"))
        dm = hip_backend.DeviceModel(tpl)
        dm.set_timing(True)
        t = {k: torch.from_numpy(inp[k]).to(dev) for k in synth.INPUT_NAMES}
        fos = list(inp["frame2step"])
        runs[key] = dict(dm=dm, dt=inp["dt"], fos=fos, fa=[t[k] for k in FWD], ba=[t[k] for k in BWD], ap=torch.from_numpy(inp["adj_pos"]).to(dev),
                         av=torch.from_numpy(inp["adj_vel"]).to(dev), bufs=dm.alloc_rollout(bs, T, len(fos), dev), f=[], b=[])
    for it in range(9):
        for key, r in runs.items():   # alternating: both models see the same clocks
            for _ in range(10):
                out = r["dm"].rollout_forward(bs, T, r["dt"], *r["fa"], frame2step=r["fos"], out=r["bufs"])
                r["dm"].rollout_backward(bs, T, r["dt"], *r["ba"], r["fos"], out[4], r["ap"], r["av"], out=r["bufs"])
            torch.cuda.synchronize()
            if it >= 4:
                r["f"].append(r["dm"].last_kernel_ms(0)); r["b"].append(r["dm"].last_kernel_ms(1))
    for key, r in runs.items():
        dm, f, b = r["dm"], np.median(r["f"]), np.median(r["b"])
        print("TIMING laikago_toes %-9s bs=%-5d nb=%d width %d quad-eligible %d fwd %.3f ms bwd %.3f ms -> %.3e env-steps/s; fwd launch %s; bwd launch %s" % (
            key, bs, dm.nb, dm.segment_width(), dm.kernel_family()[1], f, b, bs * T / ((f + b) * 1e-3), dm.last_launch_info(0), dm.last_launch_info(1)), flush=True)
