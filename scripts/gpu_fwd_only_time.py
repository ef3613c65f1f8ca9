#!/usr/bin/env python3
"""Device time of the saving forward against the forward-only one (workspace NULL: k_rollout_fwd SAVE = false) per (robot, bs, segw)
config, T = 100, HIP events around the last launch of back-to-back batches (as scripts/gpu_time.py).  Arguments: robot:bs:segw ...
(default: the configs of DESIGN.md's forward-only section).  --phys: also phys_model.forward() at the reference's 10 x 760 window with
grad enabled and under torch.no_grad() (wall time per call, synchronised).  Under rocprofv3 --kernel-trace --stats the two forward
kernels of a config carry different names (the SAVE template argument)."""
import sys, time
from gpu_common import FWD
import numpy as np, torch
from diffphys_amd import robots, synth, hip_backend

args = [a for a in sys.argv[1:] if not a.startswith("--")]
cfgs = [(a.split(":")[0], int(a.split(":")[1]), int(a.split(":")[2])) for a in args] or [
    ("laikago", 4096, 16), ("laikago", 512, 16), ("human", 1024, 32), ("quad", 8192, 32)]
dev = torch.device("cuda:0")
for name, bs, segw in cfgs:
    tpl = robots.load_template(name)
    T = 100
    inp = synth.make_inputs(tpl, name, bs=bs, nsteps=T, seed=0, seqs=("mi-trot", "mi-spin"))
    dm = hip_backend.DeviceModel(tpl); dm.set_segment_width(segw); dm.set_timing(True)
    t = {k: torch.from_numpy(inp[k]).to(dev) for k in FWD}
    fos = list(inp["frame2step"])
    res = {}
    for save in (True, False, True, False):   # interleaved: each mode twice
        bufs = dm.alloc_rollout(bs, T, len(fos), dev, backward=False, save_trajectory=save)
        ms = []
        for it in range(9):
            for _ in range(10):
                dm.rollout_forward(bs, T, inp["dt"], *[t[k] for k in FWD], frame2step=fos, out=bufs, save_trajectory=save)
            torch.cuda.synchronize()
            if it >= 4:
                ms.append(dm.last_kernel_ms(0))
        res.setdefault(save, []).append(float(np.median(ms)))
    s, f = np.median(res[True]), np.median(res[False])
    info = dm.last_launch_info(0)
    print("FWDONLY %-8s bs=%-6d segw=%-2d saving %.4f ms  forward-only %.4f ms  (%+.1f %%)  wg=%d threads=%d" % (
        name, bs, segw, s, f, 100 * (f - s) / s, info["workgroups"], info["threads_per_wg"]), flush=True)

if "--phys" in sys.argv:
    from test_gpu_workload import _model
    model, opts = _model("mi-pace", "fwdonly_time")
    model.reinit_envs(opts["num_envs"], frames_per_wdw=opts["frames_per_wdw"])
    model.eval()
    for grad in (True, False, True, False):
        with torch.set_grad_enabled(grad):
            for _ in range(3):
                model.forward()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                model.forward()
            torch.cuda.synchronize()
        print("PHYS forward %s: %.3f ms per call (10 envs x 760 steps)" % ("grad enabled" if grad else "no_grad     ", (time.perf_counter() - t0) / 20 * 1e3), flush=True)
