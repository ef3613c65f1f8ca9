#!/usr/bin/env python3
"""Device time of a rollout launch with zero torques / res_f given as tensors against the same launch with NULL for both (the forward
kernels' zero-controls twins, k_rollout_fwd ZC = true; the adjoint's selective twins with the load of torques behind its test) -- forward
and adjoint separately, per (robot, bs, segw, family) config, T = 100: HIP events around the last launch of back-to-back batches
(pd_last_kernel_ms, as scripts/gpu_time.py), the two modes interleaved, 10 samples each; median and spread (min .. max) per mode.
Arguments: robot:bs:segw:family ... (default: the configs of DESIGN.md's zero-controls section).  The outputs of the two modes are
compared (torch.equal) before anything is timed.

One process, no retries: any error ends it.  Run it under a time limit of its own, e.g.
    timeout -k 10 600 python scripts/gpu_zero_controls_time.py
Under rocprofv3 --kernel-trace --stats (a run of its own) the twins carry their own names (the last template argument)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "ppr-diffphys_amd"))
import numpy as np, torch
from diffphys_amd import robots, synth, hip_backend

args = [a for a in sys.argv[1:] if not a.startswith("--")]
cfgs = [tuple([a.split(":")[0]] + [int(x) for x in a.split(":")[1:]]) for a in args] or [
    ("laikago", 4096, 16, 1), ("laikago", 512, 64, 2), ("human", 1024, 32, 0), ("quad", 8192, 32, 0)]
dev = torch.device("cuda:0")
REST = ("target_ke", "target_kd", "body_inv_mass", "body_inertia", "body_inv_inertia")
print("library", hip_backend.build_id(), flush=True)
for name, bs, segw, family in cfgs:
    tpl = robots.load_template(name)
    T = 100
    inp = synth.make_inputs(tpl, name, bs=bs, nsteps=T, seed=0, seqs=("mi-trot", "mi-spin"))
    dm = hip_backend.DeviceModel(tpl); dm.set_segment_width(segw); dm.set_kernel_family(family); dm.set_timing(True)
    t = {k: torch.from_numpy(inp[k]).to(dev) for k in ("q_init", "qd_init", "refs", "adj_pos", "adj_vel") + REST}
    zeros = (torch.zeros(T, bs * dm.nqd, device=dev), torch.zeros(T, bs * dm.nb, 6, device=dev))
    fos = list(inp["frame2step"])
    MODES = (("zero tensors", zeros), ("NULL", (None, None)))
    bufs = {label: dm.alloc_rollout(bs, T, len(fos), dev) for label, _ in MODES}
    fwd = lambda label, c: dm.rollout_forward(bs, T, inp["dt"], t["q_init"], t["qd_init"], c[0], c[1], t["refs"], *[t[k] for k in REST],
                                              frame2step=fos, out=bufs[label])
    bwd = lambda label, c: dm.rollout_backward(bs, T, inp["dt"], t["q_init"], t["qd_init"], c[0], t["refs"], *[t[k] for k in REST], fos,
                                               bufs[label]["ws"], t["adj_pos"], t["adj_vel"], out=bufs[label])
    outs = {}
    for label, c in MODES:
        o = fwd(label, c)
        g = bwd(label, c)
        torch.cuda.synchronize()
        outs[label] = [x.clone() for x in o[:4]] + [g[k].clone() for k in sorted(g)]
    assert all(torch.equal(a, b) for a, b in zip(outs["zero tensors"], outs["NULL"])), "the two modes differ"
    del outs
    res = {}
    for kind, run in ((0, fwd), (1, bwd)):
        for label, c in MODES * 2:   # interleaved: each mode twice, five samples each time
            for it in range(9):
                for _ in range(10):
                    run(label, c)
                torch.cuda.synchronize()
                if it >= 4:
                    res.setdefault((kind, label), []).append(dm.last_kernel_ms(kind))
    for kind in (0, 1):
        info = dm.last_launch_info(kind)
        base = float(np.median(res[(kind, "zero tensors")]))
        for label, _ in MODES:
            v = np.asarray(res[(kind, label)])
            print("ZEROCTL %-8s bs=%-6d segw=%-2d family=%d  %-8s %-12s %.4f ms  (%.4f .. %.4f, %d samples)  %+.1f %%  wg=%d threads=%d" % (
                name, bs, segw, family, "adjoint" if kind else "forward", label, np.median(v), v.min(), v.max(), len(v),
                100 * (np.median(v) - base) / base, info["workgroups"], info["threads_per_wg"]), flush=True)
    del bufs, t, dm, zeros
