#!/usr/bin/env python3
"""Device time of the adjoint launch with all three per-step gradients against its selective twin (a NULL g_torques / g_res_f / g_refs:
k_rollout_bwd / k_rollout_bwd3 SEL = true) -- all three, the empty subset, res_f alone -- per (robot, bs, segw, family) config, T = 100:
HIP events around the last launch of back-to-back batches (pd_last_kernel_ms, as scripts/gpu_time.py), the modes interleaved, each
twice; median of the samples and their spread (min .. max) per mode.  Arguments: robot:bs:segw:family ... (default: the configs of
DESIGN.md's selective-adjoint section).  --warp [--bs 4096 --T 2000 --K 70]: also ForwardWarp forward + backward with the checkpointed
adjoint and its peak memory, for every input / target_ke only / res_f + target_ke requiring a gradient.

One process, no retries: any error ends it.  Run it under a time limit of its own, e.g.
    timeout -k 10 600 python scripts/gpu_grad_select_time.py --warp
Under rocprofv3 --kernel-trace --stats (a run of its own) the selective kernels carry their own names (the last template argument)."""
import sys
from gpu_common import BWD, FWD, dev_inputs
import numpy as np, torch
from diffphys_amd import dp_model, robots, synth, hip_backend


def opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


flags = ("--warp", "--bs", "--T", "--K")
args = [a for i, a in enumerate(sys.argv[1:], 1) if not a.startswith("--") and sys.argv[i - 1] not in flags[1:]]
cfgs = [tuple([a.split(":")[0]] + [int(x) for x in a.split(":")[1:]]) for a in args] or [
    ("laikago", 4096, 16, 1), ("laikago", 512, 64, 2), ("human", 1024, 32, 0), ("quad", 8192, 32, 0)]
dev = torch.device("cuda:0")
MODES = (("all three", hip_backend.GRAD_NAMES), ("none", ()), ("res_f only", ("res_f",)))
print("library", hip_backend.build_id(), flush=True)
for name, bs, segw, family in cfgs:
    tpl = robots.load_template(name)
    T = 100
    inp = synth.make_inputs(tpl, name, bs=bs, nsteps=T, seed=0, seqs=("mi-trot", "mi-spin"))
    dm = hip_backend.DeviceModel(tpl); dm.set_segment_width(segw); dm.set_kernel_family(family); dm.set_timing(True)
    t = {k: torch.from_numpy(inp[k]).to(dev) for k in FWD + ("adj_pos", "adj_vel")}
    fos = list(inp["frame2step"])
    ws = dm.rollout_forward(bs, T, inp["dt"], *[t[k] for k in FWD], frame2step=fos)[4]
    res = {}
    for label, want in MODES * 2:   # interleaved: each mode twice
        bufs = dict(grads=dm._alloc_grads(bs, T, dev, want=want))
        for it in range(9):
            for _ in range(10):
                dm.rollout_backward(bs, T, inp["dt"], *[t[k] for k in BWD], fos, ws, t["adj_pos"], t["adj_vel"], out=bufs, want=want)
            torch.cuda.synchronize()
            if it >= 4:
                res.setdefault(label, []).append(dm.last_kernel_ms(1))
    info = dm.last_launch_info(1)
    base = float(np.median(res["all three"]))
    for label, _ in MODES:
        v = np.asarray(res[label])
        print("GRADSEL %-8s bs=%-6d segw=%-2d family=%d  %-10s %.4f ms  (%.4f .. %.4f, %d samples)  %+.1f %%  wg=%d threads=%d" % (
            name, bs, segw, family, label, np.median(v), v.min(), v.max(), len(v), 100 * (np.median(v) - base) / base, info["workgroups"],
            info["threads_per_wg"]), flush=True)
    del ws, t, dm

if "--warp" in sys.argv:
    bs, T, K = opt("--bs", 4096), opt("--T", 2000), opt("--K", 70)
    tpl = robots.load_template("laikago")
    T0 = 100
    inp = synth.make_inputs(tpl, "laikago", bs=bs, nsteps=T0, seed=21, seqs=("mi-trot", "mi-spin"), penetration=0.003)
    t = dev_inputs(inp, dev, synth.INPUT_NAMES)
    for k in ("torques", "res_f", "refs"):
        t[k] = t[k].repeat((-(-T // T0),) + (1,) * (t[k].dim() - 1))[:T].contiguous()

    class Host:
        pass

    h = Host()
    h.env = robots.env_from_template("laikago", bs, device=dev)
    h.num_envs, h.steps_idx, h.frame2step, h.dt, h.checkpoint_steps = bs, range(T), list(range(0, T + 1, max(T // 10, 1))), inp["dt"], K
    per_step = T * bs * (2 * int(tpl["nqd"]) + 6 * int(tpl["nb"])) * 4
    print("WARP laikago %d envs x %d steps, checkpoint_steps = %d; the three per-step gradients are %.3f GB" % (bs, T, K, per_step / 1e9), flush=True)
    for label, needs in (("every input", synth.INPUT_NAMES), ("target_ke only", ("target_ke",)), ("res_f + target_ke", ("res_f", "target_ke"))) * 2:
        ms, peaks = [], []
        for rep in range(4):
            x = [t[k].detach().requires_grad_(k in needs) for k in synth.INPUT_NAMES]
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            m0 = torch.cuda.memory_allocated()
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            pos, vel = dp_model.ForwardWarp.apply(*x, h)
            e1.record()
            (pos.sum() + vel.sum()).backward()
            e2.record()
            torch.cuda.synchronize()
            if rep:  # the first pass warms up (frame tables, allocator)
                ms.append((e0.elapsed_time(e1), e1.elapsed_time(e2)))
                peaks.append(torch.cuda.max_memory_allocated() - m0)
            del x, pos, vel
        f, b = float(np.median([m[0] for m in ms])), float(np.median([m[1] for m in ms]))
        print("WARP %-18s forward %8.1f ms  backward %8.1f ms (%.1f .. %.1f)  peak above the inputs +%.3f GB" % (
            label, f, b, min(m[1] for m in ms), max(m[1] for m in ms), max(peaks) / 1e9), flush=True)
