"""Wall time (device events) of ForwardWarp forward + backward, Laikago, single launch against the checkpointed adjoint
(self.checkpoint_steps = K): python scripts/gpu_checkpoint_time.py [--bs 4096] [--T 2000] [--K 50 200 1000] [--reps 3]"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ppr-diffphys_amd")):
    sys.path.insert(0, p)

from diffphys_amd import dp_model, hip_backend, robots, synth  # noqa: E402


class Host:
    pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, default=4096)
    ap.add_argument("--T", type=int, default=2000)
    ap.add_argument("--K", type=int, nargs="*", default=[50, 200, 1000])
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    tpl = robots.load_template("laikago")
    T0 = 100
    R = -(-a.T // T0)
    inp = synth.make_inputs(tpl, "laikago", bs=a.bs, nsteps=T0, seed=21, seqs=("mi-trot", "mi-spin"), penetration=0.003)
    t = {k: torch.from_numpy(np.ascontiguousarray(inp[k], dtype=np.float32)).to(dev) for k in synth.INPUT_NAMES}
    for k in ("torques", "res_f", "refs"):
        t[k] = t[k].repeat((R,) + (1,) * (t[k].dim() - 1))[: a.T].contiguous()
    f2s = list(range(0, a.T + 1, max(a.T // 10, 1)))
    h = Host()
    h.env = robots.env_from_template("laikago", a.bs, device=dev)
    h.num_envs, h.steps_idx, h.frame2step, h.dt = a.bs, range(a.T), f2s, inp["dt"]
    x = [t[k].requires_grad_(True) for k in synth.INPUT_NAMES]
    print("library", hip_backend.build_id(), "| laikago %d envs x %d steps, %d frames" % (a.bs, a.T, len(f2s)))
    base = None
    for K in [None] + list(a.K):
        h.checkpoint_steps = K
        ms = []
        for rep in range(a.reps + 1):
            for v in x:
                v.grad = None
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
            pos, vel = dp_model.ForwardWarp.apply(*x, h)
            e1.record()
            (pos.sum() + vel.sum()).backward()
            e2.record()
            torch.cuda.synchronize()
            if rep:  # the first pass warms up (frame tables, allocator)
                ms.append((e0.elapsed_time(e1), e1.elapsed_time(e2)))
        f, b = min(m[0] for m in ms), min(m[1] for m in ms)
        base = base or (f + b)
        print("checkpoint_steps %-5s forward %8.1f ms  backward %8.1f ms  total %8.1f ms  = %.3f ms / step, %.2f x the single launch"
              % (K, f, b, f + b, (f + b) / a.T, (f + b) / base))


if __name__ == "__main__":
    main()
