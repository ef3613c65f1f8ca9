#!/usr/bin/env python3
"""Host cost of one rollout call: N back-to-back DeviceModel.rollout_forward calls of a tiny rollout (Laikago, bs = 4, nsteps = 1: the
kernel is over before the next call is enqueued) into preallocated buffers, one synchronise at the end -> microseconds per call.  What
is timed is the binding's argument marshalling, the library's validation and launch plan, and the HIP launch.

  gpu_host_path.py [--calls 2000]                          one run of the tree's library (or PPR_DIFFPHYS_LIB)
  gpu_host_path.py --libs A.so B.so [--repeats 5]          A/B: --repeats runs of each library, interleaved, each in a fresh process;
                                                           prints every figure, then per library the median and min .. max, and
                                                           whether the LAST library's median lies inside the FIRST one's spread
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "ppr-diffphys_amd")]


def one_run(calls):
    import torch
    from diffphys_amd import hip_backend, robots, synth

    dev = torch.device("cuda:0")
    tpl = robots.load_template("laikago")
    bs, T = 4, 1
    inp = synth.make_inputs(tpl, "laikago", bs=bs, nsteps=T, seed=0)
    dm = hip_backend.DeviceModel(tpl)
    args = [torch.from_numpy(inp[k]).to(dev) for k in hip_backend.ROLLOUT_INPUTS]
    f2s = list(inp["frame2step"])
    bufs = dm.alloc_rollout(bs, T, len(f2s), dev, backward=False)
    for _ in range(200):
        dm.rollout_forward(bs, T, inp["dt"], *args, frame2step=f2s, out=bufs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        dm.rollout_forward(bs, T, inp["dt"], *args, frame2step=f2s, out=bufs)
    torch.cuda.synchronize()
    us = (time.perf_counter() - t0) / calls * 1e6
    print("HOSTPATH %s %d calls: %.2f us / call" % (hip_backend.build_id(), calls, us), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--libs", nargs="+", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if not a.libs:
        return one_run(a.calls)
    us = {lib: [] for lib in a.libs}
    for _ in range(a.repeats):
        for lib in a.libs:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--calls", str(a.calls)], env=dict(os.environ, PPR_DIFFPHYS_LIB=lib),
                                 check=True, capture_output=True, text=True, timeout=300).stdout
            line = next(ln for ln in out.splitlines() if ln.startswith("HOSTPATH"))
            print(lib, line, flush=True)
            us[lib].append(float(line.split(":")[-1].split()[0]))
    for lib, v in us.items():
        print("HOSTPATH-AB %s: median %.2f us / call (min %.2f .. max %.2f, %d runs)" % (lib, statistics.median(v), min(v), max(v), len(v)))
    first, last = us[a.libs[0]], us[a.libs[-1]]
    inside = min(first) <= statistics.median(last) <= max(first)
    print("HOSTPATH-AB median of %s is %s the min .. max of %s" % (a.libs[-1], "inside" if inside else "OUTSIDE", a.libs[0]))


if __name__ == "__main__":
    main()
