#!/usr/bin/env python3
"""The launch plan of the rollout kernels as the public binding reports it (DeviceModel.last_launch_info), for the six models of
tests/test_gpu_forward_only.py at every segment width, kernel family, numeric policy and a ladder of batch sizes.

  python scripts/record_launch_plan.py [--out tests/golden/launch_plan.json]

`record_model()` is what tests/test_gpu_launch_plan.py replays against the committed file: every int and every error text must be
equal.  Only the public binding is used, so the script runs unchanged against an older library (PPR_DIFFPHYS_LIB): record from the
build BEFORE a change to the host's launch path, replay after it.  The plan is a function of the device's compute-unit count, which
the file stores.
"""
import argparse
import json
import os
import pathlib
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "ppr-diffphys_amd"), os.path.join(ROOT, "tests")) if p not in sys.path]

import numpy as np  # noqa: E402
import torch  # noqa: E402

MODELS = ("laikago", "human", "quad", "toy", "laikago_toes", "laikago12k")  # the model keys of test_gpu_forward_only.CASES
WIDTHS = (16, 32, 64)
FAMILIES = (0, 1, 2)
POLICIES = ("stable", "literal")
# either side of the quad-lane thresholds (2 x CUs, 4 x CUs envs), of each step of the env groups per workgroup at widths 16 and 32, and of
# the compound robots' switch to the unsplit forward (4 x CUs env groups), on a 256-CU device
BATCHES = (1, 3, 512, 513, 1024, 1025, 2049, 3073, 4097)
NSTEPS, FRAMES = 2, [0, 2]
STEP_MAJOR = ("torques", "res_f", "refs")  # [T, bs * ...]; every other input is [bs * ...]


SEED_ENVS = 4  # envs whose inputs are made; larger batches repeat them (the plan does not depend on the values)


def repeat_envs(inp, bs):
    """the inputs of bs envs: those of the SEED_ENVS envs of `inp`, repeated (numpy, flat per env)"""
    from helpers import INPUT_NAMES

    out, reps = dict(inp), -(-bs // SEED_ENVS)
    for k in INPUT_NAMES:
        a = np.asarray(inp[k])
        if k in STEP_MAJOR:
            out[k] = np.ascontiguousarray(np.tile(a.reshape(a.shape[0], SEED_ENVS, -1), (1, reps, 1))[:, :bs].reshape(a.shape[0], -1))
        else:
            out[k] = np.ascontiguousarray(np.tile(a.reshape(SEED_ENVS, -1), (reps, 1))[:bs].reshape(-1))
    return out


def _info(dm, kind):
    i = dm.last_launch_info(kind)
    return [i["workgroups"], i["threads_per_wg"], i["lds_bytes_per_wg"], i["envs_per_wg"]]


def record_model(key, dev, tmp_path):
    from diffphys_amd import hip_backend
    from diffphys_amd.hip_backend import ADJOINT_INPUTS as BWD, ROLLOUT_INPUTS as FWD
    from test_gpu_forward_only import _inputs, _run_pair, _template

    tpl, robot = _template(key, tmp_path)
    dm = hip_backend.DeviceModel(tpl)
    inp = _inputs(tpl, robot, SEED_ENVS, NSTEPS)
    inp["frame2step"] = list(FRAMES)
    per_bs = {}
    for bs in BATCHES:
        sub = repeat_envs(inp, bs)
        t = {k: torch.from_numpy(sub[k]).to(dev) for k in set(FWD) | set(BWD)}
        seeds = (torch.zeros(len(FRAMES), bs * dm.nb, 7, device=dev), torch.zeros(len(FRAMES), bs * dm.nb, 6, device=dev))
        per_bs[bs] = (sub, t, seeds)
    rec = {"default_width": dm.segment_width(), "widths": {}}
    for w in WIDTHS:
        try:
            dm.set_segment_width(w)
        except RuntimeError as e:
            rec["widths"][str(w)] = {"error": str(e)}
            continue
        plans = {}
        for family in FAMILIES:
            dm.set_kernel_family(family)
            for policy in POLICIES:
                dm.set_numeric_policy(hip_backend.NUM_LITERAL if policy == "literal" else hip_backend.NUM_STABLE)
                for bs in BATCHES:
                    _, t, (adj_pos, adj_vel) = per_bs[bs]
                    ws = dm.rollout_forward(bs, NSTEPS, inp["dt"], *[t[k] for k in FWD], frame2step=FRAMES)[4]
                    dm.rollout_backward(bs, NSTEPS, inp["dt"], *[t[k] for k in BWD], FRAMES, ws, adj_pos, adj_vel)
                    plans["f%d-%s-bs%d" % (family, policy, bs)] = [_info(dm, 0), _info(dm, 1)]
        dm.set_kernel_family(0)
        dm.set_numeric_policy(hip_backend.NUM_STABLE)
        # forward-only, and the loss-evaluating forward with an FK ride (saving, then forward-only): the loss launches' redirect to the
        # split kernel shows at 4097 envs for the compound robots
        extra = {}
        for bs in (513, 4097):
            sub = per_bs[bs][0]
            extra["forward-only-bs%d" % bs] = list(_run_pair(dm, sub, dev, False)[1][1].values())
            extra["traj-loss-fk-bs%d" % bs] = [list(info.values()) for _, info in _run_pair(dm, sub, dev, True)]
        rec["widths"][str(w)] = {"plans": plans, "extra": extra}
    torch.cuda.synchronize()
    return rec


def record(dev, tmp_path, models=MODELS):
    """-> the fixture: {"cu_count": ..., "models": {key: {"default_width": w, "widths": {"16": {"error": text} | {"plans": ..., "extra": ...}}}}}"""
    out = {"cu_count": int(torch.cuda.get_device_properties(dev).multi_processor_count), "models": {}}
    for key in models:
        out["models"][key] = record_model(key, dev, pathlib.Path(tmp_path))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "launch_plan.json"))
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        rec = record(torch.device("cuda:0"), tmp)
    with open(args.out, "w") as fh:
        text = json.dumps(rec, indent=1, sort_keys=True)
        fh.write(re.sub(r"\[\s*([-\d][-\d,\s]*?)\s*\]", lambda m: "[" + re.sub(r"\s+", " ", m.group(1)) + "]", text) + "\n")  # int lists on one line
    print("recorded %d models on %d CUs -> %s" % (len(rec["models"]), rec["cu_count"], args.out))


if __name__ == "__main__":
    main()
