"""What the scripts/gpu_*.py share: the import path of a checkout, the rollout operand order, inputs on the device, the timing rule.
The scripts run as ``python scripts/x.py``, so ``from gpu_common import ...`` finds this file by name; importing it puts the
repository, the package and tests/ on sys.path."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "ppr-diffphys_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from diffphys_amd.hip_backend import ADJOINT_INPUTS as BWD, ROLLOUT_INPUTS as FWD  # noqa: E402,F401

SEEDED = FWD + ("adj_pos", "adj_vel")   # the operands of a forward + adjoint pair


def dev_inputs(inp, dev, names=SEEDED):
    """numpy rollout inputs -> dict of contiguous float32 tensors on the device"""
    return {k: torch.from_numpy(np.ascontiguousarray(inp[k], dtype=np.float32)).to(dev) for k in names}


def timed(fn, warm=4, keep=5):
    """The timing rule of the per-op scripts: HIP events around each call of fn (whatever it enqueues), a synchronisation after each,
    ``warm`` warm-up rounds discarded, the median of the next ``keep`` -> milliseconds.  (scripts/gpu_time.py measures something else:
    batches enqueued back to back, and the kernels' own pd_last_kernel_ms.)"""
    ms = []
    for it in range(warm + keep):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        if it >= warm:
            ms.append(a.elapsed_time(b))
    return float(np.median(ms))
