#!/usr/bin/env python3
"""Checking build of the global-memory contact tables: a library built with -DPD_GLOBAL_TABLES (`make -C ppr-diffphys_amd/csrc
globaltables`) puts EVERY model's contact tables in global memory -- the kernels' GT instantiations, the launches without the tables'
LDS.  The arithmetic is the same, only the tables' address space differs, so on the inputs of tests/test_gpu_tight.py::
test_against_frozen_bits (golden + the 8-env x 100-step batch; laikago, human, quad; lane-per-body and, for Laikago, quad-lane kernels)
it must give the product library's bits: outputs and every gradient.  Each library runs in a fresh process (hip_backend._LIB_PATH set
before the library is loaded).  Run on the GPU box after both builds; prints one line per (robot, family, input) and exits 1 on a
difference.
usage: check_global_tables.py [robot ...]"""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_DIR = os.path.join(ROOT, "ppr-diffphys_amd", "diffphys_amd", "lib")
PRODUCT = os.path.join(LIB_DIR, "libpprdiffphys_hip.so")
CHECKING = os.path.join(LIB_DIR, "libpprdiffphys_hip_globaltables.so")
CASES = [("laikago", 1), ("laikago", 2), ("human", 1), ("quad", 1)]


def worker(lib_path, out_path, names):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "ppr-diffphys_amd"), os.path.join(ROOT, "tests")]
    import numpy as np
    import torch

    from diffphys_amd import hip_backend

    hip_backend._LIB_PATH = lib_path   # before anything loads the library
    from helpers import golden_inputs, load_golden
    from gpu_harness import gpu_rollout
    from diffphys_amd import robots, synth

    dev = torch.device("cuda:0")
    rec = {}
    for name, family in CASES:
        if name not in names:
            continue
        tpl = robots.load_template(name)
        dm = hip_backend.DeviceModel(tpl)
        dm.set_kernel_family(family)
        for tag, inp in (("golden", golden_inputs(load_golden(name))),
                         ("bench8", synth.make_env_inputs(tpl, name, range(8), 100, seed=77, seqs=("mi-trot", "mi-spin"), penetration=0.002))):
            out = gpu_rollout(dm, inp, dev)
            key = "%s/%d/%s/" % (name, family, tag)
            for k in ("wp_pos", "wp_vel", "grf", "jaf"):
                rec[key + k] = out[k]
            for k, v in out["grads"].items():
                rec[key + "grad_" + k] = v
            rec[key + "lds_fwd"] = np.int64(dm.last_launch_info(0)["lds_bytes_per_wg"])
    np.savez(out_path, **rec)


def main(names):
    import numpy as np

    for p in (PRODUCT, CHECKING):
        if not os.path.exists(p):
            sys.exit("missing %s: build it first (make -C ppr-diffphys_amd/csrc; make -C ppr-diffphys_amd/csrc globaltables)" % p)
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for which, lib in (("product", PRODUCT), ("globaltables", CHECKING)):
            out = os.path.join(tmp, which + ".npz")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", lib, out] + names, check=True, timeout=900)
            with np.load(out) as z:
                res[which] = {k: z[k] for k in z.files}
    a, b = res["product"], res["globaltables"]
    assert sorted(a) == sorted(b)
    bad = 0
    for case in sorted({k.rsplit("/", 1)[0] for k in a}):
        keys = [k for k in a if k.startswith(case + "/") and not k.endswith("lds_fwd")]
        diff = [k.rsplit("/", 1)[1] for k in keys if not np.array_equal(a[k], b[k])]
        bad += len(diff)
        print("%-22s %2d tensors: %s   (forward LDS per workgroup %d B -> %d B)" % (
            case, len(keys), "bit-identical" if not diff else "DIFFER: " + ", ".join(diff), int(a[case + "/lds_fwd"]), int(b[case + "/lds_fwd"])))
    print("global-tables checking build vs product library: %s" % ("bit-identical" if bad == 0 else "%d tensors differ" % bad))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--worker":
        worker(sys.argv[2], sys.argv[3], sys.argv[4:] or ["laikago", "human", "quad"])
    else:
        sys.exit(main(sys.argv[1:] or ["laikago", "human", "quad"]))
