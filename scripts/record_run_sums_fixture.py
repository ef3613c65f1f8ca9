#!/usr/bin/env python3
"""GPU: records tests/golden/run_sums_parent.npz, the fixture of tests/test_gpu_run_sums.py -- per adjoint case, kernel family and gradient
tensor the distance of the loaded library's gradients from the float64 C oracle, and the quad-lane forward outputs of the `flat` case.
Run it on the library of the commit BEFORE a change to the contact waves' run sums:
  PPR_DIFFPHYS_LIB=<that build> PPR_DIFFPHYS_ANY_ABI=1 python scripts/record_run_sums_fixture.py [OUT.npz]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "ppr-diffphys_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from oracle import ref_c  # noqa: E402

ref_c.build()
import test_gpu_run_sums as t  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else t.FIXTURE
z = t.record(out)
for k in sorted(z):
    if k.startswith("d/"):
        print("%-36s %.3e" % (k, float(z[k])))
print("library", str(z["build_id"]), "->", out, os.path.getsize(out), "bytes")
