"""Which robots have their centre-of-mass facts compiled into the adjoint kernels (hip_backend.com_facts, the device-free twin of
csrc/pd_host.hip com_facts: on top of model_facts, every body_com has x == 0 and y == 0 as fp32 (Z) and is (0, 0, 0) for every body whose
joint is not FREE (J0); tests/test_gpu_adjoint_com_facts.py holds the library to it), and how the switch reaches the library without a new
entry point."""
import ctypes
import os
import re

import numpy as np

from diffphys_amd import hip_backend, robots
from test_model_facts_host import with_limit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def with_com(tpl, body, axis, value):
    out = dict(tpl)
    com = np.array(tpl["body_com"], np.float32).reshape(-1, 3).copy()
    com[body, axis] = value
    out["body_com"] = com
    return out


def test_laikago_qualifies_and_what_breaks_each_fact():
    tpl = robots.load_template("laikago")
    nb = int(tpl["nb"])
    com = np.asarray(tpl["body_com"], np.float32).reshape(nb, 3)
    assert (com[:, :2] == 0).all() and com[0, 2] != 0 and (com[1:] == 0).all()   # the trunk's com on its z axis, the legs' at the origin
    assert hip_backend.com_facts(tpl)
    assert not hip_backend.com_facts(with_com(tpl, 3, 0, 1e-3))   # Z: an x component
    assert not hip_backend.com_facts(with_com(tpl, 0, 1, 1e-3))   # Z: a y component, on the FREE root too
    assert not hip_backend.com_facts(with_com(tpl, 5, 2, 1e-3))   # J0: a jointed body's com on its z axis
    assert hip_backend.com_facts(with_com(tpl, 0, 2, -0.2))       # the FREE root's z is free
    assert hip_backend.com_facts(with_com(tpl, 5, 2, -0.0))       # a negative zero is a zero
    # a value that is zero only after the conversion the device copy goes through
    tiny = np.array(tpl["body_com"], np.float64).reshape(nb, 3).copy()
    tiny[4, 0] = 1e-60
    assert hip_backend.com_facts(dict(tpl, body_com=tiny))
    # nothing that already fails model_facts qualifies
    limited = with_limit(tpl, 8)
    assert not hip_backend.model_facts(limited) and not hip_backend.com_facts(limited)
    for name in ("human", "quad"):
        assert not hip_backend.com_facts(robots.load_template(name))


def test_the_switch_adds_no_entry_point():
    lib = hip_backend.lib()
    hdr = open(os.path.join(ROOT, "include", "ppr_diffphys.h")).read()
    assert int(re.search(r"#define PD_PFI_NO_FACTS (\d+)", hdr).group(1)) == 16
    assert int(re.search(r"#define PD_PFI_NO_COM_FACTS (\d+)", hdr).group(1)) == 32
    assert int(re.search(r"#define PD_LAUNCH_INFO_PARENT_FRAMES (\d+)", hdr).group(1)) == 2
    assert lib.pd_abi_version() == 9
    for name in ("pd_model_set_com_facts", "pd_model_get_com_facts", "pd_model_com_facts"):
        assert not hasattr(lib, name)
    declared = sorted(set(re.findall(r"\b(pd_[A-Za-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert len(declared) == 34 and all(hasattr(lib, n) for n in declared), declared
    # a null model is refused by the new family flag and by the info call
    info = (ctypes.c_int * 4)()
    assert lib.pd_model_set_kernel_family(None, 1 + 32) != 0 and lib.pd_model_set_kernel_family(None, 1 + 8 + 16 + 32) != 0
    assert lib.pd_last_launch_info(None, 2, ctypes.byref(info)) != 0
