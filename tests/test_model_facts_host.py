"""Which robots have their adjoint kernels' model facts compiled in (hip_backend.model_facts, the device-free twin of csrc/pd_host.hip
model_facts: no limit gains on a revolute joint, a FREE root with at least six bodies behind it, at most four children per body, on top of
parent_frames_identity; tests/test_gpu_adjoint_model_facts.py holds the library to it), and how the switch reaches the library without a
new entry point."""
import ctypes
import os
import re

import numpy as np

from diffphys_amd import hip_backend, robots
from test_parent_frame_identity_host import turned

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def with_limit(tpl, dof, key="joint_limit_ke", value=50.0):
    out = dict(tpl)
    a = np.array(tpl[key], np.float32).reshape(-1).copy()
    a[dof] = value
    out[key] = a
    return out


def test_laikago_qualifies_and_what_breaks_each_fact():
    tpl = robots.load_template("laikago")
    nb = int(tpl["nb"])
    assert hip_backend.model_facts(tpl)
    # one finite joint limit: a gain on one dof, stiffness or damping
    assert not hip_backend.model_facts(with_limit(tpl, 8))
    assert not hip_backend.model_facts(with_limit(tpl, 8, "joint_limit_kd", 1.0))
    # bounds alone exert no force: the library looks at the gains (PdDevModel::has_limits)
    assert hip_backend.model_facts(with_limit(with_limit(tpl, 8, "joint_limit_lower", -0.1), 8, "joint_limit_upper", 0.1))
    # a body with five children: hang the first five jointed bodies that are not on the root yet onto it
    par = np.array(tpl["joint_parent"]).reshape(-1).copy()
    assert np.bincount(par[par >= 0], minlength=nb).max() <= 4
    five = dict(tpl)
    p5 = par.copy()
    p5[1:6] = 0
    five["joint_parent"] = p5
    assert np.bincount(p5[p5 >= 0], minlength=nb).max() >= 5
    assert hip_backend.parent_frames_identity(five) and not hip_backend.model_facts(five)
    # fewer than 7 bodies: the root and its first five
    small = {k: v for k, v in tpl.items()}
    small["nb"] = 6
    for k in ("joint_type", "joint_parent", "joint_q_start", "joint_qd_start"):
        small[k] = np.array(tpl[k]).reshape(-1)[:6].copy()
    small["joint_parent"] = np.minimum(small["joint_parent"], 4)
    for k in ("joint_X_p", "joint_X_c"):
        small[k] = np.array(tpl[k], np.float32).reshape(nb, 7)[:6].copy()
    assert hip_backend.parent_frames_identity(small) and not hip_backend.model_facts(small)


def test_everything_the_parent_frame_test_rejects_is_rejected():
    tpl = robots.load_template("laikago")
    rejected = [turned(tpl, 5, 1e-3), turned(tpl, 5, 1e-3, key="joint_X_c"), robots.load_template("human"), robots.load_template("quad")]
    neg = dict(tpl)
    X = np.array(tpl["joint_X_p"], np.float32).reshape(-1, 7).copy()
    X[3, 3] = -0.0
    neg["joint_X_p"] = X
    rejected.append(neg)
    for t in rejected:
        assert not hip_backend.parent_frames_identity(t) and not hip_backend.model_facts(t)
    assert hip_backend.model_facts(turned(tpl, 0, 0.3))   # (the FREE root's frame is no joint frame of the revolute code)


def test_the_switch_adds_no_entry_point():
    lib = hip_backend.lib()
    hdr = open(os.path.join(ROOT, "include", "ppr_diffphys.h")).read()
    assert int(re.search(r"#define PD_PFI_GENERAL (\d+)", hdr).group(1)) == 4 and int(re.search(r"#define PD_PFI_SPECIALISED (\d+)", hdr).group(1)) == 8
    assert int(re.search(r"#define PD_LAUNCH_INFO_PARENT_FRAMES (\d+)", hdr).group(1)) == 2
    assert int(re.search(r"#define PD_PFI_NO_FACTS (\d+)", hdr).group(1)) == 16
    assert lib.pd_abi_version() == 9
    for name in ("pd_model_set_model_facts", "pd_model_get_model_facts", "pd_model_set_facts"):
        assert not hasattr(lib, name)
    declared = sorted(set(re.findall(r"\b(pd_[A-Za-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert len(declared) == 34 and all(hasattr(lib, n) for n in declared), declared
    info = (ctypes.c_int * 4)()
    assert lib.pd_model_set_kernel_family(None, 1 + 8 + 16) != 0 and lib.pd_last_launch_info(None, 2, ctypes.byref(info)) != 0
