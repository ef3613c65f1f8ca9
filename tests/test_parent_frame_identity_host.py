"""Which robots qualify for the adjoint kernels of unrotated parent-side joint frames (hip_backend.parent_frames_identity, the device-free
twin of csrc/pd_host.hip parent_frames_identity; tests/test_gpu_parent_frame_identity.py holds the library to it on both robots used
here), and how the choice reaches the library without a new entry point."""
import ctypes
import os
import re

import numpy as np

from diffphys_amd import hip_backend, robots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def turned(tpl, body, angle, key="joint_X_p"):
    """a copy of the template with that body's joint frame turned by `angle` rad about x"""
    out = dict(tpl)
    X = np.array(tpl[key], np.float32).reshape(int(tpl["nb"]), 7).copy()
    X[body, 3:] = [np.sin(angle / 2), 0.0, 0.0, np.cos(angle / 2)]
    out[key] = X
    return out


def test_laikago_qualifies_and_a_turned_parent_frame_does_not():
    tpl = robots.load_template("laikago")
    assert hip_backend.parent_frames_identity(tpl)
    X_p = np.asarray(tpl["joint_X_p"], np.float32).reshape(-1, 7)
    assert (X_p[1:, 3:] == [0, 0, 0, 1]).all() and np.abs(X_p[1:, :3]).max() > 0   # (translations are free)
    t = turned(tpl, 5, 1e-3)
    assert np.asarray(t["joint_X_p"]).reshape(-1, 7)[5, 3] != 0   # 1e-3 rad survives float32
    assert not hip_backend.parent_frames_identity(t)
    # the FREE root's frame is not a joint frame of the revolute code: it may carry anything
    assert hip_backend.parent_frames_identity(turned(tpl, 0, 0.3))
    # bit for bit: a frame that is the identity by value but not by bits (-0) stays with the general kernels
    neg = dict(tpl)
    X = X_p.copy(); X[3, 3] = -0.0
    neg["joint_X_p"] = X
    assert not hip_backend.parent_frames_identity(neg)
    # not a PLAIN revolute-only model: a turned child frame, another joint type
    assert not hip_backend.parent_frames_identity(turned(tpl, 5, 1e-3, key="joint_X_c"))
    for name in ("human", "quad"):
        assert not hip_backend.parent_frames_identity(robots.load_template(name))


def test_the_switch_adds_no_entry_point():
    lib = hip_backend.lib()
    hdr = open(os.path.join(ROOT, "include", "ppr_diffphys.h")).read()
    assert int(re.search(r"#define PD_PFI_GENERAL (\d+)", hdr).group(1)) == 4 and int(re.search(r"#define PD_PFI_SPECIALISED (\d+)", hdr).group(1)) == 8
    assert int(re.search(r"#define PD_LAUNCH_INFO_PARENT_FRAMES (\d+)", hdr).group(1)) == 2
    assert not hasattr(lib, "pd_model_set_parent_frame_identity")
    info = (ctypes.c_int * 4)()
    assert lib.pd_model_set_kernel_family(None, 1 + 8) != 0 and lib.pd_last_launch_info(None, 2, ctypes.byref(info)) != 0
