#!/usr/bin/env python3
"""Compile the reference's URDF robots and AMP mocap files into small npz fixtures.

Run HERE (the container with /root/reference); outputs are committed:
  ppr-diffphys_amd/diffphys_amd/templates/{laikago,human,quad}.npz   articulation templates
  ppr-diffphys_amd/diffphys_amd/templates/mocap_laikago.npz          AMP frames of the 5 sequences

Opt-in target (not written by a plain run, so the outputs above are never rewritten by it):
  --laikago-toes   tests/golden/template_laikago_toes.npz: laikago_toes.urdf (full lower-leg collision mesh + toe spheres,
                   ~11 000 contact candidates) with Laikago's constants -- the test model of a robot whose contact tables do
                   not fit in LDS (tests/test_gpu_large_contact_sets.py).  robots.PRESETS has no such entry (the reference's
                   phys_model offers no such preset): the preset lives here, for this one compilation.
  --laikago-toes --collapse-fixed-joints --out PATH
                   the same robot with its four toe links welded into the lower legs (robots.make_env(collapse_fixed_joints=True)):
                   13 bodies, revolute-only.  The npz records that it was collapsed: it carries collapse_fixed_joints = True and the
                   map (collapse_kept / collapse_owner / collapse_X_rel, sim.CollapseMap.from_template); a template without these
                   keys was not collapsed.  No default path: the committed fixture is the uncollapsed one.

The npz files hold DATA only (flat arrays derived from the URDF / mesh / json
data files under /root/reference/data, Laikago meshes: PyBullet/Unitree
licence, see data/urdf_templates/laikago/license.txt there).  Nothing on the
GPU box reads /root/reference.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ppr-diffphys_amd"))
from diffphys_amd import robots  # noqa: E402

REF = os.environ.get("PPR_REFERENCE", "/root/reference")
# laikago_toes.urdf with the constants of the reference's "laikago" branch (dp_model.py:83-91): the same tuple as PRESETS["laikago"]
LAIKAGO_TOES = ("laikago/laikago_toes.urdf",) + robots.PRESETS["laikago"][1:]
LAIKAGO_TOES_OUT = os.path.join(ROOT, "tests", "golden", "template_laikago_toes.npz")


def _template(name, urdf_root, collapse_fixed_joints=False):
    env, art, info = robots.make_env(name, urdf_root, 1, device="cpu", collapse_fixed_joints=collapse_fixed_joints)
    tpl = env.template()
    tpl["body_names"] = np.asarray(info["body_names"])
    tpl["kp"] = np.float32(info["kp"])
    tpl["kd"] = np.float32(info["kd"])
    tpl["mass_rule"] = np.asarray(info["mass_rule"])  # which reading of dp_model.py:185-191 produced body_mass (robots.MASS_RULES)
    if collapse_fixed_joints:  # recorded only when set: every template compiled without the option keeps its keys and bits
        cmap = info["collapse_map"]
        tpl["collapse_fixed_joints"] = np.bool_(True)
        tpl["collapse_kept"], tpl["collapse_owner"], tpl["collapse_X_rel"] = cmap.kept, cmap.owner, cmap.X_rel
    return tpl


def compile_laikago_toes(ref=REF, collapse_fixed_joints=False):
    """The laikago_toes template as a dict of arrays (what --laikago-toes writes); robots.PRESETS is left as it was."""
    saved = robots.PRESETS
    robots.PRESETS = dict(saved, laikago_toes=LAIKAGO_TOES)
    try:
        return _template("laikago_toes", os.path.join(ref, "data/urdf_templates"), collapse_fixed_joints)
    finally:
        robots.PRESETS = saved


def main():
    out = robots.TEMPLATE_DIR
    os.makedirs(out, exist_ok=True)
    for name in ("laikago", "human", "quad"):
        tpl = _template(name, os.path.join(REF, "data/urdf_templates"))
        np.savez_compressed(os.path.join(out, name + ".npz"), **tpl)
        print(
            "%-8s nb=%d nq=%d nqd=%d Nc=%d mass=%s"
            % (name, tpl["nb"], tpl["nq"], tpl["nqd"], len(tpl["contact_body"]), np.round(tpl["body_mass"], 3)[:6])
        )
    mocap = {}
    for seq in ("mi-pace", "mi-trot", "mi-spin", "mi-turn", "mi-sidesteps"):
        with open(os.path.join(REF, "data/motion_sequences/%s/amp-%s.txt" % (seq, seq))) as f:
            d = json.load(f)
        mocap[seq + "/frames"] = np.asarray(d["Frames"], dtype=np.float64)
        mocap[seq + "/frame_duration"] = np.float64(d["FrameDuration"])
        print(seq, mocap[seq + "/frames"].shape, d["FrameDuration"])
    np.savez_compressed(os.path.join(out, "mocap_laikago.npz"), **mocap)


def main_laikago_toes(argv=()):
    collapse, out = "--collapse-fixed-joints" in argv, LAIKAGO_TOES_OUT
    if "--out" in argv:
        out = argv[argv.index("--out") + 1]
    elif collapse:
        sys.exit("--collapse-fixed-joints needs --out PATH (the committed fixture is the uncollapsed template)")
    tpl = compile_laikago_toes(collapse_fixed_joints=collapse)
    np.savez_compressed(out, **tpl)
    print("laikago_toes%s nb=%d nq=%d nqd=%d Nc=%d -> %s (%d bytes)"
          % (" (fixed joints collapsed)" if collapse else "", tpl["nb"], tpl["nq"], tpl["nqd"], len(tpl["contact_body"]), out, os.path.getsize(out)))


if __name__ == "__main__":
    main_laikago_toes(sys.argv[1:]) if "--laikago-toes" in sys.argv[1:] else main()
