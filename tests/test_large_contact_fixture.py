"""The laikago_toes fixture (tests/golden/template_laikago_toes.npz) that the GPU tests of robots with contact tables beyond LDS read:
the reference's laikago_toes.urdf (full lower-leg collision mesh + toe spheres) compiled with Laikago's constants by
`scripts/compile_templates.py --laikago-toes`.  Checked here for what the GPU tests rely on; where the reference tree is present the
template is recompiled and compared entry by entry."""
import os
import sys

import numpy as np
import pytest

from helpers import GOLDEN, ROOT

PATH = os.path.join(GOLDEN, "template_laikago_toes.npz")
REF = os.environ.get("PPR_REFERENCE", "/root/reference")


def load():
    with np.load(PATH) as z:
        return {k: z[k] for k in z.files}


def test_fixture_shapes_and_joint_mix():
    from diffphys_amd import robots

    tpl = load()
    lk = robots.load_template("laikago")
    nb, nq, nqd, nc = int(tpl["nb"]), int(tpl["nq"]), int(tpl["nqd"]), len(tpl["contact_body"])
    assert (nb, nq, nqd, nc) == (17, 19, 18, 11018)
    assert (nq, nqd) == (int(lk["nq"]), int(lk["nqd"])), "the same degrees of freedom as laikago"
    jt = np.asarray(tpl["joint_type"])
    assert np.bincount(jt, minlength=5).tolist() == [0, 12, 0, 4, 1]   # free root, 12 revolute, 4 fixed toes
    assert jt[0] == 4 and (jt[13:] == 3).all()
    for k, shape in (("joint_X_p", (nb, 7)), ("joint_X_c", (nb, 7)), ("joint_axis", (nb, 3)), ("body_com", (nb, 3)), ("body_mass", (nb,)),
                     ("body_inertia", (nb, 3, 3)), ("contact_point", (nc, 3)), ("contact_dist", (nc,)), ("contact_material", (nc,))):
        assert np.asarray(tpl[k]).reshape(shape).shape == shape, k
    cb = np.asarray(tpl["contact_body"])
    assert cb.min() >= 0 and cb.max() < nb
    assert np.isfinite(tpl["contact_point"]).all() and (np.asarray(tpl["body_mass"]) > 0).all()
    # Laikago's constants (the reference's "laikago" branch)
    for k in ("joint_attach_ke", "joint_attach_kd", "kp", "kd"):
        assert float(tpl[k]) == float(lk[k]), k
    assert str(tpl["body_names"][0]) == str(lk["body_names"][0]) and [str(s) for s in tpl["body_names"][13:]] == ["toeRL", "toeRR", "toeFL", "toeFR"]
    # the case it exists for: 16 B of point per candidate alone exceed the 160 KiB of LDS a workgroup may have
    assert 16 * nc > 160 * 1024 and nc <= 65535
    assert os.path.getsize(PATH) < 1 << 20


def test_fixture_matches_a_fresh_compilation():
    urdf = os.path.join(REF, "data", "urdf_templates", "laikago", "laikago_toes.urdf")
    if not os.path.exists(urdf):
        pytest.skip("reference tree not present")
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import compile_templates
    finally:
        sys.path.pop(0)
    from diffphys_amd import robots

    presets = dict(robots.PRESETS)
    fresh = compile_templates.compile_laikago_toes(REF)
    assert robots.PRESETS == presets, "the compilation leaves robots.PRESETS as it was"
    tpl = load()
    assert sorted(fresh) == sorted(tpl)
    for k in tpl:
        assert np.array_equal(np.asarray(fresh[k]), tpl[k]), k
