"""Host side of the ground-wrench op (PD_POSE_GROUND_WRENCH): the contact table's layout, the argument checks of the two pose entries for
the new op code, and ForwardWarpContact's refusals -- all without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

from ground_wrench_common import MATERIALS, two_material_template


@pytest.mark.parametrize("name", ["laikago", "human"])
def test_contact_table_layout(name):
    from diffphys_amd import hip_backend

    tpl = two_material_template(name)
    nb, nc, nmat = int(tpl["nb"]), len(tpl["contact_body"]), 2
    t = hip_backend.contact_table_host(tpl)
    L = hip_backend.contact_table_layout(nb, nc, nmat)
    assert t.dtype == np.float32 and t.size == L["floats"] and L["floats"] % 4 == 0
    assert all(L[k] % 4 == 0 for k in ("materials", "bodies", "points", "point_material"))   # float4 loads
    assert t[:4].tolist() == [nb, nc, nmat, 0]
    assert np.array_equal(t[L["materials"]: L["bodies"]].reshape(nmat, 4), MATERIALS)
    body = t[L["bodies"]: L["points"]].reshape(nb, 12)
    pts = t[L["points"]: L["point_material"]].reshape(nc, 4)
    pmat = t[L["point_material"]: L["point_material"] + nc]
    assert (t[L["point_material"] + nc:] == 0).all()
    assert np.array_equal(body[:, :3], tpl["body_com"])
    seen = 0
    for b in range(nb):
        first, count = int(body[b, 3]), int(body[b, 4])
        idx = np.flatnonzero(np.asarray(tpl["contact_body"]) == b)   # template order
        assert first == seen and count == len(idx)
        assert np.array_equal(pts[first: first + count, :3], np.asarray(tpl["contact_point"])[idx])
        assert np.array_equal(pts[first: first + count, 3], np.asarray(tpl["contact_dist"])[idx])
        assert np.array_equal(pmat[first: first + count], np.asarray(tpl["contact_material"])[idx])
        seen += count
        if count:   # the bounding sphere holds every candidate of the body, the largest dist and the reach are upper bounds
            x = pts[first: first + count, :3].astype(np.float64)
            ctr, r = body[b, 5:8].astype(np.float64), float(body[b, 8])
            assert (np.linalg.norm(x - ctr, axis=1) <= r).all()
            assert body[b, 9] >= pts[first: first + count, 3].max() and body[b, 10] >= np.linalg.norm(ctr) + r
            assert body[b, 11] == b % 2   # one material per body in this model
        else:
            assert body[b, 11] == -1
    assert seen == nc   # every candidate once
    mixed = dict(tpl, contact_material=(np.arange(nc) % 2).astype(np.int32))   # bodies that mix materials say so
    tm = hip_backend.contact_table_host(mixed)
    assert (tm[L["bodies"]: L["points"]].reshape(nb, 12)[:, 11] == -1).all()
    assert np.array_equal(tm[L["point_material"]: L["point_material"] + nc], np.arange(nc) % 2)   # (already grouped by body here)
    with pytest.raises(ValueError):
        hip_backend.contact_table(tpl, materials=torch.zeros(3, 4), device="cpu")
    with pytest.raises(ValueError):
        hip_backend.contact_table(tpl, materials=torch.zeros(8), device="cpu")


def test_pose_entries_check_the_new_op_without_a_gpu():
    from diffphys_amd import hip_backend

    lib = hip_backend.lib()
    assert hip_backend.POSE_GROUND_WRENCH == 5
    assert lib.pd_pose_op(5, 0, None, 13, None, None, None) == 0
    assert lib.pd_pose_op_vjp(5, 0, None, 13, None, None, None, None, None) == 0
    assert lib.pd_pose_op(5, 26, None, 13, None, None, None) != 0
    buf = (ctypes.c_float * 64)()   # host memory: the call must be refused before anything is launched or read
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.pd_pose_op(5, 14, p, 13, p, p, None) != 0
    assert b"n % g" in lib.pd_last_error()
    assert lib.pd_pose_op_vjp(5, 14, p, 13, p, p, p, p, None) != 0
    assert b"n % g" in lib.pd_last_error()
    assert lib.pd_pose_op(5, 0, None, 0, None, None, None) != 0   # a group size below 1 is refused at every n
    assert lib.pd_pose_op(6, 0, None, 0, None, None, None) != 0   # and op 6 does not exist


def test_forward_warp_contact_refuses_checkpointing_before_touching_the_gpu():
    from diffphys_amd import dp_model

    class Host:
        checkpoint_steps = 2
        env = None   # never read

    z = torch.zeros(1)
    with pytest.raises(NotImplementedError, match="checkpoint_steps"):
        dp_model.ForwardWarpContact.apply(*([z] * 11), torch.from_numpy(MATERIALS), Host())


def test_set_shape_materials_replaces_the_rows_and_drops_the_caches():
    from diffphys_amd import sim

    env = sim.Model.from_template(two_material_template("human"), 2, "cpu")
    env._handle, env._contact_table = object(), {"cuda:0": object()}
    rows = MATERIALS[::-1].copy()
    env.set_shape_materials(rows)
    assert env._handle is None and env._contact_table is None
    assert np.array_equal(env.template()["shape_materials"], rows) and env.template()["shape_materials"].dtype == np.float32
    with pytest.raises(ValueError):
        env.set_shape_materials(np.zeros((3, 4)))
