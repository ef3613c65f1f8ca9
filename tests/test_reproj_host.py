"""Host side of the 2D keypoint reprojection term (no GPU): parse_rtk against the reference's own outputs (tests/golden/ref_host_small.npz,
keys rtk/*, written by scripts/make_ref_fixtures.py), the op codes, and the refusals that happen before anything touches the device."""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, ROOT


@pytest.fixture(scope="module")
def ref():
    with np.load(os.path.join(GOLDEN, "ref_host_small.npz")) as z:
        return {k[4:]: z[k] for k in z.files if k.startswith("rtk/")}


def test_parse_rtk_equals_the_reference(ref):
    from diffphys_amd import dp_utils

    rtmat, kmat = dp_utils.parse_rtk(torch.from_numpy(ref["rtk"]))
    assert np.array_equal(rtmat.numpy(), ref["rtmat"]) and np.array_equal(kmat.numpy(), ref["kmat"])
    assert rtmat.shape == ref["rtk"].shape and kmat.shape == ref["rtk"].shape[:-2] + (3, 3)


def test_op_codes_and_dims():
    from diffphys_amd import hip_backend

    assert hip_backend.POSE_PROJECT == 3 and hip_backend.POSE_PROJECT_POINT == 4
    assert hip_backend._POSE_DIMS[3] == (16, 7, 2) and hip_backend._POSE_DIMS[4] == (16, 10, 2)
    hdr = open(os.path.join(ROOT, "include", "ppr_diffphys.h")).read()
    assert "PD_POSE_PROJECT = 3" in hdr and "PD_POSE_PROJECT_POINT = 4" in hdr


def test_group_size_from_the_shapes():
    """(n, g) the binding hands to pd_pose_op: the camera's leading dimensions lead the elements', what follows is the group."""
    from diffphys_amd import hip_backend as hb

    z = torch.zeros
    assert hb._pose_n(3, z(2, 3, 4, 4), z(2, 3, 5, 7)) == (30, 5, 2)     # a camera per (env, frame), 5 bodies each
    assert hb._pose_n(3, z(2, 3, 16), z(2, 3, 5, 7)) == (30, 5, 2)
    assert hb._pose_n(4, z(4, 4), z(9, 10)) == (9, 9, 2)                  # one camera for all
    assert hb._pose_n(3, z(9, 16), z(9, 7)) == (9, 0, 2)                  # a camera per element
    # no element, whichever dimension is the empty one: n = 0 and no group
    for cam, b in ((z(0, 4, 4), z(0, 5, 7)), (z(4, 4), z(0, 7)), (z(3, 4, 4), z(3, 0, 7)), (z(0, 16), z(0, 7))):
        assert hb._pose_n(3, cam, b) == (0, 0, 2)
    # ops 0-2 keep their boolean
    assert hb._pose_n(1, z(7), z(6, 7)) == (6, True, 7) and hb._pose_n(0, z(6, 7), z(6, 6)) == (6, False, 7)


def test_cpu_tensors_are_refused(ref):
    from diffphys_amd import dp_utils

    bodies, rtk = torch.from_numpy(ref["bodies"]), torch.from_numpy(ref["rtk"])
    with pytest.raises(TypeError, match="no CPU fallback"):
        dp_utils.project_bodies(bodies, rtk)
    with pytest.raises(TypeError, match="no CPU fallback"):
        dp_utils.project_bodies(bodies.double(), rtk.double())
    with pytest.raises(TypeError, match="no CPU fallback"):
        dp_utils.project_points(bodies, rtk, torch.tensor([0, 2]), torch.zeros(2, 3))


def test_shape_mismatches_raise_value_error():
    from diffphys_amd import dp_utils, hip_backend as hb

    z = torch.zeros
    for op in (hb.POSE_PROJECT, hb.POSE_PROJECT_POINT):
        nb = hb._POSE_DIMS[op][1]
        for cam in (z(3, 5), z(3, 3, 4), z(3, 4, 3), z(())):  # neither (..., 16) nor (..., 4, 4)
            with pytest.raises(ValueError, match="camera"):
                hb.pose_op(op, cam, z(3, nb))
            with pytest.raises(ValueError, match="camera"):
                hb.pose_op_vjp(op, cam, z(3, nb), z(3, 2))
        with pytest.raises(ValueError):
            hb.pose_op(op, z(3, 16), z(3, nb + 1))      # width
        with pytest.raises(ValueError):
            hb.pose_op(op, z(2, 4, 4), z(3, 5, nb))     # count: 2 cameras cannot lead 3 x 5 elements
        with pytest.raises(ValueError):
            hb.pose_op(op, z(2, 3, 16), z(2, nb))       # more camera dimensions than element dimensions
    with pytest.raises(ValueError):
        dp_utils.project_bodies(z(2, 3, 5, 7), z(2, 4, 4))
    with pytest.raises(ValueError):
        dp_utils.project_bodies(z(2, 5, 6), z(2, 4, 4))
    with pytest.raises(ValueError):
        dp_utils.project_points(z(2, 5, 7), z(2, 4, 4), torch.tensor([0, 1]), z(3, 3))


def test_reproj_loss_is_the_references_line():
    """(project(sim) - project(target)).norm(2, -1).mean(-1) / focal   (dp_model.py:781-792 of the reference, commented out there)"""
    from diffphys_amd import dp_utils

    g = torch.Generator().manual_seed(0)
    a, b = torch.randn(2, 3, 5, 2, generator=g, dtype=torch.float64), torch.randn(2, 3, 5, 2, generator=g, dtype=torch.float64)
    rtk = torch.randn(2, 3, 4, 4, generator=g, dtype=torch.float64)
    want = ((a - b) ** 2).sum(-1).sqrt().mean(-1) / rtk[:, :, 3, 0]
    assert torch.allclose(dp_utils.reproj_loss(a, b, rtk), want, rtol=1e-14, atol=0)
    assert float(dp_utils.reproj_loss(a, a, rtk).abs().max()) == 0


def test_main_has_the_flag():
    import importlib.util

    spec = importlib.util.spec_from_file_location("pd_main_reproj", os.path.join(ROOT, "ppr-diffphys_amd", "main.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    assert m.get_opts([])["traj_2d_wt"] == 0.0 and m.get_opts(["--traj_2d_wt", "0.5"])["traj_2d_wt"] == 0.5
    assert m.get_opts([])["cameras"] is None


def test_main_reads_the_cameras_file(tmp_path, ref):
    """--cameras file.npz: rtk, and the observed keypoints where the file has them -- what main() hands to phys_model.set_cameras"""
    import importlib.util

    spec = importlib.util.spec_from_file_location("pd_main_reproj", os.path.join(ROOT, "ppr-diffphys_amd", "main.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    rtk = ref["rtk"].reshape(-1, 4, 4)
    kp = np.arange(rtk.shape[0] * 5 * 2, dtype=np.float32).reshape(rtk.shape[0], 5, 2)
    only, both, none = (str(tmp_path / n) for n in ("only.npz", "both.npz", "none.npz"))
    np.savez(only, rtk=rtk)
    np.savez(both, rtk=rtk, target_2d=kp)
    np.savez(none, cameras=rtk)
    got, tgt = m.read_cameras(only)
    assert np.array_equal(got, rtk) and tgt is None
    got, tgt = m.read_cameras(both)
    assert np.array_equal(got, rtk) and np.array_equal(tgt, kp)
    with pytest.raises(KeyError, match="rtk"):
        m.read_cameras(none)
    assert m.get_opts(["--cameras", both])["cameras"] == both
