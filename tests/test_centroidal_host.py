"""Host side of the whole-body (centroidal) op, PD_POSE_CENTROIDAL = 9: the argument checks of the two pose entries for the new op code,
the mass table's layout, the wrappers' refusals, known answers of the float64 restatement the GPU tests hold the kernels to
(tests/centroidal_ref.py), and the physics pin the op exists for -- per step, the change of linear momentum is dt x (sum of the grf
forces + M g) -- in the float64 oracle on generated robots.  All without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

from centroidal_ref import SLICES, centroidal, centroidal_of, template_constants
from generated_robots import robot, rollout_inputs
from helpers import INPUT_NAMES
from joint_coords_ref import load_tpl

F64 = torch.float64


def test_pose_entries_check_the_new_op_without_a_gpu():
    from diffphys_amd import hip_backend

    lib = hip_backend.lib()
    err = lambda: lib.pd_last_error()
    assert hip_backend.POSE_CENTROIDAL == 9
    assert lib.pd_abi_version() == 9
    assert lib.pd_pose_op(9, 0, None, 13, None, None, None) == 0
    assert lib.pd_pose_op_vjp(9, 0, None, 13, None, None, None, None, None) == 0
    buf = (ctypes.c_float * 64)()   # host memory: the call must be refused before anything is launched or read
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.pd_pose_op(9, 26, None, 13, None, None, None) != 0   # a NULL operand
    assert lib.pd_pose_op(9, 26, None, 13, None, p, None) != 0 and b"NULL operand" in err()
    assert lib.pd_pose_op(9, 26, p, 13, None, p, None) != 0 and b"NULL operand" in err()
    assert lib.pd_pose_op_vjp(9, 26, None, 13, p, p, None, p, None) != 0 and b"NULL operand" in err()
    assert lib.pd_pose_op(9, 14, p, 13, p, p, None) != 0 and b"n % g" in err()
    assert lib.pd_pose_op_vjp(9, 14, p, 13, p, p, None, p, None) != 0 and b"n % g" in err()
    assert lib.pd_pose_op(9, 0, None, 0, None, None, None) != 0 and b"n % g" in err()   # a group size below 1 is refused at every n
    assert lib.pd_pose_op(9, 0, None, -3, None, None, None) != 0 and b"n % g" in err()
    assert lib.pd_pose_op(9, 0, None, 257, None, None, None) != 0 and b"256" in err()   # more bodies than a workgroup places
    assert lib.pd_pose_op(9, 257, p, 257, p, p, None) != 0 and b"256" in err()
    # the mass table has no gradient: a non-NULL g_a is refused, at n = 0 too
    assert lib.pd_pose_op_vjp(9, 13, p, 13, p, p, p, p, None) != 0 and b"g_a" in err()
    assert lib.pd_pose_op_vjp(9, 13, p, 13, p, p, p, None, None) != 0 and b"g_a" in err()
    assert lib.pd_pose_op_vjp(9, 0, None, 13, None, None, p, None, None) != 0 and b"g_a" in err()
    # a table that is not 16-byte aligned is refused before any launch
    off = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16 + 4)
    assert off.value % 16 != 0
    assert lib.pd_pose_op(9, 13, off, 13, p, p, None) != 0 and b"aligned" in err()
    for op in (7, 8, 10):   # the gap of the enum and the code after it: unknown ops
        assert lib.pd_pose_op(op, 0, None, 13, None, None, None) != 0 and b"unknown op" in err()
        assert lib.pd_pose_op(op, 13, p, 13, p, p, None) != 0 and b"unknown op" in err()
        assert lib.pd_pose_op_vjp(op, 13, p, 13, p, p, None, p, None) != 0 and b"unknown op" in err()


@pytest.mark.parametrize("name", ["laikago", "human", "quad", "mixed25"])
def test_mass_table_layout(name):
    from diffphys_amd import hip_backend

    tpl = robot(name) if name == "mixed25" else load_tpl(name)
    nb = int(tpl["nb"])
    t = hip_backend.mass_table_host(tpl)
    L = hip_backend.mass_table_layout(nb)
    assert L == dict(gravity=4, bodies=8, floats=8 + 4 * nb)
    assert t.dtype == np.float32 and t.size == L["floats"] and t.size % 4 == 0
    assert t[:4].tolist() == [nb, 0, 0, 0]
    assert np.array_equal(t[4:7], np.asarray(tpl["gravity"], np.float32).reshape(3)) and t[7] == 0
    assert t[5] < -9.0   # gravity points down the y axis
    body = t[8:].reshape(nb, 4)
    assert np.array_equal(body[:, :3], np.asarray(tpl["body_com"], np.float32).reshape(nb, 3)) and (body[:, 3] == 0).all()
    table = hip_backend.mass_table(tpl, device="cpu")
    assert hip_backend._table_tag(table) == ("mass", (nb,)) and np.array_equal(table.numpy(), t)


class _Env:
    def __init__(self, tpl):
        self.nb, self._tpl = int(tpl["nb"]), tpl

    def template(self):
        return self._tpl


def test_wrapper_refusals_without_a_gpu():
    from diffphys_amd import dp_model, dp_utils, hip_backend

    tpl = load_tpl("laikago")
    nb = int(tpl["nb"])
    with pytest.raises(ValueError, match="256"):
        hip_backend.mass_table_host(dict(tpl, nb=257))
    table = hip_backend.mass_table(tpl, device="cpu")
    rows = torch.zeros(2 * nb, 23)
    with pytest.raises(ValueError, match="mass_table"):   # a bare tensor carries no dimensions
        hip_backend.centroidal(torch.zeros(table.numel()), nb, rows)
    with pytest.raises(ValueError, match="mass_table"):   # nor does a table of another kind stand in: the tag names the kind
        hip_backend.centroidal(hip_backend.joint_table(tpl, device="cpu"), nb, rows)
    with pytest.raises(ValueError, match="23"):
        hip_backend.centroidal(table, nb, torch.zeros(2 * nb, 13))
    with pytest.raises(ValueError, match="multiple"):
        hip_backend.centroidal(table, nb, rows[:5])
    with pytest.raises(ValueError, match="nb"):
        hip_backend.centroidal(table, nb + 1, torch.zeros(2 * (nb + 1), 23))
    with pytest.raises(ValueError, match="GPU"):    # no CPU fallback: refused before any launch
        hip_backend.centroidal(table, nb, rows)
    with pytest.raises(ValueError, match="GPU"):
        hip_backend.centroidal_vjp(table, nb, rows, torch.zeros(2, 16))
    env = _Env(tpl)
    bq, bqd, m, I = torch.zeros(2, 3, nb, 7), torch.zeros(2, 3, nb, 6), torch.ones(nb), torch.zeros(nb, 3, 3)
    with pytest.raises(TypeError, match="GPU"):
        dp_model.Centroidal.apply(bq, bqd, m.expand(2, 3, nb), I.expand(2, 3, nb, 3, 3), env)
    with pytest.raises(TypeError, match="GPU"):
        dp_utils.centroidal(bq, bqd, m, I, env)
    with pytest.raises(TypeError, match="GPU"):
        dp_utils.centroidal(bq.double(), bqd.double(), m.double(), I.double(), env)
    assert dp_utils.CentroidalState._fields == ("mass", "com", "com_vel", "momentum", "angular_momentum", "kinetic", "potential")
    if torch.cuda.is_available():   # the shape checks sit behind the device check
        c = lambda a: a.cuda()
        gpu_table = hip_backend.mass_table(tpl, device="cuda")
        with pytest.raises(ValueError, match="g_out"):
            hip_backend.centroidal_vjp(gpu_table, nb, c(rows), torch.zeros(2, 15).cuda())
        with pytest.raises(TypeError, match="GPU"):
            hip_backend.centroidal_vjp(gpu_table, nb, c(rows), torch.zeros(2, 16))
        with pytest.raises(ValueError, match="body_q"):
            dp_utils.centroidal(c(bq)[..., :6], c(bqd), c(m), c(I), env)
        with pytest.raises(ValueError, match="body_qd"):
            dp_utils.centroidal(c(bq), c(bqd)[:1], c(m), c(I), env)
        with pytest.raises(ValueError, match="broadcast"):
            dp_utils.centroidal(c(bq), c(bqd), c(m)[:3], c(I), env)
        with pytest.raises(ValueError, match="broadcast"):
            dp_utils.centroidal(c(bq), c(bqd), c(m), c(I)[..., :2], env)


def rotm(q):
    x, y, z, w = q
    return np.asarray([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                       [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                       [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def get(out, name):
    v = out[..., SLICES[name]]
    return v[..., 0] if v.shape[-1] == 1 else v


def test_one_body_by_hand():
    rng = np.random.RandomState(0)
    q = rng.randn(4)
    q /= np.linalg.norm(q)
    p, w, v, com = rng.randn(3), rng.randn(3), rng.randn(3), rng.randn(3) * 0.1
    A = rng.randn(3, 3)
    I, m, g = A @ A.T + np.eye(3), 2.5, np.asarray([0.0, -9.80665, 0.0])
    R = rotm(q)
    out = centroidal(torch.tensor(np.r_[p, q])[None], torch.tensor(np.r_[w, v])[None], torch.tensor([m]), torch.tensor(I)[None],
                     torch.tensor(com)[None], torch.tensor(g)).numpy()
    assert out.shape == (16,) and out[15] == 0
    x = p + R @ com
    np.testing.assert_allclose(get(out, "mass"), m, rtol=1e-14)
    np.testing.assert_allclose(get(out, "com"), x, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(get(out, "com_vel"), v, rtol=1e-12)
    np.testing.assert_allclose(get(out, "momentum"), m * v, rtol=1e-12)
    np.testing.assert_allclose(get(out, "angular_momentum"), R @ I @ R.T @ w, rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(get(out, "kinetic"), 0.5 * m * v @ v + 0.5 * w @ (R @ I @ R.T) @ w, rtol=1e-12)
    np.testing.assert_allclose(get(out, "potential"), -m * g @ x, rtol=1e-12)


def test_two_points_on_a_spinning_rod():
    """Two equal point-like bodies (no inertia of their own) at +-r e_x, the rod spinning about e_z through its centre at rate W, the
    centre moving at u: L = 2 m r^2 W e_z about the centre, T = m r^2 W^2 + m |u|^2."""
    m, r, W = 1.5, 0.4, 3.0
    u, centre = np.asarray([0.3, -0.2, 0.1]), np.asarray([5.0, 1.0, -2.0])
    e_x, e_z = np.asarray([1.0, 0, 0]), np.asarray([0, 0, 1.0])
    bq = np.zeros((2, 7))
    bq[:, 6] = 1
    bq[0, :3], bq[1, :3] = centre + r * e_x, centre - r * e_x
    bqd = np.zeros((2, 6))
    bqd[:, :3] = W * e_z
    bqd[0, 3:], bqd[1, 3:] = u + np.cross(W * e_z, r * e_x), u - np.cross(W * e_z, r * e_x)
    out = centroidal(torch.tensor(bq), torch.tensor(bqd), torch.full((2,), m, dtype=F64), torch.zeros(2, 3, 3, dtype=F64),
                     torch.zeros(2, 3, dtype=F64), torch.tensor([0.0, -9.80665, 0.0], dtype=F64)).numpy()
    np.testing.assert_allclose(get(out, "mass"), 2 * m)
    np.testing.assert_allclose(get(out, "com"), centre, rtol=1e-14)
    np.testing.assert_allclose(get(out, "com_vel"), u, rtol=1e-13)
    np.testing.assert_allclose(get(out, "momentum"), 2 * m * u, rtol=1e-13)
    np.testing.assert_allclose(get(out, "angular_momentum"), 2 * m * r * r * W * e_z, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(get(out, "kinetic"), m * r * r * W * W + m * u @ u, rtol=1e-13)
    np.testing.assert_allclose(get(out, "potential"), 2 * m * 9.80665 * centre[1], rtol=1e-13)


def random_states(tpl, S, seed, unit=True):
    nb = int(tpl["nb"])
    rng = np.random.RandomState(seed)
    bq, bqd = rng.randn(S, nb, 7), rng.randn(S, nb, 6)
    if unit:
        bq[..., 3:] /= np.linalg.norm(bq[..., 3:], axis=-1, keepdims=True)
    mass = np.asarray(tpl["body_mass"], np.float64).reshape(nb) * rng.uniform(0.8, 1.25, nb)
    inertia = np.asarray(tpl["body_inertia"], np.float64).reshape(nb, 3, 3) * rng.uniform(0.8, 1.25, (nb, 1, 1))
    return bq, bqd, mass, inertia


@pytest.mark.parametrize("name", ["laikago", "human"])
def test_centre_of_mass_is_compute_com_on_unit_quaternions(name):
    from diffphys_amd import dp_utils

    tpl = load_tpl(name)
    bq, bqd, mass, inertia = random_states(tpl, 3, seed=1)
    out = centroidal_of(tpl, F64, bq, bqd, np.broadcast_to(mass, bq.shape[:2]), np.broadcast_to(inertia, bq.shape[:2] + (3, 3)))[0]
    com = np.asarray(tpl["body_com"], np.float64).reshape(-1, 3)
    for s in range(3):
        np.testing.assert_allclose(get(out[s], "com"), dp_utils.compute_com(bq[s], com[..., None], mass), rtol=1e-12, atol=1e-13)


def test_translation_and_common_velocity_invariance():
    """L and T do not change when every body is moved by the same vector; L does not change under a common velocity offset (T does);
    P changes by M u.  Un-normalised quaternions: the identities hold for the map the op uses, not only for rotations."""
    tpl = load_tpl("human")
    bq, bqd, mass, inertia = random_states(tpl, 4, seed=2, unit=False)
    S, nb = bq.shape[:2]
    m, I = np.broadcast_to(mass, (S, nb)), np.broadcast_to(inertia, (S, nb, 3, 3))
    base = centroidal_of(tpl, F64, bq, bqd, m, I)[0]
    d, u = np.asarray([40.0, -3.0, 25.0]), np.asarray([1.5, -0.5, 2.0])
    moved = bq.copy()
    moved[..., :3] += d
    a = centroidal_of(tpl, F64, moved, bqd, m, I)[0]
    np.testing.assert_allclose(get(a, "angular_momentum"), get(base, "angular_momentum"), rtol=1e-10, atol=1e-11)
    np.testing.assert_allclose(get(a, "kinetic"), get(base, "kinetic"), rtol=1e-13)
    np.testing.assert_allclose(get(a, "com"), get(base, "com") + d, rtol=1e-12)
    faster = bqd.copy()
    faster[..., 3:] += u
    b = centroidal_of(tpl, F64, bq, faster, m, I)[0]
    np.testing.assert_allclose(get(b, "angular_momentum"), get(base, "angular_momentum"), rtol=1e-10, atol=1e-11)
    np.testing.assert_allclose(get(b, "momentum"), get(base, "momentum") + get(base, "mass")[:, None] * u, rtol=1e-12)
    assert np.abs(get(b, "kinetic") - get(base, "kinetic")).min() > 1e-3


def momentum_identity_residual(tpl, inp, dtype=F64):
    """All steps of the torch oracle's rollout: max |P(s + 1) - P(s) - dt (sum_bodies grf[s].force + M g)| / max |rhs| and the number of
    touching body-steps."""
    from ground_wrench_common import oracle_template
    from oracle import ref_torch as rt

    T = oracle_template(tpl, dtype)
    nb, nsteps, dt = T.nb, inp["nsteps"], inp["dt"]
    t = [torch.as_tensor(np.asarray(inp[k]), dtype=dtype) for k in INPUT_NAMES]
    allq, allqd = rt.rollout(T, *t, nsteps, [0], dt, return_all=True)                       # [T + 1, bs, nb, .]
    grf = rt.rollout(T, *t, nsteps, list(range(nsteps)), dt)[2].view(nsteps, -1, nb, 6)     # [T, bs, nb, 6]
    bs = allq.shape[1]
    assert float(allqd[..., 3:].abs().max()) < 10.0   # the integrator's velocity clamp is not in play
    mass = torch.as_tensor(np.asarray(inp["body_mass"]), dtype=dtype).view(bs, nb)
    inertia = torch.as_tensor(np.asarray(inp["body_inertia"]), dtype=dtype).view(bs, nb, 3, 3)
    com, grav = template_constants(tpl, dtype)
    out = centroidal(allq, allqd, mass.expand(nsteps + 1, bs, nb), inertia.expand(nsteps + 1, bs, nb, 3, 3), com, grav)
    P, M = out[..., SLICES["momentum"]], out[..., 0]
    rhs = dt * (grf[..., 3:].sum(2) + M[:-1, :, None] * grav)
    res = float(((P[1:] - P[:-1]) - rhs).abs().max() / rhs.abs().max())
    contact = grf - torch.as_tensor(np.asarray(inp["res_f"]), dtype=dtype).view(nsteps, bs, nb, 6)
    return res, int((contact.abs().amax(-1) > 0).sum())


@pytest.mark.parametrize("name", ["mixed25", "rev64", "cmp31"])
def test_momentum_identity_in_the_float64_oracle(name):
    """Joints never change the total linear momentum and the integrator adds dt (f / m + g) to every v:
    P(s + 1) - P(s) = dt (sum grf forces + M g).  Measured: 2.8e-8, 6.1e-9, 4.0e-8 -- the fp32 rounding of the inputs' body_inv_mass
    against 1 / body_mass (5e-8); the bar 1e-6 leaves margin."""
    tpl = robot(name)
    res, touching = momentum_identity_residual(tpl, rollout_inputs(tpl, bs=3, T=8, seed=0))
    print("%s: residual %.2e over 8 steps, %d touching body-steps" % (name, res, touching))
    assert touching >= 8
    assert res <= 1e-6
    res, touching = momentum_identity_residual(tpl, rollout_inputs(tpl, bs=3, T=8, seed=0, depth=-1.0))   # in the air
    print("%s in the air: residual %.2e" % (name, res))
    assert touching == 0 and res <= 1e-6
