"""Host side of the joint-space mass-matrix op, PD_POSE_MASS_MATRIX = 23: the float64 restatement of the composite-rigid-body recursion
(tests/mass_matrix_ref.py) against the dense H = J^T M J it is held to, in either rate mode, its exact zeros, the VJP formulas the kernel
implements against autograd of the dense H, the argument checks of the two pose entries for the new op code and the wrappers' refusals.
All without a GPU.

Measured here (float64): the recursion against dense_H at most 4.6e-14 of sqrt(H_aa H_bb) (bar 1e-10); the VJP formulas against
autograd of dense_H at most 7.0e-16 of max per tensor (bar 1e-9)."""
import ctypes

import numpy as np
import pytest
import torch

from joint_coords_ref import oracle_template
from joint_wrench_ref import template
from mass_matrix_ref import (ALL_CASES, RATES, accel_case, body_weights, crba, crba_vjp, dense_H, g_out_of, related_mask, robot_template,
                             scaled_error)

F64 = torch.float64


def _state(name, S, shift=None, dtype=F64):
    C = accel_case(name, S, shift)
    tpl = C["tpl"]
    T = oracle_template(tpl, dtype)
    bq = torch.tensor(np.array(C["bq"]), dtype=dtype)
    m, I = body_weights(tpl, S, dtype)
    return C, tpl, T, bq, m, I


# ------------------------------------------------------------------------------------------------------------- (a) the recursion
@pytest.mark.parametrize("rates", RATES)
@pytest.mark.parametrize("name,S,shift", ALL_CASES)
def test_recursion_is_the_dense_matrix(name, S, shift, rates):
    """The float64 recursion against dense_H on every case: E = max |H - H_dense|_ab / sqrt(H_aa H_bb) <= 1e-10; exactly symmetric."""
    C, tpl, T, bq, m, I = _state(name, S, shift)
    H = crba(T, tpl, bq, m, I, rates)
    Hd = dense_H(T, tpl, bq, m, I, rates)
    assert H.shape == (S, T.nqd, T.nqd)
    e = scaled_error(H.numpy(), Hd.numpy())
    print("%s %s recursion against dense_H: E = %.2e" % (name, rates, e))
    assert np.isfinite(e) and e <= 1e-10
    assert torch.equal(H, H.transpose(-1, -2))


@pytest.mark.parametrize("name,S", [("mixed25", 2), ("human", 2)])
def test_unrelated_dofs_are_exactly_zero(name, S):
    """An entry between dofs of two bodies neither of which is the other's ancestor is exactly 0 in the recursion (and only rounding
    residue in dense_H); both robots branch, so there are such entries, and the related ones are not all zero."""
    C, tpl, T, bq, m, I = _state(name, S)
    mask = related_mask(tpl)
    assert (~mask).sum() > 0 and np.array_equal(mask, mask.T) and mask.diagonal().all()
    for rates in RATES:
        H = crba(T, tpl, bq, m, I, rates).numpy()
        assert (H[:, ~mask] == 0).all()
        assert float(np.abs(dense_H(T, tpl, bq, m, I, rates).numpy()[:, ~mask]).max()) <= 1e-12 * float(np.abs(H).max())
        assert (np.abs(H[:, mask]) > 0).mean() > 0.9


# ------------------------------------------------------------------------------------------------------------- (b) the VJP formulas
@pytest.mark.parametrize("rates", RATES)
@pytest.mark.parametrize("name,S", [("laikago", 2), ("human", 2), ("mixed25", 2), ("freeleaf5", 3), ("cmp31", 2)])
def test_vjp_formulas_are_autograd_of_the_dense_matrix(name, S, rates):
    """A_i, Q_i -> P_b and Z_i of the kernel's VJP, chained through the spatial inertias and motion subspaces, against autograd of
    <G, dense_H> with G not symmetric and an inertia that is not symmetric either: at most 1e-9 of max per tensor."""
    C, tpl, T, bq, m, I = _state(name, S)
    I = I + 0.05 * I.abs().amax((-1, -2), keepdim=True) * torch.tensor(np.random.RandomState(5).randn(*I.shape), dtype=F64)
    G = torch.tensor(g_out_of(C), dtype=F64)
    leaves = [t.clone().requires_grad_(True) for t in (bq, m, I)]
    want = torch.autograd.grad((dense_H(T, tpl, leaves[0], leaves[1], leaves[2], rates) * G).sum(), leaves)
    got = crba_vjp(T, tpl, bq, m, I, rates, G)
    for what, a, b in zip(("g_body_q", "g_mass", "g_inertia"), got, want):
        scale = float(b.abs().max())
        e = float((a - b).abs().max())
        print("%s %s VJP formulas %s: %.2e of max %.3g" % (name, rates, what, e / scale, scale))
        assert scale > 0 and e <= 1e-9 * scale, what
    assert torch.equal(got[2], got[2].transpose(-1, -2))   # the inertia gradient is that of sym(I)


# ------------------------------------------------------------------------------------------------------------- (c) the C ABI
def test_pose_entries_check_the_new_op_without_a_gpu():
    from diffphys_amd import hip_backend

    lib = hip_backend.lib()
    err = lambda: lib.pd_last_error()
    assert hip_backend.POSE_MASS_MATRIX == 23
    assert lib.pd_abi_version() == 9
    assert lib.pd_pose_op(23, 0, None, 13, None, None, None) == 0    # (on the parent commit 23 is an unknown op: this fails there)
    assert lib.pd_pose_op(23, 0, None, 256, None, None, None) == 0
    assert lib.pd_pose_op_vjp(23, 0, None, 13, None, None, None, None, None) == 0   # the op has a VJP kernel
    buf = (ctypes.c_float * 64)()   # host memory: the call must be refused before anything is launched or read
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.pd_pose_op(23, 26, None, 13, None, p, None) != 0 and b"NULL operand" in err()
    # a bad group size, at every n
    assert lib.pd_pose_op(23, 14, p, 13, p, p, None) != 0 and b"n % g" in err()
    assert lib.pd_pose_op(23, 0, None, 0, None, None, None) != 0 and b"n % g" in err()
    assert lib.pd_pose_op_vjp(23, 14, p, 13, p, p, None, p, None) != 0 and b"n % g" in err()
    # the cap on the bodies per state set, at every n
    assert lib.pd_pose_op(23, 0, None, 257, None, None, None) != 0 and b"at most 256" in err() and b"PD_POSE_MASS_MATRIX" in err()
    assert lib.pd_pose_op(23, 257, p, 257, p, p, None) != 0 and b"at most 256" in err()
    assert lib.pd_pose_op_vjp(23, 257, p, 257, p, p, None, p, None) != 0 and b"at most 256" in err()
    # the table has no gradient, at every n
    assert lib.pd_pose_op_vjp(23, 13, p, 13, p, p, p, p, None) != 0 and b"g_a" in err() and b"PD_POSE_MASS_MATRIX" in err()
    assert lib.pd_pose_op_vjp(23, 0, None, 13, None, None, p, None, None) != 0 and b"g_a" in err()
    off = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16 + 4)
    assert lib.pd_pose_op(23, 13, off, 13, p, p, None) != 0 and b"aligned" in err() and b"joint table" in err()
    for op in (22, 24):   # the gap before the code and the code after it: unknown ops
        assert lib.pd_pose_op(op, 0, None, 13, None, None, None) != 0 and b"unknown op" in err()
        assert lib.pd_pose_op_vjp(op, 13, p, 13, p, p, None, p, None) != 0 and b"unknown op" in err()


# ------------------------------------------------------------------------------------------------------------- (d) the binding
class _Env:
    def __init__(self, tpl):
        self.nb, self._tpl, self._contact_table = int(tpl["nb"]), tpl, None

    def template(self):
        return self._tpl


def test_wrapper_refusals_without_a_gpu():
    from diffphys_amd import dp_model, dp_utils, hip_backend

    tpl = template("laikago")
    nb, nqd = int(tpl["nb"]), int(tpl["nqd"])
    env = _Env(tpl)
    table = hip_backend.joint_table(tpl, "generalized", device="cpu")
    rows = torch.zeros(2 * nb, 17)
    with pytest.raises(ValueError, match="joint_table"):   # a bare tensor carries no dimensions
        hip_backend.mass_matrix(torch.zeros(table.numel()), nb, rows)
    with pytest.raises(ValueError, match="a mass table"):
        hip_backend.mass_matrix(hip_backend.mass_table(tpl, device="cpu"), nb, rows)
    with pytest.raises(ValueError, match=r"\(p, q xyzw, m, I row-major\)"):
        hip_backend.mass_matrix(table, nb, torch.zeros(2 * nb, 23))
    with pytest.raises(ValueError, match="multiple"):
        hip_backend.mass_matrix(table, nb, rows[:5])
    with pytest.raises(ValueError, match="nb"):
        hip_backend.mass_matrix(table, nb + 1, torch.zeros(2 * (nb + 1), 17))
    with pytest.raises(ValueError, match="GPU"):    # no CPU fallback: refused before any launch
        hip_backend.mass_matrix(table, nb, rows)
    with pytest.raises(ValueError, match="GPU"):
        hip_backend.mass_matrix_vjp(table, nb, rows, torch.zeros(2, nqd, nqd))
    bq, tau = torch.zeros(2, 3, nb, 7), torch.zeros(2, 3, nqd)
    m, I = torch.ones(nb), torch.eye(3).expand(nb, 3, 3)
    with pytest.raises(TypeError, match="GPU"):
        dp_model.MassMatrix.apply(bq, m.expand(2, 3, nb), I.expand(2, 3, nb, 3, 3), env, "generalized")
    with pytest.raises(TypeError, match="GPU"):
        dp_utils.mass_matrix(bq, m, I, env, method="crba")
    with pytest.raises(TypeError, match="GPU"):    # the default method is refused as before
        dp_utils.mass_matrix(bq, m, I, env)
    with pytest.raises(ValueError, match="GPU"):   # ... and forward_dynamics' new method, as a ValueError that names the method
        dp_utils.forward_dynamics(bq, tau, tau, m, I, env, method="crba")
    # method= and rates= are validated before anything else
    with pytest.raises(ValueError, match="method"):
        dp_utils.mass_matrix(bq, m, I, env, method="aba")
    with pytest.raises(ValueError, match="rates"):
        dp_utils.mass_matrix(bq, m, I, env, method="crba", rates="actuator")
    with pytest.raises(ValueError, match="crba"):   # the measured rates are the kernel's alone
        dp_utils.mass_matrix(bq, m, I, env, method="jacobian", rates="measured")
    with pytest.raises(ValueError, match="method"):
        dp_utils.forward_dynamics(bq, tau, tau, m, I, env, method="composite")
    assert env._contact_table is None   # nothing was built for a refused call
    if torch.cuda.is_available():   # the shape checks sit behind the device check
        c = lambda t: t.cuda()
        with pytest.raises(ValueError, match="body_q"):
            dp_utils.mass_matrix(c(bq)[..., :6], c(m), c(I), env, method="crba")
        with pytest.raises(ValueError, match="body_mass"):
            dp_utils.mass_matrix(c(bq), c(m)[:5], c(I), env, method="crba")
        with pytest.raises(ValueError, match="body_inertia"):
            dp_utils.mass_matrix(c(bq), c(m), c(I)[:, :2], env, method="crba")
