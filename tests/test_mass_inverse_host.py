"""Host side of the mass-matrix-inverse op, PD_POSE_MASS_INVERSE = 21: the argument checks of the two pose entries for the new op code,
what the float64 restatement (tests/mass_inverse_ref.py) rests on -- the dense solve against the mass matrix in either rate mode --,
the composed gradient formula against autograd of the dense solve, the closed-form partials dp_model.MassInverse.backward uses, the
slot <-> dof index round trip and the wrappers' refusals.  All without a GPU.

Measured here (float64): the recursion against solve(H, r) at most 8.3e-13 of max |x| (rev64; human 1.1e-13; bar 1e-10); the composed
gradient against autograd of the dense solve at most 6.9e-13 of max per tensor (human, g_mass; bar 1e-9)."""
import ctypes

import numpy as np
import pytest
import torch

from body_accel_ref import mass_matrix
from mass_inverse_ref import (DOFS, RATES, accel_case, body_twists, body_weights, dense_H, mass_inverse, r_of, robot_template, slot_index,
                              slots_of, twist_form, unslot)
from joint_coords_ref import oracle_template
from joint_wrench_ref import template

F64 = torch.float64
ROBOTS = [("laikago", 3), ("human", 3), ("mixed25", 2), ("cmp31", 3), ("rev64", 2), ("worldmix9", 2), ("world5", 2), ("rev256", 1),
          ("free1", 2), ("freeleaf5", 4)]


# ------------------------------------------------------------------------------------------------------------- (a) the C ABI
def test_pose_entries_check_the_new_op_without_a_gpu():
    from diffphys_amd import hip_backend

    lib = hip_backend.lib()
    err = lambda: lib.pd_last_error()
    assert hip_backend.POSE_MASS_INVERSE == 21
    assert lib.pd_abi_version() == 9
    assert lib.pd_pose_op(21, 0, None, 13, None, None, None) == 0    # (on the parent commit 21 is an unknown op: this fails there)
    assert lib.pd_pose_op(21, 0, None, 256, None, None, None) == 0
    buf = (ctypes.c_float * 64)()   # host memory: the call must be refused before anything is launched or read
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.pd_pose_op(21, 26, None, 13, None, p, None) != 0 and b"NULL operand" in err()
    # a bad group size, at every n
    assert lib.pd_pose_op(21, 14, p, 13, p, p, None) != 0 and b"n % g" in err()
    assert lib.pd_pose_op(21, 0, None, 0, None, None, None) != 0 and b"n % g" in err()
    # the cap on the bodies per state set, at every n
    assert lib.pd_pose_op(21, 0, None, 257, None, None, None) != 0 and b"at most 256" in err() and b"PD_POSE_MASS_INVERSE" in err()
    assert lib.pd_pose_op(21, 257, p, 257, p, p, None) != 0 and b"at most 256" in err()
    off = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16 + 4)
    assert lib.pd_pose_op(21, 13, off, 13, p, p, None) != 0 and b"aligned" in err() and b"joint table" in err()
    for op in (20, 22):   # the gap before the code and the code after it: unknown ops
        assert lib.pd_pose_op(op, 0, None, 13, None, None, None) != 0 and b"unknown op" in err()
        assert lib.pd_pose_op_vjp(op, 13, p, 13, p, p, None, p, None) != 0 and b"unknown op" in err()


def test_the_vjp_entry_refuses_the_op_by_name():
    """The gradient is composed from pd_pose_op(21) and op 17: pd_pose_op_vjp refuses code 21 at every n, before any launch, and says
    so; the shared refusals (n % g, the cap, g_a) still come first."""
    from diffphys_amd import hip_backend

    lib = hip_backend.lib()
    err = lambda: lib.pd_last_error()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for n, ptr in ((13, p), (0, None)):
        assert lib.pd_pose_op_vjp(21, n, ptr, 13, ptr, ptr, None, ptr, None) != 0
        assert b"PD_POSE_MASS_INVERSE" in err() and b"composed" in err() and b"pd_pose_op(21)" in err() and b"17" in err()
    assert lib.pd_pose_op_vjp(21, 14, p, 13, p, p, None, p, None) != 0 and b"n % g" in err()
    assert lib.pd_pose_op_vjp(21, 257, p, 257, p, p, None, p, None) != 0 and b"at most 256" in err()
    assert lib.pd_pose_op_vjp(21, 13, p, 13, p, p, p, p, None) != 0 and b"g_a" in err() and b"PD_POSE_MASS_INVERSE" in err()
    assert lib.pd_pose_op_vjp(21, 14, p, 13, p, p, p, p, None) != 0 and b"n % g" in err()
    assert lib.pd_pose_op_vjp(21, 257, p, 257, p, p, p, p, None) != 0 and b"at most 256" in err()


# ------------------------------------------------------------------------------------------------------------ (b) the dense solve
def _state(name, S, dtype=F64):
    C = accel_case(name, S)
    tpl = C["tpl"]
    T = oracle_template(tpl, dtype)
    bq = torch.tensor(np.array(C["bq"]), dtype=dtype)
    m, I = body_weights(tpl, S, dtype)
    return C, tpl, T, bq, m, I


@pytest.mark.parametrize("rates", RATES)
@pytest.mark.parametrize("name,S", ROBOTS)
def test_recursion_is_the_dense_solve(name, S, rates):
    """The float64 recursion against solve(H, r), H = J^T M J from body_twists_ref's columns in the same mode (generalized: also
    body_accel_ref.mass_matrix, as dp_utils.mass_matrix builds it).  Bar 1e-10 of max |x|; unused slots exactly 0."""
    C, tpl, T, bq, m, I = _state(name, S)
    r6 = torch.tensor(r_of(C), dtype=F64)
    x6 = mass_inverse(T, bq, m, I, r6, rates)
    H = dense_H(T, tpl, bq, m, I, rates)
    assert float((H - H.transpose(-1, -2)).abs().max()) <= 1e-12 * float(H.abs().max())
    if rates == "generalized" and T.nqd <= 70:
        assert float((H - mass_matrix(T, tpl, bq)).abs().max()) <= 1e-12 * float(H.abs().max())
    xd = torch.linalg.solve(H, unslot(tpl, r6)[..., None])[..., 0]
    scale = float(xd.abs().max())
    e = float((unslot(tpl, x6) - xd).abs().max())
    print("%s %s recursion against the dense solve: %.2e of max %.3g" % (name, rates, e / scale, scale))
    assert scale > 0 and e <= 1e-10 * scale
    unused = slot_index(tpl) == int(tpl["nqd"])
    assert (x6.numpy()[:, unused] == 0).all()
    assert float((slots_of(tpl, unslot(tpl, x6)) - x6).abs().max()) == 0   # the slots hold nothing but the dofs


# ------------------------------------------------------------------------------------------------------------ (c) the composed gradient
@pytest.mark.parametrize("rates", RATES)
@pytest.mark.parametrize("name,S", [("laikago", 2), ("human", 2), ("mixed25", 2), ("freeleaf5", 3)])
def test_composed_gradient_is_the_gradient_of_the_dense_solve(name, S, rates):
    """With lam = H^-1 g: the slot gradient is lam, and the gradient in poses, masses and inertias is that of
    -sum_b tlam_b . M_b . tx_b, tx = body_twists(x), tlam = body_twists(lam), x and lam held constant.  Against autograd of
    <g, solve(H, r)>, float64, bar 1e-9 of max per tensor."""
    C, tpl, T, bq, m, I = _state(name, S)
    rng = np.random.RandomState(7 + len(name))
    r = torch.tensor(rng.randn(S, T.nqd), dtype=F64)
    g = torch.tensor(rng.randn(S, T.nqd), dtype=F64)
    leaves = [t.clone().requires_grad_(True) for t in (bq, m, I, r)]
    H = dense_H(T, tpl, leaves[0], leaves[1], leaves[2], rates)
    x = torch.linalg.solve(H, leaves[3][..., None])[..., 0]
    want = torch.autograd.grad((x * g).sum(), leaves)
    with torch.no_grad():
        lam = torch.linalg.solve(H, g[..., None])[..., 0]
    q2, m2, I2 = (t.clone().requires_grad_(True) for t in (bq, m, I))
    form = -twist_form(q2, m2, I2, body_twists(T, q2, slots_of(tpl, lam), rates), body_twists(T, q2, slots_of(tpl, x.detach()), rates)).sum()
    got = list(torch.autograd.grad(form, (q2, m2, I2))) + [lam]
    for what, a, b in zip(("g_body_q", "g_mass", "g_inertia", "g_r"), got, want):
        scale = float(b.abs().max())
        e = float((a - b).abs().max())
        print("%s %s composed %s: %.2e of max %.3g" % (name, rates, what, e / scale, scale))
        assert scale > 0 and e <= 1e-9 * scale, what


# ------------------------------------------------------------------------------------------------------------ (d) the binding
class _Env:
    def __init__(self, tpl):
        self.nb, self._tpl, self._contact_table = int(tpl["nb"]), tpl, None

    def template(self):
        return self._tpl


@pytest.mark.parametrize("name", ["laikago", "human", "mixed25", "worldmix9", "freeleaf5"])
def test_slot_and_dof_indices_are_inverse(name):
    from diffphys_amd import hip_backend

    tpl = robot_template(name)
    nb, nqd = int(tpl["nb"]), int(tpl["nqd"])
    fwd, back = hip_backend.joint_rate_slot_index(tpl), hip_backend.joint_dof_slot_index(tpl)
    assert np.array_equal(fwd, slot_index(tpl)) and back.shape == (nqd,) and back.dtype == np.int64
    assert np.array_equal(fwd.reshape(-1)[back], np.arange(nqd))          # dof -> slot -> dof
    used = fwd.reshape(-1) < nqd
    assert np.array_equal(back[fwd.reshape(-1)[used]], np.nonzero(used)[0])   # slot -> dof -> slot
    assert used.sum() == nqd == sum(DOFS[int(t)] for t in np.asarray(tpl["joint_type"]).reshape(-1)[:nb])
    qd = torch.arange(1.0, nqd + 1.0)
    from diffphys_amd import dp_utils

    env = _Env(tpl)
    slots = dp_utils._rate_slots(qd, (2,), env, "cpu")
    again = slots.reshape(2, 6 * nb).index_select(-1, hip_backend.env_joint_dof_slot_index(env, "cpu"))
    assert torch.equal(again, qd.expand(2, nqd))


def test_wrapper_refusals_without_a_gpu():
    from diffphys_amd import dp_model, dp_utils, hip_backend

    tpl = template("laikago")
    nb, nqd = int(tpl["nb"]), int(tpl["nqd"])
    env = _Env(tpl)
    table = hip_backend.joint_table(tpl, "generalized", device="cpu")
    rows = torch.zeros(2 * nb, 23)
    with pytest.raises(ValueError, match="joint_table"):   # a bare tensor carries no dimensions
        hip_backend.mass_inverse(torch.zeros(table.numel()), nb, rows)
    with pytest.raises(ValueError, match="a mass table"):   # the centroidal op's rows are 23 floats wide too: the table tells them apart
        hip_backend.mass_inverse(hip_backend.mass_table(tpl, device="cpu"), nb, rows)
    with pytest.raises(ValueError, match=r"\(p, q xyzw, m, I row-major, r\[6\]\)"):
        hip_backend.mass_inverse(table, nb, torch.zeros(2 * nb, 13))
    with pytest.raises(ValueError, match="multiple"):
        hip_backend.mass_inverse(table, nb, rows[:5])
    with pytest.raises(ValueError, match="nb"):
        hip_backend.mass_inverse(table, nb + 1, torch.zeros(2 * (nb + 1), 23))
    with pytest.raises(ValueError, match="GPU"):    # no CPU fallback: refused before any launch
        hip_backend.mass_inverse(table, nb, rows)
    assert not hasattr(hip_backend, "mass_inverse_vjp")   # the gradient is composed: there is no such entry
    bq, tau = torch.zeros(2, 3, nb, 7), torch.zeros(2, 3, nqd)
    m, I = torch.ones(nb), torch.eye(3).expand(nb, 3, 3)
    with pytest.raises(TypeError, match="GPU"):
        dp_model.MassInverse.apply(bq, m.expand(2, 3, nb), I.expand(2, 3, nb, 3, 3), torch.zeros(2, 3, nb, 6), env, "generalized")
    with pytest.raises(TypeError, match="GPU"):
        dp_utils.mass_inverse(bq, tau, m, I, env)
    with pytest.raises(TypeError, match="GPU"):
        dp_utils.mass_matrix_inverse(bq, m, I, env)
    with pytest.raises(TypeError, match="GPU"):
        dp_utils.forward_dynamics(bq, tau, tau, m, I, env, method="articulated")
    with pytest.raises(ValueError, match="method"):   # a method that is none, before anything else
        dp_utils.forward_dynamics(bq, tau, tau, m, I, env, method="crba")
    assert env._contact_table is None   # nothing was built for a refused call
    if torch.cuda.is_available():   # the shape and mode checks sit behind the device check
        c = lambda t: t.cuda()
        with pytest.raises(ValueError, match="body_q"):
            dp_utils.mass_inverse(c(bq)[..., :6], c(tau), c(m), c(I), env)
        with pytest.raises(ValueError, match="tau"):
            dp_utils.mass_inverse(c(bq), c(tau)[..., :5], c(m), c(I), env)
        with pytest.raises(ValueError, match="body_mass"):
            dp_utils.mass_inverse(c(bq), c(tau), c(m)[:5], c(I), env)
        with pytest.raises(ValueError, match="rates"):
            dp_utils.mass_inverse(c(bq), c(tau), c(m), c(I), env, rates="actuator")


def test_twist_form_partials_are_autograd_of_the_form():
    """dp_model._twist_form_partials -- the closed-form partials MassInverse.backward puts between op 17 and its VJP -- against autograd of
    the form itself (mass_inverse_ref.twist_form), float64, non-unit quaternions and a non-symmetric inertia included."""
    from diffphys_amd import dp_model

    rng = np.random.RandomState(3)
    n = 7
    leaves = [torch.tensor(rng.randn(*sh), dtype=F64, requires_grad=True) for sh in ((n, 4), (n, 1), (n, 3, 3), (n, 6), (n, 6))]
    q, m, I, tx, tl = leaves
    bq = torch.cat([torch.zeros(n, 3, dtype=F64), q], -1)[None]
    form = -twist_form(bq, m[None, :, 0], I[None], tl[None], tx[None]).sum()
    g_q, g_m, g_I, g_tx, g_tl = torch.autograd.grad(form, leaves)
    with torch.no_grad():
        got = dp_model._twist_form_partials(q, m, I, tx, tl)
    for what, a, b in zip(("g_tx", "g_tl", "g_q", "g_m", "g_inertia"), got, (g_tx, g_tl, g_q, g_m, g_I)):
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-12 * float(b.abs().max()), what
