"""Host side of the body-twist op, PD_POSE_BODY_TWIST = 17: the argument checks of the two pose entries for the new op code, the
identities the float64 restatement (tests/body_twists_ref.py) rests on -- the power identity with the generalised force, the round trip
through joint_coords, the finite difference of forward kinematics --, what separates it from eval_fk's velocities, the slot index and
the wrappers' refusals.  All without a GPU.

The identities run on a float64 copy of the template with its quaternions and axes normalised in float64
(generalized_force_ref.unit_template), on float64 FK states whose pose quaternions are normalised in float64.  Measured here: power
1.6e-16 relative (bar 1e-10), round trip 6.0e-15 (bar 1e-10), finite difference 2.0e-9 against values up to 7.1 (bar 1e-6 of max),
angular parts against eval_fk 1.3e-15 (bar 1e-10), linear parts against eval_fk 0.93 m/s on Laikago (must exceed 0.1)."""
import ctypes

import numpy as np
import pytest
import torch

from body_twists_ref import CASES, DOFS, EFFORTS_OF, RATES, body_twists, slot_index, slots_of
from generalized_force_ref import generalized_force, unit_template
from joint_coords_ref import joint_coords, oracle_template, random_coords
from joint_wrench_ref import template

F64 = torch.float64
ROUND_TRIP_ROBOTS = ("laikago", "human", "mixed25", "cmp31", "rev64", "laikago_toes", "worldmix9")


# ------------------------------------------------------------------------------------------------------------- (a) the C ABI
def test_pose_entries_check_the_new_op_without_a_gpu():
    from diffphys_amd import hip_backend

    lib = hip_backend.lib()
    err = lambda: lib.pd_last_error()
    assert hip_backend.POSE_BODY_TWIST == 17
    assert lib.pd_abi_version() == 9
    assert lib.pd_pose_op(17, 0, None, 13, None, None, None) == 0    # (on the parent commit 17 is an unknown op: this fails there)
    assert lib.pd_pose_op_vjp(17, 0, None, 13, None, None, None, None, None) == 0
    assert lib.pd_pose_op(17, 0, None, 256, None, None, None) == 0
    buf = (ctypes.c_float * 64)()   # host memory: the call must be refused before anything is launched or read
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.pd_pose_op(17, 26, None, 13, None, p, None) != 0 and b"NULL operand" in err()
    assert lib.pd_pose_op_vjp(17, 26, None, 13, p, p, None, p, None) != 0 and b"NULL operand" in err()
    # a bad group size, at every n
    assert lib.pd_pose_op(17, 14, p, 13, p, p, None) != 0 and b"n % g" in err()
    assert lib.pd_pose_op_vjp(17, 14, p, 13, p, p, None, p, None) != 0 and b"n % g" in err()
    assert lib.pd_pose_op(17, 0, None, 0, None, None, None) != 0 and b"n % g" in err()
    # the cap on the bodies per state set, at every n
    assert lib.pd_pose_op(17, 0, None, 257, None, None, None) != 0 and b"at most 256" in err() and b"PD_POSE_BODY_TWIST" in err()
    assert lib.pd_pose_op_vjp(17, 257, p, 257, p, p, None, p, None) != 0 and b"at most 256" in err()
    # the table has no gradient: a non-NULL g_a is refused, at n = 0 too
    assert lib.pd_pose_op_vjp(17, 13, p, 13, p, p, p, p, None) != 0 and b"g_a" in err() and b"PD_POSE_BODY_TWIST" in err()
    assert lib.pd_pose_op_vjp(17, 0, None, 13, None, None, p, None, None) != 0 and b"g_a" in err()
    # the refusal order is the shared one: n % g, the cap, g_a
    assert lib.pd_pose_op_vjp(17, 14, p, 13, p, p, p, p, None) != 0 and b"n % g" in err()
    assert lib.pd_pose_op_vjp(17, 257, p, 257, p, p, p, p, None) != 0 and b"at most 256" in err()
    off = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16 + 4)
    assert lib.pd_pose_op(17, 13, off, 13, p, p, None) != 0 and b"aligned" in err() and b"joint table" in err()
    for op in (16, 18):   # the gap before the code and the code after it: unknown ops
        assert lib.pd_pose_op(op, 0, None, 13, None, None, None) != 0 and b"unknown op" in err()
        assert lib.pd_pose_op_vjp(op, 13, p, 13, p, p, None, p, None) != 0 and b"unknown op" in err()


# ------------------------------------------------------------------------------------------------------------ (b) the identities
def _fk_case(name, S, shift=None, seed=0, free_rates=True):
    """float64, on the unit template: (tpl, T, joint_q, joint_qd [S, nqd] standard normal, body_q with unit quaternions, eval_fk's body_qd)"""
    from oracle import ref_torch as rt

    tpl = unit_template(template(name))
    T = oracle_template(tpl)
    q, qd = random_coords(tpl, S, seed=1300 + seed, lo=0.05, hi=1.0)
    if not free_rates:
        for b in range(T.nb):
            if T.joint_type[b] == rt.JOINT_FREE:
                qd[:, T.qd_start[b]: T.qd_start[b] + 6] = 0.0
    jq, jqd = torch.tensor(q, dtype=F64), torch.tensor(qd, dtype=F64)
    bq, bqd = rt.eval_fk(T, jq, jqd)
    bq = torch.cat([bq[..., :3], bq[..., 3:] / bq[..., 3:].norm(dim=-1, keepdim=True)], -1)
    if shift is not None:
        bq = torch.cat([bq[..., :3] + torch.tensor(shift, dtype=F64), bq[..., 3:]], -1)
    return tpl, T, jq, jqd, bq, bqd


@pytest.mark.parametrize("rates", RATES)
@pytest.mark.parametrize("name,S,shift", CASES)
def test_power_identity_with_the_generalized_force(name, S, shift, rates):
    """sum tau . qd = sum wrench . twist per state set, tau = generalized_force_ref of standard-normal wrenches in the conjugate effort
    convention: the op is the transpose of op 15 in each mode.  Bar 1e-10 of sum |wrench_k twist_k| (the size of the products summed)."""
    tpl, T, _, jqd, bq, _ = _fk_case(name, S, shift)
    bf = torch.tensor(np.random.RandomState(91 + S).randn(S, T.nb, 6), dtype=F64)
    tw = body_twists(T, bq, slots_of(tpl, jqd), rates)
    tau = generalized_force(T, bq, bf, EFFORTS_OF[rates])
    lhs, rhs = (tau * jqd).sum(-1), (bf * tw).sum((1, 2))
    scale = (bf * tw).abs().sum((1, 2))
    e = float(((lhs - rhs).abs() / scale).max())
    print("%s x %d%s %s power: %.2e relative" % (name, S, " far" if shift else "", rates, e))
    assert float(tw.abs().max()) > 0 and e <= 1e-10


@pytest.mark.parametrize("rates", RATES)
@pytest.mark.parametrize("name", ROUND_TRIP_ROBOTS)
def test_round_trip_through_joint_coords(name, rates):
    """joint_coords_ref(body_q, twists, rates)[1] gives the rates back on every dof but the FREE linear ones (joint_coords' FREE linear
    rate carries Warp's unrotated-com lever: another quantity).  Bar 1e-10."""
    from oracle import ref_torch as rt

    tpl, T, _, jqd, bq, _ = _fk_case(name, 4, seed=2)
    tw = body_twists(T, bq, slots_of(tpl, jqd), rates)
    _, back = joint_coords(T, bq, tw, rates)
    keep = np.ones(T.nqd, bool)
    for b in range(T.nb):
        if T.joint_type[b] == rt.JOINT_FREE:
            keep[T.qd_start[b] + 3: T.qd_start[b] + 6] = False
    assert keep.any()
    e = float((back - jqd)[:, torch.as_tensor(keep)].abs().max())
    print("%s %s round trip: %.2e" % (name, rates, e))
    assert e <= 1e-10


@pytest.mark.parametrize("name", ["laikago", "human", "mixed25", "rev64"])
def test_linear_parts_are_the_finite_difference_of_forward_kinematics(name):
    """Generalized mode, FREE rates zero: v_b is the central difference (h = 1e-6) of x_b = p_b + R(q_b) com_b under
    eval_fk(q +- h qd).  Bar 1e-6 of max |v| (the difference's own truncation and rounding: h^2 |x'''| + eps |x| / h ~ 1e-9)."""
    from oracle import ref_torch as rt

    tpl, T, jq, jqd, bq, _ = _fk_case(name, 4, seed=4, free_rates=False)
    tw = body_twists(T, bq, slots_of(tpl, jqd), "generalized")

    def x_of(q):
        b, _ = rt.eval_fk(T, q, torch.zeros_like(jqd))
        return b[..., :3] + rt.q_rot(b[..., 3:], T.com[None].expand(b.shape[0], T.nb, 3))

    dq = torch.zeros_like(jq)   # d joint_q / dt: the rates in the coordinates' layout (FREE joints stand still)
    for b in range(T.nb):
        n = {rt.JOINT_REVOLUTE: 1, rt.JOINT_COMPOUND: 3}.get(T.joint_type[b], 0)
        dq[:, T.q_start[b]: T.q_start[b] + n] = jqd[:, T.qd_start[b]: T.qd_start[b] + n]
    h = 1e-6
    fd = (x_of(jq + h * dq) - x_of(jq - h * dq)) / (2 * h)
    scale = float(tw[..., 3:].abs().max())
    e = float((tw[..., 3:] - fd).abs().max())
    print("%s finite difference: %.2e against values up to %.3g" % (name, e, scale))
    assert scale > 0.1 and e <= 1e-6 * scale


def test_angular_parts_are_eval_fks_and_linear_parts_are_not():
    """On Laikago the angular parts equal eval_fk's to 1e-10; the linear parts do not -- eval_fk leaves out the levers of the ancestors'
    angular velocities: the difference exceeds 0.1 m/s (measured 0.93 against max |v| 2.5)."""
    tpl, T, _, jqd, bq, bqd = _fk_case("laikago", 8, seed=6)
    tw = body_twists(T, bq, slots_of(tpl, jqd), "generalized")
    e_w = float((tw[..., :3] - bqd[..., :3]).abs().max())
    e_v = float((tw[..., 3:] - bqd[..., 3:]).abs().max())
    print("laikago against eval_fk: angular %.2e, linear %.3g m/s (max |v| %.3g)" % (e_w, e_v, float(tw[..., 3:].abs().max())))
    assert e_w <= 1e-10
    assert e_v > 0.1


# ------------------------------------------------------------------------------------------------------------ (c) the binding
class _Env:
    def __init__(self, tpl):
        self.nb, self._tpl, self._contact_table = int(tpl["nb"]), tpl, None

    def template(self):
        return self._tpl


def test_joint_rate_slot_index():
    from diffphys_amd import hip_backend

    tpl = template("mixed25")
    ty = [int(t) for t in np.asarray(tpl["joint_type"]).reshape(-1)]
    assert set(ty) == {1, 3, 4, 5}   # every joint type
    idx = hip_backend.joint_rate_slot_index(tpl)
    nb, nqd = int(tpl["nb"]), int(tpl["nqd"])
    assert idx.shape == (nb, 6) and idx.dtype == np.int64
    assert np.array_equal(idx, slot_index(tpl))
    used = idx[idx < nqd]
    assert sorted(used.tolist()) == list(range(nqd))   # every dof sits behind exactly one slot
    for b in range(nb):
        assert (idx[b] < nqd).sum() == DOFS[ty[b]] and (idx[b, DOFS[ty[b]]:] == nqd).all()
    env = _Env(tpl)
    flat = hip_backend.env_joint_rate_slot_index(env, "cpu")
    assert flat.dtype == torch.int64 and np.array_equal(flat.numpy(), idx.reshape(-1))
    assert hip_backend.env_joint_rate_slot_index(env, "cpu") is flat   # cached on the model


def test_wrapper_refusals_without_a_gpu():
    from diffphys_amd import dp_model, dp_utils, hip_backend

    tpl = template("laikago")
    nb, nqd = int(tpl["nb"]), int(tpl["nqd"])
    table = hip_backend.joint_table(tpl, "measured", device="cpu")
    rows = torch.zeros(2 * nb, 13)
    with pytest.raises(ValueError, match="joint_table"):   # a bare tensor carries no dimensions
        hip_backend.body_twists(torch.zeros(table.numel()), nb, rows)
    with pytest.raises(ValueError, match="a jointforce table"):
        hip_backend.body_twists(hip_backend.joint_force_table(tpl, device="cpu"), nb, rows)
    with pytest.raises(ValueError, match=r"\(p, q xyzw, r\[6\]\)"):
        hip_backend.body_twists(table, nb, torch.zeros(2 * nb, 12))
    with pytest.raises(ValueError, match="multiple"):
        hip_backend.body_twists(table, nb, rows[:5])
    with pytest.raises(ValueError, match="nb"):
        hip_backend.body_twists_vjp(table, nb + 1, torch.zeros(2 * (nb + 1), 13), torch.zeros(2 * (nb + 1), 6))
    with pytest.raises(ValueError, match="GPU"):    # no CPU fallback: refused before any launch
        hip_backend.body_twists(table, nb, rows)
    with pytest.raises(ValueError, match="GPU"):
        hip_backend.body_twists_vjp(table, nb, rows, torch.zeros(2 * nb, 6))
    env = _Env(tpl)
    bq, qd = torch.zeros(2, 3, nb, 7), torch.zeros(2, 3, nqd)
    with pytest.raises(TypeError, match="GPU"):
        dp_model.BodyTwists.apply(bq, torch.zeros(2, 3, nb, 6), env, "generalized")
    with pytest.raises(TypeError, match="GPU"):
        dp_utils.body_twists(bq, qd, env)
    with pytest.raises(TypeError, match="GPU"):
        dp_utils.jacobian(bq, env)
    with pytest.raises(TypeError, match="GPU"):   # mass_matrix ends in the op: HIP only
        dp_utils.mass_matrix(bq, torch.ones(nb), torch.eye(3).expand(nb, 3, 3), env)
    with pytest.raises(TypeError, match="GPU"):
        dp_utils.rigid_twists(bq, torch.zeros(2, 3, nb, 6), env)
    assert env._contact_table is None   # nothing was built for a refused call
    # a FREE joint below another body: rigid_twists does not serve it, and says so before anything else
    tpl2 = dict(template("mixed25"))
    ty = np.asarray(tpl2["joint_type"]).reshape(-1)
    par = np.array(tpl2["joint_parent"]).reshape(-1).copy()
    free = int(np.flatnonzero(ty == 4)[0])
    assert par[free] < 0
    par[free] = (free + 1) % int(tpl2["nb"])
    tpl2["joint_parent"] = par
    with pytest.raises(ValueError, match="FREE joint"):
        dp_utils.rigid_twists(torch.zeros(1, int(tpl2["nb"]), 7), torch.zeros(1, int(tpl2["nb"]), 6), _Env(tpl2))
    if torch.cuda.is_available():   # the shape and mode checks sit behind the device check
        with pytest.raises(ValueError, match="body_q"):
            dp_utils.body_twists(bq.cuda()[..., :6], qd.cuda(), env)
        with pytest.raises(ValueError, match="joint_qd"):
            dp_utils.body_twists(bq.cuda(), qd.cuda()[..., :5], env)
        with pytest.raises(ValueError, match="rates"):
            dp_utils.body_twists(bq.cuda(), qd.cuda(), env, rates="actuator")
