"""Host side of the per-body ground-contact state op, PD_POSE_CONTACT_STATE = 11: the argument checks of the two pose entries for the new
op code, the wrappers' refusals, the float64 restatement the GPU tests hold the kernels to (tests/contact_state_ref.py) against the
oracle where the oracle can speak, the input conditions of EVERY GPU case (tests/contact_state_cases.py), the two losses on a state
built by hand, and main.py's two flags.  All without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

from contact_state_cases import CASES, GAP, GROUND, STRIDE_COUNTS, TIED, case, conditions, tie_case
from contact_state_ref import contact_state_of, field, input_conditions
from ground_wrench_common import candidate_probe, oracle_template, oracle_wrench
from joint_coords_ref import load_tpl

F64 = torch.float64


# ------------------------------------------------------------------------------------------------------------- (a) the C ABI
def test_pose_entries_check_the_new_op_without_a_gpu():
    from diffphys_amd import hip_backend

    lib = hip_backend.lib()
    err = lambda: lib.pd_last_error()
    assert hip_backend.POSE_CONTACT_STATE == 11
    assert lib.pd_abi_version() == 9
    assert lib.pd_pose_op(11, 0, None, 13, None, None, None) == 0
    assert lib.pd_pose_op_vjp(11, 0, None, 13, None, None, None, None, None) == 0
    buf = (ctypes.c_float * 64)()   # host memory: the call must be refused before anything is launched or read
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.pd_pose_op(11, 26, None, 13, None, None, None) != 0   # a NULL operand
    assert lib.pd_pose_op(11, 26, None, 13, None, p, None) != 0 and b"NULL operand" in err()
    assert lib.pd_pose_op(11, 26, p, 13, None, p, None) != 0 and b"NULL operand" in err()
    assert lib.pd_pose_op_vjp(11, 26, None, 13, p, p, None, p, None) != 0 and b"NULL operand" in err()
    assert lib.pd_pose_op(11, 14, p, 13, p, p, None) != 0 and b"n % g" in err()
    assert lib.pd_pose_op_vjp(11, 14, p, 13, p, p, None, p, None) != 0 and b"n % g" in err()
    assert lib.pd_pose_op(11, 0, None, 0, None, None, None) != 0 and b"n % g" in err()   # a group size below 1 is refused at every n
    assert lib.pd_pose_op(11, 0, None, -3, None, None, None) != 0 and b"n % g" in err()
    assert lib.pd_pose_op(11, 0, None, 1000, None, None, None) == 0                      # no cap on the bodies per state set
    # the contact table has no gradient HERE: a non-NULL g_a is refused, at n = 0 too
    assert lib.pd_pose_op_vjp(11, 13, p, 13, p, p, p, p, None) != 0 and b"g_a" in err() and b"PD_POSE_CONTACT_STATE" in err()
    assert lib.pd_pose_op_vjp(11, 13, p, 13, p, p, p, None, None) != 0 and b"g_a" in err()
    assert lib.pd_pose_op_vjp(11, 0, None, 13, None, None, p, None, None) != 0 and b"g_a" in err()
    # the refusal order is the table's: n % g before g_a
    assert lib.pd_pose_op_vjp(11, 14, p, 13, p, p, p, p, None) != 0 and b"n % g" in err()
    # a table that is not 16-byte aligned is refused before any launch
    off = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16 + 4)
    assert off.value % 16 != 0
    assert lib.pd_pose_op(11, 13, off, 13, p, p, None) != 0 and b"aligned" in err() and b"contact" in err()
    assert lib.pd_pose_op_vjp(11, 13, off, 13, p, p, None, p, None) != 0 and b"aligned" in err()
    for op in (7, 8, 10, 12):   # the gaps of the enum and the code after it: unknown ops
        assert lib.pd_pose_op(op, 0, None, 13, None, None, None) != 0 and b"unknown op" in err()
        assert lib.pd_pose_op(op, 13, p, 13, p, p, None) != 0 and b"unknown op" in err()
        assert lib.pd_pose_op_vjp(op, 13, p, 13, p, p, None, p, None) != 0 and b"unknown op" in err()


# ------------------------------------------------------------------------------------------------------------- (b) the binding
class _Env:
    def __init__(self, tpl):
        self.nb, self._tpl, self._contact_table = int(tpl["nb"]), tpl, None

    def template(self):
        return self._tpl


def test_wrapper_refusals_without_a_gpu():
    from diffphys_amd import dp_model, dp_utils, hip_backend

    tpl = load_tpl("laikago")
    nb = int(tpl["nb"])
    table = hip_backend.contact_table(tpl, device="cpu")
    assert hip_backend._table_tag(table)[0] == "contact"
    state = torch.zeros(2 * nb, 13)
    with pytest.raises(ValueError, match="contact_table"):   # a bare tensor carries no dimensions: no bare=True here
        hip_backend.contact_state(torch.zeros(table.numel()), nb, state)
    with pytest.raises(ValueError, match="contact_table"):
        hip_backend.contact_state_vjp(torch.zeros(table.numel()), nb, state, torch.zeros(2 * nb, 8))
    with pytest.raises(ValueError, match="a joint table"):   # a table of another kind is refused by name
        hip_backend.contact_state(hip_backend.joint_table(tpl, device="cpu"), nb, state)
    with pytest.raises(ValueError, match="a mass table"):
        hip_backend.contact_state_vjp(hip_backend.mass_table(tpl, device="cpu"), nb, state, torch.zeros(2 * nb, 8))
    with pytest.raises(ValueError, match="13"):
        hip_backend.contact_state(table, nb, torch.zeros(2 * nb, 23))
    with pytest.raises(ValueError, match="multiple"):
        hip_backend.contact_state(table, nb, state[:5])
    with pytest.raises(ValueError, match="nb"):
        hip_backend.contact_state(table, nb + 1, torch.zeros(2 * (nb + 1), 13))
    with pytest.raises(ValueError, match="GPU"):    # no CPU fallback: refused before any launch
        hip_backend.contact_state(table, nb, state)
    with pytest.raises(ValueError, match="GPU"):
        hip_backend.contact_state_vjp(table, nb, state, torch.zeros(2 * nb, 8))
    env = _Env(tpl)
    bq, bqd = torch.zeros(2, 3, nb, 7), torch.zeros(2, 3, nb, 6)
    with pytest.raises(TypeError, match="GPU"):
        dp_model.ContactState.apply(bq, bqd, env)
    with pytest.raises(TypeError, match="GPU"):
        dp_utils.contact_state(bq, bqd, env)
    with pytest.raises(TypeError, match="GPU"):
        dp_utils.contact_state(bq.double(), bqd.double(), env)
    assert dp_utils.ContactState._fields == ("height", "point_xz", "velocity", "depth", "count")
    if torch.cuda.is_available():   # the shape checks sit behind the device check
        c = lambda a: a.cuda()
        gpu_table = hip_backend.contact_table(tpl, device="cuda")
        with pytest.raises(ValueError, match="g_out"):
            hip_backend.contact_state_vjp(gpu_table, nb, c(state), torch.zeros(2 * nb, 6).cuda())
        with pytest.raises(TypeError, match="GPU"):
            hip_backend.contact_state_vjp(gpu_table, nb, c(state), torch.zeros(2 * nb, 8))
        with pytest.raises(ValueError, match="body_q"):
            dp_utils.contact_state(c(bq)[..., :6], c(bqd), env)
        with pytest.raises(ValueError, match="body_qd"):
            dp_utils.contact_state(c(bq), c(bqd)[:1], env)


# ------------------------------------------------------------------------------------------- (c) the restatement and the oracle
@pytest.mark.parametrize("name,kind", [("mixed25", "tumbled"), ("cmp31", "scaled"), ("laikago", "shipped")])
def test_restated_heights_are_the_oracles(name, kind):
    """The lowest height per body and the touch count of the restatement against ground_wrench_common.candidate_probe (the oracle's
    eval_body_contacts, per candidate) in float64: 1e-12 m."""
    tpl, bq, bqd = case(name, kind)
    out = contact_state_of(tpl, F64, bq, bqd)[0]
    c = candidate_probe(tpl, bq.astype(np.float64), bqd.astype(np.float64))[0]
    cb = np.asarray(tpl["contact_body"]).reshape(-1)
    seen = 0
    for b in range(int(tpl["nb"])):
        mine = c[:, cb == b]
        if mine.shape[1] == 0:
            assert np.isposinf(field(out, "height")[:, b]).all() and (out[:, b, 1:] == 0).all()
            continue
        seen += 1
        assert np.abs(field(out, "height")[:, b] - mine.min(1)).max() <= 1e-12
        assert np.array_equal(field(out, "count")[:, b], (~(mine > 0)).sum(1))
        np.testing.assert_allclose(field(out, "depth")[:, b], -np.where(mine > 0, 0.0, mine).sum(1), rtol=0, atol=1e-12)
    assert seen >= 1


def test_restated_velocity_is_the_oracles_friction_force():
    """A body with exactly ONE touching candidate under materials (ke, kd, kf, mu) = (1e6, 0, 1, 1e6): the friction branch is
    ft = kf vt = vt (mu fn is out of reach), so the x and z components of the body's force in oracle_wrench -- body_f MINUS the contact
    force -- are -u.x, -u.z of the restatement's lowest candidate.  1e-9 relative, float64."""
    tpl, bq, bqd = case("mixed25", "shallow")
    tpl = dict(tpl)
    tpl["shape_materials"] = np.tile(np.asarray([[1.0e6, 0.0, 1.0, 1.0e6]], np.float32), (len(tpl["shape_materials"]), 1))
    out = contact_state_of(tpl, F64, bq, bqd)[0]
    T = oracle_template(tpl, F64)
    w = oracle_wrench(T, torch.tensor(np.array(bq), dtype=F64), torch.tensor(np.array(bqd), dtype=F64)).numpy()
    one = field(out, "count") == 1
    assert one.sum() >= 5
    u = field(out, "velocity")[one]
    assert np.abs(u).max() < 400.0   # the +-500 N clamp is not in play
    for k, col in ((0, 3), (2, 5)):
        assert np.abs(w[one][:, col] + u[:, k]).max() <= 1e-9 * np.abs(u[:, k]).max()
    assert (np.abs(w[field(out, "count") == 0]) == 0).all()


# ---------------------------------------------------------------------------------------- (d) the inputs of every GPU case
@pytest.mark.parametrize("name,kind", CASES + [(str(k), "stride") for k in STRIDE_COUNTS])
def test_input_conditions_of_the_gpu_cases(name, kind):
    """contact_state_cases.conditions: no candidate within 1e-6 m of the ground; no element whose two lowest heights are closer than
    1e-5 m -- but for shipped Laikago, at most 5 % of whose elements are.  Measured here in float64: the smallest gap 1.7e-5 m over the
    generated robots, 1.15e-5 m over the stride cases; Laikago 2 of 78 elements under 1e-5 m (5.5e-7 m the smallest)."""
    C, compared = conditions(name, kind)
    tpl, bq, bqd = case(name, kind)
    assert compared.shape == bq.shape[:2] and C["ground"] >= GROUND
    assert (C["gap"][compared] >= GAP).all() and compared.mean() >= 0.95
    assert compared.all() or (name, kind) == ("laikago", "shipped")
    touching = field(contact_state_of(tpl, F64, bq, bqd)[0], "count")
    assert (touching > 0).any()
    if kind == "tumbled":   # airborne bodies too: the height is wanted for them
        assert (touching[:, C["count"] > 0] == 0).any()
    if kind == "shipped":
        assert C["count"].max() >= (96 if name == "laikago" else 8)


def test_the_stride_cases_win_on_both_sides_of_lane_64():
    """One body of k candidates (a lane takes candidates lane, lane + 64, ...) and one of three with contact_dist 0.02: over the cases
    the winning index of body 0 lies below 64 and at or above it -- k = 129 alone has both -- and body 1's candidates carry their dist."""
    winners = {}
    for k in STRIDE_COUNTS:
        tpl, bq, bqd = case(str(k), "stride")
        C = input_conditions(tpl, bq, bqd)
        assert C["count"].tolist() == [k, 3] and (np.asarray(tpl["contact_dist"])[k:] == np.float32(0.02)).all()
        winners[k] = C["winner"][:, 0]
    both = lambda w: (w < 64).any() and (w >= 64).any()
    assert both(np.concatenate(list(winners.values()))) and both(winners[129])
    assert all((winners[k] < 64).all() for k in (63, 64))


def test_the_tie_case_is_a_tie_in_every_dtype():
    tpl, bq, bqd = tie_case()
    C = input_conditions(tpl, bq, bqd)
    assert C["ground"] >= GROUND and C["count"].tolist() == [130, 3]
    assert (C["winner"][:, 0] == TIED[0]).all() and (C["gap"][:, 0] == 0).all() and (C["gap"][:, 1] >= GAP).all()
    pts = np.asarray(tpl["contact_point"])
    assert len({tuple(pts[i, [0, 2]]) for i in TIED}) == 3 and len({float(pts[i, 1]) for i in TIED}) == 1
    for dtype in (F64, torch.float32):
        out = contact_state_of(tpl, dtype, bq, bqd)[0]
        assert (field(out, "count")[:, 0] == 3).all()
        want = bq[:, 0][:, [0, 2]].astype(np.float64) + pts[TIED[0], [0, 2]].astype(np.float64)
        assert np.abs(field(out, "point_xz")[:, 0] - want).max() <= 1e-6


# --------------------------------------------------------------------------------------------------------- the two losses
def _state(height, vel, depth, count):
    from diffphys_amd import dp_utils

    h = torch.tensor(height, dtype=F64)
    return dp_utils.ContactState(h, torch.zeros(h.shape + (2,), dtype=F64), torch.tensor(vel, dtype=F64), torch.tensor(depth, dtype=F64),
                                 torch.tensor(count, dtype=F64))


def test_the_two_losses_by_hand():
    """penetration_loss = mean depth^2, skate_loss = mean clamp(1 - h / h0, 0, 1) (u.x^2 + u.z^2), both over the chosen bodies that HAVE
    candidates (height < +inf): the body without candidates is left out before any arithmetic -- no NaN in value or gradient."""
    from diffphys_amd import dp_utils

    inf = float("inf")
    cs = _state([[-0.01, 0.01, inf], [0.03, 0.0, inf]],
                [[[1.0, 5.0, 2.0], [3.0, 0.0, 0.0], [0.0, 0.0, 0.0]], [[7.0, 0.0, 0.0], [0.0, 9.0, 1.0], [0.0, 0.0, 0.0]]],
                [[0.03, 0.0, 0.0], [0.0, 0.0, 0.0]], [[2.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    leaves = [cs.height.requires_grad_(True), cs.velocity.requires_grad_(True), cs.depth.requires_grad_(True)]
    pen, skate = dp_utils.penetration_loss(cs), dp_utils.skate_loss(cs, h0=0.02)
    assert abs(float(pen.detach()) - 0.03 ** 2 / 4) <= 1e-15
    # weights: 1 (in the ground), 0.5 (half way up), 0 (above h0), 1 (on the ground)
    assert abs(float(skate.detach()) - (1.0 * 5.0 + 0.5 * 9.0 + 0.0 * 49.0 + 1.0 * 1.0) / 4) <= 1e-12
    (pen + skate).backward()
    for t in leaves:
        assert torch.isfinite(t.grad).all()
    assert float(cs.height.grad[:, 2].abs().max()) == 0 and float(cs.velocity.grad[:, 2].abs().max()) == 0
    assert abs(float(cs.depth.grad[0, 0]) - 2 * 0.03 / 4) <= 1e-15 and float(cs.velocity.grad[0, 0, 1]) == 0
    assert abs(float(cs.height.grad[0, 1]) + 9.0 / 0.02 / 4) <= 1e-9
    # a choice of bodies; one without candidates counts for nothing; none with candidates: 0
    with torch.no_grad():
        assert abs(float(dp_utils.penetration_loss(cs, bodies=[0, 2])) - 0.03 ** 2 / 2) <= 1e-15
        assert abs(float(dp_utils.skate_loss(cs, bodies=[1])) - 0.5 * 9.0 / 2 - 1.0 / 2) <= 1e-12
        assert float(dp_utils.penetration_loss(cs, bodies=[2])) == 0 and float(dp_utils.skate_loss(cs, bodies=[2])) == 0


# --------------------------------------------------------------------------------------------------------------- (e) main.py
def test_main_has_the_two_flags():
    from test_gpu_workload import _main

    m = _main()
    o = m.get_opts([])
    assert o["reg_pen_wt"] == 0.0 and o["reg_skate_wt"] == 0.0
    o = m.get_opts(["--reg_pen_wt", "0.25", "--reg_skate_wt", "2"])
    assert o["reg_pen_wt"] == 0.25 and o["reg_skate_wt"] == 2.0
