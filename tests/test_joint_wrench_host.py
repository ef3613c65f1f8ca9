"""Host side of the joint-wrench op, PD_POSE_JOINT_WRENCH = 13: the float64 restatement the GPU tests hold the kernels to
(tests/joint_wrench_ref.py) against the oracle's eval_body_joints, the input conditions of EVERY GPU case, the joint-force table, the
argument checks of the two pose entries for the new op code and the wrappers' refusals.  All without a GPU.

Measured here (error over max |reference| per tensor, the fp32 restatement against float64, the largest over the cases): see the
docstring of test_input_conditions_of_the_gpu_cases."""
import ctypes

import numpy as np
import pytest
import torch

from helpers import relmax
from joint_coords_ref import oracle_template
from joint_wrench_ref import CASES, TENSORS, case, input_conditions, rows25, slot_index, template, wrench_of

F64 = torch.float64


def g_out_of(C, seed=29):
    return np.random.RandomState(seed).randn(C["bq"].shape[0], C["nb"], 6)


# ------------------------------------------------------------------------------------------- (1) the restatement and the oracle
@pytest.mark.parametrize("name,S,kind", CASES)
def test_the_restatement_is_the_oracles_joint_pass(name, S, kind):
    """float64: value and the autograd gradient of every input against ref_torch.eval_body_joints on a zero body_f, 1e-9 relative -- the
    agreement the two oracles have with each other.  The oracle takes acos literally: every FIXED joint of the case is >= 1e-3 rad from
    the identity (asserted), where the literal form is still good for 1e-9 in float64.
    The FIXED joint's 2 acos(w) normalize(v) and its scale-invariant form are the same function of a UNIT quaternion and of no other: a
    quaternion rounded to fp32 is 1e-7 off the sphere, which the literal form turns into 1e-4 of the torque (measured: laikago_toes
    1.3e-4; so do the fp32 quaternions of turned joint frames: mixed25 8.3e-5, worldmix9 7.8e-5).  So both sides are given the case's
    states AND the template's joint_X_p with the quaternions normalised in float64, and the quaternion gradients are compared on the
    tangent space of the sphere (the radial derivative is the one thing in which the two forms differ there)."""
    from joint_coords_ref import tangent
    from oracle import ref_torch as rt

    C = case(name, S, kind)
    unit = C["bq"].astype(np.float64)
    unit[..., 3:] /= np.linalg.norm(unit[..., 3:], axis=-1, keepdims=True)
    X_p = np.asarray(C["tpl"]["joint_X_p"], np.float64).reshape(C["nb"], 7).copy()
    X_p[:, 3:] /= np.linalg.norm(X_p[:, 3:], axis=-1, keepdims=True)
    C = dict(C, bq=unit, tpl=dict(C["tpl"], joint_X_p=X_p))
    T = oracle_template(C["tpl"])
    g = g_out_of(C)
    mine = wrench_of(C, F64, g)
    names = ("bq", "bqd", "target", "act", "ke", "kd")
    t = {k: torch.tensor(np.array(C[k]), dtype=F64).requires_grad_(True) for k in names}
    for i in range(T.nb):
        if T.joint_type[i] == rt.JOINT_FIXED:
            par = T.joint_parent[i]
            q_wj = T.X_p[i, 3:].expand(S, 4) if par < 0 else rt.q_mul(t["bq"][:, par, 3:], T.X_p[i, 3:].expand(S, 4))
            r = rt.q_mul(rt.q_conj(q_wj), t["bq"][:, i, 3:]).detach()
            assert float((2 * torch.atan2(r[:, :3].norm(dim=-1), r[:, 3].abs())).min()) >= 1e-3
    out = rt.eval_body_joints(T, t["bq"], t["bqd"], torch.zeros(S, T.nb, 6, dtype=F64), t["target"], t["act"], t["ke"], t["kd"])
    if out.requires_grad:   # (free1: no joint, nothing to differentiate)
        (out * torch.as_tensor(g)).sum().backward()
    grad = lambda k: t[k].grad.numpy() if t[k].grad is not None else np.zeros(t[k].shape)
    theirs = dict(out=out.detach().numpy(), g_body_q=grad("bq"), g_body_qd=grad("bqd"), g_act=grad("act"), g_target=grad("target"),
                  g_ke=grad("ke"), g_kd=grad("kd"))
    mine["g_body_q"], theirs["g_body_q"] = tangent(mine["g_body_q"], unit), tangent(theirs["g_body_q"], unit)
    for k in TENSORS:
        assert mine[k].shape == theirs[k].shape
        assert relmax(mine[k], theirs[k]) <= 1e-9, (k, relmax(mine[k], theirs[k]))
    if name != "free1":
        assert all(np.abs(theirs[k]).max() > 0 for k in TENSORS)
    else:
        assert all(np.abs(theirs[k]).max() == 0 for k in TENSORS)


# ---------------------------------------------------------------------------------------- (2) the inputs of every GPU case
@pytest.mark.parametrize("name,S,kind", CASES)
def test_input_conditions_of_the_gpu_cases(name, S, kind):
    """Per case, in float64, before anything could be launched: every compound second angle |theta| <= 1.2 rad; no dof with a limit gain
    within 1e-4 rad of a limit; no engaged limit with |rate| < 1e-4; no component of a compound pair within 1e-3 relative of +-1e4; the
    fp32 restatement within 1e-4 of float64 per tensor, no element left out.
    Measured (fp32 restatement against float64, the largest over the cases per tensor): printed by this test; see DESIGN.md section 8."""
    C = case(name, S, kind)
    cond = input_conditions(C)
    print(name, S, kind, {k: ("%.3g" % v if isinstance(v, float) else v) for k, v in cond.items()})
    assert cond["theta"] <= 1.2
    assert cond["limit_gap"] >= 1e-4 and cond["limit_rate"] >= 1e-4 and cond["clamp_gap"] >= 1e-3
    if kind == "limits":
        assert cond["engaged"] >= 4 * 19
    g = g_out_of(C)
    r64, r32 = wrench_of(C, F64, g), wrench_of(C, torch.float32, g)
    for k in TENSORS:
        e = relmax(r32[k], r64[k])
        print("  %s %d %s fp32 restatement %-10s %.2e" % (name, S, kind, k, e))
        assert e <= 1e-4, (k, e)


def test_the_limits_case_is_beyond_both_limits_with_both_rate_signs():
    from joint_coords_ref import joint_coords

    C = case("cmp20-limits", 4, "limits")
    T = oracle_template(C["tpl"])
    jq, jqd = joint_coords(T, torch.tensor(np.array(C["bq"]), dtype=F64), torch.tensor(np.array(C["bqd"]), dtype=F64), "measured")
    first = [T.q_start[i] for i in range(T.nb) if T.joint_type[i] == 5]
    firstd = [T.qd_start[i] for i in range(T.nb) if T.joint_type[i] == 5]
    a, r = jq[:, first].numpy(), jqd[:, firstd].numpy()
    assert (a[0] > 1.5).all() and (a[1] < -1.5).all() and (a[2] > 1.5).all() and (a[3] < -1.5).all()
    for s in range(4):
        assert (r[s] > 0).any() and (r[s] < 0).any()
    assert float(T.limit_ke[firstd[0]]) == 40.0 and float(T.limit_kd[firstd[0]]) == 1.0
    # the limit force is in the value: the same case without limit gains differs
    tpl0 = dict(C["tpl"])
    tpl0["joint_limit_ke"] = np.zeros_like(np.asarray(C["tpl"]["joint_limit_ke"]))
    tpl0["joint_limit_kd"] = np.zeros_like(np.asarray(C["tpl"]["joint_limit_kd"]))
    assert relmax(wrench_of(dict(C, tpl=tpl0), F64)["out"], wrench_of(C, F64)["out"]) > 1e-2


# ------------------------------------------------------------------------------------------------------------ (3) the table
@pytest.mark.parametrize("name", ["laikago", "human", "mixed25", "worldmix9", "cmp20-limits", "free1"])
def test_joint_force_table_layout(name):
    from diffphys_amd import hip_backend

    tpl = template(name)
    nb, nqd = int(tpl["nb"]), int(tpl["nqd"])
    t = hip_backend.joint_force_table_host(tpl)
    base = hip_backend.joint_table_host(tpl, "measured")
    L = hip_backend.joint_force_table_layout(nb)
    assert t.dtype == np.float32 and t.shape == (4 + 32 * nb + 4 + 12 * nb,) == (L["floats"],)
    assert L["gains"] == base.size == 4 + 32 * nb and L["limits"] == L["gains"] + 4
    assert torch.equal(torch.from_numpy(t[:base.size].copy()), torch.from_numpy(base)) and t[3] == 0   # the prefix, rate mode measured
    assert t[L["gains"]: L["limits"]].tolist() == [float(np.float32(tpl["joint_attach_ke"])), float(np.float32(tpl["joint_attach_kd"])), 0.0, 0.0]
    slots = t[L["limits"]:].reshape(nb, 3, 4)
    idx = slot_index(tpl)
    fmax = np.finfo(np.float32).max
    lim = np.stack([np.asarray(tpl[k], np.float32).reshape(-1) for k in ("joint_limit_lower", "joint_limit_upper", "joint_limit_ke", "joint_limit_kd")], 1)
    used = 0
    for b in range(nb):
        for k in range(3):
            if idx[b, k] == nqd:
                assert slots[b, k].tolist() == [-fmax, fmax, 0.0, 0.0]
            else:
                used += 1
                assert np.array_equal(slots[b, k], lim[idx[b, k]])
    ty = np.asarray(tpl["joint_type"]).reshape(-1)
    assert used == int((ty == 1).sum() + 3 * (ty == 5).sum())
    dev_t = hip_backend.joint_force_table(tpl, device="cpu")
    assert hip_backend._table_tag(dev_t) == ("jointforce", (nb, int(tpl["nq"]), nqd))
    assert np.array_equal(dev_t.numpy(), t)
    assert np.array_equal(hip_backend.joint_slot_index(tpl), idx)


def test_a_body_with_more_than_8_children_is_refused():
    from diffphys_amd import hip_backend

    tpl = dict(template("mixed25"))
    par = np.array(tpl["joint_parent"]).reshape(-1).copy()
    assert (par == 0).sum() == 8
    hip_backend.joint_force_table_host(tpl)
    par[np.flatnonzero(par > 0)[0]] = 0   # a ninth child for the base
    tpl["joint_parent"] = par
    with pytest.raises(ValueError, match="9 children"):
        hip_backend.joint_force_table_host(tpl)


# ------------------------------------------------------------------------------------------------------------- (4) the C ABI
def test_pose_entries_check_the_new_op_without_a_gpu():
    from diffphys_amd import hip_backend

    lib = hip_backend.lib()
    err = lambda: lib.pd_last_error()
    assert hip_backend.POSE_JOINT_WRENCH == 13
    assert lib.pd_abi_version() == 9
    assert lib.pd_pose_op(13, 0, None, 13, None, None, None) == 0
    assert lib.pd_pose_op_vjp(13, 0, None, 13, None, None, None, None, None) == 0
    assert lib.pd_pose_op(13, 0, None, 256, None, None, None) == 0
    buf = (ctypes.c_float * 64)()   # host memory: the call must be refused before anything is launched or read
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.pd_pose_op(13, 26, None, 13, None, p, None) != 0 and b"NULL operand" in err()
    assert lib.pd_pose_op(13, 26, p, 13, None, p, None) != 0 and b"NULL operand" in err()
    assert lib.pd_pose_op_vjp(13, 26, None, 13, p, p, None, p, None) != 0 and b"NULL operand" in err()
    assert lib.pd_pose_op(13, 14, p, 13, p, p, None) != 0 and b"n % g" in err()
    assert lib.pd_pose_op_vjp(13, 14, p, 13, p, p, None, p, None) != 0 and b"n % g" in err()
    assert lib.pd_pose_op(13, 0, None, 0, None, None, None) != 0 and b"n % g" in err()   # a group size below 1 is refused at every n
    assert lib.pd_pose_op(13, 0, None, -3, None, None, None) != 0 and b"n % g" in err()
    # the cap on the bodies per state set, at every n
    assert lib.pd_pose_op(13, 0, None, 257, None, None, None) != 0 and b"at most 256" in err() and b"PD_POSE_JOINT_WRENCH" in err()
    assert lib.pd_pose_op_vjp(13, 257, p, 257, p, p, None, p, None) != 0 and b"at most 256" in err()
    # the table has no gradient: a non-NULL g_a is refused, at n = 0 too
    assert lib.pd_pose_op_vjp(13, 13, p, 13, p, p, p, p, None) != 0 and b"g_a" in err() and b"PD_POSE_JOINT_WRENCH" in err() and b"jointforce" in err()
    assert lib.pd_pose_op_vjp(13, 0, None, 13, None, None, p, None, None) != 0 and b"g_a" in err()
    # the refusal order is the shared one: n % g, the cap, g_a
    assert lib.pd_pose_op_vjp(13, 14, p, 13, p, p, p, p, None) != 0 and b"n % g" in err()
    assert lib.pd_pose_op_vjp(13, 257, p, 257, p, p, p, p, None) != 0 and b"at most 256" in err()
    off = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16 + 4)
    assert lib.pd_pose_op(13, 13, off, 13, p, p, None) != 0 and b"aligned" in err() and b"jointforce" in err()
    for op in (12, 14):   # the gap before the code and the code after it: unknown ops
        assert lib.pd_pose_op(op, 0, None, 13, None, None, None) != 0 and b"unknown op" in err()
        assert lib.pd_pose_op_vjp(op, 13, p, 13, p, p, None, p, None) != 0 and b"unknown op" in err()


# ------------------------------------------------------------------------------------------------------------ (5) the binding
class _Env:
    def __init__(self, tpl):
        self.nb, self._tpl, self._contact_table = int(tpl["nb"]), tpl, None

    def template(self):
        return self._tpl


def test_wrapper_refusals_without_a_gpu():
    from diffphys_amd import dp_model, dp_utils, hip_backend

    tpl = template("laikago")
    nb, nqd = int(tpl["nb"]), int(tpl["nqd"])
    table = hip_backend.joint_force_table(tpl, device="cpu")
    rows = torch.zeros(2 * nb, 25)
    with pytest.raises(ValueError, match="joint_force_table"):   # a bare tensor carries no dimensions
        hip_backend.joint_wrench(torch.zeros(table.numel()), nb, rows)
    with pytest.raises(ValueError, match="a joint table.*joint_force_table"):   # a table of another kind is refused by name
        hip_backend.joint_wrench(hip_backend.joint_table(tpl, "measured", device="cpu"), nb, rows)
    with pytest.raises(ValueError, match="a jointforce table"):
        hip_backend.joint_coords(table, nb, torch.zeros(2 * nb, 13))
    with pytest.raises(ValueError, match="a mass table"):
        hip_backend.joint_wrench_vjp(hip_backend.mass_table(tpl, device="cpu"), nb, rows, torch.zeros(2 * nb, 6))
    with pytest.raises(ValueError, match="25"):
        hip_backend.joint_wrench(table, nb, torch.zeros(2 * nb, 13))
    with pytest.raises(ValueError, match="25"):
        hip_backend.joint_wrench_vjp(table, nb, torch.zeros(2 * nb, 23), torch.zeros(2 * nb, 6))
    with pytest.raises(ValueError, match="multiple"):
        hip_backend.joint_wrench(table, nb, rows[:5])
    with pytest.raises(ValueError, match="nb"):
        hip_backend.joint_wrench(table, nb + 1, torch.zeros(2 * (nb + 1), 25))
    with pytest.raises(ValueError, match="GPU"):    # no CPU fallback: refused before any launch
        hip_backend.joint_wrench(table, nb, rows)
    with pytest.raises(ValueError, match="GPU"):
        hip_backend.joint_wrench_vjp(table, nb, rows, torch.zeros(2 * nb, 6))
    env = _Env(tpl)
    bq, bqd, c3, cd = torch.zeros(2, 3, nb, 7), torch.zeros(2, 3, nb, 6), torch.zeros(2, 3, nb, 3), torch.zeros(nqd)
    with pytest.raises(TypeError, match="GPU"):
        dp_model.JointWrench.apply(bq, bqd, c3, c3, c3, c3, env)
    with pytest.raises(TypeError, match="GPU"):
        dp_utils.joint_wrench(bq, bqd, env, cd, cd, cd)
    with pytest.raises(TypeError, match="GPU"):
        dp_utils.joint_wrench(bq.double(), bqd.double(), env, cd, cd, cd, cd)
    assert env._contact_table is None   # nothing was built for a refused call
    if torch.cuda.is_available():   # the shape checks sit behind the device check
        c = lambda a: a.cuda()
        gpu_table = hip_backend.joint_force_table(tpl, device="cuda")
        with pytest.raises(ValueError, match="g_out"):
            hip_backend.joint_wrench_vjp(gpu_table, nb, c(rows), torch.zeros(2 * nb, 8).cuda())
        with pytest.raises(TypeError, match="GPU"):
            hip_backend.joint_wrench_vjp(gpu_table, nb, c(rows), torch.zeros(2 * nb, 6))
        with pytest.raises(ValueError, match="body_q"):
            dp_utils.joint_wrench(c(bq)[..., :6], c(bqd), env, c(cd), c(cd), c(cd))
        with pytest.raises(ValueError, match="target_ke"):
            dp_utils.joint_wrench(c(bq), c(bqd), env, c(cd), c(cd)[:5], c(cd))
        with pytest.raises(ValueError, match="act3"):
            dp_model.JointWrench.apply(c(bq), c(bqd), c(c3)[:1], c(c3), c(c3), c(c3), env)


def test_rows_of_a_case_follow_the_slot_index():
    """joint_wrench_ref.rows25, the rows every GPU test launches: state, then act, target, ke, kd of dof qd_start + k in slot k, ``fill``
    in the slots no dof uses."""
    C = case("mixed25", 11)
    idx = slot_index(C["tpl"])
    r = rows25(C, fill=np.nan).reshape(11, C["nb"], 25)
    assert np.array_equal(r[..., :7], C["bq"]) and np.array_equal(r[..., 7:13], C["bqd"])
    for j, k in enumerate(("act", "target", "ke", "kd")):
        blk = r[..., 13 + 3 * j: 16 + 3 * j]
        assert np.isnan(blk[:, idx == C["nqd"]]).all() and (idx == C["nqd"]).any()
        assert np.array_equal(blk[:, idx < C["nqd"]], C[k][:, idx[idx < C["nqd"]]])
