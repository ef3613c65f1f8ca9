"""Host side of the joint-coordinates op (PD_POSE_JOINT_COORDS, the inverse of forward kinematics): the argument checks of the two pose
entries for the new op code, the joint table's layout, and the float64 restatement the GPU tests hold the kernels to
(tests/joint_coords_ref.py) against oracle/ref_torch.py -- all without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

from joint_coords_ref import (WIDTH, compound_axes, joint_coords, joint_frame, load_tpl, oracle_template, random_coords)

TEMPLATES = ["laikago", "human", "laikago_toes"]


def test_pose_entries_check_the_new_op_without_a_gpu():
    from diffphys_amd import hip_backend

    lib = hip_backend.lib()
    err = lambda: lib.pd_last_error()
    assert hip_backend.POSE_JOINT_COORDS == 6
    assert lib.pd_abi_version() == 9
    assert lib.pd_pose_op(6, 0, None, 13, None, None, None) == 0
    assert lib.pd_pose_op_vjp(6, 0, None, 13, None, None, None, None, None) == 0
    assert lib.pd_pose_op(6, 26, None, 13, None, None, None) != 0   # a NULL operand
    buf = (ctypes.c_float * 64)()   # host memory: the call must be refused before anything is launched or read
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.pd_pose_op(6, 26, None, 13, None, p, None) != 0 and b"NULL operand" in err()
    assert lib.pd_pose_op(6, 14, p, 13, p, p, None) != 0
    assert b"n % g" in err()
    assert lib.pd_pose_op_vjp(6, 14, p, 13, p, p, None, p, None) != 0
    assert b"n % g" in err()
    assert lib.pd_pose_op(6, 0, None, 0, None, None, None) != 0 and b"n % g" in err()   # a group size below 1 is refused at every n
    assert lib.pd_pose_op(6, 0, None, -3, None, None, None) != 0
    assert lib.pd_pose_op(6, 0, None, 257, None, None, None) != 0 and b"256" in err()  # more bodies than a workgroup places
    # the joint table has no gradient: a non-NULL g_a is refused, at n = 0 too
    assert lib.pd_pose_op_vjp(6, 13, p, 13, p, p, p, p, None) != 0 and b"g_a" in err()
    assert lib.pd_pose_op_vjp(6, 13, p, 13, p, p, p, None, None) != 0 and b"g_a" in err()
    assert lib.pd_pose_op_vjp(6, 0, None, 13, None, None, p, None, None) != 0 and b"g_a" in err()
    for op in (7, 8):   # unknown ops
        assert lib.pd_pose_op(op, 0, None, 13, None, None, None) != 0 and b"unknown op" in err()
        assert lib.pd_pose_op(op, 13, p, 13, p, p, None) != 0
        assert lib.pd_pose_op_vjp(op, 13, p, 13, p, p, None, p, None) != 0 and b"unknown op" in err()


@pytest.mark.parametrize("name", TEMPLATES)
def test_joint_table_layout(name):
    from diffphys_amd import hip_backend

    tpl = load_tpl(name)
    nb, nq, nqd = int(tpl["nb"]), int(tpl["nq"]), int(tpl["nqd"])
    t = hip_backend.joint_table_host(tpl, "generalized")
    L = hip_backend.joint_table_layout(nb)
    assert t.dtype == np.float32 and t.size == L["floats"] and t.size % 4 == 0
    assert L["bodies"] == 4 and L["children"] == 4 + 24 * nb and L["floats"] == 4 + 32 * nb
    assert t[:4].tolist() == [nb, nq, nqd, 1]
    tm = hip_backend.joint_table_host(tpl, "measured")
    assert tm[:4].tolist() == [nb, nq, nqd, 0] and np.array_equal(tm[4:], t[4:])
    body = t[L["bodies"]: L["children"]].reshape(nb, 24)
    kids = t[L["children"]:].reshape(nb, 8)
    par = np.asarray(tpl["joint_parent"]).reshape(nb)
    assert np.array_equal(body[:, 0], par) and np.array_equal(body[:, 1], np.asarray(tpl["joint_type"]).reshape(nb))
    assert np.array_equal(body[:, 2], np.asarray(tpl["joint_q_start"]).reshape(-1)[:nb])
    assert np.array_equal(body[:, 3], np.asarray(tpl["joint_qd_start"]).reshape(-1)[:nb])
    assert np.array_equal(body[:, 4:11], np.asarray(tpl["joint_X_p"], np.float32).reshape(nb, 7))
    assert np.array_equal(body[:, 11:14], np.asarray(tpl["joint_axis"], np.float32).reshape(nb, 3))
    assert np.array_equal(body[:, 14:18], np.asarray(tpl["joint_X_c"], np.float32).reshape(nb, 7)[:, 3:])
    assert np.array_equal(body[:, 18:21], np.asarray(tpl["body_com"], np.float32).reshape(nb, 3))
    assert (body[:, 22:] == 0).all()
    seen = 0
    for b in range(nb):
        ch = [c for c in range(nb) if par[c] == b]   # template order
        assert body[b, 21] == len(ch) and kids[b, :len(ch)].tolist() == ch and (kids[b, len(ch):] == -1).all()
        seen += len(ch)
    assert seen == int((par >= 0).sum())   # every body with a parent is the child of exactly one
    # the joints' coordinates tile [0, nq) and [0, nqd) exactly: every output float of the op has one owner
    own_q, own_qd = np.zeros(nq, int), np.zeros(nqd, int)
    for b in range(nb):
        wq, wqd = WIDTH[int(body[b, 1])]
        own_q[int(body[b, 2]): int(body[b, 2]) + wq] += 1
        own_qd[int(body[b, 3]): int(body[b, 3]) + wqd] += 1
    assert (own_q == 1).all() and (own_qd == 1).all()
    if name == "laikago_toes":
        assert (body[:, 1] == 3).sum() == 4 and nb == 17


def test_joint_table_refusals_and_wrapper_checks_without_a_gpu():
    from diffphys_amd import dp_model, dp_utils, hip_backend

    tpl = load_tpl("laikago")
    nb = int(tpl["nb"])
    with pytest.raises(ValueError, match="rates"):
        hip_backend.joint_table_host(tpl, "both")
    star = dict(tpl)   # a root with nine children
    star.update(nb=10, nq=7 + 9, nqd=6 + 9, joint_type=np.asarray([4] + [1] * 9), joint_parent=np.asarray([-1] + [0] * 9),
                joint_q_start=np.asarray([0] + list(range(7, 16))), joint_qd_start=np.asarray([0] + list(range(6, 15))),
                joint_X_p=np.tile(np.asarray([0, 0, 0, 0, 0, 0, 1.0], np.float32), (10, 1)),
                joint_X_c=np.tile(np.asarray([0, 0, 0, 0, 0, 0, 1.0], np.float32), (10, 1)),
                joint_axis=np.tile(np.asarray([1.0, 0, 0], np.float32), (10, 1)), body_com=np.zeros((10, 3), np.float32))
    with pytest.raises(ValueError, match="children"):
        hip_backend.joint_table_host(star)
    star["joint_parent"] = np.asarray([-1] + [0] * 8 + [1])
    assert hip_backend.joint_table_host(star).size == 4 + 32 * 10
    star["joint_q_start"] = np.asarray([0] + list(range(7, 15)) + [16])
    with pytest.raises(ValueError, match="coordinates"):
        hip_backend.joint_table_host(star)
    table = hip_backend.joint_table(tpl, device="cpu")
    assert hip_backend._table_tag(table) == ("joint", (nb, int(tpl["nq"]), int(tpl["nqd"])))
    state = torch.zeros(2 * nb, 13)
    with pytest.raises(ValueError, match="joint_table"):   # a bare tensor carries no dimensions
        hip_backend.joint_coords(torch.zeros(table.numel()), nb, state)
    with pytest.raises(ValueError, match="joint_table"):   # nor does a table of another kind stand in: the tag names the kind
        hip_backend.joint_coords(hip_backend.mass_table(tpl, device="cpu"), nb, state)
    with pytest.raises(ValueError, match="13"):
        hip_backend.joint_coords(table, nb, torch.zeros(2 * nb, 7))
    with pytest.raises(ValueError, match="multiple"):
        hip_backend.joint_coords(table, nb, state[:5])
    with pytest.raises(ValueError, match="nb"):
        hip_backend.joint_coords(table, nb + 1, torch.zeros(2 * (nb + 1), 13))
    with pytest.raises(ValueError, match="GPU"):    # no CPU fallback: refused before any launch
        hip_backend.joint_coords(table, nb, state)
    with pytest.raises(ValueError, match="GPU"):
        hip_backend.joint_coords_vjp(table, nb, state, torch.zeros(2, int(tpl["nq"])), torch.zeros(2, int(tpl["nqd"])))

    class Env:
        pass

    env = Env()
    env.nb = nb
    bq, bqd = torch.zeros(2, 3, nb, 7), torch.zeros(2, 3, nb, 6)
    with pytest.raises(TypeError, match="GPU"):
        dp_model.InverseKinematics.apply(bq, bqd, env)
    with pytest.raises(TypeError, match="GPU"):
        dp_utils.joint_coords(bq, bqd, env)
    with pytest.raises(TypeError, match="GPU"):
        dp_utils.joint_coords(bq.double(), bqd.double(), env, "measured")


# float64 errors of IK(FK(q, qd)) recorded for the shipped compound robots with |angles| <= 1 (their joint_X_p quaternions are fp32 numbers,
# unit only to 3e-8: the residual is the fixtures', not arithmetic): (angles and FREE coordinates, generalized rates); the bar is 4 x these
RECORDED = {"human": (3.7e-7, 2.5e-6), "quad": (5.3e-7, 2.5e-6)}


@pytest.mark.parametrize("name", ["laikago", "laikago_toes", "human", "quad"])
def test_restatement_inverts_eval_fk(name):
    bar = tuple(4 * r for r in RECORDED[name]) if name in RECORDED else (1e-12, 1e-12)
    restatement_against_eval_fk(load_tpl(name), name, *bar)


def restatement_against_eval_fk(tpl, name, bar_q, bar_qd):
    """IK(FK(q, qd)) in float64 on 64 random coordinate sets, and the measured rates against eval_body_joints' axes (shared with
    tests/test_state_ops_generated_host.py, which runs it on generated robots)."""
    from oracle import ref_torch as rt

    T = oracle_template(tpl)
    S = 64
    q, qd = (torch.as_tensor(a) for a in random_coords(tpl, S, seed=11))
    bq, bqd = rt.eval_fk(T, q, qd)
    jq, jqd = joint_coords(T, bq, bqd, "generalized")
    e_q, e_qd = float((jq - q).abs().max()), float((jqd - qd).abs().max())
    print("%s: IK(FK) max |dq| %.2e, max |dqd| %.2e (generalized)" % (name, e_q, e_qd))
    assert e_q <= bar_q and e_qd <= bar_qd, (e_q, e_qd)
    mq, mqd = joint_coords(T, bq, bqd, "measured")
    assert torch.equal(mq, jq)
    comp = [i for i in range(T.nb) if T.joint_type[i] == rt.JOINT_COMPOUND]
    other = np.ones(T.nqd, bool)
    worst = 0.0
    for i in comp:   # measured rates: dot(axis_k, w_err) on eval_body_joints' axes (ref_torch.py:308-323), exactly
        qds = T.qd_start[i]
        other[qds: qds + 3] = False
        _, q_p, w_p, _ = joint_frame(T, bq, bqd, i)
        q_c, q_off = bq[:, i, 3:], T.X_c[i, 3:].expand(S, 4)
        q_pc = rt.q_mul(rt.q_mul(rt.q_mul(rt.q_conj(q_off), rt.q_conj(q_p)), q_c), q_off)
        angles = rt.quat_decompose(q_pc)
        q_w = rt.q_mul(q_p, q_off)
        w_err = bqd[:, i, :3] - w_p
        for k, ax in enumerate(compound_axes(angles)):
            assert torch.equal(mqd[:, qds + k], rt.dot(rt.q_rot(q_w, ax), w_err))
        worst = max(worst, float((mqd[:, qds: qds + 3] - qd[:, qds: qds + 3]).abs().max()))
    assert torch.equal(mqd[:, other], jqd[:, other])   # the two modes differ for COMPOUND joints only
    if comp:
        print("%s: measured compound rates differ from the generalised velocities by up to %.2f" % (name, worst))
        assert worst > 0.5   # ... and there they are another quantity, not a rounding of the same one


@pytest.mark.parametrize("name", ["laikago", "human"])
def test_restatement_gives_the_numbers_the_joint_pass_acts_on(name):
    """A state 20 steps into the float64 rollout of a robot kicked into the ground (joints slightly violated): the restatement's revolute
    and compound angles against the lines of eval_body_joints (ref_torch.py:291-298 with its literal acos, :308-310)."""
    from diffphys_amd import synth
    from helpers import INPUT_NAMES
    from oracle import ref_torch as rt

    tpl = load_tpl(name)
    T = oracle_template(tpl)
    bs, nsteps = 2, 20
    inp = synth.make_inputs(tpl, name, bs=bs, nsteps=nsteps, seed=3, penetration=0.004)
    t = [torch.as_tensor(np.asarray(inp[k]), dtype=torch.float64) for k in INPUT_NAMES]
    allq, allqd = rt.rollout(T, *t, nsteps, [0], inp["dt"], return_all=True)
    bq, bqd = allq[nsteps], allqd[nsteps]
    assert float((bq - allq[0]).abs().max()) > 1e-4   # it moved
    assert restatement_against_the_joint_pass(T, bq, bqd) >= 12


def restatement_against_the_joint_pass(T, bq, bqd):
    """The restatement's measured coordinates of float64 states [bs, nb, 7], [bs, nb, 6] against the lines of eval_body_joints, for
    every REVOLUTE and COMPOUND joint -> their number (shared with tests/test_state_ops_generated_host.py)."""
    from oracle import ref_torch as rt

    bs = bq.shape[0]
    jq, jqd = joint_coords(T, bq, bqd, "measured")
    seen = 0
    for i in range(T.nb):
        ty, qs, qds = T.joint_type[i], T.q_start[i], T.qd_start[i]
        if ty not in (rt.JOINT_REVOLUTE, rt.JOINT_COMPOUND):
            continue
        _, q_p, w_p, _ = joint_frame(T, bq, bqd, i)
        q_c = bq[:, i, 3:]
        r_err = rt.q_mul(rt.q_conj(q_p), q_c)
        w_err = bqd[:, i, :3] - w_p
        if ty == rt.JOINT_REVOLUTE:
            axis = T.axis[i].expand(bs, 3)
            a = rt.dot(r_err[:, :3], axis)[:, None] * axis
            twist = rt.q_normalize(torch.cat([a, r_err[:, 3:]], -1))
            sgn = torch.where(rt.dot(axis, twist[:, :3]) < 0, -1.0, 1.0).to(T.dtype)
            q = rt.acos_g(twist[:, 3]) * 2.0 * sgn
            qd = rt.dot(w_err, rt.q_rot(q_p, axis))
            assert float((jq[:, qs] - q).abs().max()) <= 1e-12, (i, jq[:, qs], q)
            assert float((jqd[:, qds] - qd).abs().max()) <= 1e-12
        else:
            q_off = T.X_c[i, 3:].expand(bs, 4)
            angles = rt.quat_decompose(rt.q_mul(rt.q_mul(rt.q_mul(rt.q_conj(q_off), rt.q_conj(q_p)), q_c), q_off))
            assert float((jq[:, qs: qs + 3] - angles).abs().max()) <= 1e-12
        seen += 1
    assert seen == sum(ty in (rt.JOINT_REVOLUTE, rt.JOINT_COMPOUND) for ty in T.joint_type)
    return seen
