"""Host side of the generalised-force op, PD_POSE_GENERALIZED_FORCE = 15: the argument checks of the two pose entries for the new op
code, a known answer, the three identities the float64 restatement (tests/generalized_force_ref.py) rests on -- virtual work, the
power of a rigid twist, the round trip with the joint wrench --, dp_utils.inertial_wrench against the oracle's integrator, the
restatement's gradients against finite differences, and the wrappers' refusals.  All without a GPU.

The identities are exact for unit quaternions and axes only: the templates' constants are fp32-rounded, 1e-7 off the sphere, which the
attachment gain turns into 2e-5 of max |wrench|.  So they run on a float64 copy of the template with its quaternions and axes
normalised in float64 (generalized_force_ref.unit_template).  Measured here: virtual work 9.7e-16, round trip 6.7e-15 (bars 1e-10), inertial_wrench 4.7e-14 (bar 1e-9)."""
import ctypes

import numpy as np
import pytest
import torch

from generalized_force_ref import EFFORTS, case, force_of, g_out_of, generalized_force, subtree_sums, unit_template
from helpers import relmax
from joint_coords_ref import joint_coords, oracle_template, random_coords
from joint_wrench_ref import controls, joint_wrench, template

F64 = torch.float64
IDENTITY_ROBOTS = ("laikago", "human", "mixed25", "cmp31", "worldmix9")


# ------------------------------------------------------------------------------------------------------------- (a) the C ABI
def test_pose_entries_check_the_new_op_without_a_gpu():
    from diffphys_amd import hip_backend

    lib = hip_backend.lib()
    err = lambda: lib.pd_last_error()
    assert hip_backend.POSE_GENERALIZED_FORCE == 15
    assert lib.pd_abi_version() == 9
    assert lib.pd_pose_op(15, 0, None, 13, None, None, None) == 0
    assert lib.pd_pose_op_vjp(15, 0, None, 13, None, None, None, None, None) == 0
    assert lib.pd_pose_op(15, 0, None, 256, None, None, None) == 0
    buf = (ctypes.c_float * 64)()   # host memory: the call must be refused before anything is launched or read
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.pd_pose_op(15, 26, None, 13, None, p, None) != 0 and b"NULL operand" in err()
    assert lib.pd_pose_op_vjp(15, 26, None, 13, p, p, None, p, None) != 0 and b"NULL operand" in err()
    # a bad group size, at every n
    assert lib.pd_pose_op(15, 14, p, 13, p, p, None) != 0 and b"n % g" in err()
    assert lib.pd_pose_op_vjp(15, 14, p, 13, p, p, None, p, None) != 0 and b"n % g" in err()
    assert lib.pd_pose_op(15, 0, None, 0, None, None, None) != 0 and b"n % g" in err()
    assert lib.pd_pose_op(15, 0, None, -3, None, None, None) != 0 and b"n % g" in err()
    # the cap on the bodies per state set, at every n
    assert lib.pd_pose_op(15, 0, None, 257, None, None, None) != 0 and b"at most 256" in err() and b"PD_POSE_GENERALIZED_FORCE" in err()
    assert lib.pd_pose_op_vjp(15, 257, p, 257, p, p, None, p, None) != 0 and b"at most 256" in err()
    # the table has no gradient: a non-NULL g_a is refused, at n = 0 too
    assert lib.pd_pose_op_vjp(15, 13, p, 13, p, p, p, p, None) != 0 and b"g_a" in err() and b"PD_POSE_GENERALIZED_FORCE" in err()
    assert lib.pd_pose_op_vjp(15, 0, None, 13, None, None, p, None, None) != 0 and b"g_a" in err()
    # the refusal order is the shared one: n % g, the cap, g_a
    assert lib.pd_pose_op_vjp(15, 14, p, 13, p, p, p, p, None) != 0 and b"n % g" in err()
    assert lib.pd_pose_op_vjp(15, 257, p, 257, p, p, p, p, None) != 0 and b"at most 256" in err()
    off = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16 + 4)
    assert lib.pd_pose_op(15, 13, off, 13, p, p, None) != 0 and b"aligned" in err() and b"joint table" in err()
    for op in (14, 16):   # the gap before the code and the code after it: unknown ops
        assert lib.pd_pose_op(op, 0, None, 13, None, None, None) != 0 and b"unknown op" in err()
        assert lib.pd_pose_op_vjp(op, 13, p, 13, p, p, None, p, None) != 0 and b"unknown op" in err()


# ------------------------------------------------------------------------------------------------------------ (b) a known answer
def _pendulum():
    """One REVOLUTE body on a hinge of the world (axis z, at height 0.5), its box -- and so its centre of mass -- 0.3 along its x."""
    from diffphys_amd import sim
    from helpers import build_template

    b = sim.ModelBuilder()
    b.add_articulation()
    body = b.add_body(origin=sim.transform_identity(), parent=-1, joint_xform=sim.transform((0.0, 0.5, 0.0), sim.quat_identity()),
                      joint_type=sim.JOINT_REVOLUTE, joint_axis=(0.0, 0.0, 1.0), joint_armature=0.01, joint_limit_ke=0.0, joint_limit_kd=0.0)
    b.add_shape_box(body, pos=(0.3, 0.0, 0.0), hx=0.05, hy=0.05, hz=0.05, density=1000.0, ke=1e4, kd=0.0, kf=1e2, mu=1.0)
    return build_template(b)


def test_a_horizontal_pendulum_carries_its_weight():
    """com at distance L from a world hinge about z, horizontal, f = (0, -m g, 0): tau = -m g L with the com on +x, +m g L on -x, 0 when
    it hangs straight down; a pure torque about the axis comes through unchanged."""
    from oracle import ref_torch as rt

    tpl = unit_template(_pendulum())
    T = oracle_template(tpl)
    assert T.nb == 1 and T.nqd == 1 and T.joint_type[0] == rt.JOINT_REVOLUTE
    L = float(np.linalg.norm(np.asarray(tpl["body_com"]).reshape(3)))
    assert abs(L - 0.3) < 1e-6
    m, g = float(np.asarray(tpl["body_mass"]).reshape(-1)[0]), 9.81
    q = torch.tensor([[0.0], [np.pi], [-np.pi / 2]], dtype=F64)
    bq, _ = rt.eval_fk(T, q, torch.zeros(3, 1, dtype=F64))
    bf = torch.zeros(3, 1, 6, dtype=F64)
    bf[:, 0, 4] = -m * g
    for efforts in EFFORTS:
        tau = generalized_force(T, bq, bf, efforts)[:, 0].numpy()
        assert np.allclose(tau, [-m * g * L, m * g * L, 0.0], rtol=0, atol=1e-12 * m * g * L)
    bf = torch.zeros(3, 1, 6, dtype=F64)
    bf[:, 0, 2] = 0.7
    assert np.allclose(generalized_force(T, bq, bf)[:, 0].numpy(), 0.7, rtol=0, atol=1e-14)


# ------------------------------------------------------------------------------------------------- (c), (d) the identities
def _fk_case(name, S=4, seed=0, zero_rates=False):
    """float64, on the unit template: (T, joint_q [S, nq] requiring grad, body_q, body_qd of eval_fk, random wrenches [S, nb, 6])"""
    from oracle import ref_torch as rt

    tpl = unit_template(template(name))
    T = oracle_template(tpl)
    q, qd = random_coords(tpl, S, seed=900 + seed, lo=0.05, hi=1.0)
    if zero_rates:
        qd = np.zeros_like(qd)
    jq = torch.tensor(q, dtype=F64, requires_grad=True)
    bq, bqd = rt.eval_fk(T, jq, torch.tensor(qd, dtype=F64))
    bf = torch.tensor(np.random.RandomState(77 + seed).randn(S, T.nb, 6), dtype=F64)
    return T, jq, bq, bqd, bf


@pytest.mark.parametrize("name", IDENTITY_ROBOTS)
def test_virtual_work(name):
    """W(q) = sum_b f_b . x_b(q) + t_b . 2 (q_b(q) conj(q_b0)).xyz on FK states: dW/dq by autograd through eval_fk equals the
    generalized-mode output on every REVOLUTE and COMPOUND dof, dW/d(root position) the FREE force part; the FREE moment through the
    power of a rigid twist of the whole robot about the root's centre of mass.  Bar 1e-10 of max |output|."""
    from oracle import ref_torch as rt

    T, jq, bq, _, bf = _fk_case(name)
    S = bq.shape[0]
    x = bq[..., :3] + rt.q_rot(bq[..., 3:], T.com[None].expand(S, T.nb, 3))
    dq = rt.q_mul(bq[..., 3:], rt.q_conj(bq[..., 3:].detach()))
    W = (bf[..., 3:] * x).sum() + (bf[..., :3] * 2.0 * dq[..., :3]).sum()
    (dW,) = torch.autograd.grad(W, jq)
    out = generalized_force(T, bq.detach(), bf, "generalized")
    scale = float(out.abs().max())
    worst, seen = 0.0, set()
    for i in range(T.nb):
        ty, qs, qds = T.joint_type[i], T.q_start[i], T.qd_start[i]
        if ty == rt.JOINT_REVOLUTE:
            worst = max(worst, float((dW[:, qs] - out[:, qds]).abs().max()))
        elif ty == rt.JOINT_COMPOUND:
            worst = max(worst, float((dW[:, qs: qs + 3] - out[:, qds: qds + 3]).abs().max()))
        elif ty == rt.JOINT_FREE:
            assert T.joint_parent[i] < 0
            worst = max(worst, float((dW[:, qs: qs + 3] - out[:, qds + 3: qds + 6]).abs().max()))
            # a rigid twist (omega, v of the root's centre of mass) of the whole robot: power = N(x_i) . omega + F . v
            rng = np.random.RandomState(5)
            om, v = torch.tensor(rng.randn(S, 3)), torch.tensor(rng.randn(S, 3))
            xb = x.detach()
            vb = v[:, None] + rt.cross(om[:, None].expand(S, T.nb, 3), xb - xb[:, i: i + 1])
            power = (bf[..., :3] * om[:, None]).sum((1, 2)) + (bf[..., 3:] * vb).sum((1, 2))
            q_wj = T.X_p[i, 3:].expand(S, 4)
            mine = (out[:, qds: qds + 3] * rt.q_rot_inv(q_wj, om)).sum(-1) + (out[:, qds + 3: qds + 6] * rt.q_rot_inv(q_wj, v)).sum(-1)
            worst = max(worst, float((power - mine).abs().max()))
        seen.add(ty)
    print("%s virtual work: %.2e of max |out| = %.3g" % (name, worst / scale, scale))
    assert worst <= 1e-10 * scale
    if name == "mixed25":
        assert seen == {rt.JOINT_REVOLUTE, rt.JOINT_COMPOUND, rt.JOINT_FREE, rt.JOINT_FIXED}


@pytest.mark.parametrize("zero_rates", [True, False])
@pytest.mark.parametrize("name", IDENTITY_ROBOTS)
def test_round_trip_with_the_joint_wrench(name, zero_rates):
    """On exact FK states the joint pass's wrenches (joint_wrench_ref.joint_wrench, the jaf of a step) read back in joint space: the
    actuator-mode entry of every REVOLUTE / COMPOUND dof is -jf, jf the joint force of that dof on the measured coordinates, and the
    six entries of a FREE root are zero -- the joints' pairs are internal forces.  Bar 1e-10 of max |jaf|."""
    from oracle import ref_torch as rt

    T, _, bq, bqd, _ = _fk_case(name, seed=3, zero_rates=zero_rates)
    bq, bqd = bq.detach(), bqd.detach()
    S = bq.shape[0]
    c = {k: torch.tensor(v, dtype=F64) for k, v in controls(np.random.RandomState(11), S, T.nqd).items()}
    jaf = joint_wrench(T, bq, bqd, c["target"], c["act"], c["ke"], c["kd"])
    out = generalized_force(T, bq, jaf, "actuator")
    jq, jqd = joint_coords(T, bq, bqd, "measured")
    one = torch.ones(S, 1, dtype=F64)
    scale = float(jaf.abs().max())
    worst = 0.0
    for i in range(T.nb):
        ty, qs, qds = T.joint_type[i], T.q_start[i], T.qd_start[i]
        for k in range({rt.JOINT_REVOLUTE: 1, rt.JOINT_COMPOUND: 3}.get(ty, 0)):
            j = qds + k
            assert float(T.limit_lower[j]) < float(jq[:, qs + k].min()) and float(jq[:, qs + k].max()) < float(T.limit_upper[j])
            jf = rt.eval_joint_force(jq[:, qs + k], jqd[:, j], c["target"][:, j], c["ke"][:, j], c["kd"][:, j], c["act"][:, j],
                                     T.limit_lower[j], T.limit_upper[j], T.limit_ke[j], T.limit_kd[j], one)[:, 0]
            worst = max(worst, float((out[:, j] + jf).abs().max()))
        if ty == rt.JOINT_FREE:
            worst = max(worst, float(out[:, qds: qds + 6].abs().max()))
    print("%s round trip (zero rates %s): %.2e of max |jaf| = %.3g" % (name, zero_rates, worst / scale, scale))
    assert scale > 0 and worst <= 1e-10 * scale


# ------------------------------------------------------------------------------------------------------- (e) inertial_wrench
class _Env:
    def __init__(self, tpl):
        self.nb, self._tpl, self._contact_table = int(tpl["nb"]), tpl, None

    def template(self):
        return self._tpl


@pytest.mark.parametrize("name", ["laikago", "human"])
def test_inertial_wrench_inverts_the_integrator(name):
    """float64 on the CPU: a state stepped by ref_torch.integrate_bodies with a random body_f, no clamp active (asserted: |w'|, |v'| < 10)
    -> dp_utils.inertial_wrench recovers body_f to 1e-9 of its largest entry; gravity, the gyroscopic term and the damping included."""
    from diffphys_amd import dp_utils
    from oracle import ref_torch as rt

    tpl = template(name)
    T = oracle_template(tpl)
    S, nb, dt = 4, T.nb, 5e-4
    q, qd = random_coords(tpl, S, seed=21, lo=0.05, hi=1.0)
    bq, bqd = rt.eval_fk(T, torch.tensor(q), torch.tensor(qd))
    bq = torch.cat([bq[..., :3], rt.q_normalize(bq[..., 3:])], -1)
    rng = np.random.RandomState(3)
    mass = torch.tensor(np.tile(np.asarray(tpl["body_mass"], np.float64), (S, 1)) * rng.uniform(0.8, 1.25, (S, nb)))
    I = torch.tensor(np.tile(np.asarray(tpl["body_inertia"], np.float64).reshape(1, nb, 3, 3), (S, 1, 1, 1))) * (mass / mass.mean())[..., None, None]
    body_f = torch.tensor(rng.randn(S, nb, 6))
    body_f[..., :3] *= float(I.abs().max()) * 50.0   # torques the bodies' inertias can take without reaching the clamp
    _, nxt = rt.integrate_bodies(T, bq, bqd, body_f, 1.0 / mass, I, torch.linalg.inv(I), dt)
    assert float(nxt.abs().max()) < 10.0 and float((nxt[..., :3] - bqd[..., :3]).abs().max()) > 1e-4
    back = dp_utils.inertial_wrench(bq, bqd, nxt, dt, mass, I, _Env(tpl))
    assert back.shape == body_f.shape and back.dtype == F64
    e = relmax(back.numpy(), body_f.numpy())
    print("%s inertial_wrench: %.2e" % (name, e))
    assert e <= 1e-9
    # differentiable by autograd in the states
    nx = nxt.clone().requires_grad_(True)
    dp_utils.inertial_wrench(bq, bqd, nx, dt, mass, I, _Env(tpl)).sum().backward()
    assert nx.grad is not None and float(nx.grad.abs().max()) > 0


# ------------------------------------------------------------------------------------- (f) the restatement's own gradients
@pytest.mark.parametrize("efforts", EFFORTS)
@pytest.mark.parametrize("name", ["mixed25", "human", "worldmix9"])
def test_restatement_gradients_against_finite_differences(name, efforts):
    """float64: <autograd gradient, direction> against the central difference of <g_out, out> along three random directions of (poses,
    wrenches), step 1e-6: 1e-7 relative."""
    C = case(name, 2)
    g_out = g_out_of(C)
    r = force_of(C, F64, efforts, g_out)
    T = oracle_template(C["tpl"])
    bq, bf = torch.tensor(np.array(C["bq"]), dtype=F64), torch.tensor(np.array(C["bf"]), dtype=F64)
    L = lambda a, b: float((generalized_force(T, a, b, efforts) * torch.as_tensor(g_out, dtype=F64)).sum())
    rng = np.random.RandomState(8)
    for _ in range(3):
        dq, df = torch.tensor(rng.randn(*bq.shape)), torch.tensor(rng.randn(*bf.shape))
        h = 1e-6
        fd = (L(bq + h * dq, bf + h * df) - L(bq - h * dq, bf - h * df)) / (2 * h)
        an = float((torch.as_tensor(r["g_body_q"]) * dq).sum() + (torch.as_tensor(r["g_body_f"]) * df).sum())
        assert abs(fd - an) <= 1e-7 * max(abs(an), 1.0), (fd, an)


def test_the_sums_do_not_depend_on_the_reference_point():
    """float64: moving every position by (300, 0, -200) m changes no output beyond rounding (the moments are taken about the set's own
    body 0), and the subtree sums of the root hold the whole set's wrench."""
    near, far = case("laikago", 3), case("laikago", 3, (300.0, 0.0, -200.0))
    a, b = force_of(near, F64, "actuator")["out"], force_of(far, F64, "actuator")["out"]
    assert relmax(b, a) <= 1e-4   # (the fp32 rounding of the shifted positions moves the states themselves by 3e-5 m)
    T = oracle_template(near["tpl"])
    bq, bf = torch.tensor(np.array(near["bq"]), dtype=F64), torch.tensor(np.array(near["bf"]), dtype=F64)
    F, _, _, _ = subtree_sums(T, bq, bf)
    assert torch.allclose(F[0], bf[..., 3:].sum(1), rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------------------ (g) the binding
def test_wrapper_refusals_without_a_gpu():
    from diffphys_amd import dp_model, dp_utils, hip_backend

    tpl = template("laikago")
    nb, nqd = int(tpl["nb"]), int(tpl["nqd"])
    assert hip_backend.efforts_mode("actuator") == "measured" and hip_backend.efforts_mode("generalized") == "generalized"
    with pytest.raises(ValueError, match="efforts"):
        hip_backend.efforts_mode("measured")
    table = hip_backend.joint_table(tpl, "measured", device="cpu")   # the joint table of joint_coords, byte for byte
    assert np.array_equal(table.numpy(), hip_backend.joint_table_host(tpl, "measured")) and table[3] == 0
    rows = torch.zeros(2 * nb, 13)
    with pytest.raises(ValueError, match="joint_table"):   # a bare tensor carries no dimensions
        hip_backend.generalized_force(torch.zeros(table.numel()), nb, rows)
    with pytest.raises(ValueError, match="a jointforce table"):
        hip_backend.generalized_force(hip_backend.joint_force_table(tpl, device="cpu"), nb, rows)
    with pytest.raises(ValueError, match=r"\(p, q xyzw, t, f\)"):
        hip_backend.generalized_force(table, nb, torch.zeros(2 * nb, 12))
    with pytest.raises(ValueError, match="multiple"):
        hip_backend.generalized_force(table, nb, rows[:5])
    with pytest.raises(ValueError, match="nb"):
        hip_backend.generalized_force_vjp(table, nb + 1, torch.zeros(2 * (nb + 1), 13), torch.zeros(2, nqd))
    with pytest.raises(ValueError, match="GPU"):    # no CPU fallback: refused before any launch
        hip_backend.generalized_force(table, nb, rows)
    with pytest.raises(ValueError, match="GPU"):
        hip_backend.generalized_force_vjp(table, nb, rows, torch.zeros(2, nqd))
    env = _Env(tpl)
    bq, bf = torch.zeros(2, 3, nb, 7), torch.zeros(2, 3, nb, 6)
    with pytest.raises(TypeError, match="GPU"):
        dp_model.GeneralizedForce.apply(bq, bf, env, "actuator")
    with pytest.raises(TypeError, match="GPU"):
        dp_utils.generalized_force(bq, bf, env)
    with pytest.raises(TypeError, match="GPU"):
        dp_utils.generalized_force(bq.double(), bf.double(), env, efforts="generalized")
    with pytest.raises(TypeError, match="GPU"):   # inverse_dynamics ends in the op: HIP only
        dp_utils.inverse_dynamics(bq, bf, bf, 1e-3, torch.ones(nb), torch.eye(3).expand(nb, 3, 3), env)
    assert env._contact_table is None   # nothing was built for a refused call
    if torch.cuda.is_available():   # the shape and mode checks sit behind the device check
        with pytest.raises(ValueError, match="body_q"):
            dp_utils.generalized_force(bq.cuda()[..., :6], bf.cuda(), env)
        with pytest.raises(ValueError, match="efforts"):
            dp_utils.generalized_force(bq.cuda(), bf.cuda(), env, efforts="measured")
