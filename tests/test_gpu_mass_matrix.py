"""The joint-space mass matrix of a state (``pd_pose_op`` / ``pd_pose_op_vjp`` PD_POSE_MASS_MATRIX, k_mass_matrix and k_mass_matrix_vjp of
csrc/pd_pose.hip, dp_model.MassMatrix, dp_utils.mass_matrix(method="crba"), forward_dynamics(method="crba"),
phys_model.query(mass_matrix=True)) on a real MI355X (run with -m gpu).

Reference: mass_inverse_ref.dense_H in float64 -- H = sum_b J_b^T M_b J_b from the body twists' Jacobian, NOT the recursion the kernel
runs (tests/test_mass_matrix_host.py holds the recursion's restatement to it) -- on the SAME fp32 rows as the GPU; yardstick: the same
dense_H evaluated in fp32 torch.  Two bars, both printed:
  scaled      E(H) = max_ab |H - H64|_ab / sqrt(H64_aa H64_bb)  <= max(4 E(fp32 torch), 1e-5)   (H spans four orders of magnitude: a
              FREE block is about 20, distal hinges about 2e-3)
  per tensor  max |H - H64| / max |H64|  <= max(4 x fp32 torch, 1e-5), the project's bar; the gradients' bar, per tensor.

Measured on one MI355X: see DESIGN.md section 8."""
import functools

import numpy as np
import pytest
import torch

from body_accel_ref import rnea
from gpu_harness import dev  # noqa: F401
from helpers import relmax
from joint_coords_ref import oracle_template
from mass_inverse_ref import inverse_of, r_of, rows23, unslot
from mass_matrix_ref import (ALL_CASES, RATES, accel_case, body_weights, g_out_of, matrix_of, related_mask, robot_template, rows17,
                             scaled_error)

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32


def bar(what, gpu, f32, ref, floor=1e-5):
    e_gpu, e_32 = relmax(gpu, ref), relmax(f32, ref)
    print("%s: GPU %.2e, fp32 torch %.2e" % (what, e_gpu, e_32))
    assert np.isfinite(np.asarray(gpu)).all(), what
    assert np.isfinite(e_gpu) and e_gpu <= max(4 * e_32, floor), "%s: GPU error %.2e vs fp32 torch %.2e" % (what, e_gpu, e_32)


def scaled_bar(what, gpu, f32, ref, floor=1e-5):
    e_gpu, e_32 = scaled_error(gpu, ref), scaled_error(f32, ref)
    print("%s scaled: GPU %.2e, fp32 torch %.2e" % (what, e_gpu, e_32))
    assert np.isfinite(e_gpu) and e_gpu <= max(4 * e_32, floor), "%s: scaled GPU error %.2e vs fp32 torch %.2e" % (what, e_gpu, e_32)


@functools.lru_cache(maxsize=None)
def dense(name, S, shift, rates, dtype):
    """dense_H of a case: computed once, never written"""
    return matrix_of(accel_case(name, S, shift), dtype, rates)["out"]


@functools.lru_cache(maxsize=None)
def gpu_table(name, rates):
    from diffphys_amd import hip_backend

    return hip_backend.joint_table(robot_template(name), rates, torch.device("cuda:0"))


def launch(C, name, rates, dev, rows=None):
    """-> H [S, nqd, nqd] as numpy"""
    from diffphys_amd import hip_backend

    r = torch.from_numpy(rows17(C) if rows is None else rows).to(dev)
    out = hip_backend.mass_matrix(gpu_table(name, rates), C["nb"], r)
    assert out.shape == (r.shape[0] // C["nb"], C["nqd"], C["nqd"])
    return out.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ 1. values and structure
@pytest.mark.parametrize("rates", RATES)
@pytest.mark.parametrize("name,S,shift", ALL_CASES)
def test_op_matches_the_float64_matrix(name, S, shift, rates, dev):
    """H against float64 dense_H on the same fp32 rows.  mixed25 (a body with 8 children), rev64 (depth 64), rev256 (the cap, 256 KB of
    output per set), freeleaf5 (a FREE joint below a body), worldmix9 / world5 (massless FIXED bases) and the far-shifted Laikago (the
    reference point) catch a wrong sweep, cap, lever or hand-over.  Then the structure: the same bits on both sides of the diagonal,
    exact zeros between dofs of unrelated bodies."""
    C = accel_case(name, S, shift)
    H = launch(C, name, rates, dev)
    what = "%s x %d%s %s H" % (name, S, " far" if shift else "", rates)
    missed = []
    for check in (scaled_bar, bar):   # both figures are printed before a miss ends the test
        try:
            check(what, H, dense(name, S, shift, rates, F32), dense(name, S, shift, rates, F64))
        except AssertionError as e:
            missed.append(str(e))
    assert not missed, "; ".join(missed)
    assert np.array_equal(H, H.transpose(0, 2, 1))
    mask = related_mask(C["tpl"])
    assert (H[:, ~mask] == 0).all()
    if name == "mixed25":   # the body that gathers 8 children is in the comparison, and there are unrelated dofs
        assert (np.asarray(C["tpl"]["joint_parent"]).reshape(-1) == 0).sum() == 8 and (~mask).sum() > 0


def test_a_table_of_another_nb_gives_zeros(dev):
    """The library cannot validate a device buffer: both kernels check the table's nb against the call's and write zeros (no row of
    the table is read)."""
    from diffphys_amd import hip_backend

    C = accel_case("cmp31", 3)
    wrong = gpu_table("mixed25", "measured").clone()   # 4 + 32 * 25 floats: shorter than the table of 31 bodies
    _, (nb25, nq25, nqd25) = hip_backend._table_tag(gpu_table("mixed25", "measured"))
    assert nb25 == 25
    wrong._pd_table = ("joint", (31, nq25, nqd25))   # ... passed off as one
    rows = torch.from_numpy(rows17(C)).to(dev)
    out = hip_backend.mass_matrix(wrong, 31, rows)
    assert out.shape == (3, nqd25, nqd25) and (out == 0).all()
    g = hip_backend.mass_matrix_vjp(wrong, 31, rows, torch.ones(3, nqd25, nqd25, device=dev))
    assert g.shape == (93, 17) and (g == 0).all()


# ------------------------------------------------------------------------------------------------------------ 2. the shipped ops
@pytest.mark.parametrize("name,S", [("laikago", 41), ("human", 3), ("rev64", 5)])
def test_matrix_times_mass_inverse_is_the_identity(name, S, dev):
    """H (this op) applied to mass_inverse(r) (op 21) against r, in both modes; the products are formed in float64 from the fp32 outputs,
    so the figure is the two ops' own error.  Yardstick: the fp32 torch chain dense_H @ the restated recursion."""
    from diffphys_amd import hip_backend

    C = accel_case(name, S)
    tpl, nb = C["tpl"], C["nb"]
    for rates in RATES:
        H = launch(C, name, rates, dev).astype(np.float64)
        x = hip_backend.mass_inverse(gpu_table(name, rates), nb, torch.from_numpy(rows23(C)).to(dev)).cpu().numpy().reshape(S, nb, 6)
        to_dofs = lambda x6: unslot(tpl, torch.as_tensor(np.asarray(x6, np.float64))).numpy()
        r = to_dofs(r_of(C))
        x32 = inverse_of(C, F32, rates)["out"]
        apply = lambda M, v: np.einsum("sab,sb->sa", np.asarray(M, np.float64), to_dofs(v))
        bar("%s x %d %s H @ mass_inverse(r) against r" % (name, S, rates), apply(H, x), apply(dense(name, S, None, rates, F32), x32), r)


@pytest.mark.parametrize("name,S", [("laikago", 5), ("human", 3)])
def test_crba_against_jacobian_through_dp_utils(name, S, dev):
    """dp_utils.mass_matrix(method="crba") against method="jacobian" (the comparison path: op 17 on S * nqd * nb rows and plain torch):
    their difference over sqrt(H64_aa H64_bb) inside the same bar, max(4 E(fp32 torch dense_H), 1e-5); both against float64 printed.
    The default method keeps its bits."""
    from diffphys_amd import dp_utils, sim

    C = accel_case(name, S)
    tpl = C["tpl"]
    env = sim.Model.from_template(tpl, S, dev)
    m32, I32 = body_weights(tpl, 1, F32)
    bq, m, I = torch.from_numpy(np.array(C["bq"])).to(dev), m32[0].to(dev), I32[0].to(dev)
    a = dp_utils.mass_matrix(bq, m, I, env, method="crba")
    b = dp_utils.mass_matrix(bq, m, I, env, method="jacobian")
    assert torch.equal(b, dp_utils.mass_matrix(bq, m, I, env))
    assert a.shape == b.shape == (S, C["nqd"], C["nqd"])
    assert np.array_equal(a.cpu().numpy(), launch(C, name, "generalized", dev))
    H64, H32 = dense(name, S, None, "generalized", F64), dense(name, S, None, "generalized", F32)
    e32 = scaled_error(H32, H64)
    diff = scaled_error(H64 + (a.cpu().numpy().astype(np.float64) - b.cpu().numpy().astype(np.float64)), H64)
    print("%s x %d crba - jacobian scaled: %.2e; crba %.2e, jacobian %.2e, fp32 torch %.2e" % (
        name, S, diff, scaled_error(a.cpu().numpy(), H64), scaled_error(b.cpu().numpy(), H64), e32))
    assert diff <= max(4 * e32, 1e-5)
    with pytest.raises(ValueError, match="crba"):
        dp_utils.mass_matrix(bq, m, I, env, method="jacobian", rates="measured")
    am = dp_utils.mass_matrix(bq, m, I, env, method="crba", rates="measured")
    assert np.array_equal(am.cpu().numpy(), launch(C, name, "measured", dev))


# ------------------------------------------------------------------------------------------------------------ 3. gradients
@pytest.mark.parametrize("rates", RATES)
@pytest.mark.parametrize("name,S,shared", [("laikago", 5, False), ("laikago", 5, True), ("human", 3, False), ("cmp31", 3, False),
                                           ("mixed25", 3, False), ("freeleaf5", 4, True), ("rev64", 2, False)])
def test_gradients_through_dp_utils(name, S, shared, rates, dev):
    """dp_utils.mass_matrix(method="crba") differentiated in body_q, body_mass and body_inertia (k_mass_matrix_vjp) under a random,
    NOT symmetric upstream gradient, against float64 autograd of dense_H; shared: masses and inertias are one copy for all sets, so
    their gradients are the sums over the sets.  Yardstick: fp32 torch autograd of dense_H.  Per tensor."""
    from diffphys_amd import dp_utils, sim

    C = accel_case(name, S)
    tpl, nb, nqd = C["tpl"], C["nb"], C["nqd"]
    env = sim.Model.from_template(tpl, S, dev)
    g = g_out_of(C)
    assert np.abs(g - g.transpose(0, 2, 1)).max() > 1
    m32, I32 = body_weights(tpl, 1 if shared else S, F32)
    if shared:
        m32, I32 = m32[0], I32[0]
    t = [torch.from_numpy(np.array(x)).to(dev).requires_grad_(True) for x in (C["bq"], m32.numpy(), I32.numpy())]
    out = dp_utils.mass_matrix(t[0], t[1], t[2], env, method="crba", rates=rates)
    assert out.shape == (S, nqd, nqd)
    (out * torch.from_numpy(g).to(dev)).sum().backward()
    assert t[0].grad.shape == (S, nb, 7) and t[1].grad.shape == m32.shape and t[2].grad.shape == I32.shape
    c64, c32 = matrix_of(C, F64, rates, g, shared), matrix_of(C, F32, rates, g, shared)
    mine = dict(out=out.detach().cpu().numpy(), g_body_q=t[0].grad.cpu().numpy(), g_mass=t[1].grad.cpu().numpy(),
                g_inertia=t[2].grad.cpu().numpy())
    missed = []
    for what in ("out", "g_body_q", "g_mass", "g_inertia"):
        try:   # every figure is printed before the first miss ends the test
            bar("%s x %d %s%s %s" % (name, S, rates, " shared" if shared else "", what), mine[what], c32[what], c64[what])
        except AssertionError as e:
            missed.append(str(e))
    assert not missed, "; ".join(missed)
    gi = mine["g_inertia"]
    assert np.array_equal(gi, np.swapaxes(gi, -1, -2)) or shared   # per set: the gradient of sym(I), the same bits on both sides


# ------------------------------------------------------------------------------------------------------------ 4. bits
@pytest.mark.parametrize("rates", RATES)
def test_a_sets_bits_depend_on_nothing_but_the_set(rates, dev):
    """Forward and VJP: everything a second time, and sets 0 and 40 of the 41-set launch evaluated alone: equal bits (no atomics, fixed
    gather orders)."""
    from diffphys_amd import hip_backend

    name = "laikago"
    C = accel_case(name, 41)
    nb, nqd = C["nb"], C["nqd"]
    table = gpu_table(name, rates)
    rows, g = torch.from_numpy(rows17(C)).to(dev), torch.from_numpy(g_out_of(C)).to(dev)
    out, gb = hip_backend.mass_matrix(table, nb, rows), hip_backend.mass_matrix_vjp(table, nb, rows, g)
    assert torch.equal(out, hip_backend.mass_matrix(table, nb, rows)) and torch.equal(gb, hip_backend.mass_matrix_vjp(table, nb, rows, g))
    for s in (0, 40):
        alone = rows[s * nb: (s + 1) * nb].contiguous()
        assert torch.equal(hip_backend.mass_matrix(table, nb, alone)[0], out[s]), s
        assert torch.equal(hip_backend.mass_matrix_vjp(table, nb, alone, g[s: s + 1].contiguous()), gb[s * nb: (s + 1) * nb]), s
    assert hip_backend.mass_matrix(table, nb, torch.zeros(0, 17, device=dev)).shape == (0, nqd, nqd)
    assert hip_backend.mass_matrix_vjp(table, nb, torch.zeros(0, 17, device=dev), torch.zeros(0, nqd, nqd, device=dev)).shape == (0, 17)


@pytest.mark.parametrize("name,S", [("human", 3), ("mixed25", 3)])
def test_vjp_bits_on_a_second_launch(name, S, dev):
    """The gathers over descendants and children run in body order and the table's child order: the same bits again."""
    from diffphys_amd import hip_backend

    C = accel_case(name, S)
    table = gpu_table(name, "measured")
    rows, g = torch.from_numpy(rows17(C)).to(dev), torch.from_numpy(g_out_of(C)).to(dev)
    assert torch.equal(hip_backend.mass_matrix_vjp(table, C["nb"], rows, g), hip_backend.mass_matrix_vjp(table, C["nb"], rows, g))


# ------------------------------------------------------------------------------------------------------------ 5. entry points
def test_forward_dynamics_crba_against_dense(dev):
    """forward_dynamics(method="crba") and method="dense" on Laikago x 5 against the float64 chain solve(dense_H, tau - bias); the fp32
    torch chain is the yardstick; "dense" keeps the bits of the call without the keyword."""
    from diffphys_amd import dp_utils, sim

    name, S = "laikago", 5
    C = accel_case(name, S)
    tpl, nqd = C["tpl"], C["nqd"]
    env = sim.Model.from_template(tpl, S, dev)
    rng = np.random.RandomState(61)
    qd, tau = (rng.randn(S, nqd).astype(np.float32) for _ in range(2))
    bq, jqd, jtau = (torch.from_numpy(np.array(x)).to(dev) for x in (C["bq"], qd, tau))
    m32, I32 = body_weights(tpl, 1, F32)
    m, I = m32[0].to(dev), I32[0].to(dev)
    fd = dp_utils.forward_dynamics(bq, jqd, jtau, m, I, env, method="crba")
    plain = dp_utils.forward_dynamics(bq, jqd, jtau, m, I, env)
    assert fd.shape == (S, nqd) and torch.equal(plain, dp_utils.forward_dynamics(bq, jqd, jtau, m, I, env, method="dense"))

    def chain(dtype):
        T = oracle_template(tpl, dtype)
        q, v, f = (torch.tensor(np.array(x), dtype=dtype) for x in (C["bq"], qd, tau))
        H = torch.as_tensor(dense(name, S, None, "generalized", dtype))
        return torch.linalg.solve(H, (f - rnea(T, tpl, q, v, None))[..., None])[..., 0].numpy()

    c64, c32 = chain(F64), chain(F32)
    bar("laikago forward_dynamics(crba)", fd.cpu().numpy(), c32, c64)
    bar("laikago forward_dynamics(dense)", plain.cpu().numpy(), c32, c64)
    tq = jtau.clone().requires_grad_(True)   # ... and the chain back-propagates
    bqg = bq.clone().requires_grad_(True)
    dp_utils.forward_dynamics(bqg, jqd, tq, m, I, env, method="crba").sum().backward()
    assert torch.isfinite(tq.grad).all() and torch.isfinite(bqg.grad).all() and float(bqg.grad.abs().max()) > 0


QUERY_KEYS = {"sim_traj", "target_traj", "control_ref", "vertex_body", "sim_poses", "target_poses", "control_ref_poses", "com", "com_k",
              "body_mass", "grf", "jaf", "max_w"}   # what query() returns without a flag


def test_query_returns_the_simulated_mass_matrix(dev):
    import importlib.util
    import os

    from diffphys_amd import dp_utils
    from diffphys_amd.dataloader import DataLoader
    from diffphys_amd.phys_model import phys_model
    from helpers import ROOT

    spec = importlib.util.spec_from_file_location("pd_main_mm", os.path.join(ROOT, "ppr-diffphys_amd", "main.py"))
    pd_main = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pd_main)
    opts = pd_main.get_opts(["--seqname", "mi-pace", "--urdf_template", "laikago", "--logroot", "/tmp/pprdp_test_log/", "--logname", "mm",
                             "--num_envs", "8", "--frames_per_wdw", "4"])
    torch.manual_seed(0)
    np.random.seed(0)
    model = phys_model(opts, DataLoader(opts)).cuda()
    model.train()
    model.reinit_envs(opts["num_envs"], frames_per_wdw=opts["frames_per_wdw"])
    model.set_progress(0)
    with torch.no_grad():
        model.body_mass.mul_(torch.linspace(0.8, 1.25, model.body_mass.numel(), device=model.body_mass.device))   # "learned" masses
    model.forward(frame_start=torch.arange(8, device=model.device) * 3)
    plain = model.query()
    assert set(plain) == QUERY_KEYS
    q = model.query(mass_matrix=True)
    assert set(q) == QUERY_KEYS | {"sim_mass_matrix"}
    for k in QUERY_KEYS - {"com_k", "max_w"}:
        assert np.array_equal(np.asarray(plain[k]), np.asarray(q[k])), k
    nqd = int(model.template["nqd"])
    H = q["sim_mass_matrix"]
    assert isinstance(H, np.ndarray) and H.shape == (4, nqd, nqd) and np.array_equal(H, H.transpose(0, 2, 1))
    up = lambda frames: torch.from_numpy(np.ascontiguousarray(np.stack(list(frames), 0), dtype=np.float32)).to(dev)
    mass = model.body_mass.detach().float()
    direct = dp_utils.mass_matrix(up(model.sim_trajs), mass, model.norm_body_inertia.detach().float() * mass[:, None, None], model.env,
                                  method="crba")
    assert np.array_equal(H, direct.cpu().numpy())
    assert (np.diagonal(H, axis1=1, axis2=2) > 0).all()
