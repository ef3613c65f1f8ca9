"""The rigid-body twists of joint rates (``pd_pose_op`` PD_POSE_BODY_TWIST, k_body_twist_fwd / _vjp of csrc/pd_pose.hip,
dp_model.BodyTwists, dp_utils.body_twists / jacobian / mass_matrix / rigid_twists, phys_model's rigid_twists option) on a real MI355X
(run with -m gpu).

Reference: tests/body_twists_ref.py, the float64 torch restatement (held to its identities by tests/test_body_twists_host.py), given the
SAME fp32 rows as the GPU.  Bar (the project's, as tests/test_gpu_generalized_force.py): the GPU's error over max |reference| per tensor
<= max(4 x the error of the fp32 torch evaluation of the same restatement, 1e-5); where two fp32 ops are chained, twice that, with the
fp32 torch chain as the yardstick.  Both numbers are printed.

Measured on one MI355X (error over max |reference|; GPU / fp32 torch): see DESIGN.md section 8."""
import functools

import numpy as np
import pytest
import torch

from body_twists_ref import CASES, EFFORTS_OF, RATES, TENSORS, body_twists, case, g_out_of, rows13, slot_index, slots_of, twists_of
from generalized_force_ref import generalized_force
from gpu_harness import dev  # noqa: F401
from helpers import relmax
from joint_coords_ref import fk_states, joint_coords, oracle_template, random_coords
from joint_wrench_ref import template

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32


def bar(what, gpu, f32, ref, floor=1e-5, factor=1.0):
    e_gpu, e_32 = relmax(gpu, ref), relmax(f32, ref)
    print("%s: GPU %.2e, fp32 torch %.2e" % (what, e_gpu, e_32))
    assert np.isfinite(np.asarray(gpu)).all(), what
    assert np.isfinite(e_gpu) and e_gpu <= factor * max(4 * e_32, floor), "%s: GPU error %.2e vs fp32 torch %.2e" % (what, e_gpu, e_32)


@functools.lru_cache(maxsize=None)
def restated(name, S, shift, rates, dtype):
    """value and gradients of the restatement on a case, with the standard-normal g_out every test uses: computed once, never written"""
    C = case(name, S, shift)
    return twists_of(C, dtype, rates, g_out_of(C))


@functools.lru_cache(maxsize=None)
def gpu_table(name, rates):
    from diffphys_amd import hip_backend

    return hip_backend.joint_table(template(name), rates, torch.device("cuda:0"))


def launch(C, name, rates, dev, g_out=None, rows=None):
    """-> (out [S, nb, 6], g_rows [S, nb, 13] or None) as numpy"""
    from diffphys_amd import hip_backend

    nb = C["nb"]
    r = torch.from_numpy(rows13(C) if rows is None else rows).to(dev)
    S = r.shape[0] // nb
    out = hip_backend.body_twists(gpu_table(name, rates), nb, r)
    assert out.shape == (S * nb, 6)
    g = None
    if g_out is not None:
        go = torch.from_numpy(np.ascontiguousarray(g_out, np.float32).reshape(-1, 6)).to(dev)
        g = hip_backend.body_twists_vjp(gpu_table(name, rates), nb, r, go)
        assert g.shape == (S * nb, 13)
        g = g.cpu().numpy().reshape(S, nb, 13)
    return out.cpu().numpy().reshape(S, nb, 6), g


# ------------------------------------------------------------------------------------------------------------ 1. values and VJP
@pytest.mark.parametrize("rates", RATES)
@pytest.mark.parametrize("name,S,shift", CASES)
def test_op_and_vjp_match_the_float64_restatement(name, S, shift, rates, dev):
    """Value and g_rows of a standard-normal g_out against the float64 restatement and its autograd on the same fp32 rows.  mixed25 (a
    body with 8 children), rev64 (depth 64), rev256 (the cap) and the far-shifted Laikago catch a wrong sweep, cap or reference point."""
    C = case(name, S, shift)
    g_out = g_out_of(C)
    out, g = launch(C, name, rates, dev, g_out)
    r64, r32 = restated(name, S, shift, rates, F64), restated(name, S, shift, rates, F32)
    tag = "%s x %d%s %s " % (name, S, " far" if shift else "", rates)
    mine = dict(out=out, g_body_q=g[..., :7], g_rates=g[..., 7:])
    for k in TENSORS:
        if np.abs(r64[k]).max() == 0:   # free1, g_body_q: one FREE body with its com at its origin -- no pose enters, the gradient is 0
            assert name == "free1" and k == "g_body_q" and np.abs(mine[k]).max() <= 1e-6   # (terms of size 1 that cancel: a few fp32 ulps)
            continue
        bar(tag + k, mine[k], r32[k], r64[k])
    unused = slot_index(C["tpl"]) == C["nqd"]   # a slot no dof uses: ignored by the value (the rows fill it), zero in the gradient
    assert (mine["g_rates"][:, unused] == 0).all()
    if name == "mixed25":   # the body that gathers 8 children is in the comparison
        assert (np.asarray(C["tpl"]["joint_parent"]).reshape(-1) == 0).sum() == 8


# ------------------------------------------------------------------------------------------------------------ 2. a set's bits
@pytest.mark.parametrize("rates", RATES)
def test_a_sets_bits_depend_on_nothing_but_the_set(rates, dev):
    """Sets 0 and 40 of the 41-set launch evaluated alone, and everything a second time: equal bits, value and VJP."""
    name = "laikago"
    C = case(name, 41)
    nb = C["nb"]
    g_out = g_out_of(C)
    out, g = launch(C, name, rates, dev, g_out)
    again = launch(C, name, rates, dev, g_out)
    assert np.array_equal(out, again[0]) and np.array_equal(g, again[1])
    for s in (0, 40):
        alone = launch(C, name, rates, dev, g_out[s: s + 1], rows=rows13(C)[s * nb: (s + 1) * nb])
        assert np.array_equal(alone[0][0], out[s]) and np.array_equal(alone[1][0], g[s]), s


# ------------------------------------------------------------------------------------------------------------ 3. edges
def test_a_table_of_another_nb_gives_zeros(dev):
    """The library cannot validate a device buffer: the kernels check the table's nb against the call's and write zeros (no row of
    the table is read)."""
    from diffphys_amd import hip_backend

    C = case("cmp31", 3)
    wrong = gpu_table("mixed25", "measured").clone()   # 4 + 32 * 25 floats: shorter than the table of 31 bodies
    _, (nb25, nq25, nqd25) = hip_backend._table_tag(gpu_table("mixed25", "measured"))
    assert nb25 == 25
    wrong._pd_table = ("joint", (31, nq25, nqd25))   # ... passed off as one
    rows = torch.from_numpy(rows13(C)).to(dev)
    out = hip_backend.body_twists(wrong, 31, rows)
    g = hip_backend.body_twists_vjp(wrong, 31, rows, torch.ones(93, 6, device=dev))
    assert out.shape == (93, 6) and g.shape == (93, 13)
    assert (out == 0).all() and (g == 0).all()


def test_empty_and_graph_capture(dev):
    """n = 0; forward and VJP captured in a HIP graph replay eager's bits on new inputs."""
    from diffphys_amd import hip_backend

    name = "human"
    C = case(name, 3)
    nb = C["nb"]
    table = gpu_table(name, "measured")
    empty = torch.zeros(0, 13, device=dev)
    assert hip_backend.body_twists(table, nb, empty).shape == (0, 6)
    assert hip_backend.body_twists_vjp(table, nb, empty, torch.zeros(0, 6, device=dev)).shape == (0, 13)
    rows = torch.from_numpy(rows13(C)).to(dev)
    g_out = torch.from_numpy(g_out_of(C).reshape(-1, 6)).to(dev)
    run = lambda r, g: (hip_backend.body_twists(table, nb, r), hip_backend.body_twists_vjp(table, nb, r, g))
    rbuf, gbuf = rows.clone(), g_out.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(rbuf, gbuf)   # warm-up on the capture stream
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            cap = run(rbuf, gbuf)
    torch.cuda.current_stream().wait_stream(side)
    fresh = rows * 1.01
    g2 = torch.randn(g_out.shape, generator=torch.Generator().manual_seed(7)).to(dev)
    rbuf.copy_(fresh); gbuf.copy_(g2)
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip(cap, run(fresh, g2)):
        assert torch.equal(got, want)


# ------------------------------------------------------------------------------------------------------------ 4. autograd, op 15
def _qd_of(C, seed=61):
    return np.random.RandomState(seed).randn(C["bq"].shape[0], C["nqd"]).astype(np.float32)


@pytest.mark.parametrize("rates", RATES)
@pytest.mark.parametrize("name,S", [("laikago", 41), ("human", 3)])
def test_autograd_is_the_generalized_force_and_power_balances(name, S, rates, dev):
    """Through dp_utils.body_twists: the gradient in joint_qd of <g, twists> is dp_utils.generalized_force(body_q, g, env, the matching
    efforts) -- the op is the GPU's op 15 transposed --, and sum tau . qd = sum wrench . twist with the GPU's op 15.  Twice the bar
    (two fp32 ops chained); yardstick: the fp32 torch restatements."""
    from diffphys_amd import dp_utils, sim

    C = case(name, S)
    tpl, nb, nqd = C["tpl"], C["nb"], C["nqd"]
    env = sim.Model.from_template(tpl, S, dev)
    efforts = EFFORTS_OF[rates]
    g, qd = g_out_of(C), _qd_of(C)
    bq = torch.from_numpy(C["bq"].copy()).to(dev)
    jqd = torch.from_numpy(qd).to(dev).requires_grad_(True)
    gd = torch.from_numpy(g).to(dev)
    tw = dp_utils.body_twists(bq, jqd, env, rates=rates)
    assert tw.shape == (S, nb, 6)
    (tw * gd).sum().backward()
    tau = dp_utils.generalized_force(bq, gd, env, efforts=efforts)
    assert jqd.grad.shape == (S, nqd)

    def chain(dtype):
        T = oracle_template(tpl, dtype)
        q, w = torch.tensor(np.array(C["bq"]), dtype=dtype), torch.tensor(g, dtype=dtype)
        return (generalized_force(T, q, w, efforts).numpy(),
                body_twists(T, q, slots_of(tpl, torch.tensor(qd, dtype=dtype)), rates).numpy())

    (tau64, tw64), (tau32, tw32) = chain(F64), chain(F32)
    tag = "%s x %d %s " % (name, S, rates)
    bar(tag + "d <g, twists> / d joint_qd against generalized_force", jqd.grad.cpu().numpy(), tau32, tau64, factor=2.0)
    e_pair = np.abs(jqd.grad.cpu().numpy() - tau.cpu().numpy()).max() / np.abs(tau64).max()
    e_32 = relmax(tau32, tau64)
    print(tag + "gradient against the GPU's op 15: %.2e of max (fp32 torch %.2e)" % (e_pair, e_32))
    assert e_pair <= 2 * max(4 * e_32, 1e-5)
    # power: per set, relative to the size of the products summed
    scale = np.abs(g.astype(np.float64) * tw64).sum((1, 2))
    power = lambda t, w: np.abs((np.asarray(t, np.float64) * qd).sum(-1) - (g.astype(np.float64) * np.asarray(w, np.float64)).sum((1, 2))) / scale
    p_gpu, p_32 = power(tau.cpu().numpy(), tw.detach().cpu().numpy()).max(), power(tau32, tw32).max()
    print(tag + "power identity with the GPU's op 15: GPU %.2e, fp32 torch %.2e" % (p_gpu, p_32))
    assert p_gpu <= 2 * max(4 * p_32, 1e-5)


# ------------------------------------------------------------------------------------------------------------ 5. Jacobian, mass matrix
def _kinetic(T, bq, tw, mass, inertia):
    """sum_b m |v|^2 / 2 + wb . I wb / 2 with wb = R(q)^T w, per set"""
    from oracle import ref_torch as rt

    S = bq.shape[0]
    wb = rt.q_rot_inv(bq[..., 3:].reshape(-1, 4), tw[..., :3].reshape(-1, 3)).reshape(S, T.nb, 3)
    Iw = (inertia @ wb[..., None])[..., 0]
    return 0.5 * (mass * (tw[..., 3:] ** 2).sum(-1)).sum(-1) + 0.5 * (wb * Iw).sum((1, 2))


@pytest.mark.parametrize("name", ["laikago", "human"])
def test_jacobian_and_mass_matrix(name, dev):
    """jacobian @ qd is body_twists; qd^T mass_matrix qd / 2 is centroidal(body_q, body_twists(...)).kinetic and the float64 kinetic
    energy of the restatement's twists.  Yardstick: the fp32 torch chain, at 4 x."""
    from diffphys_amd import dp_utils, sim

    S = 3
    C = case(name, S)
    tpl, nb, nqd = C["tpl"], C["nb"], C["nqd"]
    env = sim.Model.from_template(tpl, S, dev)
    qd = _qd_of(C)
    bq, jqd = torch.from_numpy(C["bq"].copy()).to(dev), torch.from_numpy(qd).to(dev)
    m = torch.from_numpy(np.asarray(tpl["body_mass"], np.float32).reshape(nb)).to(dev)
    I = torch.from_numpy(np.asarray(tpl["body_inertia"], np.float32).reshape(nb, 3, 3)).to(dev)
    J = dp_utils.jacobian(bq, env)
    assert J.shape == (S, nb, 6, nqd)
    tw = dp_utils.body_twists(bq, jqd, env)
    H = dp_utils.mass_matrix(bq, m, I, env)
    assert H.shape == (S, nqd, nqd)
    e_h = 0.5 * torch.einsum("si,sij,sj->s", jqd, H, jqd).cpu().numpy()
    e_c = dp_utils.centroidal(bq, tw, m, I, env).kinetic.cpu().numpy()

    def chain(dtype):
        T = oracle_template(tpl, dtype)
        q = torch.tensor(np.array(C["bq"]), dtype=dtype)
        t = body_twists(T, q, slots_of(tpl, torch.tensor(qd, dtype=dtype)), "generalized")
        mm = torch.tensor(np.asarray(tpl["body_mass"], np.float32).reshape(nb), dtype=dtype)
        II = torch.tensor(np.asarray(tpl["body_inertia"], np.float32).reshape(nb, 3, 3), dtype=dtype)
        return t.numpy(), _kinetic(T, q, t, mm, II).numpy()

    (tw64, e64), (tw32, e32) = chain(F64), chain(F32)
    bar(name + " jacobian @ qd", (J @ jqd[:, None, :, None])[..., 0].cpu().numpy(), tw32, tw64)
    bar(name + " qd^T H qd / 2", e_h, e32, e64)
    bar(name + " centroidal kinetic of the twists", e_c, e32, e64)
    assert relmax(H.cpu().numpy(), H.transpose(-1, -2).cpu().numpy()) <= 1e-5   # symmetric to rounding
    bqg = bq.clone().requires_grad_(True)   # differentiable in the poses
    dp_utils.mass_matrix(bqg, m, I, env).sum().backward()
    assert bqg.grad is not None and torch.isfinite(bqg.grad).all() and float(bqg.grad.abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------ 6. rigid_twists
@pytest.mark.parametrize("name", ["laikago", "human"])
def test_rigid_twists(name, dev):
    """rigid_twists(body_q, body_twists(...)) returns its input, at twice the bar (joint_coords and body_twists chained; yardstick: the
    fp32 torch chain).  On FK states every angular part and the root's row are kept, and the other linear parts are not."""
    from diffphys_amd import dp_utils, sim

    S = 3
    tpl = template(name)
    nb, nqd = int(tpl["nb"]), int(tpl["nqd"])
    env = sim.Model.from_template(tpl, S, dev)
    q, qd = random_coords(tpl, S, seed=71, lo=0.05, hi=1.0)
    bq32, bqd32 = fk_states(tpl, q, qd)   # exact FK states, rounded to fp32
    bq = torch.from_numpy(bq32).to(dev)

    def chain(dtype, twists):
        """joint_coords then body_twists in torch, the FREE linear entries as rigid_twists takes them"""
        from oracle import ref_torch as rt

        T = oracle_template(tpl, dtype)
        b, t = torch.tensor(bq32, dtype=dtype), torch.tensor(np.asarray(twists), dtype=dtype)
        _, jqd = joint_coords(T, b, t, "generalized")
        jqd = jqd.clone()
        for i in range(T.nb):
            if T.joint_type[i] == rt.JOINT_FREE:
                assert T.joint_parent[i] < 0
                s = T.qd_start[i]
                jqd[:, s + 3: s + 6] = rt.q_rot_inv(T.X_p[i, 3:].expand(S, 4), t[:, i, 3:])
        return body_twists(T, b, slots_of(tpl, jqd), "generalized").numpy()

    # (a) a rigid state comes back
    jqd = torch.from_numpy(np.random.RandomState(73).randn(S, nqd).astype(np.float32)).to(dev)
    tw = dp_utils.body_twists(bq, jqd, env)
    back = dp_utils.rigid_twists(bq, tw, env).cpu().numpy()
    twn = tw.cpu().numpy()
    bar(name + " rigid_twists of rigid twists", back, chain(F32, twn), twn.astype(np.float64), factor=2.0)
    # (b) FK states: angular parts and the root's row kept, the other linear parts replaced
    fk = dp_utils.rigid_twists(bq, torch.from_numpy(bqd32).to(dev), env).cpu().numpy()
    fk32, fk64 = chain(F32, bqd32), chain(F64, bqd32)
    bar(name + " rigid_twists of FK states", fk, fk32, fk64, factor=2.0)
    scale = np.abs(bqd32).max()
    e_w, e_root = np.abs(fk[..., :3] - bqd32[..., :3]).max() / scale, np.abs(fk[:, 0] - bqd32[:, 0]).max() / scale
    y_w, y_root = np.abs(fk32[..., :3] - bqd32[..., :3]).max() / scale, np.abs(fk32[:, 0] - bqd32[:, 0]).max() / scale
    print("%s FK states: angular parts kept to %.2e (fp32 torch %.2e), the root's row to %.2e (%.2e); other linear parts moved by %.3g m/s" % (
        name, e_w, y_w, e_root, y_root, np.abs(fk[:, 1:, 3:] - bqd32[:, 1:, 3:]).max()))
    assert int(np.asarray(tpl["joint_type"]).reshape(-1)[0]) == 4   # body 0 is the FREE root
    assert e_w <= 2 * max(4 * y_w, 1e-5) and e_root <= 2 * max(4 * y_root, 1e-5)
    assert np.abs(fk[:, 1:, 3:] - bqd32[:, 1:, 3:]).max() > 0.1


# ------------------------------------------------------------------------------------------------------------ 7. phys_model
def test_phys_model_rigid_twists_option(dev):
    """The smallest window of the contact-state model test, reg_skate_wt > 0: with rigid_twists on the losses are finite and reg_skate
    differs from the run with it off; with the option absent, loss_dict equals the rigid_twists=False run bit for bit."""
    from test_gpu_workload import _model

    model, opts = _model("mi-pace", "bt")
    model.reinit_envs(4, frames_per_wdw=3)
    fs = torch.arange(4, device=dev)
    noise = (torch.randn(4 * 19, generator=torch.Generator().manual_seed(3)) * 0.01).to(dev)
    opts["reg_skate_wt"] = 0.5

    def run():
        out = model.forward(frame_start=fs, q_init_noise=noise.clone())
        torch.cuda.synchronize()
        return {k: v.detach().clone() for k, v in out.items()}

    assert "rigid_twists" in opts and not opts["rigid_twists"]   # the command line's default: off
    off = run()
    del opts["rigid_twists"]
    absent = run()
    assert set(absent) == set(off) and all(torch.equal(absent[k], off[k]) for k in off)
    opts["rigid_twists"] = True
    on = run()
    assert set(on) == set(off) and all(bool(torch.isfinite(v).all()) for v in on.values())
    print("loss_reg_skate: FK velocities %.4e, rigid twists %.4e" % (float(off["loss_reg_skate"]), float(on["loss_reg_skate"])))
    assert float(on["loss_reg_skate"]) > 0 and not torch.equal(on["loss_reg_skate"], off["loss_reg_skate"])
    for k in off:   # nothing else sees the option
        if k not in ("loss_reg_skate", "total_loss"):
            assert torch.equal(on[k], off[k]), k
    model.optimizer.zero_grad(set_to_none=True)   # ... and it back-propagates
    out = model.forward(frame_start=fs, q_init_noise=noise.clone())
    model.backward(out["total_loss"])
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)
