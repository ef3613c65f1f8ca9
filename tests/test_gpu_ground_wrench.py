"""The ground-contact wrench as a differentiable op (``pd_pose_op`` PD_POSE_GROUND_WRENCH), the material gradients built on it
(dp_model.ForwardWarpContact) and the differentiable grf (run on a real MI355X with -m gpu).

Model: the shipped Laikago (3 838 mesh candidates: several iterations per wave) and human (8 per body: partial waves) templates with TWO
materials (even / odd bodies), helpers.tight_inputs(seed=5), bs = 3, T = 6, env 0 lowered by 6 cm so that contact forces sit on the
+-500 N clamp.  The op runs on the states a GPU rollout saved: T * bs * nb elements.

Bars (those of tests/test_gpu_tight.py): the GPU's error against the float64 torch oracle (oracle/ref_torch.py eval_body_contacts and its
autograd) <= max(4 x the error of the same torch evaluation in float32, 1e-5), and at most that file's caps -- wrench 3e-4, gradient 6e-4
(Laikago) / 1e-4 (human).  Every test first asserts, in float64, that no candidate of its states is within 1e-6 m of the ground, where
an fp32 height may fall on the other side; no element is ever excluded."""
import functools

import numpy as np
import pytest
import torch

from ground_wrench_common import (MATERIALS, MATERIALS_B, candidate_probe, model_inputs, oracle_rollout_grads, two_material_template,
                                  wrench_and_state_grads)
from helpers import INPUT_NAMES, chain2, build_template, relmax
from gpu_harness import BWD, FWD, dev, dev_inputs  # noqa: F401
from test_gpu_tight import CAPS

pytestmark = pytest.mark.gpu

BS, T = 3, 6
FRAMES = [0, 3, 5, 6]


def check(what, a, c32, ref, cap, floor=1e-5):
    e_gpu, e_c = relmax(a, ref), relmax(c32, ref)
    print("%s: GPU %.2e, fp32 torch %.2e, cap %.1e" % (what, e_gpu, e_c, cap))
    assert np.isfinite(e_gpu) and e_gpu <= cap, "%s: GPU error %.2e above the cap %.1e (fp32 torch oracle: %.2e)" % (what, e_gpu, cap, e_c)
    assert e_gpu <= max(4 * e_c, floor), "%s: GPU error %.2e vs fp32 torch oracle %.2e" % (what, e_gpu, e_c)


def assert_off_the_ground(tpl, q, qd):
    c, fmax = candidate_probe(tpl, q, qd)
    assert np.abs(c).min() >= 1e-6, "a candidate %.2e m from the ground: pick another seed" % np.abs(c).min()
    return c, fmax


@functools.lru_cache(maxsize=None)
def case(name):
    """One GPU rollout (forward + adjoint with random seeds) of the common model; everything the tests below share, computed once."""
    from diffphys_amd import hip_backend, sim

    dev = torch.device("cuda:0")
    tpl = two_material_template(name)
    inp = model_inputs(tpl, name, BS, T, seed=5, lowered_env=0)
    env = sim.Model.from_template(tpl, BS, dev)
    dm = hip_backend.device_model(env)
    nb = dm.nb
    rng = np.random.RandomState(7)
    t = dev_inputs(inp, dev)
    adj_pos = torch.from_numpy(rng.randn(len(FRAMES), BS * nb, 7).astype(np.float32)).to(dev)
    adj_vel = torch.from_numpy(rng.randn(len(FRAMES), BS * nb, 6).astype(np.float32)).to(dev)
    pos, vel, grf, jaf, ws = dm.rollout_forward(BS, T, inp["dt"], *[t[k] for k in FWD], frame2step=FRAMES)
    g = dm.rollout_backward(BS, T, inp["dt"], *[t[k] for k in BWD], FRAMES, ws, adj_pos, adj_vel)
    bq, bqd, _, _ = dm.saved_trajectory(ws, BS, T)
    state = torch.cat([bq, bqd], -1).reshape(-1, 13).contiguous()   # [T * bs * nb, 13]
    table = hip_backend.env_contact_table(env, dev)
    q64 = bq.reshape(T * BS, nb, 7).cpu().numpy().astype(np.float64)
    qd64 = bqd.reshape(T * BS, nb, 6).cpu().numpy().astype(np.float64)
    return dict(tpl=tpl, inp=inp, env=env, dm=dm, nb=nb, t=t, pos=pos, vel=vel, grf=grf, ws=ws, g=g, state=state, table=table, q=q64, qd=qd64)


ROBOTS = ["laikago", "human"]


@pytest.mark.parametrize("name", ROBOTS)
def test_forward_matches_the_float64_contacts(name, dev, oracle_libs):
    from diffphys_amd import hip_backend

    C = case(name)
    c, fmax = assert_off_the_ground(C["tpl"], C["q"], C["qd"])
    assert np.nansum(fmax >= 500.0) >= 1, "no contact force on the +-500 N clamp"
    out = hip_backend.ground_wrench(C["table"], C["nb"], C["state"]).cpu().numpy().reshape(T * BS, C["nb"], 6)
    w64 = wrench_and_state_grads(C["tpl"], torch.float64, C["q"], C["qd"])
    w32 = wrench_and_state_grads(C["tpl"], torch.float32, C["q"], C["qd"])
    check("wrench", out, w32, w64, CAPS[name][2])
    idle = np.abs(w64).max(-1) == 0   # bodies that touch nothing (or have no candidates): exact zeros
    assert idle.any() and (~idle).any()
    assert (out[idle] == 0).all()
    assert (np.abs(out[~idle]).max(-1) > 0).all()


@pytest.mark.parametrize("name", ROBOTS)
def test_res_f_plus_op_is_the_rollouts_grf(name, dev):
    """res_f[step] + op(frame state) against the grf the rollout launch itself wrote: the candidate terms are the same bits, only the
    order of at most 31 fp32 additions differs (31 * 2^-24 = 2e-6 < 1e-5)."""
    from diffphys_amd import hip_backend

    C = case(name)
    frames = [f for f, s in enumerate(FRAMES) if s < T]
    assert len(frames) == 3
    for f in frames:
        st = torch.cat([C["pos"][f], C["vel"][f]], -1).contiguous()
        got = C["t"]["res_f"][FRAMES[f]] + hip_backend.ground_wrench(C["table"], C["nb"], st)
        e = relmax(got.cpu().numpy(), C["grf"][f].cpu().numpy())
        print("frame %d: relmax %.2e" % (f, e))
        assert e <= 1e-5, (f, e)
    assert C["grf"][frames].abs().max().item() > 10.0


@pytest.mark.parametrize("name", ROBOTS)
def test_state_vjp_matches_oracle_autograd(name, dev, oracle_libs):
    from diffphys_amd import hip_backend

    C = case(name)
    assert_off_the_ground(C["tpl"], C["q"], C["qd"])
    g_out = np.random.RandomState(3).randn(T * BS, C["nb"], 6).astype(np.float32)
    g_s, g_m = hip_backend.ground_wrench_vjp(C["table"], C["nb"], 2, C["state"], torch.from_numpy(g_out).to(dev).reshape(-1, 6))
    _, q64, qd64, m64 = wrench_and_state_grads(C["tpl"], torch.float64, C["q"], C["qd"], g_out)
    _, q32, qd32, m32 = wrench_and_state_grads(C["tpl"], torch.float32, C["q"], C["qd"], g_out)
    cap = CAPS[name][3]
    g_s = g_s.cpu().numpy().reshape(T * BS, C["nb"], 13)
    check("g_body_q", g_s[..., :7], q32, q64, cap)
    check("g_body_qd", g_s[..., 7:], qd32, qd64, cap)
    check("g_materials", hip_backend.colsum(g_m.view(-1, 8)).cpu().numpy().reshape(2, 4), m32, m64, cap)
    assert g_m.shape == (T * BS * C["nb"], 2, 4)
    # the same states with materials MIXED inside every body (candidate k takes row k % 2): the masked sweep per material row
    mixed = dict(C["tpl"], contact_material=(np.arange(len(C["tpl"]["contact_body"])) % 2).astype(np.int32))
    assert_off_the_ground(mixed, C["q"], C["qd"])
    table = hip_backend.contact_table(mixed, device=dev)
    g_s, g_m = hip_backend.ground_wrench_vjp(table, C["nb"], 2, C["state"], torch.from_numpy(g_out).to(dev).reshape(-1, 6))
    _, q64, qd64, m64 = wrench_and_state_grads(mixed, torch.float64, C["q"], C["qd"], g_out)
    _, q32, qd32, m32 = wrench_and_state_grads(mixed, torch.float32, C["q"], C["qd"], g_out)
    check("mixed g_state", g_s.cpu().numpy().reshape(T * BS, C["nb"], 13), np.concatenate([q32, qd32], -1), np.concatenate([q64, qd64], -1), cap)
    check("mixed g_materials", hip_backend.colsum(g_m.view(-1, 8)).cpu().numpy().reshape(2, 4), m32, m64, cap)


@pytest.mark.parametrize("name", ROBOTS)
def test_material_vjp_on_the_kernels_own_trajectory(name, dev, oracle_libs):
    """d loss / d materials = sum_t <g_res_f[t], dG(state_t, materials)/dmaterials>: the GPU's g_res_f and saved states through
    dp_model.material_gradient against the float64 contraction of the same two tensors."""
    from diffphys_amd import dp_model

    C = case(name)
    assert_off_the_ground(C["tpl"], C["q"], C["qd"])
    got = dp_model.material_gradient(C["dm"], C["table"], 2, C["ws"], BS, T, C["g"]["res_f"]).cpu().numpy()
    g_res_f = C["g"]["res_f"].cpu().numpy().reshape(T * BS, C["nb"], 6)
    ref = wrench_and_state_grads(C["tpl"], torch.float64, C["q"], C["qd"], g_res_f)[3]
    r32 = wrench_and_state_grads(C["tpl"], torch.float32, C["q"], C["qd"], g_res_f)[3]
    print(name, "reference material gradient", ref.tolist())
    assert (np.abs(ref).max(0) > 0).all(), "a column (ke, kd, kf, mu) without a gradient"
    if name == "human":
        assert (ref != 0).all()
    check("material gradient", got, r32, ref, CAPS[name][3])


class _Host:
    """the attributes the ForwardWarp family reads from ``self``"""

    def __init__(self, env, bs, nsteps, frame2step, dt):
        self.env, self.num_envs, self.steps_idx, self.frame2step, self.dt = env, bs, range(nsteps), list(frame2step), dt


def _e2e(name, dev, frame2step):
    from diffphys_amd import sim

    tpl = two_material_template(name)
    inp = model_inputs(tpl, name, 8, 3, seed=5)
    inp["frame2step"] = list(frame2step)
    env = sim.Model.from_template(tpl, 8, dev)
    rng = np.random.RandomState(11)
    F, N = len(frame2step), 8 * int(tpl["nb"])
    w = dict(pos=rng.randn(F, N, 7), vel=rng.randn(F, N, 6), grf=rng.randn(sum(s < 3 for s in frame2step), N, 6))
    t = dev_inputs(inp, dev)
    return tpl, inp, env, w, t


@pytest.mark.parametrize("name", ROBOTS)
def test_forward_warp_contact_material_gradient_end_to_end(name, dev, oracle_libs):
    from diffphys_amd import dp_model

    tpl, inp, env, w, t = _e2e(name, dev, [0, 3])
    M = torch.from_numpy(MATERIALS).to(dev).requires_grad_(True)
    t["refs"].requires_grad_(True)   # (res_f needs none: its adjoint is computed for the materials and dropped)
    h = _Host(env, 8, 3, inp["frame2step"], inp["dt"])
    pos, vel = dp_model.ForwardWarpContact.apply(*[t[k] for k in INPUT_NAMES], M, h)
    wp, wv = (torch.from_numpy(w[k].astype(np.float32)).to(dev) for k in ("pos", "vel"))
    ((pos * wp).sum() + (vel * wv).sum()).backward()
    assert t["res_f"].grad is None and t["refs"].grad is not None and len(h.grfs) == 1
    loss = lambda dt: (lambda p, v, g: (p * torch.as_tensor(w["pos"], dtype=dt)).sum() + (v * torch.as_tensor(w["vel"], dtype=dt)).sum())
    r64 = oracle_rollout_grads(tpl, torch.float64, inp, loss(torch.float64), ("materials", "refs"))
    r32 = oracle_rollout_grads(tpl, torch.float32, inp, loss(torch.float32), ("materials", "refs"))
    assert np.abs(r64["materials"]).max() > 0
    check("d loss / d materials", M.grad.cpu().numpy(), r32["materials"], r64["materials"], CAPS[name][3])
    check("d loss / d refs", t["refs"].grad.cpu().numpy(), r32["refs"], r64["refs"], CAPS[name][3])


@pytest.mark.parametrize("name", ROBOTS)
def test_loss_on_recomputed_grf_reaches_the_rollout_inputs(name, dev, oracle_libs):
    """grf[f] = res_f[frame2step[f]] + ground_wrench(wp_pos[f], wp_vel[f]) is differentiable through plain ForwardWarp."""
    from diffphys_amd import dp_model, dp_utils

    f2s = [0, 2, 3]
    tpl, inp, env, w, t = _e2e(name, dev, f2s)
    nb = int(tpl["nb"])
    wrt = ("q_init", "qd_init", "refs")
    for k in wrt:
        t[k].requires_grad_(True)
    h = _Host(env, 8, 3, f2s, inp["dt"])
    pos, vel = dp_model.ForwardWarp.apply(*[t[k] for k in INPUT_NAMES], h)
    rows = [f for f, s in enumerate(f2s) if s < 3]
    grf = t["res_f"][[f2s[f] for f in rows]] + dp_utils.ground_wrench(pos[rows].view(len(rows), 8, nb, 7), vel[rows].view(len(rows), 8, nb, 6),
                                                                       env).view(len(rows), 8 * nb, 6)
    assert relmax(grf.detach().cpu().numpy(), torch.stack(h.grfs).cpu().numpy()) <= 1e-5   # the launch's own side output
    (grf * torch.from_numpy(w["grf"].astype(np.float32)).to(dev)).sum().backward()
    loss = lambda dt: (lambda p, v, g: (g * torch.as_tensor(w["grf"], dtype=dt)).sum())
    r64 = oracle_rollout_grads(tpl, torch.float64, inp, loss(torch.float64), wrt, need_grf=True)
    r32 = oracle_rollout_grads(tpl, torch.float32, inp, loss(torch.float32), wrt, need_grf=True)
    for k in wrt:
        assert np.abs(r64[k]).max() > 0, k
        check("d grf loss / d " + k, t[k].grad.cpu().numpy(), r32[k], r64[k], CAPS[name][3])


def test_a_materials_update_rebuilds_the_device_model(dev):
    """After set_shape_materials(M') -- here through ForwardWarpContact with other rows -- outputs and ALL gradients are the bits of a
    fresh model whose template has M'."""
    from diffphys_amd import dp_model, hip_backend, sim

    tpl, inp, env, w, _ = _e2e("human", dev, [0, 3])
    wp, wv = (torch.from_numpy(w[k].astype(np.float32)).to(dev) for k in ("pos", "vel"))

    def run(env, rows):
        t = {k: v.requires_grad_(True) for k, v in dev_inputs(inp, dev).items()}
        M = torch.from_numpy(rows).to(dev).requires_grad_(True)
        h = _Host(env, 8, 3, inp["frame2step"], inp["dt"])
        pos, vel = dp_model.ForwardWarpContact.apply(*[t[k] for k in INPUT_NAMES], M, h)
        ((pos * wp).sum() + (vel * wv).sum()).backward()
        return [pos.detach(), vel.detach(), h.grfs[0], M.grad] + [t[k].grad for k in INPUT_NAMES]

    first = run(env, MATERIALS)
    dm0 = hip_backend.device_model(env)
    updated = run(env, MATERIALS_B)
    assert hip_backend.device_model(env) is not dm0 and np.array_equal(env.t_shape_materials, MATERIALS_B)
    fresh = run(sim.Model.from_template(two_material_template("human", MATERIALS_B), 8, dev), MATERIALS_B)
    assert not torch.equal(first[1], updated[1]) and not torch.equal(first[3], updated[3])
    for a, b in zip(updated, fresh):
        assert torch.equal(a, b)
    assert updated[3].abs().max().item() > 0


def test_edges(dev, oracle_libs):
    from diffphys_amd import hip_backend, sim

    # a chain whose child has no candidates, and the same chain without any candidate at all
    full = build_template(chain2(sim.JOINT_REVOLUTE))
    rng = np.random.RandomState(2)
    S = 5
    q = np.zeros((S, 2, 7), np.float32)
    q[..., 0] = rng.uniform(-1, 1, (S, 2))
    q[..., 1] = rng.uniform(0.02, 0.12, (S, 2))
    quat = rng.randn(S, 2, 4) * 0.2 + np.asarray([0, 0, 0, 1.0])
    q[..., 3:] = quat / np.linalg.norm(quat, axis=-1, keepdims=True)
    qd = (rng.randn(S, 2, 6) * 0.5).astype(np.float32)
    state = torch.from_numpy(np.concatenate([q, qd], -1).reshape(-1, 13)).to(dev)
    g_out = torch.from_numpy(rng.randn(S * 2, 6).astype(np.float32)).to(dev)
    for keep in (lambda b: b == 0, lambda b: b < 0):
        tpl = dict(full)
        sel = keep(np.asarray(full["contact_body"]))
        for k in ("contact_body", "contact_point", "contact_dist", "contact_material"):
            tpl[k] = np.ascontiguousarray(np.asarray(full[k])[sel])
        assert_off_the_ground(tpl, q, qd) if sel.any() else None
        table = hip_backend.contact_table(tpl, device=dev)
        nmat = len(tpl["shape_materials"])
        out = hip_backend.ground_wrench(table, 2, state)
        ref = wrench_and_state_grads(tpl, torch.float64, q, qd).reshape(-1, 6)
        assert relmax(out.cpu().numpy(), ref) <= 1e-5 if sel.any() else (out == 0).all()
        assert (out.view(S, 2, 6)[:, 1] == 0).all() and (sel.any() == bool(out.abs().max().item() > 0))
        g_s, g_m = hip_backend.ground_wrench_vjp(table, 2, nmat, state, g_out)
        assert (g_s.view(S, 2, 13)[:, 1] == 0).all() and (g_m.view(S, 2, nmat, 4)[:, 1] == 0).all()
        # n = 0
        empty = state[:0]
        assert hip_backend.ground_wrench(table, 2, empty).shape == (0, 6)
        e_s, e_m = hip_backend.ground_wrench_vjp(table, 2, nmat, empty, g_out[:0])
        assert e_s.shape == (0, 13) and e_m.shape == (0, nmat, 4)
        with pytest.raises(ValueError):
            hip_backend.ground_wrench(table, 2, state[:3])

    # either VJP output absent: the other one's bits; two runs: the same bits; a NaN state row: NaN in that element only
    C = case("laikago")
    st, nb = C["state"], C["nb"]
    g = torch.from_numpy(np.random.RandomState(4).randn(st.shape[0], 6).astype(np.float32)).to(dev)
    both = hip_backend.ground_wrench_vjp(C["table"], nb, 2, st, g)
    only_s = hip_backend.ground_wrench_vjp(C["table"], nb, 2, st, g, need_materials=False)
    only_m = hip_backend.ground_wrench_vjp(C["table"], nb, 2, st, g, need_state=False)
    again = hip_backend.ground_wrench_vjp(C["table"], nb, 2, st, g)
    assert only_s[1] is None and only_m[0] is None
    assert torch.equal(both[0], only_s[0]) and torch.equal(both[1], only_m[1])
    assert torch.equal(both[0], again[0]) and torch.equal(both[1], again[1])
    out = hip_backend.ground_wrench(C["table"], nb, st)
    assert torch.equal(out, hip_backend.ground_wrench(C["table"], nb, st))
    k = int(out.abs().amax(1).argmax().item())   # an element that touches
    bad = st.clone()
    bad[k] = float("nan")
    out_bad = hip_backend.ground_wrench(C["table"], nb, bad)
    assert torch.isnan(out_bad[k]).all()
    keep = torch.ones(st.shape[0], dtype=torch.bool, device=dev)
    keep[k] = False
    assert torch.equal(out_bad[keep], out[keep])
    with pytest.raises((TypeError, ValueError)):
        hip_backend.ground_wrench(C["table"], nb, st.cpu())
    with pytest.raises(TypeError):
        hip_backend.ground_wrench(C["table"], nb, st.double())
