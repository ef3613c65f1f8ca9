"""Zero controls: a NULL torques_dev / res_f_dev of the rollout entries means "all zeros" (include/ppr_diffphys.h, Zero controls).  Nothing
is read or allocated for an absent input, the forward launch runs the zero-controls twin of its kernel (csrc/pd_kernels.hip ZC), the
adjoint its selective twin, and EVERY result -- frame outputs, the whole workspace with its hit log, every gradient, g_torques and g_res_f
included -- is torch.equal to the launch that is given explicit torch.zeros tensors.

Shapes: the smallest that reach each kernel variant (see CASES); inputs are helpers.tight_inputs (feet in the ground, perturbed gains and
masses) with a random initial twist, so that contacts are made and broken inside the horizon, and the two controls zeroed.  Every
bit-identity case first asserts from the saved hit log that contacts were active."""
import ctypes
import os

import numpy as np
import pytest
import torch

from gpu_harness import FWD, SEEDED, dev, dev_inputs, device_model, warp_grads, warp_host  # noqa: F401
from helpers import GOLDEN, GRAD_LEAD, INPUT_NAMES, relmax, tight_inputs

pytestmark = pytest.mark.gpu

REST = ("target_ke", "target_kd", "body_inv_mass", "body_inertia", "body_inv_inertia")
STEPWISE = ("torques", "res_f", "refs")
# which of the two controls a launch is GIVEN: (torques, res_f)
MODES = {"res_f-null": (True, False), "torques-null": (False, True), "both-null": (False, False)}


def _template(key):
    from diffphys_amd import robots

    if key == "laikago_toes":  # 11 018 contact candidates: tables in global memory, the GT kernels
        with np.load(os.path.join(GOLDEN, "template_laikago_toes.npz")) as z:
            return {k: z[k] for k in z.files}, "laikago"
    return robots.load_template(key), key


def _inputs(key, bs, T, f2s, dev, seed=5):
    """-> (tpl, dt, dict of GPU tensors): tight inputs, kicked, frames at f2s with random seeds, torques and res_f ZERO"""
    tpl, robot = _template(key)
    inp = tight_inputs(tpl, robot, bs, T, seed)
    rng = np.random.RandomState(seed + 7)
    inp["qd_init"] = (rng.randn(*inp["qd_init"].shape) * 0.4).astype(np.float32)
    nb = int(tpl["nb"])
    inp["adj_pos"] = rng.randn(len(f2s), bs * nb, 7).astype(np.float32)
    inp["adj_vel"] = rng.randn(len(f2s), bs * nb, 6).astype(np.float32)
    inp["torques"] = np.zeros_like(inp["torques"])
    inp["res_f"] = np.zeros_like(inp["res_f"])
    t = dev_inputs(inp, dev, SEEDED)
    return tpl, float(inp["dt"]), t, inp


def _pair(t, mode):
    """(torques, res_f) of a launch: the zero tensors, or None where the mode leaves one out"""
    if mode is None:
        return t["torques"], t["res_f"]
    give_t, give_r = MODES[mode]
    return (t["torques"] if give_t else None), (t["res_f"] if give_r else None)


def _rollout(dm, bs, T, dt, f2s, t, mode, save=True, want=None, fam_bwd=None, state0=None, adj=None):
    """forward (into a zero-filled workspace, so that the log entries past a step's count compare too) and, with a workspace, the
    adjoint -> (outputs dict, gradients dict or None)"""
    from diffphys_amd import hip_backend

    tq, rf = _pair(t, mode)
    out = dm.alloc_rollout(bs, T, len(f2s), t["refs"].device, backward=False, save_trajectory=save)
    if save:
        out["ws"].zero_()
    init = (None, None) if state0 is not None else (t["q_init"], t["qd_init"])
    kw = dict(state0=state0) if state0 is not None else {}
    pos, vel, grf, jaf, ws = dm.rollout_forward(bs, T, dt, *init, tq, rf, t["refs"], *[t[k] for k in REST], frame2step=f2s, out=out,
                                                save_trajectory=save, **kw)
    o = dict(wp_pos=pos, wp_vel=vel, grf=grf, jaf=jaf)
    g = None
    if save:
        o["ws"] = ws.view(torch.int32)  # (planes and hit log: the mask plane and the log are integers)
        if fam_bwd is not None:
            dm.set_kernel_family(fam_bwd)
        ap, av = adj if adj is not None else (t["adj_pos"], t["adj_vel"])
        g = dm.rollout_backward(bs, T, dt, *init, tq, t["refs"], *[t[k] for k in REST], f2s, ws, ap, av,
                                want=hip_backend.GRAD_NAMES if want is None else want, **kw)
    torch.cuda.synchronize()
    return o, g


def _contacts_active(dm, ws_i32, bs, T):
    log = dm.saved_hit_log(ws_i32.view(torch.float32), bs, T)
    assert (log[..., 0] != 0).any(), "no contact in any env-step: the case would pass vacuously"


def _same(a, b, what):   # (not gpu_harness.same_bits: two dicts of tensors with the same keys, and it asserts)
    assert set(a) == set(b), (what, sorted(a), sorted(b))
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


def _variant_case(dev, key, bs, T, f2s, fam_fwd, fam_bwd, literal, segw=None, check=None):
    tpl, dt, t, _ = _inputs(key, bs, T, f2s, dev)
    dm = device_model(tpl, fam_fwd, segw, literal)
    o_ref, g_ref = _rollout(dm, bs, T, dt, f2s, t, None, fam_bwd=fam_bwd)
    _contacts_active(dm, o_ref["ws"], bs, T)
    if check:
        check(dm)
    assert set(g_ref) >= {"torques", "res_f", "refs"} and float(g_ref["res_f"].abs().max()) > 0.0
    for mode in MODES:
        dm.set_kernel_family(fam_fwd)
        o, g = _rollout(dm, bs, T, dt, f2s, t, mode, fam_bwd=fam_bwd)
        if check:
            check(dm)
        _same(o, o_ref, (key, mode, "outputs"))
        _same(g, g_ref, (key, mode, "gradients"))


# 1a-1g: (id, model, envs, steps, frames, forward family, adjoint family, segment width)
CASES = [
    ("1a-laikago-f1", "laikago", 6, 24, [0, 11, 24], 1, 1, None),
    ("1b-laikago-f2", "laikago", 6, 24, [0, 11, 24], 2, 2, None),
    ("1c-laikago-f2-fwd-f1-bwd", "laikago", 6, 24, [0, 11, 24], 2, 1, None),
    ("1d-human", "human", 4, 12, [0, 5, 12], 0, 0, None),          # compound robot: split forward, k_rollout_bwd3
    ("1e-quad", "quad", 3, 12, [0, 5, 12], 0, 0, None),
    ("1f-laikago-w64", "laikago", 6, 24, [0, 11, 24], 1, 1, 64),
    ("1g-laikago_toes", "laikago_toes", 2, 8, [0, 8], 0, 0, None),  # tables in global memory: the GT kernels
]


@pytest.mark.parametrize("literal", [False, True], ids=["stable", "literal"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_null_controls_give_the_zero_tensor_bits(dev, case, literal):
    """Cases 1a-1g: res_f NULL alone, torques NULL alone and both NULL, under both numeric policies -- outputs, the whole workspace and
    all ten gradients equal the explicit-zeros launch."""
    _, key, bs, T, f2s, ff, fb, segw = case
    _variant_case(dev, key, bs, T, f2s, ff, fb, literal, segw)


@pytest.mark.parametrize("literal", [False, True], ids=["stable", "literal"])
def test_large_batch_laikago_cull_wave_with_run_sums(dev, literal):
    """1h: Laikago 4 096 envs x 8 steps -- full workgroups: the CULLW + RUNSUM forward (three waves per env group, four groups)."""
    def check(dm):
        info = dm.last_launch_info(0)
        groups = info["envs_per_wg"] // (64 // dm.segment_width())
        assert info["threads_per_wg"] // 64 == 3 * groups and groups == 4, info

    _variant_case(dev, "laikago", 4096, 8, [0, 8], 0, 0, literal, check=check)


@pytest.mark.parametrize("literal", [False, True], ids=["stable", "literal"])
def test_large_batch_human_unsplit_forward(dev, literal):
    """1h: human at the smallest batch that selects the unsplit forward -- compound-only robots take it above PD_BWAVES (4) env groups per
    compute unit (csrc/pd_args.h pd_kernel_variant): 4 x CUs + 1 groups -- x 4 steps."""
    from diffphys_amd import hip_backend, robots

    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    epw = 64 // hip_backend.DeviceModel(robots.load_template("human")).segment_width()
    bs = 4 * cus * epw + 1

    def check(dm):
        info = dm.last_launch_info(0)
        assert info["threads_per_wg"] * epw == 64 * info["envs_per_wg"], info  # one wave per env group: the unsplit kernel ran

    _variant_case(dev, "human", bs, 4, [0, 4], 0, 0, literal, check=check)


FWD_ONLY = [("laikago", 6, 24, [0, 11, 24], 1), ("laikago", 6, 24, [0, 11, 24], 2), ("human", 4, 12, [0, 5, 12], 0), ("quad", 3, 12, [0, 5, 12], 0),
            ("laikago_toes", 2, 8, [0, 8], 0)]


@pytest.mark.parametrize("key,bs,T,f2s,family", FWD_ONLY, ids=["%s-f%d" % (c[0], c[4]) for c in FWD_ONLY])
def test_forward_only_composes(dev, key, bs, T, f2s, family):
    """2: the same robots with a NULL workspace and NULL controls: frame outputs equal the forward-only launch with zero tensors and the
    saving launch with zero tensors."""
    tpl, dt, t, _ = _inputs(key, bs, T, f2s, dev)
    dm = device_model(tpl, family)
    o_save, _ = _rollout(dm, bs, T, dt, f2s, t, None)
    _contacts_active(dm, o_save.pop("ws"), bs, T)
    o_ref, _ = _rollout(dm, bs, T, dt, f2s, t, None, save=False)
    _same(o_ref, o_save, (key, "forward-only zeros"))
    for mode in MODES:
        o, _ = _rollout(dm, bs, T, dt, f2s, t, mode, save=False)
        _same(o, o_ref, (key, mode, "forward-only"))


@pytest.mark.parametrize("ride", [False, True], ids=["traj_loss", "traj_loss_fk"])
@pytest.mark.parametrize("key,bs,T,f2s,family", [("laikago", 5, 20, [0, 9, 20], 1), ("laikago", 5, 20, [0, 9, 20], 2), ("human", 3, 12, [0, 5, 12], 0)],
                         ids=["laikago-f1", "laikago-f2", "human"])
def test_fused_entries(dev, key, bs, T, f2s, family, ride):
    """3: rollout_forward_traj_loss / rollout_backward_traj_loss, with and without the FK ride: loss table, reduced, scale, seeds, FK rows,
    frame outputs, workspace and all gradients (the LOSS instantiations of both Laikago families and of the split compound forward)."""
    tpl, dt, t, _ = _inputs(key, bs, T, f2s, dev)
    dm = device_model(tpl, family)
    nb, nq, nqd, F = dm.nb, dm.nq, dm.nqd, len(f2s)
    gen = torch.Generator().manual_seed(11)
    pos0 = dm.rollout_forward(bs, T, dt, *[t[k] for k in FWD], frame2step=f2s,
                              save_trajectory=False, want_forces=False)[0]
    tgt = (pos0.view(F, bs, nb, 7).permute(1, 0, 2, 3) + 0.05 * torch.randn(bs, F, nb, 7, generator=gen).to(dev)).contiguous()
    jq = (t["q_init"].view(1, bs, nq) + 0.1 * torch.randn(F, bs, nq, generator=gen).to(dev)).contiguous()
    jqd = (0.3 * torch.randn(F, bs, nqd, generator=gen)).to(dev).contiguous()
    aq, aqd = torch.randn(bs, F, nb, 7, generator=gen).to(dev), torch.randn(bs, F, nb, 6, generator=gen).to(dev)
    gain = torch.full((1,), 0.7, device=dev)

    def run(mode):
        tq, rf = _pair(t, mode)
        out = dm.alloc_rollout(bs, T, F, dev, backward=False)
        out["ws"].zero_()
        pos, vel, grf, jaf, ws, tl = dm.rollout_forward_traj_loss(bs, T, dt, t["q_init"], t["qd_init"], tq, rf, t["refs"], *[t[k] for k in REST],
                                                                  frame2step=f2s, target_pos=tgt, out=out, fk=(jq, jqd) if ride else None)
        o = dict(wp_pos=pos, wp_vel=vel, grf=grf, jaf=jaf, ws=ws.view(torch.int32))
        o.update({k: v.clone() for k, v in tl.items() if v is not None})
        g = dm.rollout_backward_traj_loss(bs, T, dt, t["q_init"], t["qd_init"], tq, t["refs"], *[t[k] for k in REST], f2s, ws, tl, gain,
                                          fk=(jq, jqd, aq, aqd) if ride else None)
        torch.cuda.synchronize()
        return o, g

    o_ref, g_ref = run(None)
    _contacts_active(dm, o_ref["ws"], bs, T)
    assert {"table", "reduced", "scale", "seed_pos", "seed_gt"} <= set(o_ref) and (not ride or {"fk_body_q", "fk_joint_q"} <= set(o_ref) | set(g_ref))
    assert float(o_ref["reduced"][0]) > 0.0 and float(g_ref["refs"].abs().max()) > 0.0
    for mode in MODES:
        o, g = run(mode)
        _same(o, o_ref, (key, ride, mode, "outputs"))
        _same(g, g_ref, (key, ride, mode, "gradients"))


def test_resumed_windows_chain(dev):
    """4: a 24-step rollout split at step 9 (not on a 4-step cull epoch boundary), both windows with NULL controls, chained through
    grads["state0"]: equals the single NULL launch (outputs, per-step and q_init / qd_init gradients bit for bit; the five sums over
    the steps are re-associated by the split, so they are compared against the explicit-zeros chain, which splits alike)."""
    key, bs, T, s = "laikago", 6, 24, 9
    f2s = [0, 9, 24]
    tpl, dt, t, _ = _inputs(key, bs, T, f2s, dev)
    dm = device_model(tpl, 1)
    o_one, g_one = _rollout(dm, bs, T, dt, f2s, t, "both-null")
    _contacts_active(dm, o_one["ws"], bs, T)

    def chain(mode):
        ta = dict(t, **{k: t[k][:s].contiguous() for k in STEPWISE})
        tb = dict(t, **{k: t[k][s:].contiguous() for k in STEPWISE})
        # window A: steps 0..9, frames at its states 0 and 9; window B resumes from the rows of A's last frame
        oa, _ = _rollout(dm, bs, s, dt, [0, s], ta, mode, save=False)
        st = torch.cat([oa["wp_pos"][1], oa["wp_vel"][1]], dim=1).contiguous()
        ob, gb = _rollout(dm, bs, T - s, dt, [0, T - s], tb, mode, state0=st, adj=(t["adj_pos"][1:].contiguous(), t["adj_vel"][1:].contiguous()))
        carry = gb["state0"]
        seeds = (torch.stack([t["adj_pos"][0], carry[:, :7]]).contiguous(), torch.stack([t["adj_vel"][0], carry[:, 7:]]).contiguous())
        oa2, ga = _rollout(dm, bs, s, dt, [0, s], ta, mode, adj=seeds)
        return oa, ob, ga, gb

    oa, ob, ga, gb = chain("both-null")
    za, zb, gza, gzb = chain(None)
    assert torch.equal(ob["wp_pos"][1], o_one["wp_pos"][2]) and torch.equal(ob["wp_vel"][1], o_one["wp_vel"][2])
    assert torch.equal(oa["wp_pos"][1], o_one["wp_pos"][1]) and torch.equal(ob["wp_pos"][0], o_one["wp_pos"][1])
    for k in STEPWISE:
        assert torch.equal(torch.cat([ga[k], gb[k]]), g_one[k]), k
    assert torch.equal(ga["q_init"], g_one["q_init"]) and torch.equal(ga["qd_init"], g_one["qd_init"])
    _same(ob, zb, "resumed window, outputs")
    _same(ga, gza, "first window, gradients")
    _same(gb, gzb, "resumed window, gradients")
    assert float(gb["state0"].abs().max()) > 0.0


@pytest.mark.parametrize("key,bs,family", [("laikago", 6, 1), ("laikago", 6, 2), ("human", 4, 0)], ids=["laikago-f1", "laikago-f2", "human"])
def test_selective_adjoint_composes(dev, key, bs, family):
    """4: res_f NULL with g_res_f wanted / declined, torques NULL with only g_refs wanted, both NULL with all three declined."""
    T, f2s = 12, [0, 5, 12]
    tpl, dt, t, _ = _inputs(key, bs, T, f2s, dev)
    dm = device_model(tpl, family)
    o_ref, g_ref = _rollout(dm, bs, T, dt, f2s, t, None)
    _contacts_active(dm, o_ref["ws"], bs, T)
    for mode, want in (("res_f-null", ("torques", "res_f", "refs")), ("res_f-null", ("torques", "refs")), ("torques-null", ("refs",)),
                       ("both-null", ())):
        o, g = _rollout(dm, bs, T, dt, f2s, t, mode, want=want)
        assert set(g) == set(g_ref) - (set(STEPWISE) - set(want)), (mode, want, sorted(g))
        _same(o, o_ref, (key, mode, want))
        for k in g:
            assert torch.equal(g[k], g_ref[k]), (key, mode, want, k)


@pytest.mark.parametrize("K", [None, 5], ids=["single-launch", "checkpoint-5"])
def test_forward_warp_with_none_controls(dev, monkeypatch, K):
    """5: ForwardWarp.apply(q, qd, None, None, refs, ...) against the same call with zero tensors: outputs and the .grad of every tensor
    input equal, nothing comes back for the two None positions.  K = 5 over 17 steps: the checkpointed adjoint (segments 5, 5, 5, 2)."""
    from diffphys_amd import dp_model

    bs, T = 6, 17
    f2s = [0, 8, 17]
    tpl, dt, t, _ = _inputs("laikago", bs, T, f2s, dev)
    h = warp_host("laikago", bs, T, f2s, dt, dev, K)
    pz, vz, gz = warp_grads(dp_model.ForwardWarp, INPUT_NAMES, t, h, t["adj_pos"], t["adj_vel"])
    assert float(torch.stack([x.abs().max() for x in h.grfs]).max()) > 0.0, "contacts must be active"
    pn, vn, gn = warp_grads(dp_model.ForwardWarp, INPUT_NAMES, t, h, t["adj_pos"], t["adj_vel"], absent=("torques", "res_f"))
    assert torch.equal(pn, pz) and torch.equal(vn, vz)
    assert gn["torques"] is None and gn["res_f"] is None
    for k in INPUT_NAMES:
        if k not in ("torques", "res_f"):
            assert torch.equal(gn[k], gz[k]), k
    assert float(gz["refs"].abs().max()) > 0.0
    # the Function itself hands None back for the two positions
    returned, orig = [], dp_model.ForwardWarp.backward

    def spy(ctx, *a):
        returned.append(orig(ctx, *a))
        return returned[-1]

    monkeypatch.setattr(dp_model.ForwardWarp, "backward", staticmethod(spy))
    warp_grads(dp_model.ForwardWarp, INPUT_NAMES, t, h, t["adj_pos"], t["adj_vel"], absent=("torques", "res_f"))
    assert len(returned) == 1 and returned[0][2] is None and returned[0][3] is None and returned[0][4] is not None


def test_forward_warp_state_with_none_controls(dev):
    """5: the same through ForwardWarpState: a window resumed from a body state."""
    from diffphys_amd import dp_model

    bs, T, s = 6, 17, 8
    f2s = [0, 8, 17]
    tpl, dt, t, _ = _inputs("laikago", bs, T, f2s, dev)
    dm = device_model(tpl, 0)
    pos, vel = dm.rollout_forward(bs, T, dt, *[t[k] for k in FWD], frame2step=f2s,
                                  save_trajectory=False)[:2]
    names = ("body_q0", "body_qd0") + INPUT_NAMES[2:]
    tin = dict(t, body_q0=pos[1].clone(), body_qd0=vel[1].clone())
    for k in STEPWISE:
        tin[k] = t[k][s:].contiguous()
    h = warp_host("laikago", bs, T - s, [0, T - s], dt, dev, None)
    ap, av = t["adj_pos"][1:], t["adj_vel"][1:]
    pz, vz, gz = warp_grads(dp_model.ForwardWarpState, names, tin, h, ap, av)
    assert float(torch.stack([x.abs().max() for x in h.grfs]).max()) > 0.0, "contacts must be active"
    pn, vn, gn = warp_grads(dp_model.ForwardWarpState, names, tin, h, ap, av, absent=("torques", "res_f"))
    assert torch.equal(pn, pz) and torch.equal(vn, vz) and torch.equal(pn[1], pos[2])
    assert gn["torques"] is None and gn["res_f"] is None
    for k in names:
        if k not in ("torques", "res_f"):
            assert torch.equal(gn[k], gz[k]), k
    assert float(gz["body_q0"].abs().max()) > 0.0


def test_peak_memory_drops_by_exactly_the_two_tensors(dev):
    """6: Laikago 64 envs x 200 steps, checkpoint_steps = 20, only target_ke requiring a gradient (the shape of the selective adjoint's
    memory test).  Peak allocated memory over forward + backward, measured from the same baseline -- everything but the two controls
    resident -- is lower with None controls by exactly their bytes, 200 x 64 x (13 x 6 + 18) x 4: every other allocation is the same."""
    from diffphys_amd import dp_model, robots, synth

    bs, T, K = 64, 200, 20
    tpl = robots.load_template("laikago")
    nb, nqd = int(tpl["nb"]), int(tpl["nqd"])
    assert (nb, nqd) == (13, 18)
    inp = synth.make_inputs(tpl, "laikago", bs=bs, nsteps=T, seed=2, steps_per_frame=100, penetration=0.003)
    f2s = [int(x) for x in inp["frame2step"]]
    t = dev_inputs(inp, dev, [k for k in INPUT_NAMES if k not in ("torques", "res_f")])
    ap, av = dev_inputs(inp, dev, ("adj_pos", "adj_vel")).values()
    h = warp_host("laikago", bs, T, f2s, float(inp["dt"]), dev, K)
    expect = T * bs * (nb * 6 + nqd) * 4

    def peak(with_tensors):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        x = {k: t[k].detach().requires_grad_(k == "target_ke") for k in t}
        if with_tensors:  # what a caller without the feature has to make: the two all-zero inputs
            x["torques"] = torch.zeros(T, bs * nqd, dtype=torch.float32, device=dev)
            x["res_f"] = torch.zeros(T, bs * nb, 6, dtype=torch.float32, device=dev)
        pos, vel = dp_model.ForwardWarp.apply(*[x.get(k) for k in INPUT_NAMES], h)
        ((pos * ap).sum() + (vel * av).sum()).backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, x["target_ke"].grad.clone(), pos.detach().clone()

    peak(False)  # (warm-up: the frame tables and the allocator's pools exist before anything is measured)
    p_zero, g_zero, pos_zero = peak(True)
    p_none, g_none, pos_none = peak(False)
    print("peak over forward + backward: zero tensors %d B, None %d B, difference %d B, the two tensors are %d B" % (p_zero, p_none, p_zero - p_none, expect))
    assert torch.equal(g_none, g_zero) and torch.equal(pos_none, pos_zero) and float(g_zero.abs().max()) > 0.0
    assert p_zero - p_none == expect, (p_zero, p_none, expect)


def test_phys_model_passes_no_zero_tensors(dev, monkeypatch):
    """7: one forward() + backward() at the reference window with the default skip_zeroed_mlps and absent_zero_controls = True: no
    torch.zeros of the two control shapes is made during forward(), the rollout gets None for both, contacts are active, and every
    loss term and parameter gradient equals the run that passes zero tensors (absent_zero_controls = False, the default -- an existing
    test hooks the rollout launch and reads its ten input tensors, so the default still hands over ten tensors)."""
    from diffphys_amd import hip_backend
    from test_gpu_workload import _model as workload_model

    def run(as_tensors):
        model, opts = workload_model("mi-pace", "zero_controls")
        model.absent_zero_controls = not as_tensors
        model.reinit_envs(opts["num_envs"], frames_per_wdw=opts["frames_per_wdw"])
        n, T = model.num_envs, len(model.steps_idx)
        shapes = {(n, T, 6 + model.n_dof), (n, T, 6 * model.n_links), (T, n * (6 + model.n_dof)), (T, n * model.n_links, 6)}
        made, seen = [], {}
        orig_zeros, orig_fwd = torch.zeros, hip_backend.DeviceModel.rollout_forward_traj_loss

        def zeros(*size, **kw):
            sh = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)
            if sh in shapes:
                made.append(sh)
            return orig_zeros(*size, **kw)

        def fwd(dm, bs, nsteps, dt, q_init, qd_init, torques, res_f, *a, **kw):
            seen.update(torques=torques, res_f=res_f, bs=bs, nsteps=nsteps, dm=dm)
            r = orig_fwd(dm, bs, nsteps, dt, q_init, qd_init, torques, res_f, *a, **kw)
            seen["ws"] = r[4]
            return r

        monkeypatch.setattr(hip_backend.DeviceModel, "rollout_forward_traj_loss", fwd)
        monkeypatch.setattr(torch, "zeros", zeros)
        np.random.seed(321)
        try:
            out = model.forward()
        finally:
            monkeypatch.setattr(torch, "zeros", orig_zeros)
            monkeypatch.setattr(hip_backend.DeviceModel, "rollout_forward_traj_loss", orig_fwd)
        model.backward(out["total_loss"])
        torch.cuda.synchronize()
        log = seen["dm"].saved_hit_log(seen["ws"], seen["bs"], seen["nsteps"])
        assert (log[..., 0] != 0).any(), "no contact in the window"
        losses = {k: v.detach().clone() for k, v in out.items()}
        grads = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()}
        return made, seen, losses, grads

    made, seen, losses, grads = run(False)
    assert made == [] and seen["torques"] is None and seen["res_f"] is None, (made, type(seen["torques"]))
    made_z, seen_z, losses_z, grads_z = run(True)
    assert len(made_z) == 2 and seen_z["torques"] is not None and seen_z["res_f"] is not None and float(seen_z["res_f"].abs().max()) == 0.0
    assert set(losses) == set(losses_z) and {"loss_reg_torque", "loss_reg_res_f"} <= set(losses)
    for k in losses:
        assert torch.equal(losses[k], losses_z[k]), k
    assert float(losses["loss_reg_torque"]) == 0.0 and float(losses["loss_reg_res_f"]) == 0.0
    assert set(grads) == set(grads_z) and any(g is not None and float(g.abs().sum()) > 0 for g in grads.values())
    for k in grads:
        assert (grads[k] is None) == (grads_z[k] is None) and (grads[k] is None or torch.equal(grads[k], grads_z[k])), k


SENTINEL = -12345.678


def test_refusals(dev):
    """8: with sentinel-filled outputs -- a NULL refs is still refused, by name, and the refused call writes nothing (forward and
    adjoint); NULL controls with nsteps == 0 are accepted and the frame at state 0 equals FK."""
    from diffphys_amd import hip_backend

    bs, T, f2s = 6, 12, [0, 5, 12]
    tpl, dt, t, _ = _inputs("laikago", bs, T, f2s, dev)
    dm = device_model(tpl, 0)
    lib = hip_backend.lib()
    nb, F = dm.nb, len(f2s)
    full = lambda *s: torch.full(s, SENTINEL, dtype=torch.float32, device=dev)
    pos, vel, grf, jaf, ws = full(F, bs * nb, 7), full(F, bs * nb, 6), full(F, bs * nb, 6), full(F, bs * nb, 6), full(dm.workspace_floats(bs, T))
    f2s_c = (ctypes.c_int * F)(*f2s)
    ptr = lambda x: None if x is None else x.data_ptr()
    for tq, rf in ((t["torques"], t["res_f"]), (None, None)):
        rc = lib.pd_rollout_forward(dm.h, bs, T, ctypes.c_float(dt), ptr(t["q_init"]), ptr(t["qd_init"]), ptr(tq), ptr(rf), None,
                                    *[ptr(t[k]) for k in REST], F, f2s_c, ptr(ws), ptr(pos), ptr(vel), ptr(grf), ptr(jaf), hip_backend._stream())
        torch.cuda.synchronize()
        msg = lib.pd_last_error().decode()
        assert rc != 0 and "null device pointer" in msg and "refs" in msg, (rc, msg)
        for x in (pos, vel, grf, jaf, ws):
            assert bool((x == SENTINEL).all())
    # the adjoint: a real workspace, sentinel-filled gradients
    _, _, _, _, ws_ok = dm.rollout_forward(bs, T, dt, t["q_init"], t["qd_init"], None, None, t["refs"], *[t[k] for k in REST], frame2step=f2s)
    g = {k: v.fill_(SENTINEL) for k, v in dm._alloc_grads(bs, T, dev).items()}
    rc = lib.pd_rollout_backward(dm.h, bs, T, ctypes.c_float(dt), ptr(t["q_init"]), ptr(t["qd_init"]), None, None, *[ptr(t[k]) for k in REST],
                                 F, f2s_c, ptr(ws_ok), ptr(t["adj_pos"]), ptr(t["adj_vel"]), *[ptr(g[k]) for k in FWD], hip_backend._stream())
    torch.cuda.synchronize()
    msg = lib.pd_last_error().decode()
    assert rc != 0 and "null device pointer" in msg and "refs" in msg, (rc, msg)
    assert all(bool((v == SENTINEL).all()) for v in g.values())
    # no steps: nothing to control -- NULL for all three per-step inputs is accepted, and the frame at state 0 is FK of (q_init, qd_init):
    # the bits of state 0 of the 12-step launch (eval_fk inside the rollout kernel), and pd_fk_forward's poses to the 1e-6 that
    # tests/test_gpu_tight.py holds the two FK codes to
    p0, v0, _, _, _ = dm.rollout_forward(bs, 0, dt, t["q_init"], t["qd_init"], None, None, None, *[t[k] for k in REST], frame2step=[0])
    pT, vT, _, _, _ = dm.rollout_forward(bs, T, dt, t["q_init"], t["qd_init"], t["torques"], t["res_f"], t["refs"], *[t[k] for k in REST],
                                         frame2step=f2s)
    bq, _ = dm.fk_forward(t["q_init"].view(bs, -1), t["qd_init"].view(bs, -1))
    torch.cuda.synchronize()
    assert torch.equal(p0[0], pT[0]) and torch.equal(v0[0], vT[0])
    assert relmax(bq.cpu().numpy().reshape(-1, 7), p0[0].cpu().numpy()) < 1e-6


CAPS = {  # tests/test_gpu_tight.py, test_short_horizon_tight: absolute caps (relmax per tensor) -- pose, twist, wrench, gradient
    "laikago": (2e-6, 3e-4, 3e-4, 6e-4),
    "human": (2e-6, 2e-5, 3e-4, 1e-4),
}


@pytest.mark.parametrize("key,bs,family", [("laikago", 6, 1), ("human", 4, 0)], ids=["1a-laikago", "1d-human"])
def test_null_launch_against_the_float64_oracle(dev, oracle_libs, key, bs, family):
    """A fault common to both launches of a pair cannot hide: the inputs of cases 1a / 1d at 3 steps, NULL launch, against the float64 C
    oracle run on zero arrays -- the bars of test_gpu_tight.test_short_horizon_tight: every tensor within 4 x the fp32 C oracle's own
    error against float64 (or that test's floors, 1e-6 poses and twists / 1e-5 wrenches and gradients), and under its absolute caps."""
    from oracle.ref_c import RefC

    T, f2s = 3, [0, 3]
    tpl, dt, t, inp = _inputs(key, bs, T, f2s, dev)
    inp = dict(inp, frame2step=f2s, nsteps=T)
    assert not inp["torques"].any() and not inp["res_f"].any()
    dm = device_model(tpl, family)
    o, g = _rollout(dm, bs, T, dt, f2s, t, "both-null")
    _contacts_active(dm, o["ws"], bs, T)
    res = {}
    for dtype in (np.float64, np.float32):
        rc = RefC(tpl, dtype)
        st = rc.rollout_forward(inp, T, f2s, dt)
        res[dtype] = (st, rc.rollout_backward(st, inp["adj_pos"], inp["adj_vel"]))
    (s64, g64), (s32, g32) = res[np.float64], res[np.float32]
    cap_p, cap_v, cap_w, cap_g = CAPS[key]

    def check(what, a, c32, ref, cap, floor):
        e_gpu, e_c = relmax(a.cpu().numpy().reshape(np.shape(ref)), ref), relmax(c32, ref)
        print("%s %s: GPU %.3e, fp32 C oracle %.3e" % (key, what, e_gpu, e_c))
        assert np.isfinite(e_gpu) and e_gpu <= cap, "%s: GPU error %.2e above the cap %.1e (fp32 C oracle: %.2e)" % (what, e_gpu, cap, e_c)
        assert e_gpu <= max(4 * e_c, floor), "%s: GPU error %.2e vs fp32 C oracle %.2e" % (what, e_gpu, e_c)

    check("wp_pos", o["wp_pos"], s32["wp_pos"], s64["wp_pos"], cap_p, 1e-6)
    check("wp_vel", o["wp_vel"], s32["wp_vel"], s64["wp_vel"], cap_v, 1e-6)
    check("grf", o["grf"], s32["grf"], s64["grf"], cap_w, 1e-5)
    check("jaf", o["jaf"], s32["jaf"], s64["jaf"], cap_w, 1e-5)
    for k in GRAD_LEAD:
        assert np.abs(g64[k]).max() > 0, k
        check("grad " + k, g[k], g32[k], g64[k], cap_g, 1e-5)
