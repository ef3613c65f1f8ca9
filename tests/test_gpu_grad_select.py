"""Selective adjoint: g_torques_dev / g_res_f_dev / g_refs_dev of pd_rollout_backward, pd_rollout_backward_traj_loss and
pd_rollout_backward_traj_loss_fk may each be NULL ("not wanted").  Such a launch runs the selective instantiation of the adjoint kernel
(csrc/pd_kernels.hip SEL), stores nothing for an absent gradient, and every gradient that is asked for -- the remaining per-step ones,
g_q_init / g_qd_init, the state gradient of a resumed rollout, the five summed ones, the FK ride's -- is the all-three launch's, bit for bit.

Shapes: the smallest at which the kernels can still go wrong -- Laikago 5 envs (not a multiple of the four envs of a wave: a partly filled
segment group, cloned slots) x 12 steps with frames at steps 0, 5, 12, kicked so that contacts are made and broken inside the horizon;
human and quad 3 envs (k_rollout_bwd3 at width 32: one full wave and a half-filled one)."""
import itertools

import numpy as np
import pytest
import torch

from gpu_harness import BWD, FWD, SEEDED, dev, dev_inputs, device_model, warp_grads, warp_host  # noqa: F401
from helpers import INPUT_NAMES, tight_inputs

pytestmark = pytest.mark.gpu

PARAMS = ("target_ke", "target_kd", "body_inv_mass", "body_inertia", "body_inv_inertia")
STEPWISE = ("torques", "res_f", "refs")
# the seven proper subsets of the three per-step gradients, the empty one first
SUBSETS = [s for n in range(3) for s in itertools.combinations(STEPWISE, n)]
T12, F2S = 12, [0, 5, 12]
# (robot, envs, kernel family, numeric policy literal)
CASES = [("laikago", 5, 1, False), ("laikago", 5, 2, False), ("human", 3, 0, False), ("quad", 3, 0, False)]
LITERAL_CASES = [("laikago", 5, 1, True), ("human", 3, 0, True)]


def _inputs(robot, bs, T=T12, f2s=F2S, seed=3):
    """helpers.tight_inputs (feet in the ground, non-zero twists / torques / residual wrenches, perturbed gains and masses), kicked: the
    feet leave and hit the ground inside the horizon; frames at f2s with random seeds on every one"""
    from diffphys_amd import robots

    tpl = robots.load_template(robot)
    inp = tight_inputs(tpl, robot, bs, T, seed)
    rng = np.random.RandomState(seed + 7)
    inp["qd_init"] = (rng.randn(*inp["qd_init"].shape) * 0.4).astype(np.float32)
    nb = int(tpl["nb"])
    inp["frame2step"] = list(f2s)
    inp["adj_pos"] = rng.randn(len(f2s), bs * nb, 7).astype(np.float32)
    inp["adj_vel"] = rng.randn(len(f2s), bs * nb, 6).astype(np.float32)
    return tpl, inp


_BUNDLES = {}


def _bundle(dev, robot, bs, family, literal):
    """One saving forward and the all-three adjoint of a case, computed once and left unchanged: (dm, inp, tensors, ws, reference grads)"""
    key = (robot, bs, family, literal)
    if key not in _BUNDLES:
        tpl, inp = _inputs(robot, bs)
        dm = device_model(tpl, family, literal=literal)
        t = dev_inputs(inp, dev, SEEDED)
        pos, vel, grf, jaf, ws = dm.rollout_forward(bs, T12, inp["dt"], *[t[k] for k in FWD], frame2step=F2S)
        assert float(grf.abs().max()) > 0.0, "contacts must be active"
        g = dm.rollout_backward(bs, T12, inp["dt"], *[t[k] for k in BWD], F2S, ws, t["adj_pos"], t["adj_vel"])
        torch.cuda.synchronize()
        ref = {k: v.clone() for k, v in g.items()}
        assert set(ref) == set(BWD[:2] + STEPWISE + PARAMS)
        for k, v in ref.items():
            assert bool(torch.isfinite(v).all()), k
        for k in STEPWISE + ("q_init", "target_ke"):
            assert float(ref[k].abs().max()) > 0.0, k
        _BUNDLES[key] = (dm, inp, t, ws, ref, (pos, vel))
    return _BUNDLES[key]


def _assert_same(g, ref, what):
    for k in g:
        assert torch.equal(g[k], ref[k]), (what, k, float((g[k] - ref[k]).abs().max()))


def _subsets_case(dev, robot, bs, family, literal, subsets):
    dm, inp, t, ws, ref, _ = _bundle(dev, robot, bs, family, literal)
    for want in subsets:
        g = dm.rollout_backward(bs, T12, inp["dt"], *[t[k] for k in BWD], F2S, ws, t["adj_pos"], t["adj_vel"], want=want)
        torch.cuda.synchronize()
        assert set(g) == set(ref) - (set(STEPWISE) - set(want)), (want, sorted(g))
        _assert_same(g, ref, (robot, family, literal, want))
    # the all-three launch after the selective ones: the kernel it always ran, the same bits again
    g = dm.rollout_backward(bs, T12, inp["dt"], *[t[k] for k in BWD], F2S, ws, t["adj_pos"], t["adj_vel"])
    torch.cuda.synchronize()
    assert set(g) == set(ref)
    _assert_same(g, ref, (robot, family, literal, "all"))


@pytest.mark.parametrize("robot,bs,family,literal", CASES)
def test_every_subset_gives_the_all_three_launchs_bits(dev, robot, bs, family, literal):
    """One saving forward, the all-three adjoint, then the selective adjoint of each of the seven proper subsets (the empty one included)
    on the same workspace: every gradient present in both is torch.equal, nothing exempt.  Lane-per-body and quad-lane k_rollout_bwd
    (Laikago family 1 / 2), k_rollout_bwd3 for compound (human) and generic (quad) joint mixes.  The empty subset is refused ("null
    device pointer") by a library without the feature."""
    _subsets_case(dev, robot, bs, family, literal, SUBSETS)


@pytest.mark.parametrize("robot,bs,family,literal", LITERAL_CASES)
def test_literal_policy_empty_and_res_f_only(dev, robot, bs, family, literal):
    """The PD_NUM_LITERAL objects have selective twins of their own: the empty subset and res_f alone."""
    _subsets_case(dev, robot, bs, family, literal, [(), ("res_f",)])


SENTINEL = 0x5A5A5A5A  # as a float 1.5e16: no gradient of these workloads


def _arena_grads(dm, bs, T, want, dev, resumed=False):
    """The adjoint's output buffers carved out of ONE arena filled with a sentinel bit pattern, 64 sentinel floats between neighbours and
    behind the last -> (arena as int32, dict of float views, list of (start, stop) float ranges the buffers occupy)"""
    nb, nq, nqd = dm.nb, dm.nq, dm.nqd
    shapes = dict(state0=(bs * nb, 13)) if resumed else dict(q_init=(bs * nq,), qd_init=(bs * nqd,))
    step = dict(torques=(T, bs * nqd), res_f=(T, bs * nb, 6), refs=(T, bs * nqd))
    shapes.update({k: step[k] for k in STEPWISE if k in want})
    shapes.update(target_ke=(bs * nqd,), target_kd=(bs * nqd,), body_inv_mass=(bs * nb,), body_inertia=(bs * nb, 3, 3), body_inv_inertia=(bs * nb, 3, 3))
    spans, off = {}, 64
    for k, sh in shapes.items():
        n = int(np.prod(sh))
        spans[k] = (off, off + n)
        off = (off + n + 64 + 3) & ~3   # 16-byte aligned starts
    arena = torch.full((off,), SENTINEL, dtype=torch.int32, device=dev)
    views = {k: arena[a:b].view(torch.float32).view(*shapes[k]) for k, (a, b) in spans.items()}
    return arena, views, spans


def _assert_arena(arena, spans, what):
    a = arena.cpu().numpy()
    used = np.zeros(a.shape, bool)
    for k, (lo, hi) in spans.items():
        used[lo:hi] = True
        assert not (a[lo:hi] == SENTINEL).any(), (what, k, "not fully overwritten: %d sentinels left" % int((a[lo:hi] == SENTINEL).sum()))
    assert (a[~used] == SENTINEL).all(), (what, "written outside the buffers at", np.nonzero(~used & (a != SENTINEL))[0][:8].tolist())


@pytest.mark.parametrize("robot,bs,family,literal", CASES)
def test_nothing_is_written_where_nothing_was_asked(dev, robot, bs, family, literal):
    """All output gradients in one sentinel-filled arena with sentinel gaps: after a selective launch the gaps and the tail are untouched
    and every wanted buffer is overwritten completely (the root's zero dof columns of g_torques / g_refs included), with the reference
    bits."""
    dm, inp, t, ws, ref, _ = _bundle(dev, robot, bs, family, literal)
    for want in SUBSETS:
        arena, views, spans = _arena_grads(dm, bs, T12, want, dev)
        g = dm.rollout_backward(bs, T12, inp["dt"], *[t[k] for k in BWD], F2S, ws, t["adj_pos"], t["adj_vel"], out=dict(grads=views), want=want)
        torch.cuda.synchronize()
        assert set(g) == set(views)
        _assert_arena(arena, spans, (robot, family, want))
        _assert_same(g, ref, (robot, family, want))


@pytest.mark.parametrize("robot,bs,family", [("laikago", 5, 1), ("human", 3, 0)])
def test_resumed_mode_composes(dev, robot, bs, family):
    """The chain split at step 5 of 12: the later segment, resumed from the body state of frame 5.  Its selective adjoints (empty subset,
    torques only) give the state gradient g_q_init [bs*nb][13], the wanted per-step gradients and the summed ones of the all-three
    resumed launch, bit for bit; nothing is written outside the buffers."""
    dm, inp, t, ws, ref, (pos, vel) = _bundle(dev, robot, bs, family, False)
    s, dt = 5, inp["dt"]
    st = torch.cat([pos[1], vel[1]], dim=1).contiguous()
    ctl = [t[k][s:].contiguous() for k in STEPWISE]
    par = [t[k] for k in PARAMS]
    fb = [0, T12 - s]
    ap, av = t["adj_pos"][1:].contiguous(), t["adj_vel"][1:].contiguous()
    _, _, grf, _, ws_b = dm.rollout_forward(bs, T12 - s, dt, None, None, *ctl, *par, frame2step=fb, state0=st)
    assert float(grf.abs().max()) > 0.0, "contacts must be active"
    g_all = dm.rollout_backward(bs, T12 - s, dt, None, None, ctl[0], ctl[2], *par, fb, ws_b, ap, av, state0=st)
    torch.cuda.synchronize()
    g_all = {k: v.clone() for k, v in g_all.items()}
    assert g_all["state0"].shape == (bs * dm.nb, 13) and float(g_all["state0"].abs().max()) > 0.0
    for want in ((), ("torques",)):
        arena, views, spans = _arena_grads(dm, bs, T12 - s, want, dev, resumed=True)
        g = dm.rollout_backward(bs, T12 - s, dt, None, None, ctl[0], ctl[2], *par, fb, ws_b, ap, av, state0=st, out=dict(grads=views), want=want)
        torch.cuda.synchronize()
        assert set(g) == {"state0"} | set(want) | set(PARAMS)
        _assert_arena(arena, spans, (robot, "resumed", want))
        _assert_same(g, g_all, (robot, "resumed", want))


@pytest.mark.parametrize("family", [1, 2])
def test_traj_loss_fk_entry(dev, family):
    """pd_rollout_backward_traj_loss_fk with an FK ride of 3 frames x bs on Laikago, 5 envs: the empty subset and refs alone give the
    wanted gradients and the ride's g_joint_q / g_joint_qd of the all-three call, bit for bit."""
    dm, inp, t, _, _, _ = _bundle(dev, "laikago", 5, family, False)
    bs, nb, nq, nqd, F = 5, dm.nb, dm.nq, dm.nqd, len(F2S)
    gen = torch.Generator().manual_seed(11)
    jq = (t["q_init"].view(1, bs, nq) + 0.1 * torch.randn(F, bs, nq, generator=gen).to(dev)).contiguous()
    jqd = (0.3 * torch.randn(F, bs, nqd, generator=gen)).to(dev).contiguous()
    pos0, _, _, _, _ = dm.rollout_forward(bs, T12, inp["dt"], *[t[k] for k in FWD], frame2step=F2S, save_trajectory=False, want_forces=False)
    tgt = (pos0.view(F, bs, nb, 7).permute(1, 0, 2, 3) + 0.05 * torch.randn(bs, F, nb, 7, generator=gen).to(dev)).contiguous()
    o = dm.rollout_forward_traj_loss(bs, T12, inp["dt"], *[t[k] for k in FWD], frame2step=F2S, target_pos=tgt, fk=(jq, jqd))
    aq = torch.randn(bs, F, nb, 7, generator=gen).to(dev)
    aqd = torch.randn(bs, F, nb, 6, generator=gen).to(dev)
    gain = torch.full((1,), 0.7, device=dev)
    run = lambda **kw: dm.rollout_backward_traj_loss(bs, T12, inp["dt"], *[t[k] for k in BWD], F2S, o[4], o[5], gain, fk=(jq, jqd, aq, aqd), **kw)
    ref = {k: v.clone() for k, v in run().items()}
    torch.cuda.synchronize()
    assert float(ref["fk_joint_q"].abs().max()) > 0.0 and float(ref["refs"].abs().max()) > 0.0 and float(ref["res_f"].abs().max()) > 0.0
    for want in ((), ("refs",)):
        g = run(want=want)
        torch.cuda.synchronize()
        assert set(g) == set(ref) - (set(STEPWISE) - set(want))
        _assert_same(g, ref, ("traj_loss_fk", family, want))


class _Spy:
    """records the ``want`` of every DeviceModel.rollout_backward call"""

    def __init__(self, monkeypatch):
        from diffphys_amd import hip_backend

        self.wants = []
        orig = hip_backend.DeviceModel.rollout_backward

        def spy(dm, *a, **kw):
            self.wants.append(tuple(kw.get("want", hip_backend.GRAD_NAMES)))
            return orig(dm, *a, **kw)

        monkeypatch.setattr(hip_backend.DeviceModel, "rollout_backward", spy)


@pytest.mark.parametrize("K", [None, 5], ids=["single-launch", "checkpoint-5"])
def test_forward_warp_asks_only_for_what_needs_a_gradient(dev, monkeypatch, K):
    """ForwardWarp.apply with requires_grad on torques and target_ke only: the adjoint launches ask for g_torques alone, torques.grad and
    target_ke.grad are those of the run where every input requires a gradient, bit for bit, res_f.grad and refs.grad are None.  K = 5:
    the checkpointed adjoint, segments 5, 5, 2 (5 is no multiple of the 4-step cull epoch), against the unselective checkpointed run."""
    from diffphys_amd import dp_model

    _, inp, t, _, _, _ = _bundle(dev, "laikago", 5, 1, False)
    bs, ap, av = 5, t["adj_pos"], t["adj_vel"]
    h = warp_host("laikago", bs, T12, F2S, inp["dt"], dev, K)
    full = warp_grads(dp_model.ForwardWarp, INPUT_NAMES, t, h, ap, av)[2]
    spy = _Spy(monkeypatch)
    sel = warp_grads(dp_model.ForwardWarp, INPUT_NAMES, t, h, ap, av, needs=("torques", "target_ke"))[2]
    assert spy.wants == [("torques",)] * (3 if K else 1), spy.wants
    assert torch.equal(sel["torques"], full["torques"]) and torch.equal(sel["target_ke"], full["target_ke"])
    assert float(full["torques"].abs().max()) > 0.0 and float(full["res_f"].abs().max()) > 0.0
    assert all(sel[k] is None for k in INPUT_NAMES if k not in ("torques", "target_ke")), {k: v is None for k, v in sel.items()}


def test_forward_warp_state_with_only_the_body_state(dev, monkeypatch):
    """ForwardWarpState.apply with only the body state requiring a gradient: the empty subset goes to the resumed adjoint; the state's
    gradients equal those of the run where everything requires one."""
    from diffphys_amd import dp_model

    _, inp, t, _, _, (pos, vel) = _bundle(dev, "laikago", 5, 1, False)
    s, bs = 5, 5
    names = ("body_q0", "body_qd0") + INPUT_NAMES[2:]
    tin = dict(t, body_q0=pos[1], body_qd0=vel[1])
    for k in STEPWISE:
        tin[k] = t[k][s:].contiguous()
    h = warp_host("laikago", bs, T12 - s, [0, T12 - s], inp["dt"], dev, None)
    ap, av = t["adj_pos"][1:], t["adj_vel"][1:]
    full = warp_grads(dp_model.ForwardWarpState, names, tin, h, ap, av)[2]
    spy = _Spy(monkeypatch)
    sel = warp_grads(dp_model.ForwardWarpState, names, tin, h, ap, av, needs=("body_q0", "body_qd0"))[2]
    assert spy.wants == [()], spy.wants
    assert torch.equal(sel["body_q0"], full["body_q0"]) and torch.equal(sel["body_qd0"], full["body_qd0"]) and float(full["body_q0"].abs().max()) > 0.0
    assert all(sel[k] is None for k in names[2:])


def test_backward_peak_memory_drops_by_the_per_step_gradients(dev):
    """Laikago 64 envs x 200 steps, checkpoint_steps = 20: the three per-step gradient tensors are T * bs * (2 nqd + 6 nb) * 4 = 5.8 MB and
    dominate the ~1.5 MB segment workspace.  The peak of backward() with only target_ke requiring a gradient lies below the peak with
    every input requiring one by at least 0.9 of that (derived; the 0.1 is the allocator's rounding)."""
    from diffphys_amd import dp_model, robots, synth

    bs, T, K = 64, 200, 20
    tpl = robots.load_template("laikago")
    nb, nqd = int(tpl["nb"]), int(tpl["nqd"])
    inp = synth.make_inputs(tpl, "laikago", bs=bs, nsteps=T, seed=2, steps_per_frame=100, penetration=0.003)
    f2s = [int(x) for x in inp["frame2step"]]
    t = dev_inputs(inp, dev, SEEDED)
    ap, av = t["adj_pos"], t["adj_vel"]
    h = warp_host("laikago", bs, T, f2s, inp["dt"], dev, K)

    def peak(needs):
        x = {k: t[k].detach().clone().requires_grad_(k in needs) for k in INPUT_NAMES}
        pos, vel = dp_model.ForwardWarp.apply(*[x[k] for k in INPUT_NAMES], h)
        loss = (pos * ap).sum() + (vel * av).sum()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss.backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base, x

    p_all, x_all = peak(INPUT_NAMES)
    p_sel, x_sel = peak(("target_ke",))
    expect = T * bs * (2 * nqd + 6 * nb) * 4
    print("backward peak: all inputs %d B, target_ke only %d B, difference %d B, the per-step gradients are %d B" % (p_all, p_sel, p_all - p_sel, expect))
    assert torch.equal(x_sel["target_ke"].grad, x_all["target_ke"].grad) and x_sel["torques"].grad is None
    assert p_all - p_sel >= 0.9 * expect, (p_all, p_sel, expect)


def test_selective_launch_is_captured_and_reported(dev):
    """The empty-subset adjoint, captured into a HIP graph after one warm-up and replayed twice, gives the eager launch's bits (nothing
    allocates or synchronises in the launch path); pd_last_kernel_ms and pd_last_launch_info report it like any other launch."""
    dm, inp, t, ws, ref, _ = _bundle(dev, "laikago", 5, 1, False)
    bs = 5
    bufs = dict(grads=dm._alloc_grads(bs, T12, dev, want=()))
    run = lambda: dm.rollout_backward(bs, T12, inp["dt"], *[t[k] for k in BWD], F2S, ws, t["adj_pos"], t["adj_vel"], out=bufs, want=())
    info_all = dm.last_launch_info(1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            g = run()
    torch.cuda.current_stream().wait_stream(side)
    for trial in range(2):
        for v in g.values():
            v.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        _assert_same(g, ref, ("graph replay", trial))
    dm.set_timing(True)
    try:
        run()
        torch.cuda.synchronize()
        assert dm.last_kernel_ms(1) > 0.0
        assert dm.last_launch_info(1) == info_all
    finally:
        dm.set_timing(False)
