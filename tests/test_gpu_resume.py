"""Resumed rollouts (pd_rollout_forward / pd_rollout_backward with qd_init_dev == NULL: state 0 is a body state), chaining of their
adjoints, ForwardWarpState, and the checkpointed adjoint of ForwardWarp (``self.checkpoint_steps``).

A rollout of T steps run as consecutive resumed rollouts gives the single launch's BITS: outputs, saved trajectory, per-step gradients and
the q_init / qd_init gradients.  The five gradients that are sums over the steps re-associate an fp32 sum when they are added up per
segment; they are held to the float64 adjoint of the kernel's own trajectory, with the bars the single launch is held to."""
import ctypes
import gc

import numpy as np
import pytest
import torch

from gpu_harness import FWD, SEEDED, dev, dev_inputs, device_model, same_bits, warp_grads, warp_host  # noqa: F401
from helpers import INPUT_NAMES

pytestmark = pytest.mark.gpu

PARAMS = ("target_ke", "target_kd", "body_inv_mass", "body_inertia", "body_inv_inertia")
SUMMED = PARAMS
STEPWISE = ("torques", "refs", "res_f")
# (robot, envs, kernel family)
CASES = [("laikago", 256, 1), ("laikago", 64, 2), ("human", 128, 0), ("quad", 128, 0)]
T60 = 60


def _setup(robot, bs, family, dev, T=T60, seed=0, literal=False, segw=None):
    from diffphys_amd import robots, synth

    tpl = robots.load_template(robot)
    inp = synth.make_inputs(tpl, robot, bs=bs, nsteps=T, seed=seed, steps_per_frame=20, penetration=0.003)
    return device_model(tpl, family, segw, literal), inp, dev_inputs(inp, dev)


def _resumed_forward_case(dev, robot, bs, family, splits, **kw):
    dm, inp, t = _setup(robot, bs, family, dev, **kw)
    T, dt = T60, inp["dt"]
    par = [t[k] for k in PARAMS]
    for s in splits:
        f2s = sorted(set([0, 20, 40, 60, s]))
        pos, vel, grf, jaf, ws = dm.rollout_forward(bs, T, dt, *[t[k] for k in FWD], frame2step=f2s)
        assert float(grf.abs().max()) > 0.0, "contacts must be active"
        traj = [x.clone() for x in dm.saved_trajectory(ws, bs, T)]
        fs = f2s.index(s)
        state = torch.cat([pos[fs], vel[fs]], dim=1).contiguous()
        f2s_r = [x - s for x in f2s if x >= s]
        ctl = [t[k][s:].contiguous() for k in ("torques", "res_f", "refs")]
        outs = []
        for save, st0 in ((True, state), (False, (pos[fs], vel[fs]))):   # the pair form is concatenated by the binding
            p2, v2, g2, j2, ws2 = dm.rollout_forward(bs, T - s, dt, None, None, *ctl, *par, frame2step=f2s_r, save_trajectory=save, state0=st0)
            assert (ws2 is None) == (not save)
            outs.append((p2, v2, g2, j2))
            if save:
                traj2 = dm.saved_trajectory(ws2, bs, T - s)
        torch.cuda.synchronize()
        for (p2, v2, g2, j2) in outs:
            assert float(g2.abs().max()) > 0.0, "contacts must be active"
            assert torch.equal(p2[0], pos[fs]) and torch.equal(v2[0], vel[fs]), "a frame at step 0 returns the state bit for bit"
            for name, a, b in (("wp_pos", p2, pos[fs:]), ("wp_vel", v2, vel[fs:]), ("grf", g2, grf[fs:]), ("jaf", j2, jaf[fs:])):
                assert same_bits(a, b, nan_equal=True), (robot, family, s, name)
        for k in range(4):
            assert same_bits(outs[0][k], outs[1][k], nan_equal=True), "the resumed forward-only launch equals the resumed saving launch"
        for name, a, b in zip(("body_q", "body_qd", "body_f", "clamp mask"), traj, traj2):
            assert same_bits(a[s:], b, nan_equal=True), (robot, family, s, "saved " + name)
        print("%s bs=%d family %d split %d: resumed forward continues bit for bit (frames, wrenches, saved trajectory)" % (robot, bs, family, s))


@pytest.mark.parametrize("robot,bs,family", CASES)
def test_resumed_forward_continues_bit_for_bit(dev, robot, bs, family):
    """Single launch with frames at {0, 20, 40, 60, s}; then a resumed launch from frame s's rows over the remaining steps with the
    controls sliced [s:]: every common frame's pose, twist, ground and joint wrench, and the saved states / wrenches / clamp masks of
    steps >= s are the same bits; s is no multiple of the 4-step cull epoch, so the speculation phase shifts (the hit log, which depends
    on it, is not compared: the forward bits do not)."""
    _resumed_forward_case(dev, robot, bs, family, (1, 23, 40))


def test_resumed_forward_literal_policy_and_segment_width_64(dev):
    _resumed_forward_case(dev, "laikago", 256, 1, (23,), literal=True)
    _resumed_forward_case(dev, "laikago", 256, 1, (23,), segw=64)


def _seeds(dm, bs, F, dev, seed=5, scale=1e-3):
    rng = np.random.RandomState(seed)
    N = bs * dm.nb
    return (torch.from_numpy((rng.randn(F, N, 7) * scale).astype(np.float32)).to(dev),
            torch.from_numpy((rng.randn(F, N, 6) * scale).astype(np.float32)).to(dev))


def _single_adjoint(dm, bs, T, dt, t, f2s, ap, av):
    pos, vel, grf, jaf, ws = dm.rollout_forward(bs, T, dt, *[t[k] for k in FWD], frame2step=f2s)
    assert float(grf.abs().max()) > 0.0, "contacts must be active"
    g = dm.rollout_backward(bs, T, dt, t["q_init"], t["qd_init"], t["torques"], t["refs"], *[t[k] for k in PARAMS], f2s, ws, ap, av)
    return pos, vel, g


@pytest.mark.parametrize("robot,bs,family", CASES)
def test_chained_adjoint_equals_the_single_adjoint(dev, robot, bs, family):
    """Split at s = 23, random seeds on frames {0, 20, 40, 60}: the later segment's adjoint first, its raw grads["state0"] as the seed of
    frame s of the earlier segment, then the earlier segment.  torques / refs / res_f gradients of all 60 steps and the q_init / qd_init
    gradients: torch.equal to the single launch."""
    dm, inp, t = _setup(robot, bs, family, dev)
    T, dt, s = T60, inp["dt"], 23
    f2s = [0, 20, 40, 60]
    ap, av = _seeds(dm, bs, len(f2s), dev)
    par = [t[k] for k in PARAMS]
    _, _, g1 = _single_adjoint(dm, bs, T, dt, t, f2s, ap, av)
    g1 = {k: v.clone() for k, v in g1.items()}
    # earlier segment: steps [0, s), frames 0, 20 and the boundary state s
    fa = [0, 20, s]
    ctl_a = [t[k][:s].contiguous() for k in ("torques", "res_f", "refs")]
    pa, va, ga_, ja, ws_a = dm.rollout_forward(bs, s, dt, t["q_init"], t["qd_init"], *ctl_a, *par, frame2step=fa)
    ws_a = ws_a.clone()
    # later segment: resumed from that state, frames 40 and 60
    fb = [40 - s, 60 - s]
    ctl_b = [t[k][s:].contiguous() for k in ("torques", "res_f", "refs")]
    st = (pa[2], va[2])
    pb, vb, gb_, jb, ws_b = dm.rollout_forward(bs, T - s, dt, None, None, *ctl_b, *par, frame2step=fb, state0=st)
    assert float(gb_.abs().max()) > 0.0 and float(ga_.abs().max()) > 0.0, "contacts must be active"
    gb = dm.rollout_backward(bs, T - s, dt, None, None, ctl_b[0], ctl_b[2], *par, fb, ws_b, ap[2:].contiguous(), av[2:].contiguous(), state0=st)
    assert "q_init" not in gb and gb["state0"].shape == (bs * dm.nb, 13)
    carry = gb["state0"]
    ap_a = torch.cat([ap[:2], carry[None, :, :7]]).contiguous()
    av_a = torch.cat([av[:2], carry[None, :, 7:]]).contiguous()
    ga = dm.rollout_backward(bs, s, dt, t["q_init"], t["qd_init"], ctl_a[0], ctl_a[2], *par, fa, ws_a, ap_a, av_a)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for v in g1.values())
    for k in STEPWISE:
        assert float(g1[k].abs().max()) > 0.0
        assert torch.equal(torch.cat([ga[k], gb[k]]), g1[k]), (robot, family, k)
    for k in ("q_init", "qd_init"):
        assert torch.equal(ga[k], g1[k]), (robot, family, k)
    print("%s bs=%d family %d: chained adjoint (split 23) equals the single adjoint bit for bit" % (robot, bs, family))


def _warp_grads(robot, bs, T, f2s, dt, t_in, ap, av, dev, K, attr=True):
    """ForwardWarp.apply + backward of sum(pos * ap) + sum(vel * av) -> (pos, vel, grfs, grads by input name).  attr=False: the host has no
    ``checkpoint_steps`` attribute at all"""
    from diffphys_amd import dp_model

    h = warp_host(robot, bs, T, f2s, dt, dev, K) if attr else warp_host(robot, bs, T, f2s, dt, dev)
    pos, vel, g = warp_grads(dp_model.ForwardWarp, INPUT_NAMES, t_in, h, ap, av)
    return pos, vel, [x.detach() for x in h.grfs], g


def _dist(w):
    q = lambda p: float(np.percentile(w, p))
    return "median %.1e p99 %.1e p99.5 %.1e max %.1e" % (float(np.median(w)), q(99), q(99.5), float(w.max()))


@pytest.mark.parametrize("cfg,Ks", [("C3", (7, 30)), ("C5", (7, 30)), ("C4:16", (5,))])
def test_summed_gradients_vs_float64_adjoint_of_own_trajectory(dev, oracle_libs, cfg, Ks):
    """The five gradients that are sums over the steps, added up per segment (last segment first, fp32), against the float64 adjoint of the
    kernel's own trajectory (helpers.own_trajectory_check: g64; the recomputed segments reproduce that trajectory bit for bit) -- per env,
    all ten gradient tensors, with the bars test_gradients_vs_float64_adjoint_of_own_trajectory applies to the single launch:
    human 1024 x 100 and quad 8192 x 34 (the horizons _own_traj_inputs gives them) every env < 1e-4 and the 99th percentile < 2e-5;
    Laikago, kicked, 16 steps: max < 2e-3, 99.5th percentile < 5e-4, median < 2e-5."""
    from helpers import GRAD_LEAD, grad_env_errors, own_trajectory_check
    from test_gpu_tight import _own_traj_inputs
    from diffphys_amd import hip_backend

    name, tpl, inp = _own_traj_inputs(cfg)
    dm = hip_backend.DeviceModel(tpl)
    r = own_trajectory_check(dm, tpl, inp, dev, hitlog_check=False)
    bs, T = len(r["worst"]), inp["nsteps"]
    assert (r["touch_counts"] > 0).any(), "contacts must be active"
    t = dev_inputs(inp, dev, SEEDED)
    worst = lambda e, keys: np.max(np.stack([e[k] for k in keys]), axis=0)
    w1, w1s = r["worst"], worst(r["errs"], SUMMED)
    print("%s %s %d envs x %d steps, single launch : all tensors %s | the five sums %s" % (cfg, name, bs, T, _dist(w1), _dist(w1s)))
    for K in Ks:
        assert K < T
        pos, vel, grfs, g = _warp_grads(name, bs, T, list(inp["frame2step"]), inp["dt"], t, t["adj_pos"], t["adj_vel"], dev, K)
        assert max(float(x.abs().max()) for x in grfs) > 0.0, "contacts must be active"
        gn = {k: g[k].cpu().numpy() for k in GRAD_LEAD}
        for k in STEPWISE + ("q_init", "qd_init"):
            assert np.array_equal(gn[k].reshape(-1), r["grads"][k].reshape(-1)), k
        e = grad_env_errors(gn, r["g64"], bs)
        w, ws_ = worst(e, GRAD_LEAD), worst(e, SUMMED)
        print("%s %s %d envs x %d steps, segments of %3d: all tensors %s | the five sums %s" % (cfg, name, bs, T, K, _dist(w), _dist(ws_)))
        assert all(np.isfinite(v).all() for v in gn.values())
        q = lambda a, p: float(np.percentile(a, p))
        if name != "laikago":
            assert w.max() < 1e-4 and q(w, 99) < 2e-5, (K, float(w.max()), q(w, 99))
        else:
            assert w.max() < 2e-3 and q(w, 99.5) < 5e-4 and np.median(w) < 2e-5, (K, float(w.max()), q(w, 99.5), float(np.median(w)))


class _Spy:
    """records (nsteps, save_trajectory, resumed) of every DeviceModel.rollout_forward while active"""

    def __enter__(self):
        from diffphys_amd import hip_backend

        self.calls, self.orig = [], hip_backend.DeviceModel.rollout_forward
        orig, calls = self.orig, self.calls

        def spy(dm, bs, nsteps, *a, **kw):
            calls.append((int(nsteps), kw.get("save_trajectory", True), kw.get("state0") is not None))
            return orig(dm, bs, nsteps, *a, **kw)

        hip_backend.DeviceModel.rollout_forward = spy
        return self

    def __exit__(self, *exc):
        from diffphys_amd import hip_backend

        hip_backend.DeviceModel.rollout_forward = self.orig


def _long_inputs(bs, T0, R, dev, seed=21):
    """Laikago inputs whose controls are a T0-step synth block repeated R times"""
    from diffphys_amd import robots, synth

    tpl = robots.load_template("laikago")
    inp = synth.make_inputs(tpl, "laikago", bs=bs, nsteps=T0, seed=seed, seqs=("mi-trot", "mi-spin"), penetration=0.003)
    t = dev_inputs(inp, dev)
    for k in ("torques", "res_f", "refs"):
        t[k] = t[k].repeat((R,) + (1,) * (t[k].dim() - 1)).contiguous()
    return tpl, inp, t


def test_forward_warp_checkpointed_end_to_end_and_memory(dev):
    """Laikago 4096 envs x 2000 steps, frames every 200 steps and at T, all eleven inputs requiring gradients: checkpoint_steps = 70 (the
    last segment shorter, 70 no multiple of 4) against the single launch (9.6 GB of workspace).  Outputs, grfs, per-step gradients and
    q_init / qd_init gradients the same bits; the five sums finite, their relmax printed (their bar is the float64 test above); peak
    memory of forward + backward within gradients + outputs + one 70-step workspace + boundary states + seeds + 256 MB."""
    from helpers import relmax
    from diffphys_amd import hip_backend

    free, _ = torch.cuda.mem_get_info()
    if free < 40e9:
        print("SKIP reason: %.1f GB of device memory free, the single-launch comparison needs ~40 GB" % (free / 1e9))
        pytest.skip("needs 40 GB of free device memory (%.1f GB free)" % (free / 1e9))
    bs, T0, R, K = 4096, 100, 20, 70
    T = T0 * R
    tpl, inp, t = _long_inputs(bs, T0, R, dev)
    f2s = list(range(0, T + 1, 200))
    dm = hip_backend.DeviceModel(tpl)
    F, N = len(f2s), bs * dm.nb
    ap, av = _seeds(dm, bs, F, dev, seed=8)
    from diffphys_amd import dp_model

    x = {k: t[k].requires_grad_(True) for k in INPUT_NAMES}   # the inputs themselves carry the gradients: no copies inside the measurement
    h = warp_host("laikago", bs, T, f2s, inp["dt"], dev, K)
    gc.collect()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with _Spy() as spy:
        pos, vel = dp_model.ForwardWarp.apply(*[x[k] for k in INPUT_NAMES], h)
        ((pos * ap).sum() + (vel * av).sum()).backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    pos, vel, grfs, g = pos.detach(), vel.detach(), [v.detach() for v in h.grfs], {k: x[k].grad for k in INPUT_NAMES}
    for v in x.values():
        v.grad = None
        v.requires_grad_(False)
    assert spy.calls[0] == (T, False, False), spy.calls[0]
    assert len(spy.calls) == 1 + -(-T // K) and all(n <= K and save for n, save, _ in spy.calls[1:]), spy.calls
    assert [c[2] for c in spy.calls[1:]] == [True] * (len(spy.calls) - 2) + [False]   # segment 0, the last one run, starts from q_init
    grads = sum(t[k].numel() for k in INPUT_NAMES) * 4          # the inputs' gradients
    outputs = F * N * (7 + 6 + 6 + 6) * 4
    workspace = dm.workspace_floats(bs, K) * 4
    boundaries = (-(-T // K) - 1) * N * 13 * 4
    seeds = F * N * 13 * 4                                      # the upstream gradients of wp_pos / wp_vel that autograd hands to backward
    bound = grads + outputs + workspace + boundaries + seeds + (256 << 20)
    print("checkpointed ForwardWarp 4096 x 2000, K = 70: peak +%.2f GB; bound %.2f GB (gradients %.2f, outputs %.3f, 70-step "
          "workspace %.3f, boundary states %.3f, seeds %.3f); the single launch's workspace alone %.2f GB" % (
              peak / 1e9, bound / 1e9, grads / 1e9, outputs / 1e9, workspace / 1e9, boundaries / 1e9, seeds / 1e9, dm.workspace_floats(bs, T) * 4 / 1e9))
    assert peak <= bound, (peak, bound)
    assert max(float(x.abs().max()) for x in grfs) > 0.0, "contacts must be active"
    with _Spy() as spy1:
        pos1, vel1, grfs1, g1 = _warp_grads("laikago", bs, T, f2s, inp["dt"], t, ap, av, dev, None, attr=False)
    assert spy1.calls == [(T, True, False)], spy1.calls
    assert torch.equal(pos, pos1) and torch.equal(vel, vel1)
    assert len(grfs) == len(grfs1) and all(torch.equal(a, b) for a, b in zip(grfs, grfs1))
    for k in STEPWISE + ("q_init", "qd_init"):
        assert float(g1[k].abs().max()) > 0.0
        assert torch.equal(g[k], g1[k]), k
    for k in SUMMED:
        assert bool(torch.isfinite(g[k]).all()), k
        print("  %-17s relmax against the single launch %.2e" % (k, relmax(g[k].cpu().numpy(), g1[k].cpu().numpy())))
    assert float(g["body_mass"].abs().max()) == 0.0


def test_forward_warp_state_chains_through_autograd(dev):
    """Two windows of 30 steps as two ForwardWarpState / ForwardWarp calls chained through wp_pos[-1] / wp_vel[-1], one loss.backward():
    q_init / qd_init gradients and the control gradients of both windows equal those of one 60-step ForwardWarp call with the same frame
    seeds.  Under no_grad the call allocates no workspace."""
    from diffphys_amd import dp_model, hip_backend

    robot, bs, T, W = "laikago", 256, 60, 30
    dm, inp, t = _setup(robot, bs, 0, dev)
    dt = inp["dt"]
    f2s = [0, 20, 30, 40, 60]
    ap, av = _seeds(dm, bs, len(f2s), dev, seed=6)
    pos1, vel1, grfs1, g1 = _warp_grads(robot, bs, T, f2s, dt, t, ap, av, dev, None)
    # window 1: ForwardWarp over steps [0, 30), frames 0, 20, 30; window 2: ForwardWarpState over [30, 60), frames 40, 60 (local 10, 30)
    x = {k: t[k].detach().clone().requires_grad_(True) for k in ("q_init", "qd_init") + PARAMS + ("body_mass",)}
    c1 = {k: t[k][:W].detach().clone().requires_grad_(True) for k in ("torques", "res_f", "refs")}
    c2 = {k: t[k][W:].detach().clone().requires_grad_(True) for k in ("torques", "res_f", "refs")}
    h1 = warp_host(robot, bs, W, [0, 20, 30], dt, dev, None)
    h2 = warp_host(robot, bs, W, [10, 30], dt, dev, None)
    tail = [x[k] for k in ("target_ke", "target_kd", "body_mass", "body_inv_mass", "body_inertia", "body_inv_inertia")]
    pa, va = dp_model.ForwardWarp.apply(x["q_init"], x["qd_init"], c1["torques"], c1["res_f"], c1["refs"], *tail, h1)
    pb, vb = dp_model.ForwardWarpState.apply(pa[-1], va[-1], c2["torques"], c2["res_f"], c2["refs"], *tail, h2)
    assert max(float(g.abs().max()) for g in h1.grfs + h2.grfs) > 0.0, "contacts must be active"
    assert torch.equal(pa.detach(), pos1[:3]) and torch.equal(pb.detach(), pos1[3:]) and torch.equal(vb.detach(), vel1[3:])
    loss = (pa * ap[:3]).sum() + (va * av[:3]).sum() + (pb * ap[3:]).sum() + (vb * av[3:]).sum()
    loss.backward()
    torch.cuda.synchronize()
    for k in ("q_init", "qd_init"):
        assert float(g1[k].abs().max()) > 0.0 and torch.equal(x[k].grad, g1[k]), k
    for k in STEPWISE:
        assert torch.equal(torch.cat([c1[k].grad, c2[k].grad]), g1[k]), k
    for k in SUMMED:   # autograd adds the two windows' sums: a re-associated fp32 sum (held to float64 in the test above), finite here
        assert bool(torch.isfinite(x[k].grad).all()), k
    # no_grad: forward-only, no workspace -- the peak stays below one 30-step workspace
    st = (pa[-1].detach().clone(), va[-1].detach().clone())
    gc.collect()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    with _Spy() as spy, torch.no_grad():
        pn, vn = dp_model.ForwardWarpState.apply(*st, *[c2[k].detach() for k in ("torques", "res_f", "refs")], *[v.detach() for v in tail], h2)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    assert spy.calls == [(W, False, True)], spy.calls
    assert peak < dm.workspace_floats(bs, W) * 4, (peak, dm.workspace_floats(bs, W) * 4)
    assert torch.equal(pn, pb.detach()) and torch.equal(vn, vb.detach())


def test_resumed_refusals_and_zero_steps(dev):
    """qd_init_dev == NULL with a g_qd_init_dev is refused by name, before any launch; the trajectory-loss entries refuse the resumed mode;
    nsteps == 0 resumed: frame 0 is the input state and g_state0 the seeds."""
    from diffphys_amd import hip_backend

    dm, inp, t = _setup("laikago", 8, 0, dev, T=10)
    bs, T, dt, nb = 8, 10, inp["dt"], dm.nb
    N = bs * nb
    lib = hip_backend.lib()
    rng = np.random.RandomState(3)
    state = torch.from_numpy(rng.randn(N, 13).astype(np.float32)).to(dev)   # un-normalised quaternions: taken as they are
    par = [t[k] for k in PARAMS]
    ctl = [t[k] for k in ("torques", "res_f", "refs")]
    f2s = [0, 10]
    pos, vel, grf, jaf, ws = dm.rollout_forward(bs, T, dt, None, None, *ctl, *par, frame2step=f2s, state0=state)
    ap, av = _seeds(dm, bs, 2, dev)
    g = dm._alloc_grads(bs, T, dev, resumed=True)
    SENT = -7.5
    for v in g.values():
        v.fill_(SENT)
    extra = torch.full((bs * dm.nqd,), SENT, dtype=torch.float32, device=dev)
    f2s_c = (ctypes.c_int * 2)(*f2s)
    gp = [g[k].data_ptr() for k in ("torques", "res_f", "refs", "target_ke", "target_kd", "body_inv_mass", "body_inertia", "body_inv_inertia")]
    rc = lib.pd_rollout_backward(dm.h, bs, T, ctypes.c_float(dt), state.data_ptr(), None, t["torques"].data_ptr(), t["refs"].data_ptr(),
                                 *[x.data_ptr() for x in par], 2, f2s_c, ws.data_ptr(), ap.data_ptr(), av.data_ptr(),
                                 g["state0"].data_ptr(), extra.data_ptr(), *gp, hip_backend._stream())
    assert rc != 0 and "g_qd_init" in lib.pd_last_error().decode(), lib.pd_last_error().decode()
    torch.cuda.synchronize()
    assert all(bool((v == SENT).all()) for v in g.values()) and bool((extra == SENT).all()), "a refusal writes nothing"
    # the trajectory-loss forward entry says that the resumed mode is not its own
    F = 2
    e = lambda *s: torch.zeros(*s, dtype=torch.float32, device=dev)
    tgt, table, red, scale = e(bs, F, nb, 7), e(bs, F), e(4), e(bs, F)
    rc = lib.pd_rollout_forward_traj_loss(dm.h, bs, T, ctypes.c_float(dt), state.data_ptr(), None, *[x.data_ptr() for x in ctl],
                                          *[x.data_ptr() for x in par], F, f2s_c, None, pos.data_ptr(), vel.data_ptr(), grf.data_ptr(),
                                          jaf.data_ptr(), tgt.data_ptr(), None, ctypes.c_float(0.1), None, None, table.data_ptr(),
                                          red.data_ptr(), scale.data_ptr(), hip_backend._stream())
    assert rc != 0 and "qd_init" in lib.pd_last_error().decode()
    with pytest.raises(ValueError):
        dm.rollout_forward(bs, T, dt, t["q_init"], t["qd_init"], *ctl, *par, frame2step=f2s, state0=state)
    # no steps: the state in is the frame out, the seeds in are the state gradient out (raw)
    for family in (0, 2):
        dm.set_kernel_family(family)
        none = [x[:0] for x in ctl]
        p0, v0, _, _, ws0 = dm.rollout_forward(bs, 0, dt, None, None, *none, *par, frame2step=[0], state0=state)
        assert torch.equal(torch.cat([p0[0], v0[0]], dim=1), state)
        sp, sv = _seeds(dm, bs, 1, dev, seed=9, scale=1.0)
        sp[0, 3, 2] = float("nan")   # raw: not scrubbed
        g0 = dm.rollout_backward(bs, 0, dt, None, None, none[0], none[2], *par, [0], ws0, sp, sv, state0=state)
        want = torch.cat([sp[0], sv[0]], dim=1)
        assert same_bits(g0["state0"], want, nan_equal=True) and bool(torch.isnan(g0["state0"][3, 2]))


def test_checkpointed_nan_policy_and_todays_path(dev):
    """NaNs planted in one env's frame-T seed (all of its rows), with checkpoint_steps: every returned gradient is finite, that env's per-step gradients
    are all zero (as in the single launch), the other envs are bit-identical to the run without the NaN.  checkpoint_steps >= nsteps,
    None and absent take today's path: one saving launch of nsteps steps."""
    robot, bs, T, K = "laikago", 64, 60, 17
    dm, inp, t = _setup(robot, bs, 0, dev)
    f2s, dt, nb = [0, 20, 40, 60], inp["dt"], dm.nb
    ap, av = _seeds(dm, bs, len(f2s), dev, seed=11)
    pos, vel, grfs, g = _warp_grads(robot, bs, T, f2s, dt, t, ap, av, dev, K)
    assert max(float(x.abs().max()) for x in grfs) > 0.0, "contacts must be active"
    bad = 5
    ap_n, av_n = ap.clone(), av.clone()   # the env's whole frame-T seed: pose and twist rows of all its bodies (a NaN in one component
    ap_n[-1, bad * nb: (bad + 1) * nb] = float("nan")   # reaches the other bodies' adjoints only over the following steps)
    av_n[-1, bad * nb: (bad + 1) * nb] = float("nan")
    _, _, _, gn = _warp_grads(robot, bs, T, f2s, dt, t, ap_n, av_n, dev, K)
    _, _, _, g1n = _warp_grads(robot, bs, T, f2s, dt, t, ap_n, av_n, dev, None)
    lead = dict(torques=1, res_f=1, refs=1)
    for k in INPUT_NAMES:
        assert bool(torch.isfinite(gn[k]).all()), k
        if k == "body_mass":
            continue
        env = (lambda x: x.reshape(T, bs, -1)) if k in lead else (lambda x: x.reshape(1, bs, -1))
        a, b, c = env(gn[k]), env(g[k]), env(g1n[k])
        keep = torch.arange(bs, device=dev) != bad
        assert torch.equal(a[:, keep], b[:, keep]), k          # the other envs: the bits of the run without the NaN
        if k in lead:
            assert float(a[:, bad].abs().max()) == 0.0, k     # the NaN env: zero per-step gradients ...
            assert float(c[:, bad].abs().max()) == 0.0, k     # ... as in the single launch
        if k in lead or k in ("q_init", "qd_init"):
            assert torch.equal(a, c), k                        # and the single launch's bits in every env
    for K2, attr in ((T, True), (T + 5, True), (None, True), (0, True), (None, False)):
        with _Spy() as spy:
            p2, v2, _, g2 = _warp_grads(robot, bs, T, f2s, dt, t, ap, av, dev, K2, attr=attr)
        assert spy.calls == [(T, True, False)], (K2, attr, spy.calls)
        assert torch.equal(p2, pos) and all(torch.equal(g2[k], g[k]) for k in STEPWISE + ("q_init", "qd_init"))


def test_a_horizon_the_single_adjoint_cannot_hold(dev):
    """Laikago 4096 envs x 20 000 steps: 95.7 GB of single-launch workspace on top of ~75 GB of controls and their gradients.  With
    checkpoint_steps = 150 the adjoint runs; gradients finite, contacts active; a second run with checkpoint_steps = 333 gives the same
    bits in every per-step gradient and in the q_init / qd_init gradients."""
    from diffphys_amd import hip_backend

    free, _ = torch.cuda.mem_get_info()
    if free < 120e9:
        print("SKIP reason: %.1f GB of device memory free, controls, gradients and their comparison copies need ~120 GB" % (free / 1e9))
        pytest.skip("needs 120 GB of free device memory (%.1f GB free)" % (free / 1e9))
    bs, T0, R = 4096, 100, 200
    T = T0 * R
    tpl, inp, t = _long_inputs(bs, T0, R, dev, seed=23)
    dm = hip_backend.DeviceModel(tpl)
    assert dm.workspace_floats(bs, T) * 4 > 95e9
    f2s = list(range(0, T + 1, 2000))
    ap, av = _seeds(dm, bs, len(f2s), dev, seed=12)
    keep = {}
    for K in (150, 333):
        from diffphys_amd import dp_model

        h = warp_host("laikago", bs, T, f2s, inp["dt"], dev, K)
        x = {k: t[k].requires_grad_(True) for k in INPUT_NAMES}   # (no clones: the controls are 25 GB)
        for v in x.values():
            v.grad = None
        with _Spy() as spy:
            pos, vel = dp_model.ForwardWarp.apply(*[x[k] for k in INPUT_NAMES], h)
            ((pos * ap).sum() + (vel * av).sum()).backward()
        torch.cuda.synchronize()
        assert spy.calls[0] == (T, False, False) and all(n <= K and s for n, s, _ in spy.calls[1:])
        assert max(float(g.abs().max()) for g in h.grfs) > 0.0, "contacts must be active"
        for k in INPUT_NAMES:
            assert bool(torch.isfinite(x[k].grad).all()), (K, k)
        assert float(x["res_f"].grad[:4000].abs().max()) > 0.0
        if not keep:
            keep = {k: x[k].grad for k in STEPWISE + ("q_init", "qd_init")}
        else:
            for k, v in keep.items():
                assert torch.equal(x[k].grad, v), k
        del pos, vel, h
        gc.collect()
